"""Measurement probe of multi-value columns (pinot_amd/csrc/mv.hip; DESIGN.md §3 "Multi-value columns"): synthetic
segments of SSB size -- 6 000 000 docs, 4 values per doc on average in a 10-bit multi-value column -- as many as asked.

  * the MV scan leaf: COUNT(*) under a range and under an IN predicate on the column. The scan launch sits before the
    filter launch's timing markers, so its time is device_ms - scan_kernel_ms (the whole execution minus the filter and
    aggregation kernels), less the same difference of a plan without a pre-pass (a predicate on a single-value column):
    what is left is the mv_scan_kernel launch. Bytes streamed = total_values x bits / 8 + 4 (num_docs + 1), reported
    against the 6.1 TB/s copy ceiling DESIGN.md records;
  * one materialisation per reduction kind: plan creation with the row-reduction column built minus plan creation with it
    cached (fresh segments per kind would cost a load each: the 16 other columns of evict() push it out instead);
  * the new kernels' resource usage -- VGPRs, SGPRs, LDS, scratch, spills, occupancy -- from the compiler's own
    remarks: the probe compiles pinot_amd/csrc/mv.hip with -Rpass-analysis=kernel-resource-usage (the library's flags)
    and prints one line per kernel; "resources": null where no hipcc is installed.

Warmed medians of STEPS executions, REPS fresh plans each.

  python tools/mv_probe.py [segments = 1] [docs per segment = 6000000]
"""
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
os.environ["PHIP_TOTAL_EVENTS"] = "1"
from pinot_amd import _lib  # noqa: E402
from pinot_amd.engine.plan import GpuInstancePlanMaker  # noqa: E402
from pinot_amd.engine.segment import GpuSegment  # noqa: E402
from pinot_amd.query.sql import parse  # noqa: E402
from pinot_amd.segment.creator import (ColumnIndexes, ColumnMetadata, ImmutableSegment, mv_docs_per_chunk,  # noqa: E402
                                       pack_bits)
from pinot_amd.spi import DataType  # noqa: E402

NSEG = int(sys.argv[1]) if len(sys.argv) > 1 else 1
DOCS = int(sys.argv[2]) if len(sys.argv) > 2 else 6_000_000
WARM, STEPS, REPS = 5, 30, 3
COPY_CEILING = 6.1e12
CARD = 1000  # 10 bits


def make_segment(k):
    """Built from arrays (SegmentCreator's per-row path is for test sizes): lengths 1..7, mean 4."""
    rng = np.random.default_rng(k)
    lengths = rng.integers(1, 8, DOCS)
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    total = int(lengths.sum())
    ids = rng.integers(0, CARD, total).astype(np.int32)
    ids[:CARD] = np.arange(CARD)  # every id occurs
    per_chunk = mv_docs_per_chunk(DOCS, total)
    bitset = np.zeros((total + 7) // 8, dtype=np.uint8)
    np.bitwise_or.at(bitset, starts >> 3, (0x80 >> (starts & 7)).astype(np.uint8))
    fwd = starts[::per_chunk].astype(">i4").tobytes() + bitset.tobytes() + pack_bits(ids, 10)
    seg = ImmutableSegment(f"mvprobe{k}", DOCS)
    seg.columns["m"] = ColumnIndexes(
        ColumnMetadata("m", DataType.INT, DOCS, CARD, 10, False, True, False, is_single_value=False,
                       max_number_of_multi_values=7, total_number_of_entries=total),
        fwd, np.arange(CARD, dtype=">i4").tobytes())
    a = rng.integers(0, 64, DOCS).astype(np.int32)
    seg.columns["a"] = ColumnIndexes(ColumnMetadata("a", DataType.INT, DOCS, 64, 6, False, True, False),
                                     pack_bits(a, 6), np.arange(64, dtype=">i4").tobytes())
    return seg, total


def kernel_resources():
    """Per kernel of mv.hip what hipcc's kernel-resource-usage remarks say, compiled with the library's flags."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join("pinot_amd", "csrc", "mv.hip")
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
                            "-fvisibility=hidden", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                            os.path.join(d, "mv.o"), src], capture_output=True, text=True)
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "SGPRs Spill": "sgpr_spills",
            "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"\d+(mv_\w+?_kernel)", m.group(2))
            cur = out.setdefault(name.group(1) if name else m.group(2), {})
        elif cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out or None


def prepare(sql, segs):
    t0 = time.perf_counter()
    op = GpuInstancePlanMaker().make_instance_plan(parse(sql), segs)
    op.run_raw(prepare_only=True)
    return op, 1e3 * (time.perf_counter() - t0)


def measure(sql, segs, lib):
    pre, dev, flt = [], [], []
    matched = None
    for _ in range(REPS):
        op, _ = prepare(sql, segs)
        p, d, f = [], [], []
        for i in range(WARM + STEPS):
            r = op.run_raw()
            c = r.contents
            if i >= WARM:
                p.append(c.device_ms - c.scan_kernel_ms)
                d.append(c.device_ms)
                f.append(c.filter_kernel_ms)
            matched = c.num_docs_scanned
            lib.phip_result_free(r)
        op.close()
        pre.append(statistics.median(p))
        dev.append(statistics.median(d))
        flt.append(statistics.median(f))
    return {"matched": matched, "before_filter_ms": round(statistics.median(pre), 4),
            "before_filter_ms_spread": [round(min(pre), 4), round(max(pre), 4)],
            "device_ms": round(statistics.median(dev), 4), "filter_ms": round(statistics.median(flt), 4)}


def evict(segs):
    for k in range(16):
        op, _ = prepare(f"select sum(a * {k + 2} + {k}) from t", segs)
        op.close()


def main():
    print(json.dumps({"resources": kernel_resources()}), flush=True)
    lib = _lib.load()
    _lib.check(lib.phip_init((ctypes.c_int32 * 1)(0), 1))
    built = [make_segment(k) for k in range(NSEG)]
    segs = [GpuSegment(s) for s, _ in built]
    total = sum(t for _, t in built)
    scan_bytes = total * 10 / 8.0 + 4.0 * (NSEG * (DOCS + 1))
    print(json.dumps({"segments": NSEG, "docs": NSEG * DOCS, "values": total, "scan_bytes": int(scan_bytes)}))
    base = measure("select count(*) from t where a between 3 and 20", segs, lib)
    print(json.dumps({"query": "single-value baseline", **base}), flush=True)
    for name, where in (("range", "m between 100 and 299"), ("in", "m in (3, 77, 150, 420, 421, 800, 999)"),
                        ("not in", "m not in (3, 77, 150, 420, 421, 800, 999)")):
        row = measure(f"select count(*) from t where {where}", segs, lib)
        scan_ms = row["before_filter_ms"] - base["before_filter_ms"]
        row["mv_scan_ms"] = round(scan_ms, 4)
        if scan_ms > 0:
            row["bytes_per_s"] = round(scan_bytes / (scan_ms * 1e-3) / 1e12, 3)
            row["fraction_of_copy_ceiling"] = round(scan_bytes / (scan_ms * 1e-3) / COPY_CEILING, 4)
        print(json.dumps({"query": name, **row}), flush=True)
    for fn in ("countmv", "summv", "minmv", "maxmv"):
        cold, cached = [], []
        for _ in range(REPS):
            evict(segs)
            op, c0 = prepare(f"select {fn}(m) from t where a < 20", segs)
            op2, c1 = prepare(f"select {fn}(m) from t where a < 20", segs)
            op.close()
            op2.close()
            cold.append(c0)
            cached.append(c1)
        per_seg = (statistics.median(cold) - statistics.median(cached)) / NSEG
        bytes_per_seg = scan_bytes / NSEG + 8.0 * DOCS
        print(json.dumps({"materialise": fn, "ms_per_segment": round(per_seg, 4),
                          "fraction_of_copy_ceiling": round(bytes_per_seg / (per_seg * 1e-3) / COPY_CEILING, 4)
                          if per_seg > 0 else None}), flush=True)
    print(json.dumps({"derived_info": [s.derived_info() for s in segs]}))
    for s in segs:
        s.destroy()


if __name__ == "__main__":
    main()
