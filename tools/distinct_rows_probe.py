"""Measurement probe of SELECT DISTINCT (pinot_amd/csrc/distinct_rows.hip; DESIGN.md §3 "SELECT DISTINCT"): synthetic
segments of SSB size -- 6 000 000 docs each, as many as asked -- with a 5-bit and a 3-bit column (125 keys: the LDS
bitmap), a 20-bit column (10^6 keys: the global bitmap), a 20-bit x 18-bit pair (2 x 10^11 keys: sorted keys) and a
10-bit column for the filter: selective (1 % of the docs) and unselective (90 %).

  distinct  per query and filter: the warmed wall time of an execution (phip_plan_execute to the decoded result
            struct), its device time (filter launch + the pass's bitmap clear and mark kernel; the pick, sort and
            decode launches are in the wall time only), the mark time alone, the rows returned and the regime;
  groupby   the equivalent SELECT cols, COUNT(*) ... GROUP BY cols LIMIT n on the same segments: wall time, the
            library's device time, its filter and aggregation kernel times. Run it with PHIP_LIB naming another
            build of the library (the parent commit's) to put the two side by side in one session.

Both modes print the new kernels' resource usage first -- VGPRs, SGPRs, LDS, scratch, spills, occupancy -- from the
compiler's own remarks (pinot_amd/csrc/distinct_rows.hip compiled with -Rpass-analysis=kernel-resource-usage and the
library's flags); "resources": null where no hipcc is installed. Warmed medians of STEPS executions, REPS fresh plans.

  python tools/distinct_rows_probe.py [distinct | groupby] [segments = 4] [docs per segment = 6000000]
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
from pinot_amd import _lib  # noqa: E402
from pinot_amd.engine.plan import GpuInstancePlanMaker  # noqa: E402
from pinot_amd.engine.segment import GpuSegment  # noqa: E402
from pinot_amd.query.sql import parse  # noqa: E402
from pinot_amd.segment.creator import ColumnIndexes, ColumnMetadata, ImmutableSegment, pack_bits  # noqa: E402
from pinot_amd.spi import DataType  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "distinct"
NSEG = int(sys.argv[2]) if len(sys.argv) > 2 else 4
DOCS = int(sys.argv[3]) if len(sys.argv) > 3 else 6_000_000
WARM, STEPS, REPS = 3, 15, 3
COLUMNS = {"c": (25, 5), "r": (5, 3), "k": (1_000_000, 20), "p": (200_000, 18), "f": (1000, 10)}  # cardinality, bits
QUERIES = [("low cardinality (c, r: 125 keys)", ["c", "r"], 1000), ("one wide column (k: 10^6 keys)", ["k"], 1000),
           ("sorted keys (k, p: 2 x 10^11 keys)", ["k", "p"], 1000)]
FILTERS = [("selective, 1 %", "f < 10"), ("unselective, 90 %", "f < 900")]
REGIMES = {0: "none", 1: "lds", 2: "global", 3: "sorted"}


def make_segment(i):
    """Built from arrays (SegmentCreator's per-row path is for test sizes): uniform ids, identity dictionaries."""
    rng = np.random.default_rng(1000 + i)
    seg = ImmutableSegment(f"drprobe{i}", DOCS)
    for name, (card, bits) in COLUMNS.items():
        ids = rng.integers(0, card, DOCS).astype(np.int32)
        seg.columns[name] = ColumnIndexes(ColumnMetadata(name, DataType.INT, DOCS, card, bits, False, True, False),
                                          pack_bits(ids, bits), np.arange(card, dtype=">i4").tobytes())
    return seg


def kernel_resources():
    """Per kernel of distinct_rows.hip what hipcc's kernel-resource-usage remarks say, with the library's flags."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join("pinot_amd", "csrc", "distinct_rows.hip")
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
                            "-fvisibility=hidden", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                            os.path.join(d, "distinct_rows.o"), src], capture_output=True, text=True)
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "SGPRs Spill": "sgpr_spills",
            "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"\d+(distinct_rows_\w+?_kernel)(ILi(\d)E)?", m.group(2))
            label = (name.group(1) + (f"<{REGIMES[int(name.group(3))]}>" if name.group(3) else "")) if name else m.group(2)
            cur = out.setdefault(label, {})
        elif cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out or None


def measure(sql, segs, lib):
    wall, dev, flt, agg = [], [], [], []
    rows = matched = regime = None
    for _ in range(REPS):
        op = GpuInstancePlanMaker().make_instance_plan(parse(sql), segs)
        core = getattr(op, "inner", op)
        w, d, f, a = [], [], [], []
        for i in range(WARM + STEPS):
            t0 = time.perf_counter()
            r = core.run_raw()
            t1 = time.perf_counter()
            c = r.contents
            if i >= WARM:
                w.append(1e3 * (t1 - t0))
                d.append(c.filter_kernel_ms + c.agg_kernel_ms if MODE == "distinct" else c.device_ms)
                f.append(c.filter_kernel_ms)
                a.append(c.agg_kernel_ms)
            rows, matched = int(c.num_rows if MODE == "distinct" else c.num_groups), int(c.num_docs_scanned)
            lib.phip_result_free(r)
        if MODE == "distinct":
            regime = REGIMES[core.launch_shape()["distinct_rows_regime"]]
        op.close()
        for acc, v in ((wall, w), (dev, d), (flt, f), (agg, a)):
            acc.append(statistics.median(v))
    out = {"matched": matched, "rows": rows, "wall_ms": round(statistics.median(wall), 4),
           "wall_ms_spread": [round(min(wall), 4), round(max(wall), 4)], "device_ms": round(statistics.median(dev), 4),
           "filter_ms": round(statistics.median(flt), 4)}
    if MODE == "distinct":
        out["mark_ms"] = round(statistics.median(agg), 4)
        out["regime"] = regime
    else:
        out["agg_ms"] = round(statistics.median(agg), 4)
    return out


def main():
    if MODE not in ("distinct", "groupby"):
        raise SystemExit(__doc__)
    print(json.dumps({"mode": MODE, "library": _lib.LIB_PATH, "resources": kernel_resources()}), flush=True)
    lib = _lib.load()
    _lib.check(lib.phip_init((ctypes.c_int32 * 1)(0), 1))
    segs = [GpuSegment(make_segment(i)) for i in range(NSEG)]
    print(json.dumps({"segments": NSEG, "docs": NSEG * DOCS}), flush=True)
    for label, cols, limit in QUERIES:
        for fname, where in FILTERS:
            names = ", ".join(cols)
            sql = (f"SELECT DISTINCT {names} FROM t WHERE {where} ORDER BY {names} LIMIT {limit}" if MODE == "distinct"
                   else f"SELECT {names}, COUNT(*) FROM t WHERE {where} GROUP BY {names} ORDER BY {names} LIMIT {limit}")
            try:
                row = measure(sql, segs, lib)
            except Exception as e:  # noqa: BLE001 -- a refusal is a finding of the probe
                row = {"error": f"{type(e).__name__}: {e}"}
            print(json.dumps({"query": label, "filter": fname, **row}), flush=True)
    for s in segs:
        s.destroy()


if __name__ == "__main__":
    main()
