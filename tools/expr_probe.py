"""Measurement probe of derived value columns (pinot_amd/csrc/expr.hip; DESIGN.md §3 "Derived value columns") on SSB
segments, the setup of tools/distinct_probe.py. Three fresh plans per query, warmed medians of 30 executions each:

  * materialise: plan creation with the expression's columns built (every segment's column evicted first by 16 other
    expressions) minus plan creation with them cached, per segment, and its fraction of the 6.1 TB/s copy ceiling for
    the input words + 8 B per doc;
  * the query's first execution (plan creation included) against its warmed execution;
  * SUM(LO_EXTENDEDPRICE * LO_DISCOUNT), the two-gather PHIP_EXPR_MUL path, against
    SUM(LO_EXTENDEDPRICE * LO_DISCOUNT * 1), one 8-byte load per matched doc. The baseline of that comparison is the
    parent commit's library measured in the same session (PHIP_LIB selects a library), never this tree's own number.

  python tools/expr_probe.py [scale factor = 10] [segments = 4]
"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
os.environ["PHIP_TOTAL_EVENTS"] = "1"
from pinot_amd import _lib  # noqa: E402
from pinot_amd.engine.plan import GpuInstancePlanMaker, UnsupportedOnGpu  # noqa: E402
from pinot_amd.engine.segment import GpuSegment  # noqa: E402
from pinot_amd.query.sql import parse  # noqa: E402
from tools import ssb  # noqa: E402

SF = int(sys.argv[1]) if len(sys.argv) > 1 else 10
NSEG = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WARM, STEPS, REPS = 5, 30, 3
COPY_CEILING = 6.1e12  # bytes / s, the measured copy ceiling
F = "D_YEAR = 1993 and LO_DISCOUNT between 1 and 3 and LO_QUANTITY < 25"  # SSB Q1.1's filter
REVENUE = "LO_EXTENDEDPRICE * (1 - LO_DISCOUNT) * (1 + LO_TAX)"
QUERIES = [
    ("count", f"select count(*) from lineorder where {F}"),
    ("two-gather a*b", f"select sum(LO_EXTENDEDPRICE * LO_DISCOUNT) from lineorder where {F}"),
    ("derived a*b*1", f"select sum(LO_EXTENDEDPRICE * LO_DISCOUNT * 1) from lineorder where {F}"),
    ("derived a*(1-b)*(1+c)", f"select sum({REVENUE}) from lineorder where {F}"),
    ("derived a*(1-b)*(1+c), no filter", f"select sum({REVENUE}) from lineorder"),
]


def prepare(sql, segs):
    t0 = time.perf_counter()
    op = GpuInstancePlanMaker().make_instance_plan(parse(sql), segs)
    op.run_raw(prepare_only=True)
    return op, 1e3 * (time.perf_counter() - t0)


def evict(segs):
    """Pushes every derived column out of the segments' caches: 16 other expressions."""
    for k in range(16):
        op, _ = prepare(f"select sum(LO_QUANTITY * {k + 2} + {k}) from lineorder", segs)
        op.close()


def measure(op, lib):
    dev, agg, flt, wall = [], [], [], []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        r = op.run_raw()
        t1 = time.perf_counter()
        c = r.contents
        if i >= WARM:
            dev.append(c.device_ms)
            agg.append(c.agg_kernel_ms)
            flt.append(c.filter_kernel_ms)
            wall.append(1e3 * (t1 - t0))
        lib.phip_result_free(r)
    return [statistics.median(x) for x in (dev, agg, flt, wall)]


def main():
    lib = _lib.load()
    _lib.check(lib.phip_init((ctypes.c_int32 * 1)(0), 1))
    cols = ["D_YEAR", "LO_DISCOUNT", "LO_QUANTITY", "LO_EXTENDEDPRICE", "LO_TAX"]
    segs = [GpuSegment(r) for r in ssb.make_segments(SF, cols, segments=range(NSEG))]
    docs = sum(s.num_docs for s in segs)
    in_bits = sum(segs[0].column_metadata(c).bits_per_element for c in ("LO_EXTENDEDPRICE", "LO_DISCOUNT", "LO_TAX"))
    print(json.dumps({"sf": SF, "segments": NSEG, "docs": docs, "revenue_input_bits_per_doc": in_bits}))
    for name, q in QUERIES:
        meds, cold, cached, first = [], [], [], []
        for _ in range(REPS):
            try:
                if name.startswith("derived"):
                    evict(segs)
                t0 = time.perf_counter()
                op, p_cold = prepare(q, segs)
                blk = op.next_block()
                first.append(1e3 * (time.perf_counter() - t0))
                op2, p_cached = prepare(q, segs)
                op2.close()
            except UnsupportedOnGpu as e:  # (the parent commit's library: no derived columns)
                print(json.dumps({"query": name, "refused": str(e)}), flush=True)
                break
            cold.append(p_cold)
            cached.append(p_cached)
            meds.append(measure(op, lib))
            op.close()
        else:
            row = {"query": name, "matched": blk.stats.num_docs_scanned, "answer": blk.results[0],
                   "first_execution_ms": round(statistics.median(first), 3)}
            for j, k in enumerate(("device_ms", "agg_ms", "filter_ms", "wall_ms")):
                xs = [m[j] for m in meds]
                row[k] = round(statistics.median(xs), 4)
                row[k + "_spread"] = [round(min(xs), 4), round(max(xs), 4)]
            if name.startswith("derived"):
                per_seg = (statistics.median(cold) - statistics.median(cached)) / NSEG
                row["materialise_ms_per_segment"] = round(per_seg, 4)
                if "(1-b)" in name and per_seg > 0:
                    bytes_per_seg = docs / NSEG * (in_bits / 8.0 + 8.0)
                    row["fraction_of_copy_ceiling"] = round(bytes_per_seg / (per_seg * 1e-3) / COPY_CEILING, 4)
            print(json.dumps(row), flush=True)
    if hasattr(segs[0], "derived_info"):  # (absent from the parent commit's tree)
        print(json.dumps({"derived_info": [s.derived_info() for s in segs]}))
    for s in segs:
        s.destroy()


if __name__ == "__main__":
    main()
