"""Measurement probe of exact DISTINCTCOUNT (pinot_amd/csrc/distinct.hip) on SSB segments (DESIGN.md "Exact
DISTINCTCOUNT"): per query the warmed median of the whole device sequence (phip_result.device_ms with
PHIP_TOTAL_EVENTS=1), of the distinct pass (distinct_kernel_ms: bitmap clear + mark kernel) and of the host's wall
time per execution, next to DISTINCTCOUNTHLL of the same column and COUNT(*) under the same filter (the floor).
Each query is prepared and measured REPS times with a fresh plan; the spread of those medians is printed.

  python tools/distinct_probe.py [scale factor = 10] [segments = 4]
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
from pinot_amd.engine.plan import GpuInstancePlanMaker  # noqa: E402
from pinot_amd.engine.segment import GpuSegment  # noqa: E402
from pinot_amd.query.sql import parse  # noqa: E402
from tools import ssb  # noqa: E402

SF = int(sys.argv[1]) if len(sys.argv) > 1 else 10
NSEG = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WARM, STEPS, REPS = 5, 30, 3
F = "D_YEAR = 1993 and LO_DISCOUNT between 1 and 3 and LO_QUANTITY < 25"  # SSB Q1.1's filter
QUERIES = [
    # (name, query, environment of the plan)
    ("count", f"select count(*) from lineorder where {F}", {}),
    ("supp hll", f"select DISTINCTCOUNTHLL(LO_SUPPKEY) from lineorder where {F}", {}),
    ("supp exact lds", f"select DISTINCTCOUNT(LO_SUPPKEY) from lineorder where {F}", {}),
    ("supp exact global", f"select DISTINCTCOUNT(LO_SUPPKEY) from lineorder where {F}", {"PHIP_DISTINCT_LDS_WORDS": "0"}),
    ("cust hll", f"select DISTINCTCOUNTHLL(LO_CUSTKEY) from lineorder where {F}", {}),
    ("cust exact global", f"select DISTINCTCOUNT(LO_CUSTKEY) from lineorder where {F}", {}),
    ("cust exact lds", f"select DISTINCTCOUNT(LO_CUSTKEY) from lineorder where {F}", {"PHIP_DISTINCT_LDS_WORDS": "12288"}),
    ("gb count", f"select C_REGION, count(*) from lineorder where {F} group by C_REGION", {}),
    ("gb supp hll", f"select C_REGION, DISTINCTCOUNTHLL(LO_SUPPKEY) from lineorder where {F} group by C_REGION", {}),
    ("gb supp exact", f"select C_REGION, DISTINCTCOUNT(LO_SUPPKEY) from lineorder where {F} group by C_REGION", {}),
]


def measure(op, lib):
    dev, dist, wall, flt = [], [], [], []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        r = op.run_raw()
        t1 = time.perf_counter()
        c = r.contents
        if i >= WARM:
            dev.append(c.device_ms)
            dist.append(c.distinct_kernel_ms)
            flt.append(c.filter_kernel_ms)
            wall.append(1e3 * (t1 - t0))
        lib.phip_result_free(r)
    return [statistics.median(x) for x in (dev, dist, flt, wall)]


def main():
    lib = _lib.load()
    _lib.check(lib.phip_init((ctypes.c_int32 * 1)(0), 1))
    cols = ["D_YEAR", "LO_DISCOUNT", "LO_QUANTITY", "LO_SUPPKEY", "LO_CUSTKEY", "C_REGION"]
    segs = [GpuSegment(r) for r in ssb.make_segments(SF, cols, segments=range(NSEG))]
    docs = sum(s.num_docs for s in segs)
    print(json.dumps({"sf": SF, "segments": NSEG, "docs": docs,
                      "card": {c: segs[0].column_metadata(c).cardinality for c in ("LO_SUPPKEY", "LO_CUSTKEY")}}))
    for name, q, env in QUERIES:
        meds = []
        answer = None
        for _ in range(REPS):
            os.environ.update(env)
            try:
                op = GpuInstancePlanMaker().make_instance_plan(parse(q), segs)
                blk = op.next_block()
                meds.append(measure(op, lib))
                op.close()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            matched = blk.stats.num_docs_scanned
            if answer is None and not parse(q).group_by:
                v = blk.results[0]
                answer = len(v) if isinstance(v, set) else (int(v) if isinstance(v, int) else None)
        row = {"query": name, "matched": matched, "answer": answer}
        for j, k in enumerate(("device_ms", "distinct_ms", "filter_ms", "wall_ms")):
            xs = [m[j] for m in meds]
            row[k] = round(statistics.median(xs), 4)
            row[k + "_spread"] = [round(min(xs), 4), round(max(xs), 4)]
        print(json.dumps(row), flush=True)
    for s in segs:
        s.destroy()


if __name__ == "__main__":
    main()
