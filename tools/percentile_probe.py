"""Measurement probe of exact PERCENTILE (the value counts of pinot_amd/csrc/distinct.hip) on SSB segments (DESIGN.md
"Exact PERCENTILE and MODE"): per query the warmed median of the whole device sequence (phip_result.device_ms with
PHIP_TOTAL_EVENTS=1), of the distinct pass (distinct_kernel_ms: row clear + mark kernel) and of the host's wall time per
execution, next to DISTINCTCOUNT of the same column (the pass a counts pass can approach) and COUNT(*) under the same
filter. The skewed column (LO_DISCOUNT, 11 values) runs in LDS, and in global rows with and without the in-wave
combining of equal ids (PHIP_COUNTS_COMBINE_CARD / PHIP_COUNTS_COMBINE_ROUNDS), every form measured in one process.
Each query is prepared and measured REPS times with a fresh plan; the spread of those medians is printed.

  python tools/percentile_probe.py [scale factor = 10] [segments = 4]
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
from pinot_amd.engine.reduce import reduce_blocks  # noqa: E402
from pinot_amd.engine.segment import GpuSegment  # noqa: E402
from pinot_amd.query.sql import parse  # noqa: E402
from tools import ssb  # noqa: E402

SF = int(sys.argv[1]) if len(sys.argv) > 1 else 10
NSEG = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WARM, STEPS, REPS = 5, 30, 3
F = "D_YEAR = 1993 and LO_DISCOUNT between 1 and 3 and LO_QUANTITY < 25"  # SSB Q1.1's filter
LDS, GLOBAL = {"PHIP_DISTINCT_LDS_WORDS": "12288"}, {"PHIP_DISTINCT_LDS_WORDS": "0"}
PLAIN = {"PHIP_COUNTS_COMBINE_CARD": "0"}
COMBINE8 = {"PHIP_COUNTS_COMBINE_CARD": "64", "PHIP_COUNTS_COMBINE_ROUNDS": "8"}
COMBINE = {"PHIP_COUNTS_COMBINE_CARD": "64", "PHIP_COUNTS_COMBINE_ROUNDS": "16"}  # the defaults


def _q(select, group=False, where=F):
    w = f" where {where}" if where else ""
    return (f"select C_REGION, {select} from lineorder{w} group by C_REGION" if group
            else f"select {select} from lineorder{w}")


QUERIES = [
    # (name, query, environment of the plan)
    ("count", _q("count(*)"), {}),
    ("supp distinct default", _q("DISTINCTCOUNT(LO_SUPPKEY)"), {}),
    ("supp distinct global", _q("DISTINCTCOUNT(LO_SUPPKEY)"), GLOBAL),
    ("supp p95 default", _q("PERCENTILE95(LO_SUPPKEY)"), {}),
    ("supp p95 lds", _q("PERCENTILE95(LO_SUPPKEY)"), LDS),
    ("supp p95 global", _q("PERCENTILE95(LO_SUPPKEY)"), GLOBAL),
    ("cust distinct default", _q("DISTINCTCOUNT(LO_CUSTKEY)"), {}),
    ("cust p95 default", _q("PERCENTILE95(LO_CUSTKEY)"), {}),
    ("gb count", _q("count(*)", True), {}),
    ("gb supp distinct", _q("DISTINCTCOUNT(LO_SUPPKEY)", True), {}),
    ("gb supp p95", _q("PERCENTILE95(LO_SUPPKEY)", True), {}),
    ("gb cust distinct", _q("DISTINCTCOUNT(LO_CUSTKEY)", True), {}),
    ("gb cust p95", _q("PERCENTILE95(LO_CUSTKEY)", True), {}),
    # the skewed column, under a filter that keeps all 11 values (Q1.1's keeps 3) and under Q1.1's
    ("disc distinct lds", _q("DISTINCTCOUNT(LO_DISCOUNT)", where="LO_QUANTITY < 25"), {}),
    ("disc distinct global", _q("DISTINCTCOUNT(LO_DISCOUNT)", where="LO_QUANTITY < 25"), GLOBAL),
    ("disc p95 lds", _q("PERCENTILE95(LO_DISCOUNT)", where="LO_QUANTITY < 25"), {}),
    ("disc p95 global plain", _q("PERCENTILE95(LO_DISCOUNT)", where="LO_QUANTITY < 25"), {**GLOBAL, **PLAIN}),
    ("disc p95 global combine 8", _q("PERCENTILE95(LO_DISCOUNT)", where="LO_QUANTITY < 25"), {**GLOBAL, **COMBINE8}),
    ("disc p95 global combine 16", _q("PERCENTILE95(LO_DISCOUNT)", where="LO_QUANTITY < 25"), {**GLOBAL, **COMBINE}),
    ("disc q11 p95 global plain", _q("PERCENTILE95(LO_DISCOUNT)"), {**GLOBAL, **PLAIN}),
    ("disc q11 p95 global combine 8", _q("PERCENTILE95(LO_DISCOUNT)"), {**GLOBAL, **COMBINE8}),
    ("disc q11 p95 global combine 16", _q("PERCENTILE95(LO_DISCOUNT)"), {**GLOBAL, **COMBINE}),
    ("gb disc p95 plain", _q("PERCENTILE95(LO_DISCOUNT)", True, "LO_QUANTITY < 25"), PLAIN),
    ("gb disc p95 combine 8", _q("PERCENTILE95(LO_DISCOUNT)", True, "LO_QUANTITY < 25"), COMBINE8),
    ("gb disc p95 combine 16", _q("PERCENTILE95(LO_DISCOUNT)", True, "LO_QUANTITY < 25"), COMBINE),
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
                      "card": {c: segs[0].column_metadata(c).cardinality
                               for c in ("LO_SUPPKEY", "LO_CUSTKEY", "LO_DISCOUNT")}}))
    only = os.environ.get("PROBE_ONLY")  # a substring of the names to run
    for name, q, env in QUERIES:
        if only and only not in name:
            continue
        meds = []
        answer = None
        for _ in range(REPS):
            os.environ.update(env)
            try:
                qc = parse(q)
                op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
                blk = op.next_block()
                meds.append(measure(op, lib))
                op.close()
            finally:
                for k in env:
                    os.environ.pop(k, None)
            matched = blk.stats.num_docs_scanned
            if answer is None and not qc.group_by:
                answer = reduce_blocks(qc, [blk]).rows[0][0]
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
