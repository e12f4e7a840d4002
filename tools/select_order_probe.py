"""Selection ORDER BY on SSB-shaped segments: what the device top-K costs beside selection-only and beside a sort of
every matched doc. Not run by any test or by bench.py.

    python3 tools/select_order_probe.py --sf 10 --reps 15
    PHIP_LIB=/path/to/another/libpinot_hip.so python3 tools/select_order_probe.py --legs plain    # e.g. the parent's

For K = 10 and K = 10 000, one and two ORDER BY terms, a selective and an unselective filter, one prepared plan per
leg, executed in turns (warmed: the first execution of every plan is dropped):

    order    the ORDER BY selection
    noprune  the same plan created under PHIP_SELECT_ORDER_PRUNE=0: every matched doc is a candidate
    plain    the same select list as selection-only at LIMIT K (what a library without ORDER BY can run)

and prints per leg the median wall time of one execution (the whole phip_plan_execute: launches, the waits, the copy
of the rows), the filter kernel and the gather-to-rows interval from the library's HIP events (selection-only: the
gather kernel; ORDER BY: gather + sort passes + row gather; the pruning passes lie between the two intervals and
show in the wall time only), and candidates / matched from phip_plan_launch_shape."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILTERS = {"selective": "D_YEAR = 1993 and LO_DISCOUNT between 1 and 3 and LO_QUANTITY < 25",
           "unselective": "LO_QUANTITY < 40"}
ORDERS = {1: "LO_REVENUE desc", 2: "LO_EXTENDEDPRICE desc, LO_REVENUE"}
SELECT = "LO_REVENUE, LO_EXTENDEDPRICE, LO_DISCOUNT, LO_QUANTITY"
COLUMNS = ["D_YEAR", "LO_DISCOUNT", "LO_QUANTITY", "LO_REVENUE", "LO_EXTENDEDPRICE"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=int, default=10)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--legs", default="order,noprune,plain")
    ap.add_argument("--ks", default="10,10000")
    args = ap.parse_args()
    from pinot_amd import _lib
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    from tools import ssb
    _lib.check(_lib.load().phip_init((ctypes.c_int32 * 1)(0), 1))
    nseg = (args.sf * ssb.ROWS_PER_SF) // ssb.SEGMENT_ROWS
    gsegs = []
    for i in range(0, nseg, 10):
        for r in ssb.make_segments(args.sf, COLUMNS, seed=42, segments=range(i, min(nseg, i + 10))):
            gsegs.append(GpuSegment(r))
            for ci in r.columns.values():
                ci.forward = b""
    legs = args.legs.split(",")
    ops = {}
    for fname, where in FILTERS.items():
        for k in (int(x) for x in args.ks.split(",")):
            for nterms, order in ORDERS.items():
                for leg in legs:
                    if leg == "plain" and nterms != 1:
                        continue
                    sql = f"select {SELECT} from lineorder where {where}" + \
                          ("" if leg == "plain" else f" order by {order}") + f" limit {k}"
                    if leg == "noprune":
                        os.environ["PHIP_SELECT_ORDER_PRUNE"] = "0"
                    op = GpuInstancePlanMaker().make_instance_plan(parse(sql), gsegs)
                    op.next_block()  # (the plan is created, and its overrides read, by the first execution)
                    os.environ.pop("PHIP_SELECT_ORDER_PRUNE", None)
                    ops[(fname, k, nterms, leg)] = op
    t = {key: ([], [], []) for key in ops}
    info = {}
    for _ in range(args.reps):
        for key, op in ops.items():
            t0 = time.perf_counter()
            blk = op.next_block()
            t[key][0].append((time.perf_counter() - t0) * 1e3)
            t[key][1].append(blk.filter_kernel_ms or 0.0)
            t[key][2].append(blk.agg_kernel_ms or 0.0)
            info[key] = (blk.stats.num_docs_scanned, (op.launch_shape() or {}).get("select_candidates"), blk.num_rows)
    for key in ops:
        fname, k, nterms, leg = key
        docs, cand, rows = info[key]
        wall, flt, gat = (statistics.median(v) for v in t[key])
        tail = f"candidates {cand} / matched {docs}" if leg != "plain" else f"rows kept per segment summed {docs}"
        print(f"sf{args.sf} {fname} K={k} terms={nterms if leg != 'plain' else 0} {leg}: wall p50 {wall:.3f} ms, "
              f"filter {flt:.3f} ms, gather..rows {gat:.3f} ms, rows {rows}, {tail}", flush=True)
    for op in ops.values():
        op.close()
    for g in gsegs:
        g.destroy()


if __name__ == "__main__":
    main()
