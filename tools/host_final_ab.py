"""In-process A/B of the record mode (PHIP_HOST_FINAL=0 keeps the finalize launch) on the wall time of one execution,
tools/lean_ab.py-style: one prepared plan per (setting, query), executed in turns, without timing markers
(PHIP_KERNEL_TIMING=0, completion by polling: how bench.py's timed steps and a server run).

    python3 tools/host_final_ab.py --reps 30 [--c1-rows 10000000]

Legs: sorted SSB SF100 Q1.1 / Q1.2 / Q1.3 (fused kernels) and, on one 10M-row BenchmarkQueries segment (tools/bq.py),
COUNT_OVER_BITMAP_INDEX_EQUALS (a filter-only plan) and FILTERED_SCAN_SUM (unfused: its aggregation kernel keeps the
finalize launch, so both settings run the same code). Prints per query and setting the p50 / mean / min wall time of
phip_plan_execute in microseconds, phip_plan_launch_shape's host_final, nbuf, filter_blocks, and whether the two
settings' results are bit-identical."""
import argparse
import ctypes
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ("PHIP_HOST_FINAL=0", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sf", type=int, default=100)
    ap.add_argument("--c1-rows", type=int, default=10_000_000)
    ap.add_argument("--skip-ssb", action="store_true")
    args = ap.parse_args()
    os.environ["PHIP_KERNEL_TIMING"] = "0"
    from pinot_amd import _lib
    from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    from tools import bq, ssb
    lib = _lib.load()
    _lib.check(lib.phip_init((ctypes.c_int32 * 1)(0), 1))

    def core(op):
        while not isinstance(op, GpuCombineOperator):
            op = getattr(op, "one_pass", None) or op.__dict__.get("inner") or op.__dict__["op"]
        return op

    def snap(c):
        t0 = time.perf_counter()
        res = c.run_raw()
        dt = time.perf_counter() - t0
        r = res.contents
        out = (r.num_docs_scanned, r.num_entries_scanned_in_filter,
               tuple(struct.pack("<d", r.values[i]) for i in range(r.num_aggregations)),
               tuple(r.long_values[i] for i in range(r.num_aggregations)))
        lib.phip_result_free(res)
        return dt * 1e6, out

    legs = []
    if not args.skip_ssb:
        queries = ["Q1.1", "Q1.2", "Q1.3"]
        cols = ssb.columns_for(queries)
        nseg = (args.sf * ssb.ROWS_PER_SF) // ssb.SEGMENT_ROWS
        gsegs = []
        for i in range(0, nseg, 10):
            for r in ssb.make_segments(args.sf, cols, seed=42, segments=range(i, min(nseg, i + 10)), layout="sorted"):
                gsegs.append(GpuSegment(r))
                for ci in r.columns.values():
                    if not ci.metadata.is_sorted:
                        ci.forward = b""
        legs += [("sorted " + q, ssb.SSB_QUERIES[q], gsegs) for q in queries]
    c1 = [GpuSegment(r) for r in bq.make_segments(args.c1_rows, 1)]
    legs += [(q, bq.QUERIES[q], c1) for q in ("COUNT_OVER_BITMAP_INDEX_EQUALS", "FILTERED_SCAN_SUM")]

    ops = {}
    for s in SETTINGS:
        env = dict(kv.split("=", 1) for kv in s.split())
        os.environ.update(env)
        for name, sql, segs in legs:
            op = GpuInstancePlanMaker().make_instance_plan(parse(sql), segs)
            ops[(s, name)] = (op, core(op))
            for _ in range(3):  # (the plan is created, and PHIP_HOST_FINAL read, by the first execution)
                snap(ops[(s, name)][1])
        for k in env:
            del os.environ[k]
    us = {k: [] for k in ops}
    outs = {k: set() for k in ops}
    for _ in range(args.reps):
        for k, (op, c) in ops.items():
            dt, out = snap(c)
            us[k].append(dt)
            outs[k].add(out)
    for name, _, _ in legs:
        same = all(len(outs[(s, name)]) == 1 for s in SETTINGS) and outs[(SETTINGS[0], name)] == outs[(SETTINGS[1], name)]
        for s in SETTINGS:
            v = us[(s, name)]
            shape = ops[(s, name)][1].launch_shape() or {}
            print(f"{name} [{s or 'default'}]: wall us p50 {statistics.median(v):.1f} mean {statistics.mean(v):.1f} "
                  f"min {min(v):.1f} max {max(v):.1f} (n={len(v)}, host_final={shape.get('host_final')}, "
                  f"fused_lean={shape.get('fused_lean')}, filter_blocks={shape.get('filter_blocks')}, "
                  f"nbuf={shape.get('nbuf')}, total_work={shape.get('total_work')})", flush=True)
        print(f"{name}: results {'bit-identical' if same else 'DIFFER'} across settings and executions", flush=True)
    for op, _ in ops.values():
        op.close()


if __name__ == "__main__":
    main()
