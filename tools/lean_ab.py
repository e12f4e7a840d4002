"""A/B of environment settings inside one process over the SF100 segments of one layout: one prepared plan per
(setting, query) -- the library reads its measurement overrides when a plan is created -- executed in turns, so every
setting sees the same box, the same resident segments and the same clocks.

    python3 tools/lean_ab.py --layout sorted --queries Q1.1,Q1.2,Q1.3 --reps 30 "PHIP_FUSED_LEAN=0" ""

prints per query and setting the fused kernel's time from the library's HIP events (mean / p50 / min / max, ms) and
phip_plan_launch_shape's fused_lean. A setting is "NAME=VALUE NAME=VALUE ..." ("" = the defaults)."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings", nargs="+")
    ap.add_argument("--queries", default="Q1.1,Q1.2,Q1.3")
    ap.add_argument("--layout", default="sorted")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sf", type=int, default=100)
    args = ap.parse_args()
    from pinot_amd import _lib
    from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    from tools import ssb
    _lib.check(_lib.load().phip_init((ctypes.c_int32 * 1)(0), 1))
    queries = args.queries.split(",")
    cols = ssb.columns_for(queries)
    nseg = (args.sf * ssb.ROWS_PER_SF) // ssb.SEGMENT_ROWS
    gsegs = []
    for i in range(0, nseg, 10):
        for r in ssb.make_segments(args.sf, cols, seed=42, segments=range(i, min(nseg, i + 10)), layout=args.layout):
            gsegs.append(GpuSegment(r))
            for ci in r.columns.values():
                if not ci.metadata.is_sorted:
                    ci.forward = b""

    def core(op):
        while not isinstance(op, GpuCombineOperator):
            op = getattr(op, "one_pass", None) or op.__dict__.get("inner") or op.__dict__["op"]
        return op

    ops = {}
    for s in args.settings:
        env = dict(kv.split("=", 1) for kv in s.split())
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        for q in queries:
            ops[(s, q)] = GpuInstancePlanMaker().make_instance_plan(parse(ssb.SSB_QUERIES[q]), gsegs)
            ops[(s, q)].next_block()  # (the plan is created, and its overrides read, by the first execution)
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    ms = {k: [] for k in ops}
    for _ in range(args.reps):
        for k, op in ops.items():
            blk = op.next_block()
            ms[k].append((blk.filter_kernel_ms or 0.0) + (blk.agg_kernel_ms or 0.0))
    for q in queries:
        for s in args.settings:
            v = ms[(s, q)]
            shape = core(ops[(s, q)]).launch_shape() or {}
            print(f"{args.layout} {q} [{s or 'default'}]: kernel ms mean {statistics.mean(v):.4f} p50 "
                  f"{statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f} (n={len(v)}, fused_lean="
                  f"{shape.get('fused_lean')}, filter_blocks={shape.get('filter_blocks')}, nbuf={shape.get('nbuf')})",
                  flush=True)
    for op in ops.values():
        op.close()
    for g in gsegs:
        g.destroy()


if __name__ == "__main__":
    main()
