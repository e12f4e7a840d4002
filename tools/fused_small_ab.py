"""Launch-shape A/B of the small fused scans (sorted SSB Q1.2 / Q1.3 over the SF100 segments), tools/lean_ab.py-style:
one prepared plan per (setting, query) -- the library reads its shape overrides when a plan is created -- executed in
turns inside one process, so every setting sees the same box, the same resident segments and the same clocks.

    python3 tools/fused_small_ab.py --grid --reps 30 ["PHIP_FILTER_NBUF=1 PHIP_STREAM_VALUES=0" ...]

--grid adds PHIP_STREAM_VALUES in {unset, 0} x PHIP_FUSED_SMALL in {unset, 0} x PHIP_FILTER_BPC in {unset, 1, 2, 3, 5};
further settings ("NAME=VALUE NAME=VALUE ...", "" = the defaults) follow as arguments. Two passes over the same plans:
the fused kernel's time from the library's HIP events, then the wall time of one execution without timing markers
(PHIP_KERNEL_TIMING=0 is read per execution; completion by polling, as bench.py's timed steps run). Prints per query
and setting p50 / min / max of both in microseconds with phip_plan_launch_shape's figures, and whether every
setting's results are bit-identical to the default's."""
import argparse
import ctypes
import itertools
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grid():
    out = []
    for sv, fs, bpc in itertools.product((None, "0"), (None, "0"), (None, "1", "2", "3", "5")):
        kv = [("PHIP_STREAM_VALUES", sv), ("PHIP_FUSED_SMALL", fs), ("PHIP_FILTER_BPC", bpc)]
        out.append(" ".join(f"{k}={v}" for k, v in kv if v is not None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings", nargs="*")
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--queries", default="Q1.2,Q1.3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sf", type=int, default=100)
    args = ap.parse_args()
    settings = (grid() if args.grid else []) + [s for s in args.settings if not (args.grid and s == "")]
    if not settings:
        settings = [""]
    from pinot_amd import _lib
    from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    from tools import ssb
    lib = _lib.load()
    _lib.check(lib.phip_init((ctypes.c_int32 * 1)(0), 1))
    queries = args.queries.split(",")
    cols = ssb.columns_for(queries)
    nseg = (args.sf * ssb.ROWS_PER_SF) // ssb.SEGMENT_ROWS
    gsegs = []
    for i in range(0, nseg, 10):
        for r in ssb.make_segments(args.sf, cols, seed=42, segments=range(i, min(nseg, i + 10)), layout="sorted"):
            gsegs.append(GpuSegment(r))
            for ci in r.columns.values():
                if not ci.metadata.is_sorted:
                    ci.forward = b""

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

    ops = {}
    for s in settings:
        env = dict(kv.split("=", 1) for kv in s.split())
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        for q in queries:
            op = GpuInstancePlanMaker().make_instance_plan(parse(ssb.SSB_QUERIES[q]), gsegs)
            op.next_block()  # (the plan is created, and its overrides read, by the first execution)
            ops[(s, q)] = (op, core(op))
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    kern = {k: [] for k in ops}
    wall = {k: [] for k in ops}
    outs = {k: set() for k in ops}
    for _ in range(args.reps):
        for k, (op, _) in ops.items():
            blk = op.next_block()
            kern[k].append(((blk.filter_kernel_ms or 0.0) + (blk.agg_kernel_ms or 0.0)) * 1e3)
    os.environ["PHIP_KERNEL_TIMING"] = "0"
    for rep in range(args.reps + 3):
        for k, (_, c) in ops.items():
            dt, out = snap(c)
            outs[k].add(out)
            if rep >= 3:
                wall[k].append(dt)
    del os.environ["PHIP_KERNEL_TIMING"]
    for q in queries:
        for s in settings:
            kv, wv = kern[(s, q)], wall[(s, q)]
            shape = ops[(s, q)][1].launch_shape() or {}
            same = len(outs[(s, q)]) == 1 and outs[(s, q)] == outs[(settings[0], q)]
            print(f"sorted {q} [{s or 'default'}]: kernel us p50 {statistics.median(kv):.1f} min {min(kv):.1f} max "
                  f"{max(kv):.1f} | wall us p50 {statistics.median(wv):.1f} min {min(wv):.1f} max {max(wv):.1f} "
                  f"(n={len(kv)}, total_work={shape.get('total_work')}, filter_blocks={shape.get('filter_blocks')}, "
                  f"nbuf={shape.get('nbuf')}, fused_lean={shape.get('fused_lean')}, host_final={shape.get('host_final')}, "
                  f"results {'same' if same else 'DIFFER'})", flush=True)
    for op, _ in ops.values():
        op.close()
    for g in gsegs:
        g.destroy()


if __name__ == "__main__":
    main()
