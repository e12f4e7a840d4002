"""Per-query dispatch times of the fused filter kernel from a rocprofv3 --kernel-trace CSV of
`bench.py --gpus 1 --steps 20 --warmup 5` (the sorted headline: Q1.1, Q1.2, Q1.3 in turns).

    python3 tools/fused_small_trace.py run_kernel_trace.csv --q12-blocks 944 [-o summary.json]

A dispatch is assigned to its query by its workgroup count (grid size / workgroup size), which the launch shapes make
distinct: Q1.1 1280, Q1.3 216, Q1.2 256 before the residency rule and --q12-blocks after it (tools/host_final_trace.py
assigns by duration, which no longer separates Q1.2 from Q1.3). The record-mode executions -- the bench's timed steps
-- are the dispatches no finalize_all_kernel follows; the others (timed-marker passes) are listed apart."""
import argparse
import csv
import json
import statistics


def _stats(x):
    if not x:
        return {"n": 0}
    return {"n": len(x), "median": round(statistics.median(x), 2), "mean": round(statistics.mean(x), 2),
            "min": round(min(x), 2), "max": round(max(x), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--q12-blocks", type=int, default=256)
    ap.add_argument("-o", default=None)
    args = ap.parse_args()
    rows = []
    with open(args.csv) as f:
        for r in csv.DictReader(f):
            grid = int(r.get("Grid_Size") or r.get("Grid_Size_X"))
            wg = int(r.get("Workgroup_Size") or r.get("Workgroup_Size_X"))
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid // max(wg, 1)))
    rows.sort()
    by_blocks = {1280: "Q1.1", args.q12_blocks: "Q1.2", 216: "Q1.3"}
    out = {q: {"record_mode_us": [], "with_finalize_us": []} for q in ("Q1.1", "Q1.2", "Q1.3")}
    other = {}
    for i, (s, e, name, blocks) in enumerate(rows):
        if "phip::filter_kernel<" not in name:
            continue
        q = by_blocks.get(blocks)
        if q is None:
            other[blocks] = other.get(blocks, 0) + 1
            continue
        fin = i + 1 < len(rows) and "finalize_all_kernel" in rows[i + 1][2]
        out[q]["with_finalize_us" if fin else "record_mode_us"].append((e - s) / 1e3)
    summary = {q: {k: _stats(x) for k, x in v.items()} for q, v in out.items()}
    summary["other_filter_dispatches_by_workgroups"] = other
    text = json.dumps(summary, indent=1)
    print(text)
    if args.o:
        with open(args.o, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
