"""What the finalize launch costs per query, from a rocprofv3 --kernel-trace CSV of
`bench.py --full --no-concurrent --layout sorted --group-by "" --configs ""`: for every fused filter dispatch the gap
to the finalize_all_kernel dispatch that follows it (finalize start - fused end) and that kernel's duration.

    python3 tools/host_final_trace.py run_kernel_trace.csv [-o summary.json]

The three headline queries run the same instantiation, so a dispatch is assigned to its query by its duration (sorted
SF100: Q1.1 > 70 us, Q1.2 23 .. 70 us, Q1.3 < 23 us). Every pass of the bench is in the trace (warm-up, timed steps,
parity, the roofline's timed-marker pass); the medians are the timed steps' (the large majority of the dispatches),
and min / max span all of them. fused_us_no_finalize: the fused dispatches no finalize launch follows, which are
the record-mode executions (none in a parent trace)."""
import argparse
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("-o", default=None)
    args = ap.parse_args()
    rows = []
    with open(args.csv) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    out = {q: {"fused_us": [], "fused_us_no_finalize": [], "gap_us": [], "finalize_us": []} for q in ("Q1.1", "Q1.2", "Q1.3")}
    nfinal = 0
    for i, (s, e, name) in enumerate(rows):
        if "finalize_all_kernel" in name:
            nfinal += 1
        if "phip::filter_kernel<" not in name:
            continue
        d = (e - s) / 1e3
        q = "Q1.1" if d > 70 else ("Q1.2" if d > 23 else "Q1.3")
        out[q]["fused_us"].append(d)
        if i + 1 < len(rows) and "finalize_all_kernel" in rows[i + 1][2]:
            out[q]["gap_us"].append((rows[i + 1][0] - e) / 1e3)
            out[q]["finalize_us"].append((rows[i + 1][1] - rows[i + 1][0]) / 1e3)
        else:  # (record mode: the dispatch no finalize launch follows)
            out[q]["fused_us_no_finalize"].append(d)
    summary = {"finalize_all_dispatches": nfinal, "filter_dispatches": sum(len(v["fused_us"]) for v in out.values())}
    for q, v in out.items():
        summary[q] = {k: ({"n": len(x), "median": round(statistics.median(x), 2), "mean": round(statistics.mean(x), 2),
                           "min": round(min(x), 2), "max": round(max(x), 2)} if x else {"n": 0}) for k, x in v.items()}
    text = json.dumps(summary, indent=1)
    print(text)
    if args.o:
        with open(args.o, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
