"""Measurement probe of LIKE / REGEXP_LIKE (pinot_amd/csrc/strmatch.hip; DESIGN.md §3 "String matching").

  (a) the raw pre-pass: one segment of DOCS URL-like raw STRING values of ~24 bytes, COUNT(*) under three patterns --
      ^www\\.domain1 (early exit), checkout (substring), \\.com$ (suffix). The match launch sits before the filter
      launch's timing markers, so its time is device_ms - scan_kernel_ms less the same difference of a plan without a
      pre-pass (a predicate on a dictionary column). Bytes streamed = the values' bytes + 8 (num_docs + 1), against
      the 6.1 TB/s copy ceiling DESIGN.md records, beside the RAW_STRING_SET EQ leaf on the same column (its filter
      kernel's scan_kernel_ms);
  (b) the dictionary match: cardinalities 1 K, 64 K, 1 M, 4 M at width 32 -- the device (the first call uploads the
      dictionary; then cached) against Dfa.match_many on the host: the crossover sets segment.STRMATCH_HOST_CARD.

Warmed medians.   python tools/strmatch_probe.py [docs = 6000000] [largest cardinality = 4194304]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
os.environ["PHIP_TOTAL_EVENTS"] = "1"
from pinot_amd import _lib  # noqa: E402
from pinot_amd.engine.plan import GpuInstancePlanMaker  # noqa: E402
from pinot_amd.engine.segment import GpuSegment  # noqa: E402
from pinot_amd.query import regex_dfa  # noqa: E402
from pinot_amd.query.sql import parse  # noqa: E402
from pinot_amd.segment.creator import ColumnIndexes, ColumnMetadata, ImmutableSegment, SegmentCreator, pack_bits  # noqa: E402
from pinot_amd.spi import DataType, num_bits_per_value  # noqa: E402

DOCS = int(sys.argv[1]) if len(sys.argv) > 1 else 6_000_000
MAX_CARD = int(sys.argv[2]) if len(sys.argv) > 2 else 4 << 20
WARM, STEPS = 5, 30
COPY_CEILING = 6.1e12


def pre_pass_ms(seg, where):
    op = GpuInstancePlanMaker().make_instance_plan(parse(f"SELECT COUNT(*) FROM t WHERE {where}"), [seg])
    for _ in range(WARM):
        blk = op.next_block()
    outside, inside = [], []
    for _ in range(STEPS):
        blk = op.next_block()
        outside.append(blk.device_ms - blk.scan_kernel_ms)
        inside.append(blk.scan_kernel_ms)
    return statistics.median(outside), statistics.median(inside), int(blk.results[0])


def raw_probe():
    rng = np.random.default_rng(1)
    hosts = np.array(["www.domain%d.com" % i for i in range(1, 9)] + ["www.sd.domain%d.co.ab" % i for i in range(1, 9)])
    paths = np.array(["/a", "/cart", "/checkout", "/p/123456", "/search?q=x", "/"])
    vals = np.char.add(hosts[rng.integers(0, len(hosts), DOCS)], paths[rng.integers(0, len(paths), DOCS)])
    nbytes = int(np.char.str_len(vals).sum())
    raw = SegmentCreator("smprobe", no_dictionary_columns=["s"]).add_column("s", DataType.STRING, vals) \
        .add_column("k", DataType.INT, rng.integers(0, 64, DOCS)).build()
    seg = GpuSegment(raw)
    try:
        base, _, _ = pre_pass_ms(seg, "k < 32")
        streamed = nbytes + 8 * (DOCS + 1)
        for pat in ("^www\\.domain1", "checkout", "\\.com$"):
            out, _, count = pre_pass_ms(seg, f"REGEXP_LIKE(s, '{pat}')")
            ms = out - base
            print(json.dumps({"probe": "raw_prepass", "pattern": pat, "docs": DOCS, "mean_bytes": nbytes / DOCS,
                              "matched": count, "ms": round(ms, 4), "gbps": round(streamed / ms / 1e6, 1),
                              "of_copy_ceiling": round(streamed / (ms * 1e-3) / COPY_CEILING, 3)}))
        _, inside, count = pre_pass_ms(seg, "s = 'www.domain1.com/checkout'")
        print(json.dumps({"probe": "raw_string_set_eq", "docs": DOCS, "matched": count, "ms": round(inside, 4),
                          "gbps": round(streamed / inside / 1e6, 1)}))
    finally:
        seg.destroy()


def dict_probe(card):
    width = 32
    vals = np.array([b"www.domain%09d.com/path" % i for i in range(card)], dtype="S32")  # sorted: zero-padded numbers
    bits = num_bits_per_value(card - 1)
    seg = ImmutableSegment(f"smdict{card}", card)
    seg.columns["d"] = ColumnIndexes(ColumnMetadata("d", DataType.STRING, card, card, bits, False, True, False, width),
                                     pack_bits(np.arange(card, dtype=np.int32), bits), vals.tobytes())
    g = GpuSegment(seg)
    try:
        pattern = "domain0+12"
        dfa = regex_dfa.compile_pattern(pattern)
        res = {"probe": "dictionary", "card": card, "width": width}
        for how, hc, reps in (("device", "0", 12), ("host", str(1 << 40), 3)):
            os.environ["PINOT_AMD_STRMATCH_HOST_CARD"] = hc
            times = []
            for _ in range(reps):
                g._matches.clear()
                t0 = time.perf_counter()
                ids = g.match_dictionary("d", pattern, dfa)
                times.append((time.perf_counter() - t0) * 1e3)
            if how == "device":
                res["device_first_ms"] = round(times[0], 3)   # uploads the dictionary
                res["device_cached_ms"] = round(statistics.median(times[2:]), 3)
            else:
                res["host_ms"] = round(statistics.median(times), 3)
            res["matched"] = len(ids)
        print(json.dumps(res))
    finally:
        g.destroy()
        os.environ.pop("PINOT_AMD_STRMATCH_HOST_CARD", None)


def main():
    _lib.check(_lib.load().phip_init(None, 0))
    raw_probe()
    for card in (1 << 10, 1 << 16, 1 << 20, 4 << 20):
        if card <= MAX_CARD:
            dict_probe(card)


if __name__ == "__main__":
    main()
