"""The segments of tests/test_gpu_long_waves.py: 36 ragged segments, ~0.9 M docs, ~456 work tiles of 2048 docs, laid out
so that a wave that walks a contiguous range of tiles crosses several segments whose columns differ in width.

Segment order (LAYOUT): triplets of bulk segments whose filter column ``w`` needs 3, 11 and 17 bits (so the minimum
DMA count over the segments is a strict lower bound for the tiles of the wider ones), with the tail sizes 1, 63, 64,
65, 2047, 2048, 2049, 4097, 6144 and other tiny segments between them. Segments marked ``low`` hold only tags 0 and 1:
every predicate on ``tag`` above 1 folds to match-none there and the planner drops them, so a kept segment's index
differs from its place in the work list. ``ts`` is sorted over the whole table (segment k holds [1000 k, 1000 k + 999]):
a range on it drops every segment outside it and cuts the tiles of the segments at its ends.

Columns: ts sorted INT; w INT of 3 / 11 / 17 bits; nr INT 7 bits (bit-sliced), wd INT ~20 bits; inv INT with an
inverted index; tag INT; g low-cardinality key (its dictionary shifts with the segment), gr the same values raw; hk
high-cardinality key; m LONG of random 38-bit values (the widest at which the planner still keeps an exact int64 sum:
docs x 2^38 stays below its 2^58 bound, and 40-bit values over 0.9 M docs would be summed in double); rl the same kind
raw; d DOUBLE of multiples of 0.25 below 2^30
(every partial sum is exact: 2^20 docs x 2^30 x 4 < 2^53); sk LONG with a small dictionary (the histogram walk); nl a
nullable INT; rs a raw STRING of a few short values.
"""
import numpy as np

from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType

TILE = 2048
SEED = 20240607

# (num_docs, bits of w (0: whatever the docs allow), low)
LAYOUT = [
    (31_337, 3, False), (1, 0, False), (24_001, 11, False), (70_003, 17, False), (63, 0, False),
    (11_111, 3, True), (64, 0, False), (45_055, 11, False), (2047, 0, False), (66_777, 17, False),
    (65, 0, False), (58_999, 3, False), (700, 0, True), (2048, 0, False), (17_017, 11, False),
    (2049, 0, False), (73_001, 17, False), (4097, 0, False), (39_393, 3, False), (100, 0, True),
    (6144, 0, False), (52_525, 11, False), (13_999, 3, True), (68_123, 17, False), (3, 0, False),
    (27_272, 3, False), (1500, 11, False), (35_353, 11, False), (10_241, 3, False), (71_717, 17, False),
    (129, 0, False), (48_484, 3, False), (20_479, 11, False), (5000, 3, False), (60_001, 11, False),
    (22_222, 3, False),
]
TS_LO, TS_HI = 500, 34_500  # a range on ts: cuts segments 0 and 34 about in half, drops segment 35
STRINGS = np.array(["", "a", "ab", "k7", "zz", "mid", "q"])


def tiles(num_docs):
    return (num_docs + TILE - 1) // TILE


def total_tiles(keep=lambda i, n, low: True):
    """Work tiles of the segments `keep` selects (no hull pruning)."""
    return sum(tiles(n) for i, (n, _, low) in enumerate(LAYOUT) if keep(i, n, low))


def _w_values(rng, n, bits):
    if bits == 0:
        return rng.integers(0, 6, n) * 3
    card = {3: 6, 11: 1500, 17: 66_000}[bits]
    card = min(card, n)
    v = rng.integers(0, card, n)
    v[:card] = np.arange(card)  # every value present: the width is exact
    rng.shuffle(v)
    return v * 3


def make_segment(k, n, bits, low):
    rng = np.random.default_rng(SEED + k)
    c = SegmentCreator(f"lw{k:02d}", inverted_index_columns=["inv"], no_dictionary_columns=["gr", "rl", "rs"])
    c.add_column("ts", DataType.INT, np.sort(rng.integers(1000 * k, 1000 * k + 1000, n)))
    c.add_column("w", DataType.INT, _w_values(rng, n, bits))
    c.add_column("nr", DataType.INT, rng.integers(0, 100, n))
    c.add_column("wd", DataType.INT, rng.integers(0, 1_000_000, n))
    c.add_column("inv", DataType.INT, rng.integers(0, 20, n))
    c.add_column("tag", DataType.INT, rng.integers(0, 2 if low else 10, n))
    g = rng.integers(k % 3, k % 3 + 7, n)
    c.add_column("g", DataType.INT, g)
    c.add_column("gr", DataType.INT, g)
    c.add_column("hk", DataType.INT, rng.integers(0, 30_000, n))
    c.add_column("m", DataType.LONG, rng.integers(0, 1 << 38, n))
    c.add_column("rl", DataType.LONG, rng.integers(0, 1 << 38, n))
    c.add_column("d", DataType.DOUBLE, rng.integers(0, 1 << 32, n) * 0.25)
    sk = rng.integers(-50_000, 50_000, 700 + 13 * k)
    c.add_column("sk", DataType.LONG, sk[rng.integers(0, len(sk), n)])
    c.add_column("nl", DataType.INT, rng.integers(0, 500, n), nulls=(rng.random(n) < 0.1) if k % 4 != 1 else None)
    c.add_column("rs", DataType.STRING, STRINGS[rng.integers(0, len(STRINGS), n)])
    return c.build()


_RAWS = None


def raw_segments():
    """The segments, built once per process."""
    global _RAWS
    if _RAWS is None:
        _RAWS = [make_segment(k, n, bits, low) for k, (n, bits, low) in enumerate(LAYOUT)]
    return _RAWS
