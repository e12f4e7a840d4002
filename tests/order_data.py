"""The segments of tests/test_order_by_specials.py and tests/test_gpu_order_by_specials.py: 16 groups whose final results
are the Double.compare ladder -- -inf, -DBL_MAX, a negative denormal, -0.0, 0.0, a positive denormal, DBL_MAX, +inf, a NaN
with its sign bit set, one with it clear, one born of inf - inf -- with ties, so that an ORDER BY over them and a trim at
every boundary position can be compared with java_fold.record_compare.

Two segments of 2 * 2048 + 77 and 2048 + 5 docs (segment 0 holds the ladder; the matched docs of segment 1 hold zeros in
the summed columns and other fillers in ``x``, so its dictionaries differ and the merged ladder equals segment 0's).
Group ``i`` (the index of the tables below) has the key ``G[i]``: key order differs from the tables' order.

  g / gr    INT key, dictionary / raw
  gd        DOUBLE dictionary key, GD[i]. A dictionary holds one entry per ``np.unique`` value: -0.0 and 0.0 share one
            (stored as -0.0: the groups 4 and 5 tie on gd), as would two NaNs.
  f         INT; ``f < 99`` excludes exactly the poison docs (1 + i % 3 per group and segment), which hold -inf, NaN or
            1e308 in every metric and new values in ``h``: an order taken from unfiltered values shows.
  s / s_r   DOUBLE, dictionary / raw: every matched doc 0.0 (group 10: -0.0) but the docs that hold S[i] -- a sum of
            zeros and one value (or of 1.0 + 1.25) is exact in any order. The dictionary column keeps one zero and one
            NaN, whichever ``np.unique`` met first; s_r keeps every bit, the NaN with its sign bit set among them.
  sf        FLOAT, the same ladder with the float extremes (SF[i])
  x / x_r   DOUBLE without NaN: group i's docs lie in [X[i][0], X[i][1]], both ends present; the groups 5 and 6 hold
            only -0.0 resp. only 0.0 (x_r; in the dictionary column x every zero is -0.0), group 10 only +inf (its range
            is inf - inf), group 11 only -inf
  h         INT with H[i] distinct values per group (the same in both segments): DISTINCTCOUNTHLL estimates with ties

COUNT ties: the groups of COUNT_TIE hold the same number of matched docs (and of poison docs: i % 3 is equal).

Expected values are folds (tests/java_fold.py) of the *stored* values of the docs of a group in doc order, read back
from the index bytes; nothing here runs the library or the oracle, except ``hll_registers``, which offers values to the
oracle's HyperLogLog.
"""
import functools

import numpy as np

from pinot_amd.segment.creator import SegmentCreator, read_chunk_forward
from pinot_amd.spi import DataType
from tests import java_fold as jf

TILE = 2048
NUM_DOCS = (2 * TILE + 77, TILE + 5)
NG = 16
SEED = 20261019
INF = float("inf")
DBL_MAX = 1.7976931348623157e308
DENORM = 5e-324
FLT_MAX = float(np.finfo(np.float32).max)
FLT_DENORM = float(np.float32(1.4e-45))
NAN_POS, NAN_NEG = 0x7FF8000000000000, 0xFFF8000000000000
F32_NAN_POS, F32_NAN_NEG = 0x7FC00000, 0xFFC00000


def _d(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def _f(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


G = [113, 7, 58, 21, 99, 3, 76, 40, 12, 131, 65, 29, 88, 50, 1, 107]
GD = [-INF, -DBL_MAX, -1.5, -DENORM, -0.0, 0.0, DENORM, 2.25, DBL_MAX, INF, _d(NAN_POS), 3.5, -1e10, 1e-3, 42.0, -7.25]
# the values some matched docs of group i hold in s (segment 0); every other matched doc holds ZERO[i]
S = [[_d(NAN_NEG)], [_d(NAN_POS)], [INF, -INF], [-INF], [INF], [-DBL_MAX], [DBL_MAX], [-DENORM], [DENORM], [], [],
     [-1.5], [-1.5], [2.25], [1.0, 1.25], [1e300]]
SF = [[_f(F32_NAN_NEG)], [_f(F32_NAN_POS)], [INF, -INF], [-INF], [INF], [-FLT_MAX], [FLT_MAX], [-FLT_DENORM], [FLT_DENORM],
      [], [], [-1.5], [-1.5], [2.25], [1.0, 1.25], [float(np.float32(1e30))]]
ZERO = [0.0] * 10 + [-0.0] + [0.0] * 5
# (min, max, fillers of segment 0, fillers of segment 1) of x
X = [(-INF, 7.0, [-3.5, 1.0], [6.75, -1e300]), (-DBL_MAX, DBL_MAX, [-1e308, 12.5], [1e308, -0.25]),
     (-1.5, -1.5, [], []), (-1.5, 2.5, [-1.25, 0.5], [2.25, 1.0]), (-DENORM, DENORM, [0.0], [0.0]),
     (-0.0, -0.0, [], []), (0.0, 0.0, [], []), (DENORM, DENORM, [], []), (2.25, 6.25, [2.5, 3.0], [6.0, 4.75]),
     (DBL_MAX, INF, [], []), (INF, INF, [], []), (-INF, -INF, [], []), (10.5, 20.5, [11.0, 12.25], [20.25, 15.0]),
     (-3.25, 100.0, [0.75, 99.5], [-3.0, 64.0]), (-7.0, -DENORM, [-6.5, -1.0], [-2.25, -1e-300]),
     (3.0, DBL_MAX, [3.5, 1e300], [4.0, 1e308])]
H = [1, 1, 2, 3, 3, 5, 5, 8, 8, 13, 13, 21, 21, 34, 34, 40]
COUNT_TIE = (3, 6, 9, 12)   # (equal i % 3: equal numbers of poison docs too)


def s_poison(i):
    """The poison of group i in s and sf: one kind per group, so that the unfiltered sum is exact in any order too --
    1e308 (3e38) only beside zeros and denormals, else -inf or NaN, which absorb what they meet."""
    if i in (7, 8, 9, 10):
        return 1e308, 3e38
    return (-INF, -INF) if i % 2 else (_d(NAN_POS), _f(F32_NAN_POS))


def x_poison(i):
    return -INF if i % 2 else 1e308


def group_sizes(matched_total):
    """Matched docs per group: all different but for COUNT_TIE, at least 50 each."""
    sizes = [50 + 9 * i for i in range(NG)]
    for i in COUNT_TIE:
        sizes[i] = 60
    sizes[NG - 1] += matched_total - sum(sizes)
    assert min(sizes) >= 50 and sizes[NG - 1] > max(sizes[:NG - 1])
    return sizes


def build_columns(k):
    """{name: (DataType, source values)} of segment k and the group index of every doc."""
    n = NUM_DOCS[k]
    rng = np.random.default_rng(SEED + k)
    n_poison = [1 + i % 3 for i in range(NG)]
    sizes = group_sizes(n - sum(n_poison))
    docs = rng.permutation(n)
    group = np.empty(n, dtype=np.int64)
    f = rng.integers(0, 99, n)
    s = np.zeros(n)
    sf = np.zeros(n, dtype=np.float32)
    x = np.zeros(n)
    h = np.zeros(n, dtype=np.int64)
    pos = 0
    for i in range(NG):
        mine = np.sort(docs[pos:pos + sizes[i]])
        bad = docs[pos + sizes[i]:pos + sizes[i] + n_poison[i]]
        pos += sizes[i] + n_poison[i]
        group[mine] = group[bad] = i
        f[bad] = 99
        s[mine] = ZERO[i]
        sf[mine] = ZERO[i]
        picks = rng.permutation(mine)
        if k == 0:
            s[picks[:len(S[i])]] = S[i]
            sf[picks[:len(SF[i])]] = np.array(SF[i], dtype=np.float64).astype(np.float32)
            if S[i] and S[i][0] != S[i][0]:  # (astype need not keep a NaN's sign: write the bits)
                s.view(np.uint64)[picks[0]] = NAN_NEG if i == 0 else NAN_POS
                sf.view(np.uint32)[picks[0]] = F32_NAN_NEG if i == 0 else F32_NAN_POS
        s[bad], sf[bad] = s_poison(i)
        lo, hi, fill = X[i][0], X[i][1], X[i][2 + k]
        x[mine] = np.array(fill + [lo, hi])[rng.integers(0, len(fill) + 2, len(mine))]
        x[picks[2]], x[picks[3]] = lo, hi
        x[bad] = x_poison(i)
        h[mine] = 1000 * i + np.arange(len(mine)) % H[i]
        h[bad] = 1000 * i + 500 + 10 * k + np.arange(len(bad))
    assert pos == n
    g = np.array(G)[group]
    # A dictionary holds one zero, and which of two ``np.unique`` keeps depends on the doc order. Where the sign of a
    # stored zero can reach a result (the key gd; MIN / MAX of x, whose merge of two segments' zeros depends on their
    # order in the reference) both segments store -0.0 alone. x_r keeps both zeros, each alone in its group.
    gd = np.array(GD)[group]
    gd[gd == 0] = -0.0
    xd = x.copy()
    xd[xd == 0] = -0.0
    cols = {"g": (DataType.INT, g.astype(np.int32)), "gr": (DataType.INT, g.astype(np.int32)),
            "gd": (DataType.DOUBLE, gd), "f": (DataType.INT, f.astype(np.int32)),
            "s": (DataType.DOUBLE, s), "s_r": (DataType.DOUBLE, s.copy()), "sf": (DataType.FLOAT, sf),
            "x": (DataType.DOUBLE, xd), "x_r": (DataType.DOUBLE, x), "h": (DataType.INT, h.astype(np.int32))}
    return cols, group


RAW_COLUMNS = ("gr", "s_r", "x_r")


class OrderSegment:
    """One built segment, its source columns, the group of every doc and the stored values (from the index bytes)."""

    def __init__(self, k):
        self.source, self.group = build_columns(k)
        self.n = NUM_DOCS[k]
        c = SegmentCreator(f"order{k}", no_dictionary_columns=list(RAW_COLUMNS))
        for name, (dt, v) in self.source.items():
            c.add_column(name, dt, v)
        self.raw = c.build()
        self.matched = self.source["f"][1] < 99
        self._stored = {}

    def stored_values(self, col):
        """The column's stored values in doc order (float64 for FLOAT / DOUBLE: a FLOAT widens exactly)."""
        v = self._stored.get(col)
        if v is None:
            ci = self.raw.columns[col]
            m = ci.metadata
            if m.has_dictionary:
                d = np.frombuffer(ci.dictionary, dtype=m.data_type.numpy_be, count=m.cardinality).astype(m.data_type.numpy)
                assert not m.is_sorted
                bits = np.unpackbits(np.frombuffer(ci.forward, dtype=np.uint8))[:self.n * m.bits_per_element]
                w = 1 << np.arange(m.bits_per_element - 1, -1, -1, dtype=np.int64)  # (MSB first)
                v = d[bits.reshape(self.n, m.bits_per_element).astype(np.int64) @ w]
            else:
                v = read_chunk_forward(ci.forward, m.data_type, self.n)
            if v.dtype.kind == "f":
                v = v.astype(np.float64)
            self._stored[col] = v
        return v

    def docs(self, i, filtered):
        """The docs of group i in doc order: the matched ones, or all."""
        sel = self.group == i
        return np.nonzero(sel & self.matched if filtered else sel)[0]


@functools.lru_cache(maxsize=None)
def segments():
    return tuple(OrderSegment(k) for k in range(len(NUM_DOCS)))


# ---------------------------------------------------------------------------------------------- expected values
def _values(seg, col, i, filtered):
    return seg.stored_values(col)[seg.docs(i, filtered)].tolist()


def intermediate(function, col, i, seg_ids=(0, 1), filtered=True):
    """The intermediate result of ``function(col)`` for group i: per segment the reference's grouped fold in doc order,
    the segments merged in order with its merge. count -> int, sum / min / max -> float, avg -> (sum, count),
    minmaxrange -> (min, max), values -> the distinct values DISTINCTCOUNTHLL is offered."""
    segs = segments()
    if function == "count":
        return sum(len(segs[k].docs(i, filtered)) for k in seg_ids)
    parts = [_values(segs[k], col, i, filtered) for k in seg_ids]
    if function == "values":
        return sorted(set(v for p in parts for v in p))
    if function in ("sum", "avg"):
        total = 0.0
        for k, p in enumerate(parts):
            total = jf.seq_sum(p) if k == 0 else total + jf.seq_sum(p)
        return total if function == "sum" else (total, sum(len(p) for p in parts))
    if function == "min":
        return functools.reduce(jf.merge_min, [jf.group_min(p) for p in parts])
    if function == "max":
        return functools.reduce(jf.merge_max, [jf.group_max(p) for p in parts])
    if function == "minmaxrange":
        return functools.reduce(jf.merge_minmaxrange, [jf.minmaxrange(p) for p in parts])
    raise NotImplementedError(function)


def final(function, v):
    """extractFinalResult of the double-valued functions and COUNT."""
    if function == "avg":
        return v[0] / v[1] if v[1] else -INF
    if function == "minmaxrange":
        return v[1] - v[0]
    return v


def key_value(col, i):
    """Group i's value of a key column: G[i], or the stored gd (the same in every segment)."""
    if col in ("g", "gr"):
        return G[i]
    seg = segments()[0]
    return float(seg.stored_values(col)[seg.docs(i, False)[0]])


def hll_registers(values, log2m=8):
    """The HyperLogLog registers of INT ``values`` by the oracle's route (clearspring MurmurHash.hashLong +
    HyperLogLog.offerHashed, oracle/pinot_oracle.c)."""
    import oracle
    lib = oracle.lib()
    regs = np.zeros(1 << log2m, dtype=np.uint8)
    for v in values:
        lib.oracle_hll_offer_hashed(regs.ctypes.data, log2m, lib.oracle_murmur_hash_long(int(v)))
    return regs
