"""SELECT DISTINCT test data and a numpy restatement of the GPU path's rule, independent of pinot_amd's planner.

The reference (DistinctOperator with the dictionary-based executors, DistinctCombineOperator, DistinctDataTableReducer)
returns `limit` distinct rows of the matched docs' projections, best under the ORDER BY; which of the rows that tie on
the order-by terms survive -- and, without ORDER BY, which `limit` rows at all -- follows the docs' arrival order. The
GPU path fixes the answer: rows ordered by the ORDER BY terms, then by the remaining select columns ascending in select
order; the first `limit` rows of the distinct set in that order. `distinct_rows` restates exactly that with np.unique
over the matched docs' value tuples.

Three segments of 5000 / 5003 / 4999 docs (three 2048-doc tiles each with a partial last tile). Every segment draws a
column's values from its own subset of the column's domain, so the per-segment dictionaries differ and the ids must be
remapped:
  a    INT     50 values
  s    STRING  12 values, every segment lacking two of them
  w    LONG    ~3000 values, negative ones among them
  d    DOUBLE  40 values, half of them negative
  u    INT     nearly unique per doc (a handful of duplicates, within and across segments)
  one  INT     one value
  srt  INT     40 values, sorted within the segment (a sorted-index column)
  inv  INT     12 values, with an inverted index
"""
import numpy as np

from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType

TYPES = {"a": "INT", "s": "STRING", "w": "LONG", "d": "DOUBLE", "u": "INT", "one": "INT", "srt": "INT", "inv": "INT"}
_DT = {"INT": DataType.INT, "LONG": DataType.LONG, "DOUBLE": DataType.DOUBLE, "STRING": DataType.STRING}
SIZES = (5000, 5003, 4999)


def _draw(rng, domain, absent, n):
    keep = np.array([v for i, v in enumerate(domain) if i not in absent], dtype=domain.dtype)
    return keep[rng.integers(0, len(keep), n)]


class Segment:
    def __init__(self, k, n, seed, u_values):
        rng = np.random.default_rng(seed)
        self.n = n
        s_dom = np.array([f"s{i:02d}" for i in range(12)], dtype=object)
        self.cols = {
            "a": _draw(rng, np.arange(50, dtype=np.int32), {k, k + 10}, n),
            "s": _draw(rng, s_dom, {k, k + 5}, n),
            "w": (rng.integers(0, 3000, n).astype(np.int64) - 1000) * 7919 * 1000003,
            "d": _draw(rng, (np.arange(40, dtype=np.float64) - 20) * 0.25, {2 * k, 2 * k + 21}, n),
            "u": u_values,
            "one": np.full(n, 7, dtype=np.int32),
            "srt": np.sort(_draw(rng, np.arange(40, dtype=np.int32), {3 * k + 1}, n)),
            "inv": rng.integers(0, 12, n).astype(np.int32),
        }

    def build(self, name):
        c = SegmentCreator(name, inverted_index_columns=["inv"])
        for col, vals in self.cols.items():
            c.add_column(col, _DT[TYPES[col]], vals)
        return c.build()


def make_segments():
    rng = np.random.default_rng(77)
    total = sum(SIZES)
    u = rng.permutation(total).astype(np.int32) * 3 - 20000
    dup = rng.integers(0, total, 12)  # a handful of duplicates, wherever they fall
    u[dup] = u[(dup + 4321) % total]
    out, at = [], 0
    for k, n in enumerate(SIZES):
        out.append(Segment(k, n, 100 + k, u[at:at + n].copy()))
        at += n
    return out


def column(segs, col):
    """The column over all segments, in query order."""
    vals = [s.cols[col] for s in segs]
    return np.concatenate(vals) if TYPES[col] != "STRING" else np.concatenate([np.asarray(v, dtype=object) for v in vals])


def _codes(segs, col):
    """(sorted distinct values of the column over every doc of the query, each doc's index into them): the index order
    is the value order (strings: code points = UTF-8 bytes for this ASCII data)."""
    v = column(segs, col)
    if TYPES[col] == "STRING":
        v = v.astype(str)
    uniq, inv = np.unique(v, return_inverse=True)
    return uniq, inv.astype(np.int64)


def cardinalities(segs, cols):
    return [len(_codes(segs, c)[0]) for c in cols]


def _py(col, v):
    t = TYPES[col]
    return str(v) if t == "STRING" else (float(v) if t == "DOUBLE" else int(v))


def distinct_rows(segs, cols, mask, order=(), limit=10):
    """The rule: np.unique over the matched docs' value tuples, ordered by the ORDER BY terms (``order``: [(column,
    descending)]) and then by the remaining columns ascending in select order; the first ``limit`` rows, as tuples of
    Python values in select order. ``mask``: the matched docs over all segments (bool, query order)."""
    uniqs, codes = zip(*(_codes(segs, c) for c in cols))
    ranked = [c for c, _ in order] + [c for c in cols if c not in [o for o, _ in order]]
    desc = dict(order)
    mat = np.stack([(-codes[cols.index(c)] if desc.get(c) else codes[cols.index(c)])[mask] for c in ranked], axis=1)
    rows = np.unique(mat, axis=0)[:limit] if mat.shape[0] else mat[:0]  # (lexicographic: first column most significant)
    out = []
    for r in rows:
        by_col = {c: (-x if desc.get(c) else x) for c, x in zip(ranked, r.tolist())}
        out.append(tuple(_py(c, uniqs[cols.index(c)][by_col[c]]) for c in cols))
    return out


def keys(segs, cols, mask, order=()):
    """The matched docs' distinct keys under the layout the library documents (include/pinot_hip.h select_distinct):
    mixed radix over the columns' ranks among the query's values, a descending term's digit complemented, the ORDER BY
    terms most significant, the other columns after them in select order. Ascending."""
    ranked = [c for c, _ in order] + [c for c in cols if c not in [o for o, _ in order]]
    desc = dict(order)
    key = np.zeros(int(mask.sum()), dtype=np.int64)
    for c in ranked:
        uniq, code = _codes(segs, c)
        digit = code[mask]
        key = key * len(uniq) + (len(uniq) - 1 - digit if desc.get(c) else digit)
    return np.unique(key)


def true_distinct_set(segs, cols, mask):
    """Every distinct row of the matched docs, as a Python set of value tuples (no ordering involved)."""
    vals = [column(segs, c)[mask] for c in cols]
    return {tuple(_py(c, v) for c, v in zip(cols, row)) for row in zip(*vals)}


def top_projections(segs, cols, mask, order, limit):
    """The order-by projections of the reference's answer: the distinct rows' projections onto the ORDER BY columns,
    sorted by the terms, the first ``limit`` (as a multiset the reference's answer has exactly these, whichever tying
    rows it kept). Without ORDER BY: None (any ``limit`` distinct rows are an answer)."""
    if not order:
        return None
    rows = list(true_distinct_set(segs, cols, mask))
    for c, d in reversed(list(order)):
        rows.sort(key=lambda r: r[cols.index(c)], reverse=bool(d))
    return [tuple(r[cols.index(c)] for c, _ in order) for r in rows[:limit]]
