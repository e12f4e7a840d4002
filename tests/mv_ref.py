"""Multi-value test data and a numpy restatement of the reference's multi-value semantics (the oracle knows no
multi-value column).

Filters -- BaseDictionaryBasedPredicateEvaluator.applyMV (pinot-core/.../operator/filter/predicate/
BaseDictionaryBasedPredicateEvaluator.java:164-180): an inclusive predicate (EQ, IN, RANGE) matches a doc when ANY of
its values matches; an exclusive one (NOT_EQ, NOT_IN) when ALL of its values pass, i.e. when no value is in the excluded
set.

Aggregations, per matched doc: COUNTMV adds the row's length (CountMVAggregationFunction.aggregate), SUMMV the row's
values left to right in double (SumMVAggregationFunction.aggregate), MINMV / MAXMV take the row's extremes, AVGMV is
SUMMV / COUNTMV (AvgMVAggregationFunction: AvgPair(sum, count of values)), MINMAXRANGEMV is MAXMV - MINMV.
"""
import numpy as np

from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType

# column -> (stored type, values are drawn from [0, span), id width the dictionary then has)
MV_COLUMNS = {"m1": (DataType.INT, 2, 1), "m7": (DataType.LONG, 100, 7), "m12": (DataType.DOUBLE, 3000, 12),
              "m13": (DataType.INT, 6000, 13), "m17": (DataType.LONG, None, 17)}
LONG_ROW_DOC = 2047   # the last doc of tile 0: ~700 values, across several 64-value groups, up to the tile's end
HUGE_ROW_DOC = 3000   # m17 only: ~52 000 values (a dictionary above 2^16 ids; several 16 384-value passes of the scan)
SPECIAL_DOC = 1234    # span-2 occurs only as this doc's last value, span-1 only as the next doc's first


class MvSegment:
    def __init__(self, k, n, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        self.base = 1000 * k  # (different dictionaries per segment)
        lengths = rng.integers(1, 6, n)
        lengths[:16] = 4                  # doc 15 ends exactly on the first 64-value group boundary
        lengths[100:400] = 1              # a run of single-value docs
        lengths[LONG_ROW_DOC] = 700 + k
        self.sv = {"a": rng.integers(0, 50, n).astype(np.int32), "inv": rng.integers(0, 12, n).astype(np.int32),
                   "srt": np.sort(rng.integers(0, 40, n)).astype(np.int32), "k": rng.integers(0, 7, n).astype(np.int32),
                   "v": rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)}
        self.mv = {}
        for name, (dt, span, _) in MV_COLUMNS.items():
            ln = lengths.copy()
            if span is None:
                ln[HUGE_ROW_DOC] = 52000
            off = np.concatenate(([0], np.cumsum(ln))).astype(np.int64)
            total = int(off[-1])
            if span is None:
                vals = rng.permutation(total).astype(np.int64) * 3 + self.base  # all distinct
            else:
                vals = rng.integers(0, max(span - 2, 1) if span > 2 else span, total) + self.base
                if span > 2:
                    vals[off[SPECIAL_DOC + 1] - 1] = self.base + span - 2
                    vals[off[SPECIAL_DOC + 1]] = self.base + span - 1
            if dt == DataType.DOUBLE:
                vals = vals.astype(np.float64) * 0.5  # (halves: every sum below 2^52 is exact)
            else:
                vals = vals.astype(dt.numpy)
            self.mv[name] = (vals, off)

    def build(self, name):
        c = SegmentCreator(name, inverted_index_columns=["inv", "m7"])
        c.add_column("a", DataType.INT, self.sv["a"])
        c.add_column("inv", DataType.INT, self.sv["inv"])
        c.add_column("srt", DataType.INT, self.sv["srt"])
        c.add_column("k", DataType.INT, self.sv["k"])
        c.add_column("v", DataType.LONG, self.sv["v"])
        for col, (dt, _, _) in MV_COLUMNS.items():
            vals, off = self.mv[col]
            c.add_column(col, dt, [vals[off[d]:off[d + 1]] for d in range(self.n)], multi_value=True)
        return c.build()

    # ---- applyMV -------------------------------------------------------------------------------------------------
    def any_value(self, col, value_mask_fn):
        vals, off = self.mv[col]
        return np.logical_or.reduceat(value_mask_fn(vals), off[:-1])

    def eq(self, col, v):
        return self.any_value(col, lambda x: x == v)

    def isin(self, col, vs):
        return self.any_value(col, lambda x: np.isin(x, np.asarray(vs)))

    def between(self, col, lo, hi):
        return self.any_value(col, lambda x: (x >= lo) & (x <= hi))

    def not_in(self, col, vs):  # ALL values pass = no value in the excluded set
        return ~self.isin(col, vs)

    # ---- row reductions ------------------------------------------------------------------------------------------
    def length(self, col):
        return np.diff(self.mv[col][1])

    def row_sum(self, col):
        vals, off = self.mv[col]
        return np.add.reduceat(vals, off[:-1])  # (integers and halves: exact in any order)

    def row_min(self, col):
        vals, off = self.mv[col]
        return np.minimum.reduceat(vals, off[:-1]).astype(np.float64)

    def row_max(self, col):
        vals, off = self.mv[col]
        return np.maximum.reduceat(vals, off[:-1]).astype(np.float64)

    def intermediates(self, col, mask):
        """(countmv, summv, minmv, maxmv) over the docs of `mask` (min / max: +/-inf without a doc)."""
        ln, sm = self.length(col)[mask], self.row_sum(col)[mask]
        mn, mx = self.row_min(col)[mask], self.row_max(col)[mask]
        return (int(ln.sum()), sm.sum().item() if len(sm) else 0, float(mn.min()) if len(mn) else float("inf"),
                float(mx.max()) if len(mx) else float("-inf"))


def make_segments():
    return [MvSegment(0, 5000, 11), MvSegment(1, 5003, 12), MvSegment(2, 4999, 13)]


def combine(parts):
    """Merged (countmv, summv, minmv, maxmv) of per-segment intermediates."""
    return (sum(p[0] for p in parts), sum(p[1] for p in parts), min(p[2] for p in parts), max(p[3] for p in parts))


def finals(c, s, mn, mx):
    """{function: final result} of merged intermediates (AVGMV of no value: -inf, AvgAggregationFunction's default)."""
    return {"countmv": c, "summv": float(s), "minmv": mn, "maxmv": mx,
            "avgmv": float(s) / c if c else float("-inf"), "minmaxrangemv": mx - mn}
