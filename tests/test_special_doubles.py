"""NaN, infinite, signed-zero, denormal and DBL_MAX metrics: the reference's folds (tests/java_fold.py) on hand-written
vectors, the host merges and the oracle against them, and the proof that the SUM inputs of the GPU matrix
(tests/test_gpu_special_doubles.py) are order-free. No GPU.

The segments of the matrix are built here (``special_segments``) and shared with the GPU test. Their stored values are
read back from the index bytes (``stored_values``: dictionary + fixed-bit forward index, or the raw chunks), because a
dictionary holds one entry per ``np.unique`` value: every NaN of a column is one entry and -0.0 / 0.0 are one entry,
whichever bits the builder kept. Expected values are folds of the *stored* values of the matched docs in doc order.
"""
import functools
import math
import struct

import numpy as np
import pytest

from oracle import executor
from pinot_amd.engine.results import merge_intermediate
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType
from tests import java_fold as jf

NAN = float("nan")
INF = float("inf")
TILE = 2048
N1 = TILE * 5 + 77   # five full tiles and a ragged one
N2 = TILE * 2 + 5    # the second segment (other dictionaries)
NAN_POS = 0x7FF8000000000000
NAN_NEG = 0xFFF8000000000000
DBL_MAX = 1.7976931348623157e308


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ------------------------------------------------------------------------------ the folds on hand-written vectors
def test_same_double():
    assert jf.same_double(NAN, NAN, True) and jf.same_double(NAN, -NAN, True)
    assert not jf.same_double(NAN, 1.0, False) and not jf.same_double(1.0, NAN, False)
    assert jf.same_double(-0.0, 0.0, False) and not jf.same_double(-0.0, 0.0, True)
    assert jf.same_double(0.0, 0.0, True) and jf.same_double(-0.0, -0.0, True)
    assert jf.same_double(INF, INF, True) and not jf.same_double(INF, -INF, False)
    assert not jf.same_double(1.0, 1.0000000000000002, False)


@pytest.mark.parametrize("vals,mn,mx", [
    ([NAN, 1.0], NAN, NAN),            # Math.min / Math.max: NaN if either operand is NaN
    ([1.0, NAN], NAN, NAN),
    ([-0.0, 0.0], -0.0, 0.0),          # -0.0 is the smaller zero, in either order
    ([0.0, -0.0], -0.0, 0.0),
    ([3.0, -INF, INF, 2.0], -INF, INF),
    ([], INF, -INF),                   # the holder defaults
    ([5e-324, -5e-324, 0.0], -5e-324, 5e-324),
])
def test_math_min_max_fold(vals, mn, mx):
    assert jf.same_double(jf.fold_min(vals), mn, True)
    assert jf.same_double(jf.fold_max(vals), mx, True)


@pytest.mark.parametrize("vals,mn,mx", [
    ([NAN, 1.0], 1.0, 1.0),            # value < holder / value > holder: a NaN never wins
    ([1.0, NAN], 1.0, 1.0),
    ([NAN, NAN], INF, -INF),           # ... and leaves the holder defaults
    ([-0.0, 0.0], -0.0, -0.0),         # of two zeros the first seen stays
    ([0.0, -0.0], 0.0, 0.0),
    ([2.0, -INF, INF, NAN], -INF, INF),
    ([], INF, -INF),
])
def test_compare_fold_grouped_and_minmaxrange(vals, mn, mx):
    assert jf.same_double(jf.group_min(vals), mn, True)
    assert jf.same_double(jf.group_max(vals), mx, True)
    lo, hi = jf.minmaxrange(vals)      # MinMaxRangePair.apply compares at both ends, grouped or not
    assert jf.same_double(lo, mn, True) and jf.same_double(hi, mx, True)


@pytest.mark.parametrize("a,b,mn,mx", [
    (NAN, 1.0, 1.0, 1.0),              # merge(NaN, x) = x
    (1.0, NAN, NAN, NAN),              # merge(x, NaN) = NaN
    (-0.0, 0.0, 0.0, 0.0),             # r1 < r2 is false for the two zeros: r2 is returned
    (0.0, -0.0, -0.0, -0.0),
    (2.0, 3.0, 2.0, 3.0),
    (INF, -INF, -INF, INF),
])
def test_less_than_merge(a, b, mn, mx):
    assert jf.same_double(jf.merge_min(a, b), mn, True)
    assert jf.same_double(jf.merge_max(a, b), mx, True)


def test_minmaxrange_merge_keeps_the_running_pair():
    assert jf.merge_minmaxrange((1.0, 2.0), (NAN, NAN)) == (1.0, 2.0)
    lo, hi = jf.merge_minmaxrange((NAN, NAN), (1.0, 2.0))   # a NaN end is never replaced: nothing compares beyond it
    assert math.isnan(lo) and math.isnan(hi)
    lo, hi = jf.merge_minmaxrange((-0.0, -0.0), (0.0, 0.0))
    assert jf.same_double(lo, -0.0, True) and jf.same_double(hi, -0.0, True)
    assert jf.merge_minmaxrange((1.0, 5.0), (0.5, 4.0)) == (0.5, 5.0)


def test_sequential_sum_and_avg():
    assert jf.seq_sum([]) == 0.0 and jf.avg([]) == (0.0, 0)
    assert math.isnan(jf.seq_sum([1.0, NAN])) and math.isnan(jf.seq_sum([INF, -INF]))
    assert jf.seq_sum([DBL_MAX, DBL_MAX / 2]) == INF
    assert jf.same_double(jf.seq_sum([-0.0, -0.0]), 0.0, True)   # the sum starts from +0.0
    assert jf.seq_sum([5e-324] * 3) == 1.5e-323                  # denormals add exactly
    assert jf.avg([1.0, 2.0, 4.5]) == (7.5, 3)
    assert jf.tree_sum([1.0, 2.0, 3.0, 4.0, 5.0]) == 15.0 and jf.tree_sum([]) == 0.0


# ------------------------------------------------------------------------------ host merges
_MERGE_PAIRS = [(NAN, 1.5), (1.5, NAN), (-0.0, 0.0), (0.0, -0.0), (2.0, 3.0), (3.0, 2.0), (INF, -INF), (NAN, NAN)]


@pytest.mark.parametrize("a,b", _MERGE_PAIRS)
def test_merge_intermediate_is_the_less_than_merge(a, b):
    """results.merge_intermediate(function, a, b): a is the running result (the reference's intermediateResult1)."""
    assert jf.same_double(merge_intermediate("min", a, b), jf.merge_min(a, b), True)
    assert jf.same_double(merge_intermediate("max", a, b), jf.merge_max(a, b), True)
    for pa, pb in (((a, a), (b, b)), ((a, 7.0), (b, 9.0)), ((-7.0, a), (-9.0, b))):
        got, want = merge_intermediate("minmaxrange", pa, pb), jf.merge_minmaxrange(pa, pb)
        assert jf.same_double(got[0], want[0], True) and jf.same_double(got[1], want[1], True)


def _case_operator(sql):
    """A GpuCaseAggregationOperator's fold without its inner GPU operators (the fold reads only ``plan``)."""
    from pinot_amd.engine import plan as gplan
    made = {}

    class _Inner:
        def __init__(self, query, segments, num_groups_limit, stats_filters=None):
            made["inner_query"] = query

    saved = gplan.GpuFilteredAggregationOperator
    gplan.GpuFilteredAggregationOperator = _Inner
    try:
        op = gplan.GpuCaseAggregationOperator(parse(sql), [], 0)
    finally:
        gplan.GpuFilteredAggregationOperator = saved
    return op, made["inner_query"]


@pytest.mark.parametrize("a,b", _MERGE_PAIRS)
def test_case_fold_expression_branches_merge_in_branch_order(a, b):
    """plan._fold, expression branches: the branch results merge like intermediates, the first branch the running
    result from the holder defaults (+inf / -inf)."""
    op, inner = _case_operator(
        "SELECT MIN(CASE WHEN f < 5 THEN x ELSE y END), MAX(CASE WHEN f < 5 THEN x ELSE y END), "
        "MINMAXRANGE(CASE WHEN f < 5 THEN x ELSE y END) FROM t")
    vals = [None] * len(inner.aggregations)
    for i, ag in enumerate(inner.aggregations):
        first = "x" in str(ag.argument) if ag.argument is not None else None
        if ag.function == "count":
            vals[i] = 3
        elif ag.function == "minmaxrange":
            vals[i] = (a, a) if first else (b, b)
        else:
            vals[i] = a if first else b
    mn, mx, (lo, hi) = op._fold(vals)
    want_mn = jf.merge_min(jf.merge_min(INF, a), b)
    want_mx = jf.merge_max(jf.merge_max(-INF, a), b)
    want_pair = jf.merge_minmaxrange(jf.merge_minmaxrange((INF, -INF), (a, a)), (b, b))
    assert jf.same_double(mn, want_mn, True) and jf.same_double(mx, want_mx, True)
    assert jf.same_double(lo, want_pair[0], True) and jf.same_double(hi, want_pair[1], True)


@pytest.mark.parametrize("a,b", [(-0.0, 0.0), (0.0, -0.0), (2.0, 3.0), (3.0, 2.0)])
def test_case_fold_literal_branches(a, b):
    """plan._fold, literal branches: a literal whose branch has docs merges as a value; one without docs does not."""
    sql = f"SELECT MIN(CASE WHEN f < 5 THEN {a!r} ELSE {b!r} END), MAX(CASE WHEN f < 5 THEN {a!r} ELSE {b!r} END) FROM t"
    op, inner = _case_operator(sql)
    lits = [x for p in op.plan for kind, x, s in p[2] if kind == "lit"]
    assert [jf.same_double(x, y, True) for x, y in zip(lits, (a, b, a, b))] == [True] * 4, "the parser keeps the sign"
    mn, mx = op._fold([4] * len(inner.aggregations))
    assert jf.same_double(mn, jf.merge_min(jf.merge_min(INF, a), b), True)
    assert jf.same_double(mx, jf.merge_max(jf.merge_max(-INF, a), b), True)
    mn, mx = op._fold([0] * len(inner.aggregations))
    assert mn == INF and mx == -INF


# ------------------------------------------------------------------------------ the matrix's segments
def _placements(rng, n):
    """(P1 docs, P2 docs): per tile a few docs for each; P2 always holds doc 0 and the last doc."""
    p1, p2 = [], [0, n - 1]
    for lo in range(0, n, TILE):
        hi = min(n, lo + TILE)
        docs = rng.permutation(np.arange(lo, hi))
        docs = docs[(docs != 0) & (docs != n - 1)]
        k2 = min(3, len(docs) // 4)
        k1 = min(4, max(1, len(docs) // 4))
        p2.extend(docs[:k2].tolist())
        p1.extend(docs[k2:k2 + k1].tolist())
    return np.array(sorted(p1)), np.array(sorted(set(p2)))


def _f64_from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def build_special_columns(seed, n, shift):
    """{name: (DataType, source values)} of one segment, and its placements. ``shift`` moves the finite values, so
    that two segments' dictionaries differ."""
    rng = np.random.default_rng(seed)
    p1, p2 = _placements(rng, n)
    f = rng.integers(3, 99, n)
    sparse = rng.random(n) < 0.03                   # ~3 % sparse matches of f < 3
    f[sparse] = rng.integers(0, 3, int(sparse.sum()))
    f[p1] = 1                                       # P1 docs match every filter
    f[p2] = 99                                      # P2 docs match none; f < 99 excludes exactly them
    g = rng.integers(0, 7, n)
    g[p1[:7]] = np.arange(7)[:len(p1[:7])]
    a = np.array([0, 1, 2, -1])[rng.integers(0, 4, n)]
    g3 = np.nonzero(g == 3)[0]
    p3 = g3[::3]                                    # P3: docs of group 3 only
    cols = {"f": (DataType.INT, f.astype(np.int32)), "g": (DataType.INT, g.astype(np.int32)),
            "gr": (DataType.INT, g.astype(np.int32)), "a": (DataType.INT, a.astype(np.int32))}

    def finite():
        return rng.integers(-4000, 4000, n) * 0.25 + shift

    def put(name, dt, vals):
        cols[name] = (dt, vals)
        cols[name + "_r"] = (dt, vals.copy())

    for pname, docs in (("p1", p1), ("p2", p2), ("p3", p3)):
        for name, fname, bits64, bits32 in (("dn", "fn", NAN_POS, 0x7FC00000), ("dm", "fm", NAN_NEG, 0xFFC00000)):
            v = finite()
            v.view(np.uint64)[docs] = bits64
            put(f"{name}_{pname}", DataType.DOUBLE, v)
            v32 = finite().astype(np.float32)
            v32.view(np.uint32)[docs] = bits32
            put(f"{fname}_{pname}", DataType.FLOAT, v32)
        inf = np.where(np.arange(len(docs)) % 2 == 0, INF, -INF)
        v = finite()
        v[docs] = inf
        put(f"di_{pname}", DataType.DOUBLE, v)
        v32 = finite().astype(np.float32)
        v32[docs] = inf.astype(np.float32)
        put(f"fi_{pname}", DataType.FLOAT, v32)
        zeros = rng.random(n) < 0.05
        v = np.abs(finite()) + 0.25
        v[zeros] = 0.0
        v[docs] = -0.0
        put(f"dz_{pname}", DataType.DOUBLE, v)
        v = -(np.abs(finite()) + 0.25)
        v[zeros] = 0.0
        v[docs] = -0.0
        put(f"dzn_{pname}", DataType.DOUBLE, v)
    v = finite()
    v[p1] = INF
    put("dp", DataType.DOUBLE, v)
    k = rng.integers(-1000, 1001, n)
    k[rng.random(n) < 0.05] = 0
    sign = (k < 0).astype(np.uint64)
    put("dd", DataType.DOUBLE, _f64_from_bits(np.abs(k).astype(np.uint64) | (sign << np.uint64(63))).copy())
    put("fd", DataType.FLOAT, (np.abs(k).astype(np.uint32) | (sign.astype(np.uint32) << np.uint32(31))).view(np.float32).copy())
    big = rng.integers(0, 4, n)
    v = np.where(big == 0, DBL_MAX, np.where(big == 1, DBL_MAX / 2, rng.integers(1, 4000, n) * 0.25 + abs(shift)))
    put("dh", DataType.DOUBLE, v)
    put("dhn", DataType.DOUBLE, -v)
    return cols, {"p1": p1, "p2": p2, "p3": p3}


class SpecialSegment:
    """One built segment of the matrix, its source columns and its stored values (read from the index bytes)."""

    def __init__(self, name, seed, n, shift):
        self.source, self.placements = build_special_columns(seed, n, shift)
        self.n = n
        c = SegmentCreator(name, no_dictionary_columns=[k for k in self.source if k.endswith("_r")] + ["gr"])
        for k, (dt, v) in self.source.items():
            c.add_column(k, dt, v)
        self.raw = c.build()
        self._stored = {}

    def stored_bits(self, col):
        """The column's stored values in doc order, in their own width (float32 / float64 arrays)."""
        v = self._stored.get(col)
        if v is None:
            ci = self.raw.columns[col]
            m = ci.metadata
            be = m.data_type.numpy_be
            if m.has_dictionary:
                d = np.frombuffer(ci.dictionary, dtype=be, count=m.cardinality).astype(m.data_type.numpy)
                assert not m.is_sorted
                bits = np.unpackbits(np.frombuffer(ci.forward, dtype=np.uint8))[:self.n * m.bits_per_element]
                w = 1 << np.arange(m.bits_per_element - 1, -1, -1, dtype=np.int64)  # (MSB first)
                v = d[bits.reshape(self.n, m.bits_per_element).astype(np.int64) @ w]
            else:  # PASS_THROUGH chunks lie back to back behind the header and the chunk offsets
                hdr = np.frombuffer(ci.forward, dtype=">i4", count=7)
                assert hdr[0] == 3 and hdr[5] == 0 and hdr[4] == self.n
                v = np.frombuffer(ci.forward, dtype=be, count=self.n, offset=28 + 8 * int(hdr[1])).astype(m.data_type.numpy)
            self._stored[col] = v
        return v

    def stored_values(self, col):
        """... as Python floats (a FLOAT widens exactly, as the reference's getDoubleValuesSV does)."""
        return self.stored_bits(col).astype(np.float64)

    def dictionary(self, col):
        ci = self.raw.columns[col]
        m = ci.metadata
        return np.frombuffer(ci.dictionary, dtype=m.data_type.numpy_be, count=m.cardinality).astype(m.data_type.numpy)


@functools.lru_cache(maxsize=None)
def special_segments():
    return (SpecialSegment("special0", 20261, N1, 0.0), SpecialSegment("special1", 20262, N2, 1000.5))


FILTERS = {"sparse": "f < 3", "dense": "f < 90", "not_p2": "f < 99"}
PLACED = ("dn", "dm", "fn", "fm", "di", "fi", "dz", "dzn")
NAN_KINDS = ("dn", "dm", "fn", "fm")
METRICS = tuple(f"{k}_{p}{r}" for k in PLACED for p in ("p1", "p2", "p3") for r in ("", "_r")) + \
    tuple(f"{k}{r}" for k in ("dp", "dd", "fd", "dh", "dhn") for r in ("", "_r"))
EXPRESSIONS = ("SUM(a * di_p1)", "SUM(di_p1 - di_p1)", "SUM(a * di_p1_r)", "SUM(di_p1_r - di_p1_r)")


def holds_nan(col):
    return col.split("_")[0] in NAN_KINDS


def matched(seg, flt):
    f = seg.source["f"][1]
    return f < int(FILTERS[flt].split("<")[1]) if flt is not None else np.ones(seg.n, dtype=bool)


def _expr_values(seg, expr):
    """Doc-order double values of a metric column or of one of EXPRESSIONS' arguments."""
    if "(" not in expr:
        return seg.stored_values(expr)
    arg = expr[expr.index("(") + 1:-1]
    for op in (" * ", " - "):
        if op in arg:
            x, y = arg.split(op)
            vx = seg.source[x][1].astype(np.float64) if x == "a" else seg.stored_values(x)
            vy = seg.stored_values(y)
            with np.errstate(invalid="ignore"):
                return vx * vy if op == " * " else vx - vy
    raise ValueError(expr)


@functools.lru_cache(maxsize=None)
def expected(seg_index, col, flt, grouped):
    """The folds of one column (or expression) over the docs ``flt`` matches in one segment: a dict of
    min / max / minmaxrange / sum / count, or {group: that dict} when ``grouped``. Non-grouped MIN / MAX are the
    Math.min / Math.max fold, grouped ones and MINMAXRANGE the compare fold."""
    seg = special_segments()[seg_index]
    m = matched(seg, flt)
    vals = _expr_values(seg, col)
    g = seg.source["g"][1]

    def cell(v, nongrouped):
        v = v.tolist()
        return {"min": jf.fold_min(v) if nongrouped else jf.group_min(v),
                "max": jf.fold_max(v) if nongrouped else jf.group_max(v),
                "minmaxrange": jf.minmaxrange(v), "sum": jf.seq_sum(v), "count": len(v)}

    if not grouped:
        return cell(vals[m], True)
    return {int(k): cell(vals[m & (g == k)], False) for k in np.unique(g[m]).tolist()}


def merged_expected(col, flt, grouped):
    """Both segments: per-segment folds merged in segment order with the reference's merges."""
    def merge(x, y):
        return {"min": jf.merge_min(x["min"], y["min"]), "max": jf.merge_max(x["max"], y["max"]),
                "minmaxrange": jf.merge_minmaxrange(x["minmaxrange"], y["minmaxrange"]),
                "sum": x["sum"] + y["sum"], "count": x["count"] + y["count"]}
    e0, e1 = expected(0, col, flt, grouped), expected(1, col, flt, grouped)
    if not grouped:
        return merge(e0, e1)
    out = dict(e0)
    for k, v in e1.items():
        out[k] = merge(out[k], v) if k in out else v
    return out


# ------------------------------------------------------------------------------ what the built segments hold
def test_placements_and_stored_bits():
    for seg in special_segments():
        p = seg.placements
        f, g = seg.source["f"][1], seg.source["g"][1]
        assert 0 in p["p2"] and seg.n - 1 in p["p2"]
        assert np.array_equal(np.nonzero(f == 99)[0], p["p2"]) and not (f > 99).any()  # f < 99 excludes exactly P2
        assert (f[p["p1"]] < 3).all() and set(g[p["p3"]].tolist()) == {3}
        for lo in range(0, seg.n, TILE):  # every tile holds P1 docs and sparse matches
            assert ((p["p1"] >= lo) & (p["p1"] < lo + TILE)).any()
        assert ((f < 3) & (g == 3) & np.isin(np.arange(seg.n), p["p3"])).any()
        for col in METRICS:
            src = seg.source[col][1]
            st = seg.stored_bits(col)
            u = np.uint64 if st.dtype == np.float64 else np.uint32
            if col.endswith("_r"):  # raw columns keep the source's bits: both NaN patterns, both zeros
                assert np.array_equal(st.view(u), src.view(u)), col
                continue
            # a dictionary holds one entry per np.unique value: values equal, but one NaN pattern and one zero
            assert np.array_equal(st, src, equal_nan=True), col
            d = seg.dictionary(col)
            if holds_nan(col):
                assert np.isnan(d[-1]) and not np.isnan(d[:-1]).any(), col  # one NaN entry, the last
                want = {"dn": NAN_POS, "dm": NAN_NEG, "fn": 0x7FC00000, "fm": 0xFFC00000}[col.split("_")[0]]
                assert int(d.view(u)[-1]) == want, (col, hex(int(d.view(u)[-1])))
                assert (np.isnan(st) == np.isnan(src)).all()
            if col.startswith("dz"):
                assert (d == 0).sum() == 1, col  # -0.0 and 0.0 share one entry; expected values follow its sign
    s0, s1 = special_segments()
    assert not np.array_equal(s0.dictionary("dp"), s1.dictionary("dp")[:len(s0.dictionary("dp"))])


# ------------------------------------------------------------------------------ SUM inputs are order-free
def _sum_cells():
    for si in (0, 1):
        seg = special_segments()[si]
        g = seg.source["g"][1]
        for col in METRICS + EXPRESSIONS:
            vals = _expr_values(seg, col)
            for flt in FILTERS:
                m = matched(seg, flt)
                yield (si, col, flt, None), vals[m]
                for k in range(7):
                    yield (si, col, flt, k), vals[m & (g == k)]
    # both segments as one cell: the GPU path adds the two segments' docs in no fixed order either
    s0, s1 = special_segments()
    g0, g1 = s0.source["g"][1], s1.source["g"][1]
    for col in METRICS + EXPRESSIONS:
        v0, v1 = _expr_values(s0, col), _expr_values(s1, col)
        for flt in FILTERS:
            m0, m1 = matched(s0, flt), matched(s1, flt)
            yield ("both", col, flt, None), np.concatenate([v0[m0], v1[m1]])
            for k in range(7):
                yield ("both", col, flt, k), np.concatenate([v0[m0 & (g0 == k)], v1[m1 & (g1 == k)]])


def test_sum_inputs_are_order_free():
    """Every SUM / AVG cell of the matrix folds to the same double forwards, backwards and as a pairwise tree (or to
    NaN all three ways): what lets the GPU test compare sums without a tolerance."""
    bad = []
    for cell, v in _sum_cells():
        v = v.tolist()
        fw, bw, tr = jf.seq_sum(v), jf.seq_sum(v[::-1]), jf.tree_sum(v)
        if all(math.isnan(x) for x in (fw, bw, tr)):
            continue
        if not (_bits(fw) == _bits(bw) == _bits(tr)):
            bad.append((cell, fw, bw, tr))
    assert not bad, bad[:10]


def test_sum_cells_pin_what_they_are_for():
    """dd sums are denormal (a flushed input changes them), dh sums overflow, NaN and inf - inf cells are NaN."""
    for flt in FILTERS:
        for r in ("", "_r"):
            e = expected(0, "dd" + r, flt, False)
            assert e["sum"] != 0.0 and abs(e["sum"]) < 2.3e-308
            assert 0.0 < abs(expected(0, "fd" + r, flt, False)["sum"]) < 1.2e-38
            assert expected(0, "dh" + r, flt, False)["sum"] == INF and expected(0, "dhn" + r, flt, False)["sum"] == -INF
            assert all(c["sum"] == INF for c in expected(0, "dh" + r, flt, True).values())
            assert math.isnan(expected(0, "dn_p1" + r, flt, False)["sum"])
            assert not math.isnan(expected(0, "dn_p2" + r, flt, False)["sum"])
            assert math.isnan(expected(0, f"SUM(a * di_p1{r})", flt, False)["sum"])
            assert math.isnan(expected(0, f"SUM(di_p1{r} - di_p1{r})", flt, False)["sum"])
            grp = expected(0, "dn_p3" + r, flt, True)
            assert [k for k, c in grp.items() if math.isnan(c["sum"])] == [3]


# ------------------------------------------------------------------------------ the oracle equals the folds
def check_block(qc, blk, want, grouped, sign_matters, where):
    """Failures (strings) of a results block against ``want`` (``expected`` / ``merged_expected`` per aggregation
    argument). MIN / MAX / MINMAXRANGE by same_double, sums bit-exact or NaN to NaN, counts exact."""
    bad = []

    def one(ag, got, e, at):
        f = ag.function
        if f == "count":
            ok = got == e["count"]
        elif f in ("min", "max"):
            ok = jf.same_double(got, e[f], sign_matters)
        elif f == "minmaxrange":
            ok = jf.same_double(got[0], e[f][0], False) and jf.same_double(got[1], e[f][1], False)
        else:
            s = got[0] if f == "avg" else got
            ok = (math.isnan(s) and math.isnan(e["sum"])) or _bits(float(s)) == _bits(e["sum"])
            ok = ok and (f != "avg" or got[1] == e["count"])
        if not ok:
            bad.append(f"{where} {at}{ag.function}({ag.argument}): got {got!r}, want "
                       f"{e['count'] if f == 'count' else e['sum'] if f in ('sum', 'avg') else e[f]!r}")

    if not grouped:
        for ag, got, w in zip(qc.aggregations, blk.results, want):
            one(ag, got, w, "")
        return bad
    keys = set(want[0]) if want else set()
    if {k[0] for k in blk.groups} != keys:
        return [f"{where}: groups {sorted(k[0] for k in blk.groups)}, want {sorted(keys)}"]
    for k, row in blk.groups.items():
        for ag, got, w in zip(qc.aggregations, row, want):
            one(ag, got, w[k[0]], f"g={k[0]} ")
    return bad


def queries_for(col, flt, key=None):
    """The two queries of a metric column: the compare / Math.min functions, and the sums."""
    where = f" WHERE {FILTERS[flt]}" if flt else ""
    head, tail = (f"SELECT {key}, ", f" GROUP BY {key} LIMIT 100") if key else ("SELECT ", "")
    return (f"{head}MIN({col}), MAX({col}), MINMAXRANGE({col}), COUNT(*) FROM t{where}{tail}",
            f"{head}SUM({col}), AVG({col}), COUNT(*) FROM t{where}{tail}")


def expression_query(expr, flt, key=None):
    head, tail = (f"SELECT {key}, ", f" GROUP BY {key} LIMIT 100") if key else ("SELECT ", "")
    return f"{head}{expr}, COUNT(*) FROM t WHERE {FILTERS[flt]}{tail}"


def wants(qc, col, flt, grouped, segs=(0,)):
    e = expected(segs[0], col, flt, grouped) if len(segs) == 1 else merged_expected(col, flt, grouped)
    return [e] * len(qc.aggregations)


@pytest.mark.parametrize("key", [None, "g", "gr"])
@pytest.mark.parametrize("flt", list(FILTERS))
def test_oracle_equals_the_folds(flt, key):
    """executor.execute on one segment against the folds, every function of every column of the matrix. The sign of
    a zero counts where the reference's result does not depend on the order of the docs' blocks: non-grouped MIN / MAX
    (Math.min / Math.max); the oracle's grouped zeros are the first seen too, and are checked as such."""
    seg = special_segments()[0]
    bad = []
    for col in METRICS:
        for sql in queries_for(col, flt, key):
            qc = parse(sql)
            blk, _ = executor.execute(qc, [seg.raw])
            assert blk.stats.num_docs_scanned == int(matched(seg, flt).sum())
            bad += check_block(qc, blk, wants(qc, col, flt, bool(key)), bool(key), True, sql)
    for expr in EXPRESSIONS + ("MAX(a * dp)", "MAX(a * dp_r)"):
        qc = parse(expression_query(expr, flt, key))
        blk, _ = executor.execute(qc, [seg.raw])
        bad += check_block(qc, blk, wants(qc, expr, flt, bool(key)), bool(key), True, expr)
    assert not bad, f"{len(bad)} cells: " + "; ".join(bad[:12])


def test_oracle_filter_clause_and_two_segment_merge():
    s0, s1 = special_segments()
    qc = parse("SELECT MIN(dn_p1) FILTER (WHERE f < 50), MAX(dn_p1) FILTER (WHERE f >= 50) FROM t")
    blk, _ = executor.execute(qc, [s0.raw])
    f, v = s0.source["f"][1], s0.stored_values("dn_p1")
    assert jf.same_double(blk.results[0], jf.fold_min(v[f < 50].tolist()), True) and math.isnan(blk.results[0])
    assert jf.same_double(blk.results[1], jf.fold_max(v[f >= 50].tolist()), True) and not math.isnan(blk.results[1])
    for col in ("di_p1", "dp_r", "dd", "dh_r", "dhn", "dz_p2", "dn_p2_r", "dn_p1"):
        for key in (None, "g"):
            for sql in queries_for(col, "dense", key):
                qc = parse(sql)
                blk, _ = executor.execute(qc, [s0.raw, s1.raw])
                bad = check_block(qc, blk, wants(qc, col, "dense", bool(key), (0, 1)), bool(key), False, sql)
                assert not bad, bad


# ------------------------------------------------------------------------------ the plan-time NaN decision (host side)
def _host_segment(raw):
    """A GpuSegment's host-side readers over ``raw`` without loading it onto a device."""
    from pinot_amd.engine.segment import GpuSegment
    s = GpuSegment.__new__(GpuSegment)
    s.segment, s.name, s.num_docs, s.handle = raw, raw.name, raw.num_docs, 0
    s._dicts, s._sorted, s._inv_offsets, s._specials = {}, {}, {}, {}
    s.star_trees, s.star_segments = [], []
    return s


def test_segment_flags_of_nan_and_infinity():
    for seg in special_segments():
        host = _host_segment(seg.raw)
        for col in METRICS:
            src = seg.source[col][1]
            assert host.real_specials(col) == (bool(np.isnan(src).any()), bool(np.isinf(src).any())), col
        assert host.real_specials("f") == (False, False) and host.real_specials("gr") == (False, False)


@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("compression", ["PASS_THROUGH", "SNAPPY", "ZSTANDARD", "LZ4", "LZ4_LENGTH_PREFIXED", "GZIP"])
def test_raw_chunk_flags_through_every_codec(compression, version):
    from pinot_amd.segment.creator import read_chunk_forward
    rng = np.random.default_rng(5)
    n = 2500
    d = rng.integers(-50, 50, n) * 0.5
    d.view(np.uint64)[[7, 2499]] = NAN_NEG
    fl = (rng.integers(-50, 50, n) * 0.5).astype(np.float32)
    fl[1234] = -INF
    plain = rng.integers(-50, 50, n) * 0.5
    c = SegmentCreator("codec", no_dictionary_columns=["d", "fl", "plain"], raw_version=version,
                       raw_compression={k: compression for k in ("d", "fl", "plain")})
    c.add_column("d", DataType.DOUBLE, d).add_column("fl", DataType.FLOAT, fl).add_column("plain", DataType.DOUBLE, plain)
    raw = c.build()
    got = read_chunk_forward(raw.columns["d"].forward, DataType.DOUBLE, n)
    assert np.array_equal(got.view(np.uint64), d.view(np.uint64))
    host = _host_segment(raw)
    assert host.real_specials("d") == (True, False)
    assert host.real_specials("fl") == (False, True)
    assert host.real_specials("plain") == (False, False)


class _CpuMaker:
    def __init__(self):
        self.calls = []

    def make_instance_plan(self, query, segments):
        self.calls.append(query)
        return ("cpu-plan", query)


@pytest.mark.parametrize("sql,refused", [
    ("SELECT MAX(dn_p2_r) FROM t", True),                       # NaN only in docs no filter matches: still the column
    ("SELECT MIN(dm_p1) FROM t WHERE f < 3", True),
    ("SELECT g, MINMAXRANGE(fn_p3) FROM t GROUP BY g", True),
    ("SELECT MAX(a * dp) FROM t WHERE f < 3", True),            # 0 * inf
    ("SELECT MIN(di_p1 - di_p1_r) FROM t WHERE f < 3", True),   # inf - inf
    ("SELECT MIN(dn_p1) FILTER (WHERE f < 50), MAX(di_p1) FILTER (WHERE f >= 50) FROM t", True),
    ("SELECT SUM(dn_p1), AVG(dm_p1_r), COUNT(*) FROM t WHERE f < 3", False),   # IEEE adds are already right
    ("SELECT SUM(a * di_p1), SUM(di_p1 - di_p1) FROM t WHERE f < 3", False),
    ("SELECT MIN(di_p1), MAX(di_p1_r), MINMAXRANGE(dp) FROM t WHERE f < 3", False),  # infinities compare like numbers
    ("SELECT MIN(dz_p1), MAX(dzn_p1_r), MIN(dd), MAX(dh), MIN(dhn) FROM t WHERE f < 3", False),
    ("SELECT MIN(dn_p1), MAX(dn_p1) FROM t", False),            # the dictionaries answer: no value is read
])
def test_nan_extrema_route_to_the_cpu_plan_maker(sql, refused):
    """The plan maker refuses MIN / MAX / MINMAXRANGE over NaN-holding columns (and arithmetic over infinities) at
    plan time with a reason naming NaN, so that the configured CPU plan maker answers; nothing else of the matrix."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker, UnsupportedOnGpu
    segs = [_host_segment(s.raw) for s in special_segments()]
    cpu = _CpuMaker()
    plan = GpuInstancePlanMaker(cpu_plan_maker=cpu).make_instance_plan(sql, segs)
    if not refused:
        assert not cpu.calls and not isinstance(plan, tuple)
        return
    assert plan[0] == "cpu-plan" and len(cpu.calls) == 1
    with pytest.raises(UnsupportedOnGpu, match="NaN"):
        GpuInstancePlanMaker().make_instance_plan(sql, segs)
