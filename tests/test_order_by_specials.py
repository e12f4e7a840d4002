"""ORDER BY over the Double.compare ladder on the host: the broker's ``reduce_blocks`` and the host trim ``trim_groups``
against tests/java_fold.py's ``record_compare`` (TableResizer.java:90-96: Comparator.naturalOrder() over the final
results -- for a Double, Double.compare: -0.0 < 0.0, every NaN equal to every other and above +inf). No GPU.

The blocks are built by hand from the expected intermediates of tests/order_data.py (``Ladder``: java_fold over the
stored values; the HLL registers by the oracle's route, the estimate by ``reduce.hll_cardinality``). The helpers here
(``Ladder``, ``order_terms``, ``select_list``) are shared with tests/test_gpu_order_by_specials.py.
"""
import functools

import pytest

from pinot_amd.engine.reduce import hll_cardinality, reduce_blocks, trim_groups
from pinot_amd.engine.results import GroupByResultsBlock, java_double_key
from pinot_amd.query.sql import parse
from tests import java_fold as jf
from tests import order_data as od

NAN = float("nan")
INF = float("inf")

# ORDER BY / SELECT expression -> (function, column)
AGGS = {"SUM(s)": ("sum", "s"), "SUM(s_r)": ("sum", "s_r"), "SUM(sf)": ("sum", "sf"), "AVG(s)": ("avg", "s"),
        "MIN(x)": ("min", "x"), "MAX(x)": ("max", "x"), "MIN(x_r)": ("min", "x_r"), "MAX(x_r)": ("max", "x_r"),
        "MINMAXRANGE(x)": ("minmaxrange", "x"), "COUNT(*)": ("count", None),
        "DISTINCTCOUNTHLL(h)": ("distinctcounthll", "h")}
KEYS = ("g", "gr", "gd")
SIGNED_ZERO = {"sum", "avg", "min", "max", "minmaxrange"}   # the sign of a zero counts in every double compared here


class Ladder:
    """The expected intermediates, final results and key values of the 16 groups over ``seg_ids``, filtered by
    ``f < 99`` or not; computed once per instance and left unchanged."""

    def __init__(self, seg_ids=(0, 1), filtered=True):
        self.seg_ids, self.filtered = tuple(seg_ids), filtered

    @functools.lru_cache(maxsize=None)
    def intermediate(self, expr, i):
        function, col = AGGS[expr]
        if function == "distinctcounthll":
            return od.hll_registers(od.intermediate("values", col, i, self.seg_ids, self.filtered))
        return od.intermediate(function, col, i, self.seg_ids, self.filtered)

    @functools.lru_cache(maxsize=None)
    def value(self, expr, i):
        """The value of an ORDER BY / SELECT expression for group i: a key's value or an aggregation's final result."""
        if expr in KEYS:
            return od.key_value(expr, i)
        function, _ = AGGS[expr]
        if function == "distinctcounthll":
            return hll_cardinality(self.intermediate(expr, i))
        return od.final(function, self.intermediate(expr, i))

    def terms(self, order):
        return [(functools.partial(self.value, e), asc) for e, asc in order_terms(order)]

    def ordered(self, order):
        """The groups in record_compare order (ties in group-index order: compare term values, not indices)."""
        return sorted(range(od.NG), key=functools.cmp_to_key(jf.record_compare(self.terms(order))))

    def is_total(self, order):
        cmp = jf.record_compare(self.terms(order))
        o = self.ordered(order)
        return all(cmp(a, b) < 0 for a, b in zip(o, o[1:]))


@functools.lru_cache(maxsize=None)
def ladder(seg_ids=(0, 1), filtered=True):
    return Ladder(seg_ids, filtered)


def order_terms(order):
    """'SUM(s) DESC, g' -> [('SUM(s)', False), ('g', True)]."""
    out = []
    for t in order.split(", "):
        desc = t.endswith(" DESC")
        out.append((t[:-5] if desc else t, not desc))
    return out


def flipped(order):
    """The same ORDER BY with every direction reversed."""
    return ", ".join(e + ("" if not asc else " DESC") for e, asc in order_terms(order))


def select_list(order, keys=("g",), extra=("COUNT(*)",)):
    """The group-by keys, the aggregations of the ORDER BY, and ``extra``."""
    aggs = [e for e, _ in order_terms(order) if e in AGGS]
    return list(keys) + aggs + [e for e in extra if e not in aggs]


def same_value(a, b):
    """Two final results or key values: ints exactly, doubles by java_fold.same_double with the zero's sign."""
    if isinstance(a, int) and isinstance(b, int):
        return a == b
    return jf.same_double(a, b, True)


def aggregation_expr(ag):
    """The AGGS name of a parsed aggregation."""
    col = ag.argument.name if ag.argument is not None else None
    return next(e for e, fc in AGGS.items() if fc == (ag.function, col))


def hand_block(qc, lad, keys=("g",), null_key_group=None):
    """The results block a server would answer ``qc`` with, from the expected intermediates."""
    groups = {}
    for i in range(od.NG):
        key = tuple(None if (i == null_key_group and k == "gd") else java_double_key(lad.value(k, i)) for k in keys)
        groups[key] = [lad.intermediate(aggregation_expr(a), i) for a in qc.aggregations]
    return GroupByResultsBlock(qc.aggregations, list(qc.group_by), groups)


SINGLE = ["SUM(s)", "SUM(s_r)", "SUM(sf)", "AVG(s)", "MIN(x)", "MIN(x_r)", "MAX(x)", "MAX(x_r)", "MINMAXRANGE(x)",
          "COUNT(*)", "DISTINCTCOUNTHLL(h)", "gd"]
HOST_ORDERS = [o for e in SINGLE for o in (e, e + " DESC", e + ", g", e + " DESC, g", e + ", g DESC")]


def _query(order, limit, keys=("g", "gd"), options=""):
    sel = ", ".join(select_list(order, keys))
    return parse(f"{options}SELECT {sel} FROM t GROUP BY {', '.join(keys)} ORDER BY {order} LIMIT {limit}")


def _check_rows(rows, order, lad, sel):
    """The rows are in record_compare order: the ORDER BY values of row r are those of the r-th group of the expected
    order (a sequence that ties do not change), every row is one group's own, and no group comes twice."""
    bad = []
    want = lad.ordered(order)[:len(rows)]
    by_g = {od.G[i]: i for i in range(od.NG)}
    if len({r[0] for r in rows}) != len(rows):
        bad.append(f"{order}: a group comes twice: {[r[0] for r in rows]}")
    for r, (row, w) in enumerate(zip(rows, want)):
        i = by_g.get(row[0])
        if i is None:
            bad.append(f"{order}: row {r} has the unknown key {row[0]}")
            continue
        for e, _ in order_terms(order):
            got = row[sel.index(e)]
            if not same_value(got, lad.value(e, w)):
                bad.append(f"{order}: row {r} (g={row[0]}) has {e} = {got!r}, the order wants {lad.value(e, w)!r}")
        for c, e in enumerate(sel):
            if e != "gd" and not same_value(row[c], lad.value(e, i)):
                bad.append(f"{order}: row {r} (g={row[0]}) has {e} = {row[c]!r}, its group has {lad.value(e, i)!r}")
    return bad


def _report(bad):
    assert not bad, f"{len(bad)} failing cells:\n" + "\n".join(bad)


def test_double_compare_and_top_records():
    neg_nan, pos_nan = od._d(od.NAN_NEG), od._d(od.NAN_POS)
    ladder_ = [-INF, -od.DBL_MAX, -1.5, -od.DENORM, -0.0, 0.0, od.DENORM, 2.25, od.DBL_MAX, INF, NAN]
    for a, b in zip(ladder_, ladder_[1:]):
        assert jf.double_compare(a, b) == -1 and jf.double_compare(b, a) == 1, (a, b)
    assert jf.double_compare(neg_nan, pos_nan) == 0 and jf.double_compare(neg_nan, INF) == 1
    assert jf.double_compare(pos_nan - pos_nan, neg_nan) == 0 and jf.double_compare(-INF, neg_nan) == -1
    assert jf.double_compare(0.0, 0.0) == 0 and jf.double_compare(-0.0, -0.0) == 0
    assert jf.value_compare(2 ** 63 - 1, 2 ** 63 - 2) == 1 and jf.value_compare(3, 3) == 0
    recs = [(1.0, 7), (neg_nan, 1), (-0.0, 2), (pos_nan, 3), (0.0, 4), (1.0, 5)]
    first = [(lambda r: r[0], True)]
    must, may = jf.top_records(recs, first, 3)
    assert must == [(-0.0, 2), (0.0, 4)] and sorted(may) == [(1.0, 5), (1.0, 7)]
    must, may = jf.top_records(recs, first, 5)
    assert len(must) == 4 and sorted(r[1] for r in may) == [1, 3]
    must, may = jf.top_records(recs, [(lambda r: r[0], False), (lambda r: r[1], True)], 3)
    assert [r[1] for r in must] == [1, 3] and may == [(1.0, 5)]
    assert jf.top_records(recs, first, 6) == (sorted(recs, key=functools.cmp_to_key(jf.record_compare(first))), [])


def test_double_order_image():
    """reduce.double_order ascending over both NaNs, both zeros, the infinities and a denormal (a Python-float sort key
    left the NaNs unordered: 1.0 came before -1.0 and 0.0 before -0.0)."""
    from pinot_amd.engine.reduce import double_order
    vals = [1.0, od._d(od.NAN_NEG), -1.0, NAN, 0.0, -0.0, INF, -INF, 5e-324]
    got = sorted(vals, key=double_order)
    want = [-INF, -1.0, -0.0, 0.0, 5e-324, 1.0, INF, NAN, NAN]
    assert all(jf.same_double(a, b, True) for a, b in zip(got, want)), got
    assert double_order(od._d(od.NAN_NEG)) == double_order(NAN) == double_order(INF - INF)


@pytest.mark.parametrize("order", HOST_ORDERS)
def test_reduce_blocks_orders_by_double_compare(order):
    lad = ladder()
    qc = _query(order, od.NG)
    sel = select_list(order, ("g", "gd"))
    rows = reduce_blocks(qc, [hand_block(qc, lad, ("g", "gd"))]).rows
    bad = [] if len(rows) == od.NG else [f"{order}: {len(rows)} rows"]
    bad += _check_rows(rows, order, lad, sel)
    if lad.is_total(order):
        want = [od.G[i] for i in lad.ordered(order)]
        if [r[0] for r in rows] != want:
            bad.append(f"{order}: keys {[r[0] for r in rows]}, want {want}")
    _report(bad)


@pytest.mark.parametrize("order", HOST_ORDERS)
def test_trim_groups_keeps_the_double_compare_top(order):
    lad = ladder()
    bad = []
    for k in range(5, od.NG):
        qc = _query(order, 1, options=f"SET minServerGroupTrimSize = {k}; ")
        blk = trim_groups(qc, hand_block(qc, lad, ("g", "gd")))
        kept = {od.G.index(key[0]) for key in blk.groups}
        must, may = jf.top_records(range(od.NG), lad.terms(order), k)
        if not (blk.num_groups_trimmed and len(blk.groups) == k and set(must) <= kept <= set(must) | set(may)):
            bad.append(f"{order}, trim {k}: kept {sorted(kept)}, must keep {sorted(must)}, may keep {sorted(may)}")
    _report(bad)


@pytest.mark.parametrize("nulls,asc,null_first", [("", True, False), ("", False, True), (" NULLS FIRST", True, True),
                                                  (" NULLS LAST", True, False), (" NULLS FIRST", False, True),
                                                  (" NULLS LAST", False, False)])
def test_null_key_among_special_values(nulls, asc, null_first):
    """A null gd key (group 14's, in place of 42.0) goes where NULLS FIRST / LAST or the default (nulls as the largest
    value) puts it; the values around it are in Double.compare order."""
    lad = ladder()
    order = "gd" + ("" if asc else " DESC")
    qc = parse(f"SELECT g, gd, COUNT(*) FROM t GROUP BY g, gd ORDER BY gd{'' if asc else ' DESC'}{nulls}, g LIMIT 16")
    rows = reduce_blocks(qc, [hand_block(qc, lad, ("g", "gd"), null_key_group=14)]).rows
    want = [i for i in lad.ordered(order + ", g") if i != 14]
    want = [14] + want if null_first else want + [14]
    assert [r[0] for r in rows] == [od.G[i] for i in want]
    assert rows[want.index(14)][1] is None
    for k in (5, 15):
        q2 = parse(f"SET minServerGroupTrimSize = {k}; SELECT g, gd, COUNT(*) FROM t GROUP BY g, gd "
                   f"ORDER BY gd{'' if asc else ' DESC'}{nulls}, g LIMIT 1")
        blk = trim_groups(q2, hand_block(q2, lad, ("g", "gd"), null_key_group=14))
        assert {key[0] for key in blk.groups} == {od.G[i] for i in want[:k]}
