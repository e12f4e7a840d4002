"""Conditions on the inputs of the ORDER BY tests (tests/order_data.py), checked on the CPU with java_fold alone (the
HLL estimate by ``reduce.hll_cardinality`` over the oracle's registers): the 16 final results of every ORDER BY term
hold the classes of the Double.compare ladder they are meant to, with ties, and the trim boundaries 5..15 fall both
inside ties and between distinct values. These are properties of the fixture, not measurements of the library.
"""
import numpy as np
import pytest

from tests import java_fold as jf
from tests import order_data as od
from tests.test_order_by_specials import ladder

INF = float("inf")
NAN = float("nan")
WALKS = [((0,), True), ((0, 1), True)]


def _holds(values, wanted):
    """Every value of ``wanted`` occurs among ``values`` (same_double with the zero's sign), as often as it is listed."""
    left = list(values)
    for w in wanted:
        hit = next((j for j, v in enumerate(left) if jf.same_double(v, w, True)), None)
        if hit is None:
            return False
        left.pop(hit)
    return True


def test_shape():
    segs = od.segments()
    assert [s.n for s in segs] == [2 * 2048 + 77, 2048 + 5]
    for s in segs:
        assert set(s.group.tolist()) == set(range(od.NG))
        assert int((~s.matched).sum()) == sum(1 + i % 3 for i in range(od.NG))
        for col in ("s", "s_r", "sf", "x", "x_r"):   # the docs the filter excludes hold poison in every metric
            v = s.stored_values(col)[~s.matched]
            assert all(x != x or abs(x) >= 3e38 for x in v.tolist()), col
        assert not np.isnan(s.stored_values("x")).any() and not np.isnan(s.stored_values("x_r")).any()
        assert s.raw.columns["g"].metadata.has_dictionary and not s.raw.columns["gr"].metadata.has_dictionary
        assert s.raw.columns["gd"].metadata.has_dictionary
    for col in ("s", "sf", "x", "h"):
        assert segs[0].raw.columns[col].dictionary != segs[1].raw.columns[col].dictionary, col
    assert sorted(od.G) != od.G and len(set(od.G)) == od.NG
    # the raw column keeps the NaN whose sign bit is set; a matched doc holds it
    bits = segs[0].stored_values("s_r").view(np.uint64)[segs[0].docs(0, True)]
    assert (bits == od.NAN_NEG).sum() == 1


def test_gd_key_values():
    """One gd value per group, the same in both segments; the dictionary keeps one zero (the groups 4 and 5 tie)."""
    segs = od.segments()
    vals = []
    for i in range(od.NG):
        per_seg = [set(s.stored_values("gd")[s.docs(i, False)].view(np.uint64).tolist()) for s in segs]
        assert len(per_seg[0]) == 1 and per_seg[0] == per_seg[1], i
        vals.append(od.key_value("gd", i))
    assert _holds(vals, [-INF, -od.DBL_MAX, -1.5, -od.DENORM, od.DENORM, 2.25, od.DBL_MAX, INF, NAN])
    assert jf.same_double(vals[4], -0.0, True) and jf.same_double(vals[5], -0.0, True)
    assert sorted(range(od.NG), key=lambda i: od.G[i]) != sorted(range(od.NG), key=lambda i: (vals[i] != vals[i], vals[i]))


@pytest.mark.parametrize("seg_ids,filtered", WALKS)
def test_ladder_classes(seg_ids, filtered):
    lad = ladder(seg_ids, filtered)
    finals = {e: [lad.value(e, i) for i in range(od.NG)] for e in
              ("SUM(s)", "SUM(s_r)", "SUM(sf)", "AVG(s)", "MIN(x)", "MIN(x_r)", "MAX(x_r)", "MINMAXRANGE(x)", "COUNT(*)",
               "DISTINCTCOUNTHLL(h)")}
    for e in ("SUM(s)", "SUM(s_r)"):
        assert _holds(finals[e], [NAN, NAN, NAN, -INF, INF, -od.DBL_MAX, od.DBL_MAX, -od.DENORM, od.DENORM, 0.0, 0.0,
                                  -1.5, -1.5, 2.25, 2.25, 1e300]), e
    assert _holds(finals["SUM(sf)"], [NAN, NAN, NAN, -INF, INF, -od.FLT_MAX, od.FLT_MAX, -od.FLT_DENORM, od.FLT_DENORM,
                                      0.0, 0.0, -1.5, -1.5, 2.25, 2.25])
    # AVG divides the ladder by the counts: the classes stay (a denormal over a count rounds to a zero of its sign)
    assert _holds(finals["AVG(s)"], [NAN, NAN, NAN, -INF, INF, -0.0, 0.0, 0.0, 0.0])
    assert sum(1 for v in finals["AVG(s)"] if v == v and abs(v) not in (0.0, INF)) == 7
    assert _holds(finals["MIN(x_r)"], [-INF, -INF, -od.DBL_MAX, -1.5, -1.5, -od.DENORM, -0.0, 0.0, od.DENORM, 2.25,
                                       od.DBL_MAX, INF])
    assert _holds(finals["MAX(x_r)"], [-INF, -0.0, 0.0, od.DENORM, od.DENORM, -od.DENORM, od.DBL_MAX, od.DBL_MAX, INF, INF])
    # the dictionary of x keeps one of the two zeros: the same classes, the zeros a tie
    assert _holds(finals["MIN(x)"], [-INF, -INF, -od.DBL_MAX, -1.5, -1.5, -od.DENORM, od.DENORM, 2.25, od.DBL_MAX, INF])
    assert sum(1 for v in finals["MIN(x)"] if v == 0.0) == 2
    assert _holds(finals["MINMAXRANGE(x)"], [INF, INF, NAN, NAN, 0.0, 0.0, 0.0, 4.0, 4.0, 2 * od.DENORM])
    counts = finals["COUNT(*)"]
    assert len({counts[i] for i in od.COUNT_TIE}) == 1 and len(set(counts)) == od.NG - len(od.COUNT_TIE) + 1
    est = finals["DISTINCTCOUNTHLL(h)"]
    assert all(isinstance(v, int) for v in est) and est[0] == est[1] == 1 and est[3] == est[4]
    assert 8 <= len(set(est)) < od.NG


def test_unfiltered_order_differs():
    """The poison docs change the order of every double-valued term: a trim that read unfiltered values would show."""
    for e in ("SUM(s)", "SUM(s_r)", "SUM(sf)", "AVG(s)", "MIN(x)", "MAX(x)", "MINMAXRANGE(x)"):
        a, b = ladder((0, 1), True), ladder((0, 1), False)
        assert [jf.double_to_long_bits(a.value(e, i)) for i in range(od.NG)] != \
               [jf.double_to_long_bits(b.value(e, i)) for i in range(od.NG)], e
        assert a.ordered(e + ", g") != b.ordered(e + ", g"), e


@pytest.mark.parametrize("order", ["SUM(s)", "SUM(s_r)", "SUM(sf)", "AVG(s)", "MIN(x)", "MAX(x)", "MINMAXRANGE(x)", "COUNT(*)",
                                   "DISTINCTCOUNTHLL(h)", "gd"])
def test_boundaries_fall_inside_ties_and_between_values(order):
    """Of the boundary positions 5..15 (ascending and descending), at least two fall inside a tie (the k-th and the
    k+1-th record compare equal) and at least eight between distinct values."""
    lad = ladder()
    inside = between = 0
    for o in (order, order + " DESC"):
        cmp = jf.record_compare(lad.terms(o))
        rec = lad.ordered(o)
        for k in range(5, od.NG):
            if cmp(rec[k - 1], rec[k]) == 0:
                inside += 1
            else:
                between += 1
    assert inside >= 2 and between >= 8, (inside, between)
