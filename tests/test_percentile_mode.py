"""CPU tests of exact PERCENTILE and MODE on the GPU path: parsing and result column names, the plan's primitive, the
{value: count} intermediate's merge and final results, the Python-side refusals (each leaves the query to the CPU plan
maker) and the ABI constants. The kernels are covered by tests/test_gpu_percentile_mode.py.
"""
import json
import math
import os

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine import startree
from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker, UnsupportedOnGpu, plan_aggregations
from pinot_amd.engine.reduce import (_agg_index, final_result, mode_of_counts, percentile_of_counts, reduce_blocks)
from pinot_amd.engine.results import (AggregationResultsBlock, ExecutionStatistics, GroupByResultsBlock,
                                      double_image_counts, java_double_key, merge_intermediate, value_counts)
from pinot_amd.engine.segment import GpuSegment
from pinot_amd.query.context import AggregationInfo, Identifier
from pinot_amd.query.sql import SqlError, parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.segment.dictionary import Dictionary
from pinot_amd.spi import DataType
from tests import fixtures


class _Seg:
    """What the plan maker asks of a segment before anything reaches the library (no GPU here)."""
    real_specials = GpuSegment.real_specials

    def __init__(self, raw):
        self.segment = raw
        self.name = "s"
        self.num_docs = raw.num_docs
        self.handle = 0
        self.star_trees = []
        self._specials = {}

    def has_column(self, c):
        return c in self.segment.columns

    def column_metadata(self, c):
        return self.segment.columns[c].metadata

    def dictionary(self, c):
        ci = self.segment.columns[c]
        m = ci.metadata
        return Dictionary(ci.dictionary, m.data_type, m.cardinality, m.string_width)

    def has_null_vector(self, c):
        return False


@pytest.fixture(scope="module")
def seg():
    rng = np.random.default_rng(7)
    n = 500
    c = SegmentCreator("pm", no_dictionary_columns=["r"])
    c.add_column("a", DataType.INT, rng.integers(0, 40, n))
    c.add_column("b", DataType.STRING, np.array([f"v{x}" for x in rng.integers(0, 9, n)]))
    c.add_column("g", DataType.INT, rng.integers(0, 5, n))
    c.add_column("r", DataType.LONG, rng.integers(0, 1000, n))
    d = rng.integers(0, 30, n) / 4.0
    c.add_column("d", DataType.DOUBLE, d)
    d = d.copy()
    d[5] = float("nan")
    c.add_column("dn", DataType.DOUBLE, d)
    return _Seg(c.build())


# ------------------------------------------------------------------------------------------------ ABI, parsing, names
def test_abi_constants():
    assert _lib.AGG_VALUE_COUNTS == 6
    assert (_lib.DISTINCT_SLOT_BITS, _lib.DISTINCT_SLOT_COUNTS) == (0, 1)
    with open(os.path.join(os.path.dirname(fixtures.GOLDEN), "..", "include", "pinot_hip.h")) as f:
        text = f.read()
    assert "#define PHIP_AGG_VALUE_COUNTS 6" in text and "#define PHIP_DISTINCT_SLOT_COUNTS 1" in text


def test_parsing_and_result_column_names():
    qc = parse("SELECT PERCENTILE95(column1), percentile(column1, 95), PERCENTILE(column1, '50'), "
               "PERCENTILE(column1, 99.9), MODE(col), mode(col, 'MAX'), MODE(col, 'AVG'), MODE(col, 'MIN') FROM t")
    a = qc.aggregations
    assert [x.function for x in a] == ["percentile"] * 4 + ["mode"] * 3  # (MODE(col) and MODE(col, 'MIN') are one)
    assert [(x.percentile, x.version) for x in a[:4]] == [(95.0, 0), (95.0, 1), (50.0, 1), (99.9, 1)]
    assert [x.reducer for x in a[4:]] == ["MIN", "MAX", "AVG"]
    assert [x.result_column_name for x in a] == [
        "percentile95(column1)", "percentile(column1, 95.0)", "percentile(column1, 50.0)", "percentile(column1, 99.9)",
        "mode(col)", "mode(col)", "mode(col)"]
    assert all(x.argument == Identifier("column1") for x in a[:4])
    # the columns of an un-aliased result table follow the reference's names
    blk = AggregationResultsBlock(a[:2], [{1.0: 1}, {1.0: 1}], ExecutionStatistics())
    rt = reduce_blocks(parse("SELECT PERCENTILE95(column1), percentile(column1, 95) FROM t"), [blk])
    assert rt.columns == ["percentile95(column1)", "percentile(column1, 95.0)"]
    # percentile 0 and 100 are accepted, in every spelling
    assert [x.percentile for x in parse("SELECT PERCENTILE0(c), PERCENTILE100(c), PERCENTILE(c, 0), "
                                        "PERCENTILE(c, '100') FROM t").aggregations] == [0.0, 100.0, 0.0, 100.0]
    # positional constructions from before the new fields keep working
    old = AggregationInfo("sum", Identifier("c"), 8, None)
    assert (old.percentile, old.version, old.reducer) == (None, 0, "MIN") and old.result_column_name == "sum(c)"
    assert a[1].unfiltered() == a[1]


@pytest.mark.parametrize("query", [
    "SELECT PERCENTILE(c, 101) FROM t",
    "SELECT PERCENTILE(c, -1) FROM t",
    "SELECT PERCENTILE(c, '100.5') FROM t",
    "SELECT PERCENTILE(c, 'abc') FROM t",
    "SELECT PERCENTILE(c, 'nan') FROM t",
    "SELECT PERCENTILE(c) FROM t",
    "SELECT PERCENTILE(c, d) FROM t",
    "SELECT PERCENTILE101(c) FROM t",
    "SELECT PERCENTILE95(c, 5) FROM t",
    "SELECT MODE(c, 'MEDIAN') FROM t",
    "SELECT MODE(c, 'min') FROM t",
    "SELECT MODE(c, 1) FROM t",
    "SELECT MODE(c, 'MIN', 'MAX') FROM t",
    "SELECT MODE() FROM t",
])
def test_bad_arguments_are_sql_errors(query):
    with pytest.raises(SqlError):
        parse(query)


def test_agg_index_tells_two_percentiles_of_one_column_apart():
    qc = parse("SELECT PERCENTILE50(c), PERCENTILE(c, 50), PERCENTILE90(c), MODE(c), MODE(c, 'AVG'), SUM(c) FROM t")
    assert [_agg_index(qc, e) for e, _ in qc.select] == [0, 1, 2, 3, 4, 5]
    counts = {float(v): 1 for v in range(10)}
    blk = AggregationResultsBlock(qc.aggregations, [counts, counts, counts, {1: 2, 5: 2}, {1: 2, 5: 2}, 45],
                                  ExecutionStatistics())
    assert reduce_blocks(qc, [blk]).rows == [[5.0, 5.0, 9.0, 1.0, 3.0, 45.0]]
    qg = parse("SELECT g, PERCENTILE90(c) FROM t GROUP BY g ORDER BY PERCENTILE90(c) DESC, g LIMIT 2")
    b = GroupByResultsBlock(qg.aggregations, list(qg.group_by), {(0,): [{1.0: 3}], (1,): [{7.0: 1}], (2,): [{7.0: 2}]})
    assert reduce_blocks(qg, [b, b]).rows == [[1, 7.0], [2, 7.0]]


def test_plan_aggregations_share_one_counts_primitive_per_column():
    qc = parse("SELECT PERCENTILE50(a), PERCENTILE(a, 99), MODE(a), MODE(a, 'AVG'), PERCENTILE50(g), DISTINCTCOUNT(a), "
               "COUNT(*) FROM t")
    prims, mapping = plan_aggregations(qc.aggregations)
    assert [m[0] for m in mapping] == ["percentile", "percentile", "mode", "mode", "percentile", "distinctcount", "count"]
    assert mapping[0][1] == mapping[1][1] == mapping[2][1] == mapping[3][1] != mapping[4][1]
    counts = [p for p in prims if p[0] == _lib.AGG_VALUE_COUNTS]
    assert [(p[1], p[2], p[3]) for p in counts] == [(_lib.EXPR_COLUMN, "a", None), (_lib.EXPR_COLUMN, "g", None)]
    assert len(prims) == 4  # counts(a), counts(g), distinct(a), count


# ------------------------------------------------------------------------------------------------ final results
def _sorted_list_percentile(values, p):
    """PercentileAggregationFunction.extractFinalResult on the value list itself."""
    v = sorted(values)
    return v[len(v) - 1] if p == 100 else v[int(float(len(v)) * p / 100)]


@pytest.mark.parametrize("size", [1, 2, 100, 101])
@pytest.mark.parametrize("p", [0, 50, 99.9, 100])
def test_percentile_index_rule(size, p):
    # values 10, 20, ...: as `size` distinct values, and as a few values with counts above one
    flat = [10.0 * (i + 1) for i in range(size)]
    assert percentile_of_counts({v: 1 for v in flat}, p) == _sorted_list_percentile(flat, p)
    lumpy = [float(i // 3) for i in range(size)]
    counts = {}
    for v in lumpy:
        counts[v] = counts.get(v, 0) + 1
    assert percentile_of_counts(counts, p) == _sorted_list_percentile(lumpy, p)
    # the index itself: size - 1 at 100, else the truncated size * p / 100
    want = {(1, 0): 0, (1, 50): 0, (1, 99.9): 0, (1, 100): 0, (2, 0): 0, (2, 50): 1, (2, 99.9): 1, (2, 100): 1,
            (100, 0): 0, (100, 50): 50, (100, 99.9): 99, (100, 100): 99, (101, 0): 0, (101, 50): 50, (101, 99.9): 100,
            (101, 100): 100}[(size, p)]
    assert percentile_of_counts({v: 1 for v in flat}, p) == flat[want]


def test_percentile_specials_and_empty():
    assert percentile_of_counts({}, 50) == float("-inf")
    agg = parse("SELECT PERCENTILE50(c) FROM t").aggregations[0]
    assert final_result("percentile", {}, agg) == float("-inf") and final_result("percentile", None, agg) is None
    # Double.compare order: -0.0 below 0.0, NaN after +inf
    c = {java_double_key(-0.0): 1, 0.0: 1, java_double_key(float("nan")): 1, float("inf"): 1, -1.0: 1}
    got = [percentile_of_counts(c, p) for p in (0, 20, 40, 60, 80, 100)]
    assert got[0] == -1.0 and math.copysign(1.0, got[1]) == -1.0 and got[1] == 0.0
    assert math.copysign(1.0, got[2]) == 1.0 and got[2] == 0.0 and got[3] == float("inf")
    assert got[4] != got[4] and got[5] != got[5]
    assert isinstance(percentile_of_counts({3: 2}, 50), float)  # DOUBLE whatever the keys


def test_mode_reducers_with_ties():
    c = {3: 5, 9: 5, 4: 5, 1: 2, 100: 4}
    assert [mode_of_counts(c, r) for r in ("MIN", "MAX", "AVG")] == [3.0, 9.0, 16.0 / 3.0]
    assert [mode_of_counts({7: 1}, r) for r in ("MIN", "MAX", "AVG")] == [7.0, 7.0, 7.0]
    assert [mode_of_counts({2.5: 3, -1.5: 3, 8.0: 1}, r) for r in ("MIN", "MAX", "AVG")] == [-1.5, 2.5, 0.5]
    assert [mode_of_counts({}, r) for r in ("MIN", "MAX", "AVG")] == [float("-inf")] * 3
    assert all(isinstance(mode_of_counts({3: 1, 4: 1}, r), float) for r in ("MIN", "MAX", "AVG"))
    big = {(1 << 52) + 1: 2, (1 << 52) + 3: 2, 5: 1}  # LONG keys stay integers until the final result
    assert mode_of_counts(big, "AVG") == float((1 << 52) + 2)
    aggs = parse("SELECT MODE(c), MODE(c, 'MAX'), MODE(c, 'AVG') FROM t").aggregations
    assert [final_result("mode", c, a) for a in aggs] == [3.0, 9.0, 16.0 / 3.0]
    assert final_result("mode", None, aggs[0]) is None


def test_merge_adds_counts():
    a, b = {1.0: 2, 2.0: 1}, {2.0: 4, 3.0: 1}
    assert merge_intermediate("percentile", a, b) == {1.0: 2, 2.0: 5, 3.0: 1}
    assert merge_intermediate("mode", {1: 2}, {1: 3, 7: 1}) == {1: 5, 7: 1}
    assert a == {1.0: 2, 2.0: 1} and b == {2.0: 4, 3.0: 1}  # the inputs stay (a block is reduced twice)
    assert merge_intermediate("percentile", None, b) == b and merge_intermediate("mode", {}, {1: 1}) == {1: 1}
    z = merge_intermediate("percentile", {java_double_key(-0.0): 1, 0.0: 2}, {java_double_key(-0.0): 3, 0.0: 4})
    assert len(z) == 2 and z[java_double_key(-0.0)] == 4 and z[0.0] == 6
    n = merge_intermediate("mode", {java_double_key(float("nan")): 1}, {java_double_key(float("nan")): 2})
    assert list(n.values()) == [3]
    qc = parse("SELECT PERCENTILE50(c), MODE(c) FROM t")
    blk = AggregationResultsBlock(qc.aggregations, [{1.0: 1, 9.0: 2}, {1: 1, 9: 2}], ExecutionStatistics())
    assert reduce_blocks(qc, [blk, blk]).rows == [[9.0, 9.0]]


def test_value_counts_and_double_images():
    m = value_counts(np.array([5, 7, 9], np.int64), np.array([2, 0, 1], np.uint32))
    assert m == {5: 2, 9: 1} and all(type(k) is int for k in m)
    f = value_counts(np.array([-0.0, 0.0, 1.5], np.float32), np.array([1, 2, 3], np.uint32))
    assert len(f) == 3 and f[java_double_key(-0.0)] == 1 and f[0.0] == 2 and f[1.5] == 3
    # two LONGs with one double image add their counts under PERCENTILE, and stay apart under MODE
    big = value_counts(np.array([(1 << 53), (1 << 53) + 1, 4], np.int64), np.array([1, 2, 3], np.uint32))
    assert len(big) == 3
    assert double_image_counts(big) == {float(1 << 53): 3, 4.0: 3}
    assert double_image_counts(f) is f
    qg = parse("SELECT g, PERCENTILE50(c), MODE(c) FROM t GROUP BY g")
    blk = GroupByResultsBlock(qg.aggregations, list(qg.group_by), None)
    col = np.empty(2, dtype=object)
    col[:] = [{1: 2}, big]
    blk.set_columns([np.array([7, 8])], [col], [("percentile", 0), ("mode", 0)])
    assert blk.groups == {(7,): [{1.0: 2}, {1: 2}], (8,): [{float(1 << 53): 3, 4.0: 3}, big]}
    assert all(type(k) is float for k in blk.groups[(7,)][0])


# ------------------------------------------------------------------------------------------------ plan-time refusals
@pytest.mark.parametrize("query", [
    "SELECT PERCENTILE95(r) FROM t WHERE g > 1",                                   # raw (no-dictionary) argument
    "SELECT MODE(r) FROM t WHERE g > 1",
    "SELECT PERCENTILE95(b) FROM t WHERE g > 1",                                   # STRING
    "SELECT MODE(b) FROM t WHERE g > 1",
    "SELECT PERCENTILE(a + g, 50) FROM t WHERE g > 1",                             # expression argument
    "SELECT PERCENTILE50(a) FILTER(WHERE g > 1) FROM t",                           # FILTER(WHERE)
    "SELECT MODE(a) FILTER(WHERE g > 1) FROM t GROUP BY g",
    "SELECT COUNT(*) FILTER(WHERE g > 1), PERCENTILE50(a) FROM t",                 # ... on a function beside it
    "SELECT PERCENTILE50(CASE WHEN g > 1 THEN a ELSE 0 END) FROM t",               # CASE
    "SELECT SUM(CASE WHEN g > 1 THEN a ELSE 0 END), MODE(a) FROM t",
    "SET enableNullHandling = true; SELECT PERCENTILE50(a) FROM t WHERE g > 1",    # null handling
    "SET enableNullHandling = true; SELECT g, MODE(a) FROM t GROUP BY g",
    "SELECT MODE(dn) FROM t WHERE g > 1",                                          # MODE over a dictionary with NaN
    "SELECT g, MODE(dn, 'MAX') FROM t GROUP BY g",
])
def test_python_side_refusals(query, seg):
    with pytest.raises(UnsupportedOnGpu):
        GpuInstancePlanMaker().make_instance_plan(parse(query), [seg])


def test_plans_the_gpu_takes(seg):
    for q in ("SELECT PERCENTILE95(a), MODE(a, 'AVG'), PERCENTILE(d, 50) FROM t WHERE g > 1",
              "SELECT g, MODE(d), PERCENTILE50(dn) FROM t GROUP BY g",  # (PERCENTILE orders a NaN as Arrays.sort does)
              "SELECT PERCENTILE50(a) FROM t"):
        op = GpuInstancePlanMaker().make_instance_plan(parse(q), [seg])
        assert isinstance(op, GpuCombineOperator)
        assert not op._non_scan_fit()  # the reference scans: the dictionary shortcut must not claim these functions


def test_star_tree_and_device_trim_do_not_claim_them(seg):
    assert "percentile" not in startree._STAR_FUNCS and "mode" not in startree._STAR_FUNCS
    qc = parse("SELECT PERCENTILE50(a) FROM t WHERE g > 1")
    assert startree.GpuStarTreeOperator.plan(qc, [seg], 100000) is None
    op = GpuCombineOperator(parse("SELECT g, PERCENTILE90(a) FROM t GROUP BY g ORDER BY PERCENTILE90(a), g LIMIT 3"),
                            [seg], 100000)
    assert op._trim_spec() == (-1, 0, 0, [], [])  # no device trim: every group goes to the reduce


def test_golden_file_is_consistent_with_the_fixture():
    """The recorded rows against numpy on the committed fixture (the plain, group-by and ORDER BY cases; the reference's
    test reduces the two-segment server response twice, so every value counts four times)."""
    with open(os.path.join(fixtures.GOLDEN, "percentile.json")) as f:
        cases = json.load(f)["queries"]
    assert len(cases) == 49
    data = np.load(os.path.join(fixtures.GOLDEN, "test_data_sv.npz"))

    def pct(values, p):
        v = np.sort(np.repeat(np.asarray(values, dtype=np.float64), 4))
        return float(v[len(v) - 1 if p == 100 else int(float(len(v)) * p / 100)])

    for j, p in enumerate((50, 90, 95, 99)):
        for spelling in range(3):
            plain, _, grouped, _ = cases[12 * j + 4 * spelling:12 * j + 4 * spelling + 4]
            assert str(p) in plain["query"] and " WHERE " not in plain["query"] and "GROUP BY" in grouped["query"]
            assert plain["rows"] == [[pct(data["column1"], p), pct(data["column3"], p)]]
            best = max((pct(data["column1"][data["column9"] == g], p), pct(data["column3"][data["column9"] == g], p))
                       for g in np.unique(data["column9"]))
            assert grouped["rows"] == [list(best)]
    per = sorted((pct(data["column6"][data["column11"] == k], 90), k) for k in np.unique(data["column11"]).tolist())
    assert cases[48]["rows"] == [[k, v] for v, k in per[:3]]
