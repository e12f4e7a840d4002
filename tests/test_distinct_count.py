"""CPU tests of exact DISTINCTCOUNT on the GPU path: the plan's primitives, the intermediate's merge and reduce, the
Python-side refusals (each leaves the query to the CPU plan maker) and the ABI constant. The kernels are covered by
tests/test_gpu_distinct_count.py.
"""
import json
import math
import os

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine import startree
from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker, UnsupportedOnGpu, plan_aggregations
from pinot_amd.engine.reduce import final_result, reduce_blocks
from pinot_amd.engine.results import (AggregationResultsBlock, ExecutionStatistics, GroupByResultsBlock, java_double_key,
                                      merge_intermediate)
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.segment.dictionary import Dictionary
from pinot_amd.spi import DataType
from tests import fixtures


class _Seg:
    """What the plan maker asks of a segment before anything reaches the library (no GPU here)."""

    def __init__(self, raw, nulls=()):
        self.segment = raw
        self.name = "s"
        self.num_docs = raw.num_docs
        self.handle = 0
        self._nulls = set(nulls)
        self.star_trees = []

    def has_column(self, c):
        return c in self.segment.columns

    def column_metadata(self, c):
        return self.segment.columns[c].metadata

    def dictionary(self, c):
        ci = self.segment.columns[c]
        m = ci.metadata
        return Dictionary(ci.dictionary, m.data_type, m.cardinality, m.string_width)

    def has_null_vector(self, c):
        return c in self._nulls


@pytest.fixture(scope="module")
def seg():
    rng = np.random.default_rng(7)
    n = 500
    c = SegmentCreator("dc", no_dictionary_columns=["r"])
    data = {"a": rng.integers(0, 40, n), "b": np.array([f"v{x}" for x in rng.integers(0, 9, n)])}
    c.add_column("a", DataType.INT, data["a"])
    c.add_column("b", DataType.STRING, data["b"])
    c.add_column("g", DataType.INT, rng.integers(0, 5, n))
    c.add_column("r", DataType.LONG, rng.integers(0, 1000, n))
    s = _Seg(c.build())
    s.data = data
    return s


def test_abi_constant():
    assert _lib.AGG_DISTINCT == 5
    assert "phip_result_distinct_dictionary" in _lib.EXPORTED_SYMBOLS
    names = [f for f, _ in _lib.Result._fields_]
    assert names[-5:] == ["num_distinct", "reserved_distinct", "distinct_words", "distinct_word_offsets",
                          "distinct_kernel_ms"]


def test_plan_aggregations_maps_distinctcount_and_shares_a_slot():
    qc = parse("SELECT COUNT(*), DISTINCTCOUNT(a), DISTINCTCOUNT(b), SUM(a) FROM t")
    a = qc.aggregations  # (the query context keeps one entry per function: repeat the column's here)
    prims, mapping = plan_aggregations([a[0], a[1], a[2], a[1], a[3]])
    assert [m[0] for m in mapping] == ["count", "distinctcount", "distinctcount", "distinctcount", "sum"]
    assert mapping[1][1] == mapping[3][1] != mapping[2][1]  # the repeated column shares its primitive
    dist = [p for p in prims if p[0] == _lib.AGG_DISTINCT]
    assert [(p[1], p[2], p[3]) for p in dist] == [(_lib.EXPR_COLUMN, "a", None), (_lib.EXPR_COLUMN, "b", None)]
    assert len(prims) == 4


def test_merge_is_a_union_with_java_double_semantics():
    assert merge_intermediate("distinctcount", {1, 2}, {2, 3}) == {1, 2, 3}
    assert merge_intermediate("distinctcount", {"x"}, set()) == {"x"}
    assert merge_intermediate("distinctcount", None, {1}) == {1}
    z = merge_intermediate("distinctcount", {java_double_key(0.0)}, {java_double_key(-0.0)})
    assert len(z) == 2 and sorted(math.copysign(1.0, v) for v in z) == [-1.0, 1.0]
    n = merge_intermediate("distinctcount", {java_double_key(float("nan"))}, {java_double_key(float("nan"))})
    assert len(n) == 1
    a = {1}
    merge_intermediate("distinctcount", a, {2})
    assert a == {1}  # the inputs stay as they were (a block is reduced twice by broker_response)


def test_reduce_returns_an_int_count_and_orders_by_it():
    assert final_result("distinctcount", {3, 4, 5}) == 3 and isinstance(final_result("distinctcount", {3}), int)
    assert final_result("distinctcount", None) is None
    qc = parse("SELECT DISTINCTCOUNT(a) FROM t")
    blk = AggregationResultsBlock(qc.aggregations, [{1, 2, 3}], ExecutionStatistics())
    rt = reduce_blocks(qc, [blk, AggregationResultsBlock(qc.aggregations, [{3, 4}], ExecutionStatistics())])
    assert rt.rows == [[4]] and type(rt.rows[0][0]) is int
    qg = parse("SELECT g, DISTINCTCOUNT(a) FROM t GROUP BY g ORDER BY DISTINCTCOUNT(a) DESC, g LIMIT 2")
    b1 = GroupByResultsBlock(qg.aggregations, list(qg.group_by), {(0,): [{1}], (1,): [{1, 2}], (2,): [{5}]})
    b2 = GroupByResultsBlock(qg.aggregations, list(qg.group_by), {(0,): [{2, 3}], (2,): [{5}]})
    assert reduce_blocks(qg, [b1, b2]).rows == [[0, 3], [1, 2]]


def test_columnar_group_by_block_carries_sets():
    qg = parse("SELECT g, DISTINCTCOUNT(a) FROM t GROUP BY g")
    blk = GroupByResultsBlock(qg.aggregations, list(qg.group_by), None)
    col = np.empty(2, dtype=object)
    col[:] = [{1, 2}, {3}]
    blk.set_columns([np.array([7, 8])], [col], [("distinctcount", 0)])
    assert blk.groups == {(7,): [{1, 2}], (8,): [{3}]}


def test_non_scan_shortcut_answers_from_the_dictionaries(seg):
    qc = parse("SELECT DISTINCTCOUNT(a), DISTINCTCOUNT(b), COUNT(*) FROM t")
    op = GpuCombineOperator(qc, [seg, seg], 100000)
    assert op._non_scan_fit()
    blk = op.next_block()  # (launches nothing: no library is loaded on this host)
    a = set(np.unique(seg.data["a"]).tolist())
    b = set(np.unique(seg.data["b"]).tolist())
    assert blk.results[0] == a and blk.results[1] == b and blk.results[2] == 2 * seg.num_docs
    assert blk.stats.num_entries_scanned_post_filter == 0 and blk.stats.num_docs_scanned == 2 * seg.num_docs
    assert reduce_blocks(qc, [blk]).rows == [[len(a), len(b), 2 * seg.num_docs]]
    # a filter or a group-by takes the scan
    assert not GpuCombineOperator(parse("SELECT DISTINCTCOUNT(a) FROM t WHERE g > 1"), [seg], 100000)._non_scan_fit()
    assert not GpuCombineOperator(parse("SELECT g, DISTINCTCOUNT(a) FROM t GROUP BY g"), [seg], 100000)._non_scan_fit()


@pytest.mark.parametrize("query", [
    "SELECT DISTINCTCOUNT(r) FROM t WHERE g > 1",                                  # raw (no-dictionary) argument
    "SELECT DISTINCTCOUNT(a + g) FROM t WHERE g > 1",                              # expression argument
    "SELECT DISTINCTCOUNT(a) FILTER(WHERE g > 1) FROM t",                          # FILTER(WHERE)
    "SELECT DISTINCTCOUNT(a) FILTER(WHERE g > 1) FROM t GROUP BY g",
    "SELECT COUNT(*) FILTER(WHERE g > 1), DISTINCTCOUNT(a) FROM t",                # ... on a function beside it
    "SELECT DISTINCTCOUNT(CASE WHEN g > 1 THEN a ELSE 0 END) FROM t",              # CASE
    "SET enableNullHandling = true; SELECT DISTINCTCOUNT(a) FROM t WHERE g > 1",   # null handling
    "SET enableNullHandling = true; SELECT g, DISTINCTCOUNT(a) FROM t GROUP BY g",
])
def test_python_side_refusals(query, seg):
    with pytest.raises(UnsupportedOnGpu):
        GpuInstancePlanMaker().make_instance_plan(parse(query), [seg])


def test_null_handling_with_null_vectors_refuses():
    rng = np.random.default_rng(3)
    c = SegmentCreator("dcn")
    c.add_column("a", DataType.INT, rng.integers(0, 40, 100))
    c.add_column("g", DataType.INT, rng.integers(0, 5, 100))
    s = _Seg(c.build(), nulls=("a",))
    with pytest.raises(UnsupportedOnGpu):
        GpuInstancePlanMaker().make_instance_plan(
            parse("SET enableNullHandling = true; SELECT DISTINCTCOUNT(a) FROM t WHERE g > 1"), [s])


def test_star_tree_path_does_not_claim_distinctcount(seg):
    assert "distinctcount" not in startree._STAR_FUNCS
    qc = parse("SELECT DISTINCTCOUNT(a) FROM t WHERE g > 1")
    assert startree._pair_of(qc.aggregations[0]) is None
    assert startree.GpuStarTreeOperator.plan(qc, [seg], 100000) is None


def test_order_by_distinctcount_is_left_to_the_broker_reduce(seg):
    op = GpuCombineOperator(parse("SELECT g, DISTINCTCOUNT(a) FROM t GROUP BY g ORDER BY DISTINCTCOUNT(a) LIMIT 3"),
                            [seg], 100000)
    assert op._trim_spec() == (-1, 0, 0, [], [])  # no device trim: every group goes to the reduce


def test_golden_file_is_consistent_with_the_fixture():
    """The recorded rows against numpy on the committed fixture (the no-filter and group-by cases)."""
    with open(os.path.join(fixtures.GOLDEN, "distinct_count.json")) as f:
        cases = json.load(f)["queries"]
    assert len(cases) == 6
    data = np.load(os.path.join(fixtures.GOLDEN, "test_data_sv.npz"))
    assert cases[0]["rows"] == [[len(np.unique(data["column1"])), len(np.unique(data["column3"]))]]
    per = {}
    for k, v in zip(data["column12"].tolist(), data["column11"].tolist()):
        per.setdefault(k, set()).add(v)
    assert [[k, len(per[k])] for k in sorted(per)] == cases[4]["rows"]
    best = max(((len(np.unique(data["column1"][data["column9"] == g])), len(np.unique(data["column3"][data["column9"] == g])))
                for g in np.unique(data["column9"])))
    assert [list(best)] == cases[2]["rows"]
