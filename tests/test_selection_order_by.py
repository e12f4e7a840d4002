"""CPU tests of selection ORDER BY: OFFSET parsing, the block-expression order, the CPU restatement
(tests/selection_order_ref.py) against Pinot's known answers, the order-by reduce and the leaf stage's column lookup."""
import json
import os

import pytest

from pinot_amd.engine import reduce as reduce_mod
from pinot_amd.engine.leaf_stage import DataSchema, compose_select_transferable_block
from pinot_amd.engine.results import ExecutionStatistics, SelectionResultsBlock
from pinot_amd.query.sql import parse
from tests import fixtures
from tests.selection_order_ref import double_compare_key, restate

with open(os.path.join(fixtures.GOLDEN, "selection_order_by.json")) as _f:
    GOLDEN = json.load(_f)


def golden_sql(case):
    return case["sql"].replace("{filter}", GOLDEN["filter"])


# ---- SQL ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sql, limit, offset", [
    ("SELECT a FROM t ORDER BY a LIMIT 7 OFFSET 3", 7, 3),
    ("SELECT a FROM t ORDER BY a LIMIT 7 offset 3", 7, 3),
    ("SELECT a FROM t ORDER BY a LIMIT 5000, 7000", 7000, 5000),
    ("SELECT a FROM t ORDER BY a LIMIT 7", 7, 0),
    ("SELECT a FROM t ORDER BY a", 10, 0),
    ("SELECT offset FROM t WHERE offset > 2 ORDER BY offset LIMIT 4 OFFSET 1", 4, 1),
])
def test_offset_parsing(sql, limit, offset):
    qc = parse(sql)
    assert (qc.limit, qc.offset) == (limit, offset)


def test_offset_needs_a_number():
    with pytest.raises(ValueError):
        parse("SELECT a FROM t LIMIT 3 OFFSET")


@pytest.mark.parametrize("sql, want", [
    ("SELECT a, b FROM t ORDER BY c, a", ["c", "a", "b"]),                       # an order-by expression not selected
    ("SELECT a, b, a FROM t ORDER BY b DESC, b, a", ["b", "a"]),                 # duplicates on both sides
    ("SELECT * FROM t ORDER BY c DESC", ["c", "a", "b", "d"]),                   # '*' sorted by name, '$' columns out
    ("SELECT a, b + c FROM t ORDER BY b + c, d", ["plus(b,c)", "d", "a"]),
    ("SELECT a, b FROM t", ["a", "b"]),
    ("SELECT a, b FROM t ORDER BY c LIMIT 0", ["a", "b"]),                       # LIMIT 0 ignores ORDER BY
])
def test_block_expression_order(sql, want):
    qc = parse(sql)
    assert [str(e) for e in qc.selection_block_expressions(["d", "b", "$docId", "a", "c"])] == want
    assert [str(e) for e in qc.select_expressions(["d", "b", "$docId", "a", "c"])] == \
        [str(e) for e in parse(sql.split(" ORDER BY ")[0]).select_expressions(["d", "b", "$docId", "a", "c"])]


# ---- the restatement against Pinot's known answers ----------------------------------------------------------------
def test_double_compare_key_is_double_compare():
    nan2 = float.fromhex("nan")
    vals = [float("-inf"), -1.5, -5e-324, -0.0, 0.0, 5e-324, 2.0, float("inf"), float("nan")]
    keys = [double_compare_key(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    import struct
    neg_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]
    assert double_compare_key(neg_nan) == double_compare_key(nan2)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: f"{c['test']}-{'filter' if c['filtered'] else 'all'}")
def test_restatement_matches_known_answers(case):
    raw = fixtures.test_data_sv_segment()
    blk = restate(golden_sql(case), [raw])
    assert len(blk.column_names) == case["num_columns"]
    assert blk.column_names[:2] == ["column6", "column1"]
    assert blk.column_types[:2] == ["INT", "INT"]
    assert blk.num_rows == case["num_rows"]
    last = dict(zip(blk.column_names, blk.rows[-1]))
    for k, v in case["last_row"].items():
        assert last[k] == v
    s = blk.stats
    assert s.num_docs_scanned == case["num_docs_scanned"]
    assert s.num_entries_scanned_post_filter == case["num_entries_scanned_post_filter"]
    assert s.num_total_docs == case["num_total_docs"]
    keys = [(r[0], r[1]) for r in blk.rows]
    assert keys == sorted(keys)


# ---- the order-by reduce -----------------------------------------------------------------------------------------
def _block(names, types, rows):
    return SelectionResultsBlock(names, types, [[r[j] for r in rows] for j in range(len(names))], ExecutionStatistics())


def test_order_by_reduce_offset_limit_and_select_mapping():
    qc = parse("SELECT s, a FROM t ORDER BY d DESC, a LIMIT 3 OFFSET 2")
    names, types = ["d", "a", "s"], ["DOUBLE", "INT", "STRING"]
    b0 = _block(names, types, [[float("nan"), 1, "x0"], [2.5, 1, "x1"], [0.0, 7, "x2"], [-0.0, 3, "x3"]])
    b1 = _block(names, types, [[float("nan"), 0, "y0"], [2.5, 1, "y1"], [0.0, 2, "y2"], [float("-inf"), 1, "y3"]])
    out = reduce_mod.reduce_blocks(qc, [b0, b1])
    assert out.columns == ["s", "a"]
    # merged: (nan,0,y0) (nan,1,x0) (2.5,1,x1) (2.5,1,y1) (0.0,2,y2) (0.0,7,x2) (-0.0,3,x3) (-inf,1,y3)
    assert out.rows == [["x1", 1], ["y1", 1], ["y2", 2]]
    all_rows = reduce_mod.reduce_blocks(parse("SELECT s, a FROM t ORDER BY d DESC, a LIMIT 100"), [b0, b1]).rows
    assert [r[0] for r in all_rows] == ["y0", "x0", "x1", "y1", "y2", "x2", "x3", "y3"]


def test_order_by_reduce_star_keeps_block_order_and_strings_compare_as_utf16():
    qc = parse("SELECT * FROM t ORDER BY s LIMIT 10")
    names, types = ["s", "a"], ["STRING", "INT"]
    # U+FF5E (one UTF-16 unit 0xFF5E) sorts after U+1F600 (surrogates 0xD83D ...) in String.compareTo, before it
    # in code-point / UTF-8 order
    b0 = _block(names, types, [["～", 1]])
    b1 = _block(names, types, [["\U0001F600", 2], ["a", 3]])
    out = reduce_mod.reduce_blocks(qc, [b0, b1])
    assert out.columns == ["s", "a"]
    assert out.rows == [["a", 3], ["\U0001F600", 2], ["～", 1]]


def test_selection_only_reduce_is_unchanged():
    qc = parse("SELECT a FROM t LIMIT 3")
    b = _block(["a"], ["INT"], [[5], [4], [9]])
    assert reduce_mod.reduce_blocks(qc, [b, b]).rows == [[5], [4], [9]]


# ---- the leaf stage's lookup by expression name -------------------------------------------------------------------
def test_leaf_stage_maps_an_order_by_block_to_the_select_list():
    blk = _block(["d", "a", "s"], ["DOUBLE", "INT", "STRING"], [[1.5, 1, "x"], [2.5, 2, "y"]])
    qc = parse("SELECT s, a FROM t ORDER BY d, a")
    exprs = [e for e, _ in qc.select]
    tb = compose_select_transferable_block(blk, exprs, DataSchema(["s", "a"], ["STRING", "LONG"]))
    assert tb.rows == [["x", 1], ["y", 2]]
    assert tb.schema.column_names == ["s", "a"]
