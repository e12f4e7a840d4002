"""Selection ORDER BY on the GPU (GpuSelectionOperator over select_order.hip) against the CPU restatement
(tests/selection_order_ref.py: the oracle's selection-only rows, stable-sorted by the Java comparators).

Every case compares the block row by row and bit for bit (doubles by their bytes, any NaN equal to any NaN), the
schema and every statistic. numEntriesScannedInFilter, which the oracle does not model, is compared with the library's
own selection-only execution of the same filter, which the existing suite pins.

Five segments: 6100, 5003, 40 (under one wave), 6999 docs -- three or four 2048-doc tiles each, ragged last tiles --
and one of 5500 docs that the filters `g < 90` and `gi < 90` never match.
"""
import ctypes
import functools
import json
import os
import struct

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine.leaf_stage import GpuLeafStageOperator
from pinot_amd.engine.plan import GpuInstancePlanMaker, QueryTimeoutError, UnsupportedOnGpu
from pinot_amd.engine.reduce import reduce_blocks
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType
from tests import fixtures
from tests.selection_order_ref import restate

pytestmark = pytest.mark.gpu

NUM_DOCS = (6100, 5003, 40, 6999, 5500)
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1


# NaN with either sign bit, the infinities, both zeros, denormals, DBL_MIN, +-DBL_MAX
SPECIAL_BITS = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0,
                1, 0x8000000000000001, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF]
# ASCII and BMP below U+E000 (U+D7FF is the last code point before the surrogates)
WORDS = ["alpha", "Alpha", "beta", "zeta", "\u00e4rger", "\u00e9clair", "\u4e2d\u6587", "\u65e5\u672c", "~tilde",
         "\ud7ff", "a", "ab", "abc"]


@functools.lru_cache(maxsize=None)
def raw_segments():
    out = []
    for k, n in enumerate(NUM_DOCS):
        rng = np.random.default_rng(20261020 + k)
        c = SegmentCreator(f"so{k}", inverted_index_columns=["gi"],
                           no_dictionary_columns=["ri", "rl", "rd", "rs"])
        g = rng.integers(0, 90, n) if k != 4 else np.full(n, 99)
        c.add_column("g", DataType.INT, g)
        c.add_column("gi", DataType.INT, g)
        c.add_column("i", DataType.INT, rng.integers(-2500, 2500, n))
        # distinct over all segments, uniform over a wide range
        c.add_column("u", DataType.INT, (rng.permutation(n).astype(np.int64) * 5 + k) * 40009 % 1000003 * 2001 + k)
        l = rng.integers(-10 ** 15, 10 ** 15, n)
        l[rng.integers(0, n, 3)] = LONG_MIN
        l[rng.integers(0, n, 3)] = LONG_MAX
        c.add_column("l", DataType.LONG, l)
        f = rng.normal(0, 100, n).astype(np.float32)
        f[rng.integers(0, n, 4)] = [np.inf, -np.inf, 0.0, np.nan]
        c.add_column("f", DataType.FLOAT, f)
        d = np.round(rng.normal(0, 50, n), 1)       # ties
        d[rng.integers(0, n, 3 * len(SPECIAL_BITS))] = np.array(SPECIAL_BITS * 3, dtype=np.uint64).view(np.float64)
        c.add_column("d", DataType.DOUBLE, d)     # (a dictionary keeps one NaN and one zero)
        c.add_column("rd", DataType.DOUBLE, d)    # raw: every bit pattern
        words = WORDS[k:] + [f"w{k}_{j}" for j in range(7 + 3 * k)]   # the segments' dictionaries differ
        c.add_column("s", DataType.STRING, np.array(words)[rng.integers(0, len(words), n)])
        c.add_column("ri", DataType.INT, rng.integers(-10 ** 9, 10 ** 9, n))
        c.add_column("rl", DataType.LONG, rng.integers(-10 ** 17, 10 ** 17, n))
        c.add_column("rs", DataType.STRING, np.array([f"row{k}-{j % 97}-{'x' * (j % 5)}" for j in range(n)]))
        c.add_column("c1", DataType.INT, np.full(n, 7))
        c.add_column("c9", DataType.INT, rng.integers(0, 9, n) * 1000)
        c.add_column("e", DataType.STRING, np.array(["plain", "smile\U0001F600"])[rng.integers(0, 2, n)])
        c.add_column("pu", DataType.STRING, np.array(["plain", "priv\ue000"])[rng.integers(0, 2, n)])
        nulls = np.zeros(n, dtype=bool)
        if k == 1:
            nulls[[5, 77, 4000]] = True
        c.add_column("nn", DataType.INT, rng.integers(0, 100, n), nulls=nulls if k == 1 else None)
        c.add_column("ts", DataType.INT, np.arange(n) // 3 + 1000 * k)   # sorted in every segment
        out.append(c.build())
    return out


@pytest.fixture(scope="module")
def segs(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    raws = raw_segments()
    g = [GpuSegment(r) for r in raws]
    yield raws, g
    for s in g:
        s.destroy()


_REF, _IN_FILTER = {}, {}


def _ref(sql, raws):
    if sql not in _REF:
        _REF[sql] = restate(sql, raws)
    return _REF[sql]


def _in_filter(qc, g, key):
    """numEntriesScannedInFilter of the library's selection-only execution of the same filter."""
    if key not in _IN_FILTER:
        from pinot_amd.query.context import Identifier, QueryContext
        first = next(iter(g[0].segment.columns))
        plain = QueryContext(qc.table, [(Identifier(first), None)], [], qc.filter, [], [], limit=1,
                             options=dict(qc.options))
        op = GpuInstancePlanMaker().make_instance_plan(plain, g)
        try:
            _IN_FILTER[key] = op.next_block().stats.num_entries_scanned_in_filter
        finally:
            op.close()
    return _IN_FILTER[key]


def _cell(v):
    if isinstance(v, (float, np.floating)):
        return b"nan" if v != v else struct.pack("<d", float(v))
    if isinstance(v, (int, np.integer)):
        return int(v)
    return v


def assert_block(blk, ref, in_filter=None):
    assert blk.column_names == ref.column_names
    assert blk.column_types == ref.column_types
    assert blk.num_rows == ref.num_rows
    for r, (a, b) in enumerate(zip(blk.rows, ref.rows)):
        assert [_cell(x) for x in a] == [_cell(x) for x in b], (r, a, b)
    s, o = blk.stats, ref.stats
    assert s.num_docs_scanned == o.num_docs_scanned
    assert s.num_entries_scanned_post_filter == o.num_entries_scanned_post_filter
    assert s.num_total_docs == o.num_total_docs
    assert s.num_segments_processed == o.num_segments_processed
    assert s.num_segments_matched == o.num_segments_matched
    if in_filter is not None:
        assert s.num_entries_scanned_in_filter == in_filter


def run(sql, segs, executions=1):
    """One plan of ``sql``: every execution equals the restatement. Returns (last block, launch shape, restatement)."""
    raws, g = segs
    qc = parse(sql)
    ref = _ref(sql, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, g)
    try:
        for _ in range(executions):
            blk = op.next_block()
            assert_block(blk, ref, _in_filter(qc, g, (id(g[0]), str(qc.filter))))
        shape = op.launch_shape()
    finally:
        op.close()
    matched = ref.stats.num_docs_scanned
    keep = qc.offset + qc.limit
    assert min(keep, matched) <= shape["select_candidates"] <= matched, shape
    if keep >= matched:
        assert shape["select_candidates"] == matched
    return blk, shape, ref


# ---- Pinot's known answers ------------------------------------------------------------------------------------------
with open(os.path.join(fixtures.GOLDEN, "selection_order_by.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def golden_seg(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    raw = fixtures.test_data_sv_segment()
    g = GpuSegment(raw)
    yield [raw], [g]
    g.destroy()


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: f"{c['test']}-{'filter' if c['filtered'] else 'all'}")
def test_known_answers(golden_seg, case):
    sql = case["sql"].replace("{filter}", GOLDEN["filter"])
    blk, _, _ = run(sql, golden_seg)
    assert len(blk.column_names) == case["num_columns"] and blk.num_rows == case["num_rows"]
    last = dict(zip(blk.column_names, blk.rows[-1]))
    for k, v in case["last_row"].items():
        assert last[k] == v
    assert blk.stats.num_docs_scanned == case["num_docs_scanned"]
    assert blk.stats.num_entries_scanned_post_filter == case["num_entries_scanned_post_filter"]
    assert blk.stats.num_total_docs == case["num_total_docs"]


@pytest.mark.parametrize("case", GOLDEN["refused"], ids=lambda c: c["sql"].split("FROM testTable ")[1])
def test_sorted_first_column_is_refused(golden_seg, case):
    with pytest.raises(UnsupportedOnGpu, match="sorted"):
        GpuInstancePlanMaker().make_instance_plan(parse(case["sql"]), golden_seg[1])


# ---- K ------------------------------------------------------------------------------------------------------------
MATCH_FEW = "g = 3 AND i < 0"   # ~100 docs


@pytest.mark.parametrize("limit", [1, 10, "matched", "more"])
def test_k(segs, limit):
    matched = _ref(f"SELECT i FROM t WHERE {MATCH_FEW} ORDER BY i LIMIT 1", segs[0]).stats.num_docs_scanned
    assert 20 < matched < 400
    n = {"matched": matched, "more": matched + 500}.get(limit, limit)
    blk, _, _ = run(f"SELECT i, l, s FROM t WHERE {MATCH_FEW} ORDER BY l DESC, i LIMIT {n}", segs)
    assert blk.num_rows == min(n, matched)


def test_nothing_matches(segs):
    blk, shape, _ = run("SELECT i, s FROM t WHERE g > 200 ORDER BY i LIMIT 10", segs)
    assert blk.num_rows == 0 and blk.stats.num_docs_scanned == 0 and shape["select_candidates"] == 0


@pytest.mark.parametrize("sql", [
    "SELECT i, rl FROM t WHERE g < 90 ORDER BY i LIMIT 20 OFFSET 35",
    "SELECT i, rl FROM t WHERE g < 90 ORDER BY i LIMIT 35, 20",
    # K cuts inside groups of fully tied rows (c9 has 9 values, c1 one): the tie rule decides
    "SELECT c9, c1, rl FROM t WHERE g < 90 ORDER BY c9, c1 LIMIT 7 OFFSET 2500",
    "SELECT c9, rl FROM t WHERE g < 50 ORDER BY c9 DESC LIMIT 5 OFFSET 1111",
])
def test_offset_and_ties_at_the_cut(segs, sql):
    blk, _, _ = run(sql, segs)
    qc = parse(sql)
    assert blk.num_rows == qc.offset + qc.limit
    assert len(reduce_blocks(qc, [blk]).rows) == qc.limit


# ---- directions, terms, expressions -----------------------------------------------------------------------------
@pytest.mark.parametrize("sql", [
    "SELECT i, l FROM t WHERE g < 90 ORDER BY i LIMIT 50",
    "SELECT i, l FROM t WHERE g < 90 ORDER BY i DESC LIMIT 50",
    "SELECT l, rs FROM t WHERE g < 90 ORDER BY c9 DESC, i, l DESC LIMIT 300",
    "SELECT c9, i FROM t WHERE g < 90 ORDER BY c9, i DESC LIMIT 300",
    "SELECT i FROM t WHERE g < 90 ORDER BY i, i DESC, c9 LIMIT 40",                  # a duplicated term
    "SELECT i, c9 FROM t WHERE g < 90 ORDER BY i, c9 LIMIT 40",                      # all block expressions ordered
    "SELECT i, c9, l, d FROM t WHERE g < 90 ORDER BY i, c9 LIMIT 40",                # partially ordered
    "SELECT s FROM t WHERE g < 90 ORDER BY u LIMIT 25",                              # order-by expression not selected
    "SELECT i, c9 FROM t WHERE g < 90 ORDER BY i + c9, i LIMIT 60",
    "SELECT l, i FROM t WHERE g < 30 ORDER BY l - i DESC LIMIT 60",
    "SELECT d, f FROM t WHERE g < 90 ORDER BY d * f, d LIMIT 200",
    "SELECT i FROM t ORDER BY i, l LIMIT 15",                                         # no filter
])
def test_terms_and_expressions(segs, sql):
    run(sql, segs)


def test_all_ordered_and_partially_ordered_statistics(segs):
    a, _, _ = run("SELECT i, c9 FROM t WHERE g < 90 ORDER BY i, c9 LIMIT 40", segs)
    p, _, _ = run("SELECT i, c9, l, d FROM t WHERE g < 90 ORDER BY i, c9 LIMIT 40", segs)
    m = a.stats.num_docs_scanned
    assert a.stats.num_entries_scanned_post_filter == 2 * m
    assert p.stats.num_entries_scanned_post_filter == 2 * m + 2 * (40 * 3 + 40)   # (the 40-doc segment matches 40 docs)


# ---- key types ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", ["i", "l", "f", "d", "rd", "s", "ri", "rl"])
@pytest.mark.parametrize("direction", ["", " DESC"])
def test_key_types(segs, col, direction):
    blk, _, ref = run(f"SELECT {col}, u FROM t WHERE g < 90 ORDER BY {col}{direction}, u LIMIT 120", segs)
    if col == "l":
        assert blk.rows[0][0] == (LONG_MAX if direction else LONG_MIN)
    if col in ("d", "rd", "f") and direction:
        assert blk.rows[0][0] != blk.rows[0][0]     # NaN first in DESC


def test_double_specials_all_rows(segs):
    """Every matched row of the raw DOUBLE column -- both NaNs, both zeros, denormals, infinities -- in order."""
    blk, _, _ = run("SELECT rd, d FROM t WHERE g < 90 ORDER BY rd, d DESC LIMIT 30000", segs)
    zeros = [struct.pack("<d", v) for v in blk.columns[0] if v == 0.0]
    assert struct.pack("<d", -0.0) in zeros and struct.pack("<d", 0.0) in zeros


def test_inverted_index_filter_leaf(segs):
    run("SELECT i, s FROM t WHERE gi = 17 ORDER BY s DESC, i LIMIT 50", segs)
    run("SELECT i, s FROM t WHERE gi IN (3, 4, 88) AND i > 0 ORDER BY i LIMIT 50", segs)


def test_string_order_uses_the_global_dictionary(segs):
    blk, _, _ = run("SELECT s, u FROM t WHERE g < 90 ORDER BY s, u LIMIT 4000", segs)
    assert len(set(blk.columns[0])) > 5


@pytest.mark.parametrize("col, why", [("e", "U\\+E000"), ("pu", "U\\+E000"), ("rs", "raw")])
def test_refused_string_terms(segs, col, why):
    with pytest.raises(UnsupportedOnGpu, match=why):
        GpuInstancePlanMaker().make_instance_plan(parse(f"SELECT i FROM t ORDER BY {col} LIMIT 5"), segs[1])


def test_raw_string_selected_under_order_by(segs):
    blk, _, _ = run("SELECT rs, e, i FROM t WHERE g < 90 ORDER BY i DESC, u LIMIT 70", segs)
    assert all(v.startswith("row") for v in blk.columns[2])


def test_other_refusals(segs):
    mk = GpuInstancePlanMaker()
    with pytest.raises(UnsupportedOnGpu, match="OFFSET"):
        mk.make_instance_plan(parse("SELECT i FROM t LIMIT 5 OFFSET 2"), segs[1])
    with pytest.raises(UnsupportedOnGpu, match="OFFSET"):
        mk.make_instance_plan(parse("SELECT COUNT(*) FROM t LIMIT 5 OFFSET 2"), segs[1])
    with pytest.raises(UnsupportedOnGpu, match="8 terms"):
        mk.make_instance_plan(parse("SELECT i FROM t ORDER BY i, l, f, d, rd, ri, rl, c9, c1 LIMIT 5"), segs[1])
    with pytest.raises(UnsupportedOnGpu, match="16"):
        mk.make_instance_plan(parse("SELECT * FROM t ORDER BY i + l, i - l, i * l LIMIT 5"), segs[1])
    with pytest.raises(UnsupportedOnGpu, match="sorted"):
        mk.make_instance_plan(parse("SELECT i FROM t ORDER BY ts, i LIMIT 5"), segs[1])
    run("SELECT i FROM t WHERE g < 90 ORDER BY i, ts DESC LIMIT 30", segs)   # a sorted column further down is a plain term


# ---- ties and the candidate count -------------------------------------------------------------------------------
def test_heavy_ties(segs):
    # one distinct value among the matched docs: every doc is a candidate (a constant column such as c1 is a sorted
    # one, which is refused as a first term)
    blk, shape, ref = run("SELECT c9, rl FROM t WHERE g < 90 AND c9 = 3000 ORDER BY c9 LIMIT 25", segs)
    assert shape["select_candidates"] == ref.stats.num_docs_scanned > 100
    blk, shape, ref = run("SELECT c1, i, rl FROM t WHERE g < 90 ORDER BY c1 + c1 DESC, i LIMIT 25", segs)
    assert shape["select_candidates"] == ref.stats.num_docs_scanned
    with pytest.raises(UnsupportedOnGpu, match="sorted"):
        GpuInstancePlanMaker().make_instance_plan(parse("SELECT rl FROM t ORDER BY c1, rl LIMIT 5"), segs[1])
    blk, shape, ref = run("SELECT c9, l FROM t WHERE g < 90 ORDER BY c9, l LIMIT 10", segs)
    assert shape["select_candidates"] < ref.stats.num_docs_scanned


def test_candidates_are_pruned(segs):
    blk, shape, ref = run("SELECT u FROM t WHERE g < 30 ORDER BY u LIMIT 10", segs)
    matched = ref.stats.num_docs_scanned
    assert 5000 < matched < 7000
    assert 10 <= shape["select_candidates"] < matched
    assert shape["select_candidates"] <= matched // 20   # 2048 digits over a uniform range: ~3 docs per digit


def test_pruning_disabled_returns_the_same(segs, monkeypatch):
    monkeypatch.setenv("PHIP_SELECT_ORDER_PRUNE", "0")
    blk, shape, ref = run("SELECT u, s FROM t WHERE g < 30 ORDER BY u DESC LIMIT 10", segs)
    assert shape["select_candidates"] == ref.stats.num_docs_scanned


# ---- determinism, long waves, null handling, deadline -------------------------------------------------------------
def test_two_executions_and_two_plans(segs):
    sql = "SELECT d, s, rs FROM t WHERE g < 90 ORDER BY c9, d DESC LIMIT 500"
    a, _, _ = run(sql, segs, executions=2)
    b, _, _ = run(sql, segs)
    for x, y in zip(a.columns, b.columns):
        assert [_cell(v) for v in x] == [_cell(v) for v in y]


def test_one_cu_grid(gpu_lib, monkeypatch):
    """PHIP_GRID_CUS=1 over the ~450 tiles and 36 segments of tests/long_waves_data.py: every wave of the pruning,
    candidate and gather walks takes 14+ tiles and several segments."""
    from pinot_amd.engine.segment import GpuSegment
    from tests import long_waves_data as lw
    raws = lw.raw_segments()
    g = [GpuSegment(r) for r in raws]
    try:
        monkeypatch.setenv("PHIP_GRID_CUS", "1")
        blk, shape, _ = run("SELECT nr, m, rs FROM t WHERE tag = 7 AND nr < 30 ORDER BY nr + tag DESC, wd, m LIMIT 300",
                            (raws, g))
        assert shape["select_blocks"] <= 8 and shape["total_work"] >= 10 * shape["select_blocks"] * 4, shape
        assert shape["num_work_segments"] >= 24, shape
    finally:
        for x in g:
            x.destroy()


def test_null_handling(segs):
    plain, _, _ = run("SELECT i, l FROM t WHERE g < 90 ORDER BY i, l LIMIT 40", segs)
    qc = parse("SET enableNullHandling = true; SELECT i, l FROM t WHERE g < 90 ORDER BY i, l LIMIT 40")
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs[1])
    try:
        blk = op.next_block()
    finally:
        op.close()
    assert_block(blk, plain)
    for sql in ("SELECT i FROM t ORDER BY nn, i LIMIT 5", "SELECT nn FROM t ORDER BY i LIMIT 5"):
        with pytest.raises(UnsupportedOnGpu, match="null"):
            GpuInstancePlanMaker().make_instance_plan(parse("SET enableNullHandling = true; " + sql), segs[1])
    run("SELECT i FROM t WHERE g < 90 ORDER BY nn, i LIMIT 5", segs)   # without the option the stored values order


def test_deadline_already_passed(segs):
    op = GpuInstancePlanMaker().make_instance_plan(parse("SELECT i FROM t WHERE g < 90 ORDER BY i LIMIT 5"), segs[1])
    try:
        op.run_raw(prepare_only=True)
        lib = _lib.load()
        res = ctypes.POINTER(_lib.Result)()
        _lib.check(lib.phip_plan_set_deadline(op._plan, 1))
        with pytest.raises(QueryTimeoutError):
            _lib.check(lib.phip_plan_execute(op._plan, ctypes.byref(res)))
    finally:
        op.close()


def test_leaf_stage_and_reduce(segs):
    sql = "SELECT s, i FROM t WHERE g < 90 ORDER BY l DESC, i LIMIT 12 OFFSET 3"
    ref = _ref(sql, segs[0])
    leaf = GpuLeafStageOperator(sql, segs[1])
    tb = leaf.next_block()
    assert tb.schema.column_names == ["s", "i"] and tb.schema.column_types == ["STRING", "INT"]
    assert tb.rows == [[r[2], r[1]] for r in ref.rows]
    assert leaf.next_block().is_end_of_stream
    blk, _, _ = run(sql, segs)
    table = reduce_blocks(parse(sql), [blk])
    assert table.columns == ["s", "i"] and table.rows == [[r[2], r[1]] for r in ref.rows[3:15]]
