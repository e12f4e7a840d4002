"""SELECT DISTINCT on the GPU (distinct_rows.hip) against the numpy restatement of its rule in tests/distinct_rows_ref.py:
every result equals the rule exactly -- rows, order and types -- and also has the weaker property that ties the rule
to the reference: the rows are distinct, lie inside the true distinct set, and their order-by projections are the
true top-`limit` projections.

Three segments of 5000 / 5003 / 4999 docs (three 2048-doc tiles each, the last partial) whose dictionaries differ, so
every id goes through the query-global remap. `a, s` is 600 key bits (not a multiple of 32: the last word is partial)
and lands in the LDS regime, `a, s, w` (~1.8 M bits, ~55 pick chunks) in the global bitmap, `u, w, a` (above 2^31 bits)
in sorted keys; PHIP_DISTINCT_LDS_WORDS=0 and a tiny PHIP_DISTINCT_ROWS_MAX_BYTES push the small queries through the
other two. The `grid` fixture repeats the main cases with PHIP_GRID_CUS=1 (8 pick workgroups striding over the chunks,
several each), and test_several_tiles_and_segments_per_wave runs twelve segments on that grid, where a wave walks
several tiles and crosses segment boundaries."""
import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine.plan import GpuDistinctOperator, GpuInstancePlanMaker, UnsupportedOnGpu, distinct_rows_plan
from pinot_amd.engine.reduce import reduce_blocks
from pinot_amd.engine.results import DistinctResultsBlock
from pinot_amd.engine.segment import GpuSegment
from pinot_amd.query.sql import parse
from tests import distinct_rows_ref as ref

pytestmark = pytest.mark.gpu
LDS, GLOBAL, SORTED = _lib.DISTINCT_ROWS_LDS, _lib.DISTINCT_ROWS_GLOBAL, _lib.DISTINCT_ROWS_SORTED
_NP = {"INT": np.int32, "LONG": np.int64, "DOUBLE": np.float64}


@pytest.fixture(scope="module")
def data(gpu_lib):
    segs = ref.make_segments()
    gs = [GpuSegment(s.build(f"dr{k}")) for k, s in enumerate(segs)]
    yield segs, gs
    for g in gs:
        g.destroy()


@pytest.fixture(params=[None, "1"], ids=["grid", "grid1"])
def grid(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("PHIP_GRID_CUS", request.param)
    return request.param


# name -> (WHERE clause, numpy mask over all docs in query order)
def _filters(segs):
    col = {c: ref.column(segs, c) for c in ("a", "inv", "srt", "w", "s", "d")}
    n = len(col["a"])
    return {
        "all": (None, np.ones(n, bool)),
        "all_pred": ("a >= 0", np.ones(n, bool)),
        "none_folded": ("w = 12345", np.zeros(n, bool)),                      # not a dictionary value: no work at all
        "none": ("a = 49 AND inv = 0 AND srt = 0", (col["a"] == 49) & (col["inv"] == 0) & (col["srt"] == 0)),
        "one_percent": ("inv = 3 AND a < 6", (col["inv"] == 3) & (col["a"] < 6)),
        "scan": ("a BETWEEN 10 AND 30", (col["a"] >= 10) & (col["a"] <= 30)),     # scan leaf
        "inverted": ("inv IN (2, 7)", np.isin(col["inv"], [2, 7])),              # inverted-index leaf
        "sorted": ("srt BETWEEN 5 AND 20", (col["srt"] >= 5) & (col["srt"] <= 20)),  # sorted-index leaf
        "mixed": ("srt > 8 AND (inv = 1 OR d < -2.0)", (col["srt"] > 8) & ((col["inv"] == 1) | (col["d"] < -2.0))),
    }


def _sql(cols, where, order, limit):
    q = "SELECT DISTINCT " + ", ".join(cols) + " FROM t"
    if where:
        q += " WHERE " + where
    if order:
        q += " ORDER BY " + ", ".join(f"{c} DESC" if d else c for c, d in order)
    if limit is not None:
        q += f" LIMIT {limit}"
    return q


def _verify(blk, segs, cols, mask, order, limit):
    """The block against the rule (exactly) and against the reference's freedom (the weaker property)."""
    k = 10 if limit is None else limit
    want = ref.distinct_rows(segs, cols, mask, order, k)
    assert isinstance(blk, DistinctResultsBlock)
    assert blk.column_names == list(cols) and blk.column_types == [ref.TYPES[c] for c in cols]
    for c, v in zip(cols, blk.columns):
        if ref.TYPES[c] == "STRING":
            assert all(type(x) is str for x in v)
        else:
            assert isinstance(v, np.ndarray) and v.dtype == _NP[ref.TYPES[c]], (c, getattr(v, "dtype", type(v)))
    got = [tuple(r) for r in blk.rows]
    assert got == want, (got[:5], want[:5], len(got), len(want))
    # the weaker property: distinct rows of the true distinct set, with the true top-`limit` order-by projections
    truth = ref.true_distinct_set(segs, cols, mask)
    assert len(set(got)) == len(got) == min(k, len(truth)) and set(got) <= truth
    top = ref.top_projections(segs, cols, mask, order, k)
    if top is not None:
        assert [tuple(r[cols.index(c)] for c, _ in order) for r in got] == top
    return got


def _run(data, cols, filt="all", order=(), limit=None, regime=None):
    segs, gs = data
    where, mask = _filters(segs)[filt]
    op = GpuInstancePlanMaker().make_instance_plan(parse(_sql(cols, where, order, limit)), gs)
    try:
        assert isinstance(op, GpuDistinctOperator)
        blk = op.next_block()
        got = _verify(blk, segs, cols, mask, order, limit)
        shape = op.launch_shape()
        if regime is not None:
            assert shape["distinct_rows_regime"] == regime, shape
        # the regime is the one the pure function predicts from the cardinalities
        terms = [(cols.index(c), d) for c, d in order]
        assert shape["distinct_rows_regime"] == distinct_rows_plan(ref.cardinalities(segs, cols), terms)["regime"]
        assert blk.stats.num_docs_scanned == int(mask.sum())
        assert blk.stats.num_entries_scanned_post_filter == int(mask.sum()) * len(cols)
        return got, blk, shape
    finally:
        op.close()


# ---- the data is what the docstrings say ---------------------------------------------------------------------------------
def test_data_shapes(data):
    segs, gs = data
    cards = dict(zip(ref.TYPES, ref.cardinalities(segs, list(ref.TYPES))))
    assert cards["a"] == 50 and cards["s"] == 12 and cards["d"] == 40 and cards["one"] == 1 and cards["inv"] == 12
    assert 2900 <= cards["w"] <= 3000 and cards["u"] >= sum(ref.SIZES) - 12 and cards["u"] < sum(ref.SIZES)
    assert cards["a"] * cards["s"] == 600 and 600 % 32 != 0
    assert cards["u"] * cards["w"] * cards["a"] > 2 ** 31
    for g, s in zip(gs, segs):  # per-segment dictionaries differ from the query-global ones
        assert g.column_metadata("a").cardinality == 48 and g.column_metadata("s").cardinality == 10
        assert g.column_metadata("srt").is_sorted and (ref.column([s], "d") < 0).any()
    f = _filters(segs)
    assert f["none"][1].sum() == 0 and f["none_folded"][1].sum() == 0
    assert 0.005 < f["one_percent"][1].mean() < 0.02


# ---- columns, regimes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [["a"], ["s"], ["a", "s"], ["d", "w"], ["a", "s", "d", "one"]], ids="-".join)
def test_one_two_and_four_columns(data, grid, cols):
    _, _, shape = _run(data, cols, limit=100000)
    assert shape["distinct_rows_regime"] in (LDS, GLOBAL)


def test_lds_regime_partial_last_word(data, grid):
    got, _, _ = _run(data, ["a", "s"], limit=1000, regime=LDS)
    assert len(got) == 600  # every (a, s) pair occurs: bits 0 .. 599, the last word 24 bits full


def test_same_query_in_the_global_regime(data, grid, monkeypatch):
    monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", "0")
    _run(data, ["a", "s"], limit=1000, regime=GLOBAL)
    _run(data, ["a", "s"], "one_percent", order=[("s", True)], limit=7, regime=GLOBAL)


def test_global_regime_many_chunks(data, grid):
    got, _, shape = _run(data, ["a", "s", "w"], limit=100000, regime=GLOBAL)
    assert len(got) > 14000  # nearly every doc is its own row: keys spread over all ~55 chunks
    if grid:  # the pick kernels' grids follow PHIP_GRID_CUS: 8 workgroups stride over the chunks, ~7 each
        segs, _ = data
        assert shape["select_blocks"] == 8 < distinct_rows_plan(ref.cardinalities(segs, ["a", "s", "w"]), [])["words"] // 1024


# ---- long waves: several tiles and segments per wave ------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_data(gpu_lib):
    """The three segments four times over (12 segments, 36 tiles): with PHIP_GRID_CUS=1 the mark kernel runs on 4 (LDS)
    or 8 workgroups, so a wave walks 2-3 tiles and most waves cross a segment boundary."""
    segs = ref.make_segments() * 4
    gs = [GpuSegment(s.build(f"drl{k}")) for k, s in enumerate(segs)]
    yield segs, gs
    for g in gs:
        g.destroy()


@pytest.mark.parametrize("env,regime", [({}, LDS), ({"PHIP_DISTINCT_LDS_WORDS": "0"}, GLOBAL),
                                        ({"PHIP_DISTINCT_LDS_WORDS": "0", "PHIP_DISTINCT_ROWS_MAX_BYTES": "4"}, SORTED)],
                         ids=["lds", "global", "sorted"])
def test_several_tiles_and_segments_per_wave(long_data, monkeypatch, env, regime):
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for filt, order, limit in (("all", [("s", True)], 1000), ("one_percent", [], 1000), ("sorted", [("a", False)], 17)):
        _, _, shape = _run(long_data, ["a", "s"], filt, order, limit, regime=regime)
        assert shape["total_work"] <= 36 and shape["num_work_segments"] > 3
        if filt == "all":  # more tiles than waves: a wave's range holds several tiles, 3-tile segments end inside it
            assert shape["distinct_blocks"] == (4 if regime == LDS else 8)
            assert shape["total_work"] == 36 > 4 * shape["distinct_blocks"]  # (4 waves per workgroup)


def test_sorted_keys_naturally(data, grid):
    got, _, _ = _run(data, ["u", "w", "a"], limit=100000, regime=SORTED)
    assert len(got) > 14900
    _run(data, ["u", "w", "a"], "scan", order=[("w", True), ("a", False)], limit=33, regime=SORTED)
    _run(data, ["u", "w", "a"], "none", limit=5, regime=SORTED)


@pytest.mark.parametrize("cols,order", [(["a", "s"], ()), (["a", "s"], (("s", True),)), (["d"], (("d", True),)),
                                        (["a", "s", "d", "one"], (("d", False), ("a", True)))],
                         ids=["a-s", "a-s-by-s-desc", "d-desc", "four"])
def test_small_queries_forced_into_sorted_keys(data, grid, monkeypatch, cols, order):
    monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", "0")
    monkeypatch.setenv("PHIP_DISTINCT_ROWS_MAX_BYTES", "4")
    for filt, limit in (("all", 1000), ("one_percent", 10), ("none", 10)):
        _run(data, cols, filt, order, limit, regime=SORTED)


# ---- ORDER BY ------------------------------------------------------------------------------------------------------------
ORDERS = [
    (["a", "s"], [("a", False)]),
    (["a", "s"], [("a", True)]),
    (["a", "s", "d"], [("s", True), ("a", False)]),       # a subset of the columns, STRING first
    (["a", "s", "d"], [("d", True)]),                     # the last select column alone, descending
    (["s", "w"], [("s", False), ("w", True)]),            # every column a term
    (["s"], [("s", True)]),
    (["w", "a"], [("a", False)]),                         # the second column orders, the first breaks ties ascending
    (["d", "one", "a"], [("one", True), ("d", False)]),   # a one-value term
]


@pytest.mark.parametrize("cols,order", ORDERS, ids=[",".join(c) + " by " + ",".join(o + ("-" if d else "+") for o, d in t)
                                                    for c, t in ORDERS])
def test_order_by(data, grid, cols, order):
    for limit in (None, 37):
        _run(data, cols, "scan", order, limit)


# ---- filters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["all", "all_pred", "none_folded", "none", "one_percent", "scan", "inverted", "sorted",
                                  "mixed"])
def test_filters(data, grid, filt):
    got, blk, _ = _run(data, ["a", "s"], filt, [("s", False)], 1000)
    if filt.startswith("none"):
        assert got == [] and blk.num_rows == 0 and blk.stats.num_docs_scanned == 0
    _run(data, ["inv", "d", "srt"], filt, [("srt", True)], 50)


def test_filters_through_the_other_regimes(data, monkeypatch):
    monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", "0")
    for filt in ("none", "one_percent", "inverted", "sorted"):
        _run(data, ["a", "s"], filt, [("a", True)], 1000, regime=GLOBAL)
    monkeypatch.setenv("PHIP_DISTINCT_ROWS_MAX_BYTES", "4")
    for filt in ("none_folded", "inverted", "sorted"):
        _run(data, ["a", "s"], filt, [("a", True)], 1000, regime=SORTED)


# ---- LIMIT ---------------------------------------------------------------------------------------------------------------
def _limits(segs, cols, mask, order):
    keys = ref.keys(segs, cols, mask, order)
    words = keys >> 5
    first_word = int((words == words[0]).sum())           # the popcount of the first non-empty word
    chunk = keys >> 15                                       # 1024 words of 32 keys
    later = np.nonzero(chunk > chunk[0])[0]
    inside = int(later[len(later) // 2]) + 1 if len(later) > 2 else None  # a rank that falls inside a later chunk
    return [1, first_word, inside, len(keys), len(keys) + 1, None]


@pytest.mark.parametrize("cols,filt,order,env", [
    (["a", "s"], "scan", (("s", True),), {}),                                              # LDS
    (["a", "s", "w"], "all", (), {}),                                                      # global, ~55 chunks
    (["a", "s", "w"], "mixed", (("w", True), ("a", False)), {}),
    (["a", "s", "w"], "scan", (("s", False),), {"PHIP_DISTINCT_ROWS_MAX_BYTES": "4"}),     # sorted keys
], ids=["lds", "global", "global-ordered", "sorted"])
def test_limits(data, grid, monkeypatch, cols, filt, order, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    segs, _ = data
    limits = _limits(segs, cols, _filters(segs)[filt][1], list(order))
    assert limits[1] >= 1 and limits[3] > 1
    if cols == ["a", "s", "w"] and not env:
        assert limits[2] is not None  # (the many-chunk cases do have a later chunk)
    for limit in limits[:5]:
        if limit is not None:
            got, _, _ = _run(data, cols, filt, list(order), limit)
            assert len(got) == min(limit, limits[3])
    got, _, _ = _run(data, cols, filt, list(order), None)  # no LIMIT: the default of 10
    assert len(got) == min(10, limits[3])


# ---- re-execution: a stale bitmap must show ------------------------------------------------------------------------------
@pytest.mark.parametrize("env,regime", [({}, LDS), ({"PHIP_DISTINCT_LDS_WORDS": "0"}, GLOBAL),
                                        ({"PHIP_DISTINCT_LDS_WORDS": "0", "PHIP_DISTINCT_ROWS_MAX_BYTES": "4"}, SORTED)],
                         ids=["lds", "global", "sorted"])
def test_same_plan_twice_then_another_filter(data, grid, monkeypatch, env, regime):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    segs, gs = data
    f = _filters(segs)
    cols, order = ["a", "s"], [("a", True)]
    op = GpuInstancePlanMaker().make_instance_plan(parse(_sql(cols, f["all"][0], order, 1000)), gs)
    op2 = GpuInstancePlanMaker().make_instance_plan(parse(_sql(cols, f["one_percent"][0], order, 1000)), gs)
    try:
        first = _verify(op.next_block(), segs, cols, f["all"][1], order, 1000)
        assert _verify(op.next_block(), segs, cols, f["all"][1], order, 1000) == first  # the same plan again
        assert op.launch_shape()["distinct_rows_regime"] == regime
        # a selective plan after the unselective one, then twice: bits left behind would show as extra rows
        few = _verify(op2.next_block(), segs, cols, f["one_percent"][1], order, 1000)
        assert len(few) < len(first)
        assert _verify(op2.next_block(), segs, cols, f["one_percent"][1], order, 1000) == few
        assert _verify(op.next_block(), segs, cols, f["all"][1], order, 1000) == first
    finally:
        op.close()
        op2.close()


# ---- statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["all", "one_percent", "inverted", "sorted", "none"])
def test_statistics_match_a_count_plan(data, filt):
    segs, gs = data
    where, mask = _filters(segs)[filt]
    cnt = GpuInstancePlanMaker().make_instance_plan(
        parse("SELECT COUNT(*) FROM t" + (f" WHERE {where}" if where else "")), gs)
    try:
        c = cnt.next_block()
    finally:
        cnt.close()
    assert c.results[0] == int(mask.sum())
    for order, limit in (([("a", False)], 5), ((), 100000)):
        _, blk, _ = _run(data, ["a", "s", "d"], filt, order, limit)
        s = blk.stats
        assert s.num_docs_scanned == c.stats.num_docs_scanned == int(mask.sum())
        assert s.num_entries_scanned_post_filter == 3 * int(mask.sum())
        assert s.num_entries_scanned_in_filter == c.stats.num_entries_scanned_in_filter
        assert s.num_total_docs == c.stats.num_total_docs == sum(ref.SIZES)
        assert s.num_segments_processed == c.stats.num_segments_processed == 3
        assert s.num_segments_matched == c.stats.num_segments_matched


# ---- budgets, reduce -----------------------------------------------------------------------------------------------------
def test_sort_budget_overrun_is_refused(data, monkeypatch):
    _, gs = data
    monkeypatch.setenv("PHIP_DISTINCT_ROWS_SORT_BYTES", "100000")  # 15002 docs x 3 buffers x 8 bytes do not fit
    op = GpuInstancePlanMaker().make_instance_plan(parse("SELECT DISTINCT u, w, a FROM t LIMIT 5"), gs)
    try:
        with pytest.raises(UnsupportedOnGpu, match="PHIP_DISTINCT_ROWS_SORT_BYTES"):
            op.next_block()
    finally:
        op.close()


def test_limit_zero_and_the_reduce(data):
    segs, gs = data
    f = _filters(segs)
    q = parse(_sql(["s", "a"], f["scan"][0], [("s", True)], 0))
    blk = GpuInstancePlanMaker().make_instance_plan(q, gs).next_block()
    assert blk.num_rows == 0 and blk.column_names == ["s", "a"] and blk.column_types == ["STRING", "INT"]
    assert reduce_blocks(q, [blk]).rows == []
    # two servers over two thirds of the segments each: the broker's union equals one server over everything
    q = parse(_sql(["s", "a"], f["scan"][0], [("s", True)], 40))
    halves = []
    for part in (gs[:2], gs[1:]):
        op = GpuInstancePlanMaker().make_instance_plan(q, part)
        try:
            halves.append(op.next_block())
        finally:
            op.close()
    want = ref.distinct_rows(segs, ["s", "a"], f["scan"][1], [("s", True)], 40)
    assert [tuple(r) for r in reduce_blocks(q, halves).rows] == want
