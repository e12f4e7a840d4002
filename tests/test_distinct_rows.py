"""CPU tests of SELECT DISTINCT: the parser, the key layout and regime choice (plan.distinct_rows_plan), the broker's
reduce, the plan maker's refusals and LIMIT 0. The device path is tests/test_gpu_distinct_rows.py."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine.leaf_stage import GpuLeafStageOperator
from pinot_amd.engine.plan import GpuDistinctOperator, GpuInstancePlanMaker, UnsupportedOnGpu, distinct_rows_plan
from pinot_amd.engine.reduce import distinct_order, reduce_blocks
from pinot_amd.engine.results import DistinctResultsBlock, ExecutionStatistics
from pinot_amd.query.context import Identifier
from pinot_amd.query.sql import SqlError, parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType


# ---- parser ----------------------------------------------------------------------------------------------------------
def test_distinct_is_a_keyword_after_select():
    q = parse("SELECT DISTINCT a, b FROM t WHERE c > 3 ORDER BY a DESC LIMIT 7")
    assert q.distinct and not q.is_selection and not q.is_aggregation and not q.is_group_by
    assert [e for e, _ in q.select] == [Identifier("a"), Identifier("b")]
    assert [(ob.expression, ob.ascending) for ob in q.order_by] == [(Identifier("a"), False)]
    assert q.limit == 7 and q.filter is not None
    q = parse("select distinct a from t")
    assert q.distinct and [e for e, _ in q.select] == [Identifier("a")]
    assert q.limit == 10  # (no LIMIT: the default, as elsewhere)


def test_distinct_with_parentheses():
    q = parse("SELECT DISTINCT(a) FROM t ORDER BY a LIMIT 3")
    assert q.distinct and [e for e, _ in q.select] == [Identifier("a")] and q.limit == 3


def test_alias_in_order_by_resolves_to_the_distinct_column():
    q = parse("SELECT DISTINCT a AS x, b FROM t ORDER BY x")
    assert q.distinct and q.order_by[0].expression == Identifier("a")


def test_plain_selection_is_unchanged():
    q = parse("SELECT a, b FROM t ORDER BY a LIMIT 5")
    assert not q.distinct and q.is_selection
    q = parse("SELECT distinct FROM t")  # (a column of that name: the select item ends there)
    assert not q.distinct and [e for e, _ in q.select] == [Identifier("distinct")]


@pytest.mark.parametrize("sql,reason", [
    ("SELECT DISTINCT a, COUNT(*) FROM t", "aggregation"),
    ("SELECT DISTINCT SUM(a) FROM t", "aggregation"),
    ("SELECT DISTINCT a FROM t GROUP BY a", "GROUP BY"),
    ("SELECT DISTINCT * FROM t", r"DISTINCT \*"),
    ("SELECT DISTINCT a, b FROM t ORDER BY c", "ORDER-BY columns should be included in the DISTINCT columns"),
    ("SELECT DISTINCT a FROM t ORDER BY a + 1", "ORDER-BY columns should be included in the DISTINCT columns"),
])
def test_sql_errors(sql, reason):
    with pytest.raises(SqlError, match=reason):
        parse(sql)


# ---- key layout and regime -------------------------------------------------------------------------------------------
def test_digits_follow_the_order_by_then_the_select_order():
    p = distinct_rows_plan([50, 12, 40], [(2, True), (0, False)], lds_words=8192, max_bytes=256 << 20)
    assert p["digits"] == [2, 0, 1]  # ORDER BY terms first (first term highest), then the other columns in select order
    assert p["strides"] == [12, 1, 600] and p["desc"] == [False, False, True]
    assert p["key_space"] == 50 * 12 * 40 and p["words"] == 750 and p["regime"] == _lib.DISTINCT_ROWS_LDS
    p = distinct_rows_plan([50, 12], [], lds_words=8192, max_bytes=256 << 20)
    assert p["digits"] == [0, 1] and p["strides"] == [12, 1] and p["key_space"] == 600 and p["words"] == 19


def test_ascending_key_order_is_the_row_order():
    cards, terms = [3, 4, 2], [(1, True)]
    p = distinct_rows_plan(cards, terms, lds_words=8192, max_bytes=1 << 20)
    rows = [(a, b, c) for a in range(3) for b in range(4) for c in range(2)]

    def key(r):
        return sum((cards[k] - 1 - r[k] if p["desc"][k] else r[k]) * p["strides"][k] for k in range(3))
    by_key = sorted(rows, key=key)
    by_rule = sorted(rows, key=lambda r: (-r[1], r[0], r[2]))  # ORDER BY col1 DESC, then col0, col2 ascending
    assert by_key == by_rule and sorted(map(key, rows)) == list(range(24))


def test_regime_thresholds():
    lds, mb = 8192, 256 << 20
    assert distinct_rows_plan([8192 * 32], [], lds, mb)["regime"] == _lib.DISTINCT_ROWS_LDS
    assert distinct_rows_plan([8192 * 32 + 1], [], lds, mb)["regime"] == _lib.DISTINCT_ROWS_GLOBAL
    assert distinct_rows_plan([2 ** 31], [], lds, mb)["regime"] == _lib.DISTINCT_ROWS_GLOBAL  # exactly 256 MiB of bits
    assert distinct_rows_plan([2 ** 31 + 1], [], lds, mb)["regime"] == _lib.DISTINCT_ROWS_SORTED
    assert distinct_rows_plan([600], [], 0, mb)["regime"] == _lib.DISTINCT_ROWS_GLOBAL
    assert distinct_rows_plan([600], [], 0, 16)["regime"] == _lib.DISTINCT_ROWS_SORTED
    assert distinct_rows_plan([10 ** 6], [], 10 ** 9, mb)["regime"] == _lib.DISTINCT_ROWS_GLOBAL  # the clamp: 12288 words
    assert distinct_rows_plan([12288 * 32], [], 10 ** 9, mb)["regime"] == _lib.DISTINCT_ROWS_LDS
    assert distinct_rows_plan([2 ** 31, 2 ** 31], [], lds, mb)["key_space"] == 2 ** 62
    with pytest.raises(UnsupportedOnGpu, match="2\\^63"):
        distinct_rows_plan([2 ** 31, 2 ** 31, 2], [], lds, mb)
    assert distinct_rows_plan([0, 5], [], lds, mb)["key_space"] == 5  # (an empty dictionary counts as one value)


def test_regime_reads_the_environment(monkeypatch):
    monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", "0")
    assert distinct_rows_plan([600], [])["regime"] == _lib.DISTINCT_ROWS_GLOBAL
    monkeypatch.setenv("PHIP_DISTINCT_ROWS_MAX_BYTES", "16")
    assert distinct_rows_plan([600], [])["regime"] == _lib.DISTINCT_ROWS_SORTED


# ---- the broker's reduce ---------------------------------------------------------------------------------------------
def _block(names, types, rows):
    cols = [[r[k] for r in rows] for k in range(len(names))]
    return DistinctResultsBlock(names, types, cols, ExecutionStatistics(len(rows), 0, len(rows) * len(names), 100, 1, 1))


def test_reduce_unions_orders_and_cuts():
    q = parse("SELECT DISTINCT a, s FROM t ORDER BY s DESC LIMIT 4")
    assert distinct_order(q) == [(1, True), (0, False)]
    b1 = _block(["a", "s"], ["INT", "STRING"], [(1, "z"), (2, "z"), (5, "x")])
    b2 = _block(["a", "s"], ["INT", "STRING"], [(2, "z"), (0, "y"), (3, "x")])   # (2, "z") overlaps
    b3 = _block(["a", "s"], ["INT", "STRING"], [(9, "w")])
    t = reduce_blocks(q, [b1, b2, b3])
    assert t.columns == ["a", "s"]
    assert t.rows == [[1, "z"], [2, "z"], [0, "y"], [3, "x"]]  # s DESC, ties by a ascending; (5, "x") and (9, "w") cut
    assert t.stats.num_docs_scanned == 7 and t.stats.num_total_docs == 300


def test_reduce_without_order_by_orders_by_the_select_columns():
    q = parse("SELECT DISTINCT a, d FROM t LIMIT 3")
    b1 = _block(["a", "d"], ["INT", "DOUBLE"], [(2, -1.5), (2, 0.25)])
    b2 = _block(["a", "d"], ["INT", "DOUBLE"], [(1, 7.0), (2, -1.5)])
    assert reduce_blocks(q, [b1, b2]).rows == [[1, 7.0], [2, -1.5], [2, 0.25]]
    assert reduce_blocks(parse("SELECT DISTINCT a, d FROM t"), [b1, b2]).rows == [[1, 7.0], [2, -1.5], [2, 0.25]]


def test_reduce_descending_numbers_and_zero_signs():
    q = parse("SELECT DISTINCT d FROM t ORDER BY d DESC LIMIT 10")
    b1 = _block(["d"], ["DOUBLE"], [(0.0,), (-2.0,)])
    b2 = _block(["d"], ["DOUBLE"], [(-0.0,), (3.5,), (0.0,)])
    rows = reduce_blocks(q, [b1, b2]).rows
    assert [r[0] for r in rows] == [3.5, 0.0, -0.0, -2.0]
    assert [np.signbit(r[0]) for r in rows] == [False, False, True, True]  # Double.compare: -0.0 below 0.0, both kept


def test_reduce_limit_zero_is_the_schema():
    q = parse("SELECT DISTINCT a AS x, s FROM t LIMIT 0")
    t = reduce_blocks(q, [_block(["a", "s"], ["INT", "STRING"], [])])
    assert t.columns == ["x", "s"] and t.rows == []


# ---- the plan maker --------------------------------------------------------------------------------------------------
class _Seg:
    """The planner's view of a segment: column metadata, dictionaries and null vectors."""

    def __init__(self, seg, device=-1):
        self.segment, self.name, self.num_docs, self.device = seg, seg.name, seg.num_docs, device
        self.star_trees = []

    def has_column(self, c):
        return c in self.segment.columns

    def column_metadata(self, c):
        return self.segment.columns[c].metadata

    def has_null_vector(self, c):
        return bool(getattr(self.segment.columns[c], "null_vector", None))

    def real_specials(self, c):
        return (False, False)


def _segment(name="seg", high_string=False):
    c = SegmentCreator(name, no_dictionary_columns=["raw"])
    n = 64
    c.add_column("a", DataType.INT, np.arange(n, dtype=np.int32) % 7)
    c.add_column("b", DataType.LONG, np.arange(n, dtype=np.int64) % 5)
    c.add_column("s", DataType.STRING, np.array([("\ue000" if high_string else "v") + str(i % 3) for i in range(n)]))
    c.add_column("raw", DataType.INT, np.arange(n, dtype=np.int32))
    c.add_column("nul", DataType.INT, np.arange(n, dtype=np.int32) % 4, nulls=np.arange(n) == 5)
    c.add_column("tags", DataType.INT, [[i % 3, 9] for i in range(n)], multi_value=True)
    for k in range(9):
        c.add_column(f"c{k}", DataType.INT, np.arange(n, dtype=np.int32) % 2)
    return c.build()


@pytest.fixture(scope="module")
def seg():
    return _Seg(_segment())


REFUSALS = [
    ("SELECT DISTINCT raw FROM t", "raw \\(no-dictionary\\) column raw"),
    ("SELECT DISTINCT a, tags FROM t", "multi-value column tags"),
    ("SELECT DISTINCT a + b FROM t", "expression"),
    ("SELECT DISTINCT c0, c1, c2, c3, c4, c5, c6, c7, c8 FROM t", "more than 8 columns"),
    ("SET enableNullHandling = true; SELECT DISTINCT a, nul FROM t", "enableNullHandling: column nul holds a null"),
    ("SELECT DISTINCT a FROM t LIMIT 5 OFFSET 2", "OFFSET on a query that is not an ORDER BY selection"),
    ("SELECT DISTINCT a FROM t ORDER BY a LIMIT 2, 5", "OFFSET on a query that is not an ORDER BY selection"),
]


@pytest.mark.parametrize("sql,reason", REFUSALS, ids=[r[1][:30] for r in REFUSALS])
def test_refusals_name_their_reason(seg, sql, reason):
    with pytest.raises(UnsupportedOnGpu, match=reason):
        GpuInstancePlanMaker().make_instance_plan(parse(sql), [seg])


def test_more_refusals(seg):
    high = _Seg(_segment("high", high_string=True))
    with pytest.raises(UnsupportedOnGpu, match="U\\+E000"):
        GpuInstancePlanMaker().make_instance_plan(parse("SELECT DISTINCT a, s FROM t ORDER BY s"), [high])
    # (the same column merely selected is fine: only an ordering reads the dictionary's byte order)
    GpuInstancePlanMaker().make_instance_plan(parse("SELECT DISTINCT a, s FROM t ORDER BY a"), [high])
    with pytest.raises(UnsupportedOnGpu, match="several devices"):
        GpuDistinctOperator(parse("SELECT DISTINCT a FROM t"), [seg, _Seg(_segment("other"), device=1)])
    with pytest.raises(UnsupportedOnGpu, match="star-tree's documents"):
        GpuDistinctOperator(parse("SELECT DISTINCT a FROM t"), [seg], segment_filters=[(None, None)])
    with pytest.raises(UnsupportedOnGpu, match="multi-stage leaf stage"):
        GpuLeafStageOperator("SELECT DISTINCT a FROM t", [seg]).next_block()
    with pytest.raises(UnsupportedOnGpu, match="no segments"):
        GpuDistinctOperator(parse("SELECT DISTINCT a FROM t"), [])
    # null handling with null-free DISTINCT columns is no refusal (a null elsewhere in the segment does not matter)
    GpuInstancePlanMaker().make_instance_plan(parse("SET enableNullHandling = true; SELECT DISTINCT a, b FROM t"), [seg])


def test_dispatch_and_descriptor(seg):
    op = GpuInstancePlanMaker().make_instance_plan(parse("SELECT DISTINCT b, s, a FROM t ORDER BY a DESC, b LIMIT 9"), [seg])
    assert isinstance(op, GpuDistinctOperator)
    assert op.names == ["b", "s", "a"] and op.types == ["LONG", "STRING", "INT"]
    assert op.order_terms == [(2, True), (0, False)]


def test_limit_zero_returns_the_schema_without_the_library(seg, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("LIMIT 0 must not touch the library")
    monkeypatch.setattr(_lib, "load", no_library)
    q = parse("SELECT DISTINCT a, s FROM t ORDER BY s LIMIT 0")
    blk = GpuInstancePlanMaker().make_instance_plan(q, [seg]).next_block()
    assert isinstance(blk, DistinctResultsBlock)
    assert blk.column_names == ["a", "s"] and blk.column_types == ["INT", "STRING"] and blk.num_rows == 0
    assert blk.stats.num_docs_scanned == 0 and blk.stats.num_total_docs == seg.num_docs
    t = reduce_blocks(q, [blk, blk])
    assert t.columns == ["a", "s"] and t.rows == []


# ---- a library without the distinct-rows kernels ---------------------------------------------------------------------
_HOSTSIM_SCRIPT = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2])
    import numpy as np
    from pinot_amd import _lib
    _lib.LIB_PATH = sys.argv[1]
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    from pinot_amd.segment.creator import SegmentCreator
    from pinot_amd.spi import DataType
    rng = np.random.default_rng(0)
    c = SegmentCreator("h")
    c.add_column("a", DataType.INT, rng.integers(0, 9, 300))
    c.add_column("b", DataType.LONG, rng.integers(0, 5, 300))
    g = GpuSegment(c.build())
    for sql in ("SELECT DISTINCT a FROM t", "SELECT DISTINCT a, b FROM t WHERE a < 4 ORDER BY b DESC LIMIT 3"):
        try:
            GpuInstancePlanMaker().make_instance_plan(parse(sql), [g]).next_block()
        except _lib.PhipUnsupported as e:
            assert "distinct_rows kernels" in str(e), e
        else:
            raise SystemExit("not refused: " + sql)
    GpuInstancePlanMaker().make_instance_plan(parse("SELECT a, b FROM t WHERE a < 4 LIMIT 3"), [g]).next_block()
    print("DISTINCT HOSTSIM OK")
""")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_library_without_the_distinct_rows_kernels_refuses(tmp_path):
    """The host simulation (runtime.cpp over tests/hostsim/hip_stub.cpp, no kernel unit): no launcher is registered, so
    a distinct plan is PHIP_ERR_UNSUPPORTED at plan creation; a plain selection over the same segment still runs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libpinot_hip_hostsim_distinct.so")
    src = [os.path.join(root, "pinot_amd", "csrc", "runtime.cpp"), os.path.join(root, "pinot_amd", "csrc", "node.cpp"),
           os.path.join(root, "tests", "hostsim", "hip_stub.cpp")]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O0", "-std=c++17", "-fPIC", "-shared", "-nogpulib",
                           "-o", so] + src + ["-ldl"], stderr=subprocess.DEVNULL)
    p = subprocess.run([sys.executable, "-c", _HOSTSIM_SCRIPT, so, root], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DISTINCT HOSTSIM OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
