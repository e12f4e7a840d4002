"""Small fused scans (runtime.cpp small_shape, pinot_amd/csrc/fused_shape.h): a fused aggregation of at most a few
thousand tiles takes the launch shape with the fewest tiles per wave at which every workgroup is resident at once, in
whichever of its two modes (value columns streamed with the tile / matched docs deferred and gathered) spreads wider,
and a wave may run in a single ring slot (PHIP_FILTER_NBUF=1 forces that depth). Everything a caller sees must stay
what the CPU oracle (oracle/executor.py over the same raw segments) computes.

Compared exactly: counts; int64 sums of wide random values (a lost or doubled doc shows); the sum of a DOUBLE column of
multiples of 0.25 below 2^30, bit for bit; numDocsScanned; the matched docs per segment.

Three segments of 5000, 2048 and 9 docs (a partial last tile, a one-tile segment, a sub-tile segment: 5 tiles) and one
whose dictionary holds no value of the quantity leaf, which the planner drops. The filter has the headline's shape:
bit-sliced range leaves over an 11-value and a 50-value column, the first also an operand of SUM(a * b). `cut` adds a
sorted doc-range leaf that starts inside the first tile; `empty` matches no doc of the 5000-doc segment's second tile.

Every case runs streamed and deferred, in the general and the lean instantiation, in record mode and with the finalize
launch, at the rule's ring depth and in a single slot. Under PHIP_GRID_CUS=1 with PHIP_FILTER_NBUF=1 the three segments
eight times over (40 tiles, 24 work-list entries) run on 8 workgroups: 32 waves, so waves walk two tiles and cross a
segment change through their one slot."""
import struct

import numpy as np
import pytest

from oracle import executor
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType

pytestmark = pytest.mark.gpu

SEGMENT_DOCS = (5000, 2048, 9)
AGGS = "SUM(a * b), SUM(l), SUM(d), COUNT(*)"
CASES = {
    "headline": f"SELECT {AGGS} FROM t WHERE b BETWEEN 4 AND 6 AND q BETWEEN 26 AND 35",
    # docs 800 .. 3599 of a segment: the range starts inside tile 0 and ends inside tile 1 (tile 2 is pruned)
    "cut": f"SELECT {AGGS} FROM t WHERE ts BETWEEN 2 AND 8 AND b BETWEEN 4 AND 6 AND q BETWEEN 26 AND 35",
    # q is below 40 throughout docs 2048 .. 4095 of the 5000-doc segment
    "empty": f"SELECT {AGGS} FROM t WHERE b BETWEEN 4 AND 6 AND q BETWEEN 40 AND 45",
}
SWITCHES = ("PHIP_STREAM_VALUES", "PHIP_FUSED_LEAN", "PHIP_HOST_FINAL", "PHIP_FILTER_NBUF", "PHIP_GRID_CUS", "PHIP_FILTER_BPC",
            "PHIP_FUSED_SMALL", "PHIP_FUSED_DEFER", "PHIP_FUSE", "PHIP_FILTER_WALK", "PHIP_POLL_DONE", "PHIP_FOLD_FINAL")


def _segment(name, n, rng, dropped=False):
    c = SegmentCreator(name)
    b = rng.integers(0, 11, n)
    b[:11] = np.arange(11)[:n]  # (every id occurs where the segment is long enough)
    c.add_column("b", DataType.INT, b)
    q = rng.integers(0, 50, n)
    q[2048:4096] = rng.integers(0, 40, max(0, min(n, 4096) - 2048))
    q[:2] = (30, 42)  # (both quantity ranges occur in every kept segment: no leaf folds to match-none)
    if dropped:
        q = rng.integers(0, 20, n)  # no value of either quantity range: a match-none leaf, the segment is dropped
    c.add_column("q", DataType.INT, q)
    c.add_column("ts", DataType.INT, np.arange(n, dtype=np.int64) // 400)  # sorted
    c.add_column("a", DataType.INT, rng.integers(0, 1 << 24, n))
    # (|l| x the docs of eight copies stays below 2^58, so the library sums in int64 and not in double)
    c.add_column("l", DataType.LONG, rng.integers(-10 ** 12, 10 ** 12, n))
    c.add_column("d", DataType.DOUBLE, rng.integers(0, 1 << 32, n) * 0.25)  # multiples of 0.25 below 2^30
    return c.build()


def _raws(copy):
    rng = np.random.default_rng(1212)  # (every copy holds the same docs)
    return [_segment(f"fs{copy}_{i}", n, rng) for i, n in enumerate(SEGMENT_DOCS)] + \
           [_segment(f"fs{copy}_dropped", 100, rng, dropped=True)]


def _fixture(copies):
    from pinot_amd.engine.segment import GpuSegment
    raws = [r for k in range(copies) for r in _raws(k)]
    segs = [GpuSegment(r) for r in raws]
    yield raws, segs
    for s in segs:
        s.destroy()


@pytest.fixture(scope="module")
def small(gpu_lib):
    yield from _fixture(1)


@pytest.fixture(scope="module")
def small8(gpu_lib):
    yield from _fixture(8)


_ORACLE = {}


def _oracle(sql, raws):
    """(query, oracle block, exact sums, matched docs per segment): computed once per (query, segment count) and left
    unchanged."""
    key = (sql, len(raws))
    if key not in _ORACLE:
        qc = parse(sql)
        oblk, ex = executor.execute(qc, raws)
        matched = [int(np.count_nonzero(executor.filter_mask(qc, r))) for r in raws]
        _ORACLE[key] = (qc, oblk, ex, matched)
    return _ORACLE[key]


def _core(op):
    from pinot_amd.engine.plan import GpuCombineOperator
    while not isinstance(op, GpuCombineOperator):
        op = getattr(op, "one_pass", None) or op.__dict__.get("inner") or op.__dict__["op"]
    return op


def _bits(x):
    return struct.pack("<d", float(x))


def _run(monkeypatch, sql, small, env):
    """One plan under env, executed twice: both executions equal the oracle. Returns the launch shape."""
    from pinot_amd import _lib
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    from tests.test_gpu_parity import _assert_intermediates_equal
    raws, segs = small
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PHIP_KERNEL_TIMING", "0")  # no timing markers: how a server runs (the record mode needs it)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    qc, oblk, ex, matched = _oracle(sql, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    try:
        core = _core(op)
        for _ in range(2):
            blk = op.next_block()
            assert blk.fused, "the planner did not fuse"
            assert blk.stats.num_docs_scanned == oblk.stats.num_docs_scanned == sum(matched)
            _assert_intermediates_equal(qc.aggregations, blk.results, oblk.results, ex)
            assert isinstance(blk.results[0], int) and blk.results[0] == ex[0]  # SUM(a * b): exact int64
            assert isinstance(blk.results[1], int) and blk.results[1] == ex[1]  # SUM(l)
            assert _bits(blk.results[2]) == _bits(oblk.results[2])              # SUM(d): exact in any order
            assert blk.results[3] == sum(matched)                               # COUNT(*)
            res = core.run_raw()
            try:
                r = res.contents
                assert r.num_docs_scanned == sum(matched)
                assert [int(r.segment_docs_matched[i]) for i in range(len(matched))] == matched
            finally:
                _lib.load().phip_result_free(res)
        shape = core.launch_shape()
        want_hf = 0 if env.get("PHIP_HOST_FINAL") == "0" else 1
        assert shape["host_final"] == want_hf, shape
        return shape
    finally:
        op.close()


def _env(stream, lean, **extra):
    env = {"PHIP_STREAM_VALUES": stream}
    if lean == "general":
        env["PHIP_FUSED_LEAN"] = "0"
    env.update(extra)
    return env


@pytest.mark.parametrize("lean", ["general", "lean"])
@pytest.mark.parametrize("stream", ["1", "0"], ids=["streamed", "deferred"])
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_fused_small(case, stream, lean, small, monkeypatch):
    sql = CASES[case]
    tiles = {"headline": 5, "cut": 3, "empty": 5}[case]
    # the ring depth of one workgroup per CU, which is what the rule gives a launch of fewer workgroups than CUs: the
    # deepest ring that keeps them resident (fused_shape.h)
    deepest = _run(monkeypatch, sql, small, _env(stream, lean, PHIP_FILTER_BPC="1"))["nbuf"]
    assert 2 <= deepest <= 8
    for host_final in (None, "0"):
        for nbuf in (None, "1"):
            extra = {}
            if host_final:
                extra["PHIP_HOST_FINAL"] = host_final
            if nbuf:
                extra["PHIP_FILTER_NBUF"] = nbuf
            shape = _run(monkeypatch, sql, small, _env(stream, lean, **extra))
            assert shape["total_work"] == tiles and shape["num_work_segments"] == (2 if case == "cut" else 3), shape
            assert shape["total_work"] <= shape["filter_blocks"] * 4, shape  # every wave at most one tile
            assert shape["nbuf"] == (1 if nbuf else deepest), shape
            # (a plan that streams in no segment is lean unless the general instantiation is forced)
            if stream == "0":
                assert shape["fused_lean"] == (1 if lean == "lean" else 0), shape


@pytest.mark.parametrize("case", list(CASES))
def test_gpu_fused_small_planner(case, small, monkeypatch):
    """The planner's own choice of mode (no PHIP_STREAM_VALUES): one-tile waves either way, so the density rule's
    mode stays, at the same depth."""
    shape = _run(monkeypatch, CASES[case], small, {})
    assert shape["total_work"] <= shape["filter_blocks"] * 4 and shape["filter_blocks"] == 8, shape
    assert shape["nbuf"] == _run(monkeypatch, CASES[case], small, {"PHIP_FILTER_BPC": "1"})["nbuf"], shape
    assert _run(monkeypatch, CASES[case], small, {"PHIP_FILTER_NBUF": "1"})["nbuf"] == 1


@pytest.mark.parametrize("host_final", ["record", "finalize"])
@pytest.mark.parametrize("lean", ["general", "lean"])
@pytest.mark.parametrize("stream", ["1", "0"], ids=["streamed", "deferred"])
@pytest.mark.parametrize("case", ["headline", "empty"])
def test_gpu_fused_small_single_slot_long_waves(case, stream, lean, host_final, small8, monkeypatch):
    """40 tiles over 8 workgroups in a single slot: a wave's second tile reuses the slot of its first, across a
    segment change for most waves."""
    extra = {"PHIP_GRID_CUS": "1", "PHIP_FILTER_NBUF": "1"}
    if host_final == "finalize":
        extra["PHIP_HOST_FINAL"] = "0"
    shape = _run(monkeypatch, CASES[case], small8, _env(stream, lean, **extra))
    assert shape["total_work"] == 40 and shape["filter_blocks"] == 8 and shape["num_work_segments"] == 24, shape
    assert shape["total_work"] > shape["filter_blocks"] * 4 and shape["nbuf"] == 1, shape
