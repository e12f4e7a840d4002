"""The lean fused instantiation (filter_kernel.h kBsDefer: bit-sliced conjunction + deferred gathers only) against the
CPU oracle, at the shapes where its per-wave state can go wrong.

Every case runs under three settings and must give oracle/executor.py's answers with one kernel doing both the filter
and the aggregation (agg_kernel_ms == 0.0):

    general   PHIP_FUSED_LEAN=0: the general fused instantiation
    sync      PHIP_FUSED_PIPE=0: the lean instantiation, every gather batch consumed where it is issued (the library
              flushes synchronously whatever the setting until a pipelined flush exists; the variant stays so that one
              is covered from its first day)
    default   the lean instantiation as the planner picks it

phip_plan_launch_shape's fused_lean says which instantiation really ran; the cases that must take the lean one assert
it, and the fallback cases assert the general one.

PHIP_GRID_CUS=1 gives the fused launch 8 workgroups = 32 waves, each a contiguous range of the work list (the XCD range
walk), so the 128 tiles of the `fill` segment are 4 tiles per wave, wave w owning docs [8192 w, 8192 (w + 1)); the
launch shape is asserted. Its filter columns k<n> hold the matching id at positions placed by construction: exactly n
docs in every wave's range, n = 0, 1, 255, 256, 257, 511, 512, 513 around the 256-doc gather batch and the 512-entry
deferred ring. PHIP_MATERIALIZE_MIN_DICT=4096 makes the value columns with a dictionary of >= 4 KiB read through their
packed doc-order values, as the headline's LO_EXTENDEDPRICE is, while the 11-entry b keeps its lane-resident dictionary.
"""
import numpy as np
import pytest

from oracle import executor
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType

pytestmark = pytest.mark.gpu

VARIANTS = {"general": {"PHIP_FUSED_LEAN": "0"}, "sync": {"PHIP_FUSED_PIPE": "0"}, "default": {}}
COUNTS = (0, 1, 255, 256, 257, 511, 512, 513)
WAVES = 32           # 8 workgroups x 4 waves at PHIP_GRID_CUS=1
TILES_PER_WAVE = 4
WAVE_DOCS = TILES_PER_WAVE * 2048
FILL_DOCS = WAVES * WAVE_DOCS


def _value_columns(c, n, rng, k):
    """The aggregated columns: dictionaries and packed-value bases differ per segment (k)."""
    c.add_column("a", DataType.INT, rng.integers(1000 * k, 1000 * k + (1 << 24), n))      # packed doc-order values
    c.add_column("l", DataType.LONG, rng.integers(-10 ** 12, 10 ** 12, n) + k)            # ... 41 bits wide
    c.add_column("d", DataType.DOUBLE, rng.integers(0, 40, n) * 0.25 - 3.0 * k)           # <= 64 entries: lane-resident
    c.add_column("e", DataType.DOUBLE, rng.integers(0, 300, n) * 0.5 + k)                 # 300 entries: gathered
    c.add_column("r", DataType.INT, rng.integers(-2 ** 31, 2 ** 31 - 1, n))               # raw, no dictionary


def _placed(n, positions):
    """A 10-bit filter column (1000 ids): id 0 at `positions`, ids 1..999 elsewhere."""
    v = (np.arange(n, dtype=np.int64) % 999) + 1
    v[np.asarray(positions, dtype=np.int64)] = 0
    return v


def _wave_positions(w, count):
    return w * WAVE_DOCS + (np.arange(count, dtype=np.int64) * WAVE_DOCS) // max(count, 1)


def _fill_raw():
    """One segment of 128 tiles. k<n>: n matches per wave range; kmix: wave w has COUNTS[w % 8]; kfull: fully matched
    tiles after and before sparse ones. b is 1..3 where any of those matches and cycles through 0..10 elsewhere, so
    `k = 0 AND b BETWEEN 1 AND 3` (the headline's shape: SUM(a * b) with b a filter column) keeps the placed counts.
    k0 matches 100 docs per wave range where b is 5: both leaves pass docs, their AND none."""
    rng = np.random.default_rng(71)
    n = FILL_DOCS
    c = SegmentCreator("lean_fill", no_dictionary_columns=["r"])
    hit = np.zeros(n, dtype=bool)
    for cnt in COUNTS[1:]:
        pos = np.concatenate([_wave_positions(w, cnt) for w in range(WAVES)])
        c.add_column(f"k{cnt}", DataType.INT, _placed(n, pos))
        hit[pos] = True
    pos = np.concatenate([_wave_positions(w, COUNTS[w % 8]) for w in range(WAVES)])
    c.add_column("kmix", DataType.INT, _placed(n, pos))
    hit[pos] = True
    # wave 0: two sparse tiles (100 docs each), a full tile, a sparse tile; wave 1: a full tile first, then sparse ones;
    # wave 2: a sparse tile, two full tiles, a sparse tile (a piece-wise append with a batch pending, twice running)
    full = []
    for w, tiles in ((0, "ssfs"), (1, "fsss"), (2, "sffs")):
        for j, kind in enumerate(tiles):
            t0 = w * WAVE_DOCS + j * 2048
            full.append(t0 + (np.arange(2048) if kind == "f" else (np.arange(100) * 2048) // 100))
    pos = np.concatenate(full)
    c.add_column("kfull", DataType.INT, _placed(n, pos))
    hit[pos] = True
    b = np.arange(n, dtype=np.int64) % 11
    b[hit] = 1 + (np.flatnonzero(hit) % 3)
    free = np.flatnonzero(~hit)
    pos0 = np.concatenate([free[(free >= w * WAVE_DOCS) & (free < (w + 1) * WAVE_DOCS)][:100] for w in range(WAVES)])
    c.add_column("k0", DataType.INT, _placed(n, pos0))
    b[pos0] = 5
    c.add_column("b", DataType.INT, b)
    c.add_column("w", DataType.INT, (np.arange(n, dtype=np.int64) * 7919) % 50000)   # 16 bits: no bit-sliced planes
    _value_columns(c, n, rng, 0)
    return c.build()


@pytest.fixture(scope="module")
def fill(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    raw = _fill_raw()
    seg = GpuSegment(raw)
    yield [raw], [seg]
    seg.destroy()


def _three_raws():
    """Three segments of 3 tiles, 5 tiles + 777 docs and 100 docs: ~15 % of the docs match k (every 7th doc), t is
    sorted (doc // 400: a sorted doc range cuts tiles), dictionaries and packed bases differ per segment. j matches
    where k does: with both leaves the planner's estimate stays sparse even for the 100-doc segment's 87-id
    dictionaries, so no value column streams with the tile and every segment defers."""
    rng = np.random.default_rng(72)
    raws = []
    for k, n in enumerate((2048 * 3, 2048 * 5 + 777, 100)):
        c = SegmentCreator(f"lean_three{k}", no_dictionary_columns=["r"])
        c.add_column("k", DataType.INT, _placed(n, np.arange(k, n, 7)))
        c.add_column("j", DataType.INT, _placed(n, np.arange(k, n, 7)))
        c.add_column("t", DataType.INT, np.arange(n, dtype=np.int64) // 400)
        b = np.arange(n, dtype=np.int64) % 11
        b[k::7] = 1 + (np.arange(k, n, 7) % 3)
        c.add_column("b", DataType.INT, b)
        _value_columns(c, n, rng, k + 1)
        raws.append(c.build())
    return raws


@pytest.fixture(scope="module")
def three(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    raws = _three_raws()
    segs = [GpuSegment(r) for r in raws]
    yield raws, segs
    for s in segs:
        s.destroy()


_ORACLE = {}


def _oracle(key, sql, raws):
    """(query, oracle block, exact sums): computed once per (segments, query) and left unchanged."""
    if (key, sql) not in _ORACLE:
        qc = parse(sql)
        oblk, ex = executor.execute(qc, raws)
        _ORACLE[(key, sql)] = (qc, oblk, ex)
    return _ORACLE[(key, sql)]


def _core(op):
    from pinot_amd.engine.plan import GpuCombineOperator
    while not isinstance(op, GpuCombineOperator):
        op = getattr(op, "one_pass", None) or op.__dict__.get("inner") or op.__dict__["op"]
    return op


def _run(monkeypatch, variant, key, sql, raws, segs, lean=True, env=None):
    """Executes sql under the variant, compares with the oracle, and returns the launch shape. lean: whether the
    planner must pick the lean instantiation when the variant leaves it the choice."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    from tests.test_gpu_parity import _assert_intermediates_equal
    for name in ("PHIP_FUSED_LEAN", "PHIP_FUSED_PIPE", "PHIP_STREAM_VALUES", "PHIP_FILTER_WALK"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    monkeypatch.setenv("PHIP_MATERIALIZE_MIN_DICT", "4096")
    for name, value in {**VARIANTS[variant], **(env or {})}.items():
        monkeypatch.setenv(name, value)
    qc, oblk, ex = _oracle(key, sql, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    try:
        blk = op.next_block()
        shape = _core(op).launch_shape()
    finally:
        op.close()
    assert blk.stats.num_docs_scanned == oblk.stats.num_docs_scanned
    _assert_intermediates_equal(qc.aggregations, blk.results, oblk.results, ex)
    assert blk.agg_kernel_ms == 0.0, "one kernel filters and aggregates"
    assert shape["fused_lean"] == (1 if lean and variant != "general" else 0), shape
    return shape, oblk


def _assert_fill_shape(shape):
    assert shape["total_work"] == WAVES * TILES_PER_WAVE and shape["filter_blocks"] * 4 == WAVES, shape


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("count", COUNTS)
def test_gpu_lean_batch_fill(count, variant, fill, monkeypatch):
    """Exactly `count` matched docs per wave: none (k0: the first leaf passes 100 docs per wave, the second none of
    them), one doc, a batch less / exactly / plus one, the ring less / exactly / plus one (ring wrap, and a final
    partial batch behind a full one)."""
    raws, segs = fill
    shape, oblk = _run(monkeypatch, variant, "fill", f"SELECT SUM(a * b) FROM t WHERE k{count} = 0 AND b BETWEEN 1 AND 3",
                       raws, segs)
    _assert_fill_shape(shape)
    assert oblk.stats.num_docs_scanned == WAVES * count


AGG_QUERIES = [
    "SELECT SUM(a - b), COUNT(*) FROM t WHERE kmix = 0 AND b BETWEEN 1 AND 3",          # NA = 2
    "SELECT SUM(d), MIN(d), MAX(d), SUM(r) FROM t WHERE kmix = 0 AND b BETWEEN 1 AND 3",  # NA = 4: DOUBLE dict, raw INT
    "SELECT SUM(e), MAX(l), SUM(l), COUNT(*) FROM t WHERE kmix = 0",                    # NA = 4: gathered dict, LONG
    "SELECT MAX(r) FROM t WHERE kmix = 0 AND b BETWEEN 2 AND 3",                        # NA = 1: raw INT
    "SELECT SUM(a * b), SUM(d * b), MIN(e) FROM t WHERE kmix = 0",                      # NA = 4 with 3 slots
]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("sql", AGG_QUERIES)
def test_gpu_lean_aggregations(sql, variant, fill, monkeypatch):
    """NA = 1, 2, 4 over waves with every batch-fill count side by side (kmix)."""
    raws, segs = fill
    shape, _ = _run(monkeypatch, variant, "fill", sql, raws, segs)
    _assert_fill_shape(shape)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_lean_full_tile_after_sparse(variant, fill, monkeypatch):
    """Tiles with all 2048 docs matched after, before and between sparse tiles: the piece-wise append of fused_defer
    with docs pending in the ring."""
    raws, segs = fill
    shape, oblk = _run(monkeypatch, variant, "fill", "SELECT SUM(a * b), COUNT(*) FROM t WHERE kfull = 0 AND b BETWEEN 1 AND 3",
                       raws, segs)
    _assert_fill_shape(shape)
    assert oblk.stats.num_docs_scanned == 4 * 2048 + 8 * 100


@pytest.mark.parametrize("walk", ["xcdc", "contig"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("sql", ["SELECT SUM(a * b) FROM t WHERE k = 0 AND j = 0 AND b BETWEEN 1 AND 3",
                                 "SELECT SUM(a - b), SUM(d), MAX(l), COUNT(*) FROM t WHERE k = 0 AND j = 0"])
def test_gpu_lean_segment_changes(sql, variant, walk, three, monkeypatch):
    """Three segments whose lane-resident dictionaries and packed bases differ. The contiguous walk gives the 10
    tiles to one workgroup's 4 waves, so two of them cross a segment change with deferred docs pending."""
    raws, segs = three
    shape, _ = _run(monkeypatch, variant, "three", sql, raws, segs, env={"PHIP_FILTER_WALK": walk})
    assert shape["total_work"] == 3 + 6 + 1 and shape["num_work_segments"] == 3, shape
    if walk == "contig":
        assert shape["filter_blocks"] == 1, shape


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_lean_single_tile(variant, three, monkeypatch):
    raws, segs = three
    shape, _ = _run(monkeypatch, variant, "three[2]", "SELECT SUM(a * b), MIN(d) FROM t WHERE k = 0 AND j = 0 AND b BETWEEN 1 AND 3",
                    raws[2:], segs[2:])
    assert shape["total_work"] == 1, shape


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_lean_no_match(variant, three, monkeypatch):
    """Both leaves match docs, their AND none (b is 1..3 wherever k matches)."""
    raws, segs = three
    _, oblk = _run(monkeypatch, variant, "three", "SELECT SUM(a * b), COUNT(*) FROM t WHERE k = 0 AND j = 0 AND b = 7", raws, segs)
    assert oblk.stats.num_docs_scanned == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_lean_sorted_range_only(variant, three, monkeypatch):
    """conj == 0: the program is a sorted doc range alone (docs 3600 .. 6399 of the 11017-doc segment), which cuts its
    first and last work tile. r has no dictionary, so nothing streams with the tile and the projection defers."""
    raws, segs = three
    shape, oblk = _run(monkeypatch, variant, "three[1]", "SELECT SUM(r), COUNT(*) FROM t WHERE t BETWEEN 9 AND 15",
                       raws[1:2], segs[1:2])
    assert shape["total_work"] == 3, shape
    assert oblk.stats.num_docs_scanned == 2800


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", ["wide-filter", "stream-values"])
def test_gpu_lean_fallback(case, variant, fill, monkeypatch):
    """Plans the lean shape does not cover keep the general fused instantiation: a filter column of more than 12 bits
    (no bit-sliced planes: the P-layout conjunction), or value columns streamed with the tile (PHIP_STREAM_VALUES=1)."""
    raws, segs = fill
    if case == "wide-filter":
        sql, env = "SELECT SUM(a * b) FROM t WHERE k257 = 0 AND w < 40000", None
    else:
        sql, env = "SELECT SUM(a * b) FROM t WHERE k257 = 0 AND b BETWEEN 1 AND 3", {"PHIP_STREAM_VALUES": "1"}
    _run(monkeypatch, variant, "fill", sql, raws, segs, lean=False, env=env)
