"""Record mode (pinot_amd/csrc/host_final.h): an aggregation-only plan run without timing markers ends with every
filter workgroup storing one tagged record into mapped host memory, and the host reduces the records in the finalize
kernel's fixed order -- no finalize launch. Everything the caller sees must be what the finalize launch gave, bit for
bit: the same query is prepared twice, once with PHIP_HOST_FINAL=0 (the finalize launch) and once with the default,
the two plans execute in turns, and values (as bit patterns), exact sums, docs scanned, entries scanned and the
per-segment matched counts are compared; the first answers are also checked against the CPU oracle.
phip_plan_launch_shape's host_final says which mode an execution really took.

The seven segments hold 1, 2047, 2048, 2049, 6000, 40 000 and 300 docs (a one-doc segment, partial last tiles, several
tiles): 29 tiles in 7 work-list entries. PHIP_GRID_CUS=1 and 2 give few, long-lived waves (several tiles and segment
changes per wave and per block, and waves with empty ranges); the device's own CU count gives more waves than tiles.

The tag counter's skip of 0 is proved on the CPU (tests/test_host_final_reduce.py: rec_next_tag, the function the
runtime advances it with); here the executions across the wrap must all be right and all in record mode."""
import struct
import threading

import numpy as np
import pytest

from oracle import executor
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType

pytestmark = pytest.mark.gpu

SEGMENT_DOCS = (1, 2047, 2048, 2049, 6000, 40_000, 300)
WHERE = "WHERE k = 0 AND j = 0"  # every 7th doc (from doc s of segment s): the bit-sliced conjunction of two leaves

# (name, sql, must a kernel launch)
CASES = [
    ("count", f"SELECT COUNT(*) FROM t {WHERE}", True),                                   # a filter-only plan
    ("na1", f"SELECT SUM(a * b) FROM t {WHERE}", True),                                   # an int64 product
    ("na2", f"SELECT SUM(d), MIN(e) FROM t {WHERE}", True),
    ("na4", f"SELECT SUM(a * b), SUM(d), MIN(e), MAX(l) FROM t {WHERE}", True),
    # a sorted doc range alone (conj == 0): docs 2000 .. 2799, which cut tiles 0 and 1 of the segments that have them
    # (few enough docs per tile that the planner fuses)
    ("range", "SELECT SUM(a * b), MAX(e) FROM t WHERE t BETWEEN 5 AND 6", True),
    ("nothing", "SELECT SUM(a * b), MIN(d) FROM t WHERE k = 0 AND j = 5", True),          # both ids exist, no doc has both
    ("pruned", "SELECT SUM(a * b), COUNT(*) FROM t WHERE t > 100000", False),             # every tile pruned: no launch
    ("specials", f"SELECT SUM(sn), SUM(si), MIN(z), MAX(z) FROM t {WHERE}", True),        # NaN; inf + -inf across blocks; zeros
    # two NaNs of different signs meet where the blocks' partials are combined: a stored NaN (0x7ff8...) in the first
    # block's segment, and the invalid sum's NaN (0xfff8...) of the +inf and -inf blocks
    ("nanmix", f"SELECT SUM(sm), MAX(e) FROM t {WHERE}", True),
]


def _placed(n, positions):
    """A 10-bit filter column (1000 ids): id 0 at `positions`, ids 1..999 elsewhere."""
    v = (np.arange(n, dtype=np.int64) % 999) + 1
    v[np.asarray(positions, dtype=np.int64)] = 0
    return v


def _segment(name, s, n, rng):
    c = SegmentCreator(name)
    hit = np.arange(s % 7, n, 7) if n > 1 else np.arange(0, 1)
    c.add_column("k", DataType.INT, _placed(n, hit))
    j = _placed(n, hit)
    j[j == 5] = 6
    if n > 20:
        j[np.arange(3, n, 7)[: n // 14]] = 5  # id 5 exists, never where k is 0 (3 != s % 7 is arranged below)
    c.add_column("j", DataType.INT, j)
    c.add_column("t", DataType.INT, np.arange(n, dtype=np.int64) // 400)  # sorted
    b = np.arange(n, dtype=np.int64) % 11
    c.add_column("b", DataType.INT, b)
    c.add_column("a", DataType.INT, rng.integers(1000 * s, 1000 * s + (1 << 24), n))
    c.add_column("l", DataType.LONG, rng.integers(-10 ** 12, 10 ** 12, n) + s)
    c.add_column("d", DataType.DOUBLE, rng.integers(0, 40, n) * 0.25 - 3.0 * s)
    c.add_column("e", DataType.DOUBLE, rng.integers(0, 300, n) * 0.5 + s)
    sn = rng.integers(0, 50, n) * 0.125
    if s == 4:
        sn[::97] = np.nan
    c.add_column("sn", DataType.DOUBLE, sn)
    si = rng.integers(0, 50, n) * 0.5
    if s == 4:
        si[::7] = np.inf       # (matched docs of segment 4 start at doc 4: 4 % 7 != 0 -- placed on them below)
        si[4::7] = np.inf
    if s == 5:
        si[5::7][-50:] = -np.inf  # the last tile of the 40 000-doc segment: never the block of a +inf, so the invalid
                                  # sum inf + -inf happens where the blocks' partials are combined
    c.add_column("si", DataType.DOUBLE, si)
    sm = si.copy()
    if s == 1:
        sm[1::7] = np.nan  # every matched doc of the 2047-doc segment
    c.add_column("sm", DataType.DOUBLE, sm)
    c.add_column("z", DataType.DOUBLE, np.full(n, -0.0 if s % 2 == 0 else 0.0))
    return c.build()


def _raws(prefix, docs, seed):
    rng = np.random.default_rng(seed)
    # (segment s matches from doc s % 7; s % 7 == 3 would meet j's id 5)
    return [_segment(f"{prefix}{i}", i if i % 7 != 3 else i + 1, n, rng) for i, n in enumerate(docs)]


def _gpu(raws):
    from pinot_amd.engine.segment import GpuSegment
    return [GpuSegment(r) for r in raws]


@pytest.fixture(scope="module")
def seven(gpu_lib):
    raws = _raws("hf_seven", SEGMENT_DOCS, 91)
    segs = _gpu(raws)
    yield raws, segs
    for s in segs:
        s.destroy()


@pytest.fixture(scope="module")
def forty(gpu_lib):
    raws = _raws("hf_forty", (2048,) * 40, 92)
    segs = _gpu(raws)
    yield raws, segs
    for s in segs:
        s.destroy()


@pytest.fixture(scope="module")
def uneven(gpu_lib):
    raws = _raws("hf_uneven", (300, 300, 300, 300_000, 300, 300, 300), 93)
    segs = _gpu(raws)
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


def _snapshot(core, nseg):
    """One execution; everything the record mode computes, doubles as bit patterns."""
    from pinot_amd import _lib
    res = core.run_raw()
    try:
        r = res.contents
        na = r.num_aggregations
        return (r.num_docs_scanned, r.num_entries_scanned_in_filter, r.num_entries_scanned_post_filter,
                r.num_segments_matched, tuple(struct.pack("<d", r.values[i]) for i in range(na)),
                tuple(r.long_values[i] for i in range(na)), tuple(r.segment_docs_matched[i] for i in range(nseg)))
    finally:
        _lib.load().phip_result_free(res)


def _env(monkeypatch, grid=None, **extra):
    for name in ("PHIP_HOST_FINAL", "PHIP_POLL_DONE", "PHIP_FUSED_LEAN", "PHIP_STREAM_VALUES", "PHIP_GRID_CUS", "PHIP_FILTER_BPC",
                 "PHIP_HOST_FINAL_TAG0", "PHIP_FOLD_FINAL", "PHIP_GRAPH", "PHIP_TOTAL_EVENTS", "PHIP_FILTER_WALK"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PHIP_KERNEL_TIMING", "0")  # no timing markers: how a server runs
    if grid is not None:
        monkeypatch.setenv("PHIP_GRID_CUS", str(grid))
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _plan(monkeypatch, qc, segs, host_final):
    """A prepared plan (the library reads PHIP_HOST_FINAL when the plan is created, by the first execution) and its
    first snapshot."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    if host_final:
        monkeypatch.delenv("PHIP_HOST_FINAL", raising=False)
    else:
        monkeypatch.setenv("PHIP_HOST_FINAL", "0")
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    core = _core(op)
    first = _snapshot(core, len(segs))
    monkeypatch.delenv("PHIP_HOST_FINAL", raising=False)
    return op, core, first


def _check_oracle(qc, op, oblk, ex, values=True):
    """values=False: the specials case, whose NaN sums no equality holds for -- its values are compared bit for bit
    with the finalize launch's (whose special values tests/test_gpu_special_doubles.py checks against the reference)."""
    from tests.test_gpu_parity import _assert_intermediates_equal
    blk = op.next_block()
    assert blk.stats.num_docs_scanned == oblk.stats.num_docs_scanned
    if values:
        _assert_intermediates_equal(qc.aggregations, blk.results, oblk.results, ex)


# the filter kernel's instantiation: the planner's choice (the one-doc segment matches densely and streams its values
# with the tile: the general fused kernel), the lean one (no segment streams: all defer), the general one by force
KERNELS = {"planner": {}, "lean": {"PHIP_STREAM_VALUES": "0"}, "general": {"PHIP_FUSED_LEAN": "0"}}


@pytest.mark.parametrize("lean", list(KERNELS))
@pytest.mark.parametrize("grid", [1, 2, None], ids=["cus1", "cus2", "device"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_host_final_ab(case, grid, lean, seven, monkeypatch):
    name, sql, launches = case
    raws, segs = seven
    _env(monkeypatch, grid, **KERNELS[lean])
    qc, oblk, ex = _oracle("seven", sql, raws)
    op_a, core_a, first_a = _plan(monkeypatch, qc, segs, host_final=False)
    op_b, core_b, first_b = _plan(monkeypatch, qc, segs, host_final=True)
    try:
        shots_a, shots_b = [first_a], [first_b]
        for _ in range(2):  # in turns, 3 executions each
            shots_a.append(_snapshot(core_a, len(segs)))
            assert core_a.launch_shape()["host_final"] == 0
            shots_b.append(_snapshot(core_b, len(segs)))
            shape = core_b.launch_shape()
            assert shape["host_final"] == (1 if launches else 0), shape
        print(name, grid, lean, shape, first_b)
        assert (shape["total_work"] > 0) == launches, shape
        if name not in ("count", "pruned") and lean != "planner":
            assert shape["fused_lean"] == (1 if lean == "lean" else 0), shape
        for s in shots_a + shots_b:
            assert s == first_a, (s, first_a)
        assert first_a[0] == oblk.stats.num_docs_scanned
        _check_oracle(qc, op_b, oblk, ex, values=name not in ("specials", "nanmix"))
    finally:
        op_a.close()
        op_b.close()


def _mode(monkeypatch, sql, raws, segs, key, grid=1, values=True, **env):
    """The mode of one execution under env, its answers checked against the oracle (values=False: the docs scanned
    alone -- a group-by block, whose groups other tests compare)."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    _env(monkeypatch, grid, **env)
    qc, oblk, ex = _oracle(key, sql, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    try:
        _check_oracle(qc, op, oblk, ex, values=values)
        return _core(op).launch_shape()["host_final"]
    finally:
        op.close()


def test_gpu_host_final_modes(seven, monkeypatch):
    raws, segs = seven
    sql = CASES[1][1]
    assert _mode(monkeypatch, sql, raws, segs, "seven") == 1
    assert _mode(monkeypatch, sql, raws, segs, "seven", PHIP_HOST_FINAL="0") == 0
    assert _mode(monkeypatch, sql, raws, segs, "seven", PHIP_POLL_DONE="0") == 0
    assert _mode(monkeypatch, sql, raws, segs, "seven", PHIP_FOLD_FINAL="1") == 0
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    _env(monkeypatch, 1)
    monkeypatch.delenv("PHIP_KERNEL_TIMING")  # timing markers on
    qc, oblk, ex = _oracle("seven", sql, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    try:
        _check_oracle(qc, op, oblk, ex)
        assert _core(op).launch_shape()["host_final"] == 0
        monkeypatch.setenv("PHIP_KERNEL_TIMING", "0")  # the same plan without them: the mode is the execution's
        _check_oracle(qc, op, oblk, ex)
        assert _core(op).launch_shape()["host_final"] == 1
    finally:
        op.close()
    assert _mode(monkeypatch, f"SELECT b, SUM(a) FROM t {WHERE} GROUP BY b", raws, segs, "seven", values=False) == 0
    assert _mode(monkeypatch, f"SELECT SUM(a * b), DISTINCTCOUNTHLL(l) FROM t {WHERE}", raws, segs, "seven") == 0


def test_gpu_host_final_k_fallback(forty, monkeypatch):
    """40 one-tile segments at PHIP_GRID_CUS=1. One workgroup per CU (PHIP_FILTER_BPC=1) walks all 40 entries: more
    than the 14 a 128-B record holds beside matched and scanned, so the plan keeps the finalize launch. At the default
    width a block touches at most 8 entries and the record mode applies."""
    raws, segs = forty
    sql = CASES[0][1]
    assert _mode(monkeypatch, sql, raws, segs, "forty", PHIP_FILTER_BPC="1") == 0
    assert _mode(monkeypatch, sql, raws, segs, "forty") == 1
    assert _mode(monkeypatch, CASES[3][1], raws, segs, "forty") == 1


def test_gpu_host_final_tag_wrap(seven, monkeypatch):
    raws, segs = seven
    _env(monkeypatch, 1, PHIP_HOST_FINAL_TAG0="65530")
    qc, oblk, ex = _oracle("seven", CASES[3][1], raws)
    op, core, first = _plan(monkeypatch, qc, segs, host_final=True)
    try:
        assert first[0] == oblk.stats.num_docs_scanned
        for i in range(11):  # tags 65531 .. 65535, 1 .. 7
            assert _snapshot(core, len(segs)) == first, i
            assert core.launch_shape()["host_final"] == 1
        _check_oracle(qc, op, oblk, ex)
    finally:
        op.close()


def test_gpu_host_final_uneven_finish(uneven, monkeypatch):
    """One 300 000-doc segment beside six 300-doc ones: the small segments' blocks finish long before the others."""
    raws, segs = uneven
    _env(monkeypatch)
    qc, oblk, ex = _oracle("uneven", CASES[3][1], raws)
    op_a, core_a, first_a = _plan(monkeypatch, qc, segs, host_final=False)
    op_b, core_b, first_b = _plan(monkeypatch, qc, segs, host_final=True)
    try:
        assert first_a == first_b and first_a[0] == oblk.stats.num_docs_scanned
        for i in range(199):
            assert _snapshot(core_b, len(segs)) == first_a, i
        assert core_b.launch_shape()["host_final"] == 1 and core_a.launch_shape()["host_final"] == 0
        _check_oracle(qc, op_b, oblk, ex)
    finally:
        op_a.close()
        op_b.close()


def test_gpu_host_final_concurrent(seven, monkeypatch):
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    raws, segs = seven
    _env(monkeypatch)
    sqls = [c[1] for c in CASES if c[2]]
    qcs = [parse(s) for s in sqls]
    want = []
    for qc in qcs:  # the single-threaded answers
        op, core, first = _plan(monkeypatch, qc, segs, host_final=True)
        want.append(first)
        op.close()
    errors = []

    def worker(i):
        try:
            op = GpuInstancePlanMaker().make_instance_plan(qcs[i % len(qcs)], segs)
            core = _core(op)
            for n in range(50):
                got = _snapshot(core, len(segs))
                assert got == want[i % len(qcs)], (n, got, want[i % len(qcs)])
            assert core.launch_shape()["host_final"] == 1
            op.close()
        except Exception as e:  # surfaced below
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=100)
    assert not any(t.is_alive() for t in threads), "a worker hung"
    assert not errors, errors[:3]
