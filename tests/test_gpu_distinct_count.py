"""GPU tests of exact DISTINCTCOUNT (pinot_amd/csrc/distinct.hip): the reference's known answers, and synthetic segments
against a numpy reference that does not touch the code under test -- oracle.executor.filter_mask for the matched docs,
OracleSegment.values for the column, then the distinct values per group, FLOAT / DOUBLE compared by bit pattern.
Every comparison is exact (sets of values and counts): integer OR has no rounding.
"""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

from oracle import executor
from pinot_amd import _lib
from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker, UnsupportedOnGpu
from pinot_amd.engine.reduce import broker_response, reduce_blocks
from pinot_amd.engine.segment import GpuSegment
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType
from tests import fixtures

pytestmark = pytest.mark.gpu

with open(os.path.join(fixtures.GOLDEN, "distinct_count.json")) as _f:
    KATS = json.load(_f)["queries"]

# both regimes of distinct_mark_kernel on any dictionary: "0" = every bitmap global, the default budget = LDS (all
# dictionaries here are below 8192 words)
REGIMES = {"lds": None, "global": "0"}
ALL = "f < 50 OR f >= 50"       # every doc, but through the scan (a lone always-true leaf would fold to match-all)
ONE_PERCENT = "f = 7"           # f is uniform over 0..99
NONE = "f < 30 AND f > 60"
FILTERS = (ALL, ONE_PERCENT, NONE)


def _regime(monkeypatch, regime):
    if REGIMES[regime] is None:
        monkeypatch.delenv("PHIP_DISTINCT_LDS_WORDS", raising=False)
    else:
        monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", REGIMES[regime])


def _canon(v):
    """A set member by its bits: floats (FLOAT columns read as their double image) by the double's bit pattern,
    every NaN as one."""
    if isinstance(v, (float, np.floating)):
        v = float(v)
        return ("f", struct.pack("<d", float("nan") if v != v else v))
    if isinstance(v, (int, np.integer)):
        return ("i", int(v))
    return ("s", str(v))


def _canon_set(s):
    out = {_canon(v) for v in s}
    assert len(out) == len(s), "members that differ only in how Python compares them"
    return out


def _reference(qc, raws, col, keys=()):
    """{group key tuple: set of canonical members of `col`} over the docs the filter keeps in every segment."""
    out = {}
    for raw in raws:
        mask = np.asarray(executor.filter_mask(qc, raw), dtype=bool)
        os_ = executor.OracleSegment(raw)
        vals = np.asarray(os_.values(col))[mask]
        kcols = [np.asarray(os_.values(k))[mask] for k in keys]
        if not keys:
            out.setdefault((), set()).update(_canon(v) for v in vals.tolist())
            continue
        for i, v in enumerate(vals.tolist()):
            out.setdefault(tuple(k[i].item() if hasattr(k[i], "item") else k[i] for k in kcols), set()).add(_canon(v))
    if not keys:
        out.setdefault((), set())
    return out


def _block(query, gsegs):
    qc = parse(query)
    op = GpuInstancePlanMaker().make_instance_plan(qc, gsegs)
    return qc, op, op.next_block()


def _check_plain(query, gsegs, cols):
    qc, op, blk = _block(query, gsegs)
    raws = [g.segment for g in gsegs]
    matched = sum(int(np.count_nonzero(executor.filter_mask(qc, r))) for r in raws)
    assert blk.stats.num_docs_scanned == matched
    # (a one-doc segment folds every predicate to a constant: match-all is then the dictionary shortcut's, 0 entries)
    scanned = not op._non_scan_fit()
    assert scanned or min(g.num_docs for g in gsegs) == 1
    assert blk.stats.num_entries_scanned_post_filter == (matched * len(set(cols)) if scanned else 0)
    finals = reduce_blocks(qc, [blk]).rows[0]
    for i, col in enumerate(cols):
        ref = _reference(qc, raws, col)[()]
        assert _canon_set(blk.results[i]) == ref, (query, col)
        assert finals[i] == len(ref) and type(finals[i]) is int
    return blk


# ---------------------------------------------------------------------------------------------- 1. known answers
@pytest.fixture(scope="module")
def sv(gpu_lib):
    s = GpuSegment(fixtures.test_data_sv_segment())
    yield s
    s.destroy()


@pytest.mark.parametrize("case", KATS, ids=[f"{c['ref'].split('/')[-1]}|{c['query'][-40:]}" for c in KATS])
def test_gpu_distinct_known_answers(case, sv):
    rt = broker_response(GpuInstancePlanMaker(), case["query"], [sv, sv])
    docs, post, total = case["stats"]
    assert (rt.stats.num_docs_scanned, rt.stats.num_entries_scanned_post_filter, rt.stats.num_total_docs) == \
        (docs, post, total)
    assert rt.rows == case["rows"]


# ---------------------------------------------------------------------------------------------- 2. synthetic
DOCS = (1, 63, 64, 65, 2047, 2049, 4097)   # lane and tile tails (64-doc groups, 2048-doc tiles)
CARDS = (1, 31, 32, 33, 1025)              # word tails, id widths 1..11 bits


def _small(n, seed):
    rng = np.random.default_rng(seed)
    c = SegmentCreator(f"dc{n}")
    c.add_column("f", DataType.INT, rng.integers(0, 100, n))
    for card in CARDS:
        c.add_column(f"a{card}", DataType.INT, rng.permutation(np.arange(n) % card) * 3 + 1)
    return c.build()


@pytest.fixture(scope="module")
def small(gpu_lib):
    segs = {n: GpuSegment(_small(n, 100 + n)) for n in DOCS}
    yield segs
    for s in segs.values():
        s.destroy()


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("n", DOCS)
def test_gpu_distinct_sizes_and_cardinalities(n, regime, small, monkeypatch):
    _regime(monkeypatch, regime)
    for flt in FILTERS:
        for card in CARDS:
            _check_plain(f"SELECT DISTINCTCOUNT(a{card}) FROM t WHERE {flt}", [small[n]], [f"a{card}"])
    blk = _check_plain(f"SELECT DISTINCTCOUNT(a33) FROM t WHERE {NONE}", [small[n]], ["a33"])
    assert blk.results[0] == set()


@pytest.fixture(scope="module")
def typed(gpu_lib):
    rng = np.random.default_rng(11)
    n = 3000
    c = SegmentCreator("dctyped")
    c.add_column("f", DataType.INT, rng.integers(0, 100, n))
    c.add_column("i", DataType.INT, rng.integers(-500, 500, n))
    c.add_column("l", DataType.LONG, rng.integers(0, 700, n) * (1 << 33))
    c.add_column("fl", DataType.FLOAT, (rng.integers(0, 200, n) / 8.0).astype(np.float32))
    c.add_column("s", DataType.STRING, np.array([f"k{x:03d}é" for x in rng.integers(0, 150, n)]))
    c.add_column("srt", DataType.INT, np.sort(rng.integers(0, 90, n)))  # a sorted forward index
    s = GpuSegment(c.build())
    assert s.column_metadata("srt").is_sorted
    yield s
    s.destroy()


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_distinct_types_and_sorted_column(regime, typed, monkeypatch):
    _regime(monkeypatch, regime)
    for flt in FILTERS:
        _check_plain(f"SELECT DISTINCTCOUNT(i), DISTINCTCOUNT(l), DISTINCTCOUNT(fl), DISTINCTCOUNT(s), "
                     f"DISTINCTCOUNT(srt) FROM t WHERE {flt}", [typed], ["i", "l", "fl", "s", "srt"])


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_distinct_double_zeros_and_nan(regime, gpu_lib, monkeypatch):
    """-0.0 and 0.0 are two members and NaN is one (DoubleOpenHashSet compares bits): one segment holds -0.0, the
    other 0.0, both hold NaN, so the query-global dictionary must keep the zeros apart."""
    _regime(monkeypatch, regime)
    rng = np.random.default_rng(5)
    segs = []
    for j, zero in enumerate((-0.0, 0.0)):
        n = 700 + j
        d = rng.integers(1, 40, n) / 4.0
        d[::7] = zero
        d[3::11] = float("nan")
        c = SegmentCreator(f"dcd{j}")
        c.add_column("f", DataType.INT, rng.integers(0, 100, n))
        c.add_column("d", DataType.DOUBLE, d)
        segs.append(GpuSegment(c.build()))
    try:
        blk = _check_plain(f"SELECT DISTINCTCOUNT(d) FROM t WHERE {ALL}", segs, ["d"])
        plain = [float(v) for v in blk.results[0]]  # (a JavaDoubleKey equals only its own kind: compare plain floats)
        zeros = sorted(float(np.copysign(1.0, v)) for v in plain if v == 0.0)
        assert zeros == [-1.0, 1.0] and sum(1 for v in plain if v != v) == 1
    finally:
        for s in segs:
            s.destroy()


@pytest.fixture(scope="module")
def wide(gpu_lib):
    rng = np.random.default_rng(17)
    n = 100_000
    c = SegmentCreator("dcwide")
    c.add_column("f", DataType.INT, rng.integers(0, 100, n))
    c.add_column("w", DataType.INT, rng.integers(0, 110_000, n))  # ~65-70K distinct of 100K docs: 17-bit ids
    s = GpuSegment(c.build())
    assert s.column_metadata("w").bits_per_element == 17
    yield s
    s.destroy()


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_distinct_17_bit_ids(regime, wide, monkeypatch):
    _regime(monkeypatch, regime)
    for flt in (ALL, ONE_PERCENT):
        _check_plain(f"SELECT DISTINCTCOUNT(w) FROM t WHERE {flt}", [wide], ["w"])


# ---------------------------------------------------------------------------------------------- 3. several segments
@pytest.fixture(scope="module")
def three(gpu_lib):
    rng = np.random.default_rng(23)
    segs = []
    for j, n in enumerate((1000, 2049, 4097)):
        c = SegmentCreator(f"dcm{j}")
        c.add_column("f", DataType.INT, rng.integers(0, 100, n))
        c.add_column("a", DataType.INT, rng.integers(150 * j, 150 * j + 300, n))
        c.add_column("b", DataType.STRING, np.array([f"s{x}" for x in rng.integers(20 * j, 20 * j + 40, n)]))
        c.add_column("k1", DataType.INT, rng.integers(3 * j, 3 * j + 5, n))
        c.add_column("k2", DataType.STRING, np.array([f"g{x}" for x in rng.integers(j, j + 3, n)]))
        c.add_column("x", DataType.LONG, rng.integers(-1000, 1000, n))
        segs.append(GpuSegment(c.build()))
    yield segs
    for s in segs:
        s.destroy()


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_distinct_union_over_segments(regime, three, monkeypatch):
    _regime(monkeypatch, regime)
    for flt in FILTERS:
        blk = _check_plain(f"SELECT DISTINCTCOUNT(a), DISTINCTCOUNT(b) FROM t WHERE {flt}", three, ["a", "b"])
    qc = parse(f"SELECT DISTINCTCOUNT(a) FROM t WHERE {ALL}")
    per_seg = sum(len(_reference(qc, [g.segment], "a")[()]) for g in three)
    blk = _check_plain(f"SELECT DISTINCTCOUNT(a) FROM t WHERE {ALL}", three, ["a"])
    assert len(blk.results[0]) == len(_reference(qc, [g.segment for g in three], "a")[()]) < per_seg  # union, not sum


# ---------------------------------------------------------------------------------------------- 4. group-by
def _check_groups(query, gsegs, keys, cols, others=(), limit_keys=None):
    """cols: {aggregation index: column} of the DISTINCTCOUNTs; others: {aggregation index: (function, column)}."""
    qc, _, blk = _block(query, gsegs)
    raws = [g.segment for g in gsegs]
    refs = {i: _reference(qc, raws, col, keys) for i, col in cols.items()}
    want = set(next(iter(refs.values()))) if limit_keys is None else set(limit_keys)
    assert set(blk.groups) == want
    for k in want:
        for i, col in cols.items():
            assert _canon_set(blk.groups[k][i]) == refs[i][k], (query, k, col)
    for i, (fn, col) in dict(others).items():
        for k in want:
            sel = None
            tot = 0
            for raw in raws:
                os_ = executor.OracleSegment(raw)
                sel = np.asarray(executor.filter_mask(qc, raw), dtype=bool)
                for kc, kv in zip(keys, k):
                    sel = sel & (np.asarray(os_.values(kc)) == kv)
                tot += int(np.count_nonzero(sel)) if fn == "count" else int(np.asarray(os_.values(col))[sel].sum())
            assert blk.groups[k][i] == tot, (query, k, fn)
    finals = {tuple(r[:len(keys)]): r[len(keys):] for r in reduce_blocks(qc, [blk]).rows}
    for k in list(want)[:10]:
        if k in finals:
            for i, col in cols.items():
                assert finals[k][i] == len(refs[i][k])
    return blk


@pytest.mark.parametrize("flt", FILTERS)
def test_gpu_distinct_group_by(flt, three):
    # one key column, every function of the issue's list in one query (the repeated column shares its slot)
    q = ("SELECT k1, COUNT(*), SUM(x), DISTINCTCOUNT(a), DISTINCTCOUNT(b), DISTINCTCOUNT(a) FROM t "
         f"WHERE {flt} GROUP BY k1 LIMIT 1000")
    qc, op, _ = _block(q, three)
    dist = [p for p in op.prims if p[0] == _lib.AGG_DISTINCT]
    assert len(dist) == 2
    blk = _check_groups(q, three, ["k1"], {2: "a", 3: "b"}, {0: ("count", None), 1: ("sum", "x")})
    matched = blk.stats.num_docs_scanned
    assert blk.stats.num_entries_scanned_post_filter == matched * 4  # k1, x, a, b
    # two key columns (INT x STRING), and a query with only DISTINCTCOUNT aggregations
    _check_groups(f"SELECT k1, k2, DISTINCTCOUNT(b), COUNT(*) FROM t WHERE {flt} GROUP BY k1, k2 LIMIT 1000", three,
                  ["k1", "k2"], {0: "b"}, {1: ("count", None)})
    _check_groups(f"SELECT k2, DISTINCTCOUNT(a), DISTINCTCOUNT(k1) FROM t WHERE {flt} GROUP BY k2 LIMIT 1000", three,
                  ["k2"], {0: "a", 1: "k1"})


def test_gpu_distinct_group_by_num_groups_limit(three):
    """numGroupsLimit below the number of groups: one segment keeps the first `limit` keys it meets in doc order, and
    every doc of a kept key still aggregates, so the kept groups' sets are exact."""
    seg = three[2]
    q = f"SET numGroupsLimit = 3; SELECT k1, DISTINCTCOUNT(a), COUNT(*) FROM t WHERE {ALL} GROUP BY k1 LIMIT 1000"
    k1 = np.asarray(executor.OracleSegment(seg.segment).values("k1"))
    _, first = np.unique(k1, return_index=True)
    kept = [(int(k1[i]),) for i in sorted(first.tolist())[:3]]
    assert len(np.unique(k1)) == 5
    blk = _check_groups(q, [seg], ["k1"], {0: "a"}, {1: ("count", None)}, limit_keys=kept)
    assert blk.num_groups_limit_reached


def test_gpu_distinct_num_groups_limit_over_several_segments_is_refused(three):
    """The limit is per segment: a segment that dropped a key skips that key's docs, so a kept group's set would have
    to leave those docs out, while a bitmap row holds the key's values over every segment. Over several segments the
    execution is refused (the CPU plan maker answers) instead of returning the union; below the limit the same query
    is answered, and it matches the numpy reference."""
    lib = _lib.load()
    q = f"SELECT k1, DISTINCTCOUNT(a), COUNT(*) FROM t WHERE {ALL} GROUP BY k1 LIMIT 1000"
    qc = parse("SET numGroupsLimit = 3; " + q)
    assert len(_reference(qc, [g.segment for g in three], "a", ["k1"])) == 11  # 11 groups, 5 in every segment
    op = GpuInstancePlanMaker().make_instance_plan(qc, three)
    with pytest.raises(UnsupportedOnGpu) as ei:
        op.next_block()
    assert "numGroupsLimit" in str(ei.value)
    assert getattr(ei.value, "code", _lib.PHIP_ERR_UNSUPPORTED) == _lib.PHIP_ERR_UNSUPPORTED
    with pytest.raises(UnsupportedOnGpu):  # ... on every execution of the plan, and exactly at the limit too
        op.next_block()
    with pytest.raises(UnsupportedOnGpu):
        GpuInstancePlanMaker().make_instance_plan(parse("SET numGroupsLimit = 11; " + q), three).next_block()
    # the library answers the next queries: the same one below the limit (12 > 11 groups), and a plain one
    blk = _check_groups("SET numGroupsLimit = 12; " + q, three, ["k1"], {0: "a"}, {1: ("count", None)})
    assert not blk.num_groups_limit_reached
    _check_plain(f"SELECT DISTINCTCOUNT(a) FROM t WHERE {ONE_PERCENT}", three, ["a"])
    assert lib.phip_last_error() is not None


# ---------------------------------------------------------------------------------------------- 5. / 6. re-execution, ABI
def _abi_rows(lib, res):
    r = res.contents
    nd, ng, na = int(r.num_distinct), int(r.num_groups), int(r.num_aggregations)
    offs = [int(r.distinct_word_offsets[i]) for i in range(nd + 1)]
    words = np.ctypeslib.as_array(r.distinct_words, shape=(max(ng * offs[nd], 1),))[:ng * offs[nd]].copy()
    longs = [int(r.long_values[i]) for i in range(ng * na)]
    vals = [float(r.values[i]) for i in range(ng * na)]
    exact = [int(r.long_exact[i]) for i in range(na)]
    return nd, ng, na, offs, words.reshape(ng, offs[nd]), longs, vals, exact


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_distinct_reexecution_and_abi(regime, three, monkeypatch):
    _regime(monkeypatch, regime)
    lib = _lib.load()
    for q, keys in ((f"SELECT DISTINCTCOUNT(a), COUNT(*), DISTINCTCOUNT(b) FROM t WHERE {ALL}", []),
                    (f"SELECT DISTINCTCOUNT(a), COUNT(*), DISTINCTCOUNT(b) FROM t WHERE {ONE_PERCENT}", []),
                    (f"SELECT k1, DISTINCTCOUNT(a), COUNT(*), DISTINCTCOUNT(b) FROM t WHERE {ALL} GROUP BY k1", ["k1"]),
                    (f"SELECT DISTINCTCOUNT(a), COUNT(*), DISTINCTCOUNT(b) FROM t WHERE {NONE}", [])):
        qc = parse(q)
        op = GpuCombineOperator(qc, three, 100000)
        runs = []
        for _ in range(3):  # (the replay path starts from the second execution)
            res = op.run_raw()
            try:
                nd, ng, na, offs, words, longs, vals, exact = _abi_rows(lib, res)
                dicts = []
                for s in range(nd):
                    dv = _lib.DictionaryView()
                    _lib.check(lib.phip_result_distinct_dictionary(res, s, ctypes.byref(dv)))
                    dicts.append((int(dv.data_type), int(dv.cardinality)))
                assert lib.phip_result_distinct_dictionary(res, nd, ctypes.byref(_lib.DictionaryView())) == \
                    _lib.PHIP_ERR_INVALID
            finally:
                lib.phip_result_free(res)
            runs.append((words.tobytes(), longs, vals))
            slots = [i for i, p in enumerate(op.prims) if p[0] == _lib.AGG_DISTINCT]
            assert nd == 2 and len(slots) == 2
            raws = [g.segment for g in three]
            for s, (i, col) in enumerate(zip(slots, ("a", "b"))):
                union = sorted({v for raw in raws for v in executor.OracleSegment(raw).dictionary(col).tolist()})
                assert dicts[s][1] == len(union)  # the sorted union of the segments' dictionaries
                assert offs[s + 1] - offs[s] == (len(union) + 31) // 32
                w = words[:, offs[s]:offs[s + 1]]
                bits = np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=1, bitorder="little")
                assert not bits[:, len(union):].any()  # bits beyond the cardinality are zero
                for g in range(ng):
                    assert int(bits[g].sum()) == longs[g * na + i] == vals[g * na + i] and exact[i] == 1
                if not keys:  # the ids are the union dictionary's: bit i = union[i]
                    ref = _reference(qc, raws, col)[()]
                    assert {_canon(union[j]) for j in np.nonzero(bits[0])[0].tolist()} == ref
            if NONE in q:
                assert ng == 1 and not words.any() and longs[slots[0]] == 0 and longs[slots[1]] == 0
        assert runs[0] == runs[1] == runs[2]
        blocks = [op.next_block() for _ in range(3)]
        if keys:
            assert blocks[0].groups == blocks[1].groups == blocks[2].groups
        else:
            assert blocks[0].results == blocks[1].results == blocks[2].results
        op.close()


# ---------------------------------------------------------------------------------------------- 7. library refusals
def _create(lib, op, patch=None):
    keep = []
    q = op._desc(keep)
    if patch:
        patch(q)
    h = ctypes.c_uint64(0)
    rc = lib.phip_plan_create(ctypes.byref(q), ctypes.byref(h))
    msg = lib.phip_last_error().decode(errors="replace") if rc else ""
    if rc == 0:
        lib.phip_plan_destroy(h.value)
    return rc, msg


def test_gpu_distinct_library_refusals(three, monkeypatch):
    lib = _lib.load()
    rng = np.random.default_rng(31)
    c = SegmentCreator("dcraw", no_dictionary_columns=["r"])
    c.add_column("f", DataType.INT, rng.integers(0, 100, 500))
    c.add_column("r", DataType.LONG, rng.integers(0, 50, 500))
    rawseg = GpuSegment(c.build())

    def usable():  # the library answers the next query
        _check_plain(f"SELECT DISTINCTCOUNT(a) FROM t WHERE {ONE_PERCENT}", three, ["a"])

    try:
        # a raw (no-dictionary) argument column (the Python plan refuses it first, so the descriptor is made by hand)
        op = GpuCombineOperator(parse(f"SELECT SUM(r) FROM t WHERE {ONE_PERCENT}"), [rawseg], 100000)
        op.prims = [(_lib.AGG_DISTINCT, _lib.EXPR_COLUMN, "r", None, 0, 0)]
        rc, msg = _create(lib, op)
        assert rc == _lib.PHIP_ERR_UNSUPPORTED and "raw" in msg
        usable()
        gq = parse(f"SELECT k1, DISTINCTCOUNT(a) FROM t WHERE {ALL} GROUP BY k1")
        # the bitmap budget: 11 x 5 dense keys x (>= 19 + 3 words) x 4 bytes is above 4096
        big = parse(f"SELECT k1, k2, DISTINCTCOUNT(a), DISTINCTCOUNT(b) FROM t WHERE {ALL} GROUP BY k1, k2")
        monkeypatch.setenv("PHIP_DISTINCT_MAX_BYTES", "4096")
        rc, msg = _create(lib, GpuCombineOperator(big, three, 100000))
        assert rc == _lib.PHIP_ERR_UNSUPPORTED and "PHIP_DISTINCT_MAX_BYTES" in msg
        with pytest.raises(UnsupportedOnGpu):
            GpuCombineOperator(big, three, 100000).next_block()
        monkeypatch.delenv("PHIP_DISTINCT_MAX_BYTES")
        usable()
        # ORDER BY on the distinct term: refused while the dense key space (11 keys) exceeds trim_size, taken otherwise
        def order(trim):
            def patch(q):
                q.order_by_aggregation, q.order_by_desc, q.trim_size = 0, 1, trim
            return patch
        rc, msg = _create(lib, GpuCombineOperator(gq, three, 100000), order(10))
        assert rc == _lib.PHIP_ERR_UNSUPPORTED and "ORDER BY" in msg
        terms = (_lib.OrderTerm * 1)(_lib.OrderTerm(_lib.ORDER_VALUE, 0, 0, 1))

        def by_terms(q):
            q.num_order_terms, q.order_terms, q.trim_size = 1, terms, 10
        rc, msg = _create(lib, GpuCombineOperator(gq, three, 100000), by_terms)
        assert rc == _lib.PHIP_ERR_UNSUPPORTED and "ORDER BY" in msg
        rc, msg = _create(lib, GpuCombineOperator(gq, three, 100000), order(11))
        assert rc == _lib.PHIP_OK, msg
        usable()
        # a hash-table key space (forced here; a large dense key space is re-sized into one late in plan creation)
        monkeypatch.setenv("PHIP_GB_HASH", "1")
        rc, msg = _create(lib, GpuCombineOperator(gq, three, 100000))
        assert rc == _lib.PHIP_ERR_UNSUPPORTED and "hash-table" in msg
        monkeypatch.delenv("PHIP_GB_HASH")
        usable()
        # node plans
        monkeypatch.setenv("PHIP_NODE_SPLIT", "2")
        rc, msg = _create(lib, GpuCombineOperator(gq, three, 100000))
        assert rc == _lib.PHIP_ERR_UNSUPPORTED and "node plan" in msg
        monkeypatch.delenv("PHIP_NODE_SPLIT")
        usable()
        # no partial table either
        op = GpuCombineOperator(gq, three, 100000)
        assert op.execute_partial() is None
        _check_groups(f"SELECT k1, DISTINCTCOUNT(a) FROM t WHERE {ALL} GROUP BY k1", three, ["k1"], {0: "a"})
    finally:
        rawseg.destroy()
