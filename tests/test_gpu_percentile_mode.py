"""GPU tests of exact PERCENTILE and MODE (the value counts of pinot_amd/csrc/distinct.hip): the reference's known
answers, and synthetic segments against a numpy restatement that does not touch the code under test --
oracle.executor.filter_mask for the matched docs and OracleSegment.values for the column, then the matched values sorted
and indexed (PERCENTILE) or counted (MODE). Every comparison is exact, FLOAT / DOUBLE by bit pattern: integer adds have
no rounding.
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

with open(os.path.join(fixtures.GOLDEN, "percentile.json")) as _f:
    KATS = json.load(_f)["queries"]

# both regimes of distinct_mark_kernel: "0" = every row global, the default budget = LDS (8192 words) without a group-by
REGIMES = {"lds": None, "global": "0"}
ALL = "f < 50 OR f >= 50"       # every doc, but through the scan (a lone always-true leaf would fold to match-all)
ONE_PERCENT = "f = 7"           # f is uniform over 0..99
NONE = "f < 30 AND f > 60"
FILTERS = {"all": f" WHERE {ALL}", "one_percent": f" WHERE {ONE_PERCENT}", "no_where": ""}
PCTS = (0, 1, 25, 50, 75, 90, 99, 99.9, 100)


def _regime(monkeypatch, regime):
    if REGIMES[regime] is None:
        monkeypatch.delenv("PHIP_DISTINCT_LDS_WORDS", raising=False)
    else:
        monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", REGIMES[regime])


# ---------------------------------------------------------------------------------------------- the numpy restatement
def _bits(v):
    return struct.pack("<d", float(v))


def _canon(v):
    """A value by its bits: reals (a FLOAT as its double image) by the double's bit pattern, integers as they are."""
    if isinstance(v, (float, np.floating)):
        return ("f", _bits(v))
    return ("i", int(v))


def _canon_map(m):
    out = {_canon(k): int(n) for k, n in m.items()}
    assert len(out) == len(m), "keys that differ only in how Python compares them"
    return out


def _java_order(v):
    """Double.compare as an integer key (no NaN here): the sign-magnitude bits made monotonic, so -0.0 < 0.0."""
    i = struct.unpack("<q", _bits(v))[0]
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF) - 1


def _matched_values(qc, raws, col, keys=()):
    """{group key tuple: list of `col`'s matched values (stored type) over every segment}."""
    out = {}
    for raw in raws:
        mask = np.asarray(executor.filter_mask(qc, raw), dtype=bool)
        os_ = executor.OracleSegment(raw)
        vals = np.asarray(os_.values(col))[mask].tolist()
        kcols = [np.asarray(os_.values(k))[mask].tolist() for k in keys]
        for i, v in enumerate(vals):
            out.setdefault(tuple(k[i] for k in kcols), []).append(v)
    if not keys:
        out.setdefault((), [])
    return out


def _ref_percentile(vals, p):
    """PercentileAggregationFunction.extractFinalResult: the sorted list indexed."""
    if not vals:
        return float("-inf")
    s = sorted((float(v) for v in vals), key=_java_order)
    return s[len(s) - 1] if p == 100 else s[int(float(len(s)) * p / 100)]


def _ref_counts(vals, as_double):
    out = {}
    for v in vals:
        k = _canon(float(v) if as_double else v)
        out[k] = out.get(k, 0) + 1
    return out


def _ref_mode(vals, reducer):
    """ModeAggregationFunction.extractFinalResult over the values counted by their bits; None where the values of
    maximal count hold both zeros (the reference's answer then follows its hash map's iteration order)."""
    if not vals:
        return float("-inf")
    counts, value = {}, {}
    for v in vals:
        k = _canon(v)
        counts[k] = counts.get(k, 0) + 1
        value[k] = v
    top = max(counts.values())
    modes = sorted(value[k] for k, n in counts.items() if n == top)
    if sum(1 for v in modes if v == 0) > 1:
        return None
    if reducer == "AVG":
        assert all(isinstance(v, int) and abs(v) < 1 << 53 for v in modes) and abs(sum(modes)) < 1 << 53 or len(modes) == 1
        return sum(modes) / len(modes)
    return float(modes[0] if reducer == "MIN" else modes[-1])


def _matched(qc, raws):
    return sum(int(np.count_nonzero(executor.filter_mask(qc, r))) for r in raws)


def _block(query, gsegs):
    qc = parse(query)
    op = GpuInstancePlanMaker().make_instance_plan(qc, gsegs)
    blk = op.next_block()
    return qc, op, blk


def _check_aggregations(qc, intermediates, finals, values_of, where):
    """Every PERCENTILE / MODE of the query: its intermediate's counts and its final result against the restatement.
    values_of(col) = the matched values. Returns the docs every slot aggregated (they all agree)."""
    totals = set()
    for i, ag in enumerate(qc.aggregations):
        if ag.function not in ("percentile", "mode"):
            continue
        vals = values_of(ag.argument.name)
        got = intermediates[i]
        assert _canon_map(got) == _ref_counts(vals, ag.function == "percentile"), (where, i)
        totals.add(sum(got.values()))
        if ag.function == "percentile":
            assert all(type(k) is float or isinstance(k, float) for k in got)
            assert _bits(finals[i]) == _bits(_ref_percentile(vals, ag.percentile)), (where, i, ag.percentile)
        else:
            want = _ref_mode(vals, ag.reducer)
            assert want is None or _bits(finals[i]) == _bits(want), (where, i, ag.reducer)
        assert type(finals[i]) is float
    return totals


def _check_plain(query, gsegs):
    qc, op, blk = _block(query, gsegs)
    raws = [g.segment for g in gsegs]
    matched = _matched(qc, raws)
    cols = {ag.argument.name for ag in qc.aggregations if ag.argument is not None}
    assert blk.stats.num_docs_scanned == matched
    assert not op._non_scan_fit()  # (the reference scans these functions: never the dictionary shortcut)
    assert blk.stats.num_entries_scanned_post_filter == matched * len(cols)
    finals = reduce_blocks(qc, [blk]).rows[0]
    by_col = {c: _matched_values(qc, raws, c)[()] for c in cols}
    totals = _check_aggregations(qc, blk.results, finals, by_col.__getitem__, query)
    assert totals == {matched}  # every slot's doc total is the matched docs
    for i, ag in enumerate(qc.aggregations):
        if ag.function == "distinctcount":
            assert finals[i] == len({_canon(v) for v in by_col[ag.argument.name]})
        if ag.function == "count":
            assert finals[i] == matched
    return op, blk


def _check_groups(query, gsegs, keys):
    qc, op, blk = _block(query, gsegs)
    raws = [g.segment for g in gsegs]
    matched = _matched(qc, raws)
    cols = {ag.argument.name for ag in qc.aggregations if ag.argument is not None}
    assert blk.stats.num_docs_scanned == matched
    assert blk.stats.num_entries_scanned_post_filter == matched * len(cols | set(keys))
    by_col = {c: _matched_values(qc, raws, c, keys) for c in cols}
    want = set(next(iter(by_col.values())))
    assert set(blk.groups) == want
    rows = {tuple(r[:len(keys)]): r[len(keys):] for r in reduce_blocks(qc, [blk]).rows}
    assert set(rows) == want  # (LIMIT above the groups)
    # the select list is the keys, then the aggregations in order
    total = 0
    for k in want:
        totals = _check_aggregations(qc, blk.groups[k], rows[k], lambda c: by_col[c][k], (query, k))
        assert len(totals) == 1
        total += totals.pop()
    assert total == matched
    return blk


# ---------------------------------------------------------------------------------------------- 1. known answers
@pytest.fixture(scope="module")
def sv(gpu_lib):
    s = GpuSegment(fixtures.test_data_sv_segment())
    yield s
    s.destroy()


@pytest.mark.parametrize("case", KATS, ids=[f"{c['ref'].split('/')[-1]}|{c['query'][7:34]}|{len(c['query'])}" for c in KATS])
def test_gpu_percentile_known_answers(case, sv):
    rt = broker_response(GpuInstancePlanMaker(), case["query"], [sv, sv])
    docs, post, total = case["stats"]
    assert (rt.stats.num_docs_scanned, rt.stats.num_entries_scanned_post_filter, rt.stats.num_total_docs) == \
        (docs, post, total)
    assert rt.rows == case["rows"]
    assert all(type(v) is float for v in rt.rows[0][-1:])


# ---------------------------------------------------------------------------------------------- 2. synthetic
def _segment(j, n, rng):
    """Segment j of `n` docs; every dictionary differs from the other segments', so the remap to query-global ids
    matters. c2 has two values in all (every lane of a wave on one of two words), u is distinct in every doc."""
    c = SegmentCreator(f"pm{j}_{n}", no_dictionary_columns=["r"])
    c.add_column("f", DataType.INT, rng.integers(0, 100, n))
    c.add_column("i", DataType.INT, rng.integers(100 * j - 150, 100 * j + 150, n))
    c.add_column("l", DataType.LONG, rng.integers(50 * j, 50 * j + 400, n) * (1 << 33))
    fl = (rng.integers(-20 - j, 60 + j, n) / 8.0).astype(np.float32)
    fl[::5] = 0.0
    fl[1::5] = -0.0
    c.add_column("fl", DataType.FLOAT, fl)
    d = rng.integers(-30 + j, 30 + j, n) / 4.0
    d[::3] = -0.0 if j != 1 else 0.0  # the zeros of one segment's dictionary are not the other's
    d[1::7] = 0.0
    c.add_column("d", DataType.DOUBLE, d)
    c.add_column("c2", DataType.INT, np.where((np.arange(n) + (j == 0)) % 2 == 0, 5, 9))
    c.add_column("u", DataType.INT, 10_000 * j + rng.permutation(n))
    c.add_column("m", DataType.LONG, rng.integers(j, j + 4, n) * ((1 << 44) + 1))  # integers below 2^53: AVG is exact
    c.add_column("k1", DataType.INT, rng.integers(3 * j, 3 * j + 5, n))
    c.add_column("k2", DataType.STRING, np.array([f"g{x}" for x in rng.integers(j, j + 3, n)]))
    c.add_column("r", DataType.LONG, rng.integers(0, 50, n))
    return c.build()


@pytest.fixture(scope="module")
def three(gpu_lib):
    rng = np.random.default_rng(29)
    segs = [GpuSegment(_segment(j, n, rng)) for j, n in enumerate((1, 2049, 5000))]  # (2049: one doc into a second tile)
    yield segs
    for s in segs:
        s.destroy()


def _pct_list(col):
    return ", ".join(f"PERCENTILE({col}, {p})" for p in PCTS)


@pytest.mark.parametrize("flt", list(FILTERS))
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_percentile_mode_types(regime, flt, three, monkeypatch):
    """INT, LONG, FLOAT and DOUBLE columns with both zeros, nine percentiles and the three reducers of each: one counts
    slot per column whatever the number of functions."""
    _regime(monkeypatch, regime)
    w = FILTERS[flt]
    for col in ("i", "l", "fl", "d"):
        q = f"SELECT {_pct_list(col)}, MODE({col}), MODE({col}, 'MAX'), MODE({col}, 'AVG'), PERCENTILE95({col}) FROM t{w}"
        op, _ = _check_plain(q, three)
        assert [p[0] for p in op.prims] == [_lib.AGG_VALUE_COUNTS]
    op, blk = _check_plain(f"SELECT PERCENTILE50(i), MODE(l), PERCENTILE99(fl), PERCENTILE(d, 10), MODE(m, 'AVG'), COUNT(*) "
                           f"FROM t{w}", three)
    assert sum(p[0] == _lib.AGG_VALUE_COUNTS for p in op.prims) == 5
    # the zeros stay apart in a PERCENTILE's keys: -0.0 sorts below 0.0
    if flt != "one_percent":
        keys = [k for k in blk.results[3] if float(k) == 0.0]
        assert sorted(np.copysign(1.0, float(k)) for k in keys) == [-1.0, 1.0]


@pytest.mark.parametrize("flt", list(FILTERS))
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_percentile_mode_card_2_and_all_distinct(regime, flt, three, monkeypatch):
    """c2: every lane of a wave adds to one of two words; u: every doc its own word (7051 words: within the LDS budget)."""
    _regime(monkeypatch, regime)
    w = FILTERS[flt]
    op, blk = _check_plain(f"SELECT PERCENTILE50(c2), MODE(c2), MODE(c2, 'MAX'), MODE(c2, 'AVG'), PERCENTILE(u, 99.9), "
                           f"MODE(u, 'MAX') FROM t{w}", three)
    if flt == "no_where":  # 3525 docs of each value: the tie the reducers decide
        assert blk.results[1] == {5: 3525, 9: 3525}
        assert reduce_blocks(op.query, [blk]).rows[0][1:4] == [5.0, 9.0, 7.0]
    blocks = op.launch_shape()["distinct_blocks"]
    # the regime the plan took, from its grid cap: four workgroups per CU in LDS, eight with global rows
    monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", "0")
    other = GpuInstancePlanMaker().make_instance_plan(parse(f"SELECT MODE(c2) FROM t{w}"), three)
    other.next_block()
    assert other.launch_shape()["distinct_blocks"] == blocks * (2 if regime == "lds" else 1)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_percentile_no_match_is_empty(regime, three, monkeypatch):
    _regime(monkeypatch, regime)
    op, blk = _check_plain(f"SELECT PERCENTILE50(i), MODE(i), PERCENTILE(d, 100), COUNT(*) FROM t WHERE {NONE}", three)
    assert blk.results[:3] == [{}, {}, {}]
    assert reduce_blocks(op.query, [blk]).rows == [[float("-inf"), float("-inf"), float("-inf"), 0]]


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_percentile_beside_distinctcount(regime, three, monkeypatch):
    """A bits slot and a counts slot of one column share a row (and a third slot of another column)."""
    _regime(monkeypatch, regime)
    for w in FILTERS.values():
        op, blk = _check_plain(f"SELECT DISTINCTCOUNT(i), PERCENTILE(i, 50), DISTINCTCOUNT(fl), MODE(l), SUM(m) FROM t{w}",
                               three)
        assert [p[0] for p in op.prims] == [_lib.AGG_DISTINCT, _lib.AGG_VALUE_COUNTS, _lib.AGG_DISTINCT,
                                            _lib.AGG_VALUE_COUNTS, _lib.AGG_SUM]
        assert len(blk.results[0]) == len(blk.results[1])  # the distinct values are the counted ones


@pytest.mark.parametrize("flt", list(FILTERS))
def test_gpu_percentile_mode_group_by(flt, three):
    w = FILTERS[flt]
    # one key column; two percentiles and a MODE of one column share a slot, beside the other functions
    q = (f"SELECT k1, PERCENTILE50(i), PERCENTILE(i, 99), MODE(i), COUNT(*), SUM(m), PERCENTILE90(d), MODE(c2, 'AVG') "
         f"FROM t{w} GROUP BY k1 LIMIT 1000")
    assert sum(p[0] == _lib.AGG_VALUE_COUNTS for p in GpuCombineOperator(parse(q), three, 100000).prims) == 3
    _check_groups(q, three, ["k1"])
    # two key columns (INT x STRING), and DISTINCTCOUNT beside the counts in the groups' rows
    _check_groups(f"SELECT k1, k2, PERCENTILE(fl, 75), MODE(m, 'AVG'), DISTINCTCOUNT(fl), MODE(l, 'MAX') FROM t{w} "
                  f"GROUP BY k1, k2 LIMIT 1000", three, ["k1", "k2"])
    # ORDER BY on a percentile: the broker reduce orders (11 groups, below every trim size)
    qo = f"SELECT k1, PERCENTILE90(i) FROM t{w} GROUP BY k1 ORDER BY PERCENTILE90(i) DESC, k1 LIMIT 3"
    qc, _, blk = _block(qo, three)
    ref = _matched_values(qc, [g.segment for g in three], "i", ["k1"])
    top = sorted(((-_ref_percentile(v, 90), k[0]) for k, v in ref.items()))[:3]
    assert reduce_blocks(qc, [blk]).rows == [[k, -p] for p, k in top]


# ---------------------------------------------------------------------------------------------- 3. re-execution, ABI
def _abi_rows(res):
    r = res.contents
    nd, ng, na = int(r.num_distinct), int(r.num_groups), int(r.num_aggregations)
    offs = [int(r.distinct_word_offsets[i]) for i in range(nd + 1)]
    words = np.ctypeslib.as_array(r.distinct_words, shape=(max(ng * offs[nd], 1),))[:ng * offs[nd]].copy()
    longs = [int(r.long_values[i]) for i in range(ng * na)]
    vals = [float(r.values[i]) for i in range(ng * na)]
    exact = [int(r.long_exact[i]) for i in range(na)]
    return nd, ng, na, offs, words.reshape(ng, offs[nd]), longs, vals, exact, int(r.reserved_distinct)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_percentile_reexecution_and_abi(regime, three, monkeypatch):
    """The same plan executed three times gives identical rows (the clear inside the sequence), laid out as the header
    says: a counts slot is card words, word j = the docs of dictionary entry j, the slot's value their sum."""
    _regime(monkeypatch, regime)
    lib = _lib.load()
    raws = [g.segment for g in three]
    for q, keys in ((f"SELECT PERCENTILE50(i), DISTINCTCOUNT(i), COUNT(*), MODE(fl) FROM t WHERE {ALL}", []),
                    (f"SELECT PERCENTILE50(i), DISTINCTCOUNT(i), COUNT(*), MODE(fl) FROM t WHERE {ONE_PERCENT}", []),
                    (f"SELECT k1, PERCENTILE50(i), DISTINCTCOUNT(i), COUNT(*), MODE(fl) FROM t WHERE {ALL} GROUP BY k1",
                     ["k1"]),
                    (f"SELECT PERCENTILE50(i), DISTINCTCOUNT(i), COUNT(*), MODE(fl) FROM t WHERE {NONE}", [])):
        qc = parse(q)
        matched = _matched(qc, raws)
        op = GpuCombineOperator(qc, three, 100000)
        assert [p[0] for p in op.prims] == [_lib.AGG_VALUE_COUNTS, _lib.AGG_DISTINCT, _lib.AGG_COUNT,
                                            _lib.AGG_VALUE_COUNTS]
        runs = []
        for _ in range(3):  # (the replay path starts from the second execution)
            res = op.run_raw()
            try:
                nd, ng, na, offs, words, longs, vals, exact, kinds = _abi_rows(res)
                cards = []
                for s in range(nd):
                    dv = _lib.DictionaryView()
                    _lib.check(lib.phip_result_distinct_dictionary(res, s, ctypes.byref(dv)))
                    cards.append(int(dv.cardinality))
            finally:
                lib.phip_result_free(res)
            runs.append((words.tobytes(), longs, vals))
            assert nd == 3 and kinds == 0b101  # slots in aggregation order: counts(i), bits(i), counts(fl)
            union_i = sorted({v for raw in raws for v in executor.OracleSegment(raw).dictionary("i").tolist()})
            assert cards[0] == cards[1] == len(union_i)
            assert [offs[s + 1] - offs[s] for s in range(3)] == [cards[0], (cards[1] + 31) // 32, cards[2]]
            total = 0
            for g in range(ng):
                for s, a in ((0, 0), (2, 3)):  # a counts slot's value: the docs it aggregated, exact
                    w = words[g, offs[s]:offs[s + 1]]
                    assert int(w.sum(dtype=np.int64)) == longs[g * na + a] == vals[g * na + a] == longs[g * na + 2]
                    assert exact[a] == 1
                total += longs[g * na + 0]
                # the bits slot of the same column marks exactly the counted ids
                bits = np.unpackbits(np.ascontiguousarray(words[g, offs[1]:offs[2]]).view(np.uint8), bitorder="little")
                assert np.array_equal(bits[:cards[0]].astype(bool), words[g, offs[0]:offs[1]] != 0)
            assert total == matched
            if not keys:  # the ids are the union dictionary's: word j counts union_i[j]
                ref = _ref_counts(_matched_values(qc, raws, "i")[()], False)
                w = words[0, offs[0]:offs[1]]
                assert {_canon(union_i[j]): int(w[j]) for j in np.nonzero(w)[0].tolist()} == ref
        assert runs[0] == runs[1] == runs[2]
        blocks = [op.next_block() for _ in range(3)]
        if keys:
            assert blocks[0].groups == blocks[1].groups == blocks[2].groups
        else:
            assert blocks[0].results == blocks[1].results == blocks[2].results
        op.close()


# ---------------------------------------------------------------------------------------------- 4. long waves
@pytest.fixture(scope="module")
def many(gpu_lib):
    rng = np.random.default_rng(41)
    segs = [GpuSegment(_segment(j, 6145, rng)) for j in range(12)]  # 12 x (three tiles and one doc): 48 tiles
    yield segs
    for s in segs:
        s.destroy()


@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_percentile_one_cu_grid(regime, many, monkeypatch):
    """PHIP_GRID_CUS=1: at most 4 (LDS) or 8 (global) workgroups of four waves walk the 48 tiles, so a wave takes
    several tiles and crosses from one segment into the next."""
    _regime(monkeypatch, regime)
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    op, _ = _check_plain(f"SELECT PERCENTILE50(i), MODE(c2), PERCENTILE99(d), DISTINCTCOUNT(i) FROM t WHERE {ALL}", many)
    s = op.launch_shape()
    assert s["total_work"] == 48 and s["distinct_blocks"] == (4 if regime == "lds" else 8), s
    op2, _ = _check_plain("SELECT PERCENTILE(l, 5), MODE(m, 'AVG') FROM t WHERE f < 10", many)
    _check_groups(f"SELECT k2, PERCENTILE50(i), MODE(m, 'AVG') FROM t WHERE {ALL} GROUP BY k2 LIMIT 1000", many, ["k2"])


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_gpu_percentile_mode_refusals(three, monkeypatch):
    lib = _lib.load()

    def usable():  # the library answers the next query
        _check_plain(f"SELECT PERCENTILE50(i) FROM t WHERE {ONE_PERCENT}", three)

    # a raw (no-dictionary) argument column: the plan maker refuses it, and so does the library when asked directly
    with pytest.raises(UnsupportedOnGpu):
        GpuInstancePlanMaker().make_instance_plan(parse(f"SELECT PERCENTILE50(r) FROM t WHERE {ONE_PERCENT}"), three)
    op = GpuCombineOperator(parse(f"SELECT SUM(r) FROM t WHERE {ONE_PERCENT}"), three, 100000)
    op.prims = [(_lib.AGG_VALUE_COUNTS, _lib.EXPR_COLUMN, "r", None, 0, 0)]
    with pytest.raises(UnsupportedOnGpu) as ei:
        op.run_raw()
    assert "raw" in str(ei.value) and ei.value.code == _lib.PHIP_ERR_UNSUPPORTED
    usable()
    # a STRING column, asked directly
    with pytest.raises(UnsupportedOnGpu):
        GpuInstancePlanMaker().make_instance_plan(parse(f"SELECT MODE(k2) FROM t WHERE {ONE_PERCENT}"), three)
    op = GpuCombineOperator(parse(f"SELECT DISTINCTCOUNT(k2) FROM t WHERE {ONE_PERCENT}"), three, 100000)
    op.prims = [(_lib.AGG_VALUE_COUNTS, _lib.EXPR_COLUMN, "k2", None, 0, 0)]
    with pytest.raises(UnsupportedOnGpu) as ei:
        op.run_raw()
    assert "STRING" in str(ei.value)
    usable()
    gq = f"SELECT k1, PERCENTILE50(i), COUNT(*) FROM t WHERE {ALL} GROUP BY k1 LIMIT 1000"
    # a hash-table key space (forced here; a large dense key space is re-sized into one late in plan creation)
    monkeypatch.setenv("PHIP_GB_HASH", "1")
    with pytest.raises(UnsupportedOnGpu) as ei:
        GpuCombineOperator(parse(gq), three, 100000).next_block()
    assert "hash-table" in str(ei.value)
    monkeypatch.delenv("PHIP_GB_HASH")
    usable()
    # the row budget counts a counts slot at 4 bytes per id: 11 dense keys x (>= 300 ids) x 4 bytes is above 8192,
    # where the same column's bitmap (11 x 10 words x 4 bytes) is not
    monkeypatch.setenv("PHIP_DISTINCT_MAX_BYTES", "8192")
    with pytest.raises(UnsupportedOnGpu) as ei:
        GpuCombineOperator(parse(gq), three, 100000).next_block()
    assert "PHIP_DISTINCT_MAX_BYTES" in str(ei.value)
    GpuCombineOperator(parse(gq.replace("PERCENTILE50(i)", "DISTINCTCOUNT(i)")), three, 100000).next_block()
    monkeypatch.delenv("PHIP_DISTINCT_MAX_BYTES")
    usable()
    # several segments reaching numGroupsLimit: a row holds a key's values over every segment, the limit is per segment
    op = GpuInstancePlanMaker().make_instance_plan(parse("SET numGroupsLimit = 3; " + gq), three)
    with pytest.raises(UnsupportedOnGpu) as ei:
        op.next_block()
    assert "numGroupsLimit" in str(ei.value)
    blk = _check_groups("SET numGroupsLimit = 1000; " + gq, three, ["k1"])
    assert not blk.num_groups_limit_reached
    # no partial table, no node plan
    op = GpuCombineOperator(parse(gq), three, 100000)
    assert op.execute_partial() is None
    monkeypatch.setenv("PHIP_NODE_SPLIT", "2")
    with pytest.raises(UnsupportedOnGpu) as ei:
        GpuCombineOperator(parse(gq), three, 100000).next_block()
    assert "node plan" in str(ei.value)
    monkeypatch.delenv("PHIP_NODE_SPLIT")
    usable()
    assert lib.phip_last_error() is not None
