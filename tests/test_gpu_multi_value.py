"""Multi-value columns on the GPU: the MV scan leaf (mv.hip mv_scan_kernel) and the six *MV aggregations over
row-reduction columns (mv_reduce_kernel), against the numpy restatement of the reference's semantics in tests/mv_ref.py.
Matched doc ids, counts, integer results and MIN / MAX are bit-exact; DOUBLE sums (of halves: exact) within the
project's 1e-9 relative tolerance.

Three segments of 5000 / 5003 / 4999 docs (three 2048-doc tiles each, none a multiple of 64) with their own
dictionaries, about 3 values per doc: a run of single-value docs, a row of ~700 values ending tile 0, a row that ends
exactly on a 64-value group boundary, a value that occurs only as the last value of one row and one only as the first
value of the next; id widths 1, 7, 12, 13 and 17 bits (the 17-bit column holds one row of 52 000 values: several passes
of the scan inside one tile). Every test that launches a kernel runs twice, the second time with PHIP_GRID_CUS=1: at most
8 scan workgroups then stride over a leaf's 32 tiles (its words are written up to a whole 65 536-doc key, so 29 of them
are padding tiles), which gives each of a segment's three real tiles its own workgroup. A workgroup walks several real
tiles -- the previous tile's LDS words, offsets and staged id set behind it -- where one plan holds several MV scan
leaves or segments: tile 0 of every leaf goes to workgroup 0 (the aggregation, group-by, FILTER and statistics tests,
and the two-leaf case of test_mv_leaf_with_other_leaves)."""
import numpy as np
import pytest

from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker
from pinot_amd.engine.reduce import reduce_blocks
from pinot_amd.engine.segment import GpuSegment
from pinot_amd.query.sql import parse
from tests import mv_ref

pytestmark = pytest.mark.gpu
REL = 1e-9
FUNCS = ("countmv", "summv", "minmv", "maxmv", "avgmv", "minmaxrangemv")


@pytest.fixture(scope="module")
def data(gpu_lib):
    refs = mv_ref.make_segments()
    raws = [r.build(f"mv{k}") for k, r in enumerate(refs)]
    gs = [GpuSegment(r) for r in raws]
    yield refs, raws, gs
    for s in gs:
        s.destroy()


@pytest.fixture(params=[None, "1"], ids=["grid", "grid1"])
def grid(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("PHIP_GRID_CUS", request.param)
    return request.param


def _words(mask):
    n = len(mask)
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = mask
    return np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def _check_docs(gs, refs, where, mask_fn):
    """The filter's doc set per segment, bit for bit (phip_filter_bitmap)."""
    qc = parse(f"SELECT COUNT(*) FROM t WHERE {where}")
    for g, r in zip(gs, refs):
        got = GpuCombineOperator(qc, [g], 100000).filter_bitmap()
        want = _words(mask_fn(r))
        assert np.array_equal(got, want), (where, g.name, np.nonzero(got != want)[0][:5])


def test_id_widths(data):
    _, raws, _ = data
    for col, (_, _, bits) in mv_ref.MV_COLUMNS.items():
        for raw in raws:
            m = raw.columns[col].metadata
            assert m.bits_per_element == bits and not m.is_single_value, (col, m)


# (where clause, numpy mask) -- b = the segment's value base (the dictionaries differ per segment)
def _filters():
    return [
        ("m7 = {b98}", lambda r: r.eq("m7", r.base + 98), "the value only at the end of a row"),
        ("m7 = {b99}", lambda r: r.eq("m7", r.base + 99), "the value only at the start of the next row"),
        ("m13 = {b5998}", lambda r: r.eq("m13", r.base + 5998), None),
        ("m13 = {b5999}", lambda r: r.eq("m13", r.base + 5999), None),
        ("m7 BETWEEN {b10} AND {b40}", lambda r: r.between("m7", r.base + 10, r.base + 40), None),
        ("m12 BETWEEN {h100} AND {h900}", lambda r: r.between("m12", (r.base + 100) * 0.5, (r.base + 900) * 0.5), None),
        ("m13 IN ({b3}, {b700}, {b5000}, {b5998})", lambda r: r.isin("m13", r.base + np.array([3, 700, 5000, 5998])), None),
        ("m7 <> {b5}", lambda r: r.not_in("m7", [r.base + 5]), None),
        ("m7 NOT IN ({b5}, {b50}, {b97})", lambda r: r.not_in("m7", r.base + np.array([5, 50, 97])), None),
        ("m13 NOT IN ({b0}, {b1}, {b2})", lambda r: r.not_in("m13", r.base + np.array([0, 1, 2])), None),
        ("m1 = {b1}", lambda r: r.eq("m1", r.base + 1), None),
        ("m1 <> {b1}", lambda r: r.not_in("m1", [r.base + 1]), None),
        ("m7 = -5", lambda r: np.zeros(r.n, bool), "no doc"),
        ("m7 >= 0", lambda r: np.ones(r.n, bool), "every doc"),
        ("m13 BETWEEN {b1} AND {b5990}", lambda r: r.between("m13", r.base + 1, r.base + 5990), "nearly every doc"),
        ("m17 BETWEEN {b3000} AND {b90000}", lambda r: r.between("m17", r.base + 3000, r.base + 90000), None),
        ("m17 IN ({b3}, {b30000}, {b150000})", lambda r: r.isin("m17", r.base + np.array([3, 30000, 150000])), None),
    ]


def _where(tmpl, r):
    class Sub(dict):
        def __missing__(self, key):
            return repr((r.base + int(key[1:])) * 0.5) if key[0] == "h" else str(r.base + int(key[1:]))
    return tmpl.format_map(Sub())


def test_mv_leaf_doc_sets(data, grid):
    refs, _, gs = data
    for tmpl, fn, _ in _filters():
        for g, r in zip(gs, refs):  # (per segment: the literal follows the segment's dictionary)
            _check_docs([g], [r], _where(tmpl, r), fn)


def test_special_values_land_on_their_docs(data):
    refs, _, _ = data
    for r in refs:  # (the data is what the test says it is)
        assert np.nonzero(r.eq("m7", r.base + 98))[0].tolist() == [mv_ref.SPECIAL_DOC]
        assert np.nonzero(r.eq("m7", r.base + 99))[0].tolist() == [mv_ref.SPECIAL_DOC + 1]
        off = r.mv["m7"][1]
        assert off[16] == 64 and off[mv_ref.LONG_ROW_DOC + 1] - off[mv_ref.LONG_ROW_DOC] >= 700


def test_mv_leaf_with_other_leaves(data, grid):
    """The MV leaf under AND / OR / NOT with an SV scan leaf, an inverted leaf and a sorted-range leaf."""
    refs, _, gs = data
    for g, r in zip(gs, refs):
        b = r.base
        sv = r.sv
        mv = r.between("m7", b + 10, b + 40)
        mv2 = r.not_in("m13", b + np.array([0, 1, 2, 700]))
        cases = [
            (f"m7 BETWEEN {b + 10} AND {b + 40} AND a < 25", mv & (sv["a"] < 25)),
            (f"m7 BETWEEN {b + 10} AND {b + 40} OR inv = 3", mv | (sv["inv"] == 3)),
            (f"NOT (m7 BETWEEN {b + 10} AND {b + 40}) AND srt BETWEEN 5 AND 20", ~mv & (sv["srt"] >= 5) & (sv["srt"] <= 20)),
            (f"(m7 BETWEEN {b + 10} AND {b + 40} AND inv IN (1, 5)) OR (m13 NOT IN ({b}, {b + 1}, {b + 2}, {b + 700}) AND "
             f"a > 40)", (mv & np.isin(sv["inv"], [1, 5])) | (mv2 & (sv["a"] > 40))),
            (f"NOT (m7 BETWEEN {b + 10} AND {b + 40} OR a < 10) AND m1 = {b + 1} AND srt > 3",
             ~(mv | (sv["a"] < 10)) & r.eq("m1", b + 1) & (sv["srt"] > 3)),
        ]
        for where, mask in cases:
            _check_docs([g], [r], where, lambda _r, m=mask: m)


@pytest.mark.parametrize("force", ["always", "never"])
def test_mv_inverted_index_both_ways(data, grid, monkeypatch, force):
    refs, raws, gs = data
    assert raws[0].columns["m7"].inverted is not None
    if force == "always":
        monkeypatch.setenv("PINOT_AMD_INVERTED", "always")
    else:
        monkeypatch.setenv("PINOT_AMD_INVERTED_RATIO", "0")
    for g, r in zip(gs, refs):
        b = r.base
        _check_docs([g], [r], f"m7 IN ({b + 5}, {b + 50}, {b + 98})", lambda x: x.isin("m7", x.base + np.array([5, 50, 98])))
        _check_docs([g], [r], f"m7 NOT IN ({b + 5}, {b + 50}, {b + 98})", lambda x: x.not_in("m7", x.base + np.array([5, 50, 98])))
        _check_docs([g], [r], f"m7 = {b + 99}", lambda x: x.eq("m7", x.base + 99))


def _expect(refs, col, masks):
    return mv_ref.finals(*mv_ref.combine([r.intermediates(col, m) for r, m in zip(refs, masks)]))


def _close(got, want):
    if isinstance(want, int):
        return got == want
    if want == got:
        return True
    return np.isfinite(want) and abs(got - want) <= REL * abs(want)


def _select(col):
    return ", ".join(f"{f.upper()}({col})" for f in FUNCS)


@pytest.mark.parametrize("col", ["m1", "m7", "m12", "m13", "m17"])
def test_aggregations_alone_and_filtered(data, grid, col):
    """The six functions alone, beside single-value aggregations, and under a filter on another column."""
    refs, _, gs = data
    pm = GpuInstancePlanMaker()
    for where, masks in (("", [np.ones(r.n, bool) for r in refs]), (" WHERE a < 20", [r.sv["a"] < 20 for r in refs]),
                         (" WHERE a < 0", [np.zeros(r.n, bool) for r in refs])):
        want = _expect(refs, col, masks)
        qc = parse(f"SELECT {_select(col)}, COUNT(*), SUM(v), MAX(a) FROM t{where}")
        blk = pm.make_instance_plan(qc, gs).next_block()
        row = reduce_blocks(qc, [blk]).rows[0]
        for f, got in zip(FUNCS, row):
            if f in ("countmv", "minmv", "maxmv", "minmaxrangemv") or want["countmv"] == 0:
                assert got == want[f] or (np.isnan(want[f]) and np.isnan(got)), (col, where, f, got, want[f])
            else:
                assert _close(got, want[f]), (col, where, f, got, want[f])
        assert type(row[0]) is int
        n = sum(int(m.sum()) for m in masks)
        assert row[6] == n and row[7] == float(sum(int(r.sv["v"][m].sum()) for r, m in zip(refs, masks)))
        if where:
            assert blk.stats.num_docs_scanned == n
        # each function on its own gives the same answer
        if not where:
            continue
        for f in FUNCS:
            q1 = parse(f"SELECT {f.upper()}({col}) FROM t{where}")
            got = reduce_blocks(q1, [pm.make_instance_plan(q1, gs).next_block()]).rows[0][0]
            assert _close(got, want[f]) or want["countmv"] == 0, (col, f, got, want[f])


def test_unfiltered_extremes_come_from_the_dictionaries(data):
    """MINMV / MAXMV / MINMAXRANGEMV without a filter: NonScanBasedAggregationOperator (AggregationPlanNode.java:52-59),
    with its statistics: every doc scanned, no entry."""
    refs, _, gs = data
    qc = parse("SELECT MINMV(m13), MAXMV(m13), MINMAXRANGEMV(m12) FROM t")
    op = GpuInstancePlanMaker().make_instance_plan(qc, gs)
    assert op._non_scan_fit()
    blk = op.next_block()
    n = sum(r.n for r in refs)
    assert (blk.stats.num_docs_scanned, blk.stats.num_entries_scanned_in_filter,
            blk.stats.num_entries_scanned_post_filter) == (n, 0, 0)
    ones = [np.ones(r.n, bool) for r in refs]
    w13, w12 = _expect(refs, "m13", ones), _expect(refs, "m12", ones)
    assert reduce_blocks(qc, [blk]).rows[0] == [w13["minmv"], w13["maxmv"], w12["minmaxrangemv"]]


@pytest.mark.parametrize("col", ["m7", "m12", "m17"])
def test_group_by_sv_key(data, grid, col):
    refs, _, gs = data
    qc = parse(f"SELECT k, {_select(col)}, SUM(v) FROM t WHERE inv < 9 GROUP BY k LIMIT 100")
    blk = GpuInstancePlanMaker().make_instance_plan(qc, gs).next_block()
    rows = {r[0]: r[1:] for r in reduce_blocks(qc, [blk]).rows}
    keys = sorted(set(np.concatenate([r.sv["k"] for r in refs]).tolist()))
    assert sorted(rows) == keys
    for key in keys:
        masks = [(r.sv["inv"] < 9) & (r.sv["k"] == key) for r in refs]
        want = _expect(refs, col, masks)
        for f, got in zip(FUNCS, rows[key]):
            assert _close(got, want[f]), (col, key, f, got, want[f])
        assert rows[key][6] == float(sum(int(r.sv["v"][m].sum()) for r, m in zip(refs, masks)))


def test_filter_clauses(data, grid):
    """FILTER(WHERE ...) programs, one of them over a multi-value column, with and without GROUP BY."""
    refs, _, gs = data
    f1, f2 = "a < 20", "m1 = 1 OR m1 = 1001 OR m1 = 2001"
    masks1 = [r.sv["a"] < 20 for r in refs]
    masks2 = [r.eq("m1", r.base + 1) for r in refs]
    qc = parse(f"SELECT SUMMV(m7) FILTER(WHERE {f1}), COUNTMV(m7) FILTER(WHERE {f2}), MAXMV(m13) FILTER(WHERE {f1}), "
               f"AVGMV(m12) FILTER(WHERE {f2}), COUNT(*), MINMAXRANGEMV(m13) FILTER(WHERE {f2}), "
               f"MINMV(m7) FILTER(WHERE {f1}) FROM t")
    row = reduce_blocks(qc, [GpuInstancePlanMaker().make_instance_plan(qc, gs).next_block()]).rows[0]
    assert row[0] == _expect(refs, "m7", masks1)["summv"]
    assert row[1] == _expect(refs, "m7", masks2)["countmv"]
    assert row[2] == _expect(refs, "m13", masks1)["maxmv"]
    assert _close(row[3], _expect(refs, "m12", masks2)["avgmv"])
    assert row[4] == sum(r.n for r in refs)
    assert row[5] == _expect(refs, "m13", masks2)["minmaxrangemv"]
    assert row[6] == _expect(refs, "m7", masks1)["minmv"]
    qg = parse(f"SELECT k, SUMMV(m7) FILTER(WHERE {f1}), MINMV(m13) FILTER(WHERE {f2}), "
               f"MINMAXRANGEMV(m12) FILTER(WHERE {f1}) FROM t GROUP BY k LIMIT 100")
    rows = {r[0]: r[1:] for r in reduce_blocks(qg, [GpuInstancePlanMaker().make_instance_plan(qg, gs).next_block()]).rows}
    for key, got in rows.items():
        k1 = [m & (r.sv["k"] == key) for r, m in zip(refs, masks1)]
        k2 = [m & (r.sv["k"] == key) for r, m in zip(refs, masks2)]
        assert got[0] == _expect(refs, "m7", k1)["summv"] and got[1] == _expect(refs, "m13", k2)["minmv"], (key, got)
        assert got[2] == _expect(refs, "m12", k1)["minmaxrangemv"], (key, got)


def test_reduction_column_is_cached(data, grid):
    """A second plan over the same segment finds the row-reduction column (no new materialise launch) and gives the same
    answer."""
    refs, _, gs = data
    qc = parse("SELECT SUMMV(m13), COUNTMV(m13) FROM t WHERE a < 30")
    pm = GpuInstancePlanMaker()
    first = reduce_blocks(qc, [pm.make_instance_plan(qc, gs[:1]).next_block()]).rows[0]
    builds = gs[0].derived_info()[2]
    second = reduce_blocks(qc, [pm.make_instance_plan(qc, gs[:1]).next_block()]).rows[0]
    assert gs[0].derived_info()[2] == builds and first == second
    want = _expect(refs[:1], "m13", [refs[0].sv["a"] < 30])
    assert first == [want["summv"], want["countmv"]]


def test_statistics(data, grid):
    """numEntriesScannedInFilter of an MV scan leaf counts values, not docs (MVScanDocIdIterator: _numEntriesScanned +=
    length) -- under the all-segment scan the segment's total values; numEntriesScannedPostFilter one entry per
    projected multi-value column per matched doc; numDocsScanned the matched docs."""
    refs, _, gs = data
    masks = [r.between("m7", 10, 40) for r in refs]  # (values of segment 0's dictionary only)
    qc = parse("SELECT COUNTMV(m13), SUMMV(m13), MAXMV(m12) FROM t WHERE m7 BETWEEN 10 AND 40")
    blk = GpuInstancePlanMaker().make_instance_plan(qc, gs).next_block()
    matched = sum(int(m.sum()) for m in masks)
    scanned = sum(int(r.mv["m7"][1][-1]) for r, m in zip(refs, masks) if r.base <= 40)  # (other segments: no id matches)
    assert blk.stats.num_docs_scanned == matched
    assert blk.stats.num_entries_scanned_in_filter == scanned
    assert blk.stats.num_entries_scanned_post_filter == 2 * matched
    assert blk.stats.num_total_docs == sum(r.n for r in refs)
