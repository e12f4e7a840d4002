"""Every tile walk with many tiles and several segment changes per wave (PHIP_GRID_CUS=1), against the CPU oracle.

On an MI355X the grids follow 256 CUs, so the rest of the suite gives a wave zero or one tile: the state a wave carries
from one tile to the next (the filter's LDS-DMA ring and counted waits, its segment cursor and deferred rings, the
aggregation kernel's mask queue, doc ring, LDS dictionaries and histogram bins, the distinct and selection walks'
segment cursors) only runs at production sizes. PHIP_GRID_CUS=1 sizes every tile-walking grid as for one CU -- 8
workgroups at most -- so the ~450 tiles of tests/long_waves_data.py (36 segments, column widths 3 / 11 / 17 bits side by
side, segments the planner drops) give a filter wave 14+ tiles and an aggregation wave 3.5-7, and every case asserts
from phip_plan_launch_shape that its execution really had that shape:

    total_work >= 10 x filter_blocks x 4        (more tiles per filter wave than kMaxRing = 8: the ring wraps)
    total_work >= 6 x agg_blocks x 8            (8-wave workgroups: more than kMaskAhead + 1 = 5 tiles per wave)
    total_work >= 3 x agg_blocks x 16           (16-wave workgroups)
    num_work_segments >= 24

The reference is oracle/executor.py over the same raw segments (for DISTINCTCOUNT the numpy reference of
tests/test_gpu_distinct_count.py over the oracle's filter masks), never a second run of the library. Compared exactly:
counts, int64 sums (the oracle's Python integers; m holds random 38-bit values, so a lost or doubled doc changes the
sum, and the library must return it as an exact integer), MIN / MAX, group key sets, HLL registers, distinct sets, selection rows, numDocsScanned, the docs matched per
segment, and the sums of d -- multiples of 0.25 below 2^30, exact in any order -- bit for bit. numEntriesScannedInFilter
is compared where the filter is a conjunction of scan leaves without a sorted range (one entry per doc of a kept
segment and scan leaf; the oracle does not model it, and an OR's short-circuit depends on the tiles).
"""
import struct

import numpy as np
import pytest

from oracle import executor
from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker
from pinot_amd.engine.reduce import trim_groups
from pinot_amd.query.context import Identifier
from pinot_amd.query.sql import parse
from tests import long_waves_data as lw
from tests.test_gpu_parity import _assert_intermediates_equal, _words_from_mask

pytestmark = pytest.mark.gpu

DENSE = "tag >= 2 AND nr < 90"          # ~72 % of the kept segments' docs; the `low` segments are dropped
SPARSE = "tag = 7 AND nr < 30"          # ~3 %
SORTED = f"ts BETWEEN {lw.TS_LO} AND {lw.TS_HI} AND nr < 50"   # drops the last segment, cuts the first and one more
FILTERS = {"dense": DENSE, "sparse": SPARSE}


@pytest.fixture(scope="module")
def segs(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    raws = lw.raw_segments()
    g = [GpuSegment(r) for r in raws]
    yield raws, g
    for s in g:
        s.destroy()


_ORACLE = {}


def _oracle(sql, raws, limit=None):
    """(query, oracle block, exact sums, docs matched per segment), computed once per query and left unchanged."""
    key = (sql, limit)
    if key not in _ORACLE:
        qc = parse(sql)
        kw = {} if limit is None else {"num_groups_limit": limit}
        oblk, exact = executor.execute(qc, raws, **kw)
        _ORACLE[key] = (qc, oblk, exact, _matched(sql, raws))
    return _ORACLE[key]


_MATCHED = {}


def _matched(sql, raws):
    where = sql.split(" WHERE ", 1)[1].split(" GROUP BY ")[0].split(" LIMIT ")[0] if " WHERE " in sql else None
    if where not in _MATCHED:
        qc = parse(f"SELECT COUNT(*) FROM t WHERE {where}") if where else None
        _MATCHED[where] = [int(np.count_nonzero(executor.filter_mask(qc, r))) if qc else r.num_docs for r in raws]
    return _MATCHED[where]


def _core(op):
    """The GpuCombineOperator that owns the prepared plan, under the operators that wrap it."""
    while not isinstance(op, GpuCombineOperator):
        op = getattr(op, "one_pass", None) or op.__dict__.get("inner") or op.__dict__["op"]
    return op


def _assert_long_waves(op):
    s = _core(op).launch_shape()
    assert s is not None and s["total_work"] > 0, s
    assert s["total_work"] >= 10 * s["filter_blocks"] * 4, s
    assert s["agg_waves"] in (8, 16), s
    assert s["total_work"] >= (6 if s["agg_waves"] == 8 else 3) * s["agg_blocks"] * s["agg_waves"], s
    assert s["num_work_segments"] >= 24, s
    assert 2 <= s["nbuf"] <= 8, s
    return s


def _bits(x):
    return struct.pack("<d", float(x))


def _check_values(qc, got, want, exact):
    _assert_intermediates_equal(qc.aggregations, got, want, exact)
    for ag, g, o in zip(qc.aggregations, got, want):
        if ag.function == "sum" and isinstance(ag.argument, Identifier) and ag.argument.name in ("m", "sk"):
            assert isinstance(g, int), (str(ag), g)  # (compared with the oracle's exact integer above)
        if ag.function == "sum" and isinstance(ag.argument, Identifier) and ag.argument.name == "d":
            assert _bits(g) == _bits(o), (str(ag), g, o)  # the 0.25-grid sums: exact in any order


def _check_block(qc, blk, oblk, exact):
    assert blk.stats.num_docs_scanned == oblk.stats.num_docs_scanned
    if not qc.group_by:
        _check_values(qc, blk.results, oblk.results, exact)
        return
    if getattr(blk, "num_groups_trimmed", False):
        oblk = trim_groups(qc, oblk)
    assert blk.num_groups_limit_reached == oblk.num_groups_limit_reached
    assert set(blk.groups) == set(oblk.groups)
    for k, v in oblk.groups.items():
        _check_values(qc, blk.groups[k], v, exact[k])


def _scan_entries(raws, leaves):
    """numEntriesScannedInFilter of a conjunction of scan leaves (no sorted column): per kept segment one entry per doc
    and leaf; a leaf no doc / every doc of a segment passes folds to a constant (every dictionary value occurs), and a
    match-none leaf drops the segment."""
    total = 0
    for r in raws:
        masks = [np.asarray(executor.filter_mask(parse(f"SELECT COUNT(*) FROM t WHERE {p}"), r), dtype=bool) for p in leaves]
        if any(not m.any() for m in masks):
            continue
        total += sum(0 if m.all() else 1 for m in masks) * r.num_docs
    return total


def _run(sql, segs, monkeypatch, env=(), limit=None, executions=1, walk_check=None, entries=None, cap="1"):
    """One plan under the cap and the case's switches: every execution equals the oracle and had the long-wave shape."""
    raws, g = segs
    if cap is None:
        monkeypatch.delenv("PHIP_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("PHIP_GRID_CUS", cap)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    qc, oblk, exact, matched = _oracle(sql, raws, limit)
    kw = {} if limit is None else {"num_groups_limit": limit}
    op = GpuInstancePlanMaker(**kw).make_instance_plan(qc, g)
    try:
        for _ in range(executions):
            blk = op.next_block()
            shape = _assert_long_waves(op) if cap is not None else None
            _check_block(qc, blk, oblk, exact)
            if getattr(blk, "segment_docs_matched", None) is not None:
                assert list(blk.segment_docs_matched) == matched
            if entries is not None:
                assert blk.stats.num_entries_scanned_in_filter == entries
            assert (blk.filter_kernel_ms or 0) + (blk.agg_kernel_ms or 0) > 0, "did not run on the GPU"
            if walk_check is not None:
                walk_check(blk)
        if type(op) is GpuCombineOperator and not qc.group_by and not op._non_scan_fit():
            # (an aggregation block does not carry the docs matched per segment: read them from one more execution)
            res = op.run_raw()
            try:
                r = res.contents
                assert r.num_segments_processed == len(raws)
                assert [int(r.segment_docs_matched[i]) for i in range(len(raws))] == matched
            finally:
                op._lib.phip_result_free(res)
    finally:
        op.close()
    return shape


def _fused(blk):
    assert blk.fused and blk.agg_kernel_ms == 0.0, (blk.fused, blk.agg_kernel_ms)


def _unfused(blk):
    assert not blk.fused and blk.agg_kernel_ms > 0.0, (blk.fused, blk.agg_kernel_ms)


def test_gpu_long_waves_shape_follows_the_cap(segs, monkeypatch):
    """The cap changes the grids and nothing else: one CU gives at most 8 workgroups per launch; unset, the same plan
    spreads over the device (no wave gets two tiles of this input) with the same work list, ring depth and waves."""
    raws, g = segs
    qc = parse(f"SELECT COUNT(*), SUM(m) FROM t WHERE {DENSE}")
    shapes = {}
    for cap in ("1", "2", None):
        monkeypatch.setenv("PHIP_FUSE", "0")
        if cap is None:
            monkeypatch.delenv("PHIP_GRID_CUS", raising=False)
        else:
            monkeypatch.setenv("PHIP_GRID_CUS", cap)
        op = GpuInstancePlanMaker().make_instance_plan(qc, g)
        assert op.launch_shape() is None
        op.next_block()
        shapes[cap] = op.launch_shape()
        op.close()
    one, two, free = shapes["1"], shapes["2"], shapes[None]
    # the work list: the segments in which each leaf matches some doc (a match-none leaf drops the segment)
    kept = [r for r in raws if all(np.count_nonzero(executor.filter_mask(parse(f"SELECT COUNT(*) FROM t WHERE {p}"), r))
                                   for p in ("tag >= 2", "nr < 90"))]
    tiles = sum(lw.tiles(r.num_docs) for r in kept)
    assert one["total_work"] == two["total_work"] == free["total_work"] == tiles
    assert one["num_work_segments"] == free["num_work_segments"] == len(kept) < len(raws) - 3
    assert one["filter_blocks"] <= 8 and one["agg_blocks"] == 8 and two["filter_blocks"] <= 16
    assert one["filter_blocks"] < two["filter_blocks"]
    assert free["filter_blocks"] == (tiles + 3) // 4 and free["agg_blocks"] == 8 * ((tiles + 63) // 64)
    assert one["agg_waves"] == free["agg_waves"] == 8 and one["nbuf"] == free["nbuf"]
    assert one["select_blocks"] == 8 and free["select_blocks"] == 4096


# ---------------------------------------------------------------------------------------------- filter walks
INTERP = "(tag >= 2 AND NOT (w < 9 OR nr > 80)) OR wd < 1000"
FILTER_CASES = {
    # id: (where clauses, switches)
    "interpreter": ([INTERP, "NOT (tag < 9 OR nr > 3) OR (w = 6 AND wd < 50000)"], {"PHIP_CONTIG": "0"}),
    "contiguous": ([INTERP, "NOT (tag < 9 OR nr > 3) OR (w = 6 AND wd < 50000)"], {"PHIP_CONTIG": "1"}),
    "bitsliced": ([f"{DENSE} AND w < 3000", f"{SPARSE} AND w >= 6"], {}),
    "not_bitsliced": ([f"{DENSE} AND w < 3000", f"{SPARSE} AND w >= 6"], {"PHIP_NO_BITSLICE": "1"}),
    "inverted_and_scan": (["inv IN (3, 7, 11) AND tag >= 2", "inv = 5 AND tag = 7"], {"PINOT_AMD_INVERTED": "always"}),
    "sorted_range": ([SORTED, f"ts BETWEEN {lw.TS_LO} AND {lw.TS_HI} AND inv = 4"], {}),
    "raw_long": (["rl < 137438953472 AND tag >= 2", "rl < 2748779069 AND tag >= 2"], {}),
    "raw_string": (["rs IN ('a', 'k7', 'mid') AND tag >= 2", "rs >= 'q' AND tag = 7"], {}),
    "walk_contig": ([f"{DENSE} AND wd < 800000", SPARSE], {"PHIP_FILTER_WALK": "contig"}),
    "walk_xcd": ([f"{DENSE} AND wd < 800000", SPARSE], {"PHIP_FILTER_WALK": "xcd"}),
    "walk_xcdc": ([f"{DENSE} AND wd < 800000", SPARSE], {"PHIP_FILTER_WALK": "xcdc"}),
}


@pytest.mark.parametrize("case", list(FILTER_CASES))
def test_gpu_long_waves_filter(case, segs, monkeypatch):
    """The filter kernel alone (its tile masks feed the separate aggregation kernel): the lane-major interpreter and
    the contiguous evaluator on OR / NOT programs, the conjunction bit-sliced and not, an inverted leaf beside a scan
    leaf, a sorted range that drops and cuts segments, raw LONG and raw STRING leaves, and the three tile orders."""
    wheres, env = FILTER_CASES[case]
    for where in wheres:
        _run(f"SELECT COUNT(*), SUM(m), SUM(d) FROM t WHERE {where}", segs, monkeypatch, dict(env, PHIP_FUSE="0"),
             walk_check=_unfused)


@pytest.mark.parametrize("flt", list(FILTERS))
def test_gpu_long_waves_count_only_conjunction(flt, segs, monkeypatch):
    """COUNT(*) of a conjunction: the filter kernel's matched-doc partials and per-segment counts are the result, and
    every scan leaf counts one entry per doc of a kept segment."""
    where = FILTERS[flt] + " AND w >= 6"
    leaves = ["tag >= 2" if flt == "dense" else "tag = 7", "nr < 90" if flt == "dense" else "nr < 30", "w >= 6"]
    _run(f"SELECT COUNT(*) FROM t WHERE {where}", segs, monkeypatch, entries=_scan_entries(segs[0], leaves))


def test_gpu_long_waves_filter_bitmap_per_segment(segs, monkeypatch):
    """filter_bitmap takes one segment at a time: the 1-doc, the 2049-doc and a bulk segment under the cap."""
    raws, g = segs
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    for where in (DENSE, INTERP, SORTED):
        qc = parse(f"SELECT COUNT(*) FROM t WHERE {where}")
        for i in (1, 15, 3):
            assert lw.LAYOUT[i][0] in (1, 2049, 70_003)
            words = GpuInstancePlanMaker().make_instance_plan(qc, [g[i]]).filter_bitmap()
            assert np.array_equal(words, _words_from_mask(executor.filter_mask(qc, raws[i]))), (where, i)


# ---------------------------------------------------------------------------------------------- fused aggregation
FUSED_AGGS = {1: "SUM(m)", 2: "SUM(m), SUM(d)", 4: "COUNT(*), SUM(m), SUM(d), MAX(wd)"}


@pytest.mark.parametrize("stream", ["0", "1"], ids=["gather", "stream"])
@pytest.mark.parametrize("defer", ["0", "1"], ids=["per_tile", "deferred"])
@pytest.mark.parametrize("naggs", list(FUSED_AGGS))
def test_gpu_long_waves_fused_aggregation(naggs, defer, stream, segs, monkeypatch):
    """The filter kernel aggregates its own tiles: values gathered per tile, collected in the deferred ring across tiles
    and segments (flushed before a segment change), or streamed with the tile."""
    env = {"PHIP_FUSE": "1", "PHIP_FUSED_DEFER": defer, "PHIP_STREAM_VALUES": stream}
    for where in (DENSE, SPARSE, SORTED):
        _run(f"SELECT {FUSED_AGGS[naggs]} FROM t WHERE {where}", segs, monkeypatch, env, walk_check=_fused)


# ---------------------------------------------------------------------------------------------- unfused aggregation
WALKS = {"chunks": ("0", "0", "0"), "batch": ("1", "0", "0"), "staged": ("1", "1", "0"),
         "staged_lds_dict": ("1", "1", "1")}


@pytest.mark.parametrize("walk", list(WALKS))
def test_gpu_long_waves_aggregation_walks(walk, segs, monkeypatch):
    """The aggregation kernel's four walks over the tile masks: dictionary and raw columns, a small dictionary (sk: the
    LDS dictionaries reload at a segment change), dense and sparse masks, a filter that cuts tiles."""
    db, st, ld = WALKS[walk]
    env = {"PHIP_FUSE": "0", "PHIP_DENSE_BATCH": db, "PHIP_AGG_STAGE": st, "PHIP_AGG_LDS_DICT": ld, "PHIP_AGG_HIST": "0"}
    for where in (DENSE, SPARSE, SORTED):
        _run(f"SELECT COUNT(*), SUM(m), SUM(d), MIN(wd), MAX(rl), SUM(gr), SUM(sk) FROM t WHERE {where}", segs,
             monkeypatch, env, walk_check=_unfused)


@pytest.mark.parametrize("sql", ["SELECT SUM(sk), COUNT(*) FROM t WHERE tag >= 2",
                                 "SELECT MIN(sk), MAX(sk) FROM t WHERE tag >= 2 AND nr < 95",
                                 "SELECT SUM(sk) FROM t WHERE " + SPARSE], ids=["sum", "min_max", "sparse"])
def test_gpu_long_waves_histogram(sql, segs, monkeypatch):
    """The id histogram (from the execution after one in which 30 % of the docs matched): its bins are folded and
    cleared at every segment change inside a wave. Three executions: value gathers, then the histogram twice."""
    _run(sql, segs, monkeypatch, {"PHIP_FUSE": "0"}, executions=3, walk_check=_unfused)


# ---------------------------------------------------------------------------------------------- group-by
GB = "SELECT g, COUNT(*), SUM(m), SUM(d), MAX(wd) FROM t WHERE {w} GROUP BY g LIMIT 100000"
GROUP_WALKS = {
    "lds_one_chunk_8": (GB, {"PHIP_FUSED_GB": "0", "PHIP_GB_BATCH": "0", "PHIP_GB_WAVES": "8"}),
    "lds_one_chunk_16": (GB, {"PHIP_FUSED_GB": "0", "PHIP_GB_BATCH": "0", "PHIP_GB_WAVES": "16"}),
    "lds_batched_8": (GB, {"PHIP_FUSED_GB": "0", "PHIP_GB_BATCH": "1", "PHIP_GB_WAVES": "8"}),
    "lds_batched_16": (GB, {"PHIP_FUSED_GB": "0", "PHIP_GB_BATCH": "1", "PHIP_GB_WAVES": "16"}),
    "global_table": (GB, {"PHIP_FUSED_GB": "0", "PHIP_GB_MODE": "global"}),
    "fused_hbm": (GB, {"PHIP_FUSED_GB": "2"}),
    "fused_xcd": (GB, {"PHIP_FUSED_GB": "3"}),
    "fused_lds": (GB, {"PHIP_FUSED_GB": "4"}),
    "hash": ("SELECT hk, COUNT(*), SUM(m), SUM(d) FROM t WHERE {w} GROUP BY hk LIMIT 10000000",
             {"PHIP_GB_HASH": "1", "PHIP_FUSED_GB": "0"}),
    "records": ("SELECT g, tag, COUNT(*), SUM(m), SUM(d), MAX(wd) FROM t WHERE {w} GROUP BY g, tag LIMIT 100000",
                {"PHIP_GB_RECORD": "1", "PHIP_MATERIALIZE_MIN_DICT": "0", "PHIP_FUSED_GB": "0"}),
    "raw_key": ("SELECT gr, COUNT(*), SUM(m), SUM(d) FROM t WHERE {w} GROUP BY gr LIMIT 100000", {}),
    "hll": ("SELECT g, DISTINCTCOUNTHLL(hk), COUNT(*), SUM(m) FROM t WHERE {w} GROUP BY g LIMIT 100000",
            {"PHIP_FUSED_GB": "0"}),
}


def _group_walk_check(walk):
    def check(blk):
        if walk in ("fused_hbm", "fused_xcd", "fused_lds"):
            _fused(blk)
        elif walk != "raw_key":
            _unfused(blk)
    return check


@pytest.mark.parametrize("walk", list(GROUP_WALKS))
def test_gpu_long_waves_group_by(walk, segs, monkeypatch):
    """Group-by on every table placement: the LDS table one chunk at a time and batched in 8- and 16-wave workgroups,
    the global table, the three fused tables, the hash table, group-by records, a raw key and HLL registers; two
    executions (the second may take the other LDS walk). The docs matched per segment are compared too."""
    sql, env = GROUP_WALKS[walk]
    # (the hash case's 30 K groups per segment: a quarter of the dense filter's docs keeps the oracle quick)
    for where in (DENSE if walk != "hash" else "tag >= 2 AND nr < 25", SPARSE):
        shape = _run(sql.format(w=where), segs, monkeypatch, env, executions=2,
                     walk_check=_group_walk_check(walk))
        if "PHIP_GB_WAVES" in env:
            assert shape["agg_waves"] == int(env["PHIP_GB_WAVES"]), shape


# ---------------------------------------------------------------------------------------------- other passes
def test_gpu_long_waves_filter_clause_programs(segs, monkeypatch):
    """FILTER (WHERE): two filter programs in one pass, each with its own work-list entries and tile masks."""
    shape = _run("SELECT SUM(m) FILTER (WHERE nr < 50), SUM(d) FILTER (WHERE nr >= 50 AND w >= 6) FROM t WHERE tag >= 2",
                 segs, monkeypatch)
    assert shape["num_work_segments"] >= 2 * 24


def test_gpu_long_waves_null_handling(segs, monkeypatch):
    """enableNullHandling: the null vectors' leaves and the hidden counts, with segments that have no null vector."""
    raws, g = segs
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    sql = "SET enableNullHandling = true; SELECT SUM(nl), COUNT(nl), MIN(nl), MAX(m), COUNT(*) FROM t WHERE tag >= 2"
    qc = parse(sql)
    oblk, exact = executor.execute(qc, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, g)
    try:
        blk = op.next_block()
        _assert_long_waves(op)
        assert blk.stats.num_docs_scanned == oblk.stats.num_docs_scanned
        assert blk.stats.num_entries_scanned_post_filter == oblk.stats.num_entries_scanned_post_filter
        assert all(o is not None for o in oblk.results)
        _assert_intermediates_equal(qc.aggregations, blk.results, oblk.results, exact)
    finally:
        op.close()


@pytest.mark.parametrize("regime", ["lds", "global"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "group_by"])
def test_gpu_long_waves_distinct_count(grouped, regime, segs, monkeypatch):
    """The distinct pass: its segment cursor over many segments per wave, in the LDS and the global regime. w's
    query-global dictionary is the union of 3-, 11- and 17-bit segment dictionaries."""
    from tests.test_gpu_distinct_count import _canon_set, _reference
    raws, g = segs
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    if regime == "global":
        monkeypatch.setenv("PHIP_DISTINCT_LDS_WORDS", "0")
    for where in (DENSE, SPARSE):
        sql = (f"SELECT g, DISTINCTCOUNT(w), COUNT(*), SUM(m) FROM t WHERE {where} GROUP BY g LIMIT 100000" if grouped
               else f"SELECT DISTINCTCOUNT(w), DISTINCTCOUNT(inv), COUNT(*), SUM(m) FROM t WHERE {where}")
        qc = parse(sql)
        op = GpuInstancePlanMaker().make_instance_plan(qc, g)
        try:
            blk = op.next_block()
            shape = _assert_long_waves(op)
            assert 10 * shape["distinct_blocks"] * 4 <= shape["total_work"], shape
            matched = _matched(sql, raws)
            assert blk.stats.num_docs_scanned == sum(matched)
            ref_w = _reference(qc, raws, "w", ["g"] if grouped else ())
            counts = parse(sql.replace("DISTINCTCOUNT(w), ", "").replace("DISTINCTCOUNT(inv), ", ""))
            oblk, exact = executor.execute(counts, raws)
            if grouped:
                assert set(blk.groups) == set(ref_w) == set(oblk.groups)
                for k in ref_w:
                    assert _canon_set(blk.groups[k][0]) == ref_w[k], k
                    assert blk.groups[k][1] == oblk.groups[k][0] and blk.groups[k][2] == exact[k][1], k
                assert list(blk.segment_docs_matched) == matched
            else:
                assert _canon_set(blk.results[0]) == ref_w[()]
                assert _canon_set(blk.results[1]) == _reference(qc, raws, "inv")[()]
                assert blk.results[2] == oblk.results[0] and blk.results[3] == exact[1]
        finally:
            op.close()


@pytest.mark.parametrize("sql", [f"SELECT m, rs, g, d FROM t WHERE {SPARSE} LIMIT 10000000",
                                 f"SELECT rl, w FROM t WHERE {DENSE} LIMIT 100000"],
                         ids=["every_match", "limit_ends_inside_a_segment"])
def test_gpu_long_waves_selection(sql, segs, monkeypatch):
    """The selection passes (count, gather) over many segments per wave: the rows in segment and doc order."""
    from tests.test_gpu_selection import _same
    raws, g = segs
    monkeypatch.setenv("PHIP_GRID_CUS", "1")
    qc = parse(sql)
    oblk, _ = executor.execute(qc, raws)
    op = GpuInstancePlanMaker().make_instance_plan(qc, g)
    try:
        blk = op.next_block()
        shape = _assert_long_waves(op)
        assert 10 * shape["select_blocks"] * 4 <= shape["total_work"], shape
        assert blk.column_names == oblk.column_names and blk.column_types == oblk.column_types
        assert blk.num_rows == oblk.num_rows > 0
        assert blk.stats.num_docs_scanned == oblk.stats.num_docs_scanned
        assert blk.stats.num_entries_scanned_post_filter == oblk.stats.num_entries_scanned_post_filter
        for ra, rb in zip(blk.rows, oblk.rows):
            assert all(_same(x, y) for x, y in zip(ra, rb)), (ra, rb)
    finally:
        op.close()


@pytest.mark.parametrize("mode", ["dense", "fused", "hash"])
def test_gpu_long_waves_num_groups_limit(mode, segs, monkeypatch):
    """numGroupsLimit reached in the bulk segments: the limit pass re-walks the tiles on the plan's grids (after a
    fused group-by the plain filter first writes the masks) and keeps each segment's first-seen keys."""
    env = {"dense": {"PHIP_FUSED_GB": "0"}, "fused": {"PHIP_FUSED_GB": "2"}, "hash": {"PHIP_GB_HASH": "1"}}[mode]
    _run(f"SELECT hk, COUNT(*), SUM(m), SUM(d) FROM t WHERE {DENSE} GROUP BY hk LIMIT 10000000", segs, monkeypatch, env,
         limit=3000)
    assert _oracle(f"SELECT hk, COUNT(*), SUM(m), SUM(d) FROM t WHERE {DENSE} GROUP BY hk LIMIT 10000000", segs[0],
                   3000)[1].num_groups_limit_reached


@pytest.mark.parametrize("kind", ["fused", "unfused", "group_by", "fused_group_by"])
def test_gpu_long_waves_reexecution(kind, segs, monkeypatch):
    """One prepared plan three times under the cap (tickets, tables, rings and per-segment counts reset), then a new
    plan with the cap unset: the same oracle answer every time."""
    sql, env = {
        "fused": (f"SELECT SUM(m), SUM(d) FROM t WHERE {DENSE}", {"PHIP_FUSE": "1"}),
        "unfused": (f"SELECT SUM(m), SUM(d), COUNT(*) FROM t WHERE {DENSE}", {"PHIP_FUSE": "0"}),
        "group_by": (GB.format(w=DENSE), {"PHIP_FUSED_GB": "0"}),
        "fused_group_by": (GB.format(w=DENSE), {"PHIP_FUSED_GB": "3"}),
    }[kind]
    _run(sql, segs, monkeypatch, env, executions=3)
    _run(sql, segs, monkeypatch, env, cap=None)
