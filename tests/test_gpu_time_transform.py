"""Time transforms on the GPU (transform.hip; query/time_transform.py): GROUP BY keys and filter predicates over
dateTrunc, toEpochDays and the ISO-chronology fields of a dictionary column, against the oracle over STORED columns.

The oracle cannot evaluate a transform, so every segment carries, beside `ts`, columns precomputed with
numpy.datetime64 arithmetic (tests/time_transform_ref.py: independent of both implementations under test), stored raw:
a predicate over a raw column always scans, as the reference's ExpressionFilterOperator does. A query over
`dateTrunc('day', ts)` on the GPU must equal the oracle's over `ts_day`: keys, counts and exact sums bit for bit,
DOUBLE sums within 1e-9 relative, key types LONG / INT. The oracle keeps no filter statistics, so
numEntriesScannedInFilter is held against the reference's rule where the shape fixes it -- one entry per doc a scan
leaf evaluates: every doc, for a lone leaf and under a NOT, whatever index the column has and even when no entry or
every entry passes -- and there also against the same query over the stored raw column on the GPU, the same predicate
forced to a scan. Under AND / OR the library counts per leaf and tile as it does for any scan leaf (a conjunction of
dictionary leaves counts every doc per leaf, the general walk skips a leaf on tiles an earlier one decided); the test
restates that rule over numpy masks of the oracle's predicates (_expected_entries) and asserts the exact figure.

Three segments of about 5000 docs (more than two 2048-doc tiles, a ragged last one) whose `ts` dictionaries hold about
3000 entries (more than one 2048-entry dictionary tile), 40 entries (the column sorted) and a single entry: three id
widths, no identity remap. The values span negative epochs, leap days, and ISO-week year boundaries."""
import ctypes

import numpy as np
import pytest

from oracle import executor
from pinot_amd import _lib
from pinot_amd.engine import plan as planmod
from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker, UnsupportedOnGpu, compile_filter
from pinot_amd.engine.reduce import reduce_blocks, trim_groups
from pinot_amd.engine.segment import GpuSegment
from pinot_amd.query import time_transform as tt
from pinot_amd.query.context import columns_of
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType
from tests import fixtures
from tests import time_transform_ref as ref
from tests.test_gpu_parity import _assert_intermediates_equal

pytestmark = pytest.mark.gpu
DAY = ref.MS_PER_DAY

# name -> (the transform on the GPU, the oracle's stored column, its type)
KEYS = {u: (f"dateTrunc('{u}', ts)", f"ts_{u}", DataType.LONG) for u in ref.TRUNC_UNITS}
KEYS.update({
    "hod": ("hour(ts)", "ts_hod", DataType.INT), "dow": ("dayOfWeek(ts)", "ts_dow", DataType.INT),
    "yearf": ("year(ts)", "ts_yearf", DataType.INT), "monthf": ("month(ts)", "ts_monthf", DataType.INT),
    "weekf": ("week(ts)", "ts_weekf", DataType.INT), "edays": ("toEpochDays(ts)", "ts_edays", DataType.LONG),
    "secday": ("dateTrunc('day', sec, 'SECONDS')", "sec_day", DataType.LONG),
})


def _stored(ms):
    out = {f"ts_{u}": ref.trunc(ms, u) for u in ref.TRUNC_UNITS}
    out.update({"ts_hod": ref.field(ms, "hour"), "ts_dow": ref.field(ms, "dayofweek"), "ts_yearf": ref.field(ms, "year"),
                "ts_monthf": ref.field(ms, "month"), "ts_weekf": ref.field(ms, "week"),
                "ts_edays": ref.convert(ms, "MILLISECONDS", "DAYS")})
    return out


def _pool(rng, n):
    """n distinct millisecond values clustered on ~110 days: the calendar's edges and random days of 1960 .. 2025."""
    days = [ref.ms_of(d) // DAY for d in ("1969-12-31", "1970-01-01", "1972-02-29", "1972-03-01", "2000-02-29",
                                          "2018-12-31", "2019-01-01", "2020-12-31", "2021-01-03", "2021-01-04")]
    days += rng.integers(-3650, 20200, 100).tolist()
    vals = set()
    while len(vals) < n:
        d = days[int(rng.integers(0, len(days)))]
        vals.add(int(d) * DAY + int(rng.integers(0, DAY)))
    vals = sorted(vals)
    vals[0] = -1  # (one millisecond before the epoch)
    return np.asarray(vals, dtype=np.int64)


def _build(k, n, ts):
    rng = np.random.default_rng(900 + k)
    stored = _stored(ts)
    sec = np.floor_divide(ts, 1000)
    raw_cols = list(stored) + ["sec_day"]
    c = SegmentCreator(f"tt{k}", no_dictionary_columns=raw_cols)
    c.add_column("ts", DataType.LONG, ts)
    c.add_column("sec", DataType.INT, sec.astype(np.int32))
    for name, v in stored.items():
        typ = next(t for _, col, t in KEYS.values() if col == name)
        c.add_column(name, typ, v.astype(np.int32) if typ == DataType.INT else v)
    c.add_column("sec_day", DataType.LONG, ref.date_trunc(sec, "day", "SECONDS"))
    c.add_column("m", DataType.LONG, rng.integers(-1000, 100000, n))
    c.add_column("d", DataType.DOUBLE, rng.integers(1, 10 ** 6, n) / 64.0)  # positive terms: 1e-9 bounds the rounding
    c.add_column("g", DataType.INT, rng.integers(0, 4, n) + k)
    c.add_column("f", DataType.INT, rng.integers(0, 100, n))
    return c.build()


@pytest.fixture(scope="module")
def segs(gpu_lib):
    rng = np.random.default_rng(77)
    big = _pool(rng, 3000)
    small = _pool(rng, 40)
    ts0 = np.concatenate([big, rng.choice(big, 2001)])  # every entry occurs
    rng.shuffle(ts0)
    ts1 = np.sort(np.concatenate([small, rng.choice(small, 4963)]))  # sorted on ts
    ts2 = np.full(4999, ref.ms_of("2000-02-29") + 12345678, dtype=np.int64)
    raws = [_build(0, len(ts0), ts0), _build(1, len(ts1), ts1), _build(2, len(ts2), ts2)]
    cards = [r.columns["ts"].metadata.cardinality for r in raws]
    assert cards == [3000, 40, 1] and raws[1].columns["ts"].metadata.is_sorted
    gs = [GpuSegment(r) for r in raws]
    yield raws, gs
    for g in gs:
        g.destroy()


def _both(template):
    """The query over the transforms and the oracle's over the stored columns: `{day}` names a key of KEYS."""
    return (parse(template.format(**{k: v[0] for k, v in KEYS.items()})),
            parse(template.format(**{k: v[1] for k, v in KEYS.items()})))


_ORACLE = {}


def _oracle(template, oq, raws, **kw):
    key = (template, tuple(sorted(kw.items())), tuple(sorted(oq.options.items())))
    if key not in _ORACLE:  # computed once, shared, never changed
        _ORACLE[key] = executor.execute(oq, raws, **kw)
    return _ORACLE[key]


def _group_by(template, mat, options=None, **kw):
    raws, gs = mat
    gq, oq = _both(template)
    for q in (gq, oq):
        q.options.update(options or {})
    op = GpuInstancePlanMaker(**kw).make_instance_plan(gq, gs)
    try:
        gblk = op.next_block()
    finally:
        op.close()
    oblk, exact = _oracle(template, oq, raws, **kw)
    if getattr(gblk, "num_groups_trimmed", False):
        oblk = trim_groups(oq, oblk)
    assert (gblk.filter_kernel_ms or 0) + (gblk.agg_kernel_ms or 0) > 0, "no kernel time: did not run on the GPU"
    assert gblk.stats.num_docs_scanned == oblk.stats.num_docs_scanned
    # (the projection reads a column once however many transforms read it: year(ts), month(ts) project `ts`)
    read = {c for e in gq.group_by for c in columns_of(e)} | \
        {c for a in gq.aggregations if a.argument is not None for c in columns_of(a.argument)}
    filtered = any(a.filter is not None for a in gq.aggregations)  # (FILTER clauses: each info's own projection)
    if not filtered:
        assert gblk.stats.num_entries_scanned_post_filter == gblk.stats.num_docs_scanned * len(read)
    if filtered or len(read) == len({c for e in oq.group_by for c in columns_of(e)}) + len(read - {"ts", "sec"}):
        assert gblk.stats.num_entries_scanned_post_filter == oblk.stats.num_entries_scanned_post_filter
    assert gblk.num_groups_limit_reached == oblk.num_groups_limit_reached
    assert set(gblk.groups) == set(oblk.groups)
    for k, v in oblk.groups.items():
        _assert_intermediates_equal(gq.aggregations, gblk.groups[k], v, exact[k])
    assert [str(e) for e in gblk.group_by] == [str(e) for e in gq.group_by]  # the expression is the key's name
    assert list(gblk.key_types) == list(oblk.key_types)
    assert all(t in ("LONG", "INT") or str(e) == "g" for t, e in zip(gblk.key_types, gq.group_by))
    got, want = reduce_blocks(gq, [gblk]).rows, reduce_blocks(oq, [oblk]).rows
    if not gq.order_by:
        got, want = sorted(got), sorted(want)
    assert fixtures.rows_match(got, want)
    return gblk, oblk


AGGS = "SUM(m), SUM(d), COUNT(*), MAX(m)"
SINGLE_KEYS = list(ref.TRUNC_UNITS) + ["hod", "dow", "yearf", "weekf", "edays", "secday"]


@pytest.mark.parametrize("flt", ["", " WHERE f < 37"], ids=["all", "filtered"])
@pytest.mark.parametrize("key", SINGLE_KEYS)
def test_group_by_one_transformed_key(key, flt, segs):
    gblk, _ = _group_by(f"SELECT {{{key}}}, {AGGS} FROM t{flt} GROUP BY {{{key}}} LIMIT 100000", segs)
    assert len(gblk.groups) > 1


MIXED = [
    "SELECT g, {day}, {AGGS} FROM t GROUP BY g, {day} LIMIT 100000",
    "SELECT {yearf}, {monthf}, {AGGS} FROM t WHERE f >= 20 GROUP BY {yearf}, {monthf} LIMIT 100000",
    "SELECT {month}, ts, COUNT(*) FROM t WHERE f < 50 GROUP BY {month}, ts LIMIT 100000",  # with the column itself
    "SELECT {week}, g, {dow}, SUM(m) FROM t WHERE {hod} < 12 GROUP BY {week}, g, {dow} LIMIT 100000",
]


@pytest.mark.parametrize("tuple_keys", ["0", "1"], ids=["radix", "tuple"])
@pytest.mark.parametrize("template", MIXED)
def test_group_by_mixed_keys(template, tuple_keys, segs, monkeypatch):
    if tuple_keys == "1":
        monkeypatch.setenv("PHIP_TUPLE_KEYS", "1")
    _group_by(template.replace("{AGGS}", AGGS), segs)


@pytest.mark.parametrize("template", [
    "SELECT {day}, SUM(m), COUNT(*) FROM t GROUP BY {day} ORDER BY {day} LIMIT 4",
    "SELECT {day}, SUM(m), COUNT(*) FROM t WHERE f < 80 GROUP BY {day} ORDER BY {day} DESC LIMIT 3",
    "SELECT {yearf}, {monthf}, MAX(m) FROM t GROUP BY {yearf}, {monthf} ORDER BY {yearf} DESC, {monthf} LIMIT 5",
    "SELECT {week}, SUM(m) FROM t GROUP BY {week} ORDER BY SUM(m) DESC, {week} LIMIT 4",
])
def test_order_by_transformed_key_trims_on_the_device(template, segs):
    gblk, _ = _group_by(template, segs, options={"minServerGroupTrimSize": "3"})
    assert gblk.num_groups_trimmed


@pytest.mark.parametrize("limit", [1, 17])
def test_num_groups_limit_below_the_group_count(limit, segs):
    """Per segment the first `limit` keys in doc order."""
    gblk, oblk = _group_by("SELECT {day}, COUNT(*), SUM(m) FROM t GROUP BY {day} LIMIT 100000", segs,
                           num_groups_limit=limit)
    assert oblk.num_groups_limit_reached


def test_filter_clause_beside_a_transformed_key(segs):
    _group_by("SELECT {month}, SUM(m) FILTER(WHERE f < 50), COUNT(*) FILTER(WHERE {dow} >= 6), COUNT(*) FROM t "
              "GROUP BY {month} LIMIT 100000", segs)


# ---- filters --------------------------------------------------------------------------------------------------------
D0 = ref.ms_of("2000-02-29")
FILTERS = [
    f"{{day}} = {D0}", f"{{day}} <> {D0}", f"{{day}} < {D0}", f"{{day}} >= {D0}",
    f"{{day}} BETWEEN {ref.ms_of('1972-02-29')} AND {ref.ms_of('2019-01-01')}",
    f"{{month}} IN ({ref.ms_of('2000-02-01')}, {ref.ms_of('1969-12-01')}, 5)", f"{{year}} NOT IN ({ref.ms_of('2000-01-01')}, 7)",
    "{edays} = 11016", "{edays} <> -1", "{edays} < 0", "{edays} >= 17896", "{edays} BETWEEN -1 AND 11016",
    "{edays} IN (-1, 0, 11016, 18627)", "{edays} NOT IN (11016)",
    "{hod} = 3", "{hod} <> 0", "{hod} < 6", "{hod} >= 18", "{hod} BETWEEN 9 AND 17", "{hod} IN (0, 23, 25)", "{hod} NOT IN (3, 4)",
    "{dow} = 1", "{dow} <> 7", "{dow} < 3", "{dow} >= 6", "{dow} BETWEEN 2 AND 4", "{dow} IN (1, 4, 7)", "{dow} NOT IN (2)",
    "{secday} >= 951782400 AND f < 50", "{dow} = 2 OR f = 3", "NOT {hod} < 12", "f > 10 AND NOT ({edays} < 0 OR {dow} IN (6, 7))",
    "{yearf} = 1 AND {hod} = 2",  # nothing: the leaves still scan
]


# a lone leaf and a NOT's child scan every doc
LONE = set(FILTERS[:28]) | {"NOT {hod} < 12"}
TILE = 2048  # device.h kTileDocs


def _conjunction_walk(tree, g):
    """Whether the library takes its conjunction walk for this segment's compiled program (runtime.cpp
    configure_filter_paths): only ANDs over scan leaves that are id ranges or sets over a dictionary of at most 64
    entries. An always-scan leaf that no or every entry passes is a constant id set: a bitmap above 64 entries, which
    sends the program to the general walk. (A set of scattered ids over a larger dictionary is not modelled here: no
    AND case has one.)"""
    if isinstance(tree, planmod._Leaf):  # (a lone leaf counts every doc on either walk)
        return True
    if tree.op != _lib.NODE_AND:
        return False
    for leaf in tree.children:
        if not isinstance(leaf, planmod._Leaf) or leaf.kind not in (_lib.LEAF_DICT_RANGE, _lib.LEAF_DICT_SET):
            return False
        card = g.column_metadata(leaf.column).cardinality
        ids = np.arange(leaf.lo, leaf.hi) if leaf.kind == _lib.LEAF_DICT_RANGE else np.asarray(leaf.ids)
        if card <= 64:
            continue
        if len(ids) in (0, card):
            return False
        assert len(ids) == int(ids[-1]) - int(ids[0]) + 1 and not leaf.exclusive, "a shape this model does not cover"
    return True


def _expected_entries(gfc, ofc, raws, gs):
    """numEntriesScannedInFilter by the library's documented rule, from numpy masks of the oracle's predicates over
    the stored columns. Conjunction walk: every leaf counts every doc of the segment. General walk, per 2048-doc
    tile: a leaf counts the tile's docs unless it is skipped -- the second and later children of an AND are skipped
    on a tile where no doc passed so far, those of an OR where every doc passed. An AND's children are evaluated
    leaves first, in the query's order (plan.compile_filter)."""
    total = 0
    for raw, g in zip(raws, gs):
        tree = compile_filter(g, gfc)
        n = g.num_docs
        if _conjunction_walk(tree, g):
            total += n * (1 if isinstance(tree, planmod._Leaf) else len(tree.children))
            continue
        os_ = executor.OracleSegment(raw)
        masks = {}

        def walk(fc, a, b):
            if fc.type == "PREDICATE":
                if id(fc) not in masks:
                    masks[id(fc)] = np.asarray(executor.eval_filter(os_, fc), dtype=bool)
                return masks[id(fc)][a:b], b - a
            if fc.type == "NOT":
                m, c = walk(fc.children[0], a, b)
                return ~m, c
            kids = list(fc.children)
            if fc.type == "AND":
                kids.sort(key=lambda k: 3 if k.type == "PREDICATE" else (4 if k.type == "AND" else 5))
            acc, c = walk(kids[0], a, b)
            for k in kids[1:]:
                if (not acc.any()) if fc.type == "AND" else acc.all():
                    continue
                m, ck = walk(k, a, b)
                acc = (acc & m) if fc.type == "AND" else (acc | m)
                c += ck
            return acc, c

        for a in range(0, n, TILE):
            total += walk(ofc, a, min(a + TILE, n))[1]
    return total


def _run(q, gs):
    op = GpuInstancePlanMaker().make_instance_plan(q, gs)
    try:
        return op.next_block()
    finally:
        op.close()


@pytest.mark.parametrize("path", ["0", "1000000000"], ids=["device", "host"])
@pytest.mark.parametrize("where", FILTERS)
def test_filters(where, path, segs, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_TRANSFORM_HOST_CARD", path)
    raws, gs = segs
    for g in gs:  # (an id set kept by the other path's run must not answer this one)
        g._transform_matches.clear()
    for template in (f"SELECT COUNT(*), SUM(m), SUM(d) FROM t WHERE {where}",
                     f"SELECT COUNT(*) FILTER(WHERE {where}), SUM(m) FILTER(WHERE {where}), COUNT(*) FROM t"):
        gq, oq = _both(template)
        gblk = _run(gq, gs)
        oblk, exact = _oracle(template, oq, raws)
        assert gblk.stats.num_docs_scanned == oblk.stats.num_docs_scanned, template
        _assert_intermediates_equal(gq.aggregations, gblk.results, oblk.results, exact)
        n = sum(g.num_docs for g in gs)
        scanned = gblk.stats.num_entries_scanned_in_filter
        print(f"numEntriesScannedInFilter {scanned} of {n} docs: {template}")
        clause = "FILTER(" in template
        want = _expected_entries(gq.aggregations[0].filter if clause else gq.filter,
                                 oq.aggregations[0].filter if clause else oq.filter, raws, gs)
        assert scanned == want, (template, scanned, want)
        if where in LONE:
            assert want == n
            twin = _run(oq, gs)  # the stored raw column's leaf: the same predicate as a scan
            assert scanned == twin.stats.num_entries_scanned_in_filter, template
    builds = [g.transform_match_builds for g in gs]
    assert sum(builds) > 0
    op = GpuInstancePlanMaker().make_instance_plan(_both(f"SELECT COUNT(*) FROM t WHERE {where}")[0], gs)
    op.close()
    assert [g.transform_match_builds for g in gs] == builds  # a second plan finds every id set kept


@pytest.mark.parametrize("path", ["0", "1000000000"], ids=["device", "host"])
def test_monotone_range_is_a_dict_range_leaf_that_always_scans(path, segs, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_TRANSFORM_HOST_CARD", path)
    raws, gs = segs
    for g in gs:
        g._transform_matches.clear()
    for where in (f"{{day}} BETWEEN {ref.ms_of('1972-02-29')} AND {ref.ms_of('2019-01-01')}", "{edays} >= 0",
                  f"{{year}} < {ref.ms_of('2001-01-01')}", "{secday} > 0", f"{{day}} = {D0}"):
        gq, _ = _both(f"SELECT COUNT(*) FROM t WHERE {where}")
        for g in gs:  # (an id range whenever an entry passes; no entry: the empty set, which still scans)
            leaf = compile_filter(g, gq.filter)
            some = leaf.kind == _lib.LEAF_DICT_RANGE and leaf.hi > leaf.lo
            none = leaf.kind == _lib.LEAF_DICT_SET and len(leaf.ids) == 0
            assert leaf.pattern and (some or none), (where, g.name, leaf)
            assert some or g.name != "tt0"
    # never a constant, never an index leaf: a predicate no entry passes is an empty DICT_SET that scans
    gq, _ = _both("SELECT COUNT(*) FROM t WHERE {yearf} = 1")
    for g in gs:
        leaf = compile_filter(g, gq.filter)
        assert leaf.kind == _lib.LEAF_DICT_SET and leaf.pattern and len(leaf.ids) == 0


def test_device_match_equals_host_restatement(segs, monkeypatch):
    """phip_segment_match_transform over the 3000-entry dictionary (two tiles, a ragged one) against evaluate()."""
    raws, gs = segs
    vals = np.asarray(gs[0].dictionary("ts").values, dtype=np.int64)
    monkeypatch.setenv("PINOT_AMD_TRANSFORM_HOST_CARD", "0")
    for text in ["dateTrunc('%s', ts)" % u for u in ref.TRUNC_UNITS] + ["%s(ts)" % f for f in ref.FIELDS] + \
            ["toEpochHours(ts)", "dateTrunc('week', ts, 'MILLISECONDS', 'UTC', 'DAYS')"]:
        t = tt.compile_transform(parse(f"SELECT COUNT(*) FROM t GROUP BY {text}").group_by[0])
        want = tt.evaluate(t.program, vals)
        mid = int(np.sort(want)[len(want) // 2])
        for pred in (("range", mid, (1 << 63) - 1, ()), ("range", int(want.min()), mid, ()), ("range", 1, 0, ()),
                     ("set", 0, 0, tuple(sorted({int(x) for x in want[::7]}))), ("not_set", 0, 0, (mid,)), ("set", 0, 0, ())):
            gs[0]._transform_matches.clear()
            ids = gs[0].match_transform("ts", t.program, pred)
            hit = tt.match_values(want, pred[0], pred[1], pred[2], np.asarray(pred[3], dtype=np.int64))
            assert np.array_equal(ids, np.flatnonzero(hit).astype(np.int32)), (text, pred[:3])


@pytest.fixture(scope="module")
def wide_segment(gpu_lib):
    """20 000 distinct `ts` values: ten 2048-entry dictionary tiles, more than the eight workgroups PHIP_GRID_CUS=1
    leaves dict_transform_kernel, so its grid stride runs."""
    rng = np.random.default_rng(31)
    ts = rng.permutation(np.arange(20000, dtype=np.int64) * 7_654_321 - 40_000_000_000)
    c = SegmentCreator("tt_wide")
    c.add_column("ts", DataType.LONG, ts)
    c.add_column("m", DataType.LONG, rng.integers(0, 1000, len(ts)))
    raw = c.build()
    assert raw.columns["ts"].metadata.cardinality == 20000
    g = GpuSegment(raw)
    yield ts, g
    g.destroy()


def _range_mask(lib, seg, program, lower, upper, lower_inclusive, upper_inclusive):
    """phip_segment_match_transform with a range predicate as given: the entries' mask."""
    card = seg.column_metadata("ts").cardinality
    t = _lib.TimeTransform(*program)
    pr = _lib.TransformPredicate()
    pr.kind, pr.lower, pr.upper = _lib.TT_PRED_RANGE, lower, upper
    pr.lower_inclusive, pr.upper_inclusive = int(lower_inclusive), int(upper_inclusive)
    words = np.zeros((card + 63) // 64, dtype=np.uint64)
    _lib.check(lib.phip_segment_match_transform(seg.handle, b"ts", ctypes.byref(t), ctypes.byref(pr),
                                                words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(words)))
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:card].astype(bool)


@pytest.mark.parametrize("grid_cus", [None, "1"], ids=["grid", "strided"])
def test_exclusive_bounds_and_the_grid_stride(grid_cus, gpu_lib, wide_segment, monkeypatch):
    """Range bounds with every combination of the inclusive flags, on bounds that entries hold, over ten dictionary
    tiles -- once on the device's own grid, once on eight workgroups (the kernel's stride over the tiles) -- and a
    transformed key's remap built the same way, against evaluate() and numpy."""
    if grid_cus:
        monkeypatch.setenv("PHIP_GRID_CUS", grid_cus)
    ts, g = wide_segment
    vals = np.asarray(g.dictionary("ts").values, dtype=np.int64)
    for text in ("dateTrunc('day', ts)", "dayOfYear(ts)", "toEpochHours(ts)"):
        t = tt.compile_transform(parse(f"SELECT COUNT(*) FROM t GROUP BY {text}").group_by[0])
        want = tt.evaluate(t.program, vals)
        lo, hi = (int(x) for x in np.sort(want)[[len(want) // 3, 2 * len(want) // 3]])
        assert (want == lo).any() and (want == hi).any() and lo < hi
        for li in (0, 1):
            for ui in (0, 1):
                got = _range_mask(gpu_lib, g, t.program, lo, hi, li, ui)
                ref_mask = ((want >= lo) if li else (want > lo)) & ((want <= hi) if ui else (want < hi))
                assert np.array_equal(got, ref_mask), (text, li, ui)
        assert not _range_mask(gpu_lib, g, t.program, lo, lo, 0, 1).any()  # (lo, lo]: nothing
    unit = "hour" if grid_cus else "day"  # (a program per run: each builds its remap on this run's grid)
    q = parse(f"SELECT dateTrunc('{unit}', ts), COUNT(*) FROM t GROUP BY dateTrunc('{unit}', ts) LIMIT 100000")
    before = _info(gpu_lib)[0]
    blk = _run(q, [g])
    assert _info(gpu_lib)[0] == before + 1
    keys, counts = np.unique(ref.trunc(ts, unit), return_counts=True)
    assert {k[0]: v[0] for k, v in blk.groups.items()} == dict(zip(keys.tolist(), counts.tolist()))


# ---- caches, refusals, the C ABI ------------------------------------------------------------------------------------
def _info(lib):
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.phip_transform_info(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def test_a_second_plan_builds_no_new_remap(gpu_lib, segs):
    raws, gs = segs
    sql = "SELECT dateTrunc('quarter', ts, 'MILLISECONDS', 'UTC', 'MINUTES'), COUNT(*) FROM t " \
          "GROUP BY dateTrunc('quarter', ts, 'MILLISECONDS', 'UTC', 'MINUTES') LIMIT 100000"
    before = _info(gpu_lib)[0]
    blocks = []
    for _ in range(2):
        op = GpuInstancePlanMaker().make_instance_plan(parse(sql), gs)
        blocks.append(op.next_block())
        op.close()
        if len(blocks) == 1:
            assert _info(gpu_lib)[0] == before + 1
    assert _info(gpu_lib)[0] == before + 1
    assert blocks[0].groups.keys() == blocks[1].groups.keys()
    # another program over the same column and segments is another remap
    op = GpuInstancePlanMaker().make_instance_plan(parse(sql.replace("'MINUTES'", "'HOURS'")), gs)
    op.next_block()
    op.close()
    assert _info(gpu_lib)[0] == before + 2


@pytest.fixture(scope="module")
def odd_segment(gpu_lib):
    n = 100
    rng = np.random.default_rng(5)
    c = SegmentCreator("tt_odd", no_dictionary_columns=["rawts"])
    c.add_column("ts", DataType.LONG, rng.integers(0, 10 ** 12, n))
    c.add_column("rawts", DataType.LONG, rng.integers(0, 10 ** 12, n))
    c.add_column("dbl", DataType.DOUBLE, rng.random(n))
    c.add_column("flt", DataType.FLOAT, rng.random(n).astype(np.float32))
    c.add_column("str", DataType.STRING, np.array([f"v{i % 7}" for i in range(n)]))
    c.add_column("nl", DataType.LONG, rng.integers(0, 10 ** 12, n), nulls=rng.random(n) < 0.3)
    c.add_column("huge", DataType.LONG, rng.integers(1 << 50, 1 << 51, n))
    c.add_column("mv", DataType.INT, [rng.integers(0, 50, rng.integers(1, 4)) for _ in range(n)], multi_value=True)
    c.add_column("m", DataType.LONG, rng.integers(0, 100, n))
    g = GpuSegment(c.build())
    yield g
    g.destroy()


def _refused(sql, segments, reason, options=None, exc=UnsupportedOnGpu):
    q = parse(sql)
    q.options.update(options or {})
    with pytest.raises(exc, match=reason):
        op = GpuInstancePlanMaker().make_instance_plan(q, segments)
        try:
            op.next_block()
        finally:
            op.close()


def test_refusals(segs, odd_segment, monkeypatch):
    raws, gs = segs
    odd = [odd_segment]
    for use in ("SELECT COUNT(*) FROM t GROUP BY {}", "SELECT COUNT(*) FROM t WHERE {} > 5"):
        # section 2: the compiler's
        _refused(use.format("dateTrunc('day', ts, 'MILLISECONDS', 'Asia/Tokyo')"), gs, "time zone Asia/Tokyo")
        _refused(use.format("timeConvert(ts, 'MILLISECONDS', 'WEEKS')"), gs, "WEEKS output")
        _refused(use.format("year(ts + 1)"), gs, "nested expression")
        _refused(use.format("dateTrunc('eon', ts)"), gs, "unknown dateTrunc unit", exc=ValueError)
        _refused(use.format("toEpochDays(ts, ts)"), gs, "takes 1 argument", exc=ValueError)
        # ... and the column's
        _refused(use.format("year(rawts)"), odd, "raw \\(no-dictionary\\) column rawts")
        _refused(use.format("year(dbl)"), odd, "column dbl of type DOUBLE")
        _refused(use.format("year(flt)"), odd, "column flt of type FLOAT")
        _refused(use.format("year(str)"), odd, "column str of type STRING")
        _refused(use.format("year(mv)"), odd, "multi-value")
        _refused(use.format("timeConvert(huge, 'DAYS', 'NANOSECONDS')"), odd, "column huge")
        # sections 4 and 5: null handling over a column with a null vector
        _refused(use.format("year(nl)"), odd, "null vector", options={"enableNullHandling": "true"})
    # without null handling the null docs carry the default value, as everywhere else
    q = parse("SELECT year(nl), COUNT(*) FROM t WHERE month(nl) > 0 GROUP BY year(nl) LIMIT 1000")
    blk = GpuInstancePlanMaker().make_instance_plan(q, odd).next_block()
    assert sum(v[0] for v in blk.groups.values()) == odd_segment.num_docs
    # other group-by expressions keep their refusal
    _refused("SELECT COUNT(*) FROM t GROUP BY m*2", odd, "group-by expression")
    _refused("SELECT COUNT(*) FROM t GROUP BY year(ts), m + 1", odd, "group-by expression")
    # what stays refused: an aggregation argument, a selection list, SELECT DISTINCT, a selection ORDER BY
    _refused("SELECT SUM(year(ts)) FROM t", odd, "outside the GPU expression subset")
    _refused("SELECT year(ts) FROM t LIMIT 5", odd, "outside the GPU expression subset")
    _refused("SELECT DISTINCT year(ts) FROM t", odd, "SELECT DISTINCT over the expression")
    _refused("SELECT m FROM t ORDER BY year(ts) LIMIT 5", odd, "outside the GPU expression subset")
    # segments on several devices, and the library's node plan
    q = parse("SELECT COUNT(*) FROM t GROUP BY year(ts)")
    monkeypatch.setattr(gs[1], "device", gs[0].device + 1)
    with pytest.raises(UnsupportedOnGpu, match="several devices"):
        GpuCombineOperator(q, gs, 100000)
    monkeypatch.undo()
    monkeypatch.setenv("PHIP_NODE_SPLIT", "2")
    op = GpuCombineOperator(q, gs, 100000)
    with pytest.raises(_lib.PhipUnsupported, match="node plan"):
        op.run_raw()
    op.close()


def _match_rc(lib, seg, column, program, kind=_lib.TT_PRED_RANGE, values=None, nvalues=None, words=64, flags=(0, 1, 1)):
    t = _lib.TimeTransform(*program)
    pr = _lib.TransformPredicate()
    pr.kind, pr.lower, pr.upper = kind, 0, 10
    pr.exclusive, pr.lower_inclusive, pr.upper_inclusive = flags
    if values is not None:
        arr = np.asarray(values, dtype=np.int64)
        pr.values = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    pr.num_values = len(values) if nvalues is None and values is not None else (nvalues or 0)
    out = np.zeros(words, dtype=np.uint64)
    return lib.phip_segment_match_transform(seg.handle, column.encode(), ctypes.byref(t), ctypes.byref(pr),
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(out))


def test_malformed_descriptors_through_the_c_abi(gpu_lib, segs, odd_segment):
    """Every field is checked before any launch: PHIP_ERR_INVALID, never a kernel over a bad program."""
    lib = gpu_lib
    raws, gs = segs
    good = (tt.FUNC_TRUNC, 3, 1, 1, 1, 1)
    launches = _info(lib)[1]
    assert _match_rc(lib, gs[0], "ts", good) == _lib.PHIP_OK
    assert _info(lib)[1] == launches + 1
    bad_programs = [(0, 0, 1, 1, 1, 1), (4, 0, 1, 1, 1, 1), (-1, 0, 1, 1, 1, 1), (tt.FUNC_TRUNC, 8, 1, 1, 1, 1),
                    (tt.FUNC_TRUNC, -1, 1, 1, 1, 1), (tt.FUNC_FIELD, 11, 1, 1, 1, 1), (tt.FUNC_FIELD, 0, 1000, 1, 1, 1),
                    (tt.FUNC_CONVERT, 1, 1, 1, 1, 1), (tt.FUNC_CONVERT, 0, 1, 1, 1, 60), (tt.FUNC_TRUNC, 3, 0, 1, 1, 1),
                    (tt.FUNC_TRUNC, 3, 1, -5, 1, 1), (tt.FUNC_TRUNC, 3, 1000, 1000, 1, 1), (tt.FUNC_TRUNC, 3, 1, 1, 60, 60)]
    for p in bad_programs:
        assert _match_rc(lib, gs[0], "ts", p) == _lib.PHIP_ERR_INVALID, p
    assert _match_rc(lib, gs[0], "ts", good, kind=0) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, kind=3) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, flags=(2, 1, 1)) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, flags=(0, 1, 7)) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, kind=_lib.TT_PRED_SET, values=[3, 3]) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, kind=_lib.TT_PRED_SET, values=[5, 1]) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, kind=_lib.TT_PRED_SET, nvalues=4) == _lib.PHIP_ERR_INVALID  # null values
    assert _match_rc(lib, gs[0], "ts", good, kind=_lib.TT_PRED_SET, nvalues=-1) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "ts", good, words=46) == _lib.PHIP_ERR_INVALID  # 3000 entries need 47 words
    assert _match_rc(lib, gs[0], "ts_day", good) == _lib.PHIP_ERR_INVALID  # a raw column
    assert _match_rc(lib, odd_segment, "dbl", good) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, odd_segment, "str", good) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, odd_segment, "mv", good) == _lib.PHIP_ERR_INVALID
    assert _match_rc(lib, gs[0], "nope", good) == _lib.PHIP_ERR_NOT_FOUND
    assert _match_rc(lib, odd_segment, "huge", (tt.FUNC_CONVERT, 0, 10 ** 9, 1, 1, 1)) == _lib.PHIP_ERR_UNSUPPORTED
    assert _info(lib)[1] == launches + 1  # none of them launched
    # a group-by descriptor: a malformed program, a shared entry of columns[], a derived index
    op = GpuCombineOperator(parse("SELECT COUNT(*) FROM t GROUP BY dateTrunc('day', ts), g"), gs, 100000)
    for tamper in ("unit", "function", "scale", "shared", "derived"):
        keep = []
        q = op._desc(keep)
        if tamper == "unit":
            q.group_by_transforms[0].unit = 99
        elif tamper == "function":
            q.group_by_transforms[0].function = 9
        elif tamper == "scale":
            q.group_by_transforms[0].in_div = 0
        elif tamper == "shared":
            q.group_by_columns[1] = q.group_by_columns[0]
        else:  # an index at or past the query's own columns: where a derived value column would stand
            q.group_by_columns[0] = q.num_columns
        h = ctypes.c_uint64(0)
        assert lib.phip_plan_create(ctypes.byref(q), ctypes.byref(h)) == _lib.PHIP_ERR_INVALID, tamper
    keep = []
    q = op._desc(keep)
    h = ctypes.c_uint64(0)
    assert lib.phip_plan_create(ctypes.byref(q), ctypes.byref(h)) == _lib.PHIP_OK
    _lib.check(lib.phip_plan_destroy(h.value))
    op.close()
