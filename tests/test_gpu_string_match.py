"""LIKE / REGEXP_LIKE on the GPU (strmatch.hip): the dictionary match, the raw pre-pass, their composition with the
other leaves, the statistics and the library-level checks. Every expectation comes from tests/strmatch_ref.py (Python's
re) over the generated values on the host, never from the code under test."""
import ctypes
import json
import os

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker, PatternTypeError
from pinot_amd.engine.segment import GpuSegment
from pinot_amd.query import regex_dfa
from pinot_amd.query.sql import parse
from pinot_amd.segment.creator import SegmentCreator
from pinot_amd.spi import DataType
from tests import strmatch_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "regexp_like_queries.json")) as _f:
    QUERIES = json.load(_f)
WINDOW = 2048  # device.h kStrMatchWindow
E, EMOJI = "\u00e9", "\U0001F600"
# prefix, substring, suffix-$, alternation, class, (?i), match-nothing, match-everything
PATTERNS = ["^www", "main1", "\\.com$", "ab|cd|" + E, "[0-9]{2}", "(?i)DOMAIN", "zzzzqq", ""]


def _words(mask):
    n = len(mask)
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = mask
    return np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def _mask(pattern, values):
    return np.asarray(strmatch_ref.match_many(pattern, values), dtype=bool)


def _count(segs, where, opts=""):
    qc = parse(f"{opts}SELECT COUNT(*) FROM t WHERE {where}")
    blk = GpuInstancePlanMaker().make_instance_plan(qc, segs).next_block()
    return int(blk.results[0]), blk.stats


def _golden_rows():
    n = QUERIES["num_rows"]
    dn, us, ni = QUERIES["domain_names"], QUERIES["url_suffixes"], QUERIES["no_index_values"]
    dom = [dn[i % len(dn)] for i in range(n)]
    return {"INT_COL": np.arange(n) + QUERIES["int_base"], "DOMAIN_NAMES": dom,
            "URL_COL": [dom[i] + us[i % len(us)] for i in range(n)], "NO_INDEX_COL": [ni[i % len(ni)] for i in range(n)]}


def _golden_segment(name, inverted=(), raw=(), sort=False):
    rows = _golden_rows()
    order = np.argsort(np.asarray(rows["DOMAIN_NAMES"]), kind="stable") if sort else np.arange(QUERIES["num_rows"])
    c = SegmentCreator(name, inverted_index_columns=list(inverted), no_dictionary_columns=list(raw))
    c.add_column("INT_COL", DataType.INT, rows["INT_COL"][order])
    for col in ("DOMAIN_NAMES", "URL_COL", "NO_INDEX_COL"):
        c.add_column(col, DataType.STRING, np.asarray(rows[col])[order])
    return c.build()


# ---- 1. the reference's own queries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dict", "dict_inverted", "dict_sorted", "raw"])
@pytest.mark.parametrize("host_card", ["0", "1000000000"], ids=["device", "host"])
def test_golden_queries(gpu_lib, monkeypatch, layout, host_card):
    monkeypatch.setenv("PINOT_AMD_STRMATCH_HOST_CARD", host_card)
    cols = ("DOMAIN_NAMES", "URL_COL", "NO_INDEX_COL")
    raw = _golden_segment(f"g_{layout}_{host_card}", inverted=cols if layout == "dict_inverted" else (),
                          raw=cols if layout == "raw" else (), sort=layout == "dict_sorted")
    if layout == "dict_sorted":
        assert raw.columns["DOMAIN_NAMES"].metadata.is_sorted
    seg = GpuSegment(raw)
    try:
        for where, count in QUERIES["counts"]:
            got, stats = _count([seg], where)
            assert got == count, (layout, where)
        sel = QUERIES["selection"]
        qc = parse(f"SELECT INT_COL, URL_COL FROM t WHERE {sel['filter']} LIMIT {sel['limit']}")
        blk = GpuInstancePlanMaker().make_instance_plan(qc, [seg]).next_block()
        got = [[int(r[0]), str(r[1])] for r in blk.rows]
        if layout == "dict_sorted":  # (the rows were reordered: the first matches in that order)
            rows = _golden_rows()
            order = np.argsort(np.asarray(rows["DOMAIN_NAMES"]), kind="stable")
            urls = np.asarray(rows["URL_COL"])[order]
            hit = np.flatnonzero(_mask("www.domain1.*", urls))[:sel["limit"]]
            assert got == [[int(rows["INT_COL"][order][i]), str(urls[i])] for i in hit]
        else:
            assert got == sel["rows"], layout
    finally:
        seg.destroy()


# ---- 2. the dictionary match ----------------------------------------------------------------------------------------
def _dict_values(card, width, rng):
    """`card` distinct values of at most `width` bytes: the empty string (entry 0), values that fill the width exactly
    (no pad byte), multi-byte characters, and text the patterns find."""
    frag = ["www.", "domain1", "main1", ".com", "ab", "cd", "12", "7", "x", "DOMAIN", "dOmAiN", E, EMOJI, "z", "q", "-"]
    vals = {""}
    if width >= 4:
        vals.add((EMOJI * (width // 4) + "a" * (width % 4)))            # fills the width, multi-byte
    vals.add("w" * width)                                                 # fills the width
    tries = 0
    while len(vals) < card and tries < 200 * card:
        tries += 1
        if width == 1:
            v = chr(rng.integers(1, 128))
            if v in strmatch_ref.JAVA_ONLY_TERMINATORS:
                continue
        else:
            v = "".join(frag[i] for i in rng.integers(0, len(frag), rng.integers(1, 6)))
            if rng.random() < 0.5:
                v += str(rng.integers(0, 100000))
            while len(v.encode("utf-8")) > width:
                v = v[:-1]
        vals.add(v)
    return sorted(vals)[:card] if len(vals) >= card else None


@pytest.mark.parametrize("width", [1, 7, 300])
@pytest.mark.parametrize("card", [1, 63, 64, 65, 5000])
def test_dictionary_match(gpu_lib, monkeypatch, card, width):
    rng = np.random.default_rng(card * 1000 + width)
    vals = _dict_values(card, width, rng)
    if vals is None:  # (fewer than `card` distinct values of that width exist: 127 one-byte values)
        assert width == 1 and card > 100
        vals = _dict_values(100, width, rng)
    docs = np.asarray(vals)[np.concatenate([np.arange(len(vals)), rng.integers(0, len(vals), 200)])]
    raw = SegmentCreator(f"d{card}_{width}").add_column("s", DataType.STRING, docs) \
        .add_column("k", DataType.INT, np.arange(len(docs))).build()
    m = raw.columns["s"].metadata
    assert m.cardinality == len(vals) and (m.string_width == width or len(vals) < 3)
    seg = GpuSegment(raw)
    try:
        for pattern in PATTERNS:
            want = np.flatnonzero(_mask(pattern, vals)).astype(np.int32)
            dfa = regex_dfa.compile_pattern(pattern)
            got = {}
            for how, hc in (("device", "0"), ("host", "1000000000")):
                monkeypatch.setenv("PINOT_AMD_STRMATCH_HOST_CARD", hc)
                seg._matches.clear()
                got[how] = seg.match_dictionary("s", pattern, dfa)
            assert np.array_equal(got["device"], want), (pattern, card, width)
            assert np.array_equal(got["host"], want), (pattern, card, width)
    finally:
        seg.destroy()


# ---- 3. the raw pre-pass --------------------------------------------------------------------------------------------
def _raw_values(n, rng, seed_text):
    frag = ["www.", "domain1", "main1", ".com", "ab", "cd", "12", "7", "x", "DOMAIN", "dOmAiN", E, EMOJI, "z", "q", "-", "/"]
    vals = []
    for _ in range(n):
        v = "".join(frag[i] for i in rng.integers(0, len(frag), rng.integers(0, 8)))
        while len(v.encode("utf-8")) > 40:
            v = v[:-1]
        vals.append(v)
    vals[0] = ""
    for d in range(128, 192):                       # a 64-doc group made entirely of empty strings
        vals[d] = ""
    vals[300] = "x" * (3 * WINDOW) + "7"            # 3 windows + 1 bytes, '[0-9]{2}' aside its only match is the last byte
    vals[301] = "main1"
    # a 4-byte character straddling a window boundary: group 7 (docs 448..511) starts at a 16-byte-aligned window
    # start only by chance, so put the character across every alignment once
    for k in range(4):
        vals[448 + 2 * k] = "y" * (WINDOW - 2 - k) + EMOJI + "ab"
    vals[700] = "www.domain1.com\n"                 # a value ending in a line feed
    vals[701] = seed_text
    return vals


@pytest.fixture(scope="module")
def raw_segments(gpu_lib):
    rng = np.random.default_rng(77)
    out = []
    for k, n in enumerate((5000, 2049)):
        vals = _raw_values(n, rng, f"seg{k}.com")
        other = ["".join(rng.choice(list("abcd" + E), rng.integers(0, 6))) for _ in range(n)]
        raw = SegmentCreator(f"rawm{k}", no_dictionary_columns=["s", "u"]) \
            .add_column("s", DataType.STRING, np.asarray(vals, dtype=object).astype(np.str_)) \
            .add_column("u", DataType.STRING, np.asarray(other, dtype=object).astype(np.str_)) \
            .add_column("k", DataType.INT, np.arange(n) % 97).build()
        out.append((vals, other, raw, GpuSegment(raw)))
    yield out
    for _, _, _, g in out:
        g.destroy()


def test_raw_prepass_doc_sets(raw_segments, monkeypatch):
    monkeypatch.setenv("PHIP_GRID_CUS", "1")  # 8 workgroups: each walks several tiles, and both segments' tasks
    segs = [g for _, _, _, g in raw_segments]
    for pattern in PATTERNS + ["7$"]:
        for neg in (False, True):
            where = ("NOT " if neg else "") + "REGEXP_LIKE(s, '" + pattern.replace("'", "''") + "')"
            qc = parse(f"SELECT COUNT(*) FROM t WHERE {where}")
            total = 0
            for vals, _, _, g in raw_segments:
                want = _mask(pattern, vals) != neg
                got = GpuCombineOperator(qc, [g], 100000).filter_bitmap()
                assert np.array_equal(got, _words(want)), (where, g.name, np.nonzero(got != _words(want))[0][:5])
                total += int(want.sum())
            got, stats = _count(segs, where)   # one plan over both segments: two tasks in one launch
            assert got == total, where
    vals = raw_segments[0][0]
    assert _mask("7$", vals)[300] and not _mask("7$", [vals[300][:-1]])[0]   # (matches only at its last byte)


# ---- 4. composition -------------------------------------------------------------------------------------------------
def test_composition(gpu_lib, raw_segments, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_STRMATCH_HOST_CARD", "0")
    rng = np.random.default_rng(5)
    n = 6000
    sv = np.asarray([["www.domain%d.com" % (i % 7), "ab%d" % (i % 50), "x" + E, ""][i % 4] for i in rng.integers(0, 1000, n)])
    b = rng.integers(0, 200, n)
    nulls = rng.random(n) < 0.1
    nv = np.where(nulls, None, sv)
    mv = [[sv[i], sv[(i * 7 + 1) % n]][: 1 + i % 2] for i in range(n)]
    raw = SegmentCreator("comp", inverted_index_columns=["a"]).add_column("a", DataType.STRING, sv) \
        .add_column("b", DataType.INT, b).add_column("c", DataType.STRING, nv, nulls=nulls) \
        .add_column("m", DataType.STRING, mv, multi_value=True).build()
    seg = GpuSegment(raw)
    try:
        ma = _mask("^www\\.domain[12]", sv)
        # a LIKE AND b BETWEEN (b: a bit-sliced conjunct), with a fused SUM
        qc = parse("SELECT COUNT(*), SUM(b) FROM t WHERE a LIKE 'www.domain1%' AND b BETWEEN 10 AND 120")
        want = _mask("^www\\.domain1", sv) & (b >= 10) & (b <= 120)
        blk = GpuInstancePlanMaker().make_instance_plan(qc, [seg]).next_block()
        assert int(blk.results[0]) == int(want.sum()) and int(blk.results[1]) == int(b[want].sum())
        # a pattern that matches nothing / everything beside a conjunct (the empty and the full id set)
        for pat, m in (("zzzzqq", np.zeros(n, bool)), ("", np.ones(n, bool))):
            qc = parse(f"SELECT COUNT(*), SUM(b) FROM t WHERE REGEXP_LIKE(a, '{pat}') AND b BETWEEN 10 AND 120")
            want = m & (b >= 10) & (b <= 120)
            blk = GpuInstancePlanMaker().make_instance_plan(qc, [seg]).next_block()
            assert int(blk.results[0]) == int(want.sum()) and int(blk.results[1] or 0) == int(b[want].sum()), pat
            got, _ = _count([seg], f"NOT REGEXP_LIKE(a, '{pat}') OR b < 5")
            assert got == int((~m | (b < 5)).sum()), pat
        # FILTER, GROUP BY
        qc = parse("SELECT COUNT(*) FILTER(WHERE a LIKE 'ab1%'), COUNT(*) FILTER(WHERE REGEXP_LIKE(a, 'com$')) FROM t")
        blk = GpuInstancePlanMaker().make_instance_plan(qc, [seg]).next_block()
        assert [int(x) for x in blk.results] == [int(_mask("^ab1", sv).sum()), int(_mask("com$", sv).sum())]
        qc = parse("SELECT b, COUNT(*) FROM t WHERE REGEXP_LIKE(a, '^www\\.domain[12]') GROUP BY b LIMIT 1000")
        blk = GpuInstancePlanMaker().make_instance_plan(qc, [seg]).next_block()
        want = {int(k): int(c) for k, c in zip(*np.unique(b[ma], return_counts=True))}
        assert {int(k[0]): int(v[0]) for k, v in blk.groups.items()} == want, "group-by with a match filter"
        # enableNullHandling: a null is neither LIKE nor NOT LIKE
        mc = _mask("^ab", sv)
        nh = "SET enableNullHandling = true; "
        assert _count([seg], "c LIKE 'ab%'", nh)[0] == int((mc & ~nulls).sum())
        assert _count([seg], "c NOT LIKE 'ab%'", nh)[0] == int((~mc & ~nulls).sum())
        # an MV STRING dictionary column: any value matches / none does
        mm = np.asarray([any(strmatch_ref.match_many("^x", row)) for row in mv])
        assert _count([seg], "REGEXP_LIKE(m, '^x')")[0] == int(mm.sum())
        assert _count([seg], "NOT REGEXP_LIKE(m, '^x')")[0] == int((~mm).sum())
        # one plan executed three times
        qc = parse("SELECT COUNT(*), SUM(b) FROM t WHERE a LIKE '%domain%' OR REGEXP_LIKE(m, 'ab4')")
        op = GpuInstancePlanMaker().make_instance_plan(qc, [seg])
        res = [tuple(op.next_block().results) for _ in range(3)]
        m4 = np.asarray([any(strmatch_ref.match_many("ab4", row)) for row in mv])
        want = _mask("domain", sv) | m4
        assert res[0] == res[1] == res[2] and int(res[0][0]) == int(want.sum())
    finally:
        seg.destroy()
    # OR of two match leaves with different DFAs on two raw columns, executed three times
    vals, other, _, g = raw_segments[0]
    want = _mask("main1", vals) | _mask("^[ab]+$", other)
    qc = parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(s, 'main1') OR REGEXP_LIKE(u, '^[ab]+$')")
    op = GpuInstancePlanMaker().make_instance_plan(qc, [g])
    assert [int(op.next_block().results[0]) for _ in range(3)] == [int(want.sum())] * 3
    assert np.array_equal(GpuCombineOperator(qc, [g], 100000).filter_bitmap(), _words(want))


# ---- 5. statistics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dict", "dict_inverted", "dict_sorted"])
def test_dictionary_leaf_always_scans(gpu_lib, layout):
    """FilterOperatorUtils.java:108-117: the leaf is a scan whatever index the column has, and the evaluator is never
    always-true / always-false: numEntriesScannedInFilter == num_docs."""
    raw = _golden_segment(f"st_{layout}", inverted=("DOMAIN_NAMES",) if layout == "dict_inverted" else (),
                          sort=layout == "dict_sorted")
    seg = GpuSegment(raw)
    try:
        n = QUERIES["num_rows"]
        for where, count in (("REGEXP_LIKE(DOMAIN_NAMES, 'zzzzqq')", 0), ("REGEXP_LIKE(DOMAIN_NAMES, '')", n),
                             ("DOMAIN_NAMES LIKE '%'", n), ("DOMAIN_NAMES LIKE 'www.domain1%'", 256),
                             ("DOMAIN_NAMES NOT LIKE '%domain%'", 0), ("DOMAIN_NAMES LIKE '%sd%'", 512)):
            got, stats = _count([seg], where)
            assert got == count, where
            assert stats.num_entries_scanned_in_filter == n, (layout, where)
    finally:
        seg.destroy()


def test_raw_leaf_statistics_and_shape(raw_segments):
    segs = [g for _, _, _, g in raw_segments]
    n = sum(g.num_docs for g in segs)
    op = GpuInstancePlanMaker().make_instance_plan(parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(s, 'main1')"), segs)
    stats = op.next_block().stats
    assert stats.num_entries_scanned_in_filter == n           # num_docs per match leaf of every unpruned entry
    op = GpuInstancePlanMaker().make_instance_plan(
        parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(s, 'main1') OR REGEXP_LIKE(u, 'ab')"), segs)
    assert op.next_block().stats.num_entries_scanned_in_filter == 2 * n
    shape = getattr(op, "launch_shape", None)
    if callable(shape):
        assert shape()["match_tasks"] == 4                    # two leaves x two segments in one launch


# ---- 6. library-level checks ----------------------------------------------------------------------------------------
def _match_rc(lib, seg, column, blob, nwords=None):
    blob = np.ascontiguousarray(blob, dtype=np.int32)
    out = np.zeros(1024, dtype=np.uint64)
    return lib.phip_segment_match_dictionary(seg.handle, column.encode(), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             len(blob) if nwords is None else nwords,
                                             out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(out))


class _FakeDfa:
    def __init__(self, blob):
        self.blob = blob

    def to_blob(self):
        return self.blob


def test_bad_blobs_and_types_are_refused(gpu_lib, raw_segments, monkeypatch):
    lib = gpu_lib
    raw = SegmentCreator("lib").add_column("s", DataType.STRING, np.asarray(["ab", "cd", "abcd"] * 50)) \
        .add_column("k", DataType.INT, np.arange(150)).build()
    seg = GpuSegment(raw)
    _, _, _, rseg = raw_segments[0]
    try:
        good = regex_dfa.compile_pattern("abc").to_blob()
        S, C = int(good[1]), int(good[2])
        assert _match_rc(lib, seg, "s", good) == _lib.PHIP_OK
        bad_trans = good.copy()
        bad_trans[-1] = (S << 16) | S                          # a transition == S
        bad_class = good.copy()
        bad_class[4 + (S + 31) // 32] |= C                     # byte 0's class >= C
        bad_start, bad_version, bad_caps = good.copy(), good.copy(), good.copy()
        bad_start[3] = S
        bad_version[0] = 99
        bad_caps[1] = _lib.STRMATCH_MAX_STATES + 1
        bads = [bad_trans, bad_class, bad_start, bad_version, bad_caps, good[:-1], good[:3]]
        for i, blob in enumerate(bads):
            assert _match_rc(lib, seg, "s", blob) == _lib.PHIP_ERR_INVALID, i
            # the same blob as a RAW_STRING_MATCH leaf (phip_filter_bitmap)
            from pinot_amd.engine import plan
            monkeypatch.setattr(plan.regex_dfa, "compile_pattern", lambda p, b=blob: _FakeDfa(b))
            op = GpuCombineOperator(parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(s, 'x')"), [rseg], 100000)
            with pytest.raises(_lib.PhipError) as e:
                op.filter_bitmap()
            monkeypatch.undo()
            assert e.value.code == _lib.PHIP_ERR_INVALID, i
        # a column that is not a dictionary STRING column
        assert _match_rc(lib, seg, "k", good) == _lib.PHIP_ERR_INVALID
        assert _match_rc(lib, rseg, "s", good) == _lib.PHIP_ERR_INVALID
        with pytest.raises(PatternTypeError):
            _count([seg], "k LIKE '1%'")
        with pytest.raises(ValueError):
            _count([seg], "REGEXP_LIKE(k, '1')")
    finally:
        seg.destroy()
