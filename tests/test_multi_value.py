"""CPU tests of multi-value column support: the forward index bytes against a hand-derived fixture
(tests/golden/mv_forward_index.json, derivation in its note), the segment directory round trip, the planner's mapping of
the six *MV aggregations and its refusals, and the library's answer where the multi-value kernels are absent."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd.engine import plan as planmod
from pinot_amd.engine.plan import MvReduce, UnsupportedOnGpu, check_multi_value, plan_aggregations
from pinot_amd.engine.reduce import final_result
from pinot_amd.engine.results import merge_intermediate
from pinot_amd.query.sql import parse
from pinot_amd.segment import roaring
from pinot_amd.segment.creator import (MV_ENTRY_DICT_MAGIC, SegmentCreator, mv_docs_per_chunk, mv_forward_bytes,
                                       read_mv_forward, read_mv_offsets)
from pinot_amd.segment.store import read_segment_dir, write_segment_dir
from pinot_amd.spi import DataType

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "mv_forward_index.json")) as f:
    GOLDEN = json.load(f)


# ---- forward index bytes ---------------------------------------------------------------------------------------------
def test_forward_index_small_fixture():
    g = GOLDEN["small"]
    rows = [np.asarray(r, dtype=np.int32) for r in g["rows"]]
    total = sum(len(r) for r in rows)
    assert total / len(rows) != total // len(rows)  # (9 / 5: not an integer)
    assert mv_docs_per_chunk(len(rows), total) == g["docs_per_chunk"]
    buf = mv_forward_bytes(rows, g["bits"])
    assert buf.hex() == g["hex"]
    ids, off = read_mv_forward(buf, len(rows), total, g["bits"])
    assert [ids[off[d]:off[d + 1]].tolist() for d in range(len(rows))] == g["rows"]


def test_forward_index_two_chunks_fixture():
    g = GOLDEN["chunks"]
    flat = np.zeros(sum(g["row_lengths"]), dtype=np.int32)
    flat[g["ones"]] = 1
    cuts = np.cumsum([0] + g["row_lengths"])
    rows = [flat[cuts[d]:cuts[d + 1]] for d in range(len(g["row_lengths"]))]
    assert mv_docs_per_chunk(len(rows), len(flat)) == g["docs_per_chunk"] == 2  # two chunks for three docs
    want = bytearray(g["size"])
    for o, v in g["nonzero"].items():
        want[int(o)] = v
    buf = mv_forward_bytes(rows, g["bits"])
    assert buf == bytes(want)
    ids, off = read_mv_forward(buf, len(rows), len(flat), g["bits"])
    assert np.array_equal(ids, flat) and off.tolist() == cuts.tolist()


def test_docs_per_chunk_is_the_writers_float_arithmetic():
    # 2048 / (float)(7 / 2 = 3) = 682.67 -> 683; an exact quotient stays; the inner division truncates first
    assert mv_docs_per_chunk(2, 7) == 683 and mv_docs_per_chunk(10, 40) == 512 and mv_docs_per_chunk(10, 49) == 512


def test_bad_start_bits_fail_the_read():
    rows = [np.array([0, 1], np.int32), np.array([1], np.int32), np.array([0, 0, 1], np.int32)]
    buf = bytearray(mv_forward_bytes(rows, 1))
    read_mv_forward(bytes(buf), 3, 6, 1)
    with pytest.raises(ValueError, match="row starts"):
        read_mv_forward(bytes(buf), 4, 6, 1)  # three start bits, four docs
    buf[4] |= 0x40  # a fourth start bit (value 1)
    with pytest.raises(ValueError, match="row starts"):
        read_mv_forward(bytes(buf), 3, 6, 1)


def _entry_dict_buffer(size):
    """The 24-byte header FixedBitMVEntryDictForwardIndexWriter writes (:98-105: marker, version, bits per value, unique
    entries, total values, the two buffer offsets) over zeroed sections: what tells the encoding apart is the marker."""
    import struct
    return struct.pack(">IhhIIII", MV_ENTRY_DICT_MAGIC, 1, 2, 3, 9, 28, 44) + bytes(size - 24)


def test_entry_dict_encoding_is_refused_by_name(tmp_path):
    """FixedBitMVEntryDictForwardIndexWriter buffers (first int 0xffabcdef, ForwardIndexReaderFactory.java:84) are an
    unsupported encoding, not a corrupt plain one."""
    assert MV_ENTRY_DICT_MAGIC == 0xFFABCDEF
    with pytest.raises(NotImplementedError, match="FixedBitMVEntryDictForwardIndexWriter"):
        read_mv_offsets(_entry_dict_buffer(64), 5, 9, 2)
    with pytest.raises(NotImplementedError, match="FixedBitMVEntryDictForwardIndexWriter"):
        read_mv_forward(_entry_dict_buffer(64), 5, 9, 2)
    seg, _ = _segment(n=50, inverted=())
    seg.columns["tags"].forward = _entry_dict_buffer(len(seg.columns["tags"].forward))
    write_segment_dir(seg, str(tmp_path), 3)
    with pytest.raises(NotImplementedError, match="FixedBitMVEntryDictForwardIndexWriter"):
        read_segment_dir(str(tmp_path))


def test_offsets_are_read_without_decoding_ids():
    rows = [np.array([0, 1], np.int32), np.array([1], np.int32), np.array([0, 0, 1], np.int32)]
    buf = mv_forward_bytes(rows, 1)
    assert read_mv_offsets(buf, 3, 6, 1).tolist() == [0, 2, 3, 6] == read_mv_forward(buf, 3, 6, 1)[1].tolist()


# ---- creator and directory round trip -------------------------------------------------------------------------------
def _segment(n=3000, seed=3, inverted=("tags", "a")):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, 40, rng.integers(1, 6)) * 7 for _ in range(n)]
    c = SegmentCreator("mvseg", inverted_index_columns=inverted)
    c.add_column("a", DataType.INT, rng.integers(0, 9, n))
    c.add_column("tags", DataType.LONG, rows, multi_value=True)
    c.add_column("names", DataType.STRING, [[f"n{v}" for v in r[:2]] for r in rows], multi_value=True)
    c.add_column("s", DataType.INT, np.sort(rng.integers(0, 5, n)))
    return c.build(), rows


def test_creator_metadata_and_inverted_index():
    seg, rows = _segment()
    m = seg.columns["tags"].metadata
    assert (m.is_single_value, m.is_sorted, m.has_dictionary) == (False, False, True)
    assert m.total_number_of_entries == sum(len(r) for r in rows)
    assert m.max_number_of_multi_values == max(len(r) for r in rows)
    sv = seg.columns["a"].metadata
    assert (sv.is_single_value, sv.max_number_of_multi_values, sv.total_number_of_entries) == (True, 0, 0)
    uniq = np.unique(np.concatenate(rows))
    assert m.cardinality == len(uniq)
    ids, off = read_mv_forward(seg.columns["tags"].forward, seg.num_docs, m.total_number_of_entries, m.bits_per_element)
    assert all(np.array_equal(uniq[ids[off[d]:off[d + 1]]], rows[d]) for d in range(0, seg.num_docs, 97))  # row order kept
    inv = seg.columns["tags"].inverted
    offs = np.frombuffer(inv[:4 * (m.cardinality + 1)], dtype=">u4").astype(np.int64)
    for d in (0, 5, m.cardinality - 1):  # a doc is under every id it holds, once
        want = np.array([i for i, r in enumerate(rows) if uniq[d] in r])
        assert inv[offs[d]:offs[d + 1]] == roaring.serialize(want, True)  # (the per-id doc set's own bitmap)


def test_creator_refusals():
    c = SegmentCreator("x", no_dictionary_columns=["r"])
    with pytest.raises(ValueError, match="null"):
        c.add_column("m", DataType.INT, [[1], [2]], nulls=[False, True], multi_value=True)
    with pytest.raises(ValueError, match="raw"):
        c.add_column("r", DataType.INT, [[1], [2]], multi_value=True)
    with pytest.raises(ValueError, match="at least one value"):
        c.add_column("m", DataType.INT, [[1], []], multi_value=True)


@pytest.mark.parametrize("version", [1, 3])
def test_segment_dir_round_trip(tmp_path, version):
    seg, _ = _segment()
    write_segment_dir(seg, str(tmp_path), version)
    if version == 1:
        assert os.path.exists(tmp_path / "tags.mv.fwd") and os.path.exists(tmp_path / "a.sv.unsorted.fwd")
    props = open(tmp_path / ("v3" if version == 3 else "") / "metadata.properties").read()
    m = seg.columns["tags"].metadata
    assert "column.tags.isSingleValues = false" in props and "column.a.isSingleValues = true" in props
    assert f"column.tags.maxNumberOfMultiValues = {m.max_number_of_multi_values}" in props
    assert f"column.tags.totalNumberOfEntries = {m.total_number_of_entries}" in props
    assert "column.a.maxNumberOfMultiValues" not in props  # single-value columns are written as before
    back = read_segment_dir(str(tmp_path))
    assert list(back.columns) == list(seg.columns)
    for name, ci in seg.columns.items():
        b = back.columns[name]
        assert b.metadata == ci.metadata, name
        assert (b.forward, b.dictionary, b.inverted) == (ci.forward, ci.dictionary, ci.inverted), name


def test_load_fails_when_start_bits_differ_from_docs(tmp_path):
    seg, _ = _segment(n=50, inverted=())
    write_segment_dir(seg, str(tmp_path), 1)
    path = tmp_path / "metadata.properties"
    path.write_text(path.read_text().replace("segment.total.docs = 50", "segment.total.docs = 49"))
    with pytest.raises(ValueError, match="row starts"):
        read_segment_dir(str(tmp_path))


# ---- planner ---------------------------------------------------------------------------------------------------------
class _Seg:
    """The planner's view of a segment: column metadata only."""

    def __init__(self, seg):
        self.segment, self.name, self.num_docs = seg, seg.name, seg.num_docs

    def has_column(self, c):
        return c in self.segment.columns

    def column_metadata(self, c):
        return self.segment.columns[c].metadata

    def has_null_vector(self, c):
        return False


def test_six_functions_map_to_primitives_and_reductions():
    q = parse("SELECT COUNTMV(tags), SUMMV(tags), MINMV(tags), MAXMV(tags), AVGMV(tags), MINMAXRANGEMV(tags), SUM(a) FROM t")
    assert [a.result_column_name for a in q.aggregations][:6] == [
        "countmv(tags)", "summv(tags)", "minmv(tags)", "maxmv(tags)", "avgmv(tags)", "minmaxrangemv(tags)"]
    prims, mapping = plan_aggregations(q.aggregations)
    red = {(p[0], p[2].reduce): i for i, p in enumerate(prims) if isinstance(p[2], MvReduce)}
    ln, sm = red[(_lib.AGG_SUM, _lib.MV_REDUCE_LENGTH)], red[(_lib.AGG_SUM, _lib.MV_REDUCE_SUM)]
    mn, mx = red[(_lib.AGG_MIN, _lib.MV_REDUCE_MIN)], red[(_lib.AGG_MAX, _lib.MV_REDUCE_MAX)]
    assert len(red) == 4 and all(p[2].columns == ["tags"] for p in prims[:4])
    assert mapping[:6] == [("count", ln), ("sum", sm), ("min", mn), ("max", mx), ("avg", (sm, ln)), ("minmaxrange", (mn, mx))]
    assert prims[mapping[6][1]][:3] == (_lib.AGG_SUM, _lib.EXPR_COLUMN, "a")
    assert MvReduce("tags", 2) == MvReduce("tags", 2) != MvReduce("tags", 3)


def test_results_and_types():
    assert final_result("countmv", merge_intermediate("countmv", 3, 4)) == 7 and type(final_result("countmv", 7)) is int
    assert final_result("summv", merge_intermediate("summv", 3, 4)) == 7.0 and type(final_result("summv", 7)) is float
    assert final_result("avgmv", merge_intermediate("avgmv", (6, 2), (4.0, 2))) == 2.5
    assert final_result("minmv", merge_intermediate("minmv", 3.0, 4.0)) == 3.0
    assert final_result("maxmv", merge_intermediate("maxmv", 3.0, 4.0)) == 4.0
    assert final_result("minmaxrangemv", merge_intermediate("minmaxrangemv", (3.0, 4.0), (1.0, 3.5))) == 3.0


def test_unfiltered_extremes_take_the_non_scan_path():
    seg = _Seg(_segment(n=100, inverted=())[0])
    for sql, fit in (("SELECT MINMV(tags) FROM t", True), ("SELECT MAXMV(tags), MINMAXRANGEMV(tags), COUNT(*) FROM t", True),
                     ("SELECT MINMV(tags), SUMMV(tags) FROM t", False), ("SELECT COUNTMV(tags) FROM t", False)):
        op = planmod.GpuCombineOperator.__new__(planmod.GpuCombineOperator)
        op.query, op.segments, op.trees = parse(sql), [seg], [planmod._TRUE]
        assert op._non_scan_fit() is fit, sql


REFUSALS = [
    ("SELECT tags, COUNT(*) FROM t GROUP BY tags", "GROUP BY on the multi-value column tags"),
    ("SELECT a, tags FROM t LIMIT 5", "selecting or ordering by the multi-value column tags"),
    ("SELECT a FROM t ORDER BY tags LIMIT 5", "selecting or ordering by the multi-value column tags"),
    ("SELECT * FROM t LIMIT 5", "multi-value column"),
    ("SELECT SUM(tags) FROM t", "single-value aggregation sum over the multi-value column tags"),
    ("SELECT DISTINCTCOUNT(tags) FROM t", "single-value aggregation distinctcount over the multi-value column tags"),
    ("SELECT SUMMV(a) FROM t", "summv over the single-value column a"),
    ("SELECT SUM(tags + 1) FROM t", "arithmetic over the multi-value column tags"),
    ("SELECT SUMMV(tags * 2) FROM t", "arithmetic over a multi-value column"),
    ("SELECT DISTINCTCOUNTMV(tags) FROM t", "distinctcountmv is not on the GPU path"),
    ("SELECT DISTINCTCOUNTHLLMV(tags) FROM t", "distinctcounthllmv is not on the GPU path"),
    ("SELECT PERCENTILEMV(tags, 90) FROM t", "percentilemv is not on the GPU path"),
    ("SELECT PERCENTILE95MV(tags) FROM t", "percentilemv is not on the GPU path"),
    ("SELECT PERCENTILETDIGEST50MV(tags) FROM t", "percentiletdigestmv is not on the GPU path"),
    ("SELECT DISTINCTSUMMV(tags) FROM t", "distinctsummv is not on the GPU path"),
    ("SELECT DISTINCTAVGMV(tags) FROM t", "distinctavgmv is not on the GPU path"),
    ("SELECT SUM(ARRAYLENGTH(tags)) FROM t", "ARRAYLENGTH"),
    ("SELECT COUNT(*) FROM t GROUP BY VALUEIN(tags, 7, 14)", "VALUEIN"),
    ("SET enableNullHandling = true; SELECT COUNTMV(tags) FROM t", "under enableNullHandling"),
    ("SET enableNullHandling = true; SELECT COUNT(*) FROM t WHERE tags = 7", "under enableNullHandling"),
]


@pytest.mark.parametrize("sql,reason", REFUSALS, ids=[r[1][:40] for r in REFUSALS])
def test_refusals_name_their_reason(sql, reason):
    seg = _Seg(_segment(n=100, inverted=())[0])
    q = parse(sql)
    with pytest.raises(UnsupportedOnGpu, match=reason.replace("(", r"\(").replace(")", r"\)")):
        check_multi_value(q, [seg])
        plan_aggregations(q.aggregations)


def test_more_refusals():
    seg, _ = _segment(n=100, inverted=())
    with pytest.raises(UnsupportedOnGpu, match="star-tree"):
        check_multi_value(parse("SELECT COUNTMV(tags) FROM t"), [_Seg(seg)], star_tree=True)
    from pinot_amd.segment.startree import StarTreeIndexConfig
    c = SegmentCreator("st", star_tree_configs=[StarTreeIndexConfig(["tags"], [], ["COUNT__*"], 10)])
    c.add_column("tags", DataType.INT, [[1], [2, 3]], multi_value=True)
    c.add_column("a", DataType.INT, [1, 2])
    with pytest.raises(ValueError, match="star-tree over the multi-value column tags"):
        c.build()
    # raw multi-value forward indexes (FixedByteChunkMVForwardIndexReader, VarByteChunkMVForwardIndexReader) fail the load
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_segment_dir(seg, d, 1)
        p = os.path.join(d, "metadata.properties")
        text = open(p).read().replace("column.tags.hasDictionary = true", "column.tags.hasDictionary = false")
        open(p, "w").write(text)
        with pytest.raises(NotImplementedError, match="raw \\(no-dictionary\\) multi-value column tags"):
            read_segment_dir(d)


def test_inverted_choice_prices_the_mv_forward_index_by_its_own_bytes(monkeypatch):
    """INVERTED_COST_RATIO compares the bitmaps' bytes with total_values x bits / 8, not num_docs x bits / 8."""
    seg, rows = _segment(n=2000)

    class S(_Seg):
        def dictionary(self, c):
            from pinot_amd.segment.dictionary import Dictionary
            ci = self.segment.columns[c]
            return Dictionary(ci.dictionary, ci.metadata.data_type, ci.metadata.cardinality, ci.metadata.string_width)

        def inverted_bytes(self, c, ids):
            return self.bytes

    s = S(seg)
    m = seg.columns["tags"].metadata
    docs_bytes = (seg.num_docs * m.bits_per_element + 7) // 8
    values_bytes = (m.total_number_of_entries * m.bits_per_element + 7) // 8
    assert values_bytes > 2 * docs_bytes
    monkeypatch.setenv("PINOT_AMD_INVERTED_RATIO", "1.0")
    pred = parse("SELECT COUNT(*) FROM t WHERE tags = 7").filter.predicate
    s.bytes = values_bytes  # within the forward index's own bytes: the inverted index
    assert planmod.compile_predicate(s, pred).kind == _lib.LEAF_INVERTED
    s.bytes = values_bytes + 1
    assert planmod.compile_predicate(s, pred).kind == _lib.LEAF_DICT_RANGE


# ---- a library without the multi-value kernels ----------------------------------------------------------------------
_HOSTSIM_SCRIPT = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2])
    import numpy as np
    from pinot_amd import _lib
    _lib.LIB_PATH = sys.argv[1]
    from pinot_amd.engine.plan import GpuCombineOperator
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    from pinot_amd.segment.creator import SegmentCreator
    from pinot_amd.spi import DataType
    rng = np.random.default_rng(0)
    c = SegmentCreator("h", inverted_index_columns=["m"])
    c.add_column("a", DataType.INT, rng.integers(0, 9, 300))
    c.add_column("m", DataType.INT, [rng.integers(0, 30, rng.integers(1, 4)) for _ in range(300)], multi_value=True)
    raw = c.build()
    g = GpuSegment(raw)
    import copy, struct
    bad = copy.deepcopy(raw)  # the entry-dictionary encoding: refused by name at load, not parsed as a corrupt plain one
    fwd = bad.columns["m"].forward
    bad.columns["m"].forward = struct.pack(">IhhIIII", 0xFFABCDEF, 1, 5, 3, 9, 28, 44) + bytes(len(fwd) - 24)
    try:
        GpuSegment(bad)
    except _lib.PhipUnsupported as e:
        assert "FixedBitMVEntryDictForwardIndexWriter" in str(e), e
    else:
        raise SystemExit("entry-dictionary forward index loaded")
    import os
    for env, sql in ((("PINOT_AMD_INVERTED_RATIO", "0"), "SELECT COUNT(*) FROM t WHERE m IN (3, 9)"),
                     (("PINOT_AMD_INVERTED_RATIO", "0"), "SELECT COUNT(*) FROM t WHERE m BETWEEN 3 AND 9 AND a < 4"),
                     (None, "SELECT SUMMV(m) FROM t WHERE a < 4"), (None, "SELECT COUNTMV(m) FROM t")):
        if env:
            os.environ[env[0]] = env[1]
        try:
            GpuCombineOperator(parse(sql), [g], 1000).run_raw()
        except _lib.PhipUnsupported as e:
            assert "multi-value" in str(e), e
        else:
            raise SystemExit("not refused: " + sql)
    os.environ["PINOT_AMD_INVERTED"] = "always"  # the inverted index of the column needs no multi-value kernel
    GpuCombineOperator(parse("SELECT COUNT(*) FROM t WHERE m IN (3, 9)"), [g], 1000).run_raw()
    print("MV HOSTSIM OK")
""")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_library_without_the_mv_kernels_refuses(tmp_path):
    """The host simulation (runtime.cpp over tests/hostsim/hip_stub.cpp, no kernel unit): no launcher is registered, so
    a plan with an MV scan leaf or an MV row reduction is PHIP_ERR_UNSUPPORTED; the column still loads and its inverted
    index still answers."""
    so = str(tmp_path / "libpinot_hip_hostsim_mv.so")
    src = [os.path.join(ROOT, "pinot_amd", "csrc", "runtime.cpp"), os.path.join(ROOT, "pinot_amd", "csrc", "node.cpp"),
           os.path.join(HERE, "hostsim", "hip_stub.cpp")]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O0", "-std=c++17", "-fPIC", "-shared", "-nogpulib",
                           "-o", so] + src + ["-ldl"], stderr=subprocess.DEVNULL)
    p = subprocess.run([sys.executable, "-c", _HOSTSIM_SCRIPT, so, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "MV HOSTSIM OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
