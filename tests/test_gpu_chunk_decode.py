"""The device chunk decoders (pinot_amd/csrc/load.hip, codec.h) on every codec, decode window and sequence kind.

Every case loads one small segment and reads every row back in doc order through the selection path
(SELECT col FROM t LIMIT 1000000); the rows are compared with the bytes the test wrote, bit for bit. The hand-made
streams come from tests/chunk_streams.py, and tests/test_chunk_streams.py shows on the CPU that each decodes to
model(ops) on two independent decoders and holds the sequence kinds it is named for.

The path taken (runtime.cpp load_column / load_varbyte), restated here so a case asserts where it runs: a chunk
is decoded in LDS when out_cap + in_cap + extra <= 163840 - 1024 = 162816 bytes, where out_cap is the largest
decoded chunk rounded up to 16 (var-byte: docs per chunk x (4 + longest value)), in_cap the largest encoded chunk
+ 8 rounded up to 16, and extra the codec's workspace (GZIP: 1344; ZSTANDARD: 10016 + out_cap for the literal
buffer). A launch with more than 65536 bytes raises the kernel's dynamic LDS limit first. Var-byte chunks beyond
the window are decoded from HBM into HBM (chunk_decode_global_kernel); fixed-width ones fail the load.

One case the block format rules out as stated: a match at offset 65535 cannot lie in a chunk of 8192 LONGs
(65536 bytes), because the match needs 65535 bytes before it and liblz4 wants it to start 12 bytes before the
end. The LZ4 case is a chunk of 8200 LONGs; the chunk of exactly 8192 LONGs is snappy's, whose copy-2 may copy
the one last byte from offset 65535."""
import zlib

import numpy as np
import pyarrow as pa
import pytest

from pinot_amd.segment.creator import CHUNK_COMPRESSION, SegmentCreator
from pinot_amd.spi import DataType
from tests import chunk_streams as cs
from tests.chunk_streams import encode, model

pytestmark = pytest.mark.gpu

LDS_WINDOW = 163840 - 1024
EXTRA = {"GZIP": lambda out_cap: 1344, "ZSTANDARD": lambda out_cap: 10016 + out_cap}
HANDMADE = ("SNAPPY", "LZ4", "LZ4_LENGTH_PREFIXED")
ALL_CODECS = ("SNAPPY", "ZSTANDARD", "LZ4", "LZ4_LENGTH_PREFIXED", "GZIP")


def _round16(x):
    return (x + 15) & ~15


def _lds_bytes(codec, decoded_max, bodies):
    out_cap = _round16(decoded_max)
    return out_cap + _round16(max(map(len, bodies)) + 8) + EXTRA.get(codec, lambda _: 0)(out_cap)


def _read_column(seg, col="v"):
    """Every row of ``col`` in doc order, through the selection path."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker
    from pinot_amd.engine.segment import GpuSegment
    from pinot_amd.query.sql import parse
    g = GpuSegment(seg)
    try:
        op = GpuInstancePlanMaker().make_instance_plan(parse(f"SELECT {col} FROM t LIMIT 1000000"), [g])
        blk = op.next_block()
        op.close()
        return [r[0] for r in blk.rows]
    finally:
        g.destroy()


def _fixed_segment(name, codec, dt, version, docs_per_chunk, data, bodies):
    """A one-column segment over the BE values in ``data`` whose forward index holds ``bodies``."""
    be = np.frombuffer(data, dtype=dt.numpy_be)
    vals = be.astype(dt.numpy)
    c = SegmentCreator(name, no_dictionary_columns=["v"], raw_compression={"v": codec},
                       docs_per_chunk=docs_per_chunk, raw_version=version)
    seg = c.add_column("v", dt, vals).build()
    entry = be.dtype.itemsize
    seg.columns["v"].forward = cs.fixed_chunk_index(bodies, version, docs_per_chunk, entry, len(vals), codec)
    return seg, vals


def _assert_fixed(seg, vals):
    got = _read_column(seg)
    assert len(got) == len(vals)
    assert np.asarray(got, dtype=vals.dtype).tobytes() == vals.tobytes()


def _string_segment(name, codec, version, docs_per_chunk, rows, bodies=None):
    c = SegmentCreator(name, no_dictionary_columns=["v"], raw_compression={"v": codec},
                       docs_per_chunk=docs_per_chunk, raw_version=version)
    seg = c.add_column("v", DataType.STRING, np.array(rows, dtype=object)).build()
    if bodies is not None:
        longest = max(len(r.encode("utf-8")) for r in rows)
        seg.columns["v"].forward = cs.var_byte_index(bodies, version, docs_per_chunk, longest, len(rows), codec)
    return seg


def _assert_hbm_path(seg, codec, version):
    """The header says this column decodes beyond the LDS window (load_varbyte's own rule)."""
    h = np.frombuffer(seg.columns["v"].forward[:28], dtype=">i4")
    assert (h[0], h[5]) == (version, CHUNK_COMPRESSION[codec])
    max_u = int(h[2]) * (4 + int(h[3]))
    assert max_u > LDS_WINDOW
    return max_u


# ---------------------------------------------------------------- a. LDS kernel, hand-made LZ4 / snappy chunks
@pytest.mark.parametrize("dt,version", [(DataType.LONG, 3), (DataType.INT, 2), (DataType.LONG, 2), (DataType.INT, 3)],
                         ids=["LONG-v3", "INT-v2", "LONG-v2", "INT-v3"])
@pytest.mark.parametrize("codec", HANDMADE)
def test_lds_handmade_fixed_width(gpu_lib, codec, dt, version):
    lists = cs.handmade_ops(codec)
    entry = np.dtype(dt.numpy_be).itemsize
    bodies = [encode(codec, o) for o in lists]
    seg, vals = _fixed_segment(f"hm_{codec}_{entry}_{version}", codec, dt, version, cs.HANDMADE_CHUNK_BYTES // entry,
                               b"".join(model(o) for o in lists), bodies)
    assert len(vals) % (cs.HANDMADE_CHUNK_BYTES // entry) == cs.HANDMADE_LAST_BYTES // entry  # a partial last chunk
    offs = cs.chunk_offsets(seg.columns["v"].forward)
    assert {(o - offs[0]) & 3 for o in offs} == {0, 1, 2, 3}
    assert _lds_bytes(codec, cs.HANDMADE_CHUNK_BYTES, bodies) <= 65536
    _assert_fixed(seg, vals)


@pytest.mark.parametrize("codec", HANDMADE)
def test_lds_handmade_match_at_offset_65535(gpu_lib, codec):
    """A match over the whole 16-bit offset range, in a chunk whose LDS window needs the raised limit."""
    ops = cs.snappy_ops("far", 65536) if codec == "SNAPPY" else cs.lz4_ops("far", 65600)
    docs = len(model(ops)) // 8
    assert docs == (8192 if codec == "SNAPPY" else 8200)
    bodies = [encode(codec, ops)]
    assert 65536 < _lds_bytes(codec, 8 * docs, bodies) <= LDS_WINDOW
    seg, vals = _fixed_segment(f"far_{codec}", codec, DataType.LONG, 3, docs, model(ops), bodies)
    _assert_fixed(seg, vals)


def test_lds_malformed_handmade_chunk_fails_the_load(gpu_lib):
    from pinot_amd import _lib
    from pinot_amd.engine.segment import GpuSegment
    from tests.test_chunk_streams import malformed_streams
    bad = malformed_streams()
    # the prefix one above and one below the block's decoded length; then, on the same path, an LZ4 match offset
    # beyond the decoded prefix and a snappy length off by one
    assert [b[0] for b in bad] == [4, 4, 3, 1]
    assert [int.from_bytes(b[1][:4], "little") - b[2] for b in bad[:2]] == [1, -1]
    names = {v: k for k, v in CHUNK_COMPRESSION.items()}
    for cid, body, size in bad:
        cid = names[cid]
        lists = cs.handmade_ops(cid)
        data = b"".join(model(o) for o in lists)
        bodies = [encode(cid, o) for o in lists]
        assert len(model(lists[1])) == size and (cid != "LZ4_LENGTH_PREFIXED" or body[4:] == bodies[1][4:])
        good = bodies[1]
        bodies[1] = body
        seg, vals = _fixed_segment("malformed", cid, DataType.LONG, 3, cs.HANDMADE_CHUNK_BYTES // 8, data, bodies)
        with pytest.raises(_lib.PhipError, match="malformed compressed chunk 1"):
            GpuSegment(seg)
        bodies[1] = good  # the same segment with the chunk as written loads and reads back
        seg, vals = _fixed_segment("wellformed", cid, DataType.LONG, 3, cs.HANDMADE_CHUNK_BYTES // 8, data, bodies)
        _assert_fixed(seg, vals)


# ---------------------------------------------------------------- b. LDS kernel, entropy codecs off their default
def _long_payloads(docs, seed):
    """LONG chunks after tests/test_codec.py chunks(): runs, a ramp, noise, all zeros (a zstd RLE block)."""
    rng = np.random.default_rng(seed)
    return [np.repeat(rng.integers(0, 2 ** 40, -(-docs // 25)), 25)[:docs],
            np.cumsum(rng.integers(0, 5, docs)),
            rng.integers(-2 ** 62, 2 ** 62, docs),
            np.zeros(docs, dtype=np.int64),
            rng.integers(0, 1000, docs // 3)]  # the partial last chunk: small values, long zero runs


def _zlib_strategy(level, strategy):
    def compress(data):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        return c.compress(data) + c.flush() + len(data).to_bytes(4, "big")  # GzipCompressor: + BE length
    return compress


ENTROPY_VARIANTS = {
    "zstd-5": ("ZSTANDARD", lambda d: pa.Codec("zstd", compression_level=-5).compress(d, asbytes=True)),
    "zstd1": ("ZSTANDARD", lambda d: pa.Codec("zstd", compression_level=1).compress(d, asbytes=True)),
    "zstd19": ("ZSTANDARD", lambda d: pa.Codec("zstd", compression_level=19).compress(d, asbytes=True)),
    "zstd22": ("ZSTANDARD", lambda d: pa.Codec("zstd", compression_level=22).compress(d, asbytes=True)),
    "zlib0": ("GZIP", _zlib_strategy(0, zlib.Z_DEFAULT_STRATEGY)),
    "zlib_fixed": ("GZIP", _zlib_strategy(6, zlib.Z_FIXED)),
    "zlib_huffman_only": ("GZIP", _zlib_strategy(6, zlib.Z_HUFFMAN_ONLY)),
    "zlib_rle": ("GZIP", _zlib_strategy(6, zlib.Z_RLE)),
}


@pytest.mark.parametrize("docs_per_chunk", [1000, 4500])
@pytest.mark.parametrize("variant", list(ENTROPY_VARIANTS))
def test_lds_entropy_codec_levels(gpu_lib, variant, docs_per_chunk):
    """1000 docs per chunk: the default launch. 4500: out_cap + in_cap alone pass 64 KiB (the noise chunk does not
    compress), so the launch raises the dynamic LDS limit, and the whole stays inside the window."""
    codec, compress = ENTROPY_VARIANTS[variant]
    payloads = _long_payloads(docs_per_chunk, seed=docs_per_chunk)
    data = b"".join(p.astype(">i8").tobytes() for p in payloads)
    bodies = [compress(p.astype(">i8").tobytes()) for p in payloads]
    lds = _lds_bytes(codec, 8 * docs_per_chunk, bodies)
    assert lds <= LDS_WINDOW and (lds > 65536) == (docs_per_chunk == 4500)
    seg, vals = _fixed_segment(f"ent_{variant}_{docs_per_chunk}", codec, DataType.LONG, 3, docs_per_chunk, data, bodies)
    _assert_fixed(seg, vals)


# ---------------------------------------------------------------- c. HBM kernel, the library's own compressors
@pytest.fixture(scope="module")
def long_rows():
    return cs.long_string_rows()


@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("codec", ALL_CODECS)
def test_hbm_library_compressors(gpu_lib, long_rows, codec, version):
    """Three chunks of 1000 rows (the last with 500 absent rows), a 300-byte longest row: 304 000 bytes per chunk
    buffer, so every codec decodes from HBM into HBM, with a per-chunk output stride and zstd literal scratch."""
    seg = _string_segment(f"hbm_{codec}_{version}", codec, version, 1000, long_rows)
    assert _assert_hbm_path(seg, codec, version) == 304000
    assert _read_column(seg) == long_rows


# ---------------------------------------------------------------- d. HBM kernel, hand-made LZ4 / snappy chunks
@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("codec", HANDMADE)
def test_hbm_handmade_var_byte(gpu_lib, codec, version):
    chunks = cs.handmade_var_byte(codec)
    rows = [r.decode("ascii") for chunk_rows, _ in chunks for r in chunk_rows]
    bodies = [encode(codec, ops) for _, ops in chunks]
    seg = _string_segment(f"hbm_hm_{codec}_{version}", codec, version, cs.VAR_DOCS_PER_CHUNK, rows, bodies)
    _assert_hbm_path(seg, codec, version)
    assert len(rows) == 5 * cs.VAR_DOCS_PER_CHUNK + cs.VAR_LAST_ROWS
    assert _read_column(seg) == rows


# ---------------------------------------------------------------- e. HBM kernel, chunks beyond one zstd block
@pytest.fixture(scope="module")
def many_words():
    return cs.word_rows(40000)


@pytest.mark.parametrize("codec", ["ZSTANDARD", "GZIP", "LZ4"])
def test_hbm_chunks_beyond_one_zstd_block(gpu_lib, many_words, codec):
    """16384 rows per chunk: a decoded chunk of 65536 start-offset bytes + the rows' bytes, several 128 KiB zstd
    blocks (and several deflate blocks), decoded by one lane; the last chunk is partial."""
    docs_per_chunk = 16384
    decoded = 4 * docs_per_chunk + sum(len(w) for w in many_words[:docs_per_chunk])
    assert decoded > 131072
    seg = _string_segment(f"big_{codec}", codec, 3, docs_per_chunk, many_words)
    _assert_hbm_path(seg, codec, 3)
    assert _read_column(seg) == many_words


# ---------------------------------------------------------------- f. malformed input on the HBM path
@pytest.mark.parametrize("codec", ALL_CODECS)
def test_hbm_malformed_chunk_fails_the_load(gpu_lib, long_rows, codec):
    """The second chunk's first byte flipped (LZ4: its first match offset set beyond the decoded prefix, since a
    changed token may still decode): the load fails, and the next segment loads and reads back in the same process."""
    from pinot_amd import _lib
    from pinot_amd.engine.segment import GpuSegment
    seg = _string_segment(f"bad_{codec}", codec, 3, 1000, long_rows)
    _assert_hbm_path(seg, codec, 3)
    fwd = bytearray(seg.columns["v"].forward)
    second = cs.chunk_offsets(bytes(fwd))[1]
    if codec == "LZ4":
        at = second + cs.lz4_first_offset_at(bytes(fwd[second:]))
        fwd[at:at + 2] = b"\xff\xff"  # (the prefix here: the literals before the first match, far below 65535)
        assert at - second < 4000
    else:
        fwd[second] ^= 0x5A
    seg.columns["v"].forward = bytes(fwd)
    with pytest.raises(_lib.PhipError, match="malformed compressed chunk 1"):
        GpuSegment(seg)
    good = _string_segment(f"good_{codec}", codec, 3, 1000, long_rows)
    assert _read_column(good) == long_rows
