"""The hand-made chunk streams of tests/chunk_streams.py, checked on the CPU before the GPU decodes them
(tests/test_gpu_chunk_decode.py): every stream decodes to model(ops) with Arrow's bundled liblz4 / libsnappy and
with the oracle's decoder, and every stream's census shows the sequence kinds it is named for -- so a GPU test
cannot pass on a stream that lost its hard parts. Malformed streams are rejected by both CPU decoders."""
import numpy as np
import pyarrow as pa
import pytest

from oracle import lib as oracle_lib
from tests import chunk_streams as cs
from tests.chunk_streams import (encode, handmade_ops, lz4_block, lz4_census, lz4_ops, model, snappy_block,
                                 snappy_census, snappy_ops)

HANDMADE = ("SNAPPY", "LZ4", "LZ4_LENGTH_PREFIXED")


def arrow_decode(codec, body, size):
    """The decoded bytes, or None where Arrow's decoder refuses the stream or decodes another length."""
    cid = cs.CHUNK_COMPRESSION[codec] if isinstance(codec, str) else codec
    if cid == 4:
        if len(body) < 4 or int.from_bytes(body[:4], "little") != size:
            return None  # lz4-java's LZ4DecompressorWithLength decodes exactly the prefixed length
        body = body[4:]
    try:
        out = pa.decompress(body, decompressed_size=size, codec="snappy" if cid == 1 else "lz4_raw", asbytes=True)
    except (pa.ArrowException, OSError, ValueError):
        return None
    return out if len(out) == size else None


def oracle_decode(codec, body, size):
    cid = cs.CHUNK_COMPRESSION[codec] if isinstance(codec, str) else codec
    src = np.frombuffer(body, dtype=np.uint8).copy()
    dst = np.zeros(max(size, 1), dtype=np.uint8)
    got = oracle_lib().oracle_chunk_decode(cid, src.ctypes.data, len(body), dst.ctypes.data, size)
    return dst[:got].tobytes() if got == size else None


def assert_decodes(codec, ops):
    want, body = model(ops), encode(codec, ops)
    assert arrow_decode(codec, body, len(want)) == want
    assert oracle_decode(codec, body, len(want)) == want


# ------------------------------------------------------------------------------------------ the helpers themselves
def test_model_repeats_the_period_of_an_overlapping_match():
    assert model([("L", b"abc"), ("M", 3, 7)]) == b"abcabcabca"
    assert model([("L", b"x"), ("M", 1, 5), ("L", b"yz"), ("M", 2, 3)]) == b"xxxxxxyzyzy"
    assert model([("L", b"abcd"), ("M", 4, 4), ("M", 6, 2)]) == b"abcdabcdcd"
    with pytest.raises(ValueError):
        model([("L", b"ab"), ("M", 3, 4)])


def test_lz4_length_extensions():
    """15 -> extension byte 0; 15 + 255 -> 255, 0; 15 + 254 -> 254: the remainder byte is always written."""
    tail = [("L", bytes(12))]
    for n, ext in ((14, b""), (15, b"\x00"), (269, b"\xfe"), (270, b"\xff\x00"), (271, b"\xff\x01"),
                   (15 + 510, b"\xff\xff\x00")):
        blob = lz4_block([("L", b"q" * n), ("M", 1, 4)] + tail)
        assert blob[:1 + len(ext)] == bytes([(min(n, 15) << 4)]) + ext, n
        blob = lz4_block([("L", b"q"), ("M", 1, n + 4)] + tail)
        assert blob[:4 + len(ext)] == bytes([0x10 | min(n, 15)]) + b"q\x01\x00" + ext, n
    assert lz4_block([("L", b"ab"), ("L", b"cd")]) == b"\x40abcd"  # adjacent literals merge
    assert lz4_block([]) == b"\x00"


def test_lz4_block_refuses_what_liblz4_refuses():
    """The end-of-block rules: liblz4 rejects the stream an emitter without them would write."""
    for ops in ([("L", b"x"), ("M", 1, 20), ("L", b"!")],             # 1 literal at the end
                [("L", b"x"), ("M", 1, 4), ("L", b"abcde")],          # the last match starts 9 bytes before the end
                [("L", b"x"), ("M", 1, 20)],                          # ends on a match
                [("L", b"xyz"), ("M", 1, 3), ("L", bytes(12))],       # a 3-byte match
                [("L", b"xyz"), ("M", 4, 8), ("L", bytes(12))]):      # beyond the prefix
        with pytest.raises(ValueError):
            lz4_block(ops)
    # test_oracle_handcrafted_lz4_sequences' stream (1 literal after the last match): Arrow refuses it
    assert arrow_decode(3, bytes([0x1F, ord("x"), 1, 0, 1, 0x10, ord("!")]), 22) is None
    ok = [("L", b"x"), ("M", 1, 20), ("L", b"!" * 5)]                 # the same match inside the rules
    assert arrow_decode(3, lz4_block(ok), 26) == model(ok) == b"x" * 21 + b"!" * 5


def test_snappy_block_encodings():
    assert snappy_block([("L", b"a")]) == b"\x01\x00a"
    assert snappy_block([("L", b"a", 1)]) == b"\x01\xf0\x00a"
    assert snappy_block([("L", b"a", 4)]) == b"\x01\xfc\x00\x00\x00\x00a"
    assert snappy_block([("L", b"ab"), ("M", 2, 4)]) == b"\x06\x04ab\x01\x02"
    assert snappy_block([("L", b"ab"), ("M", 2, 4, 2)]) == b"\x06\x04ab\x0e\x02\x00"
    assert snappy_block([("L", b"ab"), ("M", 2, 4)], copy_kind=4) == b"\x06\x04ab\x0f\x02\x00\x00\x00"
    assert snappy_block([("L", b"a" * 200)], literal_len_bytes=3)[:6] == b"\xc8\x01\xf8\xc7\x00\x00"
    for ops in ([("L", b"a" * 61, 0)], [("L", b"a" * 300, 1)], [("L", b"ab"), ("M", 2, 12, 1)],
                [("L", b"ab"), ("M", 2, 65, 2)], [("L", b"ab"), ("M", 3, 4)], [("L", b"")]):
        with pytest.raises(ValueError):
            snappy_block(ops)


def test_census_reads_back_what_the_emitters_wrote():
    ops = [("L", b"q" * 20), ("M", 1, 4), ("M", 20, 20), ("L", b"r" * 270), ("M", 3, 274), ("L", bytes(12))]
    c = lz4_census(lz4_block(ops))
    assert c["literal_runs"] == {20, 270, 12} and c["match_lens"] == {4, 20, 274} and c["offsets"] == {1, 20, 3}
    assert c["matches"] == {(1, 4), (20, 20), (3, 274)} and c["overlapping"] == 2
    assert c["ext255"] == 2 and c["ext0"] == 2 and c["match_after_match"] == 1 and c["size"] == len(model(ops))
    assert (c["literal_run_max"], c["match_len_max"]) == (270, 274)
    ops = [("L", b"q" * 70, 2), ("L", b"r"), ("M", 1, 4, 1), ("M", 70, 64, 2), ("M", 3, 9, 4), ("L", b"s", 3)]
    c = snappy_census(snappy_block(ops))
    assert (c["copy1"], c["copy2"], c["copy4"]) == (1, 1, 1) and c["overlapping"] == 2
    assert c["copies"] == {(1, 1, 4), (2, 70, 64), (4, 3, 9)}
    assert c["literal_width"] == {0: 1, 1: 0, 2: 1, 3: 1, 4: 0} and c["literals"] == {(2, 70), (0, 1), (3, 1)}
    assert c["size"] == len(model(ops))
    # what the library compressors emit for the existing fixed-width GPU data holds none of the hard kinds
    lib = lz4_census(pa.compress(np.arange(1000, dtype=">i8").tobytes(), codec="lz4_raw", asbytes=True))
    assert lib["size"] == 8000


def test_index_framing_matches_the_creator():
    """fixed_chunk_index / var_byte_index / var_byte_chunk write the creator's bytes around the creator's bodies."""
    from pinot_amd.segment.creator import _chunk_forward, _compress_chunk, _var_byte_forward
    from pinot_amd.spi import DataType
    rng = np.random.default_rng(2)
    vals = rng.integers(-2 ** 40, 2 ** 40, 2500)
    data = vals.astype(">i8").tobytes()
    rows = [f"row{v}" * int(k) for v, k in zip(vals.tolist(), rng.integers(0, 4, 2500))]
    enc = [r.encode() for r in rows]
    for version in (2, 3):
        for codec in ("PASS_THROUGH", "LZ4", "GZIP"):
            cid = cs.CHUNK_COMPRESSION[codec]
            bodies = [_compress_chunk(data[k:k + 8000], cid) for k in range(0, len(data), 8000)]
            assert cs.fixed_chunk_index(bodies, version, 1000, 8, 2500, codec) == \
                _chunk_forward(vals, DataType.LONG, 1000, version, codec)
            bodies = [_compress_chunk(cs.var_byte_chunk(enc[k:k + 1000], 1000), cid) for k in range(0, 2500, 1000)]
            index = cs.var_byte_index(bodies, version, 1000, max(map(len, enc)), 2500, cid)
            assert index == _var_byte_forward(rows, 1000, version, codec)
            assert cs.chunk_offsets(index)[0] == 28 + 3 * (4 if version == 2 else 8)
    with pytest.raises(ValueError):
        cs.fixed_chunk_index([b""], 3, 1000, 8, 2500, 3)


# ------------------------------------------------------------------------------------------ the GPU tests' streams
def _union(census_list, key):
    return set().union(*(c[key] for c in census_list))


@pytest.mark.parametrize("ascii_only", [False, True])
@pytest.mark.parametrize("codec", HANDMADE)
def test_handmade_streams_decode_on_both_cpu_decoders(codec, ascii_only):
    for ops in handmade_ops(codec, ascii_only=ascii_only):
        assert_decodes(codec, ops)
    far = snappy_ops("far", 65536) if codec == "SNAPPY" else lz4_ops("far", 65600)
    assert_decodes(codec, far)


@pytest.mark.parametrize("ascii_only", [False, True])
def test_handmade_lz4_census(ascii_only):
    lists = handmade_ops("LZ4", ascii_only=ascii_only)
    assert [len(model(o)) for o in lists] == [cs.HANDMADE_CHUNK_BYTES] * 5 + [cs.HANDMADE_LAST_BYTES]
    cens = [lz4_census(lz4_block(o)) for o in lists]
    runs, lens = _union(cens, "literal_runs"), _union(cens, "match_lens")
    offsets, matches = _union(cens, "offsets"), _union(cens, "matches")
    assert {14, 15, 15 + 255} <= runs and max(runs) >= 270 and any(r > 270 for r in runs)
    assert {4, 18, 19, 64, 65, 129, 19 + 255} <= lens and any(m > 274 for m in lens)
    assert {1, 2, 3, 7, 63, 64, 65} <= offsets
    assert any(off == n for off, n in matches) and any(off > n for off, n in matches)
    assert any(off < n and n > 64 for off, n in matches)       # an overlapping match of more than one lane trip
    full = cens[0]
    assert full["match_len_max"] > 64 and full["match_after_match"] >= 4 and full["ext255"] >= 4
    assert full["ext0"] >= 4                                     # 15, 15 + 255 literals; 19, 19 + 255 match bytes
    assert cens[2]["matches"] == set() and cens[2]["literal_run_max"] == cs.HANDMADE_CHUNK_BYTES
    assert {(3, 19), (2, 274), (64, 64)} <= cens[5]["matches"]  # the partial last chunk keeps hard kinds too
    far = lz4_census(lz4_block(lz4_ops("far", 65600)))
    assert 65535 in far["offsets"] and far["size"] == 65600 and far["literal_run_max"] == 65535


@pytest.mark.parametrize("ascii_only", [False, True])
def test_handmade_snappy_census(ascii_only):
    lists = handmade_ops("SNAPPY", ascii_only=ascii_only)
    assert [len(model(o)) for o in lists] == [cs.HANDMADE_CHUNK_BYTES] * 5 + [cs.HANDMADE_LAST_BYTES]
    cens = [snappy_census(snappy_block(o)) for o in lists]
    full = cens[0]
    assert {(0, 1), (0, 60), (1, 61), (3, 5), (4, 7)} <= full["literals"]
    assert any(w == 2 and n >= 256 for w, n in full["literals"])
    assert all(full["literal_width"][w] >= 1 for w in range(5))
    assert {(1, off, n) for off in (1, 2047) for n in (4, 11)} <= full["copies"]
    assert {(2, off, n) for off in (63, 64, 65, 2048) for n in (1, 64)} <= full["copies"]
    assert (2, 3, 64) in full["copies"] and full["copy4"] >= 1 and full["overlapping"] >= 3
    assert cens[2]["copies"] == set()
    last = cens[5]
    assert last["copy4"] >= 1 and (2, 3, 64) in last["copies"] and last["literal_width"][3] >= 1 \
        and last["literal_width"][4] >= 1
    far = snappy_census(snappy_block(snappy_ops("far", 65536)))
    assert (2, 65535, 1) in far["copies"] and far["size"] == 65536


@pytest.mark.parametrize("codec", HANDMADE)
@pytest.mark.parametrize("version", [2, 3])
def test_handmade_chunk_offsets_cover_every_alignment(codec, version):
    """The LDS kernel stages a chunk from the dword below its first byte (head = src & 3): every head occurs."""
    bodies = [encode(codec, o) for o in handmade_ops(codec)]
    offs = cs.chunk_offsets(cs.fixed_chunk_index(bodies, version, 350, 8, 5 * 350 + 150, codec))
    assert {(o - offs[0]) & 3 for o in offs} == {0, 1, 2, 3}


@pytest.mark.parametrize("codec", HANDMADE)
def test_handmade_var_byte_chunks(codec):
    """The var-byte chunks around the same operations: they decode to var_byte_chunk(rows) on both CPU decoders,
    the rows are ASCII, some are empty, one is the 300-byte longest, and the census still shows the hard kinds
    behind the start-offset literal."""
    chunks = cs.handmade_var_byte(codec)
    assert [len(rows) for rows, _ in chunks] == [cs.VAR_DOCS_PER_CHUNK] * 5 + [cs.VAR_LAST_ROWS]
    for (rows, ops), plain in zip(chunks, handmade_ops(codec, ascii_only=True)):
        assert model(ops) == cs.var_byte_chunk(rows, cs.VAR_DOCS_PER_CHUNK)
        assert b"".join(rows) == model(plain) and b"".join(rows).decode("ascii")
        assert max(map(len, rows)) == cs.VAR_LONG_ROW and min(map(len, rows)) == 0
        assert_decodes(codec, ops)
    # rows cut inside a match: a row boundary strictly inside the 300-byte (3, 300) match of the "full" lists
    rows, ops = chunks[0]
    if codec != "SNAPPY":
        c = lz4_census(lz4_block(ops))
        assert {(3, 300), (64, 274), (1, 4), (64, 64)} <= c["matches"] and {14, 15, 270} <= c["literal_runs"]
        start = len(model(ops[:ops.index(("M", 3, 300))])) - 4 * cs.VAR_DOCS_PER_CHUNK
        ends = np.cumsum([len(r) for r in rows])
        assert np.any((ends > start) & (ends < start + 300))
    else:
        c = snappy_census(snappy_block(ops))
        assert c["copy4"] >= 1 and (2, 3, 64) in c["copies"] and all(c["literal_width"][w] >= 1 for w in range(5))
    assert cs.VAR_DOCS_PER_CHUNK * (4 + cs.VAR_LONG_ROW) > 162816


def test_library_lz4_chunks_of_long_rows_hold_the_named_sequences():
    """What liblz4 emits for long_string_rows (the HBM-path segments of the library compressors): matches of 274
    bytes or more at offsets 1, 2 and 3 and a literal run of 270 or more, in every chunk."""
    from pinot_amd.segment.creator import _compress_chunk
    rows = [r.encode("utf-8") for r in cs.long_string_rows()]
    assert max(map(len, rows)) == 300 and b"" in rows and any(len(r) != len(r.decode()) for r in rows)
    for k in range(0, 2500, 1000):
        c = lz4_census(_compress_chunk(cs.var_byte_chunk(rows[k:k + 1000], 1000), 3))
        for off in (1, 2, 3):
            assert any(o == off and n >= 274 for o, n in c["matches"]), (k, off)
        assert c["literal_run_max"] >= 270 and c["ext255"] >= 4


# ------------------------------------------------------------------------------------------ malformed streams
def malformed_streams():
    """(codec, body, decoded size) of the malformed hand-made chunks the GPU tests load."""
    ops = handmade_ops("LZ4_LENGTH_PREFIXED")[1]
    size = len(model(ops))
    block = lz4_block(ops)
    out = [(4, (size + 1).to_bytes(4, "little") + block, size),      # length prefix one byte off
           (4, (size - 1).to_bytes(4, "little") + block, size)]
    far = bytearray(lz4_block(handmade_ops("LZ4")[1]))              # first match offset beyond the decoded prefix
    assert far[0] >> 4 == 15 and far[1] == 70 - 15                  # ("short": 70 literals, then the match)
    far[2 + 70:4 + 70] = (71).to_bytes(2, "little")
    out.append((3, bytes(far), size))
    sn = bytearray(snappy_block(handmade_ops("SNAPPY")[1]))
    sn[0] ^= 0x01                                                   # the varint length off by one
    out.append((1, bytes(sn), size))
    return out


def test_malformed_handmade_streams_are_rejected_by_both_cpu_decoders():
    for codec, body, size in malformed_streams():
        assert arrow_decode(codec, body, size) is None, codec
        assert oracle_decode(codec, body, size) is None, codec
        assert oracle_decode(codec, body, size + 1) is None, codec  # (nor with room for one byte more)
