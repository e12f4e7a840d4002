"""Entropy-coded chunk codecs: the decoder source the GPU chunk decode runs
(pinot_amd/csrc/codec.h), built for the host, against the libraries the reference binds:
GZIP = java.util.zip (zlib) Deflater/Inflater (GzipCompressor.java / GzipDecompressor.java) -- Python's zlib is
that library; ZSTANDARD = zstd-jni (libzstd) -- pyarrow's zstd codec is that library."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "codec", "libcodec_host.so")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(HERE, "codec", "codec_host.cpp")
    hdr = os.path.join(os.path.dirname(HERE), "pinot_amd", "csrc", "codec.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, src])
    L = ctypes.CDLL(SO)
    for f in (L.phip_test_pinot_gzip, L.phip_test_inflate_zlib):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return L


def chunks(seed=0):
    """Chunk payloads shaped like Pinot raw forward-index chunks (BE fixed-width values) plus hard cases."""
    rng = np.random.default_rng(seed)
    out = [b"", b"\x00" * 8, bytes(rng.integers(0, 256, 8000, dtype=np.uint8))]
    out.append(rng.integers(0, 1000, 1000).astype(">i8").tobytes())           # small LONGs: long zero runs
    out.append(np.cumsum(rng.integers(0, 5, 1000)).astype(">i8").tobytes())   # sorted timestamps
    out.append(rng.normal(size=1000).astype(">f8").tobytes())                  # DOUBLE noise
    out.append(np.repeat(rng.integers(0, 2 ** 31, 40), 25).astype(">i4").tobytes())  # runs
    out.append((b"abcdefgh" * 2000)[:16000])                                   # long matches, overlap
    out.append(rng.integers(0, 2 ** 62, 4096).astype(">i8").tobytes())        # 32 KiB incompressible-ish
    return out


def pinot_gzip(data, level):
    """GzipCompressor.compress: Deflater output + 4-byte BE uncompressed size."""
    return zlib.compress(data, level) + len(data).to_bytes(4, "big")


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_gzip_chunks_match_zlib(lib, level):
    for data in chunks(level):
        comp = pinot_gzip(data, level)
        out = ctypes.create_string_buffer(max(len(data), 1))
        n = lib.phip_test_pinot_gzip(comp, len(comp), out, len(data))
        assert n == len(data) and out.raw[:n] == data


def test_gzip_fixed_and_stored_blocks(lib):
    data = chunks(3)[4]
    for strategy in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strategy)
        comp = c.compress(data) + c.flush() + len(data).to_bytes(4, "big")
        out = ctypes.create_string_buffer(len(data))
        assert lib.phip_test_pinot_gzip(comp, len(comp), out, len(data)) == len(data)
        assert out.raw == data


def test_gzip_malformed_rejected(lib):
    data = chunks(1)[3]
    comp = bytearray(pinot_gzip(data, 6))
    out = ctypes.create_string_buffer(len(data))
    bad_adler = bytes(comp[:-5]) + bytes([comp[-5] ^ 1]) + bytes(comp[-4:])
    assert lib.phip_test_pinot_gzip(bad_adler, len(bad_adler), out, len(data)) == -1
    bad_len = bytes(comp[:-1]) + bytes([comp[-1] ^ 1])
    assert lib.phip_test_pinot_gzip(bad_len, len(bad_len), out, len(data)) == -1
    assert lib.phip_test_pinot_gzip(bytes(comp[:len(comp) // 2]), len(comp) // 2, out, len(data)) == -1
    small = ctypes.create_string_buffer(len(data) - 1)
    assert lib.phip_test_pinot_gzip(bytes(comp), len(comp), small, len(data) - 1) == -1
    rng = np.random.default_rng(5)
    for _ in range(200):  # random corruption: never crashes, never returns a wrong length silently
        b = bytearray(comp)
        i = int(rng.integers(2, len(b) - 8))
        b[i] ^= int(rng.integers(1, 256))
        n = lib.phip_test_pinot_gzip(bytes(b), len(b), out, len(data))
        assert n in (-1, len(data))
        if n == len(data):
            assert out.raw == data or zlib.adler32(out.raw) == zlib.adler32(data)


def zstd_compress(data, level):
    import pyarrow as pa
    return pa.Codec("zstd", compression_level=level).compress(data, asbytes=True)


@pytest.fixture(scope="module")
def zlib_(lib):
    lib.phip_test_zstd.restype = ctypes.c_int
    lib.phip_test_zstd.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return lib


@pytest.mark.parametrize("level", [-5, 1, 3, 9, 19, 22])
def test_zstd_chunks_match_libzstd(zlib_, level):
    for data in chunks(100 + level):
        if not data:
            continue
        comp = zstd_compress(data, level)
        out = ctypes.create_string_buffer(len(data))
        n = zlib_.phip_test_zstd(comp, len(comp), out, len(data))
        assert n == len(data) and out.raw == data, (level, len(data), n)


def test_zstd_malformed_rejected(zlib_):
    data = chunks(7)[4]
    comp = zstd_compress(data, 3)
    out = ctypes.create_string_buffer(len(data))
    assert zlib_.phip_test_zstd(comp[:-3], len(comp) - 3, out, len(data)) == -1
    assert zlib_.phip_test_zstd(b"\x00" + comp[1:], len(comp), out, len(data)) == -1
    small = ctypes.create_string_buffer(len(data) - 1)
    assert zlib_.phip_test_zstd(comp, len(comp), small, len(data) - 1) == -1
    rng = np.random.default_rng(9)
    for _ in range(300):
        b = bytearray(comp)
        i = int(rng.integers(5, len(b)))
        b[i] ^= int(rng.integers(1, 256))
        n = zlib_.phip_test_zstd(bytes(b), len(b), out, len(data))
        assert n in (-1, len(data))


# ---- frames of more than one zstd block (128 KiB): Pinot's derived var-byte chunks are 1 MiB by default -----------
@pytest.fixture(scope="module")
def big_chunks():
    from tests.chunk_streams import var_byte_chunk, word_rows
    rng = np.random.default_rng(42)
    low = bytes(rng.integers(0, 4, 300_000, dtype=np.uint8) * 17)  # 2 bits of entropy per byte: Huffman literals
    rows = [w.encode() for w in word_rows(22_000)]
    strings = var_byte_chunk(rows, len(rows))                       # 88 000 start-offset bytes + the words: ~440 KB
    assert len(strings) > 400_000
    return [low, strings, bytes(300_000)]


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_gzip_big_chunks_match_zlib(lib, big_chunks, level):
    for data in big_chunks:
        comp = pinot_gzip(data, level)
        out = ctypes.create_string_buffer(len(data))
        n = lib.phip_test_pinot_gzip(comp, len(comp), out, len(data))
        assert n == len(data) and out.raw == data, (level, len(data), n)


def test_gzip_big_chunks_fixed_and_stored_blocks(lib, big_chunks):
    for data in big_chunks:
        for strategy in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strategy)
            comp = c.compress(data) + c.flush() + len(data).to_bytes(4, "big")
            out = ctypes.create_string_buffer(len(data))
            assert lib.phip_test_pinot_gzip(comp, len(comp), out, len(data)) == len(data), (strategy, len(data))
            assert out.raw == data


def zstd_blocks(frame):
    """Block count of a single-segment-or-not zstd frame (RFC 8878 §3.1.1: magic, frame header, 3-byte block
    headers with the last-block bit)."""
    fhd = frame[4]
    single, dict_id = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3]
    fcs = (0, 2, 4, 8)[fhd >> 6] or single
    p, blocks = 5 + (0 if single else 1) + dict_id + fcs, 0
    while True:
        h = int.from_bytes(frame[p:p + 3], "little")
        blocks += 1
        p += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)  # an RLE block stores one byte
        if h & 1:
            return blocks


@pytest.mark.parametrize("level", [-5, 1, 3, 9, 19, 22])
def test_zstd_big_chunks_match_libzstd(zlib_, big_chunks, level):
    for data in big_chunks:
        comp = zstd_compress(data, level)
        assert zstd_blocks(comp) >= 3  # 300 000 bytes and more: at least three 128 KiB blocks
        out = ctypes.create_string_buffer(len(data))
        n = zlib_.phip_test_zstd(comp, len(comp), out, len(data))
        assert n == len(data) and out.raw == data, (level, len(data), n)
