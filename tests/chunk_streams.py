"""Hand-made LZ4 / snappy chunk streams and the chunk index framing around them (no GPU, no oracle).

A stream is written from a list of operations, ("L", bytes) or ("M", offset, length), so a test decides which
sequence kinds a chunk holds instead of taking what a compressor happens to emit: length extensions that end on a
0 byte, matches longer than one 64-lane trip, overlapping copies of every small period, snappy's 4-byte-offset copy
and its 2 / 3 / 4-byte literal lengths. model(ops) is what every such stream decodes to. The census functions parse a
stream back into counts and extremes, so a test can assert that a stream still holds what it is named for.

Formats: LZ4 block format (lz4_Block_format.md: token, literal length, literals, LE offset, match length; the
end-of-block rules -- the last sequence is literals only with at least 5 of them, the last match starts at least
12 bytes before the end -- are enforced by liblz4's decoder); snappy raw format (format_description.txt: varint
length, then literal / copy-1 / copy-2 / copy-4 elements); the chunk index header of BaseChunkForwardIndexWriter
(BaseChunkForwardIndexWriter.java:40-60) as pinot_amd/segment/creator.py writes it."""
import numpy as np

from pinot_amd.segment.creator import CHUNK_COMPRESSION

LZ4_LAST_LITERALS = 5   # the last sequence holds at least this many literals (when the block has a match)
LZ4_MFLIMIT = 12        # the last match starts at least this many bytes before the end of the block


# ------------------------------------------------------------------------------------------ operations
def model(ops) -> bytes:
    """The bytes a list of operations decodes to. A match copies byte by byte, so offset < length repeats the
    last ``offset`` bytes. (An operation may carry a trailing encoding hint, which decides no byte.)"""
    out = bytearray()
    for op in ops:
        if op[0] == "L":
            out += op[1]
        elif op[0] == "M":
            off, length = op[1], op[2]
            if not 0 < off <= len(out) or length < 1:
                raise ValueError(f"match {op} at position {len(out)}")
            for _ in range(length):
                out.append(out[-off])
        else:
            raise ValueError(f"operation {op!r}")
    return bytes(out)


def _lz4_len(n: int) -> bytes:
    """Length extension after a nibble of 15: (n - 15) as 255 bytes plus the remainder (a 0 byte included)."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_block(ops) -> bytes:
    """One LZ4 block: adjacent literals merged, lengths >= 15 extended. Refuses an operation list that liblz4
    would not decode: a match shorter than 4 or farther than 65535 or beyond the decoded prefix, and, once the
    block holds a match, a tail of fewer than 5 literals or a last match inside the last 12 bytes."""
    seqs, lit, pos, last_match = [], bytearray(), 0, None
    for op in ops:
        if op[0] == "L":
            lit += op[1]
            pos += len(op[1])
        elif op[0] == "M":
            _, off, length = op
            if not 1 <= off <= 65535 or off > pos or length < 4:
                raise ValueError(f"LZ4 match {op} at position {pos}")
            seqs.append((bytes(lit), off, length))
            lit = bytearray()
            last_match = pos
            pos += length
        else:
            raise ValueError(f"operation {op!r}")
    if last_match is not None:
        if len(lit) < LZ4_LAST_LITERALS:
            raise ValueError(f"LZ4 block ends with {len(lit)} literals (at least {LZ4_LAST_LITERALS})")
        if pos - last_match < LZ4_MFLIMIT:
            raise ValueError(f"LZ4 block: the last match starts {pos - last_match} bytes before the end "
                             f"(at least {LZ4_MFLIMIT})")
    out = bytearray()
    for data, off, length in seqs:
        ln, ml = len(data), length - 4
        out.append((min(ln, 15) << 4) | min(ml, 15))
        if ln >= 15:
            out += _lz4_len(ln)
        out += data
        out += off.to_bytes(2, "little")
        if ml >= 15:
            out += _lz4_len(ml)
    out.append(min(len(lit), 15) << 4)
    if len(lit) >= 15:
        out += _lz4_len(len(lit))
    out += lit
    return bytes(out)


def _varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def snappy_block(ops, literal_len_bytes=None, copy_kind=None) -> bytes:
    """One raw snappy stream. A literal's length is inline in its tag (width 0, up to 60 bytes) or follows the tag
    in 1..4 bytes; a copy is copy-1 (length 4..11, offset < 2048), copy-2 or copy-4 (length 1..64). An operation
    chooses for itself with a trailing element -- ("L", bytes, width) / ("M", offset, length, kind) -- and
    ``literal_len_bytes`` / ``copy_kind`` choose for those that do not (None: the narrowest that fits)."""
    out, pos = bytearray(_varint(len(model(ops)))), 0
    for op in ops:
        if op[0] == "L":
            data = op[1]
            width = op[2] if len(op) > 2 else literal_len_bytes
            n = len(data)
            if n < 1:
                raise ValueError("snappy literal of 0 bytes")
            if width is None:
                width = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
            if width == 0:
                if n > 60:
                    raise ValueError(f"snappy literal of {n} bytes with an inline length")
                out.append((n - 1) << 2)
            else:
                if not 1 <= width <= 4 or n - 1 >= 1 << (8 * width):
                    raise ValueError(f"snappy literal of {n} bytes in {width} length bytes")
                out.append((59 + width) << 2)
                out += (n - 1).to_bytes(width, "little")
            out += data
            pos += n
        elif op[0] == "M":
            off, length = op[1], op[2]
            kind = op[3] if len(op) > 3 else copy_kind
            if not 0 < off <= pos:
                raise ValueError(f"snappy copy {op} at position {pos}")
            if kind is None:
                kind = 1 if 4 <= length <= 11 and off < 2048 else (2 if off < 65536 else 4)
            if kind == 1:
                if not 4 <= length <= 11 or off >= 2048:
                    raise ValueError(f"snappy copy-1 {op}")
                out.append(1 | ((length - 4) << 2) | ((off >> 8) << 5))
                out.append(off & 0xFF)
            elif kind in (2, 4):
                if not 1 <= length <= 64 or off >= 1 << (8 * kind):
                    raise ValueError(f"snappy copy-{kind} {op}")
                out.append((2 if kind == 2 else 3) | ((length - 1) << 2))
                out += off.to_bytes(kind, "little")
            else:
                raise ValueError(f"snappy copy kind {kind}")
            pos += length
        else:
            raise ValueError(f"operation {op!r}")
    return bytes(out)


# ------------------------------------------------------------------------------------------ census
def lz4_census(blob: bytes) -> dict:
    """What an LZ4 block holds: ``literal_runs`` / ``match_lens`` (sets of lengths), ``literal_run_max`` /
    ``match_len_max``, ``offsets`` (set), ``matches`` (set of (offset, length)), ``overlapping`` (matches with
    offset < length), ``ext255`` (255 bytes in length extensions), ``ext0`` (extensions that end on a 0 byte),
    ``match_after_match`` (matches with no literal before them, the block's first sequence aside) and ``size``."""
    c = dict(literal_runs=set(), match_lens=set(), offsets=set(), matches=set(), overlapping=0, ext255=0, ext0=0,
             match_after_match=0, size=0)
    ip, first = 0, True

    def extend(v):
        nonlocal ip
        if v == 15:
            while True:
                b = blob[ip]
                ip += 1
                v += b
                if b != 255:
                    c["ext0"] += b == 0
                    break
                c["ext255"] += 1
        return v

    while ip < len(blob):
        tok = blob[ip]
        ip += 1
        lit = extend(tok >> 4)
        if ip + lit > len(blob):
            raise ValueError("LZ4 literals run past the block")
        ip += lit
        c["size"] += lit
        if lit or ip == len(blob):
            c["literal_runs"].add(lit)
        if ip == len(blob):
            break
        off = blob[ip] | (blob[ip + 1] << 8)
        ip += 2
        ml = extend(tok & 15) + 4
        if lit == 0 and not first:
            c["match_after_match"] += 1
        c["match_lens"].add(ml)
        c["offsets"].add(off)
        c["matches"].add((off, ml))
        c["overlapping"] += off < ml
        c["size"] += ml
        first = False
    c["literal_run_max"] = max(c["literal_runs"], default=0)
    c["match_len_max"] = max(c["match_lens"], default=0)
    return c


def snappy_census(blob: bytes) -> dict:
    """What a snappy stream holds: ``copy1`` / ``copy2`` / ``copy4`` (counts), ``copies`` (set of (kind, offset,
    length)), ``literal_width`` (count per length width, 0 = inline), ``literals`` (set of (width, length)),
    ``overlapping`` (copies with offset < length) and ``size`` (the varint's value)."""
    ip, size, shift = 0, 0, 0
    while True:
        b = blob[ip]
        ip += 1
        size |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    c = dict(copy1=0, copy2=0, copy4=0, copies=set(), literal_width={w: 0 for w in range(5)}, literals=set(),
             overlapping=0, size=size)
    while ip < len(blob):
        tag = blob[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            n, width = (tag >> 2) + 1, 0
            if n > 60:
                width = n - 60
                n = int.from_bytes(blob[ip:ip + width], "little") + 1
                ip += width
            if ip + n > len(blob):
                raise ValueError("snappy literal runs past the stream")
            ip += n
            c["literal_width"][width] += 1
            c["literals"].add((width, n))
            continue
        if kind == 1:
            length, off, k = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | blob[ip], 1
            ip += 1
        else:
            k = 2 if kind == 2 else 4
            length, off = (tag >> 2) + 1, int.from_bytes(blob[ip:ip + k], "little")
            ip += k
        c[f"copy{k}"] += 1
        c["copies"].add((k, off, length))
        c["overlapping"] += off < length
    return c


# ------------------------------------------------------------------------------------------ index framing
def _index(bodies, version, docs_per_chunk, entry, n, codec) -> bytes:
    if version not in (2, 3):
        raise ValueError(f"chunk index version {version}")
    if isinstance(codec, str):
        codec = CHUNK_COMPRESSION[codec]
    if len(bodies) != -(-n // docs_per_chunk):
        raise ValueError(f"{len(bodies)} chunk bodies for {n} docs in chunks of {docs_per_chunk}")
    off_size = 4 if version == 2 else 8
    header = np.array([version, len(bodies), docs_per_chunk, entry, n, codec, 7 * 4], dtype=">i4").tobytes()
    pos, offsets = 7 * 4 + len(bodies) * off_size, []
    for body in bodies:
        offsets.append(pos)
        pos += len(body)
    return header + np.asarray(offsets, dtype=">i4" if version == 2 else ">i8").tobytes() + b"".join(bodies)


def fixed_chunk_index(bodies, version, docs_per_chunk, entry, n, codec) -> bytes:
    """The fixed-byte chunk forward index creator._chunk_forward writes (v2: int offsets, v3: long offsets), around
    chunk bodies that are already encoded."""
    return _index(bodies, version, docs_per_chunk, entry, n, codec)


def var_byte_index(bodies, version, docs_per_chunk, longest, n, codec) -> bytes:
    """The var-byte chunk forward index creator._var_byte_forward writes (lengthOfLongestEntry in the entry slot),
    around chunk bodies that are already encoded."""
    return _index(bodies, version, docs_per_chunk, longest, n, codec)


def var_byte_chunk(rows, docs_per_chunk) -> bytes:
    """The decoded bytes of one var-byte chunk: docs_per_chunk BE int start offsets (0 for the absent rows of a
    partial chunk), then the rows' bytes."""
    if len(rows) > docs_per_chunk:
        raise ValueError(f"{len(rows)} rows in a chunk of {docs_per_chunk}")
    starts = np.zeros(docs_per_chunk, dtype=">i4")
    p = 4 * docs_per_chunk
    for j, r in enumerate(rows):
        starts[j] = p
        p += len(r)
    return starts.tobytes() + b"".join(rows)


def chunk_offsets(index: bytes):
    """The absolute chunk offsets an index's table holds."""
    version, num_chunks = (int(x) for x in np.frombuffer(index, dtype=">i4", count=2))
    return np.frombuffer(index, dtype=">i4" if version == 2 else ">i8", count=num_chunks, offset=28).tolist()


# ------------------------------------------------------------------------------------------ the hand-made chunks
# The operation lists the GPU tests decode (tests/test_gpu_chunk_decode.py) and tests/test_chunk_streams.py checks
# on the CPU. Each decodes to exactly ``size`` bytes: a fixed head of the sequence kinds it is named for, ``pad``
# 8-byte (2 literals + a 6-byte match at offset 2) sequences that only move the encoded length, and literal filler.
def _bytes(rng, n, ascii_only):
    if ascii_only:
        return bytes(rng.integers(0x61, 0x7B, n, dtype=np.uint8))  # a..z
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _fill(ops, size, rng, ascii_only, pad, min_tail, pad_op):
    for _ in range(pad):
        ops += [("L", _bytes(rng, 2, ascii_only)), pad_op]
    tail = size - len(model(ops))
    if tail < min_tail:
        raise ValueError(f"{size} bytes leave a tail of {tail}")
    if tail:
        ops.append(("L", _bytes(rng, tail, ascii_only)))
    return ops


def lz4_ops(kind, size, seed=0, pad=0, ascii_only=False):
    """LZ4 operation lists. "full": literal runs of 14, 15 (extension byte 0), 15 + 255 and 300; match lengths 4,
    18, 19 (extension 0), 64, 65, 129, 19 + 255 and 300; offsets 1, 2, 3, 7, 63, 64, 65; offset = length (64, 64),
    offset > length (200, 100); matches that directly follow a match. "short": a subset for a partial chunk.
    "literal": no match at all. "far": a match at offset 65535 (its prefix needs size >= 65535 + 33 + 12)."""
    rng = np.random.default_rng(seed)
    L = lambda n: ("L", _bytes(rng, n, ascii_only))  # noqa: E731
    if kind == "full":
        ops = [L(300), ("M", 1, 4), L(14), ("M", 2, 18), L(15), ("M", 3, 19), L(270), ("M", 7, 64), ("M", 63, 65),
               ("M", 64, 64), ("M", 65, 129), ("M", 64, 274), ("M", 200, 100), ("M", 3, 300)]
    elif kind == "short":
        ops = [L(70), ("M", 65, 4), ("M", 1, 18), L(14), ("M", 3, 19), ("M", 64, 64), L(15), ("M", 7, 129),
               ("M", 2, 274)]
    elif kind == "literal":
        ops = []
    elif kind == "far":
        ops = [L(65535), ("M", 65535, 33)]
    else:
        raise ValueError(kind)
    return _fill(ops, size, rng, ascii_only, pad, LZ4_MFLIMIT if ops else 0, ("M", 2, 6))


def snappy_ops(kind, size, seed=0, pad=0, ascii_only=False):
    """Snappy operation lists. "full": inline literals of 1 and 60 bytes, 61 bytes in 1 length byte, 2100 in 2,
    5 in 3 and 7 in 4; copy-1 of lengths 4 and 11 at offsets 1 and 2047; copy-2 of lengths 1 and 64 at offsets 63,
    64, 65 and 2048; a copy-2 (3, 64) that repeats a 3-byte period; one copy-4. "short": a subset for a partial
    chunk. "literal": one literal. "far": a copy-2 of 1 byte at offset 65535 that ends a 65536-byte chunk."""
    rng = np.random.default_rng(seed)
    L = lambda n, *w: ("L", _bytes(rng, n, ascii_only), *w)  # noqa: E731
    if kind == "full":
        ops = [L(2100, 2), L(1, 0)]
        ops += [("M", off, n, 1) for off in (1, 2047) for n in (4, 11)]
        ops += [L(60, 0)]
        ops += [("M", off, n, 2) for off in (63, 64, 65, 2048) for n in (1, 64)]
        ops += [("M", 3, 64, 2), L(61, 1), L(5, 3), L(7, 4), ("M", 100, 30, 4)]
    elif kind == "short":
        ops = [L(300, 2), ("M", 3, 64, 2), ("M", 200, 10, 4), L(3, 3), ("M", 1, 4, 1), L(1, 0), L(2, 4)]
    elif kind == "literal":
        ops = []
    elif kind == "far":
        ops = [L(65535, 2), ("M", 65535, 1, 2)]
    else:
        raise ValueError(kind)
    return _fill(ops, size, rng, ascii_only, pad, 0, ("M", 2, 6, 1))


def encode(codec, ops) -> bytes:
    """One chunk body of a ChunkCompressionType (name or number): SNAPPY, LZ4 or LZ4_LENGTH_PREFIXED (lz4-java's
    LZ4CompressorWithLength: the 4-byte LE decoded length, then the block)."""
    if isinstance(codec, str):
        codec = CHUNK_COMPRESSION[codec]
    if codec == 1:
        return snappy_block(ops)
    if codec == 3:
        return lz4_block(ops)
    if codec == 4:
        return len(model(ops)).to_bytes(4, "little") + lz4_block(ops)
    raise ValueError(f"no hand-made streams for chunk compression {codec}")


# (kind, pad) per full chunk, then the partial last chunk; the pads spread the chunks' byte offsets over src & 3
HANDMADE_CHUNKS = (("full", 0), ("short", 0), ("literal", 0), ("full", 0), ("full", 2), ("short", 0))
HANDMADE_CHUNK_BYTES = 2800  # 350 LONGs / 700 INTs
HANDMADE_LAST_BYTES = 1200   # the partial last chunk: 150 LONGs / 300 INTs


def handmade_ops(codec, ascii_only=False, chunk_bytes=HANDMADE_CHUNK_BYTES, last_bytes=HANDMADE_LAST_BYTES):
    """The operation lists of one hand-made segment: full chunks of ``chunk_bytes`` decoded bytes and a partial last
    one. LZ4_LENGTH_PREFIXED wraps the LZ4 lists."""
    if isinstance(codec, str):
        codec = CHUNK_COMPRESSION[codec]
    make = snappy_ops if codec == 1 else lz4_ops
    sizes = [chunk_bytes] * (len(HANDMADE_CHUNKS) - 1) + [last_bytes]
    return [make(kind, size, seed=100 * codec + k, pad=pad, ascii_only=ascii_only)
            for k, ((kind, pad), size) in enumerate(zip(HANDMADE_CHUNKS, sizes))]


def lz4_first_offset_at(blob: bytes) -> int:
    """The position of the first match's 2-byte offset in an LZ4 block."""
    lit, p = blob[0] >> 4, 1
    if lit == 15:
        while blob[p] == 255:
            lit, p = lit + 255, p + 1
        lit, p = lit + blob[p], p + 1
    return p + lit


# Var-byte chunks around the same operation lists: a chunk decodes to var_byte_chunk(rows), so its stream is one
# literal for the start offsets, then the operations, and its rows are model(ops) cut at arbitrary points.
VAR_DOCS_PER_CHUNK = 600  # x (4 + a 300-byte row) = 182 400 bytes: beyond the LDS decode window
VAR_LAST_ROWS = 200       # the partial last chunk: 400 absent rows
VAR_LONG_ROW = 300


def cut_rows(data: bytes, rows: int, seed: int, long_row=VAR_LONG_ROW):
    """``data`` cut into ``rows`` rows at random points (some rows empty), one of them exactly ``long_row`` bytes."""
    rng = np.random.default_rng(seed)
    a = int(rng.integers(0, len(data) - long_row + 1))
    cuts = [int(x) for x in rng.integers(0, len(data) + 1, rows - 3)]
    cuts = sorted([x for x in cuts if not a < x < a + long_row] + [a, a + long_row])
    cuts += [len(data)] * (rows - 1 - len(cuts))  # (cuts that fell inside the long row: empty rows at the end)
    cuts = [0] + cuts + [len(data)]
    return [data[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]


def handmade_var_byte(codec, docs_per_chunk=VAR_DOCS_PER_CHUNK, last_rows=VAR_LAST_ROWS):
    """[(rows, ops)] per chunk of one hand-made raw STRING column: ASCII literals, the operation lists of
    handmade_ops behind the start-offset literal."""
    out = []
    lists = handmade_ops(codec, ascii_only=True)
    for k, ops in enumerate(lists):
        rows = cut_rows(model(ops), docs_per_chunk if k + 1 < len(lists) else last_rows, seed=k)
        head = var_byte_chunk(rows, docs_per_chunk)[:4 * docs_per_chunk]
        out.append((rows, [("L", head)] + ops))
    return out


# Rows for the library compressors (the HBM path of every codec): three chunks of 1000 with a partial last one
def long_string_rows(n=2500, seed=5):
    """Raw STRING rows with a 300-byte longest value: the empty string, multi-byte UTF-8, rows of period 1, 2 and
    3 (the last twice in a row: one match across two rows) and random letters that no match shortens."""
    rng = np.random.default_rng(seed)
    vocab = ["", "é", "naïve", "日本", "zz-top", "\U0001F600"] + [f"w{j}" for j in range(200)]
    rows = [vocab[i] for i in rng.integers(0, len(vocab), n)]
    letters = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    for base in range(0, n, 1000):  # in every chunk
        at = base + 37
        # (a short run first: after a long literal run liblz4 steps over several bytes at a time, and finds the
        # period of the row it lands in at a multiple of it)
        rows[at:at + 7] = ["q" * 40, "ab" * 150, "abc" * 100, "abc" * 100, "x" * 300, "",
                           bytes(letters[rng.integers(0, 52, 300)]).decode()]
    return rows


def word_rows(n, seed=8, words=3000):
    """Rows drawn from a few thousand distinct words of 2 to 30 bytes."""
    rng = np.random.default_rng(seed)
    vocab = ["".join(chr(c) for c in rng.integers(0x61, 0x7B, int(k))) for k in rng.integers(2, 31, words)]
    return [vocab[i] for i in rng.integers(0, words, n)]
