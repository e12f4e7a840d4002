"""REGEXP_LIKE patterns compiled to byte-level DFAs (host side, pure Python + numpy).

The reference evaluates REGEXP_LIKE with ``java.util.regex`` (PatternFactory's default JavaUtilPattern) and
``Matcher.reset(value).find()`` per value (RegexpLikePredicateEvaluatorFactory.java:74-76, 108-110). This module
restates the language of that ``find()`` for the constructs listed below as a DFA over the UTF-8 bytes of the value:

  pattern -> AST -> byte NFA (code-point sets expanded to UTF-8 byte-range sequences) -> subset construction ->
  minimisation -> byte equivalence classes.

``find()`` semantics are part of the automaton: unless an alternative starts with ``^`` it hangs off a start state
that loops on every byte (every construct starts on a lead byte, so skipping bytes equals skipping code points on
valid UTF-8), and unless it ends with ``$`` it runs into an absorbing accept state. A trailing ``$`` is "an optional
final line terminator, then the end of the input" (Pattern's Dollar node without MULTILINE / UNIX_LINES).

Supported: literals (non-ASCII ones as their UTF-8 bytes), escaped metacharacters, ``\\t \\n \\r \\f \\a \\e \\xhh
\\uhhhh``, ``.``, ``\\d \\w \\s \\D \\W \\S``, classes ``[...]`` / ``[^...]`` with ranges, escapes and the predefined
classes, groups ``(...)`` / ``(?:...)``, ``|``, greedy and lazy ``* + ? {n} {n,} {n,m}``, a leading ``(?i)`` (ASCII
folding: Java without UNICODE_CASE), ``^`` first and ``$`` last in the pattern or in a top-level alternative.
Everything else raises UnsupportedOnGpu naming the construct (the CPU plan maker answers the query); a malformed
pattern raises RegexSyntaxError (a ValueError, as the reference answers BadQueryRequestException).

Known difference: Java's ``$`` does not match between ``\\r`` and ``\\n``; here ``a\\r$`` finds in ``"a\\r\\n"``.
"""
from dataclasses import dataclass

import numpy as np

from .._lib import STRMATCH_MAX_STATES, STRMATCH_MAX_TABLE_BYTES, STRMATCH_VERSION, UnsupportedOnGpu

# the design caps of include/pinot_hip.h (PHIP_STRMATCH_*)
MAX_STATES = STRMATCH_MAX_STATES
MAX_TABLE_BYTES = STRMATCH_MAX_TABLE_BYTES
BLOB_VERSION = STRMATCH_VERSION
_BUILD_STATES = 4 * MAX_STATES  # subset construction gives up here: minimisation rarely shrinks a DFA fourfold
_MAX_NFA_STATES = 1 << 16
_MAX_REPEAT = 1000

_MAX_CP = 0x10FFFF
_TERMINATORS = (0x0A, 0x0D, 0x85, 0x2028, 0x2029)


class RegexSyntaxError(ValueError):
    """A malformed pattern (java.util.regex.PatternSyntaxException -> BadQueryRequestException)."""


# ----------------------------------------------------------------------------- code point sets
def _norm(ranges):
    """Sorted, merged, surrogate-free inclusive code point ranges."""
    out = []
    for lo, hi in sorted(ranges):
        for a, b in ((lo, min(hi, 0xD7FF)), (max(lo, 0xE000), hi)):
            if a > b:
                continue
            if out and a <= out[-1][1] + 1:
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
    return tuple((a, b) for a, b in out)


def _negate(ranges):
    out, nxt = [], 0
    for lo, hi in _norm(ranges):
        if lo > nxt:
            out.append((nxt, lo - 1))
        nxt = hi + 1
    if nxt <= _MAX_CP:
        out.append((nxt, _MAX_CP))
    return _norm(out)


def _fold_ascii(ranges):
    """(?i) without UNICODE_CASE: a-z and A-Z match each other."""
    out = list(ranges)
    for lo, hi in ranges:
        a, b = max(lo, 0x41), min(hi, 0x5A)
        if a <= b:
            out.append((a + 32, b + 32))
        a, b = max(lo, 0x61), min(hi, 0x7A)
        if a <= b:
            out.append((a - 32, b - 32))
    return _norm(out)


_DIGIT = ((0x30, 0x39),)
_WORD = ((0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A))
_SPACE = ((0x09, 0x0D), (0x20, 0x20))
_PREDEF = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _negate(_DIGIT), "W": _negate(_WORD), "S": _negate(_SPACE)}
_DOT = _negate(tuple((t, t) for t in _TERMINATORS))
_SIMPLE_ESCAPES = {"t": 0x09, "n": 0x0A, "r": 0x0D, "f": 0x0C, "a": 0x07, "e": 0x1B}


def _utf8_sequences(lo, hi):
    """[lo, hi] (no surrogates inside) -> sequences of inclusive byte ranges whose product is exactly the UTF-8
    encodings of the range."""
    out = []
    stack = [(lo, hi)]
    while stack:
        lo, hi = stack.pop()
        split = False
        for top in (0x7F, 0x7FF, 0xFFFF):
            if lo <= top < hi:
                stack.append((top + 1, hi))
                stack.append((lo, top))
                split = True
                break
        if split:
            continue
        if hi <= 0x7F:
            out.append(((lo, hi),))
            continue
        n = 2 if hi <= 0x7FF else 3 if hi <= 0xFFFF else 4
        for i in range(1, n):
            m = (1 << (6 * i)) - 1
            if (lo & ~m) != (hi & ~m):
                if lo & m:
                    stack.append(((lo | m) + 1, hi))
                    stack.append((lo, lo | m))
                    split = True
                    break
                if (hi & m) != m:
                    stack.append((hi & ~m, hi))
                    stack.append((lo, (hi & ~m) - 1))
                    split = True
                    break
        if split:
            continue
        a, b = chr(lo).encode("utf-8"), chr(hi).encode("utf-8")
        out.append(tuple(zip(a, b)))
    return out


# ----------------------------------------------------------------------------- parser
# AST: ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, min, max or None) | ("empty",)
class _PatternParser:
    def __init__(self, pattern):
        self.p = pattern
        self.i = 0
        self.icase = False
        self.depth = 0

    def peek(self, k=0):
        j = self.i + k
        return self.p[j] if j < len(self.p) else ""

    def parse(self):
        """-> [(anchored_start, node, anchored_end)] per top-level alternative."""
        if self.p.startswith("(?i)"):
            self.icase = True
            self.i = 4
        alts = []
        while True:
            bol = eol = False
            if self.peek() == "^":
                bol = True
                self.i += 1
            node, eol = self.sequence(top=True)
            alts.append((bol, node, eol))
            if self.peek() == "|":
                self.i += 1
                continue
            if self.peek() == ")":
                raise RegexSyntaxError(f"unmatched closing ')' at index {self.i} of {self.p!r}")
            assert self.i == len(self.p)
            return alts

    def alternation(self):
        alts = [self.sequence()[0]]
        while self.peek() == "|":
            self.i += 1
            alts.append(self.sequence()[0])
        return alts[0] if len(alts) == 1 else ("alt", alts)

    def sequence(self, top=False):
        items = []
        while True:
            c = self.peek()
            if c == "" or c == "|" or c == ")":
                break
            if c == "$":
                if top and self.peek(1) in ("", "|"):
                    self.i += 1
                    return self._cat(items), True
                raise UnsupportedOnGpu(f"'$' before the end of the pattern or of a top-level alternative in {self.p!r}")
            if c == "^":
                raise UnsupportedOnGpu(f"'^' after the start of the pattern or of a top-level alternative in {self.p!r}")
            if c in "*+?":
                raise RegexSyntaxError(f"dangling quantifier '{c}' at index {self.i} of {self.p!r}")
            if c == "{":
                raise RegexSyntaxError(f"illegal repetition at index {self.i} of {self.p!r}")
            items.append(self.quantified(self.atom()))
        return self._cat(items), False

    @staticmethod
    def _cat(items):
        if not items:
            return ("empty",)
        return items[0] if len(items) == 1 else ("cat", items)

    def quantified(self, node):
        c = self.peek()
        if c == "*":
            lo, hi = 0, None
            self.i += 1
        elif c == "+":
            lo, hi = 1, None
            self.i += 1
        elif c == "?":
            lo, hi = 0, 1
            self.i += 1
        elif c == "{":
            j = self.p.find("}", self.i)
            body = self.p[self.i + 1:j] if j > 0 else ""
            parts = body.split(",")
            if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()) \
                    or not body.isascii():
                raise RegexSyntaxError(f"illegal repetition at index {self.i} of {self.p!r}")
            lo = int(parts[0])
            hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
            if hi is not None and hi < lo:
                raise RegexSyntaxError(f"illegal repetition range at index {self.i} of {self.p!r}")
            if lo > _MAX_REPEAT or (hi or 0) > _MAX_REPEAT:
                raise UnsupportedOnGpu(f"a repetition count above {_MAX_REPEAT} in {self.p!r}")
            self.i = j + 1
        else:
            return node
        if self.peek() == "+":
            raise UnsupportedOnGpu(f"possessive quantifier at index {self.i} of {self.p!r}")
        if self.peek() == "?":  # lazy: the same language under a boolean find()
            self.i += 1
        if self.peek() and self.peek() in "*+?{":
            raise RegexSyntaxError(f"dangling quantifier '{self.peek()}' at index {self.i} of {self.p!r}")
        return ("rep", node, lo, hi)

    def lit(self, cp):
        r = ((cp, cp),)
        return ("set", _fold_ascii(r) if self.icase else r)

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.peek(1)
                if nxt == ":":
                    self.i += 2
                elif nxt in ("=", "!"):
                    raise UnsupportedOnGpu(f"look-ahead group in {self.p!r}")
                elif nxt == "<" and self.peek(2) in ("=", "!"):
                    raise UnsupportedOnGpu(f"look-behind group in {self.p!r}")
                elif nxt == "<":
                    raise UnsupportedOnGpu(f"named group in {self.p!r}")
                elif nxt == ">":
                    raise UnsupportedOnGpu(f"atomic group in {self.p!r}")
                else:
                    raise UnsupportedOnGpu(f"inline flag group other than a leading (?i) in {self.p!r}")
            self.depth += 1
            node = self.alternation()
            self.depth -= 1
            if self.peek() != ")":
                raise RegexSyntaxError(f"unclosed group in {self.p!r}")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            self.i += 1
            return ("set", _DOT)
        if c == "\\":
            kind, v = self.escape(in_class=False)
            if kind == "set":
                return ("set", _fold_ascii(v) if self.icase else v)
            return self.lit(v)
        self.i += 1
        cp = ord(c)
        if 0xD800 <= cp <= 0xDFFF:
            raise UnsupportedOnGpu(f"a lone surrogate in {self.p!r}")
        return self.lit(cp)

    def escape(self, in_class):
        """At a backslash: -> ("cp", code point) | ("set", ranges)."""
        self.i += 1
        c = self.peek()
        if c == "":
            raise RegexSyntaxError(f"trailing backslash in {self.p!r}")
        self.i += 1
        if c in _PREDEF:
            return "set", _PREDEF[c]
        if c in _SIMPLE_ESCAPES:
            return "cp", _SIMPLE_ESCAPES[c]
        if c == "x" or c == "u":
            n = 2 if c == "x" else 4
            h = self.p[self.i:self.i + n]
            if c == "x" and self.peek() == "{":
                raise UnsupportedOnGpu(f"\\x{{...}} escape in {self.p!r}")
            if len(h) != n or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                raise RegexSyntaxError(f"illegal \\{c} escape in {self.p!r}")
            self.i += n
            cp = int(h, 16)
            if 0xD800 <= cp <= 0xDFFF:
                raise UnsupportedOnGpu(f"a surrogate \\u escape in {self.p!r}")
            return "cp", cp
        if c in "bBAzZG":
            raise UnsupportedOnGpu(f"boundary matcher \\{c} in {self.p!r}")
        if c in "pP":
            raise UnsupportedOnGpu(f"\\{c}{{..}} property / POSIX class in {self.p!r}")
        if c in "123456789" or c == "k":
            raise UnsupportedOnGpu(f"backreference \\{c} in {self.p!r}")
        if c in "QE":
            raise UnsupportedOnGpu(f"\\Q..\\E quotation in {self.p!r}")
        if c in "hHvVRXN0c":
            raise UnsupportedOnGpu(f"escape \\{c} in {self.p!r}")
        if c.isascii() and c.isalpha():
            raise RegexSyntaxError(f"illegal escape \\{c} in {self.p!r}")
        cp = ord(c)
        if 0xD800 <= cp <= 0xDFFF:
            raise UnsupportedOnGpu(f"a lone surrogate in {self.p!r}")
        return "cp", cp

    def char_class(self):
        self.i += 1  # [
        neg = False
        if self.peek() == "^":
            neg = True
            self.i += 1
        ranges = []
        first = True
        while True:
            c = self.peek()
            if c == "":
                raise RegexSyntaxError(f"unclosed character class in {self.p!r}")
            if c == "]" and not first:
                self.i += 1
                break
            if c == "]":
                raise RegexSyntaxError(f"empty or unclosed character class in {self.p!r}")
            first = False
            if c == "[":
                raise UnsupportedOnGpu(f"nested character class (or POSIX class) in {self.p!r}")
            if c == "&" and self.peek(1) == "&":
                raise UnsupportedOnGpu(f"class intersection '&&' in {self.p!r}")
            if c == "\\":
                kind, v = self.escape(in_class=True)
                if kind == "set":
                    ranges.extend(v)
                    continue
                lo = v
            else:
                lo = ord(c)
                self.i += 1
            if self.peek() == "-" and self.peek(1) not in ("]", ""):
                if self.peek(1) == "[":
                    raise UnsupportedOnGpu(f"nested character class (or POSIX class) in {self.p!r}")
                self.i += 1
                if self.peek() == "\\":
                    kind, hi = self.escape(in_class=True)
                    if kind == "set":
                        raise RegexSyntaxError(f"illegal character range in {self.p!r}")
                else:
                    hi = ord(self.peek())
                    self.i += 1
                if hi < lo:
                    raise RegexSyntaxError(f"illegal character range in {self.p!r}")
                ranges.append((lo, hi))
            else:
                ranges.append((lo, lo))
        r = _norm(ranges)
        if self.icase:
            r = _fold_ascii(r)
        return ("set", _negate(r) if neg else r)


# ----------------------------------------------------------------------------- NFA
class _Nfa:
    def __init__(self):
        self.eps = []
        self.trans = []  # per state: [(lo byte, hi byte, target)]

    def state(self):
        if len(self.eps) >= _MAX_NFA_STATES:
            raise UnsupportedOnGpu(f"a pattern whose NFA exceeds {_MAX_NFA_STATES} states")
        self.eps.append([])
        self.trans.append([])
        return len(self.eps) - 1

    def build(self, node, s):
        """Adds node's fragment after state s; -> its end state."""
        k = node[0]
        if k == "empty":
            return s
        if k == "set":
            e = self.state()
            tails = {}  # shared suffix states keep the sets of . and negated classes small
            for lo, hi in node[1]:
                for seq in _utf8_sequences(lo, hi):
                    cur = s
                    for j, (a, b) in enumerate(seq):
                        if j == len(seq) - 1:
                            self.trans[cur].append((a, b, e))
                        else:
                            key = (cur, a, b)
                            nxt = tails.get(key)
                            if nxt is None:
                                nxt = tails[key] = self.state()
                                self.trans[cur].append((a, b, nxt))
                            cur = nxt
            return e
        if k == "cat":
            for n in node[1]:
                s = self.build(n, s)
            return s
        if k == "alt":
            e = self.state()
            for n in node[1]:
                b = self.state()
                self.eps[s].append(b)
                self.eps[self.build(n, b)].append(e)
            return e
        if k == "rep":
            _, n, lo, hi = node
            for _ in range(lo):
                s = self.build(n, s)
            if hi is None:
                b = self.state()
                self.eps[s].append(b)
                x = self.build(n, b)
                e = self.state()
                self.eps[x].append(b)
                self.eps[b].append(e)
                return e
            e = self.state()
            self.eps[s].append(e)
            for _ in range(hi - lo):
                b = self.state()
                self.eps[s].append(b)
                s = self.build(n, b)
                self.eps[s].append(e)
            return e
        raise AssertionError(k)


@dataclass
class Dfa:
    """A complete DFA over bytes: state x byte class -> state. ``accept`` is read after the last byte of a value."""
    num_states: int
    num_classes: int
    start: int
    accept: np.ndarray     # bool[S]
    class_map: np.ndarray  # uint8[256]
    trans: np.ndarray      # uint16[S, C]

    def to_blob(self) -> np.ndarray:
        """The int32 words of include/pinot_hip.h's "DFA blob"."""
        S, C = self.num_states, self.num_classes
        acc = np.zeros((S + 31) // 32 * 32, dtype=np.uint8)
        acc[:S] = self.accept
        acc_words = np.packbits(acc.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
        t = np.zeros((S * C + 1) // 2 * 2, dtype="<u2")
        t[:S * C] = self.trans.reshape(-1)
        return np.concatenate([np.array([BLOB_VERSION, S, C, self.start], dtype=np.int32), acc_words.view(np.int32),
                               self.class_map.astype(np.uint8).view("<i4"), t.view("<i4")]).astype(np.int32)

    @staticmethod
    def from_blob(words) -> "Dfa":
        w = np.ascontiguousarray(words, dtype=np.int32)
        if len(w) < 4 or w[0] != BLOB_VERSION:
            raise ValueError("not a DFA blob of this version")
        S, C, start = int(w[1]), int(w[2]), int(w[3])
        aw = (S + 31) // 32
        if S < 1 or C < 1 or C > 256 or len(w) != 4 + aw + 64 + (S * C + 1) // 2:
            raise ValueError("DFA blob of the wrong size")
        acc = np.unpackbits(w[4:4 + aw].view(np.uint8), bitorder="little")[:S].astype(bool)
        cmap = w[4 + aw:4 + aw + 64].view(np.uint8).copy()
        trans = w[4 + aw + 64:].view("<u2")[:S * C].reshape(S, C).copy()
        return Dfa(S, C, start, acc, cmap, trans)

    def match_many(self, values, lengths=None) -> np.ndarray:
        """bool per value. ``values``: a list of str / bytes, or a uint8 matrix [n, width] of zero-padded rows (a
        fixed-width dictionary: a row's value ends at its first 0 byte, as the reference's readUnpaddedBytes), or
        such a matrix with explicit ``lengths``."""
        if not isinstance(values, np.ndarray):
            vals = [v.encode("utf-8") if isinstance(v, str) else bytes(v) for v in values]
            lengths = np.array([len(v) for v in vals], dtype=np.int64)
            width = int(lengths.max()) if len(vals) else 0
            mat = np.zeros((len(vals), max(width, 1)), dtype=np.uint8)
            for i, v in enumerate(vals):
                mat[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
        else:
            mat = values.reshape(len(values), -1).view(np.uint8) if values.dtype != np.uint8 else values
            if lengths is None:
                zero = mat == 0
                lengths = np.where(zero.any(axis=1), zero.argmax(axis=1), mat.shape[1])
        n = mat.shape[0]
        state = np.full(n, self.start, dtype=np.int64)
        flat = self.trans.reshape(-1).astype(np.int64)
        cmap = self.class_map.astype(np.int64)
        C = self.num_classes
        for j in range(int(np.max(lengths)) if n else 0):
            nxt = flat[state * C + cmap[mat[:, j]]]
            state = np.where(j < lengths, nxt, state)
        return self.accept[state]


def _minimise(trans, accept, start):
    """Moore partition refinement; -> (trans, accept, start) over the blocks."""
    block = accept.astype(np.int64)
    nblocks = len(np.unique(block))
    while True:
        sig = np.concatenate([block[:, None], block[trans]], axis=1)
        _, block = np.unique(sig, axis=0, return_inverse=True)
        block = block.reshape(-1)
        n = int(block.max()) + 1
        if n == nblocks:
            break
        nblocks = n
    rep = np.zeros(nblocks, dtype=np.int64)
    rep[block] = np.arange(len(block))
    return block[trans[rep]], accept[rep], int(block[start])


_CACHE = {}


def compile_pattern(pattern: str) -> Dfa:
    """java.util.regex pattern -> Dfa with find() semantics. Raises RegexSyntaxError / UnsupportedOnGpu."""
    hit = _CACHE.get(pattern)
    if hit is not None:
        return hit
    alts = _PatternParser(pattern).parse()
    nfa = _Nfa()
    start = nfa.state()
    loop = nfa.state()      # the unanchored prefix: any bytes
    nfa.eps[start].append(loop)
    nfa.trans[loop].append((0, 255, loop))
    sink = nfa.state()      # absorbing accept of an alternative without $
    nfa.trans[sink].append((0, 255, sink))
    final = nfa.state()     # accept at the end of the input
    for bol, node, eol in alts:
        b = nfa.state()
        nfa.eps[start if bol else loop].append(b)
        e = nfa.build(node, b)
        if not eol:
            nfa.eps[e].append(sink)
            continue
        nfa.eps[e].append(final)
        cr = nfa.state()    # \r, then the end or \n
        nfa.trans[e].append((0x0D, 0x0D, cr))
        nfa.eps[cr].append(final)
        nfa.trans[cr].append((0x0A, 0x0A, final))
        nfa.trans[e].append((0x0A, 0x0A, final))
        for seq in (b"\xc2\x85", b"\xe2\x80\xa8", b"\xe2\x80\xa9"):
            cur = e
            for j, byte in enumerate(seq):
                nxt = final if j == len(seq) - 1 else nfa.state()
                nfa.trans[cur].append((byte, byte, nxt))
                cur = nxt
    n = len(nfa.eps)
    # preliminary byte classes: the cuts of every transition's range
    cut = np.zeros(257, dtype=bool)
    cut[0] = True
    for tr in nfa.trans:
        for lo, hi, _ in tr:
            cut[lo] = True
            cut[hi + 1] = True
    cmap0 = (np.cumsum(cut[:256]) - 1).astype(np.int64)
    C0 = int(cmap0[-1]) + 1
    # epsilon closures as bit masks
    closure = [0] * n
    for s in range(n):
        seen, stack = 1 << s, [s]
        while stack:
            for t in nfa.eps[stack.pop()]:
                if not (seen >> t) & 1:
                    seen |= 1 << t
                    stack.append(t)
        closure[s] = seen
    move = [[0] * C0 for _ in range(n)]
    for s in range(n):
        for lo, hi, t in nfa.trans[s]:
            for c in range(int(cmap0[lo]), int(cmap0[hi]) + 1):
                move[s][c] |= closure[t]
    accept_mask = (1 << sink) | (1 << final)
    ids = {closure[start]: 0}
    order = [closure[start]]
    rows = []
    k = 0
    while k < len(order):
        m = order[k]
        k += 1
        acc = [0] * C0
        while m:
            low = m & -m
            mv = move[low.bit_length() - 1]
            for c in range(C0):
                acc[c] |= mv[c]
            m ^= low
        row = []
        for c in range(C0):
            t = ids.get(acc[c])
            if t is None:
                if len(order) >= _BUILD_STATES:
                    raise UnsupportedOnGpu(f"pattern {pattern!r}: a DFA of more than {_BUILD_STATES} states before "
                                           f"minimisation (the cap is {MAX_STATES} states)")
                t = ids[acc[c]] = len(order)
                order.append(acc[c])
            row.append(t)
        rows.append(row)
    trans = np.asarray(rows, dtype=np.int64).reshape(len(order), C0)
    accept = np.array([(m & accept_mask) != 0 for m in order], dtype=bool)
    trans, accept, st = _minimise(trans, accept, 0)
    # byte equivalence classes of the minimal DFA: identical columns of the 256-wide table
    wide = trans[:, cmap0]                               # [S, 256]
    _, first, inv = np.unique(wide.T, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    rank = np.argsort(np.argsort(first))                 # classes numbered by their first byte
    class_map = rank[inv].astype(np.uint8)
    C = int(class_map.max()) + 1
    cols = np.zeros(C, dtype=np.int64)
    cols[class_map[::-1]] = np.arange(255, -1, -1)       # a byte of each class
    S = trans.shape[0]
    if S > MAX_STATES or S * C * 2 > MAX_TABLE_BYTES:
        raise UnsupportedOnGpu(f"pattern {pattern!r}: a DFA of {S} states x {C} byte classes, over the cap of "
                               f"{MAX_STATES} states / {MAX_TABLE_BYTES} table bytes")
    dfa = Dfa(S, C, st, accept, class_map, wide[:, cols].astype(np.uint16))
    if len(_CACHE) < 256:
        _CACHE[pattern] = dfa
    return dfa
