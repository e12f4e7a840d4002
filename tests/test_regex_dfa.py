"""The pattern compiler (pinot_amd/query/regex_dfa.py) against an independent matcher (tests/strmatch_ref.py: Python's
re under re.ASCII, for inputs free of the terminators only Java knows) and a hand-written table of Java's answers for
the rest: a fixed pattern list with every supported construct, a seeded property test, the blob round trip, the caps,
and the reference's own query counts."""
import json
import os
import random

import numpy as np
import pytest

from pinot_amd._lib import UnsupportedOnGpu
from pinot_amd.query import regex_dfa
from pinot_amd.query.sql import like_to_regexp_like
from tests import strmatch_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "regexp_like_queries.json")) as _f:
    QUERIES = json.load(_f)

E, EMOJI = "\u00e9", "\U0001F600"

# one or more per supported construct; the reference tests' patterns and LIKE conversions are appended below
FIXED_PATTERNS = [
    "abc", "^abc", "abc$", "^abc$", "", "^", "$", "^$",            # literals, anchors, the empty pattern
    "a.c", "^.$", "^..$", ".*", ".+x", "^.*$",                      # dot
    "a|b", "^a|b$", "abc|^x|y$|", "(a|b)c", "(?:ab|cd)+e", "()a",    # alternation, groups
    "ab*c", "ab+c", "ab?c", "a{2}", "a{2,}", "a{1,3}b", "(ab){2,3}", "a{0}b", "a{0,0}",   # greedy quantifiers
    "ab*?c", "ab+?c", "ab??c", "a{1,3}?b",                           # lazy ones: the same language
    "[abc]", "[^abc]", "[a-c]x", "[^a-c]x", "[a-cx-z]+", "[-a]", "[a-]", "[\\]]", "[\\\\]", "[.]", "[^\\n]x", "[a^]",
    "[\\d_]+", "[^\\w]", "[\\s,]", "[\\t-\\r]", "[\\x41-\\x43]", "[\\u00e0-\\u00ff]", "[" + E + "x]", "[^" + E + "]",
    "\\d+", "\\D", "\\w+@\\w+", "\\W", "\\s", "\\S+", "^\\d{3}-\\d{4}$",
    "\\.", "\\*\\+\\?", "\\(\\)", "\\[\\]", "\\{\\}", "\\|", "\\^\\$", "\\\\", "\\/", "\\-", "\\&", "\\<\\>", "\\_", "\\%",
    "\\t", "\\n", "a\\nb", "\\x41", "\\u00e9", "\\u0041b", "\\f|\\a",
    E, "a" + E + "c", E + "+", "caf" + E + "$", EMOJI, "^" + EMOJI + "+$", "[" + EMOJI + "]",
    "(?i)abc", "(?i)[a-c]+z", "(?i)^AbC$", "(?i)[^a]", "(?i)" + E,
    "}", "]", "a]b", "a}b",                                          # literal outside their construct, as in Java
    "x*", "(a*)*b", "(a|b)*abb", "(a+)+$", "^(a|ab)(c|bcd)(d*)$",
]
FIXED_PATTERNS += QUERIES["patterns"] + [like_to_regexp_like(p) for p in QUERIES["like_patterns"]]
FIXED_PATTERNS = list(dict.fromkeys(FIXED_PATTERNS))

CORPUS = ["", "a", "b", "c", "ab", "abc", "abcd", "xabc", "abcx", "aabbcc", "abb", "aabb", "ababab", "abab", "cd", "abcd",
          "ac", "abbbc", "a\nc", "abc\n", "abc\n\n", "\nabc", "\n", "a b", " ", "\t", "a\tb", "x\ny", "\f", "\x07", "\x1b",
          "ABC", "aBc", "Abcz", "ABZ", "AZ", "0", "123", "12a", "555-1234", "5555-1234", "_", "a_b", "x@y", "-", "a-", "^", "a^",
          "$", "^$", ".", "*+?", "()", "[]", "{}", "|", "\\", "/", "&", "<>", "%", "]", "}", "a]b", "a}b", ",", "a,b",
          E, "a" + E + "c", E + E, "caf" + E, "caf" + E + "\n", "cafe", "\u00c9", "\u00e0", "\u00ff", "\u0100", "\u07ff", "\u0800",
          "\uffff", EMOJI, EMOJI + EMOJI, "a" + EMOJI + "c", "\U00010000", "\U0010ffff", "\ud7ff", "\ue000", "\u20ac",
          "A", "Ab", "aaa", "aaaa", "aab", "b" * 7, "a" * 9 + "b", "aae", "abe", "abcde", "cdcde",
          "www.domain1.com", "www.sd.domain1.co.ab", "www.domain2.com/a", "wwwxdomain1ycom", "test1", "test12", "xtest1"]
CORPUS += QUERIES["domain_names"] + [d + s for d in QUERIES["domain_names"][:4] for s in QUERIES["url_suffixes"]]
CORPUS = list(dict.fromkeys(CORPUS))


def test_fixed_list_covers_enough():
    assert len(FIXED_PATTERNS) >= 40
    for p in QUERIES["patterns"]:
        assert p in FIXED_PATTERNS


@pytest.mark.parametrize("pattern", FIXED_PATTERNS, ids=[repr(p) for p in FIXED_PATTERNS])
def test_fixed_patterns_against_reference_matcher(pattern):
    dfa = regex_dfa.compile_pattern(pattern)
    got = dfa.match_many(CORPUS)
    want = strmatch_ref.match_many(pattern, CORPUS)
    bad = [(v, w) for v, g, w in zip(CORPUS, got.tolist(), want) if g != w]
    assert not bad, (pattern, bad[:5])
    # the str and the bytes form of a value walk the same bytes
    assert np.array_equal(got, dfa.match_many([v.encode("utf-8") for v in CORPUS]))


def test_java_known_answers():
    for pattern, value, want in strmatch_ref.JAVA_KNOWN_ANSWERS:
        got = bool(regex_dfa.compile_pattern(pattern).match_many([value])[0])
        assert got == want, (pattern, value, want)


def test_reference_matcher_agrees_where_both_apply():
    """The hand-written Java table and the re-based matcher say the same on the inputs the latter is valid for."""
    n = 0
    for pattern, value, want in strmatch_ref.JAVA_KNOWN_ANSWERS:
        if strmatch_ref.valid_for(value):
            assert strmatch_ref.matches(pattern, value) == want, (pattern, value)
            n += 1
    assert n >= 8


# ---- seeded property test -------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "c", E]


def _atom(rng, depth):
    k = rng.randrange(7 if depth > 0 else 5)
    if k < 2:
        return rng.choice(ALPHABET)
    if k == 2:
        return "."
    if k == 3:
        return "[ab]"
    if k == 4:
        return "[^a]"
    if k == 5:
        return "(" + _alt(rng, depth - 1) + ")"
    return "(?:" + _seq(rng, depth - 1) + ")"


def _piece(rng, depth):
    a = _atom(rng, depth)
    # * and + only over one character: a backtracking matcher (the reference one) takes exponential time on nested
    # unbounded repeats, a DFA does not care
    q = rng.choice(["", "", "", "*", "+", "?", "{1,2}"] if len(a) == 1 or a[0] == "[" else ["", "", "?", "{1,2}"])
    return a + q


def _seq(rng, depth):
    return "".join(_piece(rng, depth) for _ in range(rng.randrange(1, 3)))


def _alt(rng, depth):
    return "|".join(_seq(rng, depth) for _ in range(rng.randrange(1, 3)))


def random_pattern(rng):
    """Depth <= 3 over {a, b, c, e-acute} with . | * + ? {1,2} [ab] [^a]; ^ and $ only where the compiler takes them:
    first / last in a top-level alternative."""
    alts = []
    for _ in range(rng.randrange(1, 3)):
        s = _seq(rng, 3) + _seq(rng, 2)
        if rng.random() < 0.3:
            s = "^" + s
        if rng.random() < 0.3:
            s = s + "$"
        alts.append(s)
    return "|".join(alts)


def random_string(rng):
    n = rng.randrange(0, 13)
    return "".join(rng.choice(ALPHABET + ["\n"]) if rng.random() < 0.97 else "d" for _ in range(n))


def test_random_patterns_against_reference_matcher():
    rng = random.Random(20240607)
    refused, checked = [], 0
    for _ in range(500):
        pattern = random_pattern(rng)
        values = [random_string(rng) for _ in range(200)]
        try:
            dfa = regex_dfa.compile_pattern(pattern)
        except UnsupportedOnGpu as e:
            refused.append((pattern, str(e)))
            continue
        got = dfa.match_many(values).tolist()
        want = strmatch_ref.match_many(pattern, values)
        bad = [(v, w) for v, g, w in zip(values, got, want) if g != w]
        assert not bad, (pattern, bad[:5])
        checked += 1
    assert not refused, refused[:3]   # the generator stays inside the supported subset: nothing is skipped
    assert checked == 500


# ---- the automaton --------------------------------------------------------------------------------------------------
def test_dfa_shape_and_find_semantics():
    d = regex_dfa.compile_pattern("abc")
    assert d.trans.shape == (d.num_states, d.num_classes) and d.trans.dtype == np.uint16
    assert d.class_map.shape == (256,) and int(d.class_map.max()) == d.num_classes - 1
    assert d.accept.shape == (d.num_states,) and 0 <= d.start < d.num_states
    assert d.num_states == 4 and d.num_classes == 4   # minimal: progress 0..2 and the absorbing accept; a, b, c, other
    absorbing = [s for s in range(d.num_states) if (d.trans[s] == s).all()]
    assert len(absorbing) == 1 and d.accept[absorbing[0]]          # not $-anchored: accepting is forever
    assert not d.accept[d.start]
    d = regex_dfa.compile_pattern("^abc$")
    dead = [s for s in range(d.num_states) if (d.trans[s] == s).all()]
    assert len(dead) == 1 and not d.accept[dead[0]]                 # anchored: a dead state, no absorbing accept
    assert regex_dfa.compile_pattern("").num_states == 1           # LIKE '%': everything matches
    # \\e is Java's escape character; Python's re has no such escape
    assert regex_dfa.compile_pattern("a\\eb").match_many(["a\x1bb", "aeb"]).tolist() == [True, False]


def test_match_many_over_a_padded_dictionary_matrix():
    vals = ["", "ab", "abc", "abcd", "xabc", "caf" + E]
    enc = [v.encode("utf-8") for v in vals]
    width = max(len(e) for e in enc)
    mat = np.frombuffer(b"".join(e + b"\0" * (width - len(e)) for e in enc), dtype=np.uint8).reshape(len(vals), width)
    for pattern in ("abc", "^abc$", "c$", "^$", E + "$", "^.{5}$"):
        want = strmatch_ref.match_many(pattern, vals)
        assert regex_dfa.compile_pattern(pattern).match_many(mat).tolist() == want, pattern


def test_blob_round_trip():
    for pattern in ("abc", "^a.c$", "(?i)[a-c]+z$", "\\w+@\\w+", "", E + "|" + EMOJI):
        d = regex_dfa.compile_pattern(pattern)
        blob = d.to_blob()
        S, C = d.num_states, d.num_classes
        assert blob.dtype == np.int32
        assert blob[:4].tolist() == [regex_dfa.BLOB_VERSION, S, C, d.start]
        assert len(blob) == 4 + (S + 31) // 32 + 64 + (S * C + 1) // 2
        back = regex_dfa.Dfa.from_blob(blob)
        assert (back.num_states, back.num_classes, back.start) == (S, C, d.start)
        assert np.array_equal(back.accept, d.accept) and np.array_equal(back.class_map, d.class_map)
        assert np.array_equal(back.trans, d.trans)
        assert np.array_equal(back.match_many(CORPUS), d.match_many(CORPUS))
    with pytest.raises(ValueError):
        regex_dfa.Dfa.from_blob(blob[:-1])


def test_caps():
    with pytest.raises(UnsupportedOnGpu, match="states"):
        regex_dfa.compile_pattern("(a|b)*a(a|b){14}")     # 2^15 states
    d = regex_dfa.compile_pattern("(a|b)*a(a|b){8}$")     # the last nine characters: 2^9 states, inside
    assert 512 <= d.num_states <= regex_dfa.MAX_STATES
    assert d.num_states * d.num_classes * 2 <= regex_dfa.MAX_TABLE_BYTES
    with pytest.raises(UnsupportedOnGpu, match="3447 states x 22 byte classes"):   # inside the states, over the bytes
        regex_dfa.compile_pattern("|".join(f"{c}.{{3}}{c}" for c in "abcde"))


# ---- the reference's query counts -----------------------------------------------------------------------------------
def _rows():
    n = QUERIES["num_rows"]
    dn, us, ni = QUERIES["domain_names"], QUERIES["url_suffixes"], QUERIES["no_index_values"]
    dom = [dn[i % len(dn)] for i in range(n)]
    return {"INT_COL": [QUERIES["int_base"] + i for i in range(n)], "DOMAIN_NAMES": dom,
            "URL_COL": [dom[i] + us[i % len(us)] for i in range(n)], "NO_INDEX_COL": [ni[i % len(ni)] for i in range(n)]}


def _filter_mask(where, rows, match):
    """The golden filters: [NOT] REGEXP_LIKE(col, 'p') | col [NOT] LIKE 'p'."""
    from pinot_amd.query.sql import parse
    f = parse(f"SELECT COUNT(*) FROM t WHERE {where}").filter
    neg = f.type == "NOT"
    p = (f.children[0] if neg else f).predicate
    m = np.asarray(match(p.values[0], rows[p.column]), dtype=bool)
    return ~m if neg else m


@pytest.mark.parametrize("which", ["reference_matcher", "dfa"])
def test_golden_counts_on_the_host(which):
    rows = _rows()
    match = strmatch_ref.match_many if which == "reference_matcher" else \
        (lambda p, vals: regex_dfa.compile_pattern(p).match_many(vals))
    assert len(QUERIES["counts"]) == 20
    for where, count in QUERIES["counts"]:
        assert int(_filter_mask(where, rows, match).sum()) == count, where
    sel = QUERIES["selection"]
    m = _filter_mask(sel["filter"], rows, match)
    got = [[rows["INT_COL"][i], rows["URL_COL"][i]] for i in np.flatnonzero(m)[:sel["limit"]]]
    assert got == sel["rows"]
