"""LIKE / REGEXP_LIKE in the query layer: the LIKE conversion against the reference's own test vectors, the parser
shapes, and what the pattern compiler refuses (each refusal names its construct) or rejects as malformed."""
import json
import os

import pytest

from pinot_amd._lib import UnsupportedOnGpu
from pinot_amd.query import regex_dfa
from pinot_amd.query.context import PredicateType
from pinot_amd.query.sql import SqlError, like_to_regexp_like, parse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_like_to_regexp_like_golden():
    with open(os.path.join(GOLDEN, "like_to_regexp.json")) as f:
        pairs = json.load(f)["pairs"]
    assert len(pairs) == 17
    for like, want in pairs:
        assert like_to_regexp_like(like) == want, like


def test_like_to_regexp_like_edges():
    # RegexpPatternConverterUtils.java:48-73: the length switch
    assert like_to_regexp_like("") == "^$"
    assert like_to_regexp_like("%") == ""
    assert like_to_regexp_like("%%%") == ""
    assert like_to_regexp_like("_") == "^.$"
    assert like_to_regexp_like("a") == "^a$"
    assert like_to_regexp_like("a%b") == "^a.*b$"
    for c in "^$.{}[]()*+?|<>-&/":
        assert like_to_regexp_like(c + "x") == "^\\" + c + "x$", c
    assert like_to_regexp_like("\\") == "^\\\\$"
    assert like_to_regexp_like("a\\") == "^a\\\\$"


def _pred(fc):
    assert fc.type == "PREDICATE", fc
    return fc.predicate


def test_parser_regexp_like():
    q = parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(url, '.*/a')")
    p = _pred(q.filter)
    assert p.type == PredicateType.REGEXP_LIKE and p.column == "url" and p.values == (".*/a",)
    q = parse("SELECT COUNT(*) FROM t WHERE regexp_like(url, 'it''s')")
    assert _pred(q.filter).values == ("it's",)


def test_parser_like_and_not_like():
    p = _pred(parse("SELECT COUNT(*) FROM t WHERE url LIKE 'www.do_ai%'").filter)
    assert p.type == PredicateType.REGEXP_LIKE and p.column == "url" and p.values == ("^www\\.do.ai",)
    f = parse("SELECT COUNT(*) FROM t WHERE url NOT LIKE '%com'").filter
    assert f.type == "NOT" and _pred(f.children[0]).values == ("com$",)
    f = parse("SELECT COUNT(*) FROM t WHERE NOT REGEXP_LIKE(url, 'x')").filter
    assert f.type == "NOT" and _pred(f.children[0]).values == ("x",)


def test_parser_boolean_shapes():
    f = parse("SELECT COUNT(*) FROM t WHERE (a LIKE 'x%' OR REGEXP_LIKE(b, 'y')) AND c BETWEEN 1 AND 2").filter
    assert f.type == "AND" and f.children[0].type == "OR"
    assert [_pred(c).type for c in f.children[0].children] == ["REGEXP_LIKE", "REGEXP_LIKE"]
    f = parse("SELECT COUNT(*) FROM t WHERE (REGEXP_LIKE(b, 'y'))").filter
    assert _pred(f).column == "b"
    f = parse("SELECT COUNT(*) FROM t WHERE (a LIKE 'x')").filter
    assert _pred(f).values == ("^x$",)
    f = parse("SELECT COUNT(*) FROM t WHERE NOT (a LIKE 'x' AND b = 1)").filter
    assert f.type == "NOT" and f.children[0].type == "AND"


def test_parser_filter_clause_and_case():
    q = parse("SELECT COUNT(*) FILTER(WHERE c LIKE 'a%'), SUM(x) FILTER(WHERE REGEXP_LIKE(c, 'b$')) FROM t")
    flts = [a.filter for a in q.aggregations]
    assert [_pred(f).values[0] for f in flts] == ["^a", "b$"]
    q = parse("SELECT SUM(CASE WHEN c LIKE 'a%' THEN 1 WHEN REGEXP_LIKE(c, 'z') THEN 2 ELSE 0 END) FROM t")
    case = q.aggregations[0].argument
    assert case.name == "case"
    assert _pred(case.args[0]).values == ("^a",) and _pred(case.args[2]).values == ("z",)


def test_parser_errors():
    with pytest.raises(SqlError):
        parse("SELECT COUNT(*) FROM t WHERE a LIKE 5")
    with pytest.raises(SqlError):
        parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(a)")
    with pytest.raises(SqlError):
        parse("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(a, b)")
    with pytest.raises(SqlError):
        parse("SELECT COUNT(*) FROM t WHERE a NOT = 'x'")


def test_pattern_on_expression_is_unsupported():
    p = _pred(parse("SELECT COUNT(*) FROM t WHERE upper(a) LIKE 'X%'").filter)
    with pytest.raises(UnsupportedOnGpu, match="expression"):
        p.column


REFUSED = [
    ("a*+", "possessive"), ("a++b", "possessive"), ("a?+", "possessive"), ("a{2}+", "possessive"),
    ("(a)\\1", "backreference"), ("(?<n>a)\\k<n>", "named group"),
    ("(?=a)b", "look-ahead"), ("(?!a)b", "look-ahead"), ("(?<=a)b", "look-behind"), ("(?<!a)b", "look-behind"),
    ("(?>a)b", "atomic"),
    ("\\bfoo", "\\\\b"), ("foo\\B", "\\\\B"), ("\\Afoo", "\\\\A"), ("foo\\z", "\\\\z"), ("foo\\Z", "\\\\Z"), ("\\Gfoo", "\\\\G"),
    ("\\p{Alpha}", "property"), ("\\P{L}x", "property"), ("[[:alpha:]]", "nested"),
    ("[a-z&&[^b]]", "intersection"), ("[a[bc]]", "nested"),
    ("a(?i)b", "inline flag"), ("(?s)a.b", "inline flag"), ("(?i:a)b", "inline flag"), ("(?m)^a", "inline flag"),
    ("a^b", "'\\^'"), ("(^a)", "'\\^'"), ("a$b", "'\\$'"), ("(a$)", "'\\$'"), ("a|(b$)", "'\\$'"),
    ("\\Qa.b\\E", "quotation"), ("a\\Rb", "escape"),
    ("(a|b)*a(a|b){14}", "states"),
]


@pytest.mark.parametrize("pattern,names", REFUSED, ids=[p for p, _ in REFUSED])
def test_refused_constructs_name_themselves(pattern, names):
    with pytest.raises(UnsupportedOnGpu, match=names):
        regex_dfa.compile_pattern(pattern)


MALFORMED = ["(a", "a)", "(a))", "*a", "a**", "+", "a|*", "?", "a{", "a{x}", "a{2,1}", "{2}", "[a", "[", "[]", "[z-a]", "a\\",
             "\\q", "\\x4", "\\u12", "(?:a"]


@pytest.mark.parametrize("pattern", MALFORMED)
def test_malformed_patterns_are_value_errors(pattern):
    with pytest.raises(ValueError) as e:
        regex_dfa.compile_pattern(pattern)
    assert isinstance(e.value, regex_dfa.RegexSyntaxError)
    assert not isinstance(e.value, UnsupportedOnGpu)


def test_caps_mirror_the_header():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pinot_hip.h")).read()
    from pinot_amd import _lib
    assert f"#define PHIP_STRMATCH_MAX_STATES {_lib.STRMATCH_MAX_STATES}\n" in hdr
    assert f"#define PHIP_STRMATCH_MAX_TABLE_BYTES {_lib.STRMATCH_MAX_TABLE_BYTES}\n" in hdr
    assert f"#define PHIP_STRMATCH_VERSION {_lib.STRMATCH_VERSION}\n" in hdr
    assert f"#define PHIP_LEAF_RAW_STRING_MATCH {_lib.LEAF_RAW_STRING_MATCH}\n" in hdr
    assert f"#define PHIP_LEAF_FLAG_ALWAYS_SCAN {_lib.LEAF_FLAG_ALWAYS_SCAN}\n" in hdr
    assert (regex_dfa.MAX_STATES, regex_dfa.MAX_TABLE_BYTES) == (_lib.STRMATCH_MAX_STATES, _lib.STRMATCH_MAX_TABLE_BYTES)
