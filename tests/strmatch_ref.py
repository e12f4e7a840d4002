"""An independent REGEXP_LIKE matcher for the string-match tests: Python's ``re`` with ``re.ASCII``.

``re.search`` under ``re.ASCII`` has the language of ``java.util.regex``'s ``find()`` for the supported constructs as
long as the INPUT holds none of ``\\r \\u0085 \\u2028 \\u2029``: the two differ only in which line terminators ``.``
excludes and ``$`` steps over (Python: ``\\n`` alone). Inputs with those characters are covered by JAVA_KNOWN_ANSWERS,
a hand-written table of what Java answers.
"""
import re

JAVA_ONLY_TERMINATORS = "\r\u0085\u2028\u2029"

# (pattern, value, java.util.regex find())
JAVA_KNOWN_ANSWERS = [
    ("^abc$", "abc\n", True),
    ("^abc$", "abc\r\n", True),
    ("^abc$", "abc\n\n", False),
    ("^abc$", "abc\u2028", True),
    ("^abc$", "abc\r", True),
    ("^abc$", "abc\u0085", True),
    ("^abc$", "abc\u2029", True),
    ("^abc$", "abc\n\r", False),
    ("^abc$", "abc", True),
    ("^abc$", "abcd", False),
    ("a.c", "a\rc", False),
    ("a.c", "a\u0085c", False),
    ("a.c", "a\u2028c", False),
    ("a.c", "a\u2029c", False),
    ("a.c", "a\nc", False),
    ("a.c", "a\u00e9c", True),
    ("a.c", "a\U0001F600c", True),
    ("a.c", "a\u0084c", True),
    ("a.c", "a\u2027c", True),
    ("(?i)AbC", "xabcx", True),
    ("(?i)AbC", "xABCx", True),
    ("(?i)\u00e9", "\u00c9", False),
    ("\\W", "\u00e9", True),
    ("\\w", "\u00e9", False),
    ("\\S", "\u2028", True),
    ("\\s", "\u0085", False),
    ("[^a]", "\r", True),
    ("^[^a]$", "\U0001F600", True),
    ("^.$", "\U0001F600", True),
    ("^..$", "\U0001F600", False),
]


def valid_for(value) -> bool:
    return not any(c in value for c in JAVA_ONLY_TERMINATORS)


def matches(pattern: str, value: str) -> bool:
    """find() of ``pattern`` in ``value`` (a str free of JAVA_ONLY_TERMINATORS)."""
    assert valid_for(value), repr(value)
    return re.search(pattern, value, re.ASCII) is not None


def match_many(pattern: str, values):
    rx = re.compile(pattern, re.ASCII)
    out = []
    for v in values:
        if isinstance(v, bytes):
            v = v.decode("utf-8")
        assert valid_for(v), repr(v)
        out.append(rx.search(v) is not None)
    return out
