"""CPU tests of the time transforms (pinot_amd/query/time_transform.py, pinot_amd/csrc/civil.h): the reference's known
answers, the numpy restatement and the shared calendar function against numpy.datetime64 arithmetic
(tests/time_transform_ref.py), the compiler's canonical programs, its errors and refusals. The calendar function runs
in a stand-alone host program built with -fsanitize=address,undefined (tests/time_transform/civil_main.cpp)."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from pinot_amd._lib import UnsupportedOnGpu
from pinot_amd.query import time_transform as tt
from pinot_amd.query.sql import parse
from pinot_amd.spi import DataType
from tests import time_transform_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_INPUT = 998449445321  # 2001-08-22T03:04:05.321Z (DateTruncTransformFunctionTest.java:140-164)
KNOWN = {"second": 998449445000, "minute": 998449440000, "hour": 998449200000, "day": 998438400000,
         "week": 998265600000, "month": 996624000000, "quarter": 993945600000, "year": 978307200000}
UNIT_PAIRS = [("SECONDS", "SECONDS"), ("SECONDS", "DAYS"), ("MILLISECONDS", "HOURS"), ("MICROSECONDS", "MILLISECONDS"),
              ("NANOSECONDS", "MINUTES"), ("DAYS", "SECONDS"), ("HOURS", "MICROSECONDS"), ("MINUTES", "MINUTES")]


def _compile(text):
    return tt.compile_transform(parse(f"SELECT COUNT(*) FROM t GROUP BY {text}").group_by[0])


def _inputs():
    return np.concatenate([ref.edge_millis(), ref.random_millis(3000, 7)])


def _in_unit(millis, unit):
    """The millisecond inputs as values of `unit` (floored: every calendar edge stays an edge)."""
    ns = ref.UNIT_NS[unit]
    if ns >= 10 ** 6:
        return np.floor_divide(millis, ns // 10 ** 6)
    return millis * (10 ** 6 // ns)


def _cases():
    """(SQL text, inputs, expected) of every unit, every field, the epoch conversions and the unit pairs."""
    ms = _inputs()
    out = []
    for u in ref.TRUNC_UNITS:
        out.append((f"dateTrunc('{u}', ts)", ms, ref.trunc(ms, u)))
        for a, b in UNIT_PAIRS:
            v = _in_unit(ms, a)
            out.append((f"dateTrunc('{u}', ts, '{a}', 'UTC', '{b}')", v, ref.date_trunc(v, u, a, b)))
        v = _in_unit(ms, "SECONDS")
        out.append((f"dateTrunc('{u.upper()}', ts, 'seconds')", v, ref.date_trunc(v, u, "SECONDS")))
    for f in ref.FIELDS:
        sql = {"dayofyear": "dayOfYear", "dayofmonth": "dayOfMonth", "dayofweek": "dayOfWeek"}.get(f, f)
        # (with the ends of the LONG range: its minimum is a LONG dimension's default null value)
        wide = np.concatenate([ms, np.asarray([-(1 << 63), -(1 << 63) + 86399999, (1 << 63) - 1], dtype=np.int64)])
        out.append((f"{sql}(ts)", wide, ref.field(wide, f)))
    for name, unit in (("toEpochSeconds", "SECONDS"), ("toEpochMinutes", "MINUTES"), ("toEpochHours", "HOURS"),
                       ("toEpochDays", "DAYS")):
        out.append((f"{name}(ts)", ms, ref.convert(ms, "MILLISECONDS", unit)))
    for a, b in UNIT_PAIRS + [("MILLISECONDS", "DAYS"), ("DAYS", "MILLISECONDS")]:
        v = _in_unit(ms, a)
        out.append((f"timeConvert(ts, '{a}', '{b}')", v, ref.convert(v, a, b)))
    return out


def test_known_answers_of_the_reference():
    for unit, want in KNOWN.items():
        prog = _compile(f"dateTrunc('{unit}', ts)").program
        assert int(tt.evaluate(prog, [KNOWN_INPUT])[0]) == want, unit
        assert int(ref.trunc([KNOWN_INPUT], unit)[0]) == want, unit  # (the yardstick agrees with the reference too)
    # roundFloor floors below 1970
    assert int(tt.evaluate(_compile("dateTrunc('day', ts)").program, [-1])[0]) == -86400000
    assert int(tt.evaluate(_compile("dateTrunc('year', ts)").program, [-1])[0]) == -31536000000
    # a negative value to a coarser unit truncates toward zero
    assert tt.evaluate(_compile("toEpochDays(ts)").program, [-1, -86400000, -86400001]).tolist() == [0, -1, -1]
    assert tt.evaluate(_compile("timeConvert(ts, 'SECONDS', 'MINUTES')").program, [-59, -60, 59]).tolist() == [0, -1, 0]
    # ISO: 2018-12-31 is the Monday of week 1 of 2019; 2021-01-03 still belongs to week 53 of 2020
    week, dow, year = (_compile(f"{f}(ts)").program for f in ("week", "dayOfWeek", "year"))
    for day, w, d, y in (("2018-12-31", 1, 1, 2018), ("2021-01-03", 53, 7, 2021), ("2021-01-04", 1, 1, 2021),
                         ("2020-12-31", 53, 4, 2020), ("1970-01-01", 1, 4, 1970)):
        v = [ref.ms_of(day)]
        assert (int(tt.evaluate(week, v)[0]), int(tt.evaluate(dow, v)[0]), int(tt.evaluate(year, v)[0])) == (w, d, y), day


def test_numpy_restatement_against_datetime64():
    for sql, values, want in _cases():
        t = _compile(sql)
        tt.check_range(t, int(values.min()), int(values.max()))
        got = tt.evaluate(t.program, values)
        assert got.dtype == np.int64
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (sql, int(values[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


def test_canonical_programs():
    P = tt.Program
    assert _compile("dateTrunc('day', ts)") == (P(tt.FUNC_TRUNC, 3, 1, 1, 1, 1), "ts", DataType.LONG)
    assert _compile("DATETRUNC('WEEK', ts, 'MILLISECONDS', 'utc', 'MILLISECONDS')").program == P(tt.FUNC_TRUNC, 4, 1, 1, 1, 1)
    assert _compile("dateTrunc('month', ts, 'SECONDS')").program == P(tt.FUNC_TRUNC, 5, 1000, 1, 1, 1000)
    assert _compile("dateTrunc('year', ts, 'MICROSECONDS', 'UTC', 'DAYS')").program == P(tt.FUNC_TRUNC, 7, 1, 1000, 1, 86400000)
    assert _compile("toEpochDays(ts)") == (P(tt.FUNC_CONVERT, 0, 1, 86400000, 1, 1), "ts", DataType.LONG)
    assert _compile("toEpochSeconds(ts)").program == _compile("timeConvert(ts, 'MILLISECONDS', 'SECONDS')").program
    assert _compile("timeConvert(ts, 'DAYS', 'HOURS')").program == P(tt.FUNC_CONVERT, 0, 24, 1, 1, 1)
    assert _compile("dayOfWeek(ts)") == (P(tt.FUNC_FIELD, 6, 1, 1, 1, 1), "ts", DataType.INT)
    assert [_compile(f"{f}(ts)").program.unit for f in tt.FIELDS] == list(range(len(tt.FIELDS)))
    assert hash(_compile("year(ts)").program) == hash(P(tt.FUNC_FIELD, 0, 1, 1, 1, 1))  # hashable: a cache key
    # not a time transform: the callers keep their present refusals
    for other in ("a*2", "a", "sum(a)", "foo(a)", "cast(a AS LONG)"):
        assert _compile(other) is None, other


def test_bad_arguments_are_bad_queries():
    for text in ("dateTrunc('day')", "dateTrunc('day', ts, 'SECONDS', 'UTC', 'DAYS', 'x')", "toEpochDays(ts, 1)",
                 "year(ts, 'UTC')", "timeConvert(ts, 'SECONDS')", "dateTrunc('fortnight', ts)",
                 "dateTrunc('day', ts, 'FORTNIGHTS')", "timeConvert(ts, 'SECONDS', 'EONS')", "dateTrunc(ts, 'day')",
                 "dateTrunc('day', ts, 'WEEKS')", "hour(5)"):
        with pytest.raises(ValueError) as e:
            _compile(text)
        assert isinstance(e.value, tt.TransformArgumentError), text


def test_refusals_name_their_reason():
    for text, reason in (("dateTrunc('day', ts, 'MILLISECONDS', 'Europe/Berlin')", "time zone Europe/Berlin"),
                         ("timeConvert(ts, 'SECONDS', 'WEEKS')", "WEEKS output"),
                         ("timeConvert(ts, 'SECONDS', 'months')", "MONTHS output"),
                         ("timeConvert(ts, 'SECONDS', 'YEARS')", "YEARS output"),
                         ("year(ts + 1)", "nested expression"), ("dateTrunc('day', ts * 1000)", "nested expression"),
                         ("toEpochDays(dateTrunc('day', ts))", "nested expression")):
        with pytest.raises(UnsupportedOnGpu, match=reason):
            _compile(text)
    t = _compile("dateTrunc('day', ts)")
    meta = dict(data_type=DataType.LONG, has_dictionary=True, is_single_value=True, hll_log2m=0)
    tt.check_column(t, SimpleNamespace(**meta))
    tt.check_column(t, SimpleNamespace(**dict(meta, data_type=DataType.INT)))
    for change, reason in ((dict(has_dictionary=False), "raw \\(no-dictionary\\) column ts"),
                           (dict(is_single_value=False), "multi-value column ts"),
                           (dict(data_type=DataType.DOUBLE), "type DOUBLE"), (dict(data_type=DataType.FLOAT), "type FLOAT"),
                           (dict(data_type=DataType.STRING), "type STRING")):
        with pytest.raises(UnsupportedOnGpu, match=reason):
            tt.check_column(t, SimpleNamespace(**dict(meta, **change)), "seg0")
    # a conversion to a finer unit that could leave int64 names the column (the reference saturates)
    big = _compile("timeConvert(ts, 'DAYS', 'NANOSECONDS')")
    tt.check_range(big, -100000, 100000)
    with pytest.raises(UnsupportedOnGpu, match="column ts"):
        tt.check_range(big, 0, 1 << 40)
    with pytest.raises(UnsupportedOnGpu, match="column ts"):
        tt.check_range(_compile("dateTrunc('day', ts, 'DAYS')"), -(1 << 62), 0)


def test_arithmetic_group_by_keys_stay_refused():
    from pinot_amd.engine.plan import GpuCombineOperator
    with pytest.raises(UnsupportedOnGpu, match="group-by expression"):
        GpuCombineOperator(parse("SELECT SUM(b) FROM t GROUP BY a*2"), [], 100000)
    with pytest.raises(UnsupportedOnGpu, match="group-by expression"):
        GpuCombineOperator(parse("SELECT SUM(b) FROM t GROUP BY dateTrunc('day', ts), a + 1"), [], 100000)


def test_integer_predicates():
    P = lambda sql: parse(f"SELECT COUNT(*) FROM t WHERE {sql}").filter.predicate  # noqa: E731
    ip = tt.integer_predicate
    assert ip(P("year(ts) = 2001"), "ts")[0] == "set" and ip(P("year(ts) = 2001"), "ts")[3].tolist() == [2001]
    assert ip(P("year(ts) <> 2001"), "ts")[0] == "not_set"
    assert ip(P("year(ts) IN (3, 1, 3, 2.5)"), "ts")[3].tolist() == [1, 3]  # a non-integral literal equals no LONG
    assert ip(P("year(ts) BETWEEN 1 AND 5"), "ts")[:3] == ("range", 1, 5)
    assert ip(P("year(ts) > 1.5"), "ts")[:3] == ("range", 2, (1 << 63) - 1)
    assert ip(P("year(ts) < 4"), "ts")[:3] == ("range", -(1 << 63), 3)
    assert ip(P("year(ts) <= 4.5"), "ts")[:3] == ("range", -(1 << 63), 4)
    kind, lo, hi, _ = ip(P("year(ts) > 9223372036854775807"), "ts")
    assert kind == "range" and lo > hi  # nothing
    vals = np.asarray([1, 2, 3, 4, 5])
    assert tt.match_values(vals, "range", 2, 4, []).tolist() == [False, True, True, True, False]
    assert tt.match_values(vals, "not_set", 0, 0, np.asarray([2, 9])).tolist() == [True, False, True, True, True]


CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CXX = CLANG if os.path.exists(CLANG) else (shutil.which("clang++") or shutil.which("g++"))


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_shared_calendar_function_under_sanitizers(tmp_path):
    """civil.h, the function the device kernel calls, compiled for the host with AddressSanitizer and
    UndefinedBehaviorSanitizer into a stand-alone program, over the same inputs against the same expectations."""
    exe = tmp_path / "civil_main"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "time_transform", "civil_main.cpp")])
    lines, want = [], []
    for sql, values, expected in _cases():
        p = _compile(sql).program
        head = " ".join(str(x) for x in p)
        lines += [f"{head} {v}" for v in values.tolist()]
        want += expected.tolist()
    bad_programs = ["0 0 1 1 1 1 5", "4 0 1 1 1 1 5", "2 8 1 1 1 1 5", "3 11 1 1 1 1 5", "3 0 1000 1 1 1 5",
                    "1 0 0 1 1 1 5", "1 0 1 -1 1 1 5", "2 0 1000 1000 1 1 5", "1 1 1 1 1 1 5", "1 0 1 1 1 60 5"]
    overflow = ["1 0 1000000 1 1 1 9223372036855", "2 3 86400000 1 1 1 -106751991168", "2 7 1 1 1000000 1 9223372036854775"]
    res = subprocess.run([str(exe)], input="\n".join(lines + bad_programs + overflow) + "\n", capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [r.split() for r in res.stdout.splitlines()]
    assert len(rows) == len(lines) + len(bad_programs) + len(overflow)
    for i, (row, w) in enumerate(zip(rows, want)):
        assert row == ["1", "1", str(w)], (lines[i], row, w)
    for row, line in zip(rows[len(lines):len(lines) + len(bad_programs)], bad_programs):
        assert row[0] == "0", line
    for row, line in zip(rows[len(lines) + len(bad_programs):], overflow):
        assert row[:2] == ["1", "0"], line
