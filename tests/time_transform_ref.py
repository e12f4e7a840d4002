"""What the time transform tests expect, from numpy.datetime64 arithmetic and Python integers alone: independent of
pinot_amd/query/time_transform.py (the numpy restatement) and of pinot_amd/csrc/civil.h (the device function)."""
import numpy as np

MS_PER_DAY = 86400000
TRUNC_UNITS = ("second", "minute", "hour", "day", "week", "month", "quarter", "year")
FIELDS = ("year", "quarter", "month", "week", "dayofyear", "dayofmonth", "dayofweek", "hour", "minute", "second",
          "millisecond")
UNIT_NS = {"NANOSECONDS": 1, "MICROSECONDS": 1000, "MILLISECONDS": 10 ** 6, "SECONDS": 10 ** 9,
           "MINUTES": 60 * 10 ** 9, "HOURS": 3600 * 10 ** 9, "DAYS": 86400 * 10 ** 9}


def _d(days):
    return np.asarray(days, dtype=np.int64).astype("M8[D]")


def _i(dates):
    return dates.astype("M8[D]").astype(np.int64)


def trunc(ms, unit):
    """Joda roundFloor of epoch millis to the unit (floors below 1970; ISO weeks from Monday)."""
    ms = np.asarray(ms, dtype=np.int64)
    fixed = {"second": 1000, "minute": 60000, "hour": 3600000, "day": MS_PER_DAY}
    if unit in fixed:
        return np.floor_divide(ms, fixed[unit]) * fixed[unit]
    days = np.floor_divide(ms, MS_PER_DAY)
    if unit == "week":
        return (days - np.mod(days + 3, 7)) * MS_PER_DAY  # Monday of the week: d - (d + 3) mod 7
    if unit == "month":
        return _i(_d(days).astype("M8[M]")) * MS_PER_DAY
    if unit == "quarter":
        months = _d(days).astype("M8[M]").astype(np.int64)  # months since 1970-01
        return _i((np.floor_divide(months, 3) * 3).astype("M8[M]")) * MS_PER_DAY
    return _i(_d(days).astype("M8[Y]")) * MS_PER_DAY


def field(ms, name):
    """The UTC ISO-chronology field of epoch millis."""
    ms = np.asarray(ms, dtype=np.int64)
    days = np.floor_divide(ms, MS_PER_DAY)
    tod = np.mod(ms, MS_PER_DAY)
    dates = _d(days)
    months = dates.astype("M8[M]").astype(np.int64)
    if name == "year":
        return dates.astype("M8[Y]").astype(np.int64) + 1970
    if name == "month":
        return np.mod(months, 12) + 1
    if name == "quarter":
        return np.mod(months, 12) // 3 + 1
    if name == "dayofmonth":
        return days - _i(dates.astype("M8[M]")) + 1
    if name == "dayofyear":
        return days - _i(dates.astype("M8[Y]")) + 1
    if name == "dayofweek":
        return np.mod(days + 3, 7) + 1
    if name == "week":  # the week's Thursday decides its weekyear
        thursday = days - np.mod(days + 3, 7) + 3
        return (thursday - _i(_d(thursday).astype("M8[Y]"))) // 7 + 1
    return {"hour": tod // 3600000, "minute": tod // 60000 % 60, "second": tod // 1000 % 60,
            "millisecond": tod % 1000}[name]


def convert(values, from_unit, to_unit):
    """java.util.concurrent.TimeUnit.convert without saturation, in Python integers: / truncates toward zero."""
    a, b = UNIT_NS[from_unit], UNIT_NS[to_unit]
    out = []
    for v in np.asarray(values).tolist():
        if a >= b:
            out.append(v * (a // b))
        else:
            q = abs(v) // (b // a)
            out.append(-q if v < 0 else q)
    return np.asarray(out, dtype=np.int64)


def date_trunc(values, unit, in_unit="MILLISECONDS", out_unit=None):
    return convert(trunc(convert(values, in_unit, "MILLISECONDS"), unit), "MILLISECONDS", out_unit or in_unit)


def ms_of(text):
    return int(np.datetime64(text, "ms").astype(np.int64))


def edge_millis():
    """-1, 0, 1; both sides of the dates where the calendar turns; ISO-week year boundaries."""
    out = [-1, 0, 1, 998449445321]
    for day in ("1970-01-01", "1972-02-29", "1972-03-01", "2000-02-29", "2000-03-01", "1900-03-01", "1900-02-28",
                "2100-02-28", "2100-03-01", "2020-12-31", "2021-01-01", "2021-01-04", "2018-12-31", "2019-01-01",
                "1969-12-29", "2015-12-31", "2016-01-03", "2016-01-04", "1600-02-29", "1582-10-15", "0001-01-01"):
        t = ms_of(day)
        out += [t - 1, t, t + 1, t + MS_PER_DAY - 1, t + MS_PER_DAY]
    return np.asarray(sorted(set(out)), dtype=np.int64)


def random_millis(n, seed, years=200):
    rng = np.random.default_rng(seed)
    span = years * 366 * MS_PER_DAY
    return rng.integers(-span, span, n, dtype=np.int64)
