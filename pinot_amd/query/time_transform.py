"""Time transforms of one column: the subset that GROUP BY keys and filter predicates take on the GPU path.

  dateTrunc(unit, col [, inUnit [, tz [, outUnit]]])   DateTruncTransformFunction.java:100-142
  toEpochSeconds / Minutes / Hours / Days (col)        DateTimeFunctions.java:80-133
  timeConvert(col, inUnit, outUnit)                    TimeConversionTransformFunction.java (TimeUnit names only)
  year, quarter, month, week, dayOfYear, dayOfMonth,
  dayOfWeek, hour, minute, second, millisecond (col)   DateTimeFunctions.java:656-1034 (the one-argument UTC forms)

``compile_transform(expr)`` turns such a call into a canonical program

    out = scale(op(scale(v, in_mul, in_div)), out_mul, out_div)

with ``scale(x, m, d) = x * m`` or Java's ``x / d`` (truncating toward zero; one of m, d is 1), and ``op`` the
identity (CONVERT), ``roundFloor`` of epoch millis to a unit (TRUNC: floors below 1970 too, proleptic Gregorian,
ISO weeks from Monday) or a UTC ISO-chronology field of epoch millis (FIELD). The same six numbers are the library's
phip_time_transform (include/pinot_hip.h) and what transform.hip evaluates per dictionary entry.

``evaluate(program, values)`` restates the program in numpy over an int64 array: the host path of small dictionaries
(engine.segment.TRANSFORM_HOST_CARD) and the CPU tests' subject. It shares nothing with the device code
(csrc/civil.h) but the calendar's definition: 400-year eras of 146097 days counted from 0000-03-01.
"""
from typing import NamedTuple, Optional

import numpy as np

from .._lib import UnsupportedOnGpu
from ..spi import DataType
from .context import Function, Identifier, Literal

FUNC_CONVERT, FUNC_TRUNC, FUNC_FIELD = 1, 2, 3  # phip_time_transform.function (0 = the plain column)

TRUNC_UNITS = ("second", "minute", "hour", "day", "week", "month", "quarter", "year")
FIELDS = ("year", "quarter", "month", "week", "dayofyear", "dayofmonth", "dayofweek", "hour", "minute", "second",
          "millisecond")

# java.util.concurrent.TimeUnit in nanoseconds
_TIME_UNITS = {"NANOSECONDS": 1, "MICROSECONDS": 1000, "MILLISECONDS": 10 ** 6, "SECONDS": 10 ** 9,
               "MINUTES": 60 * 10 ** 9, "HOURS": 3600 * 10 ** 9, "DAYS": 86400 * 10 ** 9}
_REFUSED_OUTPUTS = ("WEEKS", "MONTHS", "YEARS")  # TimeUnitTransformerFactory's custom outputs
_TO_EPOCH = {"toepochseconds": "SECONDS", "toepochminutes": "MINUTES", "toepochhours": "HOURS", "toepochdays": "DAYS"}

_MS_PER_DAY = 86400000
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


class TransformArgumentError(ValueError):
    """A time transform called with the wrong number or kind of arguments, or an unknown unit: a bad query."""


class Program(NamedTuple):
    function: int
    unit: int  # TRUNC: index into TRUNC_UNITS; FIELD: index into FIELDS; CONVERT: 0
    in_mul: int
    in_div: int
    out_mul: int
    out_div: int


class TimeTransform(NamedTuple):
    program: Program
    column: str
    result_type: DataType  # LONG, or INT for a FIELD


def is_time_transform_name(name: str) -> bool:
    return name in ("datetrunc", "timeconvert") or name in _TO_EPOCH or name in FIELDS


def _string_arg(fn, i, what):
    a = fn.args[i]
    if not isinstance(a, Literal) or not isinstance(a.value, str):
        raise TransformArgumentError(f"{fn}: {what} must be a string literal")
    return a.value


def _time_unit(fn, i, what):
    name = _string_arg(fn, i, what).upper()
    if name not in _TIME_UNITS:
        if name in _REFUSED_OUTPUTS and what == "the output unit" and fn.name == "timeconvert":
            raise UnsupportedOnGpu(f"{fn}: the {name} output of timeConvert is not on the GPU path")
        raise TransformArgumentError(f"{fn}: unknown time unit {name}")
    return _TIME_UNITS[name]


def _scale(from_ns, to_ns):
    """(mul, div) of TimeUnit.convert from a unit of from_ns nanoseconds to one of to_ns."""
    return (from_ns // to_ns, 1) if from_ns >= to_ns else (1, to_ns // from_ns)


def _column_arg(fn, i):
    a = fn.args[i]
    if isinstance(a, Identifier):
        return a.name
    if isinstance(a, Literal):
        raise TransformArgumentError(f"{fn}: argument {i + 1} must be a column")
    raise UnsupportedOnGpu(f"{fn}: the nested expression {a} as a time transform's argument is not on the GPU path")


def compile_transform(expr) -> Optional[TimeTransform]:
    """The canonical program, column and result type of a time transform call; None for any other expression. Raises
    TransformArgumentError for a wrong arity or an unknown unit, UnsupportedOnGpu for a non-UTC zone, a timeConvert
    WEEKS / MONTHS / YEARS output and a nested expression as the argument."""
    if not isinstance(expr, Function) or not is_time_transform_name(expr.name):
        return None
    n = len(expr.args)
    ms = _TIME_UNITS["MILLISECONDS"]
    if expr.name == "datetrunc":
        if not 2 <= n <= 5:
            raise TransformArgumentError(f"{expr}: dateTrunc takes 2 to 5 arguments, not {n}")
        unit = _string_arg(expr, 0, "the unit").lower()
        if unit not in TRUNC_UNITS:
            raise TransformArgumentError(f"{expr}: unknown dateTrunc unit {unit}")
        in_ns = _time_unit(expr, 2, "the input unit") if n >= 3 else ms
        if n >= 4 and _string_arg(expr, 3, "the time zone").upper() != "UTC":
            raise UnsupportedOnGpu(f"{expr}: the time zone {expr.args[3].value} is not on the GPU path (UTC only)")
        out_ns = _time_unit(expr, 4, "the output unit") if n >= 5 else in_ns
        column = _column_arg(expr, 1)
        return TimeTransform(Program(FUNC_TRUNC, TRUNC_UNITS.index(unit), *_scale(in_ns, ms), *_scale(ms, out_ns)),
                             column, DataType.LONG)
    if expr.name == "timeconvert":
        if n != 3:
            raise TransformArgumentError(f"{expr}: timeConvert takes 3 arguments, not {n}")
        in_ns = _time_unit(expr, 1, "the input unit")
        out_ns = _time_unit(expr, 2, "the output unit")
        return TimeTransform(Program(FUNC_CONVERT, 0, *_scale(in_ns, out_ns), 1, 1), _column_arg(expr, 0), DataType.LONG)
    if n != 1:
        raise TransformArgumentError(f"{expr}: {expr.name} takes 1 argument on the GPU path's subset, not {n}")
    column = _column_arg(expr, 0)
    if expr.name in _TO_EPOCH:
        return TimeTransform(Program(FUNC_CONVERT, 0, *_scale(ms, _TIME_UNITS[_TO_EPOCH[expr.name]]), 1, 1), column,
                             DataType.LONG)
    return TimeTransform(Program(FUNC_FIELD, FIELDS.index(expr.name), 1, 1, 1, 1), column, DataType.INT)


def transforms_in(expr):
    """True when a time transform call stands anywhere in the expression."""
    if isinstance(expr, Function):
        return is_time_transform_name(expr.name) or any(transforms_in(a) for a in expr.args)
    return False


def check_range(tt: TimeTransform, vmin: int, vmax: int):
    """Refuse the transform over a column whose values [vmin, vmax] could leave int64 in a multiplication
    (TimeUnit.convert saturates there; the saturation is not reproduced)."""
    p = tt.program
    for v in (int(vmin), int(vmax)):
        x = v * p.in_mul
        if not _I64_MIN <= x <= _I64_MAX:
            raise UnsupportedOnGpu(f"time transform over column {tt.column}: {v} x {p.in_mul} leaves the LONG range "
                                   f"(the reference saturates)")
        if p.function == FUNC_TRUNC:
            # (roundFloor moves a value down by less than 366 days, the output scale multiplies what is left)
            y = (abs(x) // p.in_div + 366 * _MS_PER_DAY) * p.out_mul
            if y > _I64_MAX:
                raise UnsupportedOnGpu(f"time transform over column {tt.column}: truncating {v} to "
                                       f"{TRUNC_UNITS[p.unit]} x {p.out_mul} leaves the LONG range")


def check_column(tt: TimeTransform, metadata, segment_name=""):
    """A time transform reads a single-value dictionary INT / LONG column."""
    m = metadata
    where = f" in segment {segment_name}" if segment_name else ""
    if getattr(m, "hll_log2m", 0) or m.data_type not in (DataType.INT, DataType.LONG):
        raise UnsupportedOnGpu(f"time transform over column {tt.column} of type {DataType(m.data_type).name}{where}: "
                               f"INT / LONG only on the GPU path")
    if not getattr(m, "is_single_value", True):
        raise UnsupportedOnGpu(f"time transform over the multi-value column {tt.column}{where}")
    if not m.has_dictionary:
        raise UnsupportedOnGpu(f"time transform over the raw (no-dictionary) column {tt.column}{where}")


# ------------------------------------------------------------------------------ numpy restatement
def _trunc_div(x, d):
    """Java's x / d for d > 0."""
    if d == 1:
        return x
    q = np.abs(x) // d
    return np.where(x < 0, -q, q)


def _civil(days):
    """(year, month, day of month) of epoch days: eras of 400 years = 146097 days, counted from 0000-03-01 so the
    leap day ends its year."""
    z = days + 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = np.where(mp < 10, mp + 3, mp - 9)
    return yoe + era * 400 + (m <= 2), m, d


def _days(y, m, d):
    y = y - (m <= 2)
    era = y // 400
    yoe = y - era * 400
    doy = (153 * np.where(m > 2, m - 3, m + 9) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def _trunc(ms, unit):
    name = TRUNC_UNITS[unit]
    fixed = {"second": 1000, "minute": 60000, "hour": 3600000, "day": _MS_PER_DAY}
    if name in fixed:
        return ms // fixed[name] * fixed[name]
    days = ms // _MS_PER_DAY
    if name == "week":
        return (days - (days + 3) % 7) * _MS_PER_DAY
    y, m, _ = _civil(days)
    one = np.ones_like(y)
    if name == "month":
        return _days(y, m, one) * _MS_PER_DAY
    if name == "quarter":
        return _days(y, (m - 1) // 3 * 3 + 1, one) * _MS_PER_DAY
    return _days(y, one, one) * _MS_PER_DAY


def _field(ms, unit):
    name = FIELDS[unit]
    days = ms // _MS_PER_DAY
    tod = np.mod(ms, _MS_PER_DAY)  # (not ms - days * 86400000: the product leaves int64 near the LONG minimum)
    if name == "hour":
        return tod // 3600000
    if name == "minute":
        return tod // 60000 % 60
    if name == "second":
        return tod // 1000 % 60
    if name == "millisecond":
        return tod % 1000
    if name == "dayofweek":
        return (days + 3) % 7 + 1
    if name == "week":  # the week of the weekyear: both are its Thursday's
        thursday = days - (days + 3) % 7 + 3
        wy, _, _ = _civil(thursday)
        return (thursday - _days(wy, np.ones_like(wy), np.ones_like(wy))) // 7 + 1
    y, m, d = _civil(days)
    if name == "year":
        return y
    if name == "quarter":
        return (m - 1) // 3 + 1
    if name == "month":
        return m
    if name == "dayofmonth":
        return d
    return days - _days(y, np.ones_like(y), np.ones_like(y)) + 1  # dayofyear


def evaluate(program: Program, values) -> np.ndarray:
    """The program over an int64 array (no overflow check: check_range is the caller's)."""
    p = Program(*program)
    v = np.asarray(values, dtype=np.int64)
    x = _trunc_div(v * np.int64(p.in_mul), p.in_div)
    if p.function == FUNC_TRUNC:
        x = _trunc(x, p.unit)
    elif p.function == FUNC_FIELD:
        x = _field(x, p.unit)
    elif p.function != FUNC_CONVERT:
        raise ValueError(f"time transform function code {p.function}")
    return np.asarray(_trunc_div(x * np.int64(p.out_mul), p.out_div), dtype=np.int64)


# ------------------------------------------------------------------------------ predicates over a program's values
def integer_predicate(pred, column):
    """A predicate's comparison with the transform's integer values, literals resolved to int64 as the raw-value
    evaluators do for a LONG: (kind, lo, hi, values) with kind 'range' (inclusive lo..hi; lo > hi = no value) or
    'set' / 'not_set' (sorted distinct int64 values). A non-integral EQ / IN literal matches nothing, a range bound is
    rounded inward, a bound outside int64 is clamped."""
    import math
    from decimal import Decimal, InvalidOperation

    def num(v):
        if isinstance(v, bool) or not isinstance(v, (int, float, str)):
            raise TransformArgumentError(f"time transform over column {column}: literal {v!r} is not a number")
        try:
            d = Decimal(v) if not isinstance(v, float) else Decimal(repr(v))
        except InvalidOperation:
            raise TransformArgumentError(f"time transform over column {column}: literal {v!r} is not a number") from None
        if not d.is_finite():
            raise TransformArgumentError(f"time transform over column {column}: literal {v!r} is not finite")
        return d

    if pred.type in ("EQ", "NOT_EQ", "IN", "NOT_IN"):
        vals = set()
        for v in pred.values:
            d = num(v)
            if d == d.to_integral_value() and _I64_MIN <= int(d) <= _I64_MAX:
                vals.add(int(d))
        return ("set" if pred.type in ("EQ", "IN") else "not_set"), 0, 0, np.asarray(sorted(vals), dtype=np.int64)
    if pred.type != "RANGE":
        raise UnsupportedOnGpu(f"{pred.type} over a time transform of column {column} is not on the GPU path")
    lo, hi = _I64_MIN, _I64_MAX
    if pred.lower != "*":
        d = num(pred.lower)
        lo = math.ceil(d) if pred.lower_inclusive or d != d.to_integral_value() else int(d) + 1
    if pred.upper != "*":
        d = num(pred.upper)
        hi = math.floor(d) if pred.upper_inclusive or d != d.to_integral_value() else int(d) - 1
    if lo > _I64_MAX or hi < _I64_MIN:
        lo, hi = 1, 0
    return "range", max(lo, _I64_MIN), min(hi, _I64_MAX), np.zeros(0, dtype=np.int64)


def match_values(values, kind, lo, hi, members) -> np.ndarray:
    """Boolean mask of the transformed values that the integer predicate accepts."""
    values = np.asarray(values, dtype=np.int64)
    if kind == "range":
        return (values >= lo) & (values <= hi) if lo <= hi else np.zeros(len(values), dtype=bool)
    hit = np.isin(values, members)
    return hit if kind == "set" else ~hit
