"""Query context types (host side).

Mirrors the shapes the reference's server consumes (all in pinot-common / pinot-core, used as
inputs to the hot path, not rebuilt):
  ExpressionContext      pinot-common/.../request/context/ExpressionContext.java
  FilterContext          pinot-common/.../request/context/FilterContext.java:37-39 (AND/OR/NOT/PREDICATE/CONSTANT)
  Predicate.Type         pinot-common/.../request/context/predicate/Predicate.java:30-42
  RangePredicate         pinot-common/.../request/context/predicate/RangePredicate.java:38-143
  QueryContext           pinot-core/.../query/request/context/QueryContext.java:74-757
"""
import re
from dataclasses import dataclass, field
from decimal import Decimal
from typing import List, Optional, Tuple, Union

from .._lib import UnsupportedOnGpu


# ----------------------------------------------------------------------------- expressions
@dataclass(frozen=True)
class Identifier:
    name: str

    def __str__(self):
        return self.name


@dataclass(frozen=True)
class Literal:
    value: Union[int, float, str]

    def __str__(self):
        return repr(self.value) if isinstance(self.value, str) else str(self.value)


@dataclass(frozen=True)
class Function:
    name: str  # lower-case canonical name
    args: Tuple["Expression", ...]

    def __str__(self):
        return f"{self.name}({','.join(str(a) for a in self.args)})"


@dataclass(frozen=True)
class FilterClause:
    """`agg(...) FILTER(WHERE ...)`: an aggregation with its own filter (QueryContext's
    filtered-aggregation pairs, pinot-core/.../query/request/context/QueryContext.java)."""
    function: "Function"
    filter: "FilterContext"

    def __str__(self):
        return f"{self.function} FILTER(WHERE {self.filter})"


Expression = Union[Identifier, Literal, Function, FilterClause]


def columns_of(expr) -> List[str]:
    if isinstance(expr, Identifier):
        return [expr.name]
    if isinstance(expr, FilterContext):  # a CASE condition
        return expr.columns()
    if isinstance(expr, FilterClause):
        return columns_of(expr.function)
    if isinstance(expr, Function):
        out = []
        for a in expr.args:
            for c in columns_of(a):
                if c not in out:
                    out.append(c)
        return out
    return []


# ----------------------------------------------------------------------------- predicates
class PredicateType:
    EQ = "EQ"
    NOT_EQ = "NOT_EQ"
    IN = "IN"
    NOT_IN = "NOT_IN"
    RANGE = "RANGE"
    IS_NULL = "IS_NULL"          # the column's null value vector (FilterPlanNode.java:294-307)
    IS_NOT_NULL = "IS_NOT_NULL"
    # REGEXP_LIKE(col, 'pattern'), values = (pattern,); col LIKE 'p' arrives as REGEXP_LIKE(col, like_to_regexp_like(p))
    # (RequestContextUtils.java:231-236)
    REGEXP_LIKE = "REGEXP_LIKE"


UNBOUNDED = "*"  # RangePredicate.UNBOUNDED


@dataclass(frozen=True)
class Predicate:
    type: str
    lhs: Expression
    values: Tuple = ()                 # EQ/NOT_EQ: (v,), IN/NOT_IN: (v1, ...), REGEXP_LIKE: (pattern,)
    lower: object = UNBOUNDED          # RANGE
    upper: object = UNBOUNDED
    lower_inclusive: bool = False
    upper_inclusive: bool = False

    @property
    def column(self) -> str:
        if not isinstance(self.lhs, Identifier):
            if self.type == PredicateType.REGEXP_LIKE:
                raise UnsupportedOnGpu(f"REGEXP_LIKE / LIKE over the expression {self.lhs}: columns only on the GPU path")
            raise NotImplementedError("predicates on expressions are out of scope")
        return self.lhs.name


@dataclass(frozen=True)
class FilterContext:
    type: str  # AND / OR / NOT / PREDICATE / CONSTANT
    children: Tuple["FilterContext", ...] = ()
    predicate: Optional[Predicate] = None
    constant: Optional[bool] = None

    @staticmethod
    def AND(*children):
        return FilterContext("AND", tuple(children))

    @staticmethod
    def OR(*children):
        return FilterContext("OR", tuple(children))

    @staticmethod
    def NOT(child):
        return FilterContext("NOT", (child,))

    @staticmethod
    def PRED(p: Predicate):
        return FilterContext("PREDICATE", predicate=p)

    def columns(self) -> List[str]:
        if self.type == "PREDICATE":
            lhs = self.predicate.lhs
            if isinstance(lhs, Function):
                from .time_transform import is_time_transform_name  # (imports this module)
                if is_time_transform_name(lhs.name):  # a time transform of one column reads that column
                    return columns_of(lhs)
            return [self.predicate.column]
        out = []
        for c in self.children:
            for x in c.columns():
                if x not in out:
                    out.append(x)
        return out


# ----------------------------------------------------------------------------- aggregations
SUPPORTED_AGGREGATIONS = ("count", "sum", "min", "max", "avg", "minmaxrange", "distinctcounthll",
                          "distinctcountrawhll", "distinctcount", "percentile", "mode")

# Aggregations over a multi-value column, each with the single-value function whose intermediate result, merge and
# final result it shares (CountMVAggregationFunction extends CountAggregationFunction, SumMV... extends Sum..., and so
# on, pinot-core/.../query/aggregation/function/*MVAggregationFunction.java): per matched doc they read a reduction of
# the doc's row -- its length, its sum, its extremes.
MV_AGGREGATIONS = {"countmv": "count", "summv": "sum", "minmv": "min", "maxmv": "max", "avgmv": "avg",
                   "minmaxrangemv": "minmaxrange"}
# Multi-value aggregations the parser knows by name and the GPU plan maker refuses
REFUSED_MV_AGGREGATIONS = ("distinctcountmv", "distinctcountbitmapmv", "distinctcounthllmv", "distinctcountrawhllmv",
                           "distinctcounthllplusmv", "distinctcountrawhllplusmv", "distinctsummv", "distinctavgmv",
                           "percentilemv", "percentileestmv", "percentilerawestmv", "percentiletdigestmv",
                           "percentilerawtdigestmv", "percentilekllmv", "percentilerawkllmv")


def sv_twin(function: str) -> str:
    """The single-value function an aggregation merges and finishes as (itself unless it is one of MV_AGGREGATIONS)."""
    return MV_AGGREGATIONS.get(function, function)


MODE_REDUCERS = ("MIN", "MAX", "AVG")  # ModeAggregationFunction.MultiModeReducerType


def java_double_string(v: float) -> str:
    """Double.toString of a percentile ([0, 100]): the shortest digits that round-trip, as Python's repr, but in
    computerised scientific notation below 1e-3 ('1.0E-4' where Python writes '0.0001')."""
    v = float(v)
    if v == 0.0 or abs(v) >= 1e-3:
        return repr(v)
    _, digits, exp = Decimal(repr(v)).as_tuple()
    rest = "".join(map(str, digits[1:])) or "0"
    return f"{digits[0]}.{rest}E{exp + len(digits) - 1}"


def aggregation_function_of(name: str):
    """A SQL function name -> (canonical aggregation function, percentile or None): PERCENTILEnn is PERCENTILE with
    the integer nn in its name (AggregationFunctionFactory: the name's remainder parsed as the percentile)."""
    if name in SUPPORTED_AGGREGATIONS or name in MV_AGGREGATIONS or name in REFUSED_MV_AGGREGATIONS:
        return name, None
    m = re.fullmatch(r"(percentile(?:est|tdigest|kll|rawest|rawtdigest|rawkll)?)\d+mv", name)
    if m:  # PERCENTILEnnMV and its sketches: known, refused by the GPU plan maker
        return m.group(1) + "mv", None
    if name.startswith("percentile") and name[len("percentile"):].isdigit():
        return "percentile", int(name[len("percentile"):])
    return None, None


def aggregation_call(fn: "Function"):
    """(function, percentile, version, reducer) of an aggregation call, None for another function. PERCENTILE(col, p)
    takes p as a number or a quoted one (AggregationFunctionFactory parses the literal's string); MODE(col[, 'MIN' |
    'MAX' | 'AVG']). A percentile outside [0, 100], a reducer outside the three and a wrong argument count raise
    ValueError."""
    function, nn = aggregation_function_of(fn.name)
    if function is None:
        return None
    if function == "percentile":
        if nn is not None:
            if len(fn.args) != 1:
                raise ValueError(f"{fn.name} takes one argument")
            p, version = float(nn), 0
        else:
            if len(fn.args) != 2 or not isinstance(fn.args[1], Literal):
                raise ValueError("PERCENTILE takes a column and a literal percentile")
            try:
                p, version = float(fn.args[1].value), 1
            except (TypeError, ValueError):
                raise ValueError(f"PERCENTILE: {fn.args[1].value!r} is not a number") from None
        if not 0.0 <= p <= 100.0:  # (NaN fails both comparisons)
            raise ValueError(f"percentile {p} outside [0, 100]")
        return function, p, version, "MIN"
    if function == "mode":
        if not 1 <= len(fn.args) <= 2:
            raise ValueError("MODE takes a column and an optional reducer")
        reducer = "MIN"
        if len(fn.args) == 2:
            r = fn.args[1]
            if not isinstance(r, Literal) or r.value not in MODE_REDUCERS:  # (MultiModeReducerType.valueOf: exact case)
                raise ValueError(f"MODE reducer {r} is not one of 'MIN', 'MAX', 'AVG'")
            reducer = r.value
        return function, None, 0, reducer
    return function, None, 0, "MIN"


@dataclass(frozen=True)
class AggregationInfo:
    function: str           # canonical lower-case name, e.g. "sum"
    argument: Optional[Expression]  # None for COUNT(*)
    log2m: int = 8
    filter: Optional["FilterContext"] = None  # FILTER(WHERE ...) of a filtered aggregation
    percentile: Optional[float] = None  # PERCENTILE: the percentile, in [0, 100]
    version: int = 0        # PERCENTILE: 0 = PERCENTILEnn(col), 1 = PERCENTILE(col, p) (PercentileAggregationFunction._version)
    reducer: str = "MIN"    # MODE: what becomes of several values of maximal count (MODE_REDUCERS)

    @property
    def result_column_name(self) -> str:
        """AggregationFunction.getResultColumnName(): lower-case function name + argument; COUNT(col) keeps its
        argument only under enableNullHandling (the argument is then set: CountAggregationFunction.java:44-66);
        PERCENTILE names its percentile (PercentileAggregationFunction.java:60-64)."""
        if self.function == "count":
            base = "count(*)" if self.argument is None else f"count({self.argument})"
        elif self.function == "percentile":
            base = (f"percentile{int(self.percentile)}({self.argument})" if self.version == 0
                    else f"percentile({self.argument}, {java_double_string(self.percentile)})")
        else:
            base = f"{self.function}({self.argument})"
        return base if self.filter is None else f"{base} FILTER(WHERE {self.filter})"

    def unfiltered(self) -> "AggregationInfo":
        return AggregationInfo(self.function, self.argument, self.log2m, None, self.percentile, self.version,
                               self.reducer)


@dataclass
class OrderByExpression:
    expression: Expression
    ascending: bool = True
    nulls_last: Optional[bool] = None  # NULLS FIRST / LAST; None = the default

    @property
    def is_nulls_last(self) -> bool:
        """OrderByExpressionContext.isNullsLast (pinot-core/.../request/context/OrderByExpressionContext.java:53-61):
        nulls sort as if larger than every value unless NULLS FIRST / LAST says otherwise."""
        return self.ascending if self.nulls_last is None else self.nulls_last


@dataclass
class QueryContext:
    table: str
    select: List[Tuple[Expression, Optional[str]]]
    aggregations: List[AggregationInfo]
    filter: Optional[FilterContext]
    group_by: List[Expression]
    order_by: List[OrderByExpression] = field(default_factory=list)
    limit: int = 10
    options: dict = field(default_factory=dict)
    offset: int = 0
    distinct: bool = False  # SELECT DISTINCT (QueryContext.isDistinct: the select list is the DISTINCT columns)

    @property
    def is_aggregation(self) -> bool:
        return bool(self.aggregations) and not self.group_by

    @property
    def is_group_by(self) -> bool:
        return bool(self.group_by)

    @property
    def is_selection(self) -> bool:
        """A selection (row-returning) query: no aggregation, no group-by, not DISTINCT
        (QueryContext.isSelectionQuery; QueryContextUtils.isSelectionQuery excludes a distinct query)."""
        return not self.aggregations and not self.group_by and not self.distinct

    def select_expressions(self, segment_columns=None):
        """SelectionOperatorUtils.extractExpressions (pinot-core/.../query/selection/SelectionOperatorUtils.java:
        83-124) without ORDER BY: the select expressions, deduplicated in order; SELECT * expands to the segment's
        columns sorted by name (columns starting with '$' excluded)."""
        exprs = [e for e, _ in self.select]
        if len(exprs) == 1 and isinstance(exprs[0], Identifier) and exprs[0].name == "*":
            return [Identifier(c) for c in sorted(c for c in (segment_columns or []) if not c.startswith("$"))]
        out = []
        for e in exprs:
            if e not in out:
                out.append(e)
        return out

    def selection_block_expressions(self, segment_columns=None):
        """SelectionOperatorUtils.extractExpressions (SelectionOperatorUtils.java:83-124) with ORDER BY: the order-by
        expressions first, deduplicated in ORDER BY order, then the select expressions not among them in select order
        (SELECT * = the segment's columns sorted by name, '$' columns excluded). Without ORDER BY, or with LIMIT 0
        (which ignores it), select_expressions."""
        out = []
        if self.limit > 0:
            for ob in self.order_by:
                if ob.expression not in out:
                    out.append(ob.expression)
        for e in self.select_expressions(segment_columns):
            if e not in out:
                out.append(e)
        return out
