"""The reference's MIN / MAX / MINMAXRANGE / SUM / AVG folds, restated in plain Python over ``float``s.

One function per reference method, so that a test can say which Java code path an expected value comes from. Nothing
here imports the oracle or the library: the expected values of tests/test_special_doubles.py and
tests/test_gpu_special_doubles.py come from these folds alone, applied to the matched docs in doc order.

  java_min / java_max          Math.min / Math.max (JLS, java.lang.Math): NaN if either operand is NaN; -0.0 is
                               strictly smaller than 0.0
  fold_min / fold_max          MinAggregationFunction.aggregate / MaxAggregationFunction.aggregate (:117-130,151-160):
                               a Math.min / Math.max fold of the values, then of the holder's +inf / -inf
  group_min / group_max        aggregateGroupBySV (:180-188): ``value < holder`` / ``value > holder`` from the holder
                               default +inf / -inf, in doc order -- a NaN never wins, of two zeros the first stays
  minmaxrange                  MinMaxRangePair.apply (:42-49), grouped and not: both ends by comparison
  merge_min / merge_max        MinAggregationFunction.merge (:248-251): ``r1 < r2 ? r1 : r2`` (MAX: ``>``)
  merge_minmaxrange            MinMaxRangeAggregationFunction.merge (:191): r1.apply(r2)
  seq_sum / avg                SumAggregationFunction / AvgAggregationFunction: a sequential double sum from 0.0

and the order of final results (tests/test_order_by_specials.py, tests/test_gpu_order_by_specials.py):

  double_compare               Double.compare: -0.0 < 0.0, every NaN equal to every other and greater than +inf
  record_compare / top_records TableResizer's comparator (:90-96, Comparator.naturalOrder() over extractFinalResult,
                               reversed for DESC) and the records a trim to k must / may keep under it
"""
import functools
import math
import struct

INF = float("inf")


def same_double(a, b, sign_matters):
    """True when both are NaN; otherwise when a == b and, if ``sign_matters``, their sign bits agree (so that -0.0 and
    0.0 differ)."""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if a != b:
        return False
    return not sign_matters or math.copysign(1, a) == math.copysign(1, b)


def _neg_zero(x):
    return x == 0.0 and math.copysign(1, x) < 0


def java_min(a, b):
    """Math.min(double, double)."""
    if a != a or b != b:
        return float("nan")
    if a == 0.0 and b == 0.0:
        return -0.0 if (_neg_zero(a) or _neg_zero(b)) else 0.0
    return a if a <= b else b


def java_max(a, b):
    """Math.max(double, double)."""
    if a != a or b != b:
        return float("nan")
    if a == 0.0 and b == 0.0:
        return 0.0 if not (_neg_zero(a) and _neg_zero(b)) else -0.0
    return a if a >= b else b


def fold_min(values):
    """MIN without GROUP BY: innerMin = values[0] folded with Math.min, then Math.min(innerMin, holder = +inf); no
    value leaves the holder's +inf."""
    acc = INF
    for v in values:
        acc = java_min(float(v), acc)
    return acc


def fold_max(values):
    acc = -INF
    for v in values:
        acc = java_max(float(v), acc)
    return acc


def group_min(values):
    """MIN of one group: ``if (value < holder) holder = value`` from +inf, in doc order."""
    acc = INF
    for v in values:
        v = float(v)
        if v < acc:
            acc = v
    return acc


def group_max(values):
    acc = -INF
    for v in values:
        v = float(v)
        if v > acc:
            acc = v
    return acc


def minmaxrange(values):
    """MinMaxRangePair() then apply(value) per value: (min, max)."""
    return group_min(values), group_max(values)


def merge_min(r1, r2):
    """MinAggregationFunction.merge: r1 is the running result."""
    return r1 if r1 < r2 else r2


def merge_max(r1, r2):
    return r1 if r1 > r2 else r2


def merge_minmaxrange(p1, p2):
    """p1.apply(p2): each end of p1 is replaced only when p2's end compares beyond it."""
    return (p2[0] if p2[0] < p1[0] else p1[0]), (p2[1] if p2[1] > p1[1] else p1[1])


def seq_sum(values):
    """A double sum from 0.0 in the order given."""
    acc = 0.0
    for v in values:
        acc = acc + float(v)
    return acc


def avg(values):
    """AVG's intermediate: (sequential sum, count)."""
    values = list(values)
    return seq_sum(values), len(values)


def tree_sum(values):
    """The same values summed as a pairwise tree (neighbours first), from 0.0 for an empty list."""
    level = [float(v) for v in values]
    if not level:
        return 0.0
    while len(level) > 1:
        nxt = [level[i] + level[i + 1] for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def double_to_long_bits(x):
    """Double.doubleToLongBits: the bits as a signed long, every NaN the canonical 0x7ff8000000000000."""
    if x != x:
        return 0x7FF8000000000000
    return struct.unpack("<q", struct.pack("<d", x))[0]


def double_compare(a, b):
    """Double.compare(a, b): ``<`` / ``>`` first, then the doubleToLongBits images (-0.0 below 0.0; NaN, whatever its
    sign bit or payload, equal to NaN and above +inf)."""
    a, b = float(a), float(b)
    if a < b:
        return -1
    if a > b:
        return 1
    x, y = double_to_long_bits(a), double_to_long_bits(b)
    return 0 if x == y else (-1 if x < y else 1)


def value_compare(a, b):
    """Comparable.compareTo of two final results of one ORDER BY term: Long.compare for two ints (COUNT, the HLL
    estimate, a key's position), Double.compare otherwise."""
    if isinstance(a, int) and isinstance(b, int):
        return (a > b) - (a < b)
    return double_compare(a, b)


def record_compare(terms):
    """TableResizer's comparator over ``terms`` = [(value, ascending)], ``value`` a function of a record returning
    the term's final result (a float, an int, or a key's position as an int): the first term that does not tie
    decides, DESC reversed. Returns cmp(r1, r2)."""
    def cmp(r1, r2):
        for value, ascending in terms:
            c = value_compare(value(r1), value(r2))
            if c:
                return c if ascending else -c
        return 0
    return cmp


def top_records(records, terms, k):
    """(must_keep, may_keep) of a trim of ``records`` to its first ``k`` by record_compare(terms): the records strictly
    before the k-th record's equivalence class, and that class (whose members the reference picks by heap order).
    Without ties may_keep fills exactly the remaining places."""
    cmp = record_compare(terms)
    ordered = sorted(records, key=functools.cmp_to_key(cmp))
    if k >= len(ordered):
        return ordered, []
    pivot = ordered[k - 1]
    return [r for r in ordered if cmp(r, pivot) < 0], [r for r in ordered if cmp(r, pivot) == 0]
