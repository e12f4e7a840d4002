"""Arithmetic aggregation arguments on the GPU path, host side: the expression compiler of engine/plan.py (a parsed
argument -> the postfix program of a derived value column, include/pinot_hip.h phip_expr_op), its limits and refusals,
and the program's meaning -- a numpy interpreter of the postfix ops against oracle.executor._expr_values, bit for bit.
No GPU: tests/test_gpu_expressions.py runs the programs through the library, the value-kind rule (exact int64 or
double, decided in runtime.cpp) at its edges included."""
import types

import numpy as np
import pytest

from oracle import executor
from pinot_amd import _lib
from pinot_amd.engine.plan import ExprProgram, GpuCombineOperator, UnsupportedOnGpu, _gpu_expr, plan_aggregations
from pinot_amd.query.context import Function, Identifier, Literal
from pinot_amd.query.sql import parse

COL, LONG, DBL, ADD, SUB, MUL, DIV = (_lib.EXPR_OP_PUSH_COLUMN, _lib.EXPR_OP_PUSH_LONG, _lib.EXPR_OP_PUSH_DOUBLE,
                                      _lib.EXPR_OP_ADD, _lib.EXPR_OP_SUB, _lib.EXPR_OP_MUL, _lib.EXPR_OP_DIV)


def _arg(text):
    """The parsed argument of SUM(text)."""
    return parse(f"SELECT SUM({text}) FROM t").aggregations[0].argument


def _short(prog):
    """A program's ops in short: column names, literal values, operator signs."""
    out = []
    for op, c, lv, dv in prog.ops:
        out.append(c if op == COL else lv if op == LONG else dv if op == DBL else "+-*/"[op - ADD])
    return out


SHAPES = {
    "a*(1-b)*(1+c)": ["a", 1, "b", "-", "*", 1, "c", "+", "*"],
    "a*b/100": ["a", "b", "*", 100, "/"],
    "a*2": ["a", 2, "*"],
    "-a": [0, "a", "-"],
    "(2+3)*a": [5, "a", "*"],
    "a+b+c+d": ["a", "b", "+", "c", "+", "d", "+"],
    "(a-b)*c": ["a", "b", "-", "c", "*"],
    "a/p": ["a", "p", "/"],
    "a*b-c": ["a", "b", "*", "c", "-"],
    "a*b+c": ["a", "b", "*", "c", "+"],
    "a*0.5": ["a", 0.5, "*"],
    "a*(1.5+2)": ["a", 3.5, "*"],
    "a*(7/2)": ["a", 3.5, "*"],
    "CAST(a AS DOUBLE)*b*c": ["a", "b", "*", "c", "*"],
}


@pytest.mark.parametrize("text", list(SHAPES))
def test_parse_to_program(text):
    expr, prog, b = _gpu_expr(_arg(text))
    assert expr == _lib.EXPR_COLUMN and b is None and isinstance(prog, ExprProgram)
    assert _short(prog) == SHAPES[text]
    for want, (op, c, lv, dv) in zip(SHAPES[text], prog.ops):  # literal kinds: ints stay PUSH_LONG with both images
        if isinstance(want, int):
            assert op == LONG and lv == want and dv == float(want)
        elif isinstance(want, float):
            assert op == DBL and dv == want


def test_two_operand_shapes_keep_their_tuples():
    assert _gpu_expr(_arg("a")) == (_lib.EXPR_COLUMN, "a", None)
    assert _gpu_expr(_arg("a + b")) == (_lib.EXPR_ADD, "a", "b")
    assert _gpu_expr(_arg("a - b")) == (_lib.EXPR_SUB, "a", "b")
    assert _gpu_expr(_arg("a * b")) == (_lib.EXPR_MUL, "a", "b")
    assert _gpu_expr(_arg("CAST(a AS LONG) * CAST(b AS DOUBLE)")) == (_lib.EXPR_MUL, "a", "b")
    q = parse("SELECT SUM(a * b), AVG(a), MAX(a - b) FROM t")
    prims, mapping = plan_aggregations(q.aggregations)
    assert prims == [(_lib.AGG_SUM, _lib.EXPR_MUL, "a", "b", 0, 0), (_lib.AGG_SUM, _lib.EXPR_COLUMN, "a", None, 0, 0),
                     (_lib.AGG_COUNT, 0, None, None, 0, 0), (_lib.AGG_MAX, _lib.EXPR_SUB, "a", "b", 0, 0)]
    assert mapping == [("sum", 0), ("avg", (1, 2)), ("max", 3)]


def test_literal_folding():
    assert _short(_gpu_expr(_arg("(2+3)*a"))[1]) == [5, "a", "*"]
    assert _short(_gpu_expr(_arg("a*(2*3-1)"))[1]) == ["a", 5, "*"]
    assert _short(_gpu_expr(_arg("a*(1/4)"))[1]) == ["a", 0.25, "*"]          # a division folds in double
    assert _short(_gpu_expr(_arg("a*(0.1+0.2)"))[1]) == ["a", 0.1 + 0.2, "*"]  # ... as Java adds the doubles
    # an integer fold the double computation does not reach exactly stays a double (2^53 + 1 is no double)
    prog = _gpu_expr(_arg("a*(9007199254740992+1)"))[1]
    assert prog.ops[1][0] == DBL and prog.ops[1][3] == 9007199254740992.0
    # unary minus stays minus(0, x); a negative literal is a literal
    assert _short(_gpu_expr(_arg("-a*b"))[1])[:3] == [0, "a", "-"]
    assert _short(_gpu_expr(_arg("a*-2"))[1]) == ["a", -2, "*"]
    with pytest.raises(UnsupportedOnGpu, match="reads no column"):
        _gpu_expr(Function("plus", (Literal(1), Literal(2))))


def test_identical_programs_share_one_primitive():
    q = parse("SELECT SUM(a*(1-b)), AVG(a*(1-b)), MAX(a*(1-b)), SUM(a*(2-1-b)), SUM((2+3)*a), SUM(5*a) FROM t")
    prims, mapping = plan_aggregations(q.aggregations)
    progs = {p[2] for p in prims if isinstance(p[2], ExprProgram)}
    assert len(progs) == 2  # a*(1-b) -- a*((2-1)-b) folds to it -- and 5*a
    assert mapping[0] == ("sum", 0) and mapping[1][1][0] == 0  # SUM and AVG's sum: one primitive
    assert mapping[3] == ("sum", 0)                            # the folded twin shares it
    assert mapping[4] == mapping[5]                            # (2+3)*a and 5*a
    assert prims[mapping[2][1]][0] == _lib.AGG_MAX and prims[mapping[2][1]][2] == prims[0][2]
    # programs of different filter programs never merge
    prims2, _ = plan_aggregations(q.aggregations[:2], programs=[0, 1])
    assert [p[5] for p in prims2 if p[0] == _lib.AGG_SUM] == [0, 1]


def _chain(n_cols):
    e = Identifier("c0")
    for i in range(1, n_cols):
        e = Function("plus", (e, Identifier(f"c{i}")))
    return e


def _nest(depth):
    """A right-nested sum whose evaluation holds `depth` values."""
    e = Identifier("x")
    for _ in range(depth - 1):
        e = Function("plus", (Identifier("x"), e))
    return e


def test_limits():
    assert len(_gpu_expr(_chain(8))[1].columns) == 8
    with pytest.raises(UnsupportedOnGpu, match="9 columns"):
        _gpu_expr(_chain(9))
    assert len(_gpu_expr(_nest(8))[1].ops) == 15
    with pytest.raises(UnsupportedOnGpu, match="value stack of 9"):
        _gpu_expr(_nest(9))
    e = Identifier("x")
    for _ in range(15):
        e = Function("times", (e, Identifier("x")))
    assert len(_gpu_expr(e)[1].ops) == 31
    with pytest.raises(UnsupportedOnGpu, match="33 operations"):
        _gpu_expr(Function("times", (e, Identifier("x"))))


def test_refusals():
    for sql, msg in [("SELECT DISTINCTCOUNT(a*b*c) FROM t", "distinctcount of an expression"),
                     ("SELECT PERCENTILE(a*2, 50) FROM t", "of an expression"),
                     ("SELECT MODE(a+b+c) FROM t", "of an expression")]:
        with pytest.raises(UnsupportedOnGpu, match=msg):
            plan_aggregations(parse(sql).aggregations)
    with pytest.raises(UnsupportedOnGpu, match="outside the GPU expression subset"):
        _gpu_expr(_arg("a*b*c"), derived=False)  # the selection's expressions
    with pytest.raises(UnsupportedOnGpu, match="truncates"):
        _gpu_expr(_arg("CAST(a/b AS LONG)*c"))
    with pytest.raises(UnsupportedOnGpu, match="non-integral literal"):
        _gpu_expr(_arg("CAST(a*0.5 AS INT)*c"))
    prog = _gpu_expr(_arg("CAST(a*b AS LONG)*c"))[1]
    assert prog.int_cast_columns == ("a", "b")  # (their stored types decide, per segment: _check_derived)
    with pytest.raises(UnsupportedOnGpu, match="outside the GPU expression subset"):
        _gpu_expr(Function("mod", (Identifier("a"), Literal(2))))
    with pytest.raises(UnsupportedOnGpu, match="outside the GPU expression subset"):
        _gpu_expr(Function("plus", (Identifier("a"), Literal("x"))))


class _FakeSegment:
    def __init__(self, name, intervals, types=None, docs=10):
        self.name, self.num_docs, self._iv, self._types = name, docs, intervals, types or {}

    def value_interval(self, c):
        return self._iv[c]

    def column_metadata(self, c):
        from pinot_amd.spi import DataType
        return types.SimpleNamespace(data_type=getattr(DataType, self._types.get(c, "INT")))


def _operator(segments, derived=()):
    op = object.__new__(GpuCombineOperator)
    op.segments, op.derived = list(segments), list(derived)
    return op


def test_zero_divisor_and_operand_refusals():
    seg = _FakeSegment("s0", {"a": (-5.0, 9.0), "p": (1.0, 100.0), "z": (-3.0, 4.0), "n": (-9.0, -2.0), "e": None})
    op = _operator([seg])
    tree = lambda text: _gpu_expr(_arg(text))[1].tree  # noqa: E731
    assert op._zero_divisor(tree("a/p*2")) is None
    assert op._zero_divisor(tree("a/n+1")) is None
    assert op._zero_divisor(tree("a/(p+n*0+1)")) is None          # [1, 100] + [0, 0] + 1
    assert str(op._zero_divisor(tree("a/z*2"))[0]) == "z"
    assert op._zero_divisor(tree("a/(p-50)*2")) is not None        # [-49, 50] holds 0
    assert op._zero_divisor(tree("a/(p/z)+1")) is not None         # the inner divisor
    assert op._zero_divisor(tree("a/e+1")) is not None             # unknown interval: not proven
    assert op._zero_divisor(tree("a/(2-2+p*0)+1")) is not None     # the constant 0
    # STRING operands and integer casts of real columns
    strseg = _FakeSegment("s1", {}, {"s": "STRING", "d": "DOUBLE"})
    with pytest.raises(UnsupportedOnGpu, match="STRING column s"):
        _operator([strseg], [_gpu_expr(_arg("a*s*2"))[1]])._check_derived(False)
    with pytest.raises(UnsupportedOnGpu, match="non-integral column d"):
        _operator([strseg], [_gpu_expr(_arg("CAST(d*a AS LONG)*2"))[1]])._check_derived(False)
    with pytest.raises(UnsupportedOnGpu, match="star-tree"):
        _operator([strseg], [_gpu_expr(_arg("a*2+1"))[1]])._check_derived(True)
    _operator([strseg], [_gpu_expr(_arg("CAST(a*a AS LONG)*2"))[1]])._check_derived(False)


# ---- the program's meaning -------------------------------------------------------------------------------------
def interpret(prog, columns, dtype=np.float64):
    """The postfix program over numpy columns: every op one separately rounded binary64 operation (dtype float64), or
    wrapping int64 operations (dtype int64) -- what expr.hip computes per doc."""
    stack = []
    n = len(next(iter(columns.values())))
    with np.errstate(all="ignore"):
        for op, c, lv, dv in prog.ops:
            if op == COL:
                stack.append(columns[c].astype(dtype))
            elif op in (LONG, DBL):
                stack.append(np.full(n, lv if dtype == np.int64 and op == LONG else dv, dtype=dtype))
            else:
                b, a = stack.pop(), stack.pop()
                stack.append(a + b if op == ADD else a - b if op == SUB else a * b if op == MUL else a / b)
    assert len(stack) == 1
    return stack[0]


class _Values:
    def __init__(self, cols):
        self.cols = cols

    def values(self, name):
        return self.cols[name]

    def meta(self, name):
        kind = self.cols[name].dtype.kind
        return types.SimpleNamespace(data_type=(0 if self.cols[name].dtype.itemsize == 4 else 1) if kind == "i" else 3)


@pytest.fixture(scope="module")
def random_columns():
    rng = np.random.default_rng(20)
    n = 4099
    return {"a": rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), "b": rng.integers(-10 ** 12, 10 ** 12, n),
            "c": (rng.standard_normal(n) * 1e3).astype(np.float32), "d": rng.standard_normal(n) * 1e6,
            "p": rng.integers(1, 101, n).astype(np.int32), "x": rng.random(n), "e": rng.integers(0, 50, n),
            **{f"c{i}": rng.standard_normal(n) * 10.0 ** i for i in range(8)}}


MEANING = list(SHAPES)[:10] + ["a*0.5", "a*(7/2)", "d*(1-x)*(1+x)", "b*a/100", "c/p-d*x+1", "-c*d", "(a-b)*(c-d)/(p+1)",
                               "a/e", "d*d+c"]


@pytest.mark.parametrize("text", MEANING)
def test_interpreter_equals_oracle_bit_for_bit(text, random_columns):
    arg = _arg(text)
    prog = _gpu_expr(arg)[1]
    docs = np.arange(len(random_columns["a"]))
    with np.errstate(all="ignore"):
        want = np.asarray(executor._expr_values(_Values(random_columns), arg, docs), dtype=np.float64)
    got = interpret(prog, random_columns)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_chains_equal_oracle(random_columns):
    docs = np.arange(len(random_columns["a"]))
    for e in (_chain(8), _nest(8)):
        got = interpret(_gpu_expr(e)[1], random_columns)
        want = executor._expr_values(_Values(random_columns), e, docs)
        assert np.array_equal(got.view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def test_integer_interpreter_equals_exact_values(random_columns):
    docs = np.arange(len(random_columns["a"]))
    for text in ("a*2", "-a", "(2+3)*a", "a*p-e", "(a-e)*p*3"):
        arg = _arg(text)
        got = interpret(_gpu_expr(arg)[1], random_columns, np.int64)
        want = executor._exact_values(_Values(random_columns), arg, docs)
        assert want is not None and got.dtype == np.int64 and [int(v) for v in got] == [int(v) for v in want]
