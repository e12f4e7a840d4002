"""MIN / MAX / MINMAXRANGE / SUM / AVG of NaN, infinite, signed-zero, denormal and DBL_MAX metrics on every
aggregation walk of the GPU path, against the reference's folds (tests/java_fold.py) of the stored values of the
matched docs in doc order -- never against the oracle or a second run of the library.

The segments, columns, placements (P1 the special value among the matched docs of every tile, P2 only in docs every
filter excludes -- doc 0 and the last doc of the ragged tile among them --, P3 in the docs of group 3 only) and the
expected values come from tests/test_special_doubles.py, which also proves on the CPU that every SUM input here folds
to the same double in any order: sums are compared bit for bit (or NaN to NaN), counts exactly, MIN / MAX /
MINMAXRANGE by java_fold.same_double. The sign of a zero counts for non-grouped MIN / MAX on one segment only:
elsewhere the reference keeps the first-seen zero, and doc order is not a GPU notion.

What may be refused (UnsupportedOnGpu with a reason naming NaN, so that the CPU plan maker answers): a query whose
MIN / MAX / MINMAXRANGE reads a column that holds NaN, or a column that holds an infinity under an arithmetic
expression (0 * inf). Every other cell must run on the GPU: all of di, dp, dz, dzn, dd, dh, every SUM / AVG cell (the
NaN ones too), every P2 cell of a column without NaN.

Two segments: the reference's merge ``r1 < r2 ? r1 : r2`` makes a NaN matched in one segment only depend on the order
the segments' results arrive in (merge(NaN, x) = x, merge(x, NaN) = NaN) -- in the reference itself; such a cell is
not asserted and by construction does not occur here: both segments place their special values alike, so a NaN is
matched in both or in neither.
"""
import numpy as np
import pytest

from pinot_amd.query.sql import parse
from tests import java_fold as jf
from tests.test_special_doubles import (EXPRESSIONS, FILTERS, METRICS, check_block, expression_query, holds_nan,
                                        matched, queries_for, special_segments, wants)

pytestmark = pytest.mark.gpu

MAX_EXPRESSIONS = ("MAX(a * dp)", "MAX(a * dp_r)")   # 0 * inf = NaN under MAX: inside the NaN allowance
FILTER_CLAUSE = "SELECT MIN({c}) FILTER (WHERE f < 50), MAX({c}) FILTER (WHERE f >= 50) FROM t"


@pytest.fixture(scope="module")
def gpu_segments(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    segs = [GpuSegment(s.raw) for s in special_segments()]
    yield segs
    for s in segs:
        s.destroy()


def _run(sql, segs):
    """(query, block, None), or (query, None, reason) when the plan maker refuses the query."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker, UnsupportedOnGpu
    qc = parse(sql)
    try:
        op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    except UnsupportedOnGpu as e:
        return qc, None, str(e)
    try:
        return qc, op.next_block(), None
    finally:
        close = getattr(op, "close", None)
        if close is not None:
            close()


def _cells(flt, key):
    """(sql, column or expression the expected values fold, may the query be refused) of one filter and key."""
    for col in METRICS:
        mm, sums = queries_for(col, flt, key)
        yield mm, col, holds_nan(col)
        yield sums, col, False
    for expr in EXPRESSIONS:
        yield expression_query(expr, flt, key), expr, False
    for expr in MAX_EXPRESSIONS:
        yield expression_query(expr, flt, key), expr, True


def _check_cells(flt, key, segs, seg_ids, sign_matters, walk_check=None):
    """Runs every cell of one filter and key; returns the failures. A refusal is a failure outside the allowance and
    must name NaN."""
    bad = []
    grouped = key is not None
    for sql, col, refusable in _cells(flt, key):
        qc, blk, reason = _run(sql, segs)
        if blk is None:
            if not refusable:
                bad.append(f"{sql}: refused outside the NaN allowance ({reason})")
            elif "NaN" not in reason:
                bad.append(f"{sql}: refused without naming NaN ({reason})")
            continue
        n = sum(int(matched(special_segments()[i], flt).sum()) for i in seg_ids)
        if blk.stats.num_docs_scanned != n:
            bad.append(f"{sql}: num_docs_scanned {blk.stats.num_docs_scanned}, want {n}")
        if not (blk.filter_kernel_ms or 0) + (blk.agg_kernel_ms or 0) > 0:
            bad.append(f"{sql}: no kernel time -- did not run on the GPU")
        if walk_check is not None:
            bad += [f"{sql}: {m}" for m in walk_check(blk)]
        bad += check_block(qc, blk, wants(qc, col, flt, grouped, seg_ids), grouped, sign_matters, sql)
    return bad


def _report(bad):
    assert not bad, f"{len(bad)} failing cells:\n" + "\n".join(bad)


WALKS = {"chunks": ("0", "0", "0"), "batch": ("1", "0", "0"), "staged": ("1", "1", "0"),
         "staged_lds_dict": ("1", "1", "1")}


@pytest.mark.parametrize("fuse", ["0", "1"], ids=["unfused", "fused"])
@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("flt", list(FILTERS))
def test_gpu_special_doubles_aggregation(flt, walk, fuse, gpu_segments, monkeypatch):
    """Non-grouped, one segment: the per-64-doc chunk walk, the dense-tile batch walk plain / LDS-staged / with LDS
    dictionaries, each through the separate aggregation kernel and fused into the filter kernel. Non-grouped MIN / MAX
    are Math.min / Math.max folds: the sign of a zero counts."""
    db, st, ld = WALKS[walk]
    monkeypatch.setenv("PHIP_DENSE_BATCH", db)
    monkeypatch.setenv("PHIP_AGG_STAGE", st)
    monkeypatch.setenv("PHIP_AGG_LDS_DICT", ld)
    monkeypatch.setenv("PHIP_FUSE", fuse)

    def walk_check(blk):
        if fuse == "1":
            return [] if blk.fused and blk.agg_kernel_ms == 0.0 else \
                [f"PHIP_FUSE=1 but fused={blk.fused}, agg_kernel_ms={blk.agg_kernel_ms}"]
        return ["PHIP_FUSE=0 but the block reports itself fused"] if blk.fused else []

    _report(_check_cells(flt, None, gpu_segments[:1], (0,), True, walk_check))


def _filter_clause_expected(seg, col):
    f, v = seg.source["f"][1], seg.stored_values(col)
    return jf.fold_min(v[f < 50].tolist()), jf.fold_max(v[f >= 50].tolist()), int((f < 50).sum()) + int((f >= 50).sum())


@pytest.mark.parametrize("col", ["dn_p1", "dn_p1_r", "di_p1", "di_p1_r", "dz_p1_r"])
def test_gpu_special_doubles_filter_clause(col, gpu_segments):
    """MIN(c) FILTER (WHERE f < 50), MAX(c) FILTER (WHERE f >= 50): two filter programs in one pass."""
    seg = special_segments()[0]
    qc, blk, reason = _run(FILTER_CLAUSE.format(c=col), gpu_segments[:1])
    if blk is None:
        assert holds_nan(col) and "NaN" in reason, reason
        return
    mn, mx, n = _filter_clause_expected(seg, col)
    assert blk.stats.num_docs_scanned == n
    assert jf.same_double(blk.results[0], mn, True), (blk.results[0], mn)
    assert jf.same_double(blk.results[1], mx, True), (blk.results[1], mx)


GROUP_WALKS = {"lds_table": {}, "global_table": {"PHIP_GB_MODE": "global"}, "fused_hbm": {"PHIP_FUSED_GB": "2"},
               "fused_xcd": {"PHIP_FUSED_GB": "3"}, "fused_lds": {"PHIP_FUSED_GB": "4"}, "hash": {"PHIP_GB_HASH": "1"}}


def _group_walk_check(walk):
    def check(blk):
        out = []
        if walk in ("fused_hbm", "fused_xcd") and not blk.fused:
            out.append(f"{walk}: the block does not report itself fused")
        if blk.fused and blk.agg_kernel_ms != 0.0:
            out.append(f"{walk}: fused with agg_kernel_ms={blk.agg_kernel_ms}")
        return out
    return check


@pytest.mark.parametrize("walk", list(GROUP_WALKS))
@pytest.mark.parametrize("flt", list(FILTERS))
def test_gpu_special_doubles_group_by(flt, walk, gpu_segments, monkeypatch):
    """Grouped on the dictionary key g, one segment: the LDS table, the global table, the three fused tables and the
    hash table. Grouped MIN / MAX are compare folds: a NaN never wins, and P3 leaves the six other groups untouched."""
    for k, v in GROUP_WALKS[walk].items():
        monkeypatch.setenv(k, v)
    _report(_check_cells(flt, "g", gpu_segments[:1], (0,), False, _group_walk_check(walk)))


@pytest.mark.parametrize("walk", ["default", "hash"])
@pytest.mark.parametrize("flt", list(FILTERS))
def test_gpu_special_doubles_group_by_raw_key(flt, walk, gpu_segments, monkeypatch):
    """Grouped on gr, the same key stored raw (value - min keyed)."""
    monkeypatch.setenv("PHIP_GB_HASH", "1" if walk == "hash" else "0")
    _report(_check_cells(flt, "gr", gpu_segments[:1], (0,), False))


@pytest.mark.parametrize("key", [None, "g", "gr"], ids=["aggregation", "group_by", "group_by_raw_key"])
@pytest.mark.parametrize("flt", list(FILTERS))
def test_gpu_special_doubles_two_segments(flt, key, gpu_segments):
    """Both segments (their dictionaries differ): per-segment folds merged with the reference's comparison merges.
    Every column places its special values alike in both segments, so no cell depends on the merge order (see the
    module docstring for the one that would: a NaN matched in one segment only)."""
    _report(_check_cells(flt, key, gpu_segments, (0, 1), False))


def _double_compare_key(x):
    """Double.compare's total order: -0.0 below 0.0, NaN above +inf."""
    return (1, 0.0, 0) if x != x else (0, x, 0 if (x == 0 and np.signbit(x)) else 1)


def test_gpu_special_doubles_non_scan(gpu_segments):
    """No filter, dictionary columns: NonScanBasedAggregationOperator answers from the dictionary -- MIN its first
    value, MAX its last, in Double.compare order (so MAX of a NaN-holding column is NaN while MIN is its smallest
    number), whatever a scan would have folded."""
    seg = special_segments()[0]
    bad = []
    for col in (c for c in METRICS if not c.endswith("_r")):
        vals = sorted(set(seg.stored_values(col).tolist()), key=_double_compare_key)
        lo, hi = vals[0], vals[-1]
        if holds_nan(col):
            assert hi != hi and lo == lo
        qc, blk, reason = _run(f"SELECT MIN({col}), MAX({col}), MINMAXRANGE({col}), COUNT(*) FROM t", gpu_segments[:1])
        if blk is None:
            bad.append(f"{col}: refused ({reason})")
            continue
        mn, mx, (rlo, rhi), n = blk.results
        if not (jf.same_double(mn, lo, True) and jf.same_double(mx, hi, True) and jf.same_double(rlo, lo, True)
                and jf.same_double(rhi, hi, True) and n == seg.n):
            bad.append(f"{col}: got {blk.results}, want {(lo, hi, seg.n)}")
    _report(bad)


def test_gpu_special_doubles_refusal_reaches_the_cpu_plan_maker(gpu_segments):
    """A refused NaN cell goes to the configured CPU plan maker; the same query over a column without NaN does not."""
    from pinot_amd.engine.plan import GpuInstancePlanMaker

    class _CpuMaker:
        def __init__(self):
            self.calls = []

        def make_instance_plan(self, query, segments):
            self.calls.append(query)
            return ("cpu-plan", query)

    for col in ("dn_p2", "dm_p1_r", "fn_p3", "fm_p2_r"):
        _, blk, reason = _run(f"SELECT MAX({col}) FROM t WHERE f < 90", gpu_segments[:1])
        if blk is not None:
            continue  # (kernels that answer the cell exactly need no route)
        cpu = _CpuMaker()
        plan = GpuInstancePlanMaker(cpu_plan_maker=cpu).make_instance_plan(f"SELECT MAX({col}) FROM t WHERE f < 90",
                                                                           gpu_segments[:1])
        assert plan[0] == "cpu-plan" and len(cpu.calls) == 1 and "NaN" in reason
    cpu = _CpuMaker()
    op = GpuInstancePlanMaker(cpu_plan_maker=cpu).make_instance_plan("SELECT MAX(di_p1), SUM(dn_p1) FROM t WHERE f < 90",
                                                                     gpu_segments[:1])
    assert not cpu.calls
    blk = op.next_block()
    assert blk.results[0] == float("inf") and blk.results[1] != blk.results[1]
