"""The device trim (trim.hip: order_keys_kernel, term_keys_kernel, key_order_kernel, trim_gather_kernel) over the
Double.compare ladder of tests/order_data.py, with the trim boundary at every position 5..15 from both ends.

Expected values come from java_fold over the fixture's stored values (tests/test_order_by_specials.py ``Ladder``) --
never from the oracle, ``trim_groups`` or a second run of the library; the HLL estimate is ``reduce.hll_cardinality``
over registers offered by the oracle's route, a restatement separate from the kernel's ``hll_estimate``.

``LIMIT 1`` with ``SET minServerGroupTrimSize = t`` makes the trim size exactly t. Per query: the block is trimmed to t
groups; must_keep <= kept <= must_keep + may_keep (java_fold.top_records: equality where the ORDER BY ends in a key);
every kept group carries the expected intermediates (doubles by same_double with the zero's sign, counts and HLL
registers exactly); the broker's rows over the trimmed block are the first LIMIT of the expected order; the kernels
ran. Ties at the boundary: the device keeps the lowest group index -- not the smallest key under the hash table --, the
reference whatever its heap holds; the assertion allows any member of the tied class.
"""
import functools

import numpy as np
import pytest

from pinot_amd.engine.plan import GpuCombineOperator, GpuInstancePlanMaker
from pinot_amd.engine.reduce import reduce_blocks
from pinot_amd.query.sql import parse
from tests import java_fold as jf
from tests import order_data as od
from tests.test_order_by_specials import (AGGS, KEYS, _check_rows, aggregation_expr, flipped, ladder, order_terms,
                                          same_value, select_list)

pytestmark = pytest.mark.gpu

SINGLE_TERMS = ["SUM(s)", "SUM(s_r)", "SUM(sf)", "MIN(x)", "MIN(x_r)", "MAX(x)", "MAX(x_r)", "COUNT(*)"]
GENERAL_TERMS = ["AVG(s)", "MINMAXRANGE(x)", "DISTINCTCOUNTHLL(h), g", "SUM(s) DESC, g", "gd DESC, SUM(s)",
                 "COUNT(*), AVG(s) DESC, g"]
KEY_TERMS = ["gd", "gd DESC", "gd, g DESC"]
PATH = {**{o: "single" for o in SINGLE_TERMS}, **{o: "general" for o in GENERAL_TERMS}, **{o: "keys" for o in KEY_TERMS}}
WALKS = [(h, key, nseg, filtered) for h in ("0", "1") for key in ("g", "gr") for nseg in (1, 2)
         for filtered in (True, False)]


def _walk_id(w):
    h, key, nseg, filtered = w
    return f"{'hash' if h == '1' else 'table'}-{key}-{nseg}seg-{'filtered' if filtered else 'unfiltered'}"


@pytest.fixture(scope="module")
def gpu_segments(gpu_lib):
    from pinot_amd.engine.segment import GpuSegment
    segs = [GpuSegment(s.raw) for s in od.segments()]
    yield segs
    for s in segs:
        s.destroy()


def _core(op):
    """The GpuCombineOperator that owns the prepared plan, under the operators that wrap it."""
    while not isinstance(op, GpuCombineOperator):
        op = getattr(op, "one_pass", None) or op.__dict__.get("inner") or op.__dict__["op"]
    return op


def _with_key(order, key):
    """The ORDER BY with the group key ``g`` replaced by ``key``."""
    return ", ".join((key if e == "g" else e) + ("" if asc else " DESC") for e, asc in order_terms(order))


def _check_intermediates(qc, blk, keys, lad, tag):
    """Every kept group's key values and intermediates against java_fold's."""
    bad = []
    by_g = {od.G[i]: i for i in range(od.NG)}
    for key, vals in blk.groups.items():
        i = by_g.get(key[0])
        if i is None:
            bad.append(f"{tag}: unknown key {key}")
            continue
        for k, kv in zip(keys[1:], key[1:]):
            if not same_value(kv, lad.value(k, i)):
                bad.append(f"{tag}: group {key[0]} has {k} = {kv!r}, want {lad.value(k, i)!r}")
        for ag, got in zip(qc.aggregations, vals):
            e = aggregation_expr(ag)
            want = lad.intermediate(e, i)
            if ag.function == "count":
                ok = isinstance(got, int) and got == want
            elif ag.function == "distinctcounthll":
                ok = np.array_equal(got, want)
            elif ag.function == "avg":
                ok = jf.same_double(got[0], want[0], True) and int(got[1]) == want[1]
            elif ag.function == "minmaxrange":
                ok = jf.same_double(got[0], want[0], True) and jf.same_double(got[1], want[1], True)
            else:
                ok = jf.same_double(got, want, True)
            if not ok:
                bad.append(f"{tag}: group {key[0]} has {e} = {got!r}, want {want!r}")
    return bad


def _run(order, key, limit, trim, segs, lad, path=None, options=""):
    """One query; returns its failing cells."""
    keys = (key, "gd") if any(e == "gd" for e, _ in order_terms(order)) else (key,)
    sel = select_list(order, keys)
    where = " WHERE f < 99" if lad.filtered else ""
    sql = (f"SET minServerGroupTrimSize = {trim if limit == 1 else 5}; {options}SELECT {', '.join(sel)} FROM t{where} "
           f"GROUP BY {', '.join(keys)} ORDER BY {order} LIMIT {limit}")
    tag = f"{order} / trim {trim} / LIMIT {limit}"
    qc = parse(sql)
    op = GpuInstancePlanMaker().make_instance_plan(qc, segs)
    try:
        if path is not None:
            spec = _core(op)._trim_spec()
            took = "general" if spec[4] else "keys" if spec[3] else "single" if spec[0] >= 0 else "none"
            if took != path or spec[2] != trim:
                return [f"{tag}: the plan orders by the {took} path with trim size {spec[2]}, expected {path}, {trim}"]
        blk = op.next_block()
    finally:
        close = getattr(op, "close", None)
        if close is not None:
            close()
    bad = []
    if not (getattr(blk, "num_groups_trimmed", False) and len(blk.groups) == trim):
        bad.append(f"{tag}: num_groups_trimmed={getattr(blk, 'num_groups_trimmed', None)}, {len(blk.groups)} groups")
    n = sum(lad.value("COUNT(*)", i) for i in range(od.NG))
    if blk.stats.num_docs_scanned != n:
        bad.append(f"{tag}: num_docs_scanned {blk.stats.num_docs_scanned}, want {n}")
    if not (blk.filter_kernel_ms or 0) + (blk.agg_kernel_ms or 0) > 0:
        bad.append(f"{tag}: no kernel time -- did not run on the GPU")
    by_g = {od.G[i]: i for i in range(od.NG)}
    kept = {by_g.get(k[0]) for k in blk.groups}
    must, may = jf.top_records(range(od.NG), lad.terms(order), trim)
    if not set(must) <= kept <= set(must) | set(may):
        bad.append(f"{tag}: kept {sorted(od.G[i] for i in kept if i is not None)}, must keep "
                   f"{sorted(od.G[i] for i in must)}, may keep {sorted(od.G[i] for i in may)}")
    bad += _check_intermediates(qc, blk, keys, lad, tag)
    rows = reduce_blocks(qc, [blk]).rows
    if len(rows) != limit:
        bad.append(f"{tag}: {len(rows)} rows")
    bad += [f"{tag}: {m}" for m in _check_rows(rows, order, lad, sel)]
    if lad.is_total(order) and [r[0] for r in rows] != [od.G[i] for i in lad.ordered(order)[:limit]]:
        bad.append(f"{tag}: rows {[r[0] for r in rows]}, want {[od.G[i] for i in lad.ordered(order)[:limit]]}")
    return bad


def _report(bad):
    assert not bad, f"{len(bad)} failing cells:\n" + "\n".join(bad)


@pytest.mark.parametrize("walk", WALKS, ids=_walk_id)
@pytest.mark.parametrize("order", SINGLE_TERMS + GENERAL_TERMS + KEY_TERMS)
def test_gpu_order_by_specials(order, walk, gpu_segments, monkeypatch):
    """Every term as written and with every direction reversed, the trim size 5..15 with LIMIT 1, then LIMIT 2 and 3
    (trim sizes 10 and 15)."""
    use_hash, key, nseg, filtered = walk
    monkeypatch.setenv("PHIP_GB_HASH", use_hash)
    lad = ladder(tuple(range(nseg)), filtered)
    segs = gpu_segments[:nseg]
    path = PATH[order]
    order = _with_key(order, key)
    bad = []
    for o in (order, flipped(order)):
        for t in range(5, od.NG):
            bad += _run(o, key, 1, t, segs, lad, path if t == 5 else None)
    bad += _run(order, key, 2, 10, segs, lad)
    bad += _run(flipped(order), key, 3, 15, segs, lad)
    _report(bad)


@pytest.mark.parametrize("order", ["SUM(s_r) DESC, g", "AVG(s), g DESC"])
def test_gpu_order_by_specials_segment_trim(order, gpu_segments):
    """SET minSegmentGroupTrimSize = 6: each segment keeps its top 6 by the ORDER BY (a total order: no tie to choose
    from), the survivors' partials merge, and the server trim keeps 5 of them."""
    lads = [ladder((k,), True) for k in (0, 1)]
    qc = parse(f"SET minSegmentGroupTrimSize = 6; SET minServerGroupTrimSize = 5; SELECT g, SUM(s_r), AVG(s), COUNT(*) "
               f"FROM t WHERE f < 99 GROUP BY g ORDER BY {order} LIMIT 1")
    op = GpuInstancePlanMaker().make_instance_plan(qc, gpu_segments)
    try:
        blk = op.next_block()
    finally:
        op.close()
    assert getattr(blk, "segment_trimmed", False)
    exprs = [aggregation_expr(a) for a in qc.aggregations]
    merged = {}
    for lad in lads:   # (the reference's merges: SUM adds, AVG adds both, COUNT adds)
        for i in lad.ordered(order)[:6]:
            part = [lad.intermediate(e, i) for e in exprs]
            if i in merged:
                part = [(a[0] + b[0], a[1] + b[1]) if isinstance(a, tuple) else a + b for a, b in zip(merged[i], part)]
            merged[i] = part

    def value(e, i):
        if e in KEYS:
            return od.G[i]
        v = merged[i][exprs.index(e)]
        return od.final(AGGS[e][0], v)

    terms = [(functools.partial(value, e), asc) for e, asc in order_terms(order)]
    must, may = jf.top_records(sorted(merged), terms, 5)
    assert len(must) == 4 and len(may) == 1
    want = set(must) | set(may)
    assert blk.num_groups_trimmed and {od.G.index(k[0]) for k in blk.groups} == want
    for key, vals in blk.groups.items():
        for e, got, exp in zip(exprs, vals, merged[od.G.index(key[0])]):
            if isinstance(exp, tuple):
                assert jf.same_double(got[0], exp[0], True) and int(got[1]) == exp[1], (key, e, got, exp)
            elif isinstance(exp, int):
                assert got == exp, (key, e, got, exp)
            else:
                assert jf.same_double(got, exp, True), (key, e, got, exp)
    assert reduce_blocks(qc, [blk]).rows[0][0] == od.G[(must + may)[0]]
    assert (blk.filter_kernel_ms or 0) + (blk.agg_kernel_ms or 0) > 0
