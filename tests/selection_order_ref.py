"""CPU restatement of a selection ORDER BY (SelectionOrderByOperator + SelectionOrderByCombineOperator) for the tests.

The oracle's selection-only execution of the same query -- the block expressions as its select list, no ORDER BY, a
LIMIT above every doc count -- yields every matched row in (segment, doc) order. Those rows are stable-sorted by the
Java comparators, term by term: INT / LONG by value, FLOAT / DOUBLE by Double.compare (-0.0 < 0.0, every NaN equal
and above +inf), STRING by String.compareTo (UTF-16 code units). A DESC term reverses that term's comparison only, so
rows equal on every term keep (segment, doc) order: the tie rule of GpuSelectionOperator. The first K = OFFSET + LIMIT
rows are the block. Statistics by SelectionOrderByOperator's formulas:

    numDocsScanned              = matched docs, all segments
    numEntriesScannedPostFilter = matched x (distinct columns of the order-by expressions)
                                  + sum over segments of min(matched_seg, K) x (distinct columns only the other
                                    block expressions read)
    the rest as the selection-only execution reports them.
"""
import functools
import struct

from oracle import executor
from pinot_amd.engine.results import ExecutionStatistics, SelectionResultsBlock
from pinot_amd.query.context import QueryContext, columns_of
from pinot_amd.query.sql import parse


def double_compare_key(v):
    """An integer that orders doubles as Double.compare does."""
    if v != v:
        u = 0x7FF8000000000000
    else:
        u = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return (u ^ 0xFFFFFFFFFFFFFFFF) if u >> 63 else (u | (1 << 63))


def _key(v):
    if isinstance(v, float):
        return double_compare_key(v)
    if isinstance(v, str):
        return v.encode("utf-16-be")
    return int(v)


def all_rows(qc, raws):
    """(block names, block types, every matched row in (segment, doc) order, matched docs per segment, the
    selection-only statistics) of the ORDER BY selection ``qc``."""
    exprs = qc.selection_block_expressions(list(raws[0].columns))
    plain = QueryContext(qc.table, [(e, None) for e in exprs], [], qc.filter, [], [], limit=1 << 40,
                         options=dict(qc.options))
    rows, matched, names, types, stats = [], [], None, None, None
    for r in raws:
        blk, _ = executor.execute(plain, [r])
        names, types = blk.column_names, blk.column_types
        rows.extend(blk.rows)
        matched.append(blk.num_rows)
        if stats is None:
            stats = blk.stats
        else:
            stats.merge(blk.stats)
    return exprs, names, types, rows, matched, stats


def restate(sql_or_qc, raws):
    """The expected SelectionResultsBlock of an ORDER BY selection over the raw segments."""
    qc = parse(sql_or_qc) if isinstance(sql_or_qc, str) else sql_or_qc
    assert qc.is_selection and qc.order_by and qc.limit > 0
    exprs, names, types, rows, matched, plain = all_rows(qc, raws)
    terms = [(names.index(str(ob.expression)), ob.ascending) for ob in qc.order_by]

    def compare(a, b):
        for i, asc in terms:
            ka, kb = _key(a[i]), _key(b[i])
            if ka != kb:
                return (-1 if ka < kb else 1) * (1 if asc else -1)
        return 0

    rows = sorted(rows, key=functools.cmp_to_key(compare))  # stable: ties keep (segment, doc) order
    keep = qc.offset + qc.limit
    rows = rows[:keep]
    order_cols, rest_cols = set(), set()
    for ob in qc.order_by:
        order_cols.update(columns_of(ob.expression))
    for e in exprs:
        rest_cols.update(c for c in columns_of(e) if c not in order_cols)
    total = sum(matched)
    stats = ExecutionStatistics(total, plain.num_entries_scanned_in_filter,
                                total * len(order_cols) + sum(min(m, keep) for m in matched) * len(rest_cols),
                                plain.num_total_docs, plain.num_segments_processed, sum(1 for m in matched if m > 0))
    cols = [[r[j] for r in rows] for j in range(len(names))]
    return SelectionResultsBlock(list(names), list(types), cols, stats)
