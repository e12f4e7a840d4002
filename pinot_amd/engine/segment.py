"""HBM-resident segment (the GPU side of ImmutableSegmentLoader.load).

``GpuSegment(segment)`` hands every column's index buffers to ``phip_segment_load`` — the point
where the reference maps them (ImmutableSegmentLoader.java:222-280,
PhysicalColumnIndexContainer.java:44-68) — and keeps the host-side readers the plan needs
(dictionaries for predicate evaluation, the sorted index for doc ranges).
"""
import ctypes
import os

import numpy as np

from .. import _lib
from ..segment.creator import ImmutableSegment, read_chunk_forward
from ..segment.dictionary import Dictionary
from ..spi import DataType

# Dictionaries below this cardinality are matched on the host (Dfa.match_many over the padded dictionary matrix), the
# others on the device (phip_segment_match_dictionary). PINOT_AMD_STRMATCH_HOST_CARD overrides it: 0 = always the
# device, a huge value = always the host. Measured crossover: DESIGN.md §3 "String matching".
STRMATCH_HOST_CARD = 256

# The same choice for a time transform's comparison over a numeric dictionary (match_transform): below this cardinality
# query.time_transform.evaluate on the host, the others on the device (phip_segment_match_transform).
# PINOT_AMD_TRANSFORM_HOST_CARD overrides it, as above. The default is the string match's: the crossover of this pair is
# unmeasured (DESIGN.md §3 "Time transforms").
TRANSFORM_HOST_CARD = 256


class GpuSegment:
    def __init__(self, segment: ImmutableSegment, device: int = -1):
        lib = _lib.load()
        self.segment = segment
        self.name = segment.name
        self.num_docs = segment.num_docs
        self.device = device  # (-1: the library's default device)
        self._dicts = {}
        self._sorted = {}
        self._inv_offsets = {}
        self._specials = {}  # column -> (holds NaN, holds an infinity): real_specials
        self._intervals = {}  # column -> (min, max) or None: value_interval
        self._matches = {}  # (column, pattern) -> matching dict ids: match_dictionary
        self._transform_matches = {}  # (column, program, predicate) -> matching dict ids: match_transform
        self.transform_match_builds = 0  # id sets match_transform computed (not found kept)
        cols = list(segment.columns.values())
        descs = (_lib.ColumnDesc * max(len(cols), 1))()
        keep = []
        for i, ci in enumerate(cols):
            m = ci.metadata
            d = descs[i]
            name = m.name.encode()
            keep.append(name)
            d.name = name
            d.data_type = int(m.data_type)
            if getattr(m, "hll_log2m", 0):  # star-tree DISTINCTCOUNTHLL pair: register rows
                d.fwd_kind = _lib.FWD_HLL_REGISTERS
            elif not getattr(m, "is_single_value", True):
                if not m.has_dictionary:
                    raise _lib.UnsupportedOnGpu(f"raw (no-dictionary) multi-value column {m.name}")
                d.fwd_kind = _lib.FWD_FIXED_BIT_MV
                d.total_values = m.total_number_of_entries
                d.max_values_per_doc = m.max_number_of_multi_values
            elif not m.has_dictionary:
                d.fwd_kind = _lib.FWD_RAW_CHUNK
            elif m.is_sorted:
                d.fwd_kind = _lib.FWD_SORTED
            else:
                d.fwd_kind = _lib.FWD_FIXED_BIT
            d.cardinality = m.cardinality
            d.bits_per_value = m.hll_log2m if getattr(m, "hll_log2m", 0) else m.bits_per_element
            d.string_width = m.string_width
            for attr, buf in (("forward", ci.forward), ("dictionary", ci.dictionary), ("inverted", ci.inverted),
                              ("null_vector", getattr(ci, "null_vector", None))):
                if buf is None:
                    setattr(d, attr, None)
                    setattr(d, attr + "_bytes", 0)
                else:
                    arr = np.frombuffer(buf, dtype=np.uint8)
                    keep.append(arr)
                    setattr(d, attr, arr.ctypes.data if len(arr) else None)
                    setattr(d, attr + "_bytes", len(arr))
        sd = _lib.SegmentDesc()
        nm = segment.name.encode()
        sd.name = nm
        sd.device = device
        sd.num_docs = segment.num_docs
        sd.num_columns = len(cols)
        sd.columns = descs
        handle = ctypes.c_uint64(0)
        _lib.check(lib.phip_segment_load(ctypes.byref(sd), ctypes.byref(handle)))
        self.handle = handle.value
        del keep
        # star-tree indexes load with their segment (ImmutableSegmentLoader -> StarTreeIndexReader): the star-tree
        # documents are resident like any segment's columns
        self.star_trees = list(getattr(segment, "star_trees", []) or [])
        self.star_segments = [GpuSegment(t.docs, device) for t in self.star_trees]

    # ---- host-side readers (DataSource equivalents) -----------------------------------------
    def column_metadata(self, column):
        return self.segment.columns[column].metadata

    def has_null_vector(self, column) -> bool:
        """The column has a null value vector, i.e. some doc is null (NullValueVectorCreator writes none otherwise;
        DataSource.getNullValueVector() != null)."""
        ci = self.segment.columns.get(column)
        return ci is not None and bool(getattr(ci, "null_vector", None))

    def has_column(self, column):
        return column in self.segment.columns

    def dictionary(self, column) -> Dictionary:
        d = self._dicts.get(column)
        if d is None:
            ci = self.segment.columns[column]
            m = ci.metadata
            d = Dictionary(ci.dictionary, m.data_type, m.cardinality, m.string_width)
            self._dicts[column] = d
        return d

    def real_specials(self, column):
        """(holds NaN, holds an infinity) of a FLOAT / DOUBLE column, from what the segment knows without a scan of
        the docs where it can: a sorted dictionary keeps NaN last (Double.compare order) and the infinities at its
        ends; a raw column's chunks are read once, when a plan first asks, and the flags kept. (False, False) for
        the other types."""
        flags = self._specials.get(column)
        if flags is None:
            m = self.column_metadata(column)
            if m.data_type not in (DataType.FLOAT, DataType.DOUBLE) or getattr(m, "hll_log2m", 0):
                flags = (False, False)
            else:
                if m.has_dictionary:
                    v = self.dictionary(column).values
                    nan = bool(len(v)) and bool(np.isnan(v[-1]))
                    ends = v[[0, len(v) - 1 - nan]] if len(v) > nan else v[:0]
                else:
                    ends = v = read_chunk_forward(self.segment.columns[column].forward, m.data_type, self.num_docs)
                    nan = bool(np.isnan(v).any())
                flags = (nan, bool(np.isinf(ends).any()))
            self._specials[column] = flags
        return flags

    def value_interval(self, column):
        """(min, max) of a numeric column's values as floats, NaN left out -- the dictionary's ends, or one read of a
        raw column's chunks, kept; None for a column without docs or values. For a divisor's interval
        (plan._refuse_nan_extrema)."""
        if column not in self._intervals:
            m = self.column_metadata(column)
            if m.has_dictionary:
                v = np.asarray(self.dictionary(column).values)
            else:
                v = read_chunk_forward(self.segment.columns[column].forward, m.data_type, self.num_docs)
            v = np.asarray(v, dtype=np.float64)
            v = v[~np.isnan(v)]
            self._intervals[column] = (float(v.min()), float(v.max())) if len(v) else None
        return self._intervals[column]

    def match_dictionary(self, column, pattern, dfa) -> np.ndarray:
        """Sorted int32 dict ids of the dictionary STRING column's entries that ``dfa`` (query.regex_dfa.Dfa, compiled
        from ``pattern``) accepts -- what the reference's DictionaryBasedRegexpLikePredicateEvaluator finds out per
        scanned doc (RegexpLikePredicateEvaluatorFactory.java:74-76), once per entry. Kept per (column, pattern)."""
        key = (column, pattern)
        ids = self._matches.get(key)
        if ids is None:
            ci = self.segment.columns[column]
            m = ci.metadata
            card, width = m.cardinality, m.string_width
            host_card = int(os.environ.get("PINOT_AMD_STRMATCH_HOST_CARD", STRMATCH_HOST_CARD))
            if card < host_card:
                mat = np.frombuffer(ci.dictionary, dtype=np.uint8, count=card * width).reshape(card, width)
                hit = dfa.match_many(mat) if card else np.zeros(0, dtype=bool)
            else:
                blob = np.ascontiguousarray(dfa.to_blob(), dtype=np.int32)
                words = np.zeros(max((card + 63) // 64, 1), dtype=np.uint64)
                _lib.check(_lib.load().phip_segment_match_dictionary(
                    self.handle, column.encode(), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(blob),
                    words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(words)))
                hit = np.unpackbits(words.view(np.uint8), bitorder="little")[:card].astype(bool)
            ids = np.flatnonzero(hit).astype(np.int32)
            if len(self._matches) < 1024:
                self._matches[key] = ids
        return ids

    def match_transform(self, column, program, predicate) -> np.ndarray:
        """Sorted int32 dict ids of the dictionary INT / LONG column's entries v whose time transform
        (query.time_transform.Program ``program``) passes ``predicate`` = (kind, lo, hi, members) as
        time_transform.integer_predicate resolves it -- what the reference's ExpressionFilterOperator finds out per
        scanned doc, once per entry. Kept per (column, program, predicate)."""
        from ..query import time_transform as tt
        program = tt.Program(*program)
        kind, lo, hi, members = predicate
        key = (column, program, (kind, int(lo), int(hi), tuple(members)))
        ids = self._transform_matches.get(key)
        if ids is None:
            self.transform_match_builds += 1
            card = self.column_metadata(column).cardinality
            host_card = int(os.environ.get("PINOT_AMD_TRANSFORM_HOST_CARD", TRANSFORM_HOST_CARD))
            if card < host_card:
                vals = tt.evaluate(program, np.asarray(self.dictionary(column).values, dtype=np.int64))
                hit = tt.match_values(vals, kind, lo, hi, np.asarray(members, dtype=np.int64))
            else:
                t = _lib.TimeTransform(*program)
                pr = _lib.TransformPredicate()
                vals = np.ascontiguousarray(members, dtype=np.int64)
                if kind == "range":
                    pr.kind = _lib.TT_PRED_RANGE
                    pr.lower, pr.upper, pr.lower_inclusive, pr.upper_inclusive = int(lo), int(hi), 1, 1
                else:
                    pr.kind = _lib.TT_PRED_SET
                    pr.exclusive = int(kind == "not_set")
                    pr.values = vals.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if len(vals) else None
                    pr.num_values = len(vals)
                words = np.zeros(max((card + 63) // 64, 1), dtype=np.uint64)
                _lib.check(_lib.load().phip_segment_match_transform(
                    self.handle, column.encode(), ctypes.byref(t), ctypes.byref(pr),
                    words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(words)))
                hit = np.unpackbits(words.view(np.uint8), bitorder="little")[:card].astype(bool)
            ids = np.flatnonzero(hit).astype(np.int32)
            if len(self._transform_matches) < 1024:
                self._transform_matches[key] = ids
        return ids

    def derived_info(self):
        """(count, bytes, builds) of the segment's derived value columns (phip_segment_derived_info): how many it holds,
        their HBM bytes, and the materialise launches since load."""
        n, b, k = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.load().phip_segment_derived_info(self.handle, ctypes.byref(n), ctypes.byref(b), ctypes.byref(k)))
        return n.value, b.value, k.value

    def inverted_bytes(self, column, dict_ids) -> int:
        """Bytes of the inverted-index bitmaps of `dict_ids` (the bytes an inverted leaf reads)."""
        if column not in self._inv_offsets:
            ci = self.segment.columns[column]
            card = ci.metadata.cardinality
            self._inv_offsets[column] = np.frombuffer(ci.inverted[:4 * (card + 1)], dtype=">u4").astype(np.int64)
        offs = self._inv_offsets[column]
        ids = np.asarray(dict_ids, dtype=np.int64)
        return int(np.sum(offs[ids + 1] - offs[ids])) if len(ids) else 0

    def sorted_doc_range(self, column, dict_id):
        """SortedIndexReaderImpl.getDocIds(dictId) (SortedIndexReaderImpl.java:114-116): inclusive pair."""
        p = self._sorted.get(column)
        if p is None:
            p = np.frombuffer(self.segment.columns[column].forward, dtype=">i4").astype(np.int64).reshape(-1, 2)
            self._sorted[column] = p
        return int(p[dict_id, 0]), int(p[dict_id, 1])

    def device_bytes(self) -> int:
        out = ctypes.c_uint64(0)
        _lib.check(_lib.load().phip_segment_device_bytes(self.handle, ctypes.byref(out)))
        return out.value

    def destroy(self):
        for s in getattr(self, "star_segments", []):
            s.destroy()
        self.star_segments = []
        if self.handle:
            _lib.check(_lib.load().phip_segment_unload(self.handle))
            self.handle = 0
