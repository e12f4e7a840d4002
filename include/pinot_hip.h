/*
 * pinot_hip.h -- C ABI of libpinot_hip.so, the MI355X-native segment query hot path.
 *
 * Drop-in boundary. The reference's Java server keeps its operator surface and
 * calls these entry points through Java 21 FFM (INTEGRATION.md shows the bindings):
 *
 *   phip_segment_load    <- ImmutableSegmentLoader.load
 *                           (pinot-segment-local/.../indexsegment/immutable/ImmutableSegmentLoader.java:155-190,
 *                           222-280): per column the forward index, dictionary and inverted index
 *                           buffers that PhysicalColumnIndexContainer (…/segment/index/column/
 *                           PhysicalColumnIndexContainer.java:44-68) maps, handed over as raw bytes
 *                           (PinotDataBuffer.toDirectByteBuffer, pinot-segment-spi/.../memory/
 *                           PinotDataBuffer.java:671-696) and pinned in HBM.
 *   phip_segment_unload  <- IndexSegment.destroy
 *   phip_query           <- InstancePlanMakerImplV2.makeInstancePlan
 *                           (pinot-core/.../plan/maker/InstancePlanMakerImplV2.java:172-199) when the
 *                           query option selects the GPU: one call replaces, for all segments of the
 *                           query, FilterPlanNode/BaseFilterOperator.getTrues
 *                           (pinot-core/.../operator/filter/BaseFilterOperator.java:85-93),
 *                           AggregationOperator.getNextBlock (…/operator/query/AggregationOperator.java:63-80),
 *                           GroupByOperator.getNextBlock (…/operator/query/GroupByOperator.java:100-140)
 *                           and the CombineOperator merge (…/operator/combine/BaseSingleBlockCombineOperator.java:58-162).
 *                           Results are the intermediate values AggregationResultsBlock /
 *                           GroupByResultsBlock carry (…/operator/blocks/results/).
 *   phip_filter_bitmap   <- BaseFilterOperator.getTrues / getBitmaps for one segment (doc-id set as
 *                           64-doc bitmap words; the bit for doc d is bit d%64 of word d/64).
 *
 * Conventions: every function returns int32_t status (PHIP_OK = 0); on error the calling
 * thread's message is available from phip_last_error(). Host buffers passed in are borrowed for
 * the duration of the call only; the library owns all device memory. All entry points are
 * thread-safe (per-device mutex). No HIP/torch types cross the boundary.
 */
#ifndef PINOT_HIP_H_
#define PINOT_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
#define PHIP_EXTERN extern "C"
#else
#define PHIP_EXTERN extern
#endif
#define PHIP_API PHIP_EXTERN __attribute__((visibility("default")))

/* ---- status ------------------------------------------------------------------------------ */
#define PHIP_OK 0
#define PHIP_ERR_INVALID 1     /* malformed descriptor / plan */
#define PHIP_ERR_HIP 2         /* a HIP runtime call failed */
#define PHIP_ERR_UNSUPPORTED 3 /* shape outside the GPU subset: caller falls back to the Java path */
#define PHIP_ERR_NOT_FOUND 4   /* unknown segment handle or column */
#define PHIP_ERR_NO_DEVICE 5   /* no usable GPU */
#define PHIP_ERR_TIMEOUT 6     /* the plan's deadline passed (QueryTimeoutException: BaseSingleBlockCombineOperator
                                  .java:137-144 checks QueryContext.getEndTimeMs) */
#define PHIP_ERR_CANCELLED 7   /* phip_plan_cancel stopped the execution (QueryCancelledException) */

/* ---- stored data types (FieldSpec.DataType, single-value) ---------------------------------- */
#define PHIP_TYPE_INT 0
#define PHIP_TYPE_LONG 1
#define PHIP_TYPE_FLOAT 2
#define PHIP_TYPE_DOUBLE 3
#define PHIP_TYPE_STRING 4

/* ---- forward index encodings -------------------------------------------------------------- */
#define PHIP_FWD_FIXED_BIT 0 /* FixedBitSVForwardIndexWriter: ceil(N*b/8) BE bytes, MSB first */
#define PHIP_FWD_SORTED 1    /* SortedIndexReaderImpl: card x (start,end) BE int32, inclusive */
#define PHIP_FWD_HLL_REGISTERS 3 /* per doc 2^bits_per_value u8 HyperLogLog registers (a star-tree DISTINCTCOUNTHLL
                                  * function-column pair): DISTINCTCOUNTHLL max-merges them; no other use */
#define PHIP_FWD_RAW_CHUNK 2 /* BaseChunkForwardIndexWriter v2/v3 fixed-width chunks (and v4/v5 power-of-two chunks,
                              * FixedBytePower2ChunkSVForwardIndexReader): PASS_THROUGH, or SNAPPY / LZ4 /
                              * LZ4_LENGTH_PREFIXED / ZSTANDARD / GZIP decoded on the GPU at load (a malformed chunk
                              * fails the load); v1 (4-int header, SNAPPY chunks: BaseChunkForwardIndexReader.java:86-95)
                              * as well. A STRING column: VarByteChunkForwardIndexWriter v1..v3 chunks (per chunk
                              * numDocsPerChunk BE int start offsets, then the UTF-8 bytes), any codec */

#define PHIP_FWD_FIXED_BIT_MV 4 /* a dictionary-encoded multi-value column, FixedBitMVForwardIndexWriter: numChunks BE
                                * int chunk offsets (docsPerChunk = ceil(2048 / (float)(total_values / num_docs)), the
                                * inner division an integer one), a bitset of total_values bits with a bit (MSB first) at
                                * each doc's first value, then the total_values dict ids bit-packed as PHIP_FWD_FIXED_BIT
                                * packs them. A buffer that starts with 0xffabcdef is the entry-dictionary encoding
                                * (FixedBitMVEntryDictForwardIndexWriter): PHIP_ERR_UNSUPPORTED. Every doc has at least
                                * one value: a bitset whose set bits are not one per doc fails the load. Resident as the packed ids plus num_docs + 1 u32 value offsets.
                                * Filter leaves (PHIP_LEAF_DICT_RANGE / DICT_SET / INVERTED) match a doc when ANY of its
                                * values matches, an exclusive leaf when NONE of its values is in the set
                                * (BaseDictionaryBasedPredicateEvaluator.applyMV); an aggregation reads the column only
                                * through a row reduction (phip_derived_column.reduction). No null vector; not a group-by
                                * key, a select expression or an operand of arithmetic (PHIP_ERR_UNSUPPORTED). */

typedef struct phip_column_desc {
  const char *name;
  int32_t data_type;      /* PHIP_TYPE_* */
  int32_t fwd_kind;       /* PHIP_FWD_* */
  int32_t cardinality;    /* dictionary length (0 for raw columns) */
  int32_t bits_per_value; /* fixed-bit width: getNumBitsPerValue(card-1) */
  int32_t string_width;   /* STRING dictionary: bytes per '\0'-padded entry */
  int32_t reserved;
  const uint8_t *forward;
  uint64_t forward_bytes;
  const uint8_t *dictionary; /* BE fixed-width sorted values (NULL for raw columns) */
  uint64_t dictionary_bytes;
  const uint8_t *inverted; /* (card+1) BE u32 offsets + portable Roaring bitmaps, or NULL */
  uint64_t inverted_bytes;
  /* Null value vector (NullValueVectorReaderImpl: `<column>.bitmap.nullvalue`, one portable Roaring bitmap of the
   * docs whose value is null; NullValueVectorCreator writes it only when some doc is null), or NULL. Kept in HBM as
   * dense doc words for PHIP_LEAF_NULL leaves. */
  const uint8_t *null_vector;
  uint64_t null_vector_bytes;
  int64_t total_values;       /* PHIP_FWD_FIXED_BIT_MV: the values of all docs (totalNumberOfEntries); else unused */
  int32_t max_values_per_doc; /* PHIP_FWD_FIXED_BIT_MV: the longest row (maxNumberOfMultiValues); else unused */
  int32_t reserved_mv;
} phip_column_desc;

typedef struct phip_segment_desc {
  const char *name;
  int32_t device;      /* device ordinal, -1 = current default device */
  int32_t num_docs;
  int32_t num_columns;
  int32_t reserved;
  const phip_column_desc *columns;
} phip_segment_desc;

/* ---- filter program ----------------------------------------------------------------------
 * Per segment, a preorder tree: an AND/OR node is followed by its num_children subtrees; NOT by
 * one subtree. Leaves carry the per-segment outcome of the reference's PredicateEvaluator
 * (dictionary ids are per segment): RangePredicateEvaluatorFactory (dict-id range [lo,hi)),
 * In/NotIn/Eq/NotEq evaluators (dict-id set), SortedIndexBasedFilterOperator (doc ranges) or
 * InvertedIndexFilterOperator (dict ids whose bitmaps are OR-ed, complemented if exclusive). */
#define PHIP_NODE_LEAF 0
#define PHIP_NODE_AND 1
#define PHIP_NODE_OR 2
#define PHIP_NODE_NOT 3

#define PHIP_LEAF_MATCH_ALL 0  /* predicate alwaysTrue for this segment */
#define PHIP_LEAF_MATCH_NONE 1 /* predicate alwaysFalse for this segment */
#define PHIP_LEAF_DICT_RANGE 2 /* scan forward index: lo <= dictId < hi */
#define PHIP_LEAF_DICT_SET 3   /* scan forward index: dictId in ids (xor exclusive) */
#define PHIP_LEAF_DOC_RANGES 4 /* ids = count x (startDoc, endDoc) inclusive, sorted, disjoint */
#define PHIP_LEAF_INVERTED 5   /* OR of inverted-index bitmaps of ids (xor exclusive) */
/* Raw (no-dictionary) columns, value-based (RawValueBasedPredicateEvaluator, ScanBasedFilterOperator.java:58-66).
 * ids points at `count` int32 words holding a phip_raw_range (RAW_RANGE) or count/2 int64 values -- doubles for
 * FLOAT/DOUBLE columns -- (RAW_SET, xor exclusive). */
#define PHIP_LEAF_RAW_RANGE 6
#define PHIP_LEAF_RAW_SET 7
/* Raw STRING columns (var-byte chunks): the values compared in String.compareTo order. ids points at `count` int32
 * words: RAW_STRING_RANGE = [lo_len][hi_len][lo_inclusive][hi_inclusive][lo UTF-8 bytes][hi UTF-8 bytes], a length
 * of -1 = unbounded (StringRawValueBasedRangePredicateEvaluator, RangePredicateEvaluatorFactory.java); RAW_STRING_SET
 * = [n][n + 1 byte offsets][the n values' UTF-8 bytes] (raw EQ / NOT_EQ / IN / NOT_IN, xor exclusive). */
#define PHIP_LEAF_RAW_STRING_RANGE 8
#define PHIP_LEAF_RAW_STRING_SET 9
/* The column's null value vector (IS NULL: BitmapBasedFilterOperator over NullValueVectorReader.getNullBitmap,
 * FilterPlanNode.java:294-307; exclusive = IS NOT NULL). A column without a null vector matches no doc (all docs when
 * exclusive). With enableNullHandling the host composes these with the other leaves (BaseColumnFilterOperator's
 * trues AND NOT nulls, the And / Or / Not operators' getFalses), so the library needs nothing else for nulls. */
#define PHIP_LEAF_NULL 10
/* REGEXP_LIKE / LIKE over a raw STRING column (RegexpLikePredicateEvaluatorFactory's RawValueBasedRegexpLike-
 * PredicateEvaluator, RegexpLikePredicateEvaluatorFactory.java:108-110: Matcher.reset(value).find() per scanned doc;
 * LIKE arrives as REGEXP_LIKE, RequestContextUtils.java:231-236). ids points at `count` int32 words holding a DFA
 * blob (below); a doc matches when the DFA accepts the value's UTF-8 bytes (xor exclusive). The library walks the DFA
 * over the column's resident bytes in a pass of its own before the filter launch (strmatch.hip) and hands the filter
 * kernels dense doc words, as for an inverted leaf. numEntriesScannedInFilter counts num_docs per such leaf of every
 * unpruned (segment, program) entry: ScanBasedFilterOperator scans every doc (FilterOperatorUtils.java:108-117 makes a
 * REGEXP_LIKE leaf without an FST index a scan, whatever other index the column has). */
#define PHIP_LEAF_RAW_STRING_MATCH 11

/* ---- DFA blob -----------------------------------------------------------------------------
 * A complete deterministic automaton over bytes with find() semantics built in (the caller's compiler adds the
 * unanchored prefix loop and the absorbing accept state): a value matches when the walk from `start` over all its
 * bytes ends in an accepting state. int32 words, little-endian:
 *   [0] PHIP_STRMATCH_VERSION   [1] S = states   [2] C = byte classes   [3] start state
 *   ceil(S / 32) accept words: bit s % 32 of word s / 32 = state s accepts
 *   64 words = 256 bytes: the class (< C) of every byte value
 *   S x C uint16 transitions, row-major (state, class) -> state (< S), padded with one zero u16 to a whole word
 * The library checks every field before any launch (PHIP_ERR_INVALID otherwise): the version, 1 <= S <=
 * PHIP_STRMATCH_MAX_STATES, 1 <= C <= 256, S x C x 2 <= PHIP_STRMATCH_MAX_TABLE_BYTES, start < S, every class < C,
 * every transition < S, and that `count` is exactly the blob's word count; no kernel depends on the caller for staying
 * inside its table. A Java caller can fill the blob from Lucene's ByteRunAutomaton.
 * The caps are what one workgroup's LDS holds beside the waves' staging windows with two workgroups resident per CU. */
#define PHIP_STRMATCH_VERSION 1
#define PHIP_STRMATCH_MAX_STATES 4096
#define PHIP_STRMATCH_MAX_TABLE_BYTES 65536

/* In phip_filter_node.exclusive of a DICT_RANGE / DICT_SET leaf: keep the leaf a scan of the forward index even when its
 * ids are none or all of the dictionary's, where the library otherwise folds it to MATCH_NONE / MATCH_ALL and may prune
 * the segment. A dictionary REGEXP_LIKE leaf sets it: the reference's evaluator is never always-true / always-false and
 * its leaf always scans (FilterOperatorUtils.java:108-117), so numEntriesScannedInFilter counts the scan. */
#define PHIP_LEAF_FLAG_ALWAYS_SCAN 2

typedef struct phip_raw_range {
  int64_t lo_int, hi_int; /* INT/LONG columns: lo_int <= v <= hi_int */
  double lo_real, hi_real; /* FLOAT/DOUBLE columns, with the inclusive flags below */
  int32_t lo_inclusive, hi_inclusive;
} phip_raw_range;

typedef struct phip_filter_node {
  int32_t op;           /* PHIP_NODE_* */
  int32_t num_children; /* AND/OR */
  int32_t leaf_kind;    /* PHIP_LEAF_* */
  int32_t column;       /* index into phip_query_desc.columns */
  int32_t lo, hi;       /* DICT_RANGE */
  int32_t exclusive;    /* DICT_SET / INVERTED / RAW_SET / RAW_STRING_SET / RAW_STRING_MATCH / NULL: bit 0 = match the
                         * complement; DICT_RANGE / DICT_SET: | PHIP_LEAF_FLAG_ALWAYS_SCAN */
  int32_t count;        /* number of ids (DICT_SET/INVERTED) or of ranges (DOC_RANGES) */
  const int32_t *ids;
} phip_filter_node;

/* ---- aggregations ------------------------------------------------------------------------- */
#define PHIP_AGG_COUNT 0 /* CountAggregationFunction */
#define PHIP_AGG_SUM 1   /* SumAggregationFunction (int64 exact for INT/LONG inputs, f64 otherwise) */
#define PHIP_AGG_MIN 2   /* MinAggregationFunction (default +inf) */
#define PHIP_AGG_MAX 3   /* MaxAggregationFunction (default -inf) */
#define PHIP_AGG_HLL 4   /* DistinctCountHLLAggregationFunction: HyperLogLog(log2m) registers */
#define PHIP_AGG_DISTINCT 5 /* DistinctCountAggregationFunction: exact, dictionary-id bitmap */
/* PHIP_AGG_DISTINCT (DistinctCountAggregationFunction over BaseDistinctAggregateAggregationFunction,
 * pinot-core/.../query/aggregation/function/BaseDistinctAggregateAggregationFunction.java:131-160 aggregates a
 * dictionary column as a bitmap of dictionary ids, :306-330 its group-by form, :671-690 converts ids to a value set
 * when the segment result is extracted, :760-800 merges by set union). Here the ids are the QUERY-GLOBAL dictionary's
 * (the sorted union of the segments' dictionaries), so one device bitmap is already the merged intermediate of every
 * segment of the query. expr must be PHIP_EXPR_COLUMN and column_a a dictionary-encoded column (INT / LONG / FLOAT /
 * DOUBLE / STRING) in every segment. Each PHIP_AGG_DISTINCT aggregation is one "distinct slot", numbered in
 * aggregation order. Results: values[] / long_values[] hold the exact count (long_exact = 1) and
 * phip_result.distinct_words the bitmaps:
 *   row of group g = distinct_words + g * distinct_word_offsets[num_distinct];
 *   slot s of it   = row + distinct_word_offsets[s], ceil(card_s / 32) u32 words, card_s = the cardinality that
 *                    phip_result_distinct_dictionary(result, s) returns; bit i of word w = global id 32 w + i is
 *                    present; bits at and beyond card_s are 0.
 * The words over the returned dictionary are the mergeable intermediate: the union of two results equals the OR of
 * their words once both are re-based on the union of their dictionaries' values (within one result every group and
 * every segment already shares the dictionary, so there the union IS the OR).
 * PHIP_ERR_UNSUPPORTED (the CPU plan maker answers) for: a raw (no-dictionary) argument column; an expression
 * argument; several filter programs (FILTER(WHERE) / CASE) or null_group_by beside a DISTINCT; hash-table, tuple
 * (> 2^62) and raw-key group-by key spaces; bitmaps above PHIP_DISTINCT_MAX_BYTES (environment, default 256 MiB:
 * dense key space x sum over slots of ceil(card_s / 32) x 4 bytes); an ORDER BY term or order_by_aggregation on a
 * DISTINCT aggregation unless the dense key space is at most trim_size (the server trim can then never fire, and
 * ordering is the broker reduce's job as for every untrimmed result); node plans (segments on several devices or
 * PHIP_NODE_SPLIT) and phip_plan_execute_partial; a library built without the distinct pass. phip_plan_execute (not
 * plan creation) returns PHIP_ERR_UNSUPPORTED when the groups of a plan over SEVERAL segments reach num_groups_limit:
 * the limit is per segment (a segment that dropped a key skips that key's docs), while a bitmap row holds a key's
 * values over every segment; over one segment the kept groups' sets are exact and are returned.
 * PHIP_DISTINCT_LDS_WORDS (environment, read at plan creation, default 8192): without a group-by, bitmaps of at most
 * this many words in all are combined per workgroup in LDS and flushed with one global atomic OR per non-zero word;
 * larger ones, and every group-by, set bits in the global bitmap directly (test before set). */
#define PHIP_AGG_VALUE_COUNTS 6 /* per-id value counts: the exact multiset PERCENTILE and MODE are computed from */
/* PHIP_AGG_VALUE_COUNTS (PercentileAggregationFunction.java:77-100 keeps every value in a DoubleArrayList and :155-172
 * sorts and indexes it; ModeAggregationFunction.java:81-155 keeps a value -> count map): a distinct slot that holds a
 * u32 COUNT per query-global dictionary id where a PHIP_AGG_DISTINCT slot holds a bit. Slots of both kinds are numbered
 * together in aggregation order and share a group's row (phip_result.reserved_distinct tells them apart):
 *   slot s of a row = row + distinct_word_offsets[s], card_s u32 words; word i = the number of matched docs of the
 *                     group whose value is entry i of phip_result_distinct_dictionary(result, s).
 * values[] / long_values[] hold the sum of the slot's words = the docs aggregated (long_exact = 1). The words over the
 * returned dictionary are the mergeable intermediate: two results merge by adding the counts of equal VALUES. The
 * caller computes PERCENTILE (walk the values in order by cumulative count) and MODE (the values of maximal count) from
 * them; several percentiles and modes of one column need one aggregation. No value is gathered on the device.
 * Everything PHIP_AGG_DISTINCT refuses is refused here too (PHIP_DISTINCT_MAX_BYTES counts such a slot at 4 bytes per
 * id), and besides: a STRING column (PHIP_ERR_UNSUPPORTED), and segments of 2^32 docs or more in all (a u32 count could
 * wrap). Regimes as for PHIP_AGG_DISTINCT: in LDS (no group-by, the row within PHIP_DISTINCT_LDS_WORDS) every workgroup
 * adds into its own copy and flushes each non-zero word with one global atomic add; otherwise one global atomic add per
 * doc, lanes of a wave that hold the same id and row combined into one add when the dictionary is small
 * (PHIP_COUNTS_COMBINE_CARD, default 64 ids, 0 = never; PHIP_COUNTS_COMBINE_ROUNDS, default 16: environment, read at
 * plan creation, measurement overrides).
 * PERCENTILEEST / PERCENTILETDIGEST / PERCENTILEKLL, raw columns and expression arguments are not on this path. */
#define PHIP_DISTINCT_SLOT_BITS 0   /* bit s of phip_result.reserved_distinct: a PHIP_AGG_DISTINCT slot, ceil(card / 32) words */
#define PHIP_DISTINCT_SLOT_COUNTS 1 /* a PHIP_AGG_VALUE_COUNTS slot, card words */

#define PHIP_EXPR_COLUMN 0 /* a */
#define PHIP_EXPR_ADD 1    /* a + b   (AdditionTransformFunction) */
#define PHIP_EXPR_SUB 2    /* a - b   (SubtractionTransformFunction.java:99-124) */
#define PHIP_EXPR_MUL 3    /* a * b   (MultiplicationTransformFunction.java:90-106) */

/* ---- derived value columns: arbitrary arithmetic in aggregation arguments ----------------------------------
 * An aggregation argument wider than the two-operand forms above -- a * (1 - b) * (1 + c), a * b / 100, a + b + c --
 * is a postfix program over the query's columns and numeric literals, the chain of double transform functions the
 * reference evaluates it with (pinot-core/.../operator/transform/function/AdditionTransformFunction.java,
 * SubtractionTransformFunction.java, MultiplicationTransformFunction.java, DivisionTransformFunction.java and
 * LiteralTransformFunction.java). The library evaluates the program once per segment into a doc-order value column
 * (expr.hip), keeps it with the segment and reads it like any raw column: phip_query_desc.derived[k] is column index
 * num_columns + k, valid only as column_a of a PHIP_AGG_SUM / MIN / MAX / HLL aggregation with expr ==
 * PHIP_EXPR_COLUMN (any other use -- a group-by column, a filter leaf, a select expression, PHIP_AGG_DISTINCT /
 * PHIP_AGG_VALUE_COUNTS -- is PHIP_ERR_INVALID). Every operation is one separately rounded IEEE binary64 operation
 * (no fused multiply-add), as Java computes it. A SUM reads an exact int64 image instead when every leaf is an INT /
 * LONG column or a PUSH_LONG, no DIV occurs, the value ranges of the segments' columns bound every intermediate below
 * 2^62 and the whole sum below 2^58 (long_exact = 1 then). MIN, MAX and DISTINCTCOUNTHLL always read doubles.
 * Limits (PHIP_ERR_UNSUPPORTED past them): PHIP_EXPR_MAX_OPS ops, a stack of PHIP_EXPR_MAX_STACK values,
 * PHIP_EXPR_MAX_COLUMNS distinct columns per program; num_columns + the derived columns' value kinds <= 16; STRING
 * and HLL-register operands; PHIP_DERIVED_MAX_BYTES (environment, per device, default 64 GiB) of derived columns all
 * pinned by live plans; a library without the kernel. A malformed program is PHIP_ERR_INVALID. A segment keeps its 16
 * most recently used derived columns; a plan keeps the ones it reads alive until phip_plan_destroy.
 * num_entries_scanned_post_filter counts a program's distinct columns, as the reference's projection does. */
#define PHIP_EXPR_OP_PUSH_COLUMN 0 /* push columns[column] of the doc */
#define PHIP_EXPR_OP_PUSH_LONG 1   /* push long_value */
#define PHIP_EXPR_OP_PUSH_DOUBLE 2 /* push double_value */
#define PHIP_EXPR_OP_ADD 3         /* pop b, pop a, push a + b */
#define PHIP_EXPR_OP_SUB 4         /* ... a - b */
#define PHIP_EXPR_OP_MUL 5         /* ... a * b */
#define PHIP_EXPR_OP_DIV 6         /* ... a / b */
#define PHIP_EXPR_MAX_OPS 32
#define PHIP_EXPR_MAX_STACK 8
#define PHIP_EXPR_MAX_COLUMNS 8

typedef struct phip_expr_op {
  int32_t op;     /* PHIP_EXPR_OP_* */
  int32_t column; /* PUSH_COLUMN: index into phip_query_desc.columns */
  int64_t long_value;
  double double_value;
} phip_expr_op;

/* Row reductions of a multi-value column (PHIP_FWD_FIXED_BIT_MV): a derived column whose program is the single op
 * PUSH_COLUMN of that column and whose `reduction` is one of the kinds below holds one value per doc -- the doc's
 * number of values, the sum of its values, or its smallest / largest value -- so COUNTMV / SUMMV / AVGMV / MINMV /
 * MAXMV / MINMAXRANGEMV are PHIP_AGG_SUM / MIN / MAX over it (mv.hip). LENGTH is int64; SUM is int64 for an INT / LONG
 * column while max_values_per_doc x the dictionary's extremes stays below 2^62 and the whole sum below 2^58, else the
 * row's values added left to right in double (SumMVAggregationFunction.aggregate); MIN / MAX are doubles. Cached and
 * budgeted with the arithmetic columns. A reduction over a single-value column, reduction 0 over a multi-value one, and
 * any reduction in a library without the kernel are PHIP_ERR_UNSUPPORTED. */
#define PHIP_MV_REDUCE_NONE 0   /* an arithmetic program (above) */
#define PHIP_MV_REDUCE_LENGTH 1
#define PHIP_MV_REDUCE_SUM 2
#define PHIP_MV_REDUCE_MIN 3
#define PHIP_MV_REDUCE_MAX 4

typedef struct phip_derived_column {
  const phip_expr_op *ops;
  int32_t num_ops;
  int32_t reduction; /* PHIP_MV_REDUCE_* */
} phip_derived_column;

typedef struct phip_aggregation {
  int32_t function; /* PHIP_AGG_* */
  int32_t expr;     /* PHIP_EXPR_* (ignored for COUNT) */
  int32_t column_a; /* index into phip_query_desc.columns; num_columns + k = derived column k (PHIP_EXPR_COLUMN only) */
  int32_t column_b;
  int32_t log2m; /* HLL */
  int32_t program; /* filter program whose docs this aggregation reads (0 unless num_filter_programs > 1) */
} phip_aggregation;

/* A time transform of one single-value dictionary INT / LONG column (dateTrunc, toEpochSeconds ... toEpochDays,
 * timeConvert, and the UTC ISO-chronology fields; DateTruncTransformFunction.java:100-142, DateTimeFunctions.java:80-133
 * and :656-1034, TimeConversionTransformFunction.java). The value of a dictionary entry v is
 *     scale(op(scale(v, in_mul, in_div)), out_mul, out_div)
 * where scale(x, m, d) is x * m or Java's x / d (truncating toward zero; of m and d one is 1, both >= 1) and op works
 * on UTC epoch milliseconds: PHIP_TT_CONVERT the identity (unit 0, no output scale), PHIP_TT_TRUNC Joda's roundFloor
 * to `unit` = PHIP_TT_SECOND ... PHIP_TT_YEAR (floors below 1970 too; ISO weeks from Monday; the proleptic Gregorian
 * calendar), PHIP_TT_FIELD the field `unit` = PHIP_TT_FIELD_YEAR ... PHIP_TT_FIELD_MILLISECOND (no scales; dayOfWeek
 * 1 = Monday ... 7 = Sunday, week = the ISO week of the weekyear). TimeUnit.convert's saturation is not reproduced: a
 * program whose products over the column's [min, max] could leave int64 is PHIP_ERR_UNSUPPORTED. function 0
 * (PHIP_TT_NONE) = the plain column. Any other malformed program is PHIP_ERR_INVALID, before any launch. */
#define PHIP_TT_NONE 0
#define PHIP_TT_CONVERT 1
#define PHIP_TT_TRUNC 2
#define PHIP_TT_FIELD 3
#define PHIP_TT_SECOND 0
#define PHIP_TT_MINUTE 1
#define PHIP_TT_HOUR 2
#define PHIP_TT_DAY 3
#define PHIP_TT_WEEK 4
#define PHIP_TT_MONTH 5
#define PHIP_TT_QUARTER 6
#define PHIP_TT_YEAR 7
#define PHIP_TT_FIELD_YEAR 0
#define PHIP_TT_FIELD_QUARTER 1
#define PHIP_TT_FIELD_MONTH 2
#define PHIP_TT_FIELD_WEEK 3
#define PHIP_TT_FIELD_DAY_OF_YEAR 4
#define PHIP_TT_FIELD_DAY_OF_MONTH 5
#define PHIP_TT_FIELD_DAY_OF_WEEK 6
#define PHIP_TT_FIELD_HOUR 7
#define PHIP_TT_FIELD_MINUTE 8
#define PHIP_TT_FIELD_SECOND 9
#define PHIP_TT_FIELD_MILLISECOND 10
typedef struct phip_time_transform {
  int32_t function; /* PHIP_TT_* */
  int32_t unit;
  int64_t in_mul, in_div, out_mul, out_div;
} phip_time_transform;

/* A comparison of a time transform's values with int64 literals (phip_segment_match_transform): PHIP_TT_PRED_RANGE =
 * lower <= / < value <= / < upper by the inclusive flags (an unbounded side: INT64_MIN / INT64_MAX inclusive);
 * PHIP_TT_PRED_SET = value among the num_values strictly ascending `values` (0 values: nothing). exclusive = 1
 * complements the answer (NOT_EQ / NOT_IN). */
#define PHIP_TT_PRED_RANGE 1
#define PHIP_TT_PRED_SET 2
typedef struct phip_transform_predicate {
  int32_t kind;
  int32_t exclusive;
  int64_t lower, upper;
  int32_t lower_inclusive, upper_inclusive;
  const int64_t *values;
  int32_t num_values;
  int32_t reserved;
} phip_transform_predicate;

typedef struct phip_query_desc {
  int32_t num_columns;
  int32_t num_segments;
  const char *const *columns; /* column names; nodes/aggregations refer to them by index */
  const uint64_t *segments;   /* handles from phip_segment_load */
  const int32_t *filter_offsets;          /* [num_filter_programs * num_segments + 1] into filter_nodes: program p
                                           * of segment s = [p * num_segments + s, + 1); empty = match all */
  const phip_filter_node *filter_nodes;
  int32_t num_aggregations;
  int32_t num_group_by;
  const phip_aggregation *aggregations;
  const int32_t *group_by_columns; /* indices into columns */
  int64_t num_groups_limit;        /* InstancePlanMakerImplV2 numGroupsLimit (default 100,000) */
  /* Server-level trim of a group-by with ORDER BY on one aggregation (IndexedTable.finish ->
   * TableResizer.getTopRecords, GroupByUtils.java:96-140): when trim_size > 0 and more groups than trim_size
   * exist, only the top trim_size groups by aggregations[order_by_aggregation] (Double.compare order,
   * descending when order_by_desc) are returned; ties at the boundary keep the lowest group key.
   * order_by_aggregation = -1 disables it. */
  int32_t order_by_aggregation;
  int32_t order_by_desc;
  int64_t trim_size;               /* max(5 * limit, minServerGroupTrimSize) (GroupByUtils.java:55-58) */
  /* ORDER BY on group-by columns instead (takes precedence when > 0): entry j = k + 1 (ASC) or -(k + 1)
   * (DESC) for group-by column k; the query-global dictionaries are value-sorted, so id order is value order. */
  int32_t num_order_by_keys;
  /* enableNullHandling group keys (NoDictionarySingleColumnGroupKeyGenerator.getKeyForNullValue /
   * NoDictionaryMultiColumnGroupKeyGenerator, pinot-core/.../groupby/NoDictionary*GroupKeyGenerator.java): bit k =
   * group-by column k's null docs (its null value vector) form one more key value, the null key -- group key id =
   * the column's phip_dictionary_view.cardinality in phip_result.group_keys; it is counted toward numGroupsLimit in
   * first-seen order like any key, sorts after every value in an ascending key trim and first in a descending one
   * (the reference's default NULLS LAST / NULLS FIRST). 0 = the stored default values are the keys. */
  int32_t null_group_by;
  const int32_t *order_by_keys;
  /* Any other ORDER BY (TableResizer, pinot-core/.../data/table/TableResizer.java:90-125,410-450): a list of
   * terms, each a group-by column or an aggregation's final result, mixed freely (takes precedence over both
   * fields above when > 0). The device sorts the groups by the whole list (stable; ties keep the lowest group key)
   * and keeps trim_size of them. */
  int32_t num_order_terms;
  /* Filtered aggregations in one pass (FilteredAggregationOperator.java:67-113, one program per
   * AggregationFunctionUtils.buildFilteredAggregationInfos info): when > 1, filter_offsets holds that many
   * programs per segment, one filter launch evaluates all of them into one tile mask each, and one aggregation
   * launch aggregates every function over its own program's docs (phip_aggregation.program). Statistics sum over
   * the programs (numDocsScanned, entries scanned; a segment matched when any program matched). Aggregation only
   * (no group-by), at most 8 programs. 0 or 1 = one program. */
  int32_t num_filter_programs;
  const struct phip_order_term *order_terms;
  /* Selection (row-returning) queries, the leaf of a multi-stage join (SelectionOnlyOperator,
   * pinot-core/.../operator/query/SelectionOnlyOperator.java:40-170, and SelectionOnlyCombineOperator): when
   * num_select > 0 (no aggregations, no group-by, one filter program) each segment keeps its first select_limit
   * matched docs in doc order, the segments' rows are concatenated in query order up to select_limit rows, and
   * every row holds the select expressions (phip_result.select_*). Statistics: numDocsScanned = the rows each
   * segment kept, numEntriesScannedPostFilter = that x the distinct columns the expressions read. */
  int32_t num_select;
  /* Programs whose filter scans count in num_entries_scanned_in_filter: bit p = program p; 0 = every program.
   * A CASE aggregation's branch programs re-evaluate the query's filter AND a WHEN condition, while the
   * reference scans each original filter once (CaseTransformFunction evaluates the WHENs in the transform,
   * pinot-core/.../transform/function/CaseTransformFunction.java): only those programs count. */
  uint32_t stats_programs;
  const struct phip_select_expr *select;
  int64_t select_limit;
  /* Derived value columns (see phip_expr_op above): derived[k] is column index num_columns + k. 0 / NULL = none. */
  int32_t num_derived;
  int32_t reserved_derived;
  const phip_derived_column *derived;
  /* Selection ORDER BY (SelectionOrderByOperator, pinot-core/.../operator/query/SelectionOrderByOperator.java, with
   * SelectionOrderByCombineOperator): when num_select_order > 0 the result is the first select_keep (= offset + limit)
   * rows of the matched docs sorted by the terms, each a select[] index with a direction: INT / LONG by value, FLOAT /
   * DOUBLE and a op b in Double.compare order (-0.0 < 0.0, every NaN one value above +inf), dictionary STRING in the
   * dictionaries' order. Rows equal on every term keep ascending (segment position in the query, doc id) order, so
   * the rows are a stable sort of the selection-only rows. select[] holds the block's expressions, the ORDER BY
   * expressions among them; select_limit is not read. At most 8 terms; a raw STRING term is PHIP_ERR_UNSUPPORTED.
   * Statistics: numDocsScanned = the matched docs; numEntriesScannedPostFilter = matched x the distinct columns of
   * the term expressions + sum over the segments of min(matched, select_keep) x the distinct columns only the other
   * expressions read. All zero (as in every descriptor from before these fields) = no ORDER BY. */
  int32_t num_select_order;
  int32_t reserved_select_order;
  const struct phip_select_order_term *select_order;
  int64_t select_keep;
  /* SELECT DISTINCT (DistinctOperator, pinot-core/.../operator/query/DistinctOperator.java:57-87, with
   * DistinctExecutorFactory.java:55-148's dictionary-based executors and DistinctCombineOperator's merge): when
   * select_distinct = 1 the descriptor is a selection's -- select[] holds the DISTINCT columns in select order
   * (PHIP_EXPR_COLUMN only, at most 8, single-value dictionary columns of any type), select_order / num_select_order
   * the ORDER BY terms (each one of the columns; may be 0), select_keep the limit (> 0); select_limit is not read -- and
   * the result is the distinct rows of the matched docs, ordered by the ORDER BY terms and then by the remaining columns
   * ascending in select order, cut to the first select_keep rows. The reference's choice among rows that tie on the
   * terms, and of the `limit` rows of a query without ORDER BY, depends on the docs' arrival order; this rule is one
   * of the answers it may give. Rows come back in final order in phip_result's selection fields (num_rows,
   * num_select, select_types, select_values; STRING columns as ids of phip_result_select_dictionary).
   * The device keys every doc by a mixed radix over the columns' query-global ids (a DESC term's digit is card - 1 -
   * id; the ORDER BY terms are the most significant digits) and keeps the key set in the regime the key space K =
   * the product of the cardinalities admits (phip_plan_launch_shape, PHIP_SHAPE_DISTINCT_ROWS_REGIME): a bitmap of K
   * bits in every workgroup's LDS when its words fit PHIP_DISTINCT_LDS_WORDS (as PHIP_AGG_DISTINCT); else a global
   * bitmap when K / 8 <= PHIP_DISTINCT_ROWS_MAX_BYTES (environment, read at plan creation, default 256 MiB); else,
   * for K < 2^63, one u64 key per matched doc sorted and made unique, the buffers (keys, sorted, unique, sort scratch,
   * sized for every doc of the work list) within PHIP_DISTINCT_ROWS_SORT_BYTES (default 4 GiB). Past that budget, or
   * at K >= 2^63, PHIP_ERR_UNSUPPORTED.
   * Statistics: numDocsScanned = every matched doc, numEntriesScannedPostFilter = matched x the columns, the filter
   * statistics the filter launch's. The reference stops as soon as `limit` distinct rows exist when there is no
   * ORDER BY, so its counts there depend on where it stopped; whenever it cannot stop early (ORDER BY, or fewer
   * distinct rows than `limit`) the numbers are equal.
   * PHIP_ERR_UNSUPPORTED besides: a raw (no-dictionary), multi-value or HLL register column, an expression, several
   * devices (a node plan), a library built without the distinct-rows kernels. All zero = not a distinct query. */
  int32_t select_distinct;
  int32_t reserved_select_distinct;
  /* GROUP BY over time transforms: null, or num_group_by programs, one per group-by column; function PHIP_TT_NONE = the
   * plain column. Key k is then program k's value of group_by_columns[k] (which stays the real column's index: a
   * single-value dictionary INT / LONG column in every segment): the group-by walks gather the same per-segment id
   * remap as for a plain key, only its query-global ids number the ascending distinct values of the program over the
   * segments' dictionaries (built on the device once per (segments, column, program) and kept with the other remaps),
   * so id order is value order and the table choice, tuple keys, key-ordered trims, num_groups_limit and
   * phip_result_dictionary (data type LONG, or INT for a PHIP_TT_FIELD) work as for any key. Two keys over one column
   * must name it through two entries of columns[] (each entry carries one remap). A transformed key's plan builds no
   * group-by records. PHIP_ERR_INVALID: a malformed program, a column that is not such a column. PHIP_ERR_UNSUPPORTED:
   * a node plan (segments on several devices), null_group_by on a transformed key whose column has a null vector, a
   * program that could overflow, a library built without the kernel. */
  const struct phip_time_transform *group_by_transforms;
} phip_query_desc;

typedef struct phip_select_order_term {
  int32_t select_index; /* index into phip_query_desc.select */
  int32_t descending;
} phip_select_order_term;

typedef struct phip_select_expr {
  int32_t expr;     /* PHIP_EXPR_*: a column, or a op b (evaluated in double, as the transform functions do) */
  int32_t column_a; /* index into phip_query_desc.columns */
  int32_t column_b;
  int32_t reserved;
} phip_select_expr;

#define PHIP_ORDER_GROUP_KEY 0 /* group-by column `a` (GroupByExpressionExtractor) */
#define PHIP_ORDER_VALUE 1     /* aggregations[a] as double: SUM / MIN / MAX / COUNT (AggregationFunctionExtractor) */
#define PHIP_ORDER_AVG 2       /* aggregations[a] (SUM) / aggregations[b] (COUNT); -inf when the count is 0 */
#define PHIP_ORDER_RANGE 3     /* aggregations[b] (MAX) - aggregations[a] (MIN): MINMAXRANGE */
#define PHIP_ORDER_HLL 4       /* aggregations[a] (DISTINCTCOUNTHLL): its registers' cardinality estimate */

typedef struct phip_order_term {
  int32_t kind; /* PHIP_ORDER_* */
  int32_t a;
  int32_t b;
  int32_t desc; /* 1 = DESC */
} phip_order_term;

/* ---- results ------------------------------------------------------------------------------
 * Library-owned, valid until phip_result_free. For an aggregation-only query num_groups = 1.
 * values[g*num_aggregations + a] holds SUM/MIN/MAX/COUNT as double (HLL: estimate);
 * long_values[...] the exact int64 SUM (integral inputs) or COUNT.
 * hll_registers: [num_groups][num_hll][1 << log2m] u8 in aggregation order of the HLL aggs.
 * group_keys[g*num_group_by + k]: id in the query-global dictionary of group-by column k;
 * phip_result_dictionary returns that dictionary's values. */
typedef struct phip_result {
  int64_t num_docs_scanned;
  int64_t num_entries_scanned_in_filter;
  int64_t num_entries_scanned_post_filter;
  int64_t num_total_docs;
  int32_t num_segments_processed;
  int32_t num_segments_matched;
  int32_t num_groups_limit_reached;
  int32_t num_aggregations;
  int64_t num_groups;
  int32_t num_group_by;
  int32_t num_hll;
  const double *values;
  const int64_t *long_values;
  const uint8_t *hll_registers;
  const int32_t *group_keys;
  double scan_kernel_ms; /* device time of the fused filter/aggregate kernel(s) */
  double device_ms;      /* device time of the query's filter / aggregation kernels (whole sequence incl. memsets and
                          * finalize when PHIP_TOTAL_EVENTS=1: two more timing markers, ~4 us each on the queue) */
  int32_t num_groups_trimmed; /* 1 when the group set was trimmed to phip_query_desc.trim_size */
  int32_t fused;              /* 1 when the filter kernel aggregated its own tiles (one launch: filter_kernel_ms and
                                 filter_bytes then cover both, agg_* are 0) */
  /* long_exact[a] = 1 when long_values[g*num_aggregations + a] holds the exact integer result (COUNT, and SUM
   * over INT/LONG inputs whose bound sum |value| stays below 2^58); 0 when the SUM accumulated in double like
   * SumAggregationFunction (a possible int64 overflow) -- values[] is then the only result. */
  const int32_t *long_exact;
  /* Per-kernel device time and algorithmic bytes (the roofline numerators):
   * filter_bytes = per work tile, the fixed-bit words of every scanned column (256*b bytes), the dense words of
   * every inverted leaf (256) and the raw values of raw leaves -- what the filter launch must stream;
   * agg_bytes = per segment, matched docs x (b/8 per projected dictionary column, value width per raw one) plus
   * min(card, matched) dictionary entries per gathered column. Intermediates (tile masks, tables) excluded. */
  double filter_kernel_ms;
  double agg_kernel_ms;
  int64_t filter_bytes;
  int64_t agg_bytes;
  /* Selection queries (phip_query_desc.num_select > 0): num_rows rows of num_select columns, column-major 8-byte
   * slots select_values[k * num_rows + r]; select_types[k] says how to read column k: PHIP_TYPE_INT / LONG = int64,
   * PHIP_TYPE_FLOAT / DOUBLE = double bits (FLOAT values are exact floats; expressions are DOUBLE), PHIP_TYPE_STRING
   * = id in a query-global dictionary (phip_result_select_dictionary). */
  int64_t num_rows;
  int32_t num_select;
  int32_t reserved_select;
  const int32_t *select_types;
  const uint64_t *select_values;
  /* Per segment of the query (num_segments_processed entries): the docs that passed its filter, summed over the
   * filter programs -- the docs its GroupByOperator keyed, so min(this, key space, numGroupsLimit) bounds the
   * group records the segment hands the combine (GroupByCombineOperator.java:128-157; the plan maker's
   * minSegmentGroupTrimSize / groupTrimThreshold checks). For a phip_plan_finish result: this GPU's. */
  const int64_t *segment_docs_matched;
  /* The part of filter_bytes the filter launch STREAMS (the staged tiles' words, LDS-DMA); for a fused launch
   * filter_bytes also holds its gathers (agg_bytes folded in). The traffic calibration separates the two. */
  int64_t stream_bytes;
  /* Per filter program (phip_query_desc.num_filter_programs entries, 1 for one program): the docs that passed it over
   * all segments -- the reference's numDocsScanned when programs are the plan maker's own device (the null-handling
   * group-by's IS NOT NULL programs), not FilteredGroupByOperator infos. For a phip_plan_finish result: this GPU's. */
  const int64_t *program_docs_matched;
  /* PHIP_AGG_DISTINCT / PHIP_AGG_VALUE_COUNTS (see their definitions above): the number of distinct slots, the
   * groups' rows back to back (num_groups x distinct_word_offsets[num_distinct] words) and the num_distinct + 1 word
   * offsets of the slots inside a row. NULL / 0 without such an aggregation. reserved_distinct holds the slots' kinds:
   * bit s set = slot s is a PHIP_AGG_VALUE_COUNTS slot (PHIP_DISTINCT_SLOT_COUNTS: card_s words of u32 counts), clear =
   * a PHIP_AGG_DISTINCT slot (PHIP_DISTINCT_SLOT_BITS: ceil(card_s / 32) bitmap words). At most 8 slots per plan. */
  int32_t num_distinct;
  int32_t reserved_distinct;
  const uint32_t *distinct_words;
  const int64_t *distinct_word_offsets;
  /* Device time of the distinct pass (bitmap clear + mark kernel; the finish kernel is not in it). A measurement
   * aid like the other *_kernel_ms fields: it reads 0 when the execution recorded no timing markers
   * (PHIP_KERNEL_TIMING=0 on an aggregation-only plan) and when the plan replayed its captured graph (PHIP_GRAPH). */
  double distinct_kernel_ms;
} phip_result;

typedef struct phip_dictionary_view {
  int32_t data_type;
  int32_t cardinality;
  int32_t string_width;
  int32_t reserved;
  const void *values; /* LE int32/int64/float/double array, or card x string_width bytes */
} phip_dictionary_view;

/* ---- entry points -------------------------------------------------------------------------- */
PHIP_API int32_t phip_init(const int32_t *devices, int32_t num_devices);
PHIP_API int32_t phip_shutdown(void);
PHIP_API int32_t phip_device_count(int32_t *out_count);
PHIP_API const char *phip_last_error(void);
PHIP_API const char *phip_version(void);
/* HIP_VERSION the library was built against and hipRuntimeGetVersion of the runtime it bound to (a process that
 * also runs PyTorch-ROCm shares torch's bundled runtime; the loader refuses a major-version mismatch). No
 * reference counterpart: a build/runtime sanity check of the FFM loader. */
PHIP_API int32_t phip_runtime_versions(int32_t *out_built, int32_t *out_runtime);

PHIP_API int32_t phip_segment_load(const phip_segment_desc *desc, uint64_t *out_handle);
PHIP_API int32_t phip_segment_unload(uint64_t handle);
PHIP_API int32_t phip_segment_device_bytes(uint64_t handle, uint64_t *out_bytes);
/* REGEXP_LIKE / LIKE over a dictionary STRING column (single- or multi-value): runs the DFA blob `dfa` (dfa_words int32
 * words, "DFA blob" above) once over the column's `cardinality` dictionary entries instead of the docs
 * (RegexpLikePredicateEvaluatorFactory's DictionaryBasedRegexpLikePredicateEvaluator looks the value up and matches it
 * per scanned doc, RegexpLikePredicateEvaluatorFactory.java:74-76). Bit i % 64 of out_words[i / 64] is set iff entry i
 * matches; bits at and past the cardinality are 0. An entry is the bytes before its first 0 pad byte, or all
 * string_width of them (FixedByteValueReaderWriter.readUnpaddedBytes). num_words must be >= ceil(cardinality / 64).
 * The caller turns the ids into DICT_RANGE / DICT_SET leaves. The dictionary's bytes are uploaded on the first call
 * and stay with the segment (phip_segment_device_bytes then includes them). Errors: PHIP_ERR_INVALID for a bad blob,
 * a column that is not a dictionary STRING column, or too few words; PHIP_ERR_UNSUPPORTED in a library built without
 * the kernel. */
PHIP_API int32_t phip_segment_match_dictionary(uint64_t handle, const char *column, const int32_t *dfa, int32_t dfa_words,
                                               uint64_t *out_words, int64_t num_words);
/* The twin of phip_segment_match_dictionary for a time transform over a single-value dictionary INT /
 * LONG column: evaluates `transform` once per dictionary entry and compares it with `predicate`. Bit i % 64 of
 * out_words[i / 64] is set iff entry i's value passes; bits at and past the cardinality are 0. The caller turns the
 * ids into DICT_RANGE / DICT_SET leaves flagged PHIP_LEAF_FLAG_ALWAYS_SCAN (ExpressionFilterOperator always scans).
 * Every field is validated before any launch: PHIP_ERR_INVALID for a malformed program or predicate (an unknown kind,
 * values that do not ascend strictly, a null `values` with num_values > 0), a column that is not a dictionary INT /
 * LONG column, too few words; PHIP_ERR_UNSUPPORTED for a program that could overflow over the column's values and in
 * a library built without the kernel. */
PHIP_API int32_t phip_segment_match_transform(uint64_t handle, const char *column, const phip_time_transform *transform,
                                              const phip_transform_predicate *predicate, uint64_t *out_words,
                                              int64_t num_words);
/* Since phip_init: the transformed group-by remaps built (a plan that finds its remap kept builds none) and the
 * phip_segment_match_transform launches. */
PHIP_API int32_t phip_transform_info(int64_t *out_remap_builds, int64_t *out_match_launches);
/* The segment's derived value columns (phip_query_desc.derived): how many it holds now (at most 16), their bytes, and
 * the materialise launches since load -- a plan whose expression the segment already holds launches none.
 * phip_segment_device_bytes stays what the segment's load pinned: it does not include these bytes (nor the other
 * first-use derivatives), which come and go with the queries; a cache sized against device memory adds out_bytes. */
PHIP_API int32_t phip_segment_derived_info(uint64_t handle, int32_t *out_count, int64_t *out_bytes, int64_t *out_builds);

PHIP_API int32_t phip_query(const phip_query_desc *query, phip_result **out_result);

/* Prepared queries: InstancePlanMakerImplV2.makeInstancePlan returns a Plan that
 * GlobalPlanImplV0.execute runs (pinot-core/.../plan/GlobalPlanImplV0.java:48-57). phip_plan_create does
 * every host-side step once (predicate programs per segment, descriptors, launch shapes, device buffers);
 * phip_plan_execute replays the launch sequence (eagerly; PHIP_GRAPH=1 opts into a captured hipGraph) and
 * returns a result exactly as phip_query would. A plan keeps its segments' HBM alive: unloading a
 * segment a plan uses defers the release to phip_plan_destroy. Executions of one plan serialise. */
PHIP_API int32_t phip_plan_create(const phip_query_desc *query, uint64_t *out_plan);
PHIP_API int32_t phip_plan_execute(uint64_t plan, phip_result **out_result);
PHIP_API int32_t phip_plan_destroy(uint64_t plan);
/* Query deadline and cancellation (QueryContext.getEndTimeMs / the server's cancel of a running query,
 * BaseSingleBlockCombineOperator.java:137-144, QueryScheduler cancel): an execution checks them between its launch
 * phases -- before enqueuing, after the main kernels, before a numGroupsLimit pass and before the server trim -- and
 * returns PHIP_ERR_TIMEOUT / PHIP_ERR_CANCELLED there (a launch in flight completes: kernels are not interrupted,
 * as the reference's operators only check between blocks). deadline_ms: wall-clock milliseconds since the Unix
 * epoch (System.currentTimeMillis), 0 = none. A cancel is sticky: the plan belongs to one query. */
PHIP_API int32_t phip_plan_set_deadline(uint64_t plan, int64_t deadline_ms);
PHIP_API int32_t phip_plan_cancel(uint64_t plan);
PHIP_API int32_t phip_result_dictionary(const phip_result *result, int32_t group_by_index,
                                        phip_dictionary_view *out_view);
PHIP_API void phip_result_free(phip_result *result);

/* The query-global dictionary of distinct slot `distinct_index` (the ids phip_result.distinct_words' bits stand for):
 * the sorted union of the column's dictionary values over the query's segments, exactly as phip_result_dictionary
 * returns a group-by column's. */
PHIP_API int32_t phip_result_distinct_dictionary(const phip_result *result, int32_t distinct_index,
                                                 phip_dictionary_view *out_view);

/* Values of select column k of a selection result that holds STRING dictionary ids. */
PHIP_API int32_t phip_result_select_dictionary(const phip_result *result, int32_t select_index,
                                               phip_dictionary_view *out_view);

/* Filter only, one segment: words_out receives ceil(num_docs/64) bitmap words. */
PHIP_API int32_t phip_filter_bitmap(const phip_query_desc *query, uint64_t *words_out, int64_t num_words);

/* ---- multi-GPU servers: one process per GPU, partial group tables merged on the device ----------------
 * The reference's combine merges per-segment group-by results by VALUE on one JVM
 * (GroupByCombineOperator.java:138-147 upserting into an IndexedTable). A server spread over several GPUs
 * instead keys every group-by column by a NODE-GLOBAL dictionary: the sorted union of
 * the column's dictionary values over every segment on every GPU, registered once per column after load.
 * Plans created afterwards key that column by ids in it on every GPU, so each GPU's dense partial table has
 * the same shape and key order and the GPUs merge them element-wise with RCCL all-reduce on the device
 * buffers -- no host round trip of group records.
 *
 * phip_global_dictionary: values as phip_dictionary_view lays them out (LE typed array, or
 * cardinality x string_width '\0'-padded bytes), ascending, distinct. Registering a column again replaces
 * it for plans created later; cardinality = -1 removes the registration. Columns are keyed by the name the
 * query descriptors use (one table per server process). A segment value missing from it fails plan creation
 * with PHIP_ERR_INVALID. */
PHIP_API int32_t phip_global_dictionary(int32_t device, const char *column, int32_t data_type, int32_t cardinality,
                                        int32_t string_width, const void *values);

/* Row kinds of a partial table; the reduce operator of each row follows from its kind. */
#define PHIP_ROW_COUNT 0   /* int64 doc count per group (row 0; unused rows of COUNT aggregations hold 0): SUM */
#define PHIP_ROW_SUM_I64 1 /* exact int64 sum: SUM (int64) */
#define PHIP_ROW_SUM_F64 2 /* double sum (bits): SUM (float64) */
#define PHIP_ROW_MIN 3     /* order-preserving u64 image of a double (f64_ordered): MIN as unsigned */
#define PHIP_ROW_MAX 4     /* same image: MAX as unsigned */
#define PHIP_ROW_HLL 5     /* row unused (0); the registers are in phip_partial.hll: MAX (int32) */
#define PHIP_PARTIAL_MAX_ROWS 9

typedef struct phip_partial {
  int64_t num_groups;   /* dense key space G = product of the group-by columns' (global) cardinalities */
  int32_t num_rows;     /* 1 + num_aggregations */
  int32_t num_hll;
  int32_t log2m;
  int32_t device;
  uint64_t *table;      /* DEVICE memory owned by the plan: [num_rows][G] u64, row 0 = doc count per group */
  uint32_t *hll;        /* DEVICE memory: [num_hll][G][1 << log2m] u32 registers, or NULL */
  /* row_kinds[r] for r < num_rows. A caller merging GPUs whose plans disagree on SUM_I64 vs SUM_F64 for a
   * row (the int64-overflow bound is per GPU) converts its int64 row to doubles in place and sets the kind to
   * PHIP_ROW_SUM_F64 before phip_plan_finish. */
  int32_t row_kinds[PHIP_PARTIAL_MAX_ROWS];
  int32_t global_keys;  /* 1 when every group-by column is keyed by a registered global dictionary (else the
                         * key order is this GPU's own and the table must not be merged element-wise) */
  /* This GPU's execution statistics (phip_result order: docs scanned, entries scanned in filter, entries
   * scanned post filter, total docs, segments processed, segments matched); summed over GPUs by the caller. */
  int64_t stats[6];
  /* Aggregation-only plans (num_groups = 1): the same six statistics as int64 in DEVICE memory right after the
   * table's last row (stats_dev = table + num_rows), so one int64 SUM all-reduce covers the table's integer rows and
   * them; phip_plan_finish then reads the merged statistics from there. NULL for group-by partials (stats[] holds
   * them). */
  int64_t *stats_dev;
  /* 1: hll holds u8 registers ([num_hll][G][1 << log2m] bytes: the all-reduce MAX runs on them directly); 0: u32. */
  int32_t hll_u8;
  int32_t reserved_partial;
} phip_partial;

/* Runs a dense group-by plan up to its partial table and returns it (the kernels have completed). An
 * aggregation-only plan (AggregationResultsBlockMerger.java:34-49's inputs) hands out a one-group table: row 0 =
 * matched docs, row 1 + a = aggregation a in its row kind's encoding (MIN / MAX as the order-preserving u64 image),
 * the statistics in stats_dev and u8 HLL registers -- all in device memory, so GPUs merge them with RCCL
 * all-reduces and no host copy. Returns
 * PHIP_ERR_UNSUPPORTED, with nothing to merge, for hash-table key spaces and when the GPU's distinct groups
 * reach numGroupsLimit (the per-segment first-seen limit needs the record path: phip_plan_execute). Until
 * phip_plan_finish the table belongs to the caller: it may all-reduce it in place (on any stream, synchronised
 * before phip_plan_finish). No other execution of the same plan may start in between (the library refuses one
 * with PHIP_ERR_INVALID until phip_plan_finish or phip_plan_abandon_partial). */
PHIP_API int32_t phip_plan_execute_partial(uint64_t plan, phip_partial *out_partial);
/* Compacts the (merged) partial table into a result exactly as phip_plan_execute would -- present groups,
 * the server-level trim (trim_size), statistics taken from merged->stats. */
PHIP_API int32_t phip_plan_finish(uint64_t plan, const phip_partial *merged, phip_result **out_result);
/* Gives a pending partial table back without finishing it (the GPUs agreed to merge records instead). While a
 * partial is pending, phip_plan_execute / phip_plan_execute_partial on the plan return PHIP_ERR_INVALID. */
PHIP_API int32_t phip_plan_abandon_partial(uint64_t plan);

/* ---- multi-GPU servers in ONE process: node plans ------------------------------------------------------
 * A Pinot server is one JVM that owns every GPU of its node: BaseCombineOperator fans a query's segments out over
 * worker threads (pinot-core/.../operator/combine/BaseCombineOperator.java:98-143) and merges their blocks in that
 * process (BaseSingleBlockCombineOperator.java:129-162, GroupByCombineOperator.java:138-147). phip_plan_create /
 * phip_query over segments loaded on SEVERAL devices (phip_segment_desc.device) returns a node plan -- no other call
 * changes, so the Java binding needs nothing beyond this header:
 *   - each device's segments form one single-device sub-plan; the group-by columns of every sub-plan are keyed by the
 *     node plan's own node-global dictionaries (the sorted union of the column's values over all its segments, built
 *     at plan creation -- no phip_global_dictionary registration needed), so the devices' dense partial tables have
 *     the same shape and key order;
 *   - phip_plan_execute runs the sub-plans concurrently, one host thread and one execution lane per device, up to
 *     their dense partial tables (phip_plan_execute_partial's), then merges them ON THE DEVICES: one RCCL reduce to
 *     the root device (the first device in query order) over the node's communicator (ncclCommInitAll over the
 *     node plan's devices, created once per device set, librccl loaded on first use; xGMI peer-to-peer) -- int64 SUM
 *     for counts and exact sums, f64 SUM, unsigned MIN / MAX of the order-preserving images, MAX of the HLL registers
 *     -- and finishes the merged table on the root (compaction, server trim, copy-out) exactly as phip_plan_finish;
 *   - where the devices cannot share a communicator (two parts on one device, no loadable librccl) the non-root
 *     tables are copied to the root device (hipMemcpyPeerAsync) and folded in by the library's merge kernel, the same
 *     operators;
 *   - hash-table key spaces (node-global keys, each part's table sized for every doc of the node): the non-root
 *     parts' keys, rows and registers are copied to the root device and inserted into the root's table by key
 *     (PHIP_EXCHANGE_HASH), then finished as above;
 *   - aggregation-only queries (one group) and group-bys without a mergeable partial table (a device reaching
 *     numGroupsLimit -- the per-segment first-seen limit --, a full hash table, raw group-by keys, tuple keys, parts
 *     whose null keys differ) run each sub-plan to its records and merge them on the host by key VALUE, as the
 *     reference's combine does (untrimmed: the broker's ORDER BY / LIMIT applies to exact groups).
 * Statistics are summed over the devices; segment_docs_matched covers every segment in query order; kernel times
 * are the slowest device's. Selection queries over several devices return PHIP_ERR_UNSUPPORTED. The deadline and
 * cancel calls apply to every sub-plan. phip_plan_execute_partial / phip_plan_finish / phip_plan_abandon_partial on
 * a node plan return PHIP_ERR_INVALID (it merges internally).
 * PHIP_NODE_SPLIT=k (environment, read at plan creation) splits a query whose segments share one device into k parts
 * on that device -- a rehearsal of the node path on a one-GPU box (the peer-merge exchange; k = 1: one part and a
 * one-rank RCCL communicator). PHIP_NODE_EXCHANGE=peer forces the merge kernel, =rccl refuses the fallback. */
#define PHIP_EXCHANGE_NONE 0    /* a single-device plan */
#define PHIP_EXCHANGE_RCCL 1    /* the last execution reduced the partial tables with RCCL */
#define PHIP_EXCHANGE_PEER 2    /* ... copied them to the root device and merged them with the merge kernel */
#define PHIP_EXCHANGE_RECORDS 3 /* ... merged the sub-plans' records on the host */
#define PHIP_EXCHANGE_HASH 4    /* ... inserted the other sub-plans' hash-table groups into the root's table on the root device */
/* Devices (sub-plans) of a plan and the exchange its last execution used (PHIP_EXCHANGE_*; NONE before the first). */
PHIP_API int32_t phip_plan_exchange(uint64_t plan, int32_t *out_parts, int32_t *out_kind);

/* The launch shape of a single-device plan's last execution (all 0 before the first), for tests that must know how
 * many tiles and segments one wave walked: out_shape[i], i < num_values, in the order below. The grids follow the
 * device's CU count, or PHIP_GRID_CUS=n (environment, n >= 1, read at plan creation) in its place: every tile-walking
 * launch (filter, aggregation, distinct, selection, numGroupsLimit pass) and every buffer sized from its grid then
 * follow n CUs, while the choice of kernel variant and walk keeps following the device. A node plan returns
 * PHIP_ERR_INVALID. */
#define PHIP_SHAPE_TOTAL_WORK 0     /* 2048-doc work tiles of the query */
#define PHIP_SHAPE_FILTER_BLOCKS 1  /* workgroups of the filter launch (4 waves each) */
#define PHIP_SHAPE_AGG_BLOCKS 2     /* workgroups of the aggregation launch */
#define PHIP_SHAPE_AGG_WAVES 3      /* waves per aggregation workgroup (8 or 16) */
#define PHIP_SHAPE_NBUF 4           /* LDS-DMA ring slots per filter wave */
#define PHIP_SHAPE_WORK_SEGMENTS 5  /* entries of the work list (segments x programs the planner kept) */
#define PHIP_SHAPE_DISTINCT_BLOCKS 6 /* upper bound of the distinct pass's workgroups (4 waves each) */
#define PHIP_SHAPE_SELECT_BLOCKS 7  /* upper bound of the selection passes' workgroups (4 waves each) */
#define PHIP_SHAPE_FUSED_LEAN 8     /* 1: the filter launch was the lean fused instantiation (bit-sliced + deferred) */
#define PHIP_SHAPE_HOST_FINAL 9     /* 1: the execution ran in record mode (tagged per-block records reduced on the host, no
                                     * finalize launch; PHIP_HOST_FINAL=0 at plan creation keeps the launch) */
#define PHIP_SHAPE_SELECT_CANDIDATES 10 /* selection ORDER BY: the rows the top-K pruning pass left to gather and sort
                                         * (select_keep <= candidates <= matched when matched >= select_keep, else
                                         * = matched; saturates at INT32_MAX) */
#define PHIP_SHAPE_DISTINCT_ROWS_REGIME 11 /* SELECT DISTINCT: how the plan keeps its key set -- 0 not a distinct plan, 1
                                           * a bitmap in every workgroup's LDS, 2 a global bitmap, 3 sorted keys */
#define PHIP_SHAPE_MATCH_TASKS 12 /* RAW_STRING_MATCH leaves (one task per leaf of an unpruned segment x program entry)
                                   * the string-match launch of the execution walked; 0: no such launch */
#define PHIP_LAUNCH_SHAPE_VALUES 13
PHIP_API int32_t phip_plan_launch_shape(uint64_t plan, int32_t *out_shape, int32_t num_values);

#endif /* PINOT_HIP_H_ */
