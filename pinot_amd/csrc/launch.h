// launch.h -- the host-callable kernel launchers: the one interface between the host runtime (runtime.cpp) and the
// kernel translation units. Every launcher is declared here once and nowhere else; the header is included by the
// caller, by the .hip file that defines the launcher, and by the host simulation's stand-ins (tests/hostsim/
// hip_stub.cpp), so a signature that drifts fails to compile instead of becoming a second overload. Default arguments
// appear here only. Host types alone (device.h): it compiles without device compilation. The node plans' merge
// launchers (node_merge.hip) are in node.h.
#ifndef PINOT_HIP_LAUNCH_H_
#define PINOT_HIP_LAUNCH_H_

#include <hip/hip_runtime.h>

#include "device.h"

namespace phip {

// ---- filter.hip --------------------------------------------------------------------------------------------------
hipError_t launch_roaring_or(const RoaringTask *tasks, const RoaringGroup *groups, int32_t ngroups, hipStream_t s);
// Which filter_kernel instantiation a launch runs (filter_kernel.h; one translation unit each, filter_k_*.hip).
enum FilterVariant : int32_t {
  FV_GENERAL = 0,  // the filter-program interpreter
  FV_CONJ,         // every segment's program takes the conjunctive fast path: the interpreter is compiled out, which
                   // frees registers for more resident waves. Every variant below is conjunctive too, and has q.agg set:
  FV_FUSED,        // the aggregation runs inside (no aggregation launch)
  FV_FUSED_LEAN,   // ... in its lean shape (kBsDefer): every segment's program is the bit-sliced conjunction and
                   // every segment defers its projection -- the host decides (runtime.cpp configure_fusion)
  FV_GB,           // the dense group-by runs inside, into the HBM table (GB_GLOBAL)
  FV_GB_XCD,       // ... into kXcdCopies XCD-private copies of it (GB_XCD), merged after the launch
  FV_GB_LDS,       // ... into each workgroup's LDS table (GB_LDS), its slabs reduced after the launch
};
// naggs: the fused aggregations (FV_FUSED / FV_FUSED_LEAN: rounded up to the 1 / 2 / 4 instantiation; else unused)
// e0 / e1: optional start / stop events recorded by the kernel's own dispatch (hipExtLaunchKernel)
hipError_t launch_filter(const DevFilter &q, FilterVariant variant, int naggs, int nblocks, size_t lds_bytes,
                         hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t launch_masks_to_words(const uint32_t *masks, int32_t tile0, int32_t ntiles, uint64_t *words, int64_t nwords,
                                 hipStream_t s);
// The record mode of aggregation-only plans (host_final.h) rides in DevFilter (rec, rec_first, rec_stride, rec_tag): no
// launcher signature knows of it. The host simulation's stand-in launch_filter stores no records, so the runtime takes
// the mode only after filter.hip has said, from a static initialiser, that its kernels do (like ExprLauncher below).
void register_filter_records(bool on);  // defined in runtime.cpp

// ---- aggregate.hip -----------------------------------------------------------------------------------------------
hipError_t launch_agg(const DevAggQuery &q, const DevAggQuery *dq, int nblocks, size_t lds, hipStream_t s,
                      hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t launch_slab_reduce(const uint64_t *slab, int32_t nslabs, int32_t tbl_words, int64_t G, const int32_t *kinds,
                              uint64_t *out, const uint32_t *hslab, int32_t hll_words, uint32_t *hout, hipStream_t s);
hipError_t launch_finalize_all(const uint64_t *pa, int nba, int na, const int32_t *ka, const uint64_t *pf, int nbf,
                               const int32_t *kf, uint64_t *segm, int nseg, uint32_t *hll, int hll_words, uint64_t *out,
                               hipStream_t s, uint32_t *ticket = nullptr, uint64_t seq = 0);
hipError_t launch_xcd_init(uint64_t *tab, int64_t words, int64_t G, const int32_t *kinds, hipStream_t s);
hipError_t launch_xcd_merge(uint64_t *tab, int64_t words, int64_t G, const int32_t *kinds, uint32_t *hll,
                            int64_t hll_words, hipStream_t s);
hipError_t launch_fill_u64(uint64_t *p, int64_t n, uint64_t v, hipStream_t s);
hipError_t launch_group_count(const uint64_t *counts, int64_t n, int32_t *chunk_counts, int64_t nchunks,
                              int64_t *offsets, hipStream_t s);
hipError_t launch_group_compact(const uint64_t *counts, int64_t n, const int64_t *offsets, int64_t nchunks,
                                int64_t *keys, hipStream_t s);
hipError_t launch_group_gather(const int64_t *keys, int64_t ngroups, int64_t ndense, int32_t naggs, int32_t own_count,
                               const int32_t *kinds, const uint64_t *table, const uint32_t *hll, int32_t nhll,
                               int32_t log2m, double *vals, int64_t *longs, uint8_t *hll_out, hipStream_t s);
hipError_t launch_group_gather_mapped(const int64_t *keys, const int64_t *d_ngroups, int64_t ndense, int32_t naggs,
                                      int32_t own_count, const int32_t *kinds, const uint64_t *table,
                                      int64_t *out_count, int64_t *out_keys, double *vals, int64_t *longs,
                                      const uint32_t *hll, int32_t nhll, int32_t log2m, uint32_t *hll_out,
                                      hipStream_t s);
hipError_t launch_hash_keys(int64_t *slots, int64_t n, const uint64_t *keys, hipStream_t s);

// ---- load.hip ----------------------------------------------------------------------------------------------------
hipError_t launch_bswap32(uint32_t *p, int64_t n, hipStream_t s);
hipError_t launch_bswap64(uint64_t *p, int64_t n, hipStream_t s);
hipError_t launch_sorted_to_packed(const uint32_t *be_pairs, int32_t card, int32_t *ids_tmp, int64_t n, int32_t bits,
                                   uint32_t *words, int64_t nwords, hipStream_t s);
hipError_t launch_materialize_hll16(const uint32_t *words, int32_t bits, const uint32_t *table, int64_t n, uint16_t *out,
                                    hipStream_t s);
hipError_t launch_materialize_packed(const uint32_t *words, int32_t bits, const void *dict, int32_t width, int64_t n,
                                     int64_t base, int32_t vbits, int64_t nwords, uint32_t *out, hipStream_t s);
hipError_t launch_materialize(const uint32_t *words, int32_t bits, const void *dict, int32_t width, int64_t n,
                              void *vals, hipStream_t s);
hipError_t launch_materialize_record(const RecSrcs &fs, int nf, int64_t n, int W, uint32_t *out, hipStream_t s);
hipError_t launch_minmax_i64(const void *raw, int32_t type, int64_t n, int64_t *out, hipStream_t s,
                             const uint64_t *nulls = nullptr);
size_t chunk_decode_extra_lds(int codec, int32_t out_cap);
hipError_t launch_chunk_decode(int codec, int entry, const uint8_t *blob, const RawChunk *chunks, int32_t nchunks,
                               int32_t out_cap, int32_t in_cap, size_t lds, uint8_t *out, int32_t *err, int32_t *sizes,
                               hipStream_t s);
hipError_t launch_bitslice(const uint32_t *words, int32_t bits, int64_t ntiles, uint32_t *planes, hipStream_t s);
hipError_t launch_chunk_decode_global(int codec, const uint8_t *blob, const RawChunk *chunks, int32_t nchunks, uint8_t *out,
                                      int32_t *err, int32_t *sizes, uint8_t *lits, uint64_t lits_stride, hipStream_t s);
hipError_t launch_varbyte_offsets(const uint8_t *stage, const uint64_t *chunk_base, const int32_t *chunk_size,
                                  int32_t per_chunk, int64_t n, uint64_t *len, uint64_t *off, void *temp,
                                  size_t *temp_bytes, int32_t *err, hipStream_t s);
hipError_t launch_varbyte_copy(const uint8_t *stage, const uint64_t *chunk_base, const int32_t *chunk_size,
                               int32_t per_chunk, int64_t n, const uint64_t *off, uint8_t *out, hipStream_t s);

// ---- trim.hip ----------------------------------------------------------------------------------------------------
hipError_t launch_trim_order(const double *vals, const int64_t *keys, const KeyOrder *ko, int64_t n, int32_t naggs,
                             int32_t agg, int32_t desc, void *scratch, size_t *scratch_bytes, const int32_t **order_out,
                             hipStream_t s);
hipError_t launch_trim_order_terms(const double *vals, const int64_t *keys, const OrderTerms *ot, int64_t n,
                                   int32_t naggs, const uint8_t *hll, int64_t hll_bytes, int32_t m_regs, void *scratch,
                                   size_t *scratch_bytes, const int32_t **order_out, hipStream_t s);
hipError_t launch_trim_gather(const int32_t *order, int64_t k, int32_t naggs, int64_t hll_bytes, const int64_t *keys,
                              const double *vals, const int64_t *longs, const uint8_t *hll, int64_t *keys_out,
                              double *vals_out, int64_t *longs_out, uint8_t *hll_out, hipStream_t s);

// ---- limit.hip ---------------------------------------------------------------------------------------------------
hipError_t launch_limit_prepare(const int64_t *slots, int64_t n, const uint64_t *hkeys, const uint32_t *first_doc,
                                int32_t nseg, uint64_t *sortkey, int32_t *idx, hipStream_t s);
hipError_t launch_limit_bounds(const uint64_t *sk_sorted, int64_t n, int64_t *first, int64_t *last, hipStream_t s);
hipError_t launch_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *k_in, uint64_t *k_out, const void *v_in,
                             void *v_out, bool wide, int64_t n, int end_bit, hipStream_t s);
hipError_t launch_limit_select(const uint64_t *sk_sorted, const int32_t *idx_sorted, int64_t n, const int64_t *seg_start,
                               int64_t limit, const int64_t *slots, const uint64_t *hkeys, int32_t nseg, uint64_t *key2,
                               int64_t *slot2, hipStream_t s);
hipError_t launch_limit_runs(void *temp, size_t *scan_bytes, const uint64_t *k, int64_t n, int32_t *head, int32_t *run,
                             hipStream_t s);
hipError_t launch_limit_reduce(const uint64_t *k, const int64_t *slot2, int64_t n, const int32_t *head, const int32_t *run,
                               int64_t cap, int32_t naggs, int32_t own_count, const int32_t *kinds,
                               const uint64_t *table, const uint32_t *hll, int32_t nhll, int32_t log2m,
                               int64_t *keys_out, double *vals, int64_t *longs, uint8_t *hll_out, hipStream_t s);

// ---- select.hip --------------------------------------------------------------------------------------------------
// The count and gather walks run on at most max_blocks workgroups (4096 unless PHIP_GRID_CUS lowers it).
hipError_t launch_select_count(const DevSelQuery *q, int64_t total_work, int max_blocks, int64_t *tile_cnt,
                               hipStream_t s);
hipError_t launch_select_scan(void *temp, size_t *temp_bytes, const int64_t *in, int64_t *out, int64_t n, hipStream_t s);
hipError_t launch_select_bases(const DevSelQuery *q, int64_t *seg_base, int64_t *kept, int64_t *total, hipStream_t s);
hipError_t launch_select_str_lens(const uint64_t *loc, int64_t rows, const uint64_t *const *offs, uint32_t *lens,
                                  hipStream_t s);
hipError_t launch_select_str_bytes(const uint64_t *loc, int64_t rows, const uint8_t *const *strs,
                                   const uint64_t *const *offs, const uint64_t *dst_off, uint8_t *dst, hipStream_t s);
hipError_t launch_select_gather(const DevSelQuery *q, int64_t total_work, int max_blocks, uint64_t *out,
                                int64_t num_rows, hipStream_t s);

// ---- select_order.hip (selection ORDER BY) -----------------------------------------------------------------------
// Registered like ExprLauncher below (null in the host simulation: an ORDER BY selection is PHIP_ERR_UNSUPPORTED).
// hist / mask walk the work tiles as launch_select_count does; the runtime zeroes DevSelOrder.bins before hist. sort:
// cols = the gathered candidates [num_select][n]; *scratch_bytes on a null scratch; *order_out = the candidates'
// final order (in the scratch). rows: out[k][r] = cols[k][order[r]] for r < rows.
struct SelectOrderLaunchers {
  hipError_t (*hist)(const DevSelQuery *q, const DevSelOrder *o, int64_t total_work, int max_blocks, hipStream_t s);
  hipError_t (*pick)(const DevSelOrder *o, hipStream_t s);
  hipError_t (*mask)(const DevSelQuery *q, const DevSelOrder *o, int64_t total_work, int max_blocks, hipStream_t s);
  hipError_t (*sort)(const uint64_t *cols, int64_t n, const SelOrderTerm *terms, int32_t num_terms, void *scratch,
                     size_t *scratch_bytes, const int32_t **order_out, hipStream_t s);
  hipError_t (*rows)(const uint64_t *cols, int64_t n, int32_t ncols, const int32_t *order, int64_t rows, uint64_t *out,
                     hipStream_t s);
};
void register_select_order_launchers(const SelectOrderLaunchers *l);  // defined in runtime.cpp

// ---- distinct.hip (exact DISTINCTCOUNT) --------------------------------------------------------------------------
hipError_t launch_distinct_mark(const DevDistinctQuery *q, int64_t total_work, int lds, size_t lds_bytes,
                                int max_blocks, hipStream_t s);
hipError_t launch_distinct_finish(const DevDistinctQuery *q, const int64_t *keys, int64_t num_out, int64_t *counts,
                                  uint32_t *out, hipStream_t s);

// ---- expr.hip (derived value columns) ----------------------------------------------------------------------------
// Not a launcher the runtime calls by name: the host simulation's stand-ins define every launcher above and nothing
// else, so the runtime holds a pointer of this type (null by default: a query with derived columns is then
// PHIP_ERR_UNSUPPORTED) and expr.hip registers its launcher from a static initialiser. e: the program in device
// memory; out: num_docs values, double or (integral) int64_t.
typedef hipError_t (*ExprLauncher)(const DevExpr *e, int32_t num_docs, bool integral, void *out, hipStream_t s);
void register_expr_launcher(ExprLauncher f);  // defined in runtime.cpp

// ---- mv.hip (multi-value columns) --------------------------------------------------------------------------------
// Registered like ExprLauncher (null in the host simulation: an MV scan leaf or an MV row reduction is then
// PHIP_ERR_UNSUPPORTED). scan: `tasks` in device memory, total_tiles = the sum of their num_tiles, on at most
// max_blocks workgroups. reduce: the task by value.
struct MvLaunchers {
  hipError_t (*scan)(const MvScanTask *tasks, int32_t ntasks, int32_t total_tiles, int max_blocks, hipStream_t s);
  hipError_t (*reduce)(const MvReduceTask &t, hipStream_t s);
};
void register_mv_launchers(const MvLaunchers *l);  // defined in runtime.cpp

// ---- strmatch.hip (REGEXP_LIKE / LIKE) ---------------------------------------------------------------------------
// Registered like ExprLauncher (null in the host simulation: a RAW_STRING_MATCH leaf or phip_segment_match_dictionary
// is then PHIP_ERR_UNSUPPORTED). match: `tasks` in device memory, total_tiles = the sum of their num_tiles, on at most
// max_blocks workgroups; table_words = the largest task's table image in u32 words (it sizes the launch's LDS).
struct StrMatchLaunchers {
  hipError_t (*match)(const StrMatchTask *tasks, int32_t ntasks, int32_t total_tiles, int32_t table_words,
                      int max_blocks, hipStream_t s);
};
void register_strmatch_launchers(const StrMatchLaunchers *l);  // defined in runtime.cpp

// ---- distinct_rows.hip (SELECT DISTINCT) -------------------------------------------------------------------------
// Registered like ExprLauncher (null in the host simulation: a distinct query is then PHIP_ERR_UNSUPPORTED).
// mark: one pass over the matched docs on at most max_blocks workgroups; DR_LDS / DR_GLOBAL set the docs' key bits in
// q->bitmap (cleared by the caller), DR_SORTED writes the keys to keys[rank] for rank < num_keys. count: set bits per
// chunk of kDistinctRowsChunkWords bitmap words into chunk_cnt[0 .. nchunks) and 0 into chunk_cnt[nchunks]. emit:
// chunk_off = the exclusive prefix of chunk_cnt; the keys of rank < keep, ascending, into keys[rank]; both stride
// over the chunks on at most max_blocks workgroups. decode:
// out[k * rows + r] = SELECT column k's slot of keys[r].
struct DistinctRowsLaunchers {
  hipError_t (*mark)(const DevDistinctRows *q, int regime, int64_t total_work, size_t lds_bytes, int max_blocks,
                     uint64_t *keys, int64_t num_keys, hipStream_t s);
  hipError_t (*count)(const uint32_t *bitmap, int64_t num_words, int max_blocks, int64_t *chunk_cnt, hipStream_t s);
  hipError_t (*emit)(const uint32_t *bitmap, int64_t num_words, int max_blocks, const int64_t *chunk_off, int64_t keep,
                     uint64_t *keys, hipStream_t s);
  hipError_t (*decode)(const uint64_t *keys, int64_t rows, const DistinctRowsDecode &d, uint64_t *out, hipStream_t s);
};
void register_distinct_rows_launchers(const DistinctRowsLaunchers *l);  // defined in runtime.cpp

// ---- transform.hip (time transforms over a dictionary) ------------------------------------------------------------
// Registered like ExprLauncher (null in the host simulation: a transformed group-by key or phip_segment_match_transform
// is then PHIP_ERR_UNSUPPORTED). dict: the task in device memory, its ceil(card / 2048) tiles on at most max_blocks
// workgroups. remap: out[i] = the position of images[i] among the u ascending distinct images at uniq, i < n.
struct TransformLaunchers {
  hipError_t (*dict)(const TransformTask *task, int32_t card, int max_blocks, hipStream_t s);
  hipError_t (*remap)(const uint64_t *images, int64_t n, const uint64_t *uniq, int64_t u, int32_t *out, hipStream_t s);
};
void register_transform_launchers(const TransformLaunchers *l);  // defined in runtime.cpp

// ---- keys.hip ----------------------------------------------------------------------------------------------------
hipError_t set_str_hash_bits(int bits);
hipError_t launch_raw_images(const void *raw, int32_t type, int64_t n, uint64_t *out, hipStream_t s);
hipError_t launch_sort_unique_u64(void *temp, size_t *temp_bytes, uint64_t *in, uint64_t *sorted, uint64_t *out,
                                  int64_t *num_out, int64_t n, hipStream_t s);
hipError_t launch_raw_key_ids(const void *raw, int32_t type, int64_t n, const uint64_t *uniq, int64_t u, int32_t *ids,
                              hipStream_t s);
hipError_t launch_str_hash_unique(void *temp, size_t *temp_bytes, const uint8_t *bytes, const uint64_t *off, int64_t n,
                                  uint64_t *hash, int32_t *docs, uint64_t *hash_sorted, int32_t *docs_sorted,
                                  uint64_t *uniq, int32_t *rep, int64_t *num_out, hipStream_t s);
hipError_t launch_str_verify(const uint8_t *bytes, const uint64_t *off, int64_t n, const uint64_t *uniq, const int32_t *rep,
                             int64_t u, int32_t *collided, hipStream_t s);
hipError_t launch_str_rep_lens(const uint64_t *off, const int32_t *rep, int64_t u, uint32_t *lens, hipStream_t s);
hipError_t launch_str_rep_bytes(const uint8_t *bytes, const uint64_t *off, const int32_t *rep, int64_t u,
                                const uint64_t *dst_off, uint8_t *dst, hipStream_t s);
hipError_t launch_raw_str_ids(const uint8_t *bytes, const uint64_t *off, int64_t n, const uint64_t *uniq, int64_t u,
                              const int32_t *map, int32_t *ids, hipStream_t s);
hipError_t launch_tuple_words(const TupleCols &tc, int64_t n, uint64_t *out, hipStream_t s);
hipError_t launch_tuple_rank(void *temp, size_t *temp_bytes, const uint64_t *words, int32_t nw, int64_t n, int32_t *ids,
                             uint64_t *uniq, int64_t ucap, int64_t *num_out, hipStream_t s);
hipError_t launch_gather_ids(const int32_t *local, const int32_t *map, int64_t n, int32_t *out, hipStream_t s);

}  // namespace phip

#endif  // PINOT_HIP_LAUNCH_H_
