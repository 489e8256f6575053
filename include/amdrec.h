/* libamdrec - C ABI of the MI355X-native retrieval + ranking hot path.
 *
 * The reference (saitejasrivilli/movie-recommender-demo) is pure Python and defines no FFI:
 * its boundary is the Python class surface (two_tower_model.py, transformer_ranker.py,
 * faiss_retrieval.py, inference.py) plus the faiss / ATen calls behind it.  Each entry point
 * below replaces one of those third-party call sites (cited per function); the Python
 * drop-ins in movie-recommender-demo_amd/amdrec bind them with ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer on the current HIP device unless marked "host";
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *    asynchronously on it, nothing synchronises with the host, nothing allocates: scratch
 *    memory is a caller-provided, 256-byte aligned `workspace` sized by the matching
 *    *_workspace() query;
 *  - return value: 0 = ok, < 0 = error (AMDREC_E*); amdrec_last_error() returns the message
 *    of the calling thread's last error;
 *  - matrices are row-major float32; `ld*` = leading dimension in elements.
 */
#ifndef AMDREC_H
#define AMDREC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMDREC_ABI_VERSION 14 /* (v14 later gained amdrec_exclude_compact, then amdrec_remove_plan[_workspace] and amdrec_rows_gather:
                               * added exports, nothing else changed; and the
                               * first-FFN hidden cache: amdrec_ranker_project_ads_hidden, amdrec_x3_weights.stream_hc ... at the
                               * struct's end, amdrec_ranker_params.ad_hidden_cache - the number stays, the library and its
                               * binding ship together and the struct layouts are checked against the compiler, tests/test_abi.py;
                               * amdrec_select_topk then gained its cand_pos argument under the same rule; so did CTR-first ranking:
                               * amdrec_ranker_forward_ctr_first ..., amdrec_x3_weights.stream_ctr ... at the struct's end; and
                               * the eligibility masks: amdrec_flat_search_eligible, amdrec_flat_search_mixed_eligible, added exports; then
                               * the same masks in the inverted-list scans: amdrec_ivf_scan_eligible, amdrec_ivf_scan_grouped_eligible,
                               * amdrec_ivf_scan_grouped_mixed_eligible, amdrec_ivfpq_scan_finite_eligible, added exports; then
                               * the per-group caps: amdrec_select_topk_capped, amdrec_group_cap_compact, added exports; then
                               * auction ranking: amdrec_select_topk_auction, an added export; then
                               * per-ad score boosts: amdrec_flat_search_boosted, amdrec_flat_search_mixed_boosted, added exports; then
                               * the same boosts in the inverted-list scans: amdrec_ivf_scan[_grouped[_mixed]][_eligible]_boosted and
                               * amdrec_ivf_filter_bounds_boosted, added exports; then
                               * value ranking: amdrec_select_topk_value, amdrec_select_topk_value_auction, added exports; then
                               * candidate injection: amdrec_include_merge, an added export; then
                               * exploration: amdrec_select_topk_sampled, an added export.
                               * A library that reports v14 may therefore carry any prefix of these additions: a caller that
                               * needs one of them probes for the symbol (dlsym; amdrec._lib.exported_symbols() lists what the
                               * Python binding requires and load() fails on a library that lacks one)) */
#define AMDREC_MAX_K 2048
#define AMDREC_MAX_INCLUDE 64 /* entries of a per-request must-consider list (amdrec_include_merge) */

int amdrec_abi_version(void);
const char* amdrec_last_error(void);

/* ---- retrieval: exact inner-product top-k over a flat corpus ---------------------------
 * Replaces faiss IndexFlatIP.search as called by FAISSIndex.search (faiss_retrieval.py:155):
 * scores = queries . corpus^T, k largest per query, sorted descending (ties: lower position
 * first).  out_pos = position in the corpus + pos_offset (the shard's first global row),
 * unfilled slots (k > nrows) = -1 / -inf like faiss.  Rows are expected L2-normalised by the
 * caller (amdrec_l2_normalize), as FAISSIndex.add/search do (:114-115, :146-147).
 * n_fixup (device int, may be NULL) receives the number of queries that took the slow
 * exact fix-up path.  dim % 4 == 0, dim <= 2048, 1 <= k <= AMDREC_MAX_K.
 * Non-finite input: a row whose score against the query is NaN (a NaN coordinate in the row or in the
 * query, inf * 0, inf - inf) is never returned; the result is the exact top-k of the other rows, and the
 * slots they cannot fill are -1 / -inf also when k <= nrows.  The mixed form below gives the same result,
 * and counts EVERY query in n_fixup when max_norm is non-finite (a NaN or inf in the shadowed corpus). */
int amdrec_flat_search_workspace(int64_t nq, int64_t nrows, int k, size_t* bytes /*host*/);
int amdrec_flat_search(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                       const float* queries, int64_t nq, int64_t ld_queries, int k,
                       int64_t pos_offset, float* out_scores /*[nq][k]*/,
                       int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                       int* n_fixup, void* stream);

/* Mixed-precision form of the same search (same result contract: the exact fp32 top-k).  The sample and filter
 * passes read `corpus_bf16`, a bf16 (round-to-nearest) copy of the corpus made by amdrec_bf16_rows, with the bf16
 * MFMA; candidates are re-scored in fp32 from `corpus` and the result is certified against the error bound
 * eps = ||dq|| (M + D) + ||q|| D + 2 dim 2^-24 ||q|| (M + D),  dq = bf16(q) - q,  M = max_norm[0] = the largest row norm
 * and D = max_norm[1] = the largest row rounding-error norm ||x - bf16(x)|| of the corpus (max_norm: device float[2],
 * accumulated by amdrec_bf16_rows; at worst eps = (2^-7 + 2^-16) ||q|| M, the both-operands-half-an-ulp-off case);
 * uncertified queries take the exact fp32 fix-up scan.  dim % 8 == 0.
 * Turns the filter pass from fp32-MFMA-bound into memory-bound (half the bytes, 16x the MFMA rate). */
int amdrec_bf16_rows(const float* x, int64_t rows, int64_t ld, int dim, uint16_t* out /*[rows][ld_out] bf16*/,
                     int64_t ld_out, float* max_norm /*device float[2], in/out (atomic max), may be NULL*/, void* stream);
int amdrec_flat_search_mixed_workspace(int64_t nq, int64_t nrows, int k, int dim, size_t* bytes /*host*/);
int amdrec_flat_search_mixed(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                             const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                             const float* queries, int64_t nq, int64_t ld_queries, int k,
                             int64_t pos_offset, float* out_scores /*[nq][k]*/,
                             int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                             int* n_fixup, void* stream);

/* Per-request eligibility masks: the same two searches over the rows each query may be shown.  One 64-bit tag per
 * corpus row (`tags`, exactly nrows words; the library does not interpret the bits), two 64-bit words per query; row r is
 * eligible for query q iff
 *     (tags[r] & require_all[q]) == require_all[q]  and  (require_any[q] == 0 or (tags[r] & require_any[q]) != 0),
 * so require_all = require_any = 0 admits every row.  Result: the exact top-k of the query's ELIGIBLE rows in the search's
 * own order (score descending, ties -> lower position), the scores the plain search returns for those rows; the NaN rule
 * above holds; with fewer than k eligible rows the tail is unfilled (-inf / -1) - such a query takes the exact
 * fix-up scan and is counted in n_fixup.  The predicate is tested inside the corpus pass
 * where a row enters the candidate pool, so the number of ineligible rows is not limited (unlike an exclusion list).
 * All three are device pointers and all three are required (tags 64-byte aligned, the masks 8-byte aligned); workspace: the
 * size the matching *_workspace query gives. */
int amdrec_flat_search_eligible(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                const float* queries, int64_t nq, int64_t ld_queries, int k,
                                int64_t pos_offset, float* out_scores /*[nq][k]*/,
                                int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                                int* n_fixup, void* stream, const uint64_t* tags /*[nrows]*/,
                                const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/);
int amdrec_flat_search_mixed_eligible(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                      const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                                      const float* queries, int64_t nq, int64_t ld_queries, int k,
                                      int64_t pos_offset, float* out_scores /*[nq][k]*/,
                                      int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                                      int* n_fixup, void* stream, const uint64_t* tags /*[nrows]*/,
                                      const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/);

/* Per-ad score boosts: the same two searches under the retrieval key
 *     s(q, r) = ip(q, r) + weight[q] * boost[r],
 * one float per corpus row (`boost`, exactly nrows values, finite), one float per query (`weight`).  ip is the score the
 * matching plain entry returns for the row; t = weight[q] * boost[r] is one rounded fp32 multiply and s = ip + t one rounded
 * fp32 add - two roundings, never a fused multiply-add.  Result: the exact top-k under s (s descending, ties -> lower
 * position), s returned as the score; a row whose ip is NaN is never returned; unfilled slots as above; a query with
 * weight 0 gets the plain search's positions.  The key is evaluated inside the corpus pass (sample, filter, re-score and
 * fix-up scan all see it), so a boost can lift a row from any rank.  `boost_max`: a host upper bound of max |boost|, used by
 * the mixed form's error bound only (a bound that is too small can cost exactness, one that is too large only speed).
 * Both pointers are device pointers and required (boost 64-byte aligned); workspace: the size the matching *_workspace
 * query gives. */
int amdrec_flat_search_boosted(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                               const float* queries, int64_t nq, int64_t ld_queries, int k,
                               int64_t pos_offset, float* out_scores /*[nq][k]*/,
                               int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                               int* n_fixup, void* stream, const float* boost /*[nrows]*/,
                               const float* weight /*[nq]*/, float boost_max);
int amdrec_flat_search_mixed_boosted(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                     const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                                     const float* queries, int64_t nq, int64_t ld_queries, int k,
                                     int64_t pos_offset, float* out_scores /*[nq][k]*/,
                                     int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                                     int* n_fixup, void* stream, const float* boost /*[nrows]*/,
                                     const float* weight /*[nq]*/, float boost_max);

/* ---- retrieval: IVF-Flat (faiss IndexIVFFlat, METRIC_INNER_PRODUCT, IndexFlatIP quantizer:
 * faiss_retrieval.py:50-55, searched at :150-155 with index.nprobe = nprobe) ---------------------
 * Layout: corpus rows stored list-contiguous `lists[N][ld]` (list l = rows [list_off[l], list_off[l+1]))
 * with row_pos[r] = position of stored row r in insertion order.  A search is
 *   1. amdrec_flat_search(centroids, nlist, ..., k = nprobe)  -> probes[nq][nprobe]  (-1 = none)
 *   2. pool_base[q][p] = exclusive prefix sum of the probed lists' lengths (host-side plumbing)
 *   3. amdrec_ivf_scan   -> pool_keys[q][pool_base[q][p] + i] = key(score, row_pos + pos_offset)
 *   4. amdrec_ivf_select -> exact k best of each query's pool, (score desc, position asc).
 * The scan is exact over the probed lists; which lists are probed depends on the trained centroids. */
int amdrec_ivf_scan(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                    const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                    const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                    int64_t pool_ld, int64_t pos_offset, void* stream);
/* Batched form of step 3: the (query, probe) pairs sorted by list (pair_query / pair_probe, group_off
 * [nlist+1]); qtile_prefix[nlist+1] = prefix sum of ceil(group size / qtile); qtile_bound >= qtile_prefix[nlist]
 * (a host-side upper bound, e.g. pairs/qtile + nlist, <= 65535).  Every list is read once per qtile-query group
 * by an fp32-MFMA GEMM tile instead of once per probing query; qtile = 64, or 32 when the groups are sparse (few probing
 * queries per list) - the value given to amdrec_ivf_group.  Same pool layout and keys as amdrec_ivf_scan. */
int amdrec_ivf_scan_grouped(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                            const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries,
                            int64_t ld_queries, const int64_t* group_off, const int64_t* qtile_prefix,
                            int64_t qtile_bound, int qtile, const int64_t* pair_query, const int64_t* pair_probe,
                            const int64_t* pool_base, int nprobe, uint64_t* pool_keys, int64_t pool_ld,
                            int64_t pos_offset, const float* tau /*or NULL*/, int64_t ld_tau,
                            int64_t* pool_fill /*[nq] or NULL*/, void* stream);
/* Filter mode of the grouped scan (tau != NULL): a row's key is kept only if its score >= tau[q * ld_tau], appended to
 * query q's pool row at pool_fill[q]++ (seeded by the caller with the keys already there; pool_base is not used).
 * With tau[q] = the k-th score over a SUBSET of the probed lists (a lower bound of the final k-th score) the union of
 * that subset's keys and the kept rows of the remaining lists contains the exact top-k: amdrec.ivf scans the nearest
 * eighth of the probes unfiltered, selects, and scans the rest with this filter - the pool shrinks ~5x. */
/* The same filter mode with a bf16 PREFILTER (ABI v10; same call site, faiss_retrieval.py:150-155): the (list, query tile)
 * GEMMs run on `lists_bf16` / `queries_bf16` (round-to-nearest copies made by amdrec_bf16_rows; the lists' copy also yields
 * max_norm[2] = {largest row norm, largest row rounding-error norm}) with the bf16 MFMA and only nominate rows: a row whose
 * bf16 score is >= tau_lo[q] is re-scored in fp32 from `lists` / `queries` and appended to query q's pool row at
 * pool_fill[q]++ if that exact score passes tau[q * ld_tau].  With tau_lo[q] = tau[q] - eps_q (amdrec_ivf_filter_bounds: the
 * flat search's error bound, see amdrec_flat_search_mixed) every row with fp32 score >= tau is nominated, so the pool
 * receives the same rows as amdrec_ivf_scan_grouped's filter mode, with fp32 keys.  dim % 8 == 0. */
int amdrec_ivf_filter_bounds(const float* queries, int64_t nq, int64_t ld_queries, int dim,
                             const uint16_t* queries_bf16, int64_t ld_queries_bf16, const float* max_norm /*device float[2]*/,
                             const float* tau, int64_t ld_tau, float* tau_lo /*[nq]*/, void* stream);
int amdrec_ivf_scan_grouped_mixed(const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim,
                                  const int64_t* row_pos, const int64_t* list_off, int nlist, int64_t max_list_rows,
                                  const float* queries, int64_t ld_queries, const uint16_t* queries_bf16,
                                  int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
                                  int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys,
                                  int64_t pool_ld, int64_t pos_offset, const float* tau, int64_t ld_tau,
                                  const float* tau_lo /*[nq]*/, int64_t* pool_fill /*[nq]*/, void* stream);
/* Per-request eligibility masks in the list scans: the three scans above over the rows each query may be shown (the
 * contract of amdrec_flat_search_eligible).  Each entry takes the argument list of its plain twin plus three device
 * pointers, all required and 8-byte aligned (checked with the other arguments, before the first HIP call):
 *   list_tags   [N]  one 64-bit tag per LIST-ORDER row, list_tags[r] = tag of corpus row row_pos[r]; exactly N words read,
 *   require_all [nq] / require_any [nq]: indexed by the query numbers of the call - those of `queries` / `probes` /
 *   pair_query (a driver that passes queries + s per chunk offsets the masks the same way).
 * Row r is eligible for query q iff (list_tags[r] & require_all[q]) == require_all[q] and (require_any[q] == 0 or
 * (list_tags[r] & require_any[q]) != 0).  nq == 0 / nothing to scan: AMDREC_OK as the plain twins.
 * The KEY-0 rule: where a scan writes a slot per (query, row) - amdrec_ivf_scan_eligible, amdrec_ivf_scan_grouped_eligible
 * with tau == NULL - the slot of an ineligible pair is written as key 0, the value amdrec_ivf_select[_split] treats as
 * an empty slot (skipped by its histograms and its gather); it is written, not skipped, because the pool is not cleared
 * between searches, and pool_base / pool_count stay the slot counts of the plain scan.  In filter mode (tau != NULL) the
 * predicate is and-ed with score >= tau: an ineligible row is not appended.  amdrec_ivf_scan_grouped_mixed_eligible tests
 * the predicate at nomination, BEFORE the re-score: an ineligible row costs neither a nomination slot nor the fp32 row read.
 * An eligible row's key is, bit for bit, the key its plain twin writes for it.  With tau[q] = the k-th score of the
 * ELIGIBLE rows of a subset of the probes (-inf with fewer than k) the two-phase search stays exact. */
int amdrec_ivf_scan_eligible(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                             const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                             const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                             int64_t pool_ld, int64_t pos_offset, void* stream, const uint64_t* list_tags /*[N], list order*/,
                             const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/);
int amdrec_ivf_scan_grouped_eligible(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                     const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries,
                                     int64_t ld_queries, const int64_t* group_off, const int64_t* qtile_prefix,
                                     int64_t qtile_bound, int qtile, const int64_t* pair_query, const int64_t* pair_probe,
                                     const int64_t* pool_base, int nprobe, uint64_t* pool_keys, int64_t pool_ld,
                                     int64_t pos_offset, const float* tau /*or NULL*/, int64_t ld_tau,
                                     int64_t* pool_fill /*[nq] or NULL*/, void* stream,
                                     const uint64_t* list_tags /*[N], list order*/, const uint64_t* require_all /*[nq]*/,
                                     const uint64_t* require_any /*[nq]*/);
int amdrec_ivf_scan_grouped_mixed_eligible(const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim,
                                           const int64_t* row_pos, const int64_t* list_off, int nlist, int64_t max_list_rows,
                                           const float* queries, int64_t ld_queries, const uint16_t* queries_bf16,
                                           int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
                                           int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys,
                                           int64_t pool_ld, int64_t pos_offset, const float* tau, int64_t ld_tau,
                                           const float* tau_lo /*[nq]*/, int64_t* pool_fill /*[nq]*/, void* stream,
                                           const uint64_t* list_tags /*[N], list order*/, const uint64_t* require_all /*[nq]*/,
                                           const uint64_t* require_any /*[nq]*/);
/* Stage-1 score boosts in the list scans: the three scans above, and their *_eligible twins, under the retrieval key of
 * amdrec_flat_search_boosted,
 *     s(q, r) = ip(q, r) + weight[q] * boost[r],
 * where ip is, bit for bit, the score the twin without the boost files for the row, t = weight[q] * boost[r] one rounded
 * fp32 multiply and s = ip + t one rounded fp32 add (never fused); s is what the key holds, under the scans' own rule (a NaN
 * s is filed as -inf).  Each entry takes the argument list of its twin plus two device pointers, both required and 4-byte
 * aligned (checked with the other arguments, before the first HIP call):
 *   list_boosts [N]  one float per LIST-ORDER row, list_boosts[r] = boost of corpus row row_pos[r]; exactly N values read,
 *   weight      [nq] indexed by the query numbers of the call, as require_all / require_any are.
 * Slot mode files key(s) where the twin files key(ip) (key 0 for an ineligible pair as before); filter mode keeps a row when
 * s >= tau[q * ld_tau] - with tau[q] = the k-th BOOSTED score over a subset of the probes, still a lower bound of the final
 * k-th boosted score, the two-phase search stays exact.  The bf16 prefilter nominates on fl(bf16 score + t) >= tau_lo[q] and
 * files fl(fp32 re-score + t); its tau_lo comes from amdrec_ivf_filter_bounds_boosted (the plain entry's arguments + weight
 * and boost_max, a finite host upper bound of max |boost|), which widens the plain bound for the two roundings:
 *     tau_lo = tau - eps_q - c (|weight[q]| boost_max + ||q|| (M + D) + eps_q),   c = 3e-7 >= 5 * 2^-24
 * (derivation: csrc/ivf.hip, above ivf_filter_bounds_kernel).  A non-finite bound re-scores every row, as in the plain entry.
 * The probes are the caller's: a boost does not change which lists are scanned. */
int amdrec_ivf_scan_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                            const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                            const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                            int64_t pool_ld, int64_t pos_offset, void* stream, const float* list_boosts /*[N], list order*/,
                            const float* weight /*[nq]*/);
int amdrec_ivf_scan_eligible_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                     const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                                     const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                                     int64_t pool_ld, int64_t pos_offset, void* stream,
                                     const uint64_t* list_tags /*[N], list order*/, const uint64_t* require_all /*[nq]*/,
                                     const uint64_t* require_any /*[nq]*/, const float* list_boosts /*[N], list order*/,
                                     const float* weight /*[nq]*/);
int amdrec_ivf_scan_grouped_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                    const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries,
                                    int64_t ld_queries, const int64_t* group_off, const int64_t* qtile_prefix,
                                    int64_t qtile_bound, int qtile, const int64_t* pair_query, const int64_t* pair_probe,
                                    const int64_t* pool_base, int nprobe, uint64_t* pool_keys, int64_t pool_ld,
                                    int64_t pos_offset, const float* tau /*or NULL*/, int64_t ld_tau,
                                    int64_t* pool_fill /*[nq] or NULL*/, void* stream,
                                    const float* list_boosts /*[N], list order*/, const float* weight /*[nq]*/);
int amdrec_ivf_scan_grouped_eligible_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                             const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries,
                                             int64_t ld_queries, const int64_t* group_off, const int64_t* qtile_prefix,
                                             int64_t qtile_bound, int qtile, const int64_t* pair_query,
                                             const int64_t* pair_probe, const int64_t* pool_base, int nprobe,
                                             uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
                                             const float* tau /*or NULL*/, int64_t ld_tau, int64_t* pool_fill /*[nq] or NULL*/,
                                             void* stream, const uint64_t* list_tags /*[N], list order*/,
                                             const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/,
                                             const float* list_boosts /*[N], list order*/, const float* weight /*[nq]*/);
int amdrec_ivf_filter_bounds_boosted(const float* queries, int64_t nq, int64_t ld_queries, int dim,
                                     const uint16_t* queries_bf16, int64_t ld_queries_bf16,
                                     const float* max_norm /*device float[2]*/, const float* tau, int64_t ld_tau,
                                     float* tau_lo /*[nq]*/, void* stream, const float* weight /*[nq]*/, float boost_max);
int amdrec_ivf_scan_grouped_mixed_boosted(const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim,
                                          const int64_t* row_pos, const int64_t* list_off, int nlist, int64_t max_list_rows,
                                          const float* queries, int64_t ld_queries, const uint16_t* queries_bf16,
                                          int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
                                          int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys,
                                          int64_t pool_ld, int64_t pos_offset, const float* tau, int64_t ld_tau,
                                          const float* tau_lo /*[nq]*/, int64_t* pool_fill /*[nq]*/, void* stream,
                                          const float* list_boosts /*[N], list order*/, const float* weight /*[nq]*/);
int amdrec_ivf_scan_grouped_mixed_eligible_boosted(
    const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim, const int64_t* row_pos,
    const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries, int64_t ld_queries,
    const uint16_t* queries_bf16, int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
    int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
    const float* tau, int64_t ld_tau, const float* tau_lo /*[nq]*/, int64_t* pool_fill /*[nq]*/, void* stream,
    const uint64_t* list_tags /*[N], list order*/, const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/,
    const float* list_boosts /*[N], list order*/, const float* weight /*[nq]*/);
/* Step 1 as a dense key table (replaces the `index.search` of faiss's IndexFlatIP quantizer inside IndexIVFFlat.search,
 * faiss_retrieval.py:50-55, :150-155): keys[q][c] = 64-bit (score of query q against centroid c, ~c) for every centroid -
 * the pool format of amdrec_ivf_select, which then yields the nprobe best centroids per query (score desc, lower centroid
 * first).  Same fp32-MFMA scores as amdrec_flat_search over the centroid table, without its candidate machinery.
 * keys: 16-byte aligned; ld_keys even and >= nlist (an odd nlist's last pair writes one padding key). */
int amdrec_ivf_coarse_keys(const float* centroids, int nlist, int64_t ld_centroids, int dim, const float* queries,
                           int64_t nq, int64_t ld_queries, uint64_t* keys /*[nq][ld_keys]*/, int64_t ld_keys, void* stream);
/* Aware probes (opt-in per index; amdrec/probes.py has the rule): the same table with the request's masks and boost weight
 * applied per LIST through per-list summaries.  keys[q][l] = 0 - the empty slot amdrec_ivf_select skips - when list l is
 * empty (list_len[l] == 0) or, with masks, (tag_or[l] & require_all[q]) != require_all[q] or (require_any[q] != 0 and
 * (tag_or[l] & require_any[q]) == 0); else the key of s = c + w * b (two rounded fp32 operations; b = boost_hi[l] for
 * w = weight[q] >= 0, boost_lo[l] otherwise) with c the score amdrec_ivf_coarse_keys files, bit for bit; s = c without a
 * weight.  tag_or / require_all / require_any: all three or none (NULL); boost_hi / boost_lo / weight likewise.  The per-list
 * arrays are 16-byte aligned and hold nlist entries (nothing is read beyond); an odd nlist's padding key is written as 0. */
int amdrec_ivf_coarse_keys_aware(const float* centroids, int nlist, int64_t ld_centroids, int dim, const float* queries,
                                 int64_t nq, int64_t ld_queries, uint64_t* keys /*[nq][ld_keys]*/, int64_t ld_keys,
                                 const int64_t* list_len /*[nlist]*/, const uint64_t* tag_or /*[nlist]*/,
                                 const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/,
                                 const float* boost_hi /*[nlist]*/, const float* boost_lo /*[nlist]*/,
                                 const float* weight /*[nq]*/, void* stream);
/* The summaries: tag_or[l] = OR of list_tags over list l's rows [list_off[l], list_off[l+1]) (list_tags NULL: not written),
 * boost_hi[l] / boost_lo[l] = max / min of list_boosts over them (list_boosts NULL: not written); an empty list gets 0 / 0.0.
 * Exact (order-independent reductions, no atomics).  Made when the list-order copies are made, never at search time. */
int amdrec_ivf_list_summaries(const int64_t* list_off /*[nlist+1]*/, int nlist, const uint64_t* list_tags /*[N] or NULL*/,
                              const float* list_boosts /*[N] or NULL*/, uint64_t* tag_or /*[nlist]*/, float* boost_hi /*[nlist]*/,
                              float* boost_lo /*[nlist]*/, void* stream);
int amdrec_ivf_select(const uint64_t* pool_keys, int64_t pool_ld, const int64_t* pool_count /*[nq]*/,
                      int64_t nq, int k, float* out_scores /*[nq][k]*/, int64_t* out_pos /*[nq][k]*/,
                      void* stream);
/* The same selection for FEW queries with LARGE pools (one request against nlist 100 / nprobe 10 at 1M ads: 100 000 keys):
 * `slices` workgroups per query select the k best of a slice of the pool each into workspace[nq][slices][k] (64-bit keys:
 * nq * slices * k * 8 bytes), the last one to finish (a ticket per query: tickets[nq], int32, zero on entry, zero again
 * on return) selects the k best of those.  Same result as amdrec_ivf_select. */
int amdrec_ivf_select_split(const uint64_t* pool_keys, int64_t pool_ld, const int64_t* pool_count /*[nq]*/, int64_t nq, int k,
                            int slices, float* out_scores, int64_t* out_pos, void* workspace, size_t workspace_bytes,
                            int32_t* tickets, void* stream);
/* Step 2 as kernels (no host sync, capturable): from probes[nq][nprobe] and the list lengths, the pool layout
 * (pool_base[nq][nprobe], pool_count[nq]) and the (query, probe) pairs grouped by list for amdrec_ivf_scan_grouped
 * (pair_query / pair_probe [nq*nprobe], group_off / qtile_prefix [nlist+1]; order inside a group is unspecified - it
 * does not influence any result).  workspace: >= 4*(nlist+1) + 4*nq*nprobe + 512 bytes. */
int amdrec_ivf_group(const int64_t* probes /*[nq][ld_probes], the first nprobe columns*/, int64_t ld_probes, int64_t nq,
                     int nprobe, int nlist, const int64_t* list_len /*[nlist]*/,
                     int64_t* pool_base, int64_t* pool_count, int64_t* pair_query, int64_t* pair_probe,
                     int64_t* group_off, int64_t* qtile_prefix, int qtile /*32 or 64*/, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Index build (faiss IndexIVFFlat.train / .add behind FAISSIndex.train / .add, faiss_retrieval.py:83-95, :118).
 * amdrec_ivf_assign: assign[r] = arg max_c <x[r], centroids[c]> (the IndexFlatIP quantizer; ties -> lower c;
 * fp32 MFMA GEMM with an arg-max epilogue), best_score optional.  workspace: >= 8*rows + 256 bytes.
 * amdrec_ivf_kmeans_step: one spherical Lloyd iteration in place: assign, per-centroid sum (64-bit fixed-point integer
 * atomics: order-independent, so training is bit-reproducible), centroid = sum / |sum| (empty clusters keep theirs). */
int amdrec_ivf_assign(const float* x, int64_t rows, int64_t ld, int dim, const float* centroids, int nlist,
                      int64_t ld_centroids, int64_t* assign /*[rows]*/, float* best_score /*[rows] or NULL*/,
                      void* workspace, size_t workspace_bytes, void* stream);
int amdrec_ivf_kmeans_workspace(int64_t rows, int dim, int nlist, size_t* bytes /*host*/);
int amdrec_ivf_kmeans_step(const float* x, int64_t rows, int64_t ld, int dim, float* centroids /*in/out*/, int nlist,
                           int64_t ld_centroids, void* workspace, size_t workspace_bytes, void* stream);

/* ---- retrieval: IVFPQ (faiss IndexIVFPQ(IndexFlatIP quantizer, d, nlist, m, 8): metric L2, by_residual; faiss_retrieval.py
 * :56-63, searched at :150-155) - ABI v11 ---------------------------------------------------------------------------------
 * The coarse level is the IVF index's (centroids, amdrec_ivf_assign, amdrec_ivf_coarse_keys + amdrec_ivf_select,
 * amdrec_ivf_group).  m in {4, 8, 16, 32} sub-spaces of dsub = dim / m values (dim % m == 0, dsub % 4 == 0, dim <= 2048),
 * 256 codewords each: codebooks [m][256][dsub] fp32.  x rows are L2-normalised, assign[r] their list, the residual is
 * x[r] - centroids[assign[r]].
 * amdrec_ivfpq_encode: codes[r][s] = arg min_j |residual_s - C_s[j]|^2 (computed as arg max <r_s, C_s[j]> - |C_s[j]|^2 / 2;
 * ties -> lower j), uint8 [rows][m].
 * amdrec_ivfpq_train_step: one L2 Lloyd iteration of every sub-space in place (encode + 64-bit fixed-point sums: order-
 * independent, bit-reproducible); an empty codeword keeps its value; a row with a non-finite coordinate adds to no
 * codeword.  rows <= 2^20. */
int amdrec_ivfpq_encode(const float* x, int64_t rows, int64_t ld, int dim, const int64_t* assign, const float* centroids,
                        int64_t ld_centroids, int nlist, const float* codebooks, int m, uint8_t* codes /*[rows][m]*/,
                        void* stream);
int amdrec_ivfpq_train_workspace(int64_t rows, int dim, int m, size_t* bytes /*host*/);
int amdrec_ivfpq_train_step(const float* x, int64_t rows, int64_t ld, int dim, const int64_t* assign, const float* centroids,
                            int64_t ld_centroids, int nlist, float* codebooks /*in/out*/, int m, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Search: probes[nq][nprobe] (amdrec_ivf_select over amdrec_ivf_coarse_keys) ->
 *   amdrec_ivfpq_tables: tables[q * nprobe + p][s][j] = |(queries[q] - centroids[probes[q][p]])_s - C_s[j]|^2 (fp32)
 *   amdrec_ivf_group (qtile 32 or 64) -> amdrec_ivfpq_scan: pool_keys[q][pool_base[q][p] + i] = key(-sum_s table[code_s],
 *       row_pos + pos_offset) over the rows of every probed list (codes stored list-contiguous [N][m], 16-byte aligned);
 *       amdrec_ivfpq_scan_finite (ABI v13) is the same scan where list l's rows at or past list_off[l] + list_finite[l]
 *       (rows with a non-finite coordinate, kept at the end of their list) get key(-inf, pos): after every finite row
 *   amdrec_ivf_select -> (score desc = distance asc, position asc) -> amdrec_ivfpq_distances: distances = -scores
 *   (unfilled slots: +inf). */
int amdrec_ivfpq_tables(const float* queries, int64_t nq, int64_t ld_queries, int dim, const int64_t* probes,
                        int64_t ld_probes, int nprobe, const float* centroids, int64_t ld_centroids, int nlist,
                        const float* codebooks, int m, float* tables /*[nq*nprobe][m][256]*/, void* stream);
int amdrec_ivfpq_scan(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off, int nlist,
                      int64_t max_list_rows, const float* tables, int nprobe, const int64_t* group_off,
                      const int64_t* qtile_prefix, int64_t qtile_bound, int qtile, const int64_t* pair_query,
                      const int64_t* pair_probe, const int64_t* pool_base, int64_t npairs, uint64_t* pool_keys,
                      int64_t pool_ld, int64_t pos_offset, void* stream);
int amdrec_ivfpq_scan_finite(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off,
                             const int64_t* list_finite /*[nlist]*/, int nlist, int64_t max_list_rows, const float* tables,
                             int nprobe, const int64_t* group_off, const int64_t* qtile_prefix, int64_t qtile_bound,
                             int qtile, const int64_t* pair_query, const int64_t* pair_probe, const int64_t* pool_base,
                             int64_t npairs, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset, void* stream);
/* amdrec_ivfpq_scan_finite over the rows each query may be shown: list_tags / require_all / require_any and the key-0 rule
 * as amdrec_ivf_scan_grouped_eligible above (both loops, the finite rows and the -inf tail, store key 0 for an ineligible
 * (query, row) pair); an eligible row's key is the plain scan's. */
int amdrec_ivfpq_scan_finite_eligible(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off,
                                      const int64_t* list_finite /*[nlist]*/, int nlist, int64_t max_list_rows,
                                      const float* tables, int nprobe, const int64_t* group_off, const int64_t* qtile_prefix,
                                      int64_t qtile_bound, int qtile, const int64_t* pair_query, const int64_t* pair_probe,
                                      const int64_t* pool_base, int64_t npairs, uint64_t* pool_keys, int64_t pool_ld,
                                      int64_t pos_offset, void* stream, const uint64_t* list_tags /*[N], list order*/,
                                      const uint64_t* require_all /*[nq]*/, const uint64_t* require_any /*[nq]*/);
int amdrec_ivfpq_distances(const float* scores /*[nq][k]*/, int64_t nq, int k, float* distances /*[nq][k], may alias*/,
                           void* stream);
/* Refine (ABI v14; faiss IndexRefineFlat over the IVFPQ index): re-rank each query's kc candidates (corpus positions as
 * amdrec_ivf_select writes them, -1 = unfilled, distinct within a query) by the exact squared L2 distance sum_i (q_i - x_i)^2
 * in fp32 to the kept row x = rows[pos] (fp32, or with rows_bf16 = 1 bf16 widened to fp32), and write the k <= kc best:
 * out_dist ascending (ties -> lower position), out_pos = position + pos_offset.  A row with finite[pos] == 0 (finite may be
 * NULL: every row finite), or whose distance is NaN, gets +inf and ranks after every finite row, by position; unfilled
 * candidates and positions outside [0, nrows) come last as +inf / -1.  A row's distance is evaluated in one fixed order: it
 * does not depend on nq, on the other candidates or on the launch shape.  1 <= k <= kc <= AMDREC_MAX_K, dim % 4 == 0
 * (% 8 for bf16 rows), nq <= 65535.  Few queries are split over several workgroups each when the caller gives
 * `workspace` (>= nq * kc * 8 bytes) and `tickets` (int32 [nq], zero on entry, zero again on return); both may be NULL. */
int amdrec_ivfpq_rerank(const void* rows, int rows_bf16, int64_t nrows, int64_t ld_rows, int dim,
                        const uint8_t* finite /*[nrows] or NULL*/, const float* queries, int64_t nq, int64_t ld_queries,
                        const int64_t* cand_pos /*[nq][kc]*/, int kc, int64_t pos_offset, int k,
                        float* out_dist /*[nq][k]*/, int64_t* out_pos /*[nq][k]*/, void* workspace, size_t workspace_bytes,
                        int32_t* tickets, void* stream);

/* Cross-shard merge (absent in the single-device reference): for queries
 * [q0, q0+nq) merge n_lists per-shard top-k lists (scores/positions of list g start
 * g*list_stride_bytes after the base pointers; each list is [nq_total][k]; positions are global int32
 * (the exchange format: 8 bytes per candidate on the wire), -1 = unfilled) into the global top-k, same
 * order rule as amdrec_flat_search: score descending (-0.0 == +0.0), equal scores -> lower position.  An entry
 * with a negative position or a NaN score is dropped wherever it stands in its list; slots that cannot be filled
 * come back as -inf / -1.  Output row i belongs to query q0 + i.  1 <= n_lists*k <= 16384,
 * list_stride_bytes % 4 == 0, q0 >= 0; nq <= 0 returns AMDREC_OK without reading a pointer. */
int amdrec_topk_merge(const float* scores, const int32_t* pos, int n_lists, int64_t list_stride_bytes,
                      int64_t q0, int64_t nq, int k, float* out_scores /*[nq][k]*/,
                      int64_t* out_pos /*[nq][k]*/, void* stream);
/* Same with SHORT lists: every shard sends only its best list_k rows per query (each list is [nq_total][list_k]), which
 * cuts a shard's exact re-scoring and the wire bytes by k / list_k.  Every list must be sorted in the search's own order
 * (score descending, equal scores -> lower position), so that a row a shard did not send is strictly behind its list's
 * last entry in that order.  A list is FULL when its last entry has a position >= 0 and a score that is not NaN (a NaN or
 * unfilled last entry: the shard had no more rows, nothing was cut).  The merged top-k is the exact global top-k iff no
 * FULL list's last entry lies strictly ahead of the merged k-th entry in the (score, position) order; *n_inexact (device
 * int32, NOT reset: accumulates) is incremented once for every query where that cannot be shown - some FULL list ends
 * ahead of the merged k-th entry, or fewer than k entries merged while some list is FULL.  A tie in score alone is not
 * counted: a last entry that IS the merged k-th, or has its score at a higher position, proves the list was cut behind
 * the boundary; the same score at a lower position is ahead and is counted.  Entries with a negative position or a NaN
 * score are dropped wherever they stand, as in amdrec_topk_merge.  The caller repeats a counted batch with list_k = k
 * (amdrec.sharded.ShardedRecommender does).  1 <= n_lists*list_k <= 16384 and 1 <= k <= 16384 (k may exceed
 * n_lists*list_k: the tail is -inf / -1); n_inexact must not be NULL. */
int amdrec_topk_merge_partial(const float* scores, const int32_t* pos, int n_lists, int list_k,
                              int64_t list_stride_bytes, int64_t q0, int64_t nq, int k,
                              float* out_scores /*[nq][k]*/, int64_t* out_pos /*[nq][k]*/,
                              int32_t* n_inexact /*device*/, void* stream);

/* ---- two-tower encoders (eval mode) ------------------------------------------------------
 * Replaces the ATen call chain of UserTower.forward / AdTower.forward
 * (two_tower_model.py:98-121, :167-184): per-column embedding lookup + concat
 * (EmbeddingLayer.forward :33-49) [+ numerical tail :113] -> (Linear, BatchNorm1d(eval), ReLU,
 * Dropout(identity)) x n -> Linear -> F.normalize(p=2, dim=1).
 * BatchNorm is folded into the preceding Linear by the host (exact in eval mode):
 *   W' = W * g / sqrt(var + eps),  b' = (b - mean) * g / sqrt(var + eps) + beta.
 * Weights are [out][ldw] row-major with K zero-padded to ldw (multiple of 32). */
#define AMDREC_MAX_LAYERS 8
#define AMDREC_MAX_TASKS 4

typedef struct {
    int32_t n_feat;              /* categorical columns (6 user / 20 ad) */
    int32_t emb_dim;             /* 16; power of two >= 4 */
    int32_t n_num;               /* numerical tail width (13 user / 0 ad) */
    int32_t n_layers;            /* Linear layers incl. the output layer */
    int32_t dims[AMDREC_MAX_LAYERS + 1]; /* dims[0] = n_feat*emb_dim + n_num, dims[l+1] = width of layer l */
    int32_t ldw[AMDREC_MAX_LAYERS];
    const float* tables;         /* all embedding tables back to back [sum(card)][emb_dim] */
    const int32_t* table_off;    /* device [n_feat]: first row of column f */
    const int32_t* cards;        /* device [n_feat]: cardinality of column f */
    const float* w[AMDREC_MAX_LAYERS];
    const float* b[AMDREC_MAX_LAYERS];
    /* != 0: amdrec_l2_normalize applied to the output rows in the same call - the rows go to an inner-product search
     * that normalises its queries (faiss.normalize_L2 on the tower's already normalised output, faiss_retrieval.py:147
     * after two_tower_model.py:121): the same two roundings as the two calls, one launch fewer. */
    int32_t renormalize;
} amdrec_tower_params;

int amdrec_tower_workspace(const amdrec_tower_params* p /*host*/, int64_t rows, size_t* bytes /*host*/);
/* cat int64 [rows][n_feat] (the reference casts .long()), num float32 [rows][n_num] or NULL,
 * out float32 [rows][ld_out] unit rows.  bad_index_flag (device int, may be NULL) is set to 1 if
 * any categorical index is outside [0, card) - torch raises IndexError there; the kernels clamp
 * so nothing is read out of bounds. */
int amdrec_tower_forward(const amdrec_tower_params* p /*host*/, const int64_t* cat, const float* num,
                         int64_t rows, float* out, int64_t ld_out, int* bad_index_flag,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- TransformerRanker.forward (eval mode) -> logits --------------------------------------
 * Replaces the ATen call chain of transformer_ranker.py:332-380.  With seq_len == 1 (:358) the
 * 8-head attention is exactly W_o(W_v x + b_v) + b_o (softmax over one key == 1), so W_q / W_k
 * are not parameters here.  pos[0] is folded into b_proj and cross weights are passed
 * transposed ([out][in]) by the host. */
typedef struct {
    /* [d_model][ldw_dm].  w_v may be NULL: then w_o / b_o hold the pre-multiplied W_o*W_v and
     * W_o*b_v + b_o (exact algebra at seq_len 1; only the fp32 rounding order differs) and the
     * attention block is ONE GEMM. */
    const float *w_v, *b_v, *w_o, *b_o;
    const float *ln1_g, *ln1_b;
    const float *w_1, *b_1;               /* [d_ff][ldw_dm] */
    const float *w_2, *b_2;               /* [d_model][ldw_ff] */
    const float *ln2_g, *ln2_b;
    int32_t ldw_dm, ldw_ff;
    /* Optional host-split planes of w_o / w_1 / w_2 for the error-compensated bf16-MFMA GEMM ("x6", used for passes of
     * more than 8192 rows; NULL -> fp32 MFMA).  Layout [out][ldw/16][3][16] bf16: for every 16-column group the planes
     * h, m, l of the exact 3-way truncation split w = h + m + l (h = w with the low 16 bits cleared, m = (w - h)
     * likewise, l = w - h - m; each plane stored as the high 16 bits of that fp32 value).  Same result contract as the
     * fp32 path: error at the level of an fp32 fma chain. */
    const uint16_t *w_o_x6, *w_1_x6, *w_2_x6;
} amdrec_encoder_layer;

/* Weights of the fp16x3 "row-owner" engine (csrc/x3_common.hpp; optional: stream == NULL -> engine off).  The engine
 * runs everything after the feature projection - the encoder layers (transformer_ranker.py:136-155 with the seq-1
 * attention :59-88), the cross layers (:199-202) and the heads (:375-378) - in ONE kernel with the activations in
 * registers; every fp32 operand is split into two fp16 planes (after an exact power-of-two scaling) and a product is
 * three fp16 MFMAs accumulated in fp32: fp32 in, fp32 out, error at the level of an fp32 fma chain.
 * `stream` = all weight matrices as 1 KB MFMA fragment sets in consumption order (the packing, incl. the k permutation
 * inside a 16-wide k-step, is defined by amdrec/weights.py pack_x3_stream and mirrored by csrc/rowowner*.hpp); `sw_*` = the
 * power-of-two scale of each packed matrix; `hn*` / `hb*` = 16 * max_j ||w_j||_2 and max_j |b_j| of the first matrix of
 * each two-stage block (FFN per layer, heads): the kernel bounds a row's hidden activations by hn * max|x| + hb to scale them.
 * Requires d_model == 256, d_ff % 32 == 0, head_h1 % 32 == 0, head_h2 == 64 and the pre-multiplied attention
 * (w_v == NULL); used for passes of at least `min_rows` rows (0 = default 8193). */
typedef struct {
    const void* stream;
    int64_t chunks;              /* stream length in 16 KB chunks */
    int64_t min_rows;
    const float* params;         /* every bias / LayerNorm weight / head vector of the chain as one device blob (layout:
                                  * csrc/ranker_x3.hip x3_param_floats; amdrec/weights.py pack_x3_params), copied into LDS
                                  * once per workgroup */
    int64_t n_params;            /* floats, padded to a multiple of 1024; must fit 44 KB of LDS */
    int64_t variant;             /* 32: rowowner.hpp (32 rows per wave, one wave per SIMD); 16: rowowner16.hpp (16 rows per
                                  * wave, two waves per SIMD); the stream is packed for exactly one of them */
    float sw_ov[AMDREC_MAX_LAYERS], sw_1[AMDREC_MAX_LAYERS], sw_2[AMDREC_MAX_LAYERS];
    float hn[AMDREC_MAX_LAYERS], hb[AMDREC_MAX_LAYERS];
    float sw_cross[AMDREC_MAX_LAYERS];
    float sw_h1, sw_h2, hn_head, hb_head;
    /* Optional second packing of the SAME fragment sets for the column-split kernel (csrc/rowowner16c.hpp; variant 16
     * only): a workgroup of four waves owns 16 rows and the waves split each layer's output features, so that one
     * request's 500 candidates (inference.py:241-250) spread over 32 CUs instead of 8 - results bit-identical to the
     * 16-row kernel.  Every 16 KB chunk holds one group of four fragment sets per wave (amdrec/weights.py x3c_stream_*).
     * Used for passes of at most cs_max_rows rows (0 = default 4096, < 0 = never); NULL -> off. */
    const void* stream_cs;
    int64_t chunks_cs;
    int64_t cs_max_rows;
    /* != 0 (ABI v12): layer 1's attention block is folded into the feature projection.  At seq_len 1 everything of
     * encoder layer 1 before its first LayerNorm is linear in the projection output x0:  z = x0 + W_ov x0 + b_ov =
     * W_p' f + b_p'  with  W_p' = (I + W_ov) W_p,  b_p' = (I + W_ov) b_p + b_ov  (formed on the host in float64).  Then
     * w_proj / w_proj_user / w_proj_ad / b_proj (and so ad_proj_cache) hold the folded projection, the chain starts with a
     * LayerNorm-only phase (LN1 of layer 1: no weights, no stream chunks), layer 1's W_ov fragments are in neither stream
     * and its b_ov is not in the parameter blob.  Only this engine runs such parameters: requires n_layers >= 1 and
     * min_rows == 1 (every pass takes the engine); layers[0] keeps the unfolded W_ov / b_ov (amdrec_ranker_x3_prefix). */
    int64_t fold_attn1;
    /* Optional (needs fold_attn1 and variant 16): stage 1 of layer 1's FFN served from a per-ad cache.  After the
     * fold the chain starts with x1 = LN1(z), z = ad_proj_cache[ad] + U[user], and W_1 x1 + b_1 is linear in z once the
     * row's deviation is known:  W_1 x1 + b_1 = rstd * W_1c z + c,  W_1c = W_1 diag(gamma1) (I - 11^T/256),  c = W_1 beta1
     * + b_1,  rstd = 1/sqrt(var(z) + eps)  (the centering matrix is folded into W_1c: no mean term).  W_1c z splits into
     * P[ad] = W_1c a_ad (ad_hidden_cache, built by amdrec_ranker_project_ads_hidden) and Q[user] = W_1c u_user, which the
     * user-projection launch writes next to U (rows [U | Q] from the stacked w_user_uq / b_user_uq).  The kernel then forms
     * the hidden tile as relu((P + Q) * rstd + c) from two row loads instead of 256 x 1024 weight elements.
     *   stream_hc / chunks_hc : the 16-row kernel's stream without layer 1's stage-1 fragment sets
     *   params_hc             : the parameter blob (n_params floats) with c in the place of layer 1's b_1
     *   w_user_uq / b_user_uq : [d_model + d_ff][ldw_proj_user] = [w_proj_user ; W_1c w_proj_user], [b_proj ; W_1c b_proj]
     *   w_hidden_ad           : [d_ff][ldw_proj_ad] = W_1c w_proj_ad    (all composed on the host in float64)
     * Used only by passes that take the 128-row kernel (> 16384 rows) with both caches set; NULL -> off. */
    const void* stream_hc;
    int64_t chunks_hc;
    const float* params_hc;
    const float* w_user_uq;
    const float* b_user_uq;
    const float* w_hidden_ad;
    /* Optional (variant 16, n_tasks >= 2): the streams of CTR-first ranking (amdrec_ranker_forward_ctr_first /
     * amdrec_ranker_winner_heads).  The SAME fragment sets, from the same split, under the same scales and hidden bounds (sw_h1,
     * sw_h2, hn_head, hb_head stay the values over the STACKED heads), cut by task:
     *   stream_ctr / stream_ctr_cs / stream_ctr_hc : `stream` / `stream_cs` / `stream_hc` up to its first heads fragment set,
     *                                                then the heads of task 0 alone
     *   stream_win / stream_win_cs                  : the heads of tasks 1 .. n_tasks - 1 alone, in the 16-row / column-split order
     * A stream that is NULL makes amdrec_ranker_ctr_first_supported answer 0 for the calls that would read it. */
    const void* stream_ctr;
    int64_t chunks_ctr;
    const void* stream_ctr_cs;
    int64_t chunks_ctr_cs;
    const void* stream_ctr_hc;
    int64_t chunks_ctr_hc;
    const void* stream_win;
    int64_t chunks_win;
    const void* stream_win_cs;
    int64_t chunks_win_cs;
    /* Products per MAC (added to ABI v14 without a version step: a new field at the struct's end, 0 in zero-initialised
     * parameters).  0 or 3: the fp16x3 arithmetic above.  1: the single-product engine - a product is ah*bh alone, ONE fp16
     * MFMA per MAC on the high planes of the SAME streams, scales, bounds and parameter blobs (nothing else is packed for it;
     * the low fragment sets travel with the chunks and are never read).  Opt-in reduced precision: operands carry 11
     * significant bits, logits come out with a relative error near 1e-4 of the row maximum instead of fp32's 1e-7.  Needs
     * variant 16; every pass runs the 64-row (<= 16384 rows) or the 128-row shape of the 16-row kernel - never the
     * column-split or the 32-row kernel - with the fold, the hidden cache and the CTR-first streams as under 3.  Any other
     * value makes the parameters ineligible for the engine. */
    int64_t products;
} amdrec_x3_weights;

typedef struct {
    int32_t n_user_feat, n_ad_feat, emb_dim, n_num;
    int32_t d_model, d_ff, n_layers, n_cross, n_tasks, head_h1, head_h2;
    float ln_eps;
    int32_t ldw_proj, ldw_cross, ldw_head1, ldw_head2;
    const float* tables;            /* user tables then ad tables, [sum(card)][emb_dim] */
    const int32_t* table_off;       /* device [n_user_feat + n_ad_feat] */
    const int32_t* cards;           /* device [n_user_feat + n_ad_feat] */
    const float* w_proj;            /* [d_model][ldw_proj], columns = [user emb | ad emb | numerical] */
    const float* b_proj;            /* bias + positional_encoding[0,0,:] */
    /* Optional split of w_proj for the broadcast form (user_rowdiv > 1): the [user emb | numerical] columns
     * and the [ad emb] columns as two matrices.  When both are set the user part is computed once per USER
     * row and added to each of its candidates' ad part (transformer_ranker.py:355 is linear in its input). */
    const float* w_proj_user;       /* [d_model][ldw_proj_user] or NULL */
    const float* w_proj_ad;         /* [d_model][ldw_proj_ad]   or NULL */
    int32_t ldw_proj_user, ldw_proj_ad;
    amdrec_encoder_layer layers[AMDREC_MAX_LAYERS];
    const float* cross_wt[AMDREC_MAX_LAYERS];  /* cross_weights[i]^T : [out][ldw_cross] */
    const float* cross_b[AMDREC_MAX_LAYERS];
    const float* head_w1;           /* first Linear of all heads stacked: [n_tasks*head_h1][ldw_head1] */
    const float* head_b1;
    const float* head_w2[AMDREC_MAX_TASKS];   /* [head_h2][ldw_head2] */
    const float* head_b2[AMDREC_MAX_TASKS];
    const float* head_w3[AMDREC_MAX_TASKS];   /* [head_h2] */
    const float* head_b3[AMDREC_MAX_TASKS];   /* [1] */
    /* Optional candidate-side cache for the broadcast form: ad_proj_cache[a] = w_proj_ad . emb(ad_cat[a]) for every
     * row of the resident ad-feature table (amdrec_ranker_project_ads; like the ad-tower embeddings it depends on
     * the ad and the weights only, so it is computed once per index build).  When set (with w_proj_user/w_proj_ad)
     * the ad half of the projection GEMM becomes a row gather: x0[r] = ad_proj_cache[ad row of r] + U[user of r],
     * the same two addends in the same order as the uncached path (bit-identical). */
    const float* ad_proj_cache;     /* [n_ad_rows][ld_ad_proj_cache] or NULL */
    int64_t ld_ad_proj_cache;
    /* Optional second candidate-side cache (see amdrec_x3_weights.stream_hc): ad_hidden_cache[a] = w_hidden_ad .
     * emb(ad_cat[a]), d_ff floats per row of the SAME table as ad_proj_cache.  The per-call user half Q lives in the
     * workspace next to U (amdrec_ranker_workspace accounts for it while this pointer is set). */
    const float* ad_hidden_cache;   /* [n_ad_rows][ld_ad_hidden_cache] or NULL */
    int64_t ld_ad_hidden_cache;
    /* Optional x6 planes (see amdrec_encoder_layer) of cross_wt[i] and head_w1. */
    const uint16_t* cross_wt_x6[AMDREC_MAX_LAYERS];
    const uint16_t* head_w1_x6;
    amdrec_x3_weights x3;
} amdrec_ranker_params;

int amdrec_ranker_workspace(const amdrec_ranker_params* p /*host*/, int64_t rows, size_t* bytes /*host*/);
/* Row r of the batch uses user_cat/numerical row r / user_rowdiv (user_rowdiv = 1: one feature
 * row per batch row as in forward(); = stage1_k: one user broadcast over its candidates, replacing
 * Tensor.repeat at inference.py:241-242) and ad_cat row (ad_rowmap ? ad_rowmap[r] : r)
 * (ad_rowmap = candidate ids into a resident ad-feature table: the lookup the reference stubs
 * out at inference.py:244-248).  out_logits[t * ld_logits + r], t = ctr, engagement, revenue.
 * n_user_rows / n_ad_rows = rows of user_cat / ad_cat (for index validation only).
 * An ad_rowmap entry outside [0, n_ad_rows) never faults: every gather clamps it into the table.  A NEGATIVE entry means
 * "no candidate" (an unfilled slot of a search result): its logits are those of ad row 0 - unspecified, finite for finite
 * weights and features - every other row's logits are what they are with any valid row in its place, bit for bit, and
 * amdrec_select_topk(cand_pos = ad_rowmap) keeps such a slot out of the result.  bad_index_flag (device int, may be NULL)
 * is set to 1 when a user_cat / ad_cat index is outside its table or an ad_rowmap entry is >= n_ad_rows (the reference's
 * ad_table[cand] raises there); negative ad_rowmap entries do not set it. */
int amdrec_ranker_forward(const amdrec_ranker_params* p /*host*/, const int64_t* user_cat,
                          const float* numerical, int64_t user_rowdiv, const int64_t* ad_cat,
                          const int64_t* ad_rowmap, int64_t rows, float* out_logits, int64_t ld_logits,
                          int* bad_index_flag, int64_t n_user_rows, int64_t n_ad_rows, void* workspace,
                          size_t workspace_bytes, void* stream);

/* CTR-first ranking (added to ABI v14 without a version step: new exports, new amdrec_x3_weights fields at the struct's end).
 * The callers of the reference rank a user's candidates by the CTR logit alone and report the other tasks for the winners
 * only (inference.py:258-288, faiss_retrieval.py:355-369).  Pass 1 runs the projection, the trunk and the head of task 0 on
 * every candidate and keeps each row's trunk state; the selection runs on that one logit row; pass 2 runs the other heads on
 * the winners' stored rows.  Every number either pass produces is, bit for bit, the one amdrec_ranker_forward +
 * amdrec_select_topk produce: a wave owns its rows, and the same fragment sets meet the same fp32 state in the same order
 * under the same scales.
 *
 * amdrec_ranker_forward_ctr_first: the arguments of amdrec_ranker_forward, plus trunk_out [rows][ld_trunk] (ld_trunk >= 256,
 * % 4 == 0, 16-byte aligned): row r's 256 floats are the state the heads receive.  out_logits[r] = the logit of task 0 (one
 * row; ld_logits >= rows is still required).  Workspace: amdrec_ranker_ctr_first_workspace.  An error (AMDREC_EINVAL) where
 * amdrec_ranker_ctr_first_supported(p, rows) is 0: there is no fall-back inside the entry.
 * amdrec_ranker_ctr_first_supported: non-zero when every pass of a `rows`-row call, and a winner pass of `rows` rows, would
 * run a 16-row kernel of the fp16x3 engine (x3.variant 16, every pass at least x3.min_rows rows) with the streams it reads
 * packed, n_tasks >= 2; p's cache pointers count (they select the hidden-cache program).  Otherwise the caller runs
 * amdrec_ranker_forward.
 * amdrec_ranker_winner_heads: slots [n_users][top_k] = amdrec_select_topk's out_slots over k_c candidates per user; winner
 * row i = u * top_k + j reads trunk[u * k_c + slots[i]] (clamped into [0, n_trunk_rows); n_trunk_rows >= n_users * k_c) and
 * out_scores[t][u][j] = sigmoid(logit of task t), t = 1 .. n_tasks - 1, by the expression amdrec_select_topk uses; 0.0 where
 * the slot is negative (no winner: the tail of a short list, or top_k > k_c).  Plane 0 of out_scores is not written.  Two
 * launches: the heads-only program on the kernel its row count selects, and the sigmoid.  n_users * top_k < 2^31.
 * amdrec_ranker_ctr_first_workspace: the bytes that serve amdrec_ranker_forward_ctr_first on `rows` rows and
 * amdrec_ranker_winner_heads on n_winner_rows = n_users * top_k rows: the larger of the two needs - amdrec_ranker_workspace's
 * for `rows` (0 for rows == 0) and (n_tasks - 1) * n_winner_rows floats, rounded up to 256 bytes. */
int amdrec_ranker_forward_ctr_first(const amdrec_ranker_params* p /*host*/, const int64_t* user_cat,
                                    const float* numerical, int64_t user_rowdiv, const int64_t* ad_cat,
                                    const int64_t* ad_rowmap, int64_t rows, float* out_logits /*[rows]*/,
                                    int64_t ld_logits, int* bad_index_flag, int64_t n_user_rows, int64_t n_ad_rows,
                                    float* trunk_out /*[rows][ld_trunk]*/, int64_t ld_trunk, void* workspace,
                                    size_t workspace_bytes, void* stream);
int amdrec_ranker_ctr_first_supported(const amdrec_ranker_params* p /*host*/, int64_t rows);
int amdrec_ranker_winner_heads(const amdrec_ranker_params* p /*host*/, const float* trunk /*[n_trunk_rows][ld_trunk]*/,
                               int64_t ld_trunk, int64_t n_trunk_rows, const int32_t* slots /*[n_users][top_k]*/,
                               int64_t n_users, int k_c, int top_k, float* out_scores /*[n_tasks][n_users][top_k]*/,
                               void* workspace, size_t workspace_bytes, void* stream);
int amdrec_ranker_ctr_first_workspace(const amdrec_ranker_params* p /*host*/, int64_t rows, int64_t n_winner_rows,
                                      size_t* bytes /*host*/);

/* Test / debugging entry of the fp16x3 engine: run the first n_phases phases of the chain (phase order: per encoder
 * layer {attention + LN1, FFN + LN2}, then the cross layers, then the heads; n_phases < 0 = all) on dense projected
 * rows X [rows][ldx] and return the rows after the last executed phase in x_out [rows][ld_out] (may be NULL) and, when
 * the heads ran, the logits.  workspace: >= ceil(rows / 128) * 128 * 1024 bytes.  Lets the parity tests localise an
 * error to one phase; amdrec_ranker_forward uses the same kernel for whole passes.  X is always the UNFOLDED projection
 * x0: with x3.fold_attn1 the entry first forms z = x0 + W_ov x0 + b_ov (fp32 fma chains, from layers[0].w_o / b_o) into
 * the workspace and runs the folded chain on it, whose first phase (LN1 alone) then stands for "attention + LN1". */
int amdrec_ranker_x3_prefix(const amdrec_ranker_params* p /*host*/, const float* X, int64_t ldx, int64_t rows,
                            int n_phases, float* x_out, int64_t ld_out, float* logits, int64_t ld_logits,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Fills the candidate-side cache described at amdrec_ranker_params.ad_proj_cache: out[a] = w_proj_ad . emb(ad_cat[a])
 * (no bias; the user half carries it), a = 0..n_ads-1.  workspace: >= 4*d_model + 256 bytes. */
int amdrec_ranker_project_ads(const amdrec_ranker_params* p /*host*/, const int64_t* ad_cat, int64_t n_ads,
                              float* out /*[n_ads][ld_out]*/, int64_t ld_out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Fills amdrec_ranker_params.ad_hidden_cache: out[a] = x3.w_hidden_ad . emb(ad_cat[a]) (d_ff floats per ad, no bias),
 * with the tile GEMM of amdrec_ranker_project_ads.  workspace: >= 4*d_ff + 256 bytes. */
int amdrec_ranker_project_ads_hidden(const amdrec_ranker_params* p /*host*/, const int64_t* ad_cat, int64_t n_ads,
                                     float* out /*[n_ads][ld_out]*/, int64_t ld_out, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* faiss.normalize_L2 (faiss_retrieval.py:115, :147): every row scaled by 1/||row||_2, rows of
 * zero norm left as they are.  out may alias in.  dim % 4 == 0. */
int amdrec_l2_normalize(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows,
                        int dim, void* stream);

/* FAISSIndex.search's id remap (faiss_retrieval.py:159-160, a Python list comprehension):
 * out[i] = id_map[pos[i]]; pos == -1 reads id_map[n_map-1] exactly like Python's id_map[-1]. */
int amdrec_remap_ids(const int64_t* pos, const int64_t* id_map, int64_t n_map, int64_t* out,
                     int64_t n, void* stream);

/* Per-request exclusion lists (added to ABI v14 without a version step: a new export, every other entry as it was).  The
 * search ran unfiltered for kc candidates per query; this drops, per query, every candidate whose key is in the query's
 * exclusion list exclude[q][0 .. n_exclude) (ad ids or positions, whatever `keys` holds; negative entries are padding and
 * match nothing; duplicates allowed) and writes the first k survivors in their order: out_keys / out_scores / out_carry
 * [nq][k].  `carry` (may be NULL, then out_carry is NULL too) is a second int64 block that travels with the keys: the corpus
 * positions when the keys are remapped ids; out_keys may be NULL when it is given.  A candidate that is already unfilled
 * (carry < 0, or key < 0 without carry) is never matched and keeps its place.  Slots past the last survivor get fill_key /
 * fill_score / fill_carry (the index type's unfilled convention: -1, -inf or +inf, -1).  One launch, one workgroup per
 * query, no workspace.  1 <= k <= kc <= AMDREC_MAX_K, 1 <= n_exclude < AMDREC_MAX_K, ld_exclude >= n_exclude; outputs must
 * not alias inputs. */
int amdrec_exclude_compact(const int64_t* keys /*[nq][kc]*/, const float* scores /*[nq][kc]*/,
                           const int64_t* carry /*[nq][kc] or NULL*/, int64_t nq, int kc,
                           const int64_t* exclude /*[nq][ld_exclude]*/, int n_exclude, int64_t ld_exclude, int k,
                           int64_t fill_key, float fill_score, int64_t fill_carry, int64_t* out_keys /*[nq][k]*/,
                           float* out_scores /*[nq][k]*/, int64_t* out_carry /*[nq][k] or NULL*/, void* stream);

/* Per-request must-consider lists (added to ABI v14 without a version step: a new export, every other entry as it was).  The
 * search ran for k entries per query: pos / scores [nq][k], ordered by score descending, ties to the lower position, unfilled
 * slots (position < 0) last.  include[q][0 .. n_include) are corpus POSITIONS the query must also consider.  An entry counts
 * when it lies in [0, n_rows), no earlier entry of the list holds it, row X[p] passes the query's masks (tags / require_all /
 * require_any, all three or all NULL: (tags[p] & all) == all and (any == 0 or (tags[p] & any) != 0)), its id (ids[p], or p
 * where ids is NULL) is not in exclude[q][0 .. n_exclude) (NULL: no exclusion block; negative entries are padding), and its
 * score - the searches' fp32 re-score chain of <X[p], Q[q]>, plus boost_w[q] * boosts[p] as two rounded operations where
 * boosts is given - is not NaN.  Entries that count and that the result already holds change nothing: those columns stay as
 * they are.  The m others are merged in: max(0, f + m - k) of the result's f filled columns that the list does not name
 * leave, lowest rank first, and the output is the rest and the m in the same order, unfilled slots (-1, -inf) last.
 * out_injected (may be NULL) is 1 exactly in the slots of the m.  One launch, one workgroup per query, no workspace.
 * 1 <= n_include <= min(k, AMDREC_MAX_INCLUDE), k <= AMDREC_MAX_K, d % 4 == 0, d <= 2048, n_rows < 2^32, X 16-byte aligned
 * with ldx % 4 == 0; outputs must not alias inputs. */
int amdrec_include_merge(const int64_t* pos /*[nq][k]*/, const float* scores /*[nq][k]*/, int64_t nq, int k,
                         const int64_t* include /*[nq][ld_include]*/, int n_include, int64_t ld_include,
                         const float* X /*[n_rows][ldx]*/, int64_t ldx, int64_t n_rows, int d, const float* Q /*[nq][ldq]*/,
                         int64_t ldq, const int64_t* tags /*[n_rows] or NULL*/, const int64_t* require_all /*[nq] or NULL*/,
                         const int64_t* require_any /*[nq] or NULL*/, const int64_t* exclude /*[nq][ld_exclude] or NULL*/,
                         int n_exclude, int64_t ld_exclude, const int64_t* ids /*[n_rows] or NULL*/,
                         const float* boosts /*[n_rows] or NULL*/, const float* boost_w /*[nq] or NULL*/,
                         int64_t* out_pos /*[nq][k]*/, float* out_scores /*[nq][k]*/, uint8_t* out_injected /*[nq][k] or NULL*/,
                         void* stream);

/* Live corpus: removing rows without recomputing any (two more exports added to ABI v14, every other entry as it was).  A
 * removal is an order-preserving compaction of every per-row array the caller keeps: amdrec_remove_plan says which rows stay,
 * amdrec_rows_gather moves one array.
 *
 * amdrec_remove_plan: row i of n has the key ids[i] (ids == NULL: the key is i itself) and stays unless that key is in
 * `remove` (n_remove entries, ascending, unique, >= 0; a negative key matches nothing).  kept[0 .. *n_kept) = the old
 * positions of the rows that stay, ascending; the rest of kept[n] is left as it was; *n_kept is a DEVICE scalar.  Three plain
 * launches (flag + count per 1024 rows, one workgroup scanning the counts, write); no workgroup waits for another.
 * 0 <= n <= 2^31 - 1.  n == 0 writes *n_kept = 0 (or nothing, if n_kept is NULL) and needs no other pointer; n_remove == 0
 * (remove may be NULL) makes kept the identity.  Workspace: amdrec_remove_plan_workspace(n), 256-byte aligned. */
int amdrec_remove_plan_workspace(int64_t n, size_t* bytes /*host*/);
int amdrec_remove_plan(const int64_t* ids /*[n] or NULL*/, int64_t n, const int64_t* remove /*[n_remove]*/,
                       int64_t n_remove, int64_t* kept /*[n]*/, int64_t* n_kept /*device scalar*/, void* workspace,
                       size_t workspace_bytes, void* stream);

/* dst[j] = src[pos[j]] for j < n_out, byte for byte: rows of row_bytes >= 1 bytes, row pitches ld_*_bytes >= row_bytes (the
 * padding between rows is neither read nor written).  Out of place: the byte ranges of src (n_src rows) and dst (n_out rows)
 * must not overlap.  A position outside [0, n_src) is never read: that row of dst is zero-filled.  Accesses are 16 bytes wide
 * when src, dst, both pitches and row_bytes are all multiples of 16, else the widest of 8 / 4 / 1 that divides them all;
 * byte offsets are 64-bit; one launch whose capped grid strides over the rows.  n_out == 0 returns at once. */
int amdrec_rows_gather(const void* src, int64_t ld_src_bytes, int64_t n_src, const int64_t* pos /*[n_out]*/,
                       int64_t n_out, int64_t row_bytes, void* dst, int64_t ld_dst_bytes, void* stream);

/* Optional per-launch timing: HIP events recorded on the launch stream around every GEMM-shaped
 * kernel launch, accumulated per kernel tag ("<epilogue>_<BP>x<BQ>", DESIGN.md maps tags to
 * symbol names).  flops / bytes are the ALGORITHMIC 2*M*N*K and operand+result bytes of the
 * launches.  amdrec_profile_report synchronises with the recorded events. */
typedef struct {
    char name[64];
    int64_t launches;
    double total_ms, flops, bytes;
} amdrec_profile_entry;
int amdrec_profile_enable(int on);   /* also clears the counters */
/* Time only the launches whose tag starts with tag_prefix (NULL or "" = all): an event pair costs the stream ~10 us of
 * idle GPU per launch, so a benchmark times every kernel in a pre-pass and only its dominant one in the timed region. */
int amdrec_profile_only(const char* tag_prefix);
int amdrec_profile_report(amdrec_profile_entry* out /*host*/, int max_entries, int* n /*host*/);

/* Request-side numerical prep (inference.py:186-195): out[r][c] = (log1p(|x[r][c]|) - mean[c]) / scale[c],
 * float32 (the reference produces float64 there and crashes its own float32 model). out may alias x. */
int amdrec_prep_numerical(const float* x, const float* mean /*[cols]*/, const float* scale /*[cols]*/,
                          float* out, int64_t rows, int cols, void* stream);

/* Stage-2 selection (inference.py:258-263: sigmoid -> np.argsort(ctr)[::-1][:top_k]): per user
 * the top_k of its k_c candidates by the LOGIT of task `rank_task` (sigmoid is monotone), order
 * (logit desc, candidate slot asc).  out_ids[u][i] = cand_ids[u][slot], out_scores[t][u][i] =
 * sigmoid(logits[t][u*k_c + slot]), out_slots (optional) = the winning slots.  NaN logits rank after every other logit.
 * cand_pos (device, may be NULL = every slot is a candidate): the candidates' stage-1 corpus positions.  A slot with
 * cand_pos < 0 was left unfilled by the search and is NOT a candidate, whatever its logit and its cand_ids entry (an id is
 * the caller's to choose; validity is decided by position): it ranks after every real candidate, NaN logits included.
 * Where a user has fewer than top_k real candidates (unfilled slots, or top_k > k_c) the tail reads out_ids = -1,
 * out_scores = 0.0 for every task, out_slots = -1. */
int amdrec_select_topk(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks,
                       int rank_task, const int64_t* cand_ids /*[n_users][k_c]*/,
                       const int64_t* cand_pos /*[n_users][k_c] or NULL*/, int64_t n_users,
                       int k_c, int top_k, int64_t* out_ids /*[n_users][top_k]*/,
                       float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots, void* stream);

/* Per-group caps ("at most c ads of one advertiser"; two more exports added to ABI v14, every other entry as it was).  The
 * rule is greedy in rank order: an entry is accepted while fewer than max_per_group accepted entries share its group - which
 * equals "keep an entry iff fewer than max_per_group BETTER-RANKED entries have its group, then cut", so every entry is
 * decided from its own group's prefix alone.  A group key is an int64 per corpus row, group_of[n_group_rows], read at an
 * entry's corpus position; a negative key means ungrouped (never capped), and a position outside [0, n_group_rows) is never
 * read and counts as ungrouped.  1 <= max_per_group <= AMDREC_MAX_K.
 *
 * amdrec_select_topk_capped: amdrec_select_topk under the cap - its arguments in the same order, then the groups.  The
 * candidates are amdrec_select_topk's (a slot with cand_pos < 0 is none; cand_pos is REQUIRED here) and are visited in its
 * order (logit desc, slot asc, NaN logits after every other logit); a candidate's group is group_of[cand_pos].  A candidate
 * of group g >= 0 is accepted iff fewer than max_per_group earlier candidates in that order have group g (NaN-logit
 * candidates count and are capped like any other); ungrouped candidates are always accepted.  The first top_k accepted
 * candidates are the result, in order; the tail past the last one reads out_ids = -1, out_scores = 0.0, out_slots = -1 as
 * amdrec_select_topk's short-list tail.  out_scores, out_slots and the probability expression are amdrec_select_topk's.
 * One launch, no workspace; every argument is validated before the first HIP call. */
int amdrec_select_topk_capped(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks,
                              int rank_task, const int64_t* cand_ids /*[n_users][k_c]*/,
                              const int64_t* cand_pos /*[n_users][k_c]*/, int64_t n_users,
                              int k_c, int top_k, int64_t* out_ids /*[n_users][top_k]*/,
                              float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots,
                              const int64_t* group_of /*[n_group_rows], indexed by cand_pos*/, int64_t n_group_rows,
                              int max_per_group, void* stream);

/* amdrec_group_cap_compact: the same rule on a search result.  pos / scores [nq][kc] are a search's positions and scores in
 * the index's own order; an entry is kept iff fewer than max_per_group earlier FILLED entries of its row share its
 * non-negative group group_of[pos].  An unfilled entry (pos < 0) is never counted and never dropped: it keeps its place
 * behind the filled ones.  out_pos / out_scores [nq][k] receive the first k kept entries in their order; the slots past the
 * last one get -1 / fill_score (the index type's unfilled convention: -inf, or +inf for IVFPQ).  One launch, one workgroup
 * per query, no workspace.  1 <= k <= kc <= AMDREC_MAX_K; outputs must not alias inputs. */
int amdrec_group_cap_compact(const int64_t* pos /*[nq][kc]*/, const float* scores /*[nq][kc]*/, int64_t nq, int kc,
                             const int64_t* group_of /*[n_group_rows]*/, int64_t n_group_rows, int max_per_group, int k,
                             float fill_score, int64_t* out_pos /*[nq][k]*/, float* out_scores /*[nq][k]*/, void* stream);

/* Auction ranking (one more export added to ABI v14, every other entry as it was): amdrec_select_topk ordered by expected
 * revenue, with an optional per-user reserve, the per-group cap of amdrec_select_topk_capped and generalised second prices.
 * For candidate slot i of user u (a candidate iff cand_pos >= 0; cand_pos is REQUIRED):
 *   p = the probability amdrec_select_topk reports for logits[rank_task], b = bid_of[cand_pos] (1.0 for a position >=
 *   n_bid_rows, which is never read; bids are finite and >= +0.0), e = b * p, one fp32 multiply.
 * Order: e descending, slot ascending, a NaN e (NaN logit) after every other candidate.  reserve (device [n_users], may be
 * NULL): a candidate is dropped iff !(e >= reserve[u]) - a NaN e too - and is then no candidate: it cannot win, does not
 * count towards a cap and sets nobody's price.  max_per_group > 0: the greedy cap over group_of[cand_pos] in that order on
 * the candidates that pass the reserve; 0: no cap, group_of is not looked at and may be NULL.
 * The first top_k accepted candidates win.  With next(r) = the candidate the same selection would report at rank r + 1 (for
 * the last rank the (top_k + 1)-th accepted one, if any) and floor = max(reserve[u] or 0, e of next(r), a missing or NaN one
 * counting 0): out_price = NaN where the winner's e is NaN, 0.0 where floor == 0, else min(b, floor / p) with the correctly
 * rounded fp32 division - the smallest bid that keeps the rank, never above the winner's own.  out_ecpm = e.  NaN outputs
 * are the canonical quiet NaN (0x7fc00000).  out_ids / out_scores / out_slots as amdrec_select_topk; the unfilled tail reads
 * id -1, slot -1, probability 0.0, eCPM 0.0, price 0.0.  One launch, no workspace; every argument is validated before the
 * first HIP call. */
int amdrec_select_topk_auction(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks, int rank_task,
                               const int64_t* cand_ids /*[n_users][k_c]*/, const int64_t* cand_pos /*[n_users][k_c]*/,
                               int64_t n_users, int k_c, int top_k, const float* bid_of /*[n_bid_rows], by cand_pos*/,
                               int64_t n_bid_rows, const float* reserve /*[n_users] or NULL*/,
                               const int64_t* group_of /*[n_group_rows]; NULL without a cap*/, int64_t n_group_rows,
                               int max_per_group /*0: no cap*/, int64_t* out_ids /*[n_users][top_k]*/,
                               float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots /*or NULL*/,
                               float* out_ecpm /*[n_users][top_k]*/, float* out_price /*[n_users][top_k]*/, void* stream);

/* Diversified selection (one more export added to ABI v14, every other entry as it was): amdrec_select_topk re-ordered by
 * relevance discounted by similarity to what is already chosen - a multiplicative MMR.  Per user:
 *   candidates and relevance order are amdrec_select_topk's (cand_pos is REQUIRED; logit desc, slot asc, NaN logits last);
 *   max_per_group > 0: a candidate is accepted iff fewer than max_per_group better-ranked candidates share its non-negative
 *   group group_of[cand_pos] (amdrec_select_topk_capped's acceptance); 0: every candidate is accepted, group_of may be NULL;
 *   the POOL is the first `pool` accepted candidates.  Member i has rel_i = the probability amdrec_select_topk reports for
 *   logits[rank_task], and m_i = 0.  For rank r = 0 .. top_k - 1 the untaken member with the largest
 *   v_i = rel_i * fmaf(-lam, m_i, 1.0f) (fp32) wins; equal values go to the member earlier in the relevance order, a NaN value
 *   ranks after every other (among NaNs the earlier member).  After winner w, every remaining i: m_i = fminf(1, fmaxf(m_i,
 *   s_iw)), s_iw = the fp32 inner product of rows cand_pos[i] and cand_pos[w] of `rows` (accumulation order unspecified; a NaN
 *   s_iw leaves m_i as it was; a negative one does not discount).  A position >= n_rows is never read: similarity 0.
 * Winners go out in pick order as amdrec_select_topk writes them; out_values[u][r] = the winning v.  The tail past the last
 * winner (a pool shorter than top_k) reads id -1, slot -1, probabilities 0.0, value 0.0.  With lam == 0 the result equals
 * amdrec_select_topk's (amdrec_select_topk_capped's under a cap) bit for bit.
 * 1 <= top_k <= pool <= 128, 1 <= k_c <= AMDREC_MAX_K, 1 <= dim <= ld_rows, pool * dim <= 32768 (the pool's rows are staged
 * in one workgroup's LDS), lam finite in [0, 1].  One launch, one workgroup per user, no workspace; every argument is
 * validated before the first HIP call; n_users <= 0 returns OK without looking at a pointer. */
int amdrec_select_topk_diverse(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks, int rank_task,
                               const int64_t* cand_ids /*[n_users][k_c]*/, const int64_t* cand_pos /*[n_users][k_c]*/,
                               int64_t n_users, int k_c, int top_k, const float* rows /*[n_rows][ld_rows]*/, int64_t n_rows,
                               int64_t ld_rows, int dim, float lam, int pool,
                               const int64_t* group_of /*[n_group_rows]; NULL without a cap*/, int64_t n_group_rows,
                               int max_per_group /*0: no cap*/, int64_t* out_ids /*[n_users][top_k]*/,
                               float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots /*or NULL*/,
                               float* out_values /*[n_users][top_k]*/, void* stream);

/* Value ranking (two more exports added to ABI v14, every other entry as it was): the selections above ordered by a weighted
 * blend of EVERY task's probability instead of the ranking task alone.  weights (device float32 [n_users][n_tasks]) are per
 * user; n_tasks <= AMDREC_MAX_TASKS.  For candidate slot i of user u (a candidate iff cand_pos >= 0; cand_pos is REQUIRED):
 *   p_t = the probability amdrec_select_topk reports for logits[t].  The tasks are visited in order t = 0 .. n_tasks - 1; a
 *   term whose weight is 0 (either sign) is skipped and its logit has no influence, NaN included; y_t = p_t, in the auction
 *   variant y_r = e = b * p_r for r = rank_task, b = bid_of[cand_pos] (1.0 for a position >= n_bid_rows, which is never
 *   read); x_t = w_t * y_t; v = the first unskipped x_t, then v = v + x_t.  Every product, sum, difference and quotient here
 *   is one rounded fp32 operation, never contracted.  All weights zero: v = +0.0.
 * Order: v descending (-0.0 and +0.0 tie), slot ascending, a NaN v after every other candidate in slot order; a slot that is
 * no candidate never wins.  max_per_group > 0: the greedy cap of amdrec_select_topk_capped in that order; 0: no cap, group_of
 * is not looked at and may be NULL.  The first top_k accepted candidates win; out_ids / out_scores / out_slots as
 * amdrec_select_topk, out_values[u][rank] = v, formed from the probabilities that out_scores reports: the blend of out_scores
 * (and out_ecpm) equals it bit for bit.  A NaN output is the canonical quiet NaN; the unfilled tail reads id -1, slot -1,
 * probabilities 0.0, value 0.0.  With weights 1.0 * onehot(r) the order is by p_r: amdrec_select_topk's for a user whose p_r
 * are pairwise distinct - NOT the logit order in general, because saturated sigmoids tie and resolve by slot.
 *
 * amdrec_select_topk_value_auction: reserve (device [n_users], may be NULL): a candidate is dropped iff !(v >= reserve[u]),
 * as in amdrec_select_topk_auction.  floor = max(reserve[u] or 0, v of the candidate the same selection reports at the next
 * rank - for the last rank the (top_k + 1)-th accepted one; a missing or NaN one counts 0).  q = the chain with term r left
 * out (a chain of its own, +0.0 when nothing is left), d = w_r * p_r, num = floor - q.  out_price = NaN where the winner's v
 * is NaN, 0.0 where !(num > 0), 0.0 where !(d > 0) (the bid does not hold the rank), else min(b, num / d).  out_ecpm = e.
 * The tail reads eCPM 0.0 and price 0.0.  With weights 1.0 * onehot(rank_task) ids, slots, eCPMs and prices are
 * amdrec_select_topk_auction's bit for bit.
 * One launch, no workspace; every argument is validated before the first HIP call; n_users <= 0 returns OK without looking
 * at a pointer. */
int amdrec_select_topk_value(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks,
                             const int64_t* cand_ids /*[n_users][k_c]*/, const int64_t* cand_pos /*[n_users][k_c]*/,
                             int64_t n_users, int k_c, int top_k, const float* weights /*[n_users][n_tasks]*/,
                             const int64_t* group_of /*[n_group_rows]; NULL without a cap*/, int64_t n_group_rows,
                             int max_per_group /*0: no cap*/, int64_t* out_ids /*[n_users][top_k]*/,
                             float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots /*or NULL*/,
                             float* out_values /*[n_users][top_k]*/, void* stream);
int amdrec_select_topk_value_auction(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks, int rank_task,
                                     const int64_t* cand_ids /*[n_users][k_c]*/, const int64_t* cand_pos /*[n_users][k_c]*/,
                                     int64_t n_users, int k_c, int top_k, const float* weights /*[n_users][n_tasks]*/,
                                     const float* bid_of /*[n_bid_rows], by cand_pos*/, int64_t n_bid_rows,
                                     const float* reserve /*[n_users] or NULL*/,
                                     const int64_t* group_of /*[n_group_rows]; NULL without a cap*/, int64_t n_group_rows,
                                     int max_per_group /*0: no cap*/, int64_t* out_ids /*[n_users][top_k]*/,
                                     float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots /*or NULL*/,
                                     float* out_values /*[n_users][top_k]*/, float* out_ecpm /*[n_users][top_k]*/,
                                     float* out_price /*[n_users][top_k]*/, void* stream);

/* Exploration (one more export added to ABI v14, every other entry as it was): amdrec_select_topk_capped with a sampled
 * order behind a greedy prefix, and the probability of every pick.  Its arguments in the same order, then temperature
 * (device float32 [n_users]), seeds (device uint64 [n_users]), greedy (the prefix g, one value per call) and out_propensity.
 * max_per_group == 0: no cap, group_of is not looked at and may be NULL.  cand_pos is REQUIRED.  Per user u:
 *   mix64(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31 (mod 2^64);
 *   h_i = mix64(mix64(seeds[u]) ^ (uint64) cand_ids[u][i]); U_i = ((h_i >> 41) + 0.5) * 2^-23; G_i = -log(-log(U_i)) in fp64;
 *   for a finite logit z_i of rank_task: x_i = (double) z_i / (double) temperature[u], k_i = (float)(x_i + G_i).
 *   Sampled order S: +inf logits in slot order, then the finite ones by (k desc, slot asc), then -inf logits in slot order,
 *   then NaN logits in slot order.  A user with !(temperature[u] > 0) is served greedily: S = amdrec_select_topk's order.
 *   The first `greedy` winners are amdrec_select_topk_capped's (amdrec_select_topk's without a cap); the walk then goes on
 *   over S, skipping what is chosen, with the group counts carried over, until top_k winners stand or S is used up.
 *   out_propensity[u][rank] = 1.0 for a rank below `greedy`, for a greedily served user and for a winner whose logit is not
 *   finite; else exp(x_w - m) / sum_{i in R} exp(x_i - m) in fp64, rounded once to fp32 (it may round to 0.0), R = the
 *   finite-logit candidates not yet chosen whose group is not full, m = their largest x.
 * out_ids / out_scores / out_slots as amdrec_select_topk; the unfilled tail reads id -1, slot -1, probabilities 0.0,
 * propensity 0.0.  The noise is keyed on the ad id: it does not depend on the candidate order or on the batch.
 * 1 <= top_k <= 128, 0 <= greedy <= top_k, 1 <= k_c <= AMDREC_MAX_K, 0 <= max_per_group <= AMDREC_MAX_K.  One launch, one
 * workgroup per user, no workspace; every argument is validated before the first HIP call; n_users <= 0 returns OK without
 * looking at a pointer. */
int amdrec_select_topk_sampled(const float* logits /*[n_tasks][ld]*/, int64_t ld_logits, int n_tasks, int rank_task,
                               const int64_t* cand_ids /*[n_users][k_c]*/, const int64_t* cand_pos /*[n_users][k_c]*/,
                               int64_t n_users, int k_c, int top_k, int64_t* out_ids /*[n_users][top_k]*/,
                               float* out_scores /*[n_tasks][n_users][top_k]*/, int32_t* out_slots /*or NULL*/,
                               const int64_t* group_of /*[n_group_rows]; NULL without a cap*/, int64_t n_group_rows,
                               int max_per_group /*0: no cap*/, const float* temperature /*[n_users]*/,
                               const uint64_t* seeds /*[n_users]*/, int greedy, float* out_propensity /*[n_users][top_k]*/,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDREC_H */
