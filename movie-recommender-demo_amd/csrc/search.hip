// Exact inner-product top-k over a flat corpus (replaces faiss IndexFlatIP.search as called
// from FAISSIndex.search, faiss_retrieval.py:155).
//
// Algorithm ("threshold-prefiltered exact top-k"), all on device, no host sync:
//   1. sample pass : scores of every query against an evenly spaced subset of corpus tiles
//                    (fp32 MFMA GEMM, dense store)                     ~3 % of the corpus
//   2. threshold   : per query tau_q ~ the r-th largest sample score (r-th largest of 256 per-group
//                    maxima); the expected number of corpus rows with score >= tau_q is ~max(2k, k+900)
//   3. filter pass : fp32 MFMA GEMM over the whole corpus; the epilogue appends
//                    (score, row) keys with score >= tau_q to a per-query candidate list
//   4. finalize    : per query, if k <= count <= capacity the exact top-k is inside the
//                    list (every row >= tau is there) -> bitonic sort of 64-bit keys in LDS
//   5. fix-up      : queries whose count fell outside [k, capacity] (adversarial order,
//                    massive ties) are re-done by an exact streaming scan (16 slices per
//                    query, running threshold) + merge.  Blocks of healthy queries exit at once.
// The result is exact for every input; only the speed depends on the data.
// Order: score descending, equal scores -> lower row first (deterministic).
//
// Mixed-precision variant (amdrec_flat_search_mixed): passes 1-3 run on a bf16 copy of the corpus and of the
// queries with v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate, half the HBM bytes), which turns the filter from
// MFMA-bound into memory-bound; the result stays the exact fp32 one because
//   * eps_q = ||dq|| (M + D) + ||q|| D bounds |approx - exact| for every row, from the MEASURED rounding errors of the
//     query (dq) and of the corpus (D = max row error norm, M = max row norm; see eps_bound below): at worst the classical
//     (2u + u^2) |q| |x| with u = 2^-8, ~4x smaller on real data; plus the fp32 accumulation slack,
//   * finalize radix-selects a_k = the k-th largest approximate score, keeps the candidates with approx >= a_k - 2 eps
//     (anything below is beaten by k rows), RE-SCORES them in fp32 from the fp32 corpus and sorts them,
//   * and certifies: every row outside the list has approx < tau, i.e. exact < tau + eps; if the k-th re-scored
//     value is >= tau + eps nothing outside can enter the top-k.  A query that fails the certificate (or the
//     count test) goes to the same exact fp32 fix-up scan as before.
// For dims 32 / 64 / 128 / 256 the corpus pass of this variant is scan_filter_kernel (below), not a generic GEMM tile.
// Per-request eligibility masks (amdrec_flat_search*_eligible): the same searches over the rows a query may be shown.  The
// predicate is a compile-time type of every kernel (NoElig / Elig, below): the sample turns ineligible scores into -inf, so
// tau sits at the quantile that admits ~target ELIGIBLE rows; the filter tests it with the threshold; the fix-up scan, which
// also answers every query with fewer than k eligible rows, where a key is formed.
#include <type_traits>
#include "gemm_core.hpp"
#include "topk_utils.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int CAND_CAP = 8192;     // candidate keys per query (64 KB LDS sort)
constexpr long long CAND_STRIDE = 2 * CAND_CAP;   // mixed search: keys between the queries' blocks ([segments | overflow])
constexpr int SAMPLE_RANK = 64;    // r
constexpr int KMAX = 2048;
constexpr int FIX_BUF = 4096;      // fix-up scan buffer (keys)
constexpr int FIX_GRID_Q = 256;    // queries worked on at a time by the fix-up kernels
constexpr int SAMPLE_G = 256;      // rows per sample block (== BP of every search shape / divides it)

// ---- per-request eligibility (amdrec_flat_search*_eligible) ----------------------------
// Row r may be returned to query q iff (tags[r] & all[q]) == all[q] and (any[q] == 0 or (tags[r] & any[q]) != 0); one
// 64-bit tag per corpus row, two 64-bit masks per query (amdrec.h has the contract).  Every search kernel takes the
// predicate as a type: NoElig, an empty one, in the searches without masks - their kernels are the ones they were -, Elig
// in the filtered instantiations.
__device__ __forceinline__ bool tag_ok(uint64_t t, uint64_t all, uint64_t any) {
    return (t & all) == all && (any == 0ull || (t & any) != 0ull);
}
struct NoElig {
    static constexpr bool on = false, boosted = false;
    __device__ __forceinline__ bool ok(long long, int) const { return true; }
};
struct Elig {
    static constexpr bool on = true, boosted = false;
    const uint64_t* tags;    // [nrows]
    const uint64_t* all;     // [nq]
    const uint64_t* any;     // [nq]
    __device__ __forceinline__ bool ok(long long row, int q) const { return tag_ok(tags[row], all[q], any[q]); }
};

// ---- per-ad score boosts (amdrec_flat_search*_boosted) ----------------------------------
// key(q, r) = <q, x_r> + w_q * boost[r]: one float per corpus row, one weight per query (amdrec.h has the contract).  The
// third alternative of the same compile-time type: every kernel that forms a score takes Boosted where the other searches
// take NoElig / Elig, and the code it adds sits behind `if constexpr (EL::boosted)` - the other instantiations are the code
// they were.  The returned score is TWO rounded fp32 operations, t = w * b and s = ip + t, never a fused multiply-add
// (the translation unit is compiled with contraction on): boost_term / boost_add (topk_utils.hpp) are the only places that form them.
struct Boosted {
    static constexpr bool on = false, boosted = true;
    const float* boost;      // [nrows]
    const float* weight;     // [nq]
    float boost_max = 0.f;   // >= max |boost| (the finalize kernels' error bound; the other kernels do not take it)
    __device__ __forceinline__ bool ok(long long, int) const { return true; }
    __device__ __forceinline__ float term(long long row, int q) const { return boost_term(weight[q], boost[row]); }
    // the score of row `row` for query q from its inner product
    __device__ __forceinline__ float score(float ip, long long row, int q) const { return boost_add(ip, term(row, q)); }
};
#define AMDREC_BOOST_FIN Boosted, const float*, const float*, float
// finalize_mixed_kernel takes the boost as BO (NoElig: none; Boosted) with its arguments behind the ones it always took.
// eps: with t in both chains the bf16 pass's bound grows by the fp32 slack of the larger partial sums (derivation above
// finalize_mixed_kernel); term: what rescore_keys adds to a re-scored inner product.
template <class BO>
__device__ __forceinline__ float fin_eps(float eps, int d, int q, const BO& bo) {
    if constexpr (BO::boosted)
        return eps * (1.f + 2.f / (float)d) + (float)(d + 1) * 1.2e-7f * (fabsf(bo.weight[q]) * bo.boost_max * 1.0001f);
    else
        return eps;
}
template <class BO>
__device__ __forceinline__ auto fin_term(const BO& bo, int q) {
    if constexpr (BO::boosted) return RowBoost{bo.boost, bo.weight[q]};
    else return NoTerm{};
}
// profile tag of a kernel family for the predicate type
template <class EL>
constexpr const char* tag_for(const char* plain, const char* elig, const char* boost) {
    return EL::boosted ? boost : (EL::on ? elig : plain);
}

// ---- epilogues (lane <-> query, registers <-> corpus rows) ---------------------------
template <class EL>
struct EpiStoreScoresT {
    static constexpr const char* name = tag_for<EL>("search_sample", "search_sample_elig", "search_sample_boost");
    static constexpr double out_bytes_per_elem = 1.0;
    static constexpr size_t lds_bytes(int) { return 0; }
    float* out;          // [nq][ld]
    long long ld;
    int nq;
    long long n_sample;  // sample rows
    DenseRows map;       // to test validity of the mapped row
    [[no_unique_address]] EL el;   // an ineligible (query, row) element is stored as -inf
    template <class A>
    __device__ void operator()(A& acc, float*) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            int q = acc.q(j, lane);
            if (q >= nq) continue;
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    int p = acc.p(i, 4 * g, lane);   // 4 consecutive rows p..p+3
                    if (p >= n_sample) continue;
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float s = acc.v[i][j][4 * g + e];
                        const long long row = map.map(p + e);
                        if constexpr (EL::boosted) s = el.score(s, row < map.rows ? row : 0, q);   // tau: a quantile of the BOOSTED scores
                        v[e] = (row < map.rows && el.ok(row, q)) ? s : -INFINITY;
                    }
                    *reinterpret_cast<f32x4*>(out + (long long)q * ld + p) = v;
                }
        }
    }
};
struct EpiStoreScores : EpiStoreScoresT<NoElig> {};

// Filter epilogue: keys of (score >= tau_q) elements are appended to the per-query candidate lists.  A returning
// global atomic per hit made the epilogue a chain of ~10 dependent 1-2 us round trips per wave (measured: the bf16
// filter spent more time here than in its K loop), so hits are first collected in an LDS list (LDS atomics), and after
// one barrier each hit is appended by its own lane: the global atomics of a block go out together.  Hits beyond the
// LDS list (threshold-less small corpora, adversarial data) take the direct path.
constexpr int HIT_CAP = 2048;
template <class EL>
struct EpiFilterT {
    static constexpr const char* name = tag_for<EL>("search_filter", "search_filter_elig", "search_filter_boost");
    static constexpr double out_bytes_per_elem = 0.0;
    static constexpr size_t lds_bytes(int) { return 16 + (size_t)HIT_CAP * 12; }
    const float* tau;            // [nq]
    unsigned long long* cand;    // [nq][stride], the first cap of each block are used
    int* cnt;                    // [nq]
    int cap, nq;
    long long nrows;
    long long stride;
    [[no_unique_address]] EL el;   // tested with the threshold: the lists only ever hold eligible rows
    __device__ __forceinline__ void append(int q, unsigned long long key) const {
        const int pos = atomicAdd(&cnt[q], 1);
        if (pos < cap) cand[(long long)q * stride + pos] = key;
    }
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
        int* lcount = reinterpret_cast<int*>(smem);
        unsigned long long* hkey = reinterpret_cast<unsigned long long*>(smem + 4);      // 16-byte offset
        int* hq = reinterpret_cast<int*>(hkey + HIT_CAP);
        if (threadIdx.x == 0) *lcount = 0;          // the K loop's last barrier released the staging tiles
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            int q = acc.q(j, lane);
            float t = (q < nq) ? tau[q] : __builtin_nanf("");      // NaN: no score compares >= it
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float s = acc.v[i][j][r];
                    int p = acc.p(i, r, lane);
                    if constexpr (EL::boosted) s = el.score(s, p < nrows ? p : 0, q < nq ? q : 0);   // (NaN stays NaN)
                    if (s >= t && p < nrows && el.ok(p, q)) {
                        const unsigned long long key = make_key(s, (uint32_t)p);
                        const int slot = atomicAdd(lcount, 1);
                        if (slot < HIT_CAP) { hkey[slot] = key; hq[slot] = q; }
                        else append(q, key);
                    }
                }
        }
        __syncthreads();
        const int n = *lcount < HIT_CAP ? *lcount : HIT_CAP;
        for (int h = threadIdx.x; h < n; h += blockDim.x) append(hq[h], hkey[h]);
    }
};
struct EpiFilter : EpiFilterT<NoElig> {};

// Threshold from the sample: tau[q] only has to BOUND the candidate count (any value with
// k <= #{score >= tau} <= capacity gives the exact result), so instead of an exact radix select of the
// r-th largest sample score (3 histogram passes, measured 157 us per launch) each of 256 thread groups
// takes the maximum of its strided share of the sample and tau is the r-th largest of those 256 maxima:
// one coalesced pass.  The true sample rank of that value is >= r (two of the top values may share a
// group; expected r + r^2/512), i.e. the threshold errs on the side of MORE candidates, far inside the capacity.
// NaN counts as lowest; fewer than r finite maxima -> -inf.
constexpr int THR_NT = 1024;
__global__ __launch_bounds__(THR_NT) void sample_threshold_kernel(const float* S, long long ld, long long n, int r,
                                                                  float* tau) {
    __shared__ float mx[THR_NT];
    const int q = blockIdx.x, tid = threadIdx.x;
    const float* row = S + (long long)q * ld;
    float m = -INFINITY;
    // four independent 16-byte loads in flight per thread (one block per query: the pass is latency-bound)
    for (long long i0 = 4ll * tid; i0 < n; i0 += 16 * THR_NT) {  // n % 256 == 0, rows 16-byte aligned
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + 4ll * u * THR_NT;
            v[u] = i < n ? *reinterpret_cast<const f32x4*>(row + i) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) m = (v[u][e] > m) ? v[u][e] : m;   // NaN compares false: ignored
    }
    mx[tid] = m;
    __syncthreads();
    // 256 group maxima (each over 4 threads' shares), ranked by the first 4 waves
    __shared__ float gm[256];
    if (tid < 256) {
        m = fmaxf(fmaxf(mx[tid], mx[tid + 256]), fmaxf(mx[tid + 512], mx[tid + 768]));
        gm[tid] = m;
    }
    __syncthreads();
    if (tid >= 256) return;
    int rank = 0;                     // number of maxima ahead of mine (ties: lower thread first)
    for (int j = 0; j < 256; ++j) {
        const float o = gm[j];
        rank += (o > m) || (o == m && j < tid);
    }
    if (rank == r - 1) tau[q] = m;    // exactly one thread has this rank (r <= 256)
}

// step 4: sort each query's candidate list, or flag it for the fix-up
__global__ __launch_bounds__(512) void finalize_kernel(const unsigned long long* cand, const int* cnt, int cap,
                                                       int k, long long nrows, int* fail, float* outD,
                                                       long long* outI, long long pos_offset) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const int q = blockIdx.x;
    const int c = cnt[q];
    const int need = (int)(nrows < k ? nrows : k);
    if (c < need || c > cap) { give_up(fail, q, gridDim.x); return; }
    int P = 2;
    while (P < c) P <<= 1;
    for (int i = threadIdx.x; i < P; i += blockDim.x) keys[i] = (i < c) ? cand[(long long)q * cap + i] : 0ull;
    __syncthreads();
    bitonic_desc(keys, P);
    write_result(keys, c, k, q, outD, outI, pos_offset);
}

// step 5: exact streaming scan of one corpus slice for a failed query; the block that finishes a query's LAST slice (a
// ticket per query: last_workgroup) merges the slices and writes the result.  One launch: in the common case - no failed
// query - it is the only cost of the fix-up, and two empty launches cost 8 us of a 140 us single-query search.
// EL: the eligibility predicate, tested where a row's key is formed; EP: its pointers, none for NoElig - fixup_kernel<NoElig>
// takes the arguments the scan always took and is the code it always was -, (tags, all, any) for Elig.  A filtered query
// with fewer than k eligible rows always ends here - its candidate count fails the finalize's count test - and gets its
// eligible rows in order and an unfilled tail.
template <class EL, class... EP>
__global__ __launch_bounds__(512) void fixup_kernel(const float* X, long long ldx, long long nrows, int d,
                                                    const float* Q, long long ldq, const int* fail, int nq,
                                                    int k, int nslices, unsigned long long* scratch, int* ticket,
                                                    float* outD, long long* outI, long long pos_offset, EP... elig) {
    const EL el{elig...};
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];      // merge: k * nslices keys (<= CAND_CAP)
    __shared__ __attribute__((aligned(16))) unsigned long long buf[FIX_BUF];
    __shared__ __attribute__((aligned(16))) float qv[2048];
    __shared__ unsigned long long thr;
    __shared__ int count;
    // 1-D grid (query-major) of nslices x min(nq, FIX_GRID_Q) blocks, each looping over its queries: failures are
    // rare, and one block per (query, slice) cost 0.07 ms of empty blocks at 4096 queries
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NW = 8, U = 8;
    const int s = blockIdx.x % nslices;
    if (fail[nq] == 0) return;                                 // fail[nq] = number of failed queries
    for (int q = blockIdx.x / nslices; q < nq; q += gridDim.x / nslices) {
    if (!fail[q]) continue;                                    // block-uniform
    for (int i = tid; i < d; i += 512) qv[i] = Q[(long long)q * ldq + i];
    if (tid == 0) { thr = 0ull; count = 0; }
    __syncthreads();
    const long long per = (nrows + nslices - 1) / nslices;
    const long long begin = (long long)s * per, end = (begin + per < nrows) ? begin + per : nrows;
    const int d4 = d >> 2;
    auto compact = [&]() {
        int c = count;
        for (int i = tid; i < FIX_BUF; i += 512) if (i >= c) buf[i] = 0ull;
        __syncthreads();
        bitonic_desc(buf, FIX_BUF);
        if (tid == 0) {
            int nc = c < k ? c : k;
            count = nc;
            thr = (nc == k) ? buf[k - 1] : 0ull;
        }
        __syncthreads();
    };
    for (long long row0 = begin; row0 < end; row0 += NW * U) {
        float a[U];
        const f32x4* xr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long r = row0 + w * U + u;
            r = r < end ? r : end - 1;                         // clamped: branch-free loads, result dropped below
            xr[u] = reinterpret_cast<const f32x4*>(X + r * ldx);
        }
        dot_rows<U>(xr, qv, d4, lane, a);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long r = row0 + w * U + u;
            if (lane == 0 && r < end && a[u] == a[u] && el.ok(r, q)) {
                if constexpr (EL::boosted) a[u] = el.score(a[u], r, q);
                unsigned long long key = make_key(a[u], (uint32_t)r);
                if (key > thr) {
                    int pos = atomicAdd(&count, 1);
                    buf[pos] = key;   // pos < FIX_BUF guaranteed by the compaction rule below
                }
            }
        }
        __syncthreads();
        // block-uniform decision: every thread reads `count` before anyone may change it again
        if (__syncthreads_or(count > FIX_BUF - NW * U)) compact();
    }
    compact();
    const int c = count;
    unsigned long long* dst = scratch + ((long long)q * nslices + s) * k;
    for (int i = tid; i < k; i += 512) dst[i] = (i < c) ? buf[i] : 0ull;
    // (last_workgroup's first barrier also stands before count / thr / buf are reset)
    if (last_workgroup(&ticket[q], nslices, false)) {          // merge the query's slices
        const int total = k * nslices;
        int P = 2;
        while (P < total) P <<= 1;
        for (int i = tid; i < P; i += 512) keys[i] = (i < total) ? scratch[(long long)q * total + i] : 0ull;
        __syncthreads();
        bitonic_desc(keys, P);
        write_result(keys, total < k ? total : k, k, q, outD, outI, pos_offset);
    }
    __syncthreads();
    }
}

// Cross-shard merge: n_lists sorted lists of list_k entries per query (one per corpus shard, positions
// already global) -> the global top-k.  One block per query, bitonic sort in LDS.
// Short lists (list_k < k, amdrec_topk_merge_partial): a shard sends only its best list_k rows in the search's own total
// order (score descending, ties -> lower position), so every row it did NOT send is strictly behind its last entry in
// that order.  The merged top-k is therefore the exact global top-k iff no FULL list's last entry lies strictly ahead of
// the merged k-th entry - compared as (score, position) keys, the order the merge itself sorts by.  A tie in SCORE alone
// proves nothing either way and is not counted (duplicate ads with bit-identical embeddings are routine,
// training_pipeline.py:523): the last entry of a list may BE the merged k-th, or tie with it at a higher position, and
// the rows behind it still cannot enter.  A query for which the rule fails - a full list that ends ahead of the merged
// k-th key, or fewer than k merged entries - is counted in *inexact.
__global__ __launch_bounds__(512) void topk_merge_kernel(const char* scores, const char* pos, int n_lists, int list_k,
                                                         long long list_stride_bytes, long long q0, int k,
                                                         float* outD, long long* outI, int* inexact) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const long long q = blockIdx.x;
    const int total = n_lists * list_k;
    int P = 2;
    while (P < total) P <<= 1;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        unsigned long long key = 0ull;
        if (i < total) {
            const int g = i / list_k, j = i - g * list_k;
            const float* sg = reinterpret_cast<const float*>(scores + (long long)g * list_stride_bytes);
            const int* pg = reinterpret_cast<const int*>(pos + (long long)g * list_stride_bytes);
            const long long p = pg[(q0 + q) * list_k + j];
            const float sc = sg[(q0 + q) * list_k + j];
            if (p >= 0 && sc == sc) key = make_key(sc, (uint32_t)p);
        }
        keys[i] = key;
    }
    __syncthreads();
    bitonic_desc(keys, P);
    if (inexact != nullptr) {
        const unsigned long long kth = k <= P ? keys[k - 1] : 0ull;
        bool cut = false;
        for (int g = threadIdx.x; g < n_lists; g += blockDim.x) {
            const float* sg = reinterpret_cast<const float*>(scores + (long long)g * list_stride_bytes);
            const int* pg = reinterpret_cast<const int*>(pos + (long long)g * list_stride_bytes);
            const long long p = pg[(q0 + q) * list_k + list_k - 1];
            const float sc = sg[(q0 + q) * list_k + list_k - 1];
            const bool full = p >= 0 && sc == sc;
            cut |= full && (kth == 0ull || make_key(sc, (uint32_t)p) > kth);
        }
        if (__syncthreads_or(cut) && threadIdx.x == 0) atomicAdd(inexact, 1);
    }
    write_result(keys, total < k ? total : k, k, q, outD, outI, 0);
}

// ---- streaming bf16 filter (the mixed search's corpus pass for dim in {32, 64, 128, 256}) ---------------------
// The generic GEMM tiles re-stage the query tile for every corpus tile and prefetch one 128-byte K-step ahead: with
// K = 256 bf16 a tile is only four K-steps of 0.4 us of MFMA each, far less than the HBM latency, and the pass ran
// latency-bound at ~14 % of HBM.  Here the roles are fixed for the whole launch instead:
//  * one 8-wave workgroup per CU; wave w owns queries [64 w, 64 w + 64) of the block's 512-query group and keeps
//    their bf16 fragments for the WHOLE K extent in registers (2 x KS x 4 VGPRs = 128 at dim 256): queries are read
//    once per launch, never staged through LDS (groups of <= 256 queries: the spare waves share the tile's rows);
//  * the corpus streams through a two-deep LDS ring of 128-row full-K tiles (64 KB at dim 256) filled by LDS-DMA
//    (global_load_lds, 16 B per lane, source-side XOR swizzle so the fragment reads are conflict-free); the next tile
//    is in flight during the MFMAs on the current one - one barrier per tile;
//  * every wave multiplies the same 32 corpus rows at a time (one A fragment per k16 step, read from LDS four steps
//    ahead) with its own 64 queries: 2 accumulator tiles, v_mfma_f32_32x32x16_bf16, then compares against tau_q;
//  * hits go to a wave-private LDS list without atomics (ballot + lane prefix; the wave's count lives in an SGPR);
//    one tile later the wave files them in the workgroup's OWN segment of each query's candidate block (slot-major,
//    CAND_CAP / workgroups slots per query; the slot comes from an LDS counter) - no global atomic, and the key stores
//    go out before the next tile's DMA so the in-order vmcnt wait for that DMA never waits for them.  A full segment
//    spills to the query's overflow block through a global counter; finalize_mixed_kernel reads the segments in place.
// Each corpus byte is read from HBM once per 512 queries; waves whose queries lie beyond nq skip their MFMAs, so a
// small batch runs at the HBM rate and a full one at the bf16 MFMA rate.
// tau of ONE query by ONE wave from its row of group maxima gm[0 .. n) (n % 4 == 0, 16-byte aligned): float4 chunk i
// belongs to group i % 256; tau = the r-th largest of the 256 group maxima (r <= 256; fewer than r finite maxima -> -inf;
// NaN never wins a maximum).  The same estimator as sample_threshold_kernel: expected sample rank of the result r + r^2/512,
// i.e. the candidate count errs high, far inside the capacity.  Selection without LDS: a lane holds 4 of the 256 maxima
// as order-preserving 32-bit keys; the r-th largest is built bit by bit (largest T with #{key >= T} >= r), each count a
// ballot + scalar popcount per register - ~500 instructions, where ranking every value against all 256 through LDS cost
// 25 us per query.
__device__ __forceinline__ float wave_tau(const float* row, long long n, int r, int lane) {
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const long long nch = n >> 2;
    for (long long c0 = 0; c0 < nch; c0 += 512) {           // eight independent 16-byte loads in flight per lane
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = c0 + 64 * u + lane;
            v[u] = i < nch ? *reinterpret_cast<const f32x4*>(row + 4 * i) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) m[u & 3] = v[u][e] > m[u & 3] ? v[u][e] : m[u & 3];     // chunk i -> group i % 256
    }
    uint32_t key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t b = __float_as_uint(m[u]);
        key[u] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);     // unsigned order == float order (no NaN among the maxima)
    }
    uint32_t T = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t c = T | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) cnt += __builtin_popcountll(__ballot(key[u] >= c));
        if (cnt >= r) T = c;                                  // wave-uniform
    }
    const uint32_t b = (T & 0x80000000u) ? (T & 0x7fffffffu) : ~T;
    return __uint_as_float(b);
}

// Round 4 measured four other variants of the corpus pass and builds without its DMA or its hit path; none is kept
// (profiles/r04_scan_ab.log, profiles/r04_scan_elim.log).  They are compile-time switches in
// `git show 4973481e75:movie-recommender-demo_amd/csrc/search.hip`, the last version that has them.
constexpr int SCAN_ROWS = 128;          // corpus rows per LDS tile
constexpr int SCAN_WHITS = 128;         // hit-list entries per wave and tile (expected ~11; overflow -> direct append)
constexpr int SCAN_QGROUP = 512;        // queries per workgroup (8 waves x 64)
constexpr int SCAN_HIT_BYTES = 2 * 8 * SCAN_WHITS * 12;   // [2 lists][8 waves] x {keys u64[SCAN_WHITS], q int[SCAN_WHITS]}

// LDS stores of the hit list, hidden from the compiler: it orders every LDS write it can see after the LDS-DMA in
// flight (s_waitcnt vmcnt(0)), which would stall each wave on the next tile's loads at its first hit.  The hit lists
// and the tile ring are disjoint and a wave's LDS operations execute in order, so no wait is needed.
__device__ __forceinline__ void lds_store_hit_opaque(uint32_t key_addr, unsigned long long key, uint32_t q_addr, int q) {
    asm volatile("ds_write_b64 %0, %1\n\tds_write_b32 %2, %3" ::"v"(key_addr), "v"(key), "v"(q_addr), "v"(q) : "memory");
}

// Two 64-bit words from wave-uniform addresses by SCALAR loads.  Spelled out because the compiler, which cannot prove that
// the kernel's own stores leave the words alone, reads them with vector loads otherwise - and a vector load's wait
// (vmcnt counts in order) is also a wait for the LDS-DMA of the next tile.  The scalar loads return on lgkmcnt.
__device__ __forceinline__ void scalar_load_2x64(const uint64_t* p0, const uint64_t* p1, uint64_t& v0, uint64_t& v1) {
    asm volatile("s_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(v0), "=&s"(v1) : "s"(p0), "s"(p1) : "memory");
}
// ... and eight consecutive ones (64 bytes) in one load: w[2 i], w[2 i + 1] = the halves of word i
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ u32x16 scalar_load_8x64(const uint64_t* p) {
    u32x16 w;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(w) : "s"(p) : "memory");
    return w;
}

// ... and 32 consecutive floats (128 bytes, the boosts of one 32-row quarter) in two loads behind one wait
__device__ __forceinline__ void scalar_load_32xf32(const float* p, u32x16& lo, u32x16& hi) {
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo), "=&s"(hi) : "s"(p));
}
// The boosts of a 32-row quarter as the streaming kernels' accumulators see them: bt[4 g + e] = boost of corpus row
// urow + 8 g + 4 fh + e (fh: the lane's half).  The 32 values are wave-uniform, like the eligibility tags: two scalar
// loads, which return on their own counter and never queue behind the LDS-DMA in flight, then one select per value by
// the lane half.  FULL: all 32 rows are corpus rows (urow is a multiple of 32 and the array 64-byte aligned, so the loads
// stay inside it).  In the corpus's last, partial tile a quarter that lies inside the corpus takes the same two loads, one
// beyond its end reads nothing, and the one quarter the corpus ends in (at most one per search, none when nrows % 32 == 0)
// loads the two candidates of each value on their own from clamped rows - 16 pairs of scalar loads, each behind its own
// wait: what the eligibility path does for its tags there.
__device__ __forceinline__ void scalar_load_2xf32(const float* p0, const float* p1, uint32_t& v0, uint32_t& v1) {
    asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dword %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(v0), "=&s"(v1) : "s"(p0), "s"(p1));
}
template <bool FULL>
__device__ __forceinline__ void quarter_boosts(const float* boost, int urow, int fh, int nrows, float (&bt)[16]) {
    if (FULL || urow + 32 <= nrows) {                          // (wave-uniform) every row of the quarter is a corpus row
        u32x16 lo, hi;
        scalar_load_32xf32(boost + urow, lo, hi);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t b0 = g < 2 ? lo[8 * g + e] : hi[8 * (g - 2) + e];
                const uint32_t b1 = g < 2 ? lo[8 * g + 4 + e] : hi[8 * (g - 2) + 4 + e];
                bt[4 * g + e] = __uint_as_float(fh ? b1 : b0);
            }
    } else if (urow >= nrows) {                                // no row of the quarter is: nothing is read
#pragma unroll
        for (int r = 0; r < 16; ++r) bt[r] = 0.f;
    } else {                                                   // the one quarter the corpus ends in: row by row, clamped
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r0 = urow + 8 * g + e, r1 = r0 + 4;
                uint32_t b0, b1;
                scalar_load_2xf32(boost + (r0 < nrows ? r0 : nrows - 1), boost + (r1 < nrows ? r1 : nrows - 1), b0, b1);
                bt[4 * g + e] = __uint_as_float(fh ? b1 : b0);
            }
    }
}

// 16 bytes from global `g` to LDS `l` by LDS-DMA (the LDS address is wave-uniform: lane i's bytes land at l + 16 i)
__device__ __forceinline__ void lds_dma16(const unsigned char* g, unsigned char* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l,
                                     16, 0, 0);
}

// The LDS tile of the streaming passes (scan_filter_kernel, sample_max_kernel) for KS = dim / 16: SCAN_ROWS rows of CPR
// 16-byte chunks, the chunk slot swizzled by row, filled by PASSES LDS-DMA passes of the workgroup's 512 lanes.
// DMA lane map: LDS chunk slot L = u * 512 + tid of pass u -> row u * RPP + tid / CPR, slot tid % CPR; the source chunk
// (slot ^ swizzle(row)) does not depend on u (RPP is a multiple of the swizzle period), so a lane's source address is a
// per-lane byte offset plus a scalar per (tile, pass).
template <int KS>
struct ScanTile {
    static constexpr int CPR = 2 * KS;                                  // 16-byte chunks per row
    static constexpr int FM = CPR < 16 ? CPR - 1 : 15;                  // swizzle mask
    static constexpr int FS = CPR >= 16 ? 0 : (CPR == 8 ? 1 : 2);       // swizzle row shift
    static constexpr int CHUNKS = SCAN_ROWS * CPR;
    static constexpr int PASSES = CHUNKS / 512;
    static constexpr int RPP = 512 / CPR;                               // rows per DMA pass
    static constexpr int AHEAD = KS < 4 ? KS : 4;                       // A fragments read ahead of their MFMA
    static_assert(CHUNKS % 512 == 0, "tile must fill whole DMA passes");

    // byte offset of lane tid's source chunk in its row (row tid / CPR of every pass)
    static __device__ __forceinline__ int src_chunk(int tid) { return ((tid % CPR) ^ (((tid / CPR) >> FS) & FM)) * 16; }
    // byte offset of lane tid's source chunk from a pass's first row, in a corpus of row stride ld16 bf16 values
    static __device__ __forceinline__ uint32_t lane_off(int tid, long long ld16) {
        return (uint32_t)(tid / CPR * (int)ld16 * 2 + src_chunk(tid));
    }
};

// EL (NoElig or Elig): the eligibility predicate.  It is tested in the out-of-line hit path only, never per element: a lane
// keeps the masks of its two queries beside tq[]; a corpus row belongs to an accumulator register and a lane half (a query
// to a lane), so the tags a wave needs in one four-element group are those of eight consecutive rows at a wave-uniform
// address - ONE scalar load per entry of the hit path, which returns on its own counter and so never waits for the LDS-DMA
// of the next tile that is in flight (a vector load would queue behind it).  The loads stay inside the nrows tags: whole
// tiles by construction, the last tile by clamping the row.  The predicate is ANDed into `hit` before the ballot, so the
// wave lists, the segments and the overflow block only ever hold eligible rows, and finalize and certificate need no
// change: a row outside the list is below tau or ineligible.
// EP: the predicate's pointers as trailing kernel arguments - none for NoElig, whose instantiation takes the arguments the
// kernel always took and compiles to the code it always was; (tags, all, any) for Elig.
template <int KS, class EL = NoElig, class... EP>       // KS = dim / 16 in {2, 4, 8, 16}
__global__ __launch_bounds__(512, 1) void scan_filter_kernel(const uint16_t* __restrict__ X16, long long ld16,
                                                             long long nrows, const uint16_t* __restrict__ Q16, int nq,
                                                             float* __restrict__ tau, unsigned long long* cand,
                                                             int* segcnt, int* ocnt, int seg_cap, int nx,
                                                             const float* __restrict__ gm, long long ldm, long long gm_n,
                                                             int rank, EP... elig) {
    const EL el{elig...};
    using Tile = ScanTile<KS>;
    constexpr int CPR = Tile::CPR, TILE_CHUNKS = Tile::CHUNKS, AHEAD = Tile::AHEAD;
    constexpr int NSLOT = 2;                                     // ring slots of SCAN_ROWS rows: the DMA runs a tile ahead
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* tilebuf = lds;                                                  // [NSLOT][TILE_CHUNKS * 16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);                        // scalar: wave-uniform branches below
    unsigned char* hitbase = lds + NSLOT * TILE_CHUNKS * 16 + w * (SCAN_WHITS * 12);   // this wave's list 0; list 1 is
    constexpr int LIST_STRIDE = 8 * SCAN_WHITS * 12;                               // LIST_STRIDE bytes further
    int* lcnt = reinterpret_cast<int*>(lds + NSLOT * TILE_CHUNKS * 16 + SCAN_HIT_BYTES);   // [SCAN_QGROUP] hits per query, this WG
    lcnt[tid] = 0;                                                                 // (before the first DMA is in flight)
    const int frow = lane & 31, fh = lane >> 5;
    const int bx = blockIdx.x % nx, by = blockIdx.x / nx;
    // Work split inside the workgroup.  A full group gives every wave its own 64 queries and all 128 rows of a tile; a
    // group with fewer queries would leave most waves idle and one or two waves with the whole tile's MFMAs, threshold
    // scan and hit handling (measured: 0.205 ms at 128 queries against 0.117 with the split), so the waves without
    // queries of their own take a share of the tile's ROWS instead: 1 / 2 / 4 / 8 query waves x up to four 32-row parts.
    const int nqg = nq - by * SCAN_QGROUP < SCAN_QGROUP ? nq - by * SCAN_QGROUP : SCAN_QGROUP;
    const int qsh = nqg <= 64 ? 0 : (nqg <= 128 ? 1 : (nqg <= 256 ? 2 : 3));       // log2 of the query waves
    const int parts = (8 >> qsh) < 4 ? (8 >> qsh) : 4;                              // 4 / 4 / 2 / 1
    const int part = w >> qsh;
    const int q0 = by * SCAN_QGROUP + (w & ((1 << qsh) - 1)) * 64;
    const bool active = q0 < nq && part < parts;
    const int rq_begin = part * (4 / parts), rq_end = rq_begin + 4 / parts;
    const bool second = q0 + 32 < nq;                                              // second query tile has real queries
    const int ntiles = (int)((nrows + SCAN_ROWS - 1) / SCAN_ROWS);
    const int nrows_i = (int)nrows;                                                // < 2^31 (checked by the entry point)

    // query fragments (clamped rows); the thresholds tq are filled in below, once they are known
    bf16x8 qf[2][KS];
    float tq[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + j * 32 + frow;
        const int qc = q < nq ? q : nq - 1;
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_)
            qf[j][s_] = *reinterpret_cast<const bf16x8*>(Q16 + (long long)qc * (16 * KS) + (2 * s_ + fh) * 8);
    }

    const uint32_t lane_off = Tile::lane_off(tid, ld16);
    auto dma = [&](int row0i, int buf) {                           // SCAN_ROWS rows from corpus row `row0i` into ring slot `buf`
        const long long row0 = row0i;
        unsigned char* lbase = tilebuf + (size_t)buf * TILE_CHUNKS * 16 + (size_t)(w * 64) * 16;           // wave-uniform
        if (row0 + SCAN_ROWS <= nrows) {
            const unsigned char* gb = reinterpret_cast<const unsigned char*>(X16) + row0 * ld16 * 2;
#pragma unroll
            for (int u = 0; u < Tile::PASSES; ++u)
                lds_dma16(gb + (long long)u * Tile::RPP * ld16 * 2 + lane_off, lbase + (size_t)u * 512 * 16);
        } else {                                                   // last tile: rows past the end are clamped
#pragma unroll
            for (int u = 0; u < Tile::PASSES; ++u) {
                long long r = row0 + u * Tile::RPP + tid / CPR;
                r = r < nrows ? r : nrows - 1;
                lds_dma16(reinterpret_cast<const unsigned char*>(X16) + r * ld16 * 2 + Tile::src_chunk(tid),
                          lbase + (size_t)u * 512 * 16);
            }
        }
    };
    // A hit goes to THIS workgroup's segment of the query's candidate block: the slot comes from an LDS counter, so the
    // corpus pass issues no global atomic (a returning device-scope atomic per hit, and its store waited for at the end
    // of the tile, cost 0.07-0.25 ms per pass: profiles/r02_scan_hit_cost.log).  A full segment spills to the query's
    // overflow block through a global counter (large k, skewed data: rare).
    const int qbase = by * SCAN_QGROUP;
    auto append = [&](int q, unsigned long long key) {
        const int slot = atomicAdd(&lcnt[q - qbase], 1);
        unsigned long long* blk = cand + (long long)q * CAND_STRIDE;
        if (slot < seg_cap) {
            blk[slot * nx + bx] = key;                     // slot-major: the used slots of all segments are the block's head
        } else {
            const int o = atomicAdd(&ocnt[q], 1);
            if (o < CAND_CAP) blk[CAND_CAP + o] = key;
        }
    };
    // 32 corpus rows (LDS image at `lb`, fragment k-offset swizzle G) x NJ query tiles: K loop with the A fragments
    // read AHEAD steps before their MFMA, then the threshold scan.  wcount = this wave's hits so far in this tile.
    uint64_t qall[2] = {0ull, 0ull}, qany[2] = {0ull, 0ull};       // (filtered instantiations only)
    float wq[2] = {0.f, 0.f};                                      // (boosted instantiations only) weights of the lane's queries
    auto quarter = [&](auto nj_tag, auto full_tag, const unsigned char* lb, int G, int prow, uint32_t list_addr,
                       int& wcount, int urow) {                    // urow: the quarter's first corpus row (wave-uniform)
        constexpr int NJ = decltype(nj_tag)::value;
        constexpr bool FULL = decltype(full_tag)::value;           // every row of the tile is a corpus row
        f32x16 acc[NJ];
        if constexpr (EL::boosted) {
            // the accumulators start at t = w_q * boost[row] where the plain pass zeroes them: the threshold test, the hit
            // lists and the keys see the boosted approximate score and nothing downstream of the MFMAs changes
            float bt[16];
            quarter_boosts<FULL>(el.boost, urow, fh, nrows_i, bt);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = boost_term(wq[j], bt[r]);
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        }
        bf16x8 a[AHEAD];
#pragma unroll
        for (int s_ = 0; s_ < AHEAD; ++s_) a[s_] = *reinterpret_cast<const bf16x8*>(lb + ((32 * s_) ^ G));
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_) {
            const bf16x8 cur = a[s_ % AHEAD];
            if (s_ + AHEAD < KS) a[s_ % AHEAD] = *reinterpret_cast<const bf16x8*>(lb + ((32 * (s_ + AHEAD)) ^ G));
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur, qf[j][s_], acc[j], 0, 0, 0);
        }
        // The source reads a fragment AHEAD k-steps before its MFMAs, but the machine scheduler hoists ALL KS reads of the
        // quarter to its top (it has the registers) and waits for the last of them before the first MFMA: a quarter then
        // runs [16 LDS reads, one full wait] [32 MFMAs] [threshold scan] with nothing overlapped - 0.21 ms per pass with
        // DMA and hits compiled out, against 0.10 at the MFMA rate (profiles/r04_scan_elim.log, the ISA in DESIGN.md).
        // The schedule is therefore spelled out: AHEAD reads, then per k-step the NJ MFMAs followed by one read.
        __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);                           // DS reads
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_) {
            __builtin_amdgcn_sched_group_barrier(0x008, NJ, 0);                          // MFMAs of k-step s_
            if (s_ + AHEAD < KS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // the read AHEAD steps on
        }
        // Threshold scan.  A hit is rare per element (~1.4e-3) but a taken branch per element costs more than the
        // MFMAs it follows, so four elements share one test (their maximum; NaN never wins) and the per-element code is
        // out of line.  (A single v_max3 tree + one test over all 16 elements of a tile was measured in a same-box A/B,
        // profiles/r02_scan_tree16_ab.log: 25 % SLOWER at 512 queries - 0.383 vs 0.307 ms - the four short independent
        // chains overlap with the MFMAs better than one deep one.)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float m4 = fmaxf(fmaxf(acc[j][4 * g], acc[j][4 * g + 1]), fmaxf(acc[j][4 * g + 2], acc[j][4 * g + 3]));
                if (__builtin_expect(__ballot(m4 >= tq[j]) == 0ull, 1)) continue;
                // (filtered, whole tile) the tags of the group's eight rows urow + 8 g .. + 7 in one scalar load: one wait per
                // entry of the hit path, which a wave enters for ~30 % of its groups - some lane of 64 has a hit in 4 elements
                u32x16 tw = {};
                if constexpr (EL::on) {
                    if constexpr (FULL) tw = scalar_load_8x64(el.tags + urow + 8 * g);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sc = acc[j][4 * g + e];
                    const int p = prow + e + 8 * g;
                    bool hit = sc >= tq[j] && (FULL || p < nrows_i);
                    if constexpr (EL::on) {
                        // rows urow + e + 8 g (lanes 0-31) and + 4 (lanes 32-63); last tile: clamped into the nrows tags
                        // (skipping the test for an element no lane has a hit in - one more ballot and branch - was measured
                        // slower: 0.407 against 0.377 ms per pass at 512 queries, and 17 spilled SGPRs at dim 256)
                        uint64_t t0, t1;
                        if constexpr (FULL) {
                            t0 = tw[2 * e] | ((uint64_t)tw[2 * e + 1] << 32);
                            t1 = tw[2 * e + 8] | ((uint64_t)tw[2 * e + 9] << 32);
                        } else {
                            const int r0 = urow + e + 8 * g, r1 = r0 + 4;
                            scalar_load_2x64(el.tags + (r0 < nrows_i ? r0 : nrows_i - 1),
                                             el.tags + (r1 < nrows_i ? r1 : nrows_i - 1), t0, t1);
                        }
                        hit = hit && tag_ok(fh ? t1 : t0, qall[j], qany[j]);
                    }
                    const unsigned long long mask = __ballot(hit);
                    if (mask) {                                    // wave-uniform
                        if (hit) {
                            const int q = q0 + j * 32 + frow;
                            const unsigned long long key = make_key(sc, (uint32_t)p);
                            const int slot = wcount + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                            if (slot < SCAN_WHITS)
                                lds_store_hit_opaque(list_addr + slot * 8, key, list_addr + SCAN_WHITS * 8 + slot * 4, q);
                            else append(q, key);
                        }
                        wcount += __builtin_popcountll(mask);
                    }
                }
            }
    };

    // tile sequence of this workgroup: bx, bx + nx, ...
    const int my_tiles = bx < ntiles ? (ntiles - bx + nx - 1) / nx : 0;
    auto tile_row0 = [&](int i) { return (bx + i * nx) * SCAN_ROWS; };             // < 2^31 (entry point)
#pragma unroll
    for (int i = 0; i < NSLOT - 1; ++i)
        if (i < my_tiles) dma(tile_row0(i), i);
    // Thresholds.  Batches of <= 8 queries (gm != nullptr): no threshold launch - while the first tile is in flight wave w
    // computes tau of query w from the sample's group maxima (wave_tau: a deterministic function of gm, so every workgroup
    // arrives at the same value), workgroup 0 publishes it for the finalize.  Columns >= nq get NaN: no score compares >= it.
    __shared__ float tau_sh[8];
    if (gm != nullptr) {
        if (w < nq) {
            const float tw = wave_tau(gm + (long long)w * ldm, gm_n, rank, lane);
            if (lane == 0) {
                tau_sh[w] = tw;
                if (bx == 0) tau[w] = tw;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                               // first tile landed, tau_sh written
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + j * 32 + frow;
        tq[j] = (q < nq) ? (gm != nullptr ? tau_sh[q] : tau[q]) : __builtin_nanf("");
        if constexpr (EL::on) {
            qall[j] = el.all[q < nq ? q : nq - 1];
            qany[j] = el.any[q < nq ? q : nq - 1];
        }
        if constexpr (EL::boosted) wq[j] = el.weight[q < nq ? q : nq - 1];
    }
    int it = 0, wprev = 0;                                         // wprev: hits of the previous tile awaiting their append
    for (; it < my_tiles; ++it) {
        const int buf = it % NSLOT, lst = it & 1;
        const int prow0 = tile_row0(it);
        // previous tile's hits: slots from the LDS counters, keys to the segment - issued BEFORE this tile's DMA so that the
        // end-of-tile wait for the DMA (vmcnt counts in order) never waits for these stores
        const unsigned char* lprev = hitbase + (lst ^ 1) * LIST_STRIDE;
        const int npend = wprev < SCAN_WHITS ? wprev : SCAN_WHITS;
        for (int h = lane; h < npend; h += 64)
            append(reinterpret_cast<const int*>(lprev + SCAN_WHITS * 8)[h],
                   reinterpret_cast<const unsigned long long*>(lprev)[h]);
        // (the DMA goes out right after the barrier: issuing it behind the first quarter's MFMAs, the move that gained 4 % in
        // the row-owner kernel, cost 30 % here - 0.355 against 0.268 ms at 512 queries, profiles/r03_scan_late_dma_ab.log: with a
        // two-deep ring the next tile needs the whole of this tile's compute time to land)
        // the tile read NSLOT - 1 iterations from now: its ring slot was read in the previous iteration
        if (it + NSLOT - 1 < my_tiles) dma(tile_row0(it + NSLOT - 1), (it + NSLOT - 1) % NSLOT);
        int wcount = 0;
        if (active) {
            // fragment address = lane row base + compile-time row offset + ((32 s) ^ G): the swizzle term depends on
            // the lane only through G.  G is made opaque per 32-row step so that the fragment addresses are recomputed
            // (one v_xor each) instead of being hoisted out of the loops into live registers (spills at KS = 16).
            int G = (fh ^ ((frow >> Tile::FS) & Tile::FM)) << 4;
            const unsigned char* lb = tilebuf + (size_t)buf * TILE_CHUNKS * 16 + frow * CPR * 16;
            const uint32_t list_addr =
                (uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)(hitbase + lst * LIST_STRIDE);
            const bool full = prow0 + SCAN_ROWS <= nrows_i;
            // one quarter LOOP per (query tiles, full tile) variant: with the variant chosen inside the loop the compiler
            // merged the four variants' identical fragment reads in front of the branch - in a different basic block than
            // their MFMAs, where no schedule can interleave them
            auto quarters = [&](auto nj_tag, auto full_tag) {
#pragma unroll 1
                for (int rq = rq_begin; rq < rq_end; ++rq) {
                    asm volatile("" : "+v"(G));
                    quarter(nj_tag, full_tag, lb + rq * 32 * CPR * 16, G, prow0 + rq * 32 + 4 * fh, list_addr, wcount,
                            prow0 + rq * 32);
                }
            };
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            if (second) {
                if (full) quarters(I2{}, std::true_type{});
                else      quarters(I2{}, std::false_type{});
            } else {
                if (full) quarters(I1{}, std::true_type{});
                else      quarters(I1{}, std::false_type{});
            }
        }
        wprev = wcount;
        // my share of the next tile has landed, my hit stores are done: the DMA issued above is the youngest operation
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                 // this tile consumed by every wave, the next one visible
    }
    // the last tile's hits
    const unsigned char* llast = hitbase + ((it & 1) ^ 1) * LIST_STRIDE;
    const int nlast = wprev < SCAN_WHITS ? wprev : SCAN_WHITS;
    for (int h = lane; h < nlast; h += 64)
        append(reinterpret_cast<const int*>(llast + SCAN_WHITS * 8)[h], reinterpret_cast<const unsigned long long*>(llast)[h]);
    __syncthreads();
    if (tid < nqg) segcnt[(long long)(qbase + tid) * nx + bx] = lcnt[tid];      // every (query, segment) count is written: no memset
}

// ---- fused query conversion + sample pass of the mixed search (dims 32 / 64 / 128 / 256) ---------------------------
// One launch instead of three (bf16_rows_kernel for the queries, a generic-tile GEMM that stored the DENSE sample score
// matrix - 94 MB at 512 queries x 46k sample rows - and the threshold kernel that read it back): the same streaming
// structure as scan_filter_kernel over an evenly spaced subset of 128-row corpus tiles, with
//  * the queries converted fp32 -> bf16 in the prologue (same rounding as bf16_rows_kernel; the workgroups with bx == 0
//    also write the bf16 rows the corpus pass reads, and every workgroup clears its share of the search's counters);
//  * the epilogue keeping only MAXIMA: per (query, 16- / 4- / 1-row group) one float in gm[nq][ldm] - the threshold only
//    needs the r-th largest of ~256 group maxima of the sample (see wave_tau), and a maximum of maxima is the maximum.
// SUB = values per lane, query tile and 32-row quarter: 1 (16-row groups), 4 (4-row groups), 16 (every score: corpora so
// small that coarser groups would leave fewer than ~1000 columns).  Column of a value: ((tile * 4 + quarter) * 2 + fh) * SUB + i.
// EL = Elig: the score of an ineligible (query, row) pair becomes -inf before it enters a group
// maximum (before it is stored, SUB == 16), so the r-th largest maximum - wave_tau, unchanged - is taken over the query's
// ELIGIBLE sample rows and sits at the quantile that admits ~target eligible rows whatever fraction of the corpus is
// eligible; fewer than r eligible sample rows -> fewer than r finite maxima -> tau = -inf.
template <int KS, int SUB, class EL = NoElig, class... EP>
__global__ __launch_bounds__(512, 1) void sample_max_kernel(const uint16_t* __restrict__ X16, long long ld16, int tstride,
                                                            int n_tiles, const float* __restrict__ Q, long long ldq, int nq,
                                                            uint16_t* __restrict__ Q16, float* __restrict__ gm, long long ldm,
                                                            int nx, int* zero, long long n_zero, EP... elig) {
    const EL el{elig...};
    using Tile = ScanTile<KS>;
    constexpr int CPR = Tile::CPR, TILE_CHUNKS = Tile::CHUNKS, PASSES = Tile::PASSES, AHEAD = Tile::AHEAD;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];                      // [2][TILE_CHUNKS * 16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;
    const int bx = blockIdx.x % nx, by = blockIdx.x / nx;
    for (long long i = (long long)blockIdx.x * 512 + tid; i < n_zero; i += (long long)gridDim.x * 512) zero[i] = 0;
    // the same work split as the corpus pass: waves without queries of their own take a share of the tile's rows (written
    // out in both kernels: a shared helper, or one kernel's expression for `parts` in the other, changes their code)
    const int nqg = nq - by * SCAN_QGROUP < SCAN_QGROUP ? nq - by * SCAN_QGROUP : SCAN_QGROUP;
    const int qsh = nqg <= 64 ? 0 : (nqg <= 128 ? 1 : (nqg <= 256 ? 2 : 3));
    const int parts = qsh <= 1 ? 4 : (qsh == 2 ? 2 : 1);
    const int part = w >> qsh;
    const int q0 = by * SCAN_QGROUP + (w & ((1 << qsh) - 1)) * 64;
    const bool active = q0 < nq && part < parts;
    const int rq_begin = part * (4 / parts), rq_end = rq_begin + 4 / parts;
    const bool second = q0 + 32 < nq;

    // query fragments: 8 consecutive floats -> 8 bf16 (round to nearest even, NaN kept: bf16_rows_kernel's rounding)
    bf16x8 qf[2][KS];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + j * 32 + frow;
        const int qc = q < nq ? q : nq - 1;
        const bool wr = bx == 0 && part == 0 && q < nq;              // exactly one lane pair per (query, k-step) writes
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_) {
            const float* src = Q + (long long)qc * ldq + (2 * s_ + fh) * 8;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
            uint32_t h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = e < 4 ? v0[e & 3] : v1[e & 3];
                const uint32_t u = __float_as_uint(v);
                h[e] = (v != v) ? 0x7fc0u : ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
            }
            const u32x4 pk{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            qf[j][s_] = __builtin_bit_cast(bf16x8, pk);
            if (wr && q0 + j * 32 < nq) *reinterpret_cast<u32x4*>(Q16 + (long long)q * (16 * KS) + (2 * s_ + fh) * 8) = pk;
        }
    }
    uint64_t qall[2] = {0ull, 0ull}, qany[2] = {0ull, 0ull};       // (filtered instantiations only) masks of the lane's queries
    if constexpr (EL::on) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + j * 32 + frow;
            qall[j] = el.all[q < nq ? q : nq - 1];
            qany[j] = el.any[q < nq ? q : nq - 1];
        }
    }
    float wq[2] = {0.f, 0.f};                                      // (boosted instantiations only) weights of the lane's queries
    if constexpr (EL::boosted) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = q0 + j * 32 + frow;
            wq[j] = el.weight[q < nq ? q : nq - 1];
        }
    }
    // tile DMA (sample tiles are whole tiles: no clamped path)
    const uint32_t lane_off = Tile::lane_off(tid, ld16);
    auto dma = [&](int st_, int buf) {
        const long long row0 = (long long)st_ * tstride * SCAN_ROWS;
        unsigned char* lbase = lds + (size_t)buf * TILE_CHUNKS * 16 + (size_t)(w * 64) * 16;
        const unsigned char* gb = reinterpret_cast<const unsigned char*>(X16) + row0 * ld16 * 2;
#pragma unroll
        for (int u = 0; u < PASSES; ++u) lds_dma16(gb + (long long)u * Tile::RPP * ld16 * 2 + lane_off, lbase + (size_t)u * 512 * 16);
    };
    // both buffers are requested up front (a workgroup of a 1M-row search has one or two tiles: their latencies overlap);
    // from the third tile on a buffer is re-filled as soon as every wave has left it
    int t = bx;
    if (t < n_tiles) dma(t, 0);
    if (t + nx < n_tiles) {
        dma(t + nx, 1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PASSES) : "memory");     // the first tile's pieces (issued first) landed
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int it = 0; t < n_tiles; t += nx, ++it) {
        const int buf = it & 1;
        if (it > 0 && t + nx < n_tiles) dma(t + nx, buf ^ 1);
        if (active) {
            int G = (fh ^ ((frow >> Tile::FS) & Tile::FM)) << 4;
            const unsigned char* lb = lds + (size_t)buf * TILE_CHUNKS * 16 + frow * CPR * 16;
            // one quarter loop per number of live query tiles, the LDS-read / MFMA interleave spelled out (as in
            // scan_filter_kernel's quarter: with `if (second)` inside the K loop every k-step ended a basic block)
            auto quarters = [&](auto nj_tag) {
                constexpr int NJ = decltype(nj_tag)::value;
#pragma unroll 1
                for (int rq = rq_begin; rq < rq_end; ++rq) {
                    asm volatile("" : "+v"(G));
                    const unsigned char* lq = lb + rq * 32 * CPR * 16;
                    f32x16 acc[NJ];
                    if constexpr (EL::boosted) {
                        // as in the corpus pass: the sample's scores are the boosted ones, so tau lands on THEIR quantile
                        const int urow = (int)((long long)t * tstride * SCAN_ROWS) + rq * 32;      // < 2^31 (entry point)
                        float bt[16];
                        quarter_boosts<true>(el.boost, urow, fh, 0, bt);
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[j][r] = boost_term(wq[j], bt[r]);
                    } else {
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
                    }
                    bf16x8 a[AHEAD];
#pragma unroll
                    for (int s_ = 0; s_ < AHEAD; ++s_) a[s_] = *reinterpret_cast<const bf16x8*>(lq + ((32 * s_) ^ G));
#pragma unroll
                    for (int s_ = 0; s_ < KS; ++s_) {
                        const bf16x8 cur = a[s_ % AHEAD];
                        if (s_ + AHEAD < KS) a[s_ % AHEAD] = *reinterpret_cast<const bf16x8*>(lq + ((32 * (s_ + AHEAD)) ^ G));
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur, qf[j][s_], acc[j], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);
#pragma unroll
                    for (int s_ = 0; s_ < KS; ++s_) {
                        __builtin_amdgcn_sched_group_barrier(0x008, NJ, 0);
                        if (s_ + AHEAD < KS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    const long long col0 = (((long long)t * 4 + rq) * 2 + fh) * SUB;
                    if constexpr (EL::on) {
                        // acc[j][4 g + e] is corpus row (tile row0) + 32 rq + 8 g + 4 fh + e: four tags per g and lane
                        const uint64_t* tg = el.tags + (long long)t * tstride * SCAN_ROWS + rq * 32 + 4 * fh;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            uint64_t tw[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) tw[e] = tg[8 * g + e];
#pragma unroll
                            for (int j = 0; j < NJ; ++j)
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (!tag_ok(tw[e], qall[j], qany[j])) acc[j][4 * g + e] = -INFINITY;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int q = q0 + j * 32 + frow;
                        if (q >= nq) continue;
                        float* dst = gm + (long long)q * ldm + col0;
                        if (SUB == 16) {
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                *reinterpret_cast<f32x4*>(dst + 4 * g) = f32x4{acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
                        } else {
                            float m4[4];
#pragma unroll
                            for (int g = 0; g < 4; ++g) {       // v > m ? v : m: a NaN score never wins (sample_threshold_kernel's rule)
                                float m = acc[j][4 * g];
#pragma unroll
                                for (int e = 1; e < 4; ++e) m = acc[j][4 * g + e] > m ? acc[j][4 * g + e] : m;
                                m4[g] = m;
                            }
                            if (SUB == 4) {
                                *reinterpret_cast<f32x4*>(dst) = f32x4{m4[0], m4[1], m4[2], m4[3]};
                            } else {
                                float m = m4[0];
#pragma unroll
                                for (int g = 1; g < 4; ++g) m = m4[g] > m ? m4[g] : m;
                                *dst = m;
                            }
                        }
                    }
                }
            };
            if (second) quarters(std::integral_constant<int, 2>{});
            else quarters(std::integral_constant<int, 1>{});
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// tau[q] for every query from the group maxima: one wave per query, eight queries per workgroup
__global__ __launch_bounds__(512) void tau_from_maxima_kernel(const float* gm, long long ldm, long long n, int r, int nq,
                                                              float* tau) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 8 + w;
    if (q >= nq) return;
    const float t = wave_tau(gm + (long long)q * ldm, n, r, lane);
    if (lane == 0) tau[q] = t;
}

// segments per query = workgroups per 512-query group of the streaming pass; each owns CAND_CAP / nseg candidate slots
static inline int scan_segments(long long nrows, long long nq) {
    const long long ntiles = (nrows + SCAN_ROWS - 1) / SCAN_ROWS;
    const long long ny = (nq + SCAN_QGROUP - 1) / SCAN_QGROUP;
    long long nx = 256 / ny;                       // one workgroup per CU
    if (nx < 1) nx = 1;
    if (nx > ntiles) nx = ntiles;
    return (int)(nx < 1 ? 1 : nx);
}

template <class EL>
struct ScanKernels;                      // the streaming and fix-up kernels of a search without (NoElig) / with (Elig) eligibility masks
template <>
struct ScanKernels<NoElig> {
    static constexpr const char *scan_tag = "search_filter_stream128x512_bf16", *sample_tag = "search_sample_max128x512_bf16";
    template <int KS> static constexpr auto scan() { return scan_filter_kernel<KS>; }
    template <int KS, int SUB> static constexpr auto sample() { return sample_max_kernel<KS, SUB>; }
    static auto fixup() { return fixup_kernel<NoElig>; }
};
template <>
struct ScanKernels<Elig> {
    static constexpr const char *scan_tag = "search_filter_stream128x512_bf16_elig",
                                *sample_tag = "search_sample_max128x512_bf16_elig";
#define AMDREC_ELIG_ARGS Elig, const uint64_t*, const uint64_t*, const uint64_t*
    template <int KS> static constexpr auto scan() { return scan_filter_kernel<KS, AMDREC_ELIG_ARGS>; }
    template <int KS, int SUB> static constexpr auto sample() { return sample_max_kernel<KS, SUB, AMDREC_ELIG_ARGS>; }
    static auto fixup() { return fixup_kernel<AMDREC_ELIG_ARGS>; }
#undef AMDREC_ELIG_ARGS
};
template <>
struct ScanKernels<Boosted> {
    static constexpr const char *scan_tag = "search_filter_stream128x512_bf16_boost",
                                *sample_tag = "search_sample_max128x512_bf16_boost";
#define AMDREC_BOOST_ARGS Boosted, const float*, const float*
    template <int KS> static constexpr auto scan() { return scan_filter_kernel<KS, AMDREC_BOOST_ARGS>; }
    template <int KS, int SUB> static constexpr auto sample() { return sample_max_kernel<KS, SUB, AMDREC_BOOST_ARGS>; }
    static auto fixup() { return fixup_kernel<AMDREC_BOOST_ARGS>; }
#undef AMDREC_BOOST_ARGS
};
// launches `kern` with the predicate's pointers after the arguments every instantiation takes (NoElig: none)
template <class Kern, class... Args>
static void launch_with(NoElig, Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
}
template <class Kern, class... Args>
static void launch_with(Elig el, Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(kern, grid, block, lds, st, args..., el.tags, el.all, el.any);
}
template <class Kern, class... Args>
static void launch_with(Boosted bo, Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(kern, grid, block, lds, st, args..., bo.boost, bo.weight);
}

template <int KS, class EL = NoElig>
static hipError_t launch_scan(const uint16_t* X16, long long ld16, long long nrows, const uint16_t* Q16, int nq,
                              float* tau, unsigned long long* cand, int* segcnt, int* ocnt, hipStream_t st,
                              const float* gm = nullptr, long long ldm = 0, long long gm_n = 0, int rank = 0, EL el = EL{}) {
    auto kern = ScanKernels<EL>::template scan<KS>();
    constexpr size_t lds_bytes = 2ull * SCAN_ROWS * 2 * KS * 16 + SCAN_HIT_BYTES + SCAN_QGROUP * 4;
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    static PerDeviceOnce attr_done;
    if (attr_done.pending()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_done.mark();
    }
    const int ny = (nq + SCAN_QGROUP - 1) / SCAN_QGROUP;
    const int nx = scan_segments(nrows, nq);
    const int d = 16 * KS;
    ProfScope prof(ScanKernels<EL>::scan_tag, 2.0 * (double)nrows * (double)nq * d,
                   2.0 * ((double)nrows * d * ny + (double)nq * d), st);
    launch_with(el, kern, dim3((unsigned)(nx * ny)), dim3(512), lds_bytes, st, X16, ld16, nrows, Q16, nq, tau, cand, segcnt,
                ocnt, CAND_CAP / nx, nx, gm, ldm, gm_n, rank);
    return hipGetLastError();
}

// the fused conversion + sample launch: n_tiles evenly spaced 128-row tiles -> gm[nq][ldm], ldm = columns = n_tiles * 8 * SUB
struct SamplePlan {
    int n_tiles, tstride, sub;
    long long cols;
};
static inline SamplePlan sample_plan(long long nrows, long long n_sample_rows) {
    SamplePlan sp;
    const long long full = nrows / SCAN_ROWS;                          // whole tiles only
    long long nt = (n_sample_rows + SCAN_ROWS - 1) / SCAN_ROWS;
    if (nt > full) nt = full;
    if (nt < 1) nt = 1;
    sp.n_tiles = (int)nt;
    sp.tstride = (int)(full / nt);
    const long long rows = nt * SCAN_ROWS;
    sp.sub = rows / 16 >= 1024 ? 1 : (rows / 4 >= 1024 ? 4 : 16);      // keep >= ~1000 columns where the sample allows
    sp.cols = nt * 8 * sp.sub;
    return sp;
}
template <int KS, class EL = NoElig>
static hipError_t launch_sample(const uint16_t* X16, long long ld16, const SamplePlan& sp, const float* Q, long long ldq,
                                int nq, uint16_t* Q16, float* gm, int* zero, long long n_zero, hipStream_t st, EL el = EL{}) {
    using K = ScanKernels<EL>;
    constexpr size_t lds_bytes = 2ull * SCAN_ROWS * 2 * KS * 16;
    static PerDeviceOnce attr_done;
    if (attr_done.pending()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K::template sample<KS, 1>()),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(K::template sample<KS, 4>()),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(K::template sample<KS, 16>()),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_done.mark();
    }
    const int ny = (nq + SCAN_QGROUP - 1) / SCAN_QGROUP;
    int nx = 256 / ny;
    nx = nx < 1 ? 1 : (nx > sp.n_tiles ? sp.n_tiles : nx);
    const int d = 16 * KS;
    ProfScope prof(K::sample_tag, 2.0 * (double)sp.n_tiles * SCAN_ROWS * (double)nq * d,
                   2.0 * (double)sp.n_tiles * SCAN_ROWS * d * ny + 4.0 * (double)nq * d + 4.0 * (double)nq * sp.cols, st);
    const dim3 grid((unsigned)(nx * ny)), block(512);
    if (sp.sub == 1)
        launch_with(el, K::template sample<KS, 1>(), grid, block, lds_bytes, st, X16, ld16, sp.tstride, sp.n_tiles, Q, ldq, nq,
                    Q16, gm, sp.cols, nx, zero, n_zero);
    else if (sp.sub == 4)
        launch_with(el, K::template sample<KS, 4>(), grid, block, lds_bytes, st, X16, ld16, sp.tstride, sp.n_tiles, Q, ldq, nq,
                    Q16, gm, sp.cols, nx, zero, n_zero);
    else
        launch_with(el, K::template sample<KS, 16>(), grid, block, lds_bytes, st, X16, ld16, sp.tstride, sp.n_tiles, Q, ldq, nq,
                    Q16, gm, sp.cols, nx, zero, n_zero);
    return hipGetLastError();
}

// fp32 rows -> bf16 rows (round to nearest even, NaN kept), one wave per row; optionally max_norm[0] = the maximum row norm
// and max_norm[1] = the maximum ROUNDING-ERROR norm max_r ||x_r - bf16(x_r)||_2, the two corpus-side terms of the search's
// error bound (atomic max over the float bits: norms are >= 0 so the unsigned order is the float order; NaN/inf propagate
// and make every certificate fail -> exact fix-up path).
__global__ __launch_bounds__(256) void bf16_rows_kernel(const float* x, long long rows, long long ld, int d,
                                                        uint16_t* out, long long ld_out, float* max_norm,
                                                        int* zero = nullptr, long long n_zero = 0) {
    // optional: clear n_zero ints (the search's counters, so that a search call needs no separate memset launch)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_zero; i += (long long)gridDim.x * 256) zero[i] = 0;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    float ss = 0.f, ds = 0.f;
    for (int c = lane; c < (d >> 2); c += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ld + 4 * c);
        uint32_t h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t u = __float_as_uint(v[e]);
            h[e] = (v[e] != v[e]) ? 0x7fc0u : bf16_rne(u);
            ss += v[e] * v[e];
            const float dv = v[e] - __uint_as_float(h[e] << 16);       // exact: the rounding error of this component
            ds += dv * dv;
        }
        uint2 pk{h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
        *reinterpret_cast<uint2*>(out + r * ld_out + 4 * c) = pk;
    }
    if (max_norm) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ss += __shfl_xor(ss, o, 64);
            ds += __shfl_xor(ds, o, 64);
        }
        if (lane == 0) {
            // the maxima only grow: look first, update only when this row raises one.  An unconditional atomicMax per row
            // serialised 2 x 10M device-scope atomics on two addresses: 227 ms for a 10M-row shadow that moves 15 GB
            // (profiles/r04_ivf10m_kernel_stats.csv), 68 GB/s
            unsigned int* m = reinterpret_cast<unsigned int*>(max_norm);
            const unsigned int a = __float_as_uint(sqrtf(ss));
            // rounded UP a little: the sum above is itself an fp32 evaluation
            const unsigned int b = __float_as_uint(sqrtf(ds) * 1.0001f);
            if (__hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a) atomicMax(m, a);
            if (__hip_atomic_load(m + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < b) atomicMax(m + 1, b);
        }
    }
}

// Error bound of the bf16 pass, from MEASURED rounding errors (rigorous, and ~4x tighter than the worst case on real data):
// with q~ = bf16(q), x~ = bf16(x), dq = q~ - q, dx = x~ - x:   q~.x~ - q.x = dq.x~ + q.dx   (an identity), hence
//   |approx - exact| <= ||dq|| ||x~|| + ||q|| ||dx|| <= ||dq|| (M + D) + ||q|| D,    M = max_r ||x_r||, D = max_r ||dx_r||
// (M, D accumulated by amdrec_bf16_rows when the shadow is written; ||dq|| computed here from the query itself), plus
// 2 d 2^-24 ||q|| (M + D) for the two fp32 accumulations being compared.  The worst case of this bound is the classical
// (2u + u^2) ||q|| M with u = 2^-8 (every component half an ulp off: tests/test_search_gpu.py::
// test_mixed_worst_case_rounding, where round 1's u = 2^-9 constant returned a wrong top-k); on random unit vectors
// ||dq|| ~ ||dx|| ~ 0.0008, i.e. eps ~ 0.0018 instead of 0.0078: half as many candidates survive the prune and are re-scored.
// With a boost (fin_eps): the two numbers compared are a = fl(t (+) q~.x~), the MFMA chain STARTED at t = fl(w b) (generic
// tiles: fl(fl(q~.x~) + t)), and s = fl(fl(q.x) + t).  t is the same number on both sides and adds no error of its own; what
// grows is the fp32 slack, because every partial sum of the approximate chain is now bounded by P = |w| B + ||q|| (M + D)
// (B >= max |boost|) instead of ||q|| (M + D), and s carries one more rounding of a value <= P.  With u = 2^-24:
//   approximate chain  d u P  (generic tiles: d u ||q|| (M + D) + u P),   exact side  d u ||q|| M + u P,
// so beyond the plain bound's 2 d u ||q|| (M + D) the slack is at most (d + 1) u |w| B + 2 u ||q|| (M + D).  The last term is
// <= eps_plain / d (eps_plain contains d * 1.2e-7 ||q|| (M + D) and 1.2e-7 > 2 u); fin_eps takes
//   eps = eps_plain (1 + 2 / d) + (d + 1) * 1.2e-7 * |w| B * 1.0001        (twice the terms above)
// and uses it wherever eps_plain was: the prune a_k - 2 eps, the certificate tau + eps, in both finalize kernels.  A query
// with w = 0 pays the factor 1 + 2 / d only; |w| B = 256 at d = 256 gives eps ~ 0.008 + eps_plain, i.e. the worst case of
// the bf16 bound again: more survivors to re-score, never a wrong result.  A non-finite w makes eps non-finite: fix-up scan.
// (eps_bound itself lives in topk_utils.hpp: the IVF scan's bf16 prefilter uses the same bound)

// step 4 of the mixed-precision search: select a_k -> prune -> fp32 re-score -> exact sort -> certificate, one workgroup per
// query.  The candidate keys (<= CAPK / NT + overflow share per thread) stay in registers for the selection: a 3-pass radix
// select of the k-th largest approximate score (LDS histograms), then only the survivors of the pruning rule go to LDS, are
// re-scored and sorted (typically ~1.25 k keys instead of the whole list at k = 500).
// Small batches (<= FUSED_MAX_NQ queries) take finalize_fused_kernel below instead: several workgroups per query.
// Shapes <NT threads, CAPK candidates>: <512, 8192> is the general one (two workgroups per CU: 64 KB of keys each).  The
// sharded search asks for SHORT lists of MANY queries (8 ranks: 4096 queries x k = 128, ~400 candidates each), where a
// workgroup's time is a chain of dependent steps (loads, three histogram passes, re-score rounds, sort), not work: 33 us per
// query and only two chains in flight per CU - 0.26 ms of a rank's 0.68 ms search.  <128, 1024> and <256, 2048> keep 8 / 4
// workgroups per CU in flight (16 waves either way); a query with more candidates than CAPK goes to the exact fix-up scan
// (the host picks a shape with twice the expected count, 10 sigma of the threshold estimate).
constexpr int FUSED_MAX_NQ = 128;
// Candidate input: block q of `cand` (cstride keys) = nseg segments of seg_cap slots, slot-major (slot s of segment g at
// s * nseg + g) [+ an overflow block at CAND_CAP when the streaming pass produced it]; segcnt[q][nseg] = hits each segment
// saw (may exceed seg_cap: the excess went to the overflow block, ocnt[q] entries).  The generic GEMM pass writes one
// segment (nseg = 1, seg_cap = CAND_CAP, no overflow).
// BO / BP: the boost and its arguments (boost, weight, boost_max) - NoElig and none in the kernel every search without
// boosts launches, Boosted in the boosted searches.  (The module's LDS lowering numbers the kernels that reach LDS variables
// through a call in NAME order and each kernel loads its number as a constant: `Boosted` sorts behind `NoElig`, so the
// boosted instantiations take numbers after this kernel's and leave its constant alone.)
template <int NT, int CAPK, class BO = NoElig, class... BP>
__global__ __launch_bounds__(NT, NT == 512 ? 2 : 4) void finalize_mixed_kernel(const unsigned long long* cand, long long cstride,
                                                                       const int* segcnt, int nseg, int seg_cap, const int* ocnt,
                                                                       int k, long long nrows, const float* tau,
                                                                       const float* max_norm, const float* X, long long ldx,
                                                                       int d, const float* Q, long long ldq, int* fail,
                                                                       float* outD, long long* outI, long long pos_offset,
                                                                       BP... bp) {
    const BO bo{bp...};
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];      // [CAPK] then qv[d]
    float* qv = reinterpret_cast<float*>(keys + CAPK);
    __shared__ int hist[2048];
    __shared__ int scratch[NT + 2];
    __shared__ float red[16];
    __shared__ int m_sh;
    __shared__ int seg_n[256], maxn_sh, fill_sh;
    constexpr bool GENERAL = CAPK == CAND_CAP;                // threads read the slot-major candidate area directly
    constexpr int NW = NT / 64;
    constexpr int PER = CAPK / NT;                            // candidate keys per thread
    constexpr int OVP = GENERAL ? 2048 / NT : 0;              // + overflow keys per thread (general shape: up to 2048 per query)
    static_assert(!GENERAL || NT == 512, "the general shape is 512 threads");
    const int q = blockIdx.x, nq = gridDim.x, tid = threadIdx.x;
    const int need = (int)(nrows < k ? nrows : k);
    if (tid == 0) { maxn_sh = 0; fill_sh = 0; m_sh = 0; }
    const int oc = ocnt[q];
    const int c = segment_counts<NT>(segcnt + (long long)q * nseg, nseg, seg_cap, oc, need, CAPK, seg_n,
                                     GENERAL ? nullptr : &maxn_sh);
    if (c < 0) { give_up(fail, q, nq); return; }
    const unsigned long long* blk = cand + (long long)q * cstride;
    unsigned long long mine[PER + OVP];
    if constexpr (GENERAL) {
        // the candidates stay where the pass put them: thread <- slots tid + NT j of the segment area
#pragma unroll
        for (int j = 0; j < PER; ++j) mine[j] = slot_valid(tid + NT * j, nseg, seg_cap, seg_n) ? blk[tid + NT * j] : 0ull;
#pragma unroll
        for (int j = 0; j < OVP; ++j) mine[PER + j] = (tid + NT * j < oc) ? blk[CAND_CAP + tid + NT * j] : 0ull;
    } else {
        // short lists: the occupied prefix of the slot-major area (slots below the fullest segment's count) and the overflow
        // block are compacted through LDS, then (behind query_eps' barrier) dealt to the threads' registers
        const int lim = maxn_sh * nseg;
        for (int s_ = tid; s_ < lim; s_ += NT)
            if (slot_valid(s_, nseg, seg_cap, seg_n)) keys[atomicAdd(&fill_sh, 1)] = blk[s_];
        for (int i = tid; i < oc; i += NT) keys[atomicAdd(&fill_sh, 1)] = blk[CAND_CAP + i];
    }
    const float eps = fin_eps(query_eps<NT>(Q + (long long)q * ldq, d, qv, red, max_norm), d, q, bo);
    if constexpr (!GENERAL) {
#pragma unroll
        for (int j = 0; j < PER; ++j) mine[j] = (tid + NT * j < c) ? keys[tid + NT * j] : 0ull;
        __syncthreads();                                      // keys[] is reused for the survivors
    }
    if (!(eps < INFINITY)) { give_up(fail, q, nq); return; }  // NaN / inf norms: exact path (block-uniform)
    if (need == 0) {
        write_result(keys, 0, k, q, outD, outI, pos_offset);
        return;
    }
    // a_k = need-th largest approximate score (orderable 32-bit image); always found: c >= need
    const uint32_t a_k = select_prefix_desc<NT, 3>(hist, scratch, need, [&](auto count_key) {
#pragma unroll
        for (int j = 0; j < PER + OVP; ++j) count_key(mine[j]);
    });
    // prune: a row with approx < a_k - 2 eps has exact < a_k - eps <= exact of each of the k best-by-approx rows
    const float cut = f32_from_orderable(a_k) - 2.f * eps;
#pragma unroll
    for (int j = 0; j < PER + OVP; ++j)
        if (mine[j] != 0ull && key_score(mine[j]) >= cut) keys[atomicAdd(&m_sh, 1)] = mine[j];
    __syncthreads();
    const int m = m_sh;                                       // need <= m <= c
    // 8 rows in flight per wave, two workgroups per CU (<= 128 VGPRs): with 16 in flight the kernel needed 169 and ran one
    // workgroup per CU, its select and sort phases - barriers and LDS latency - covered by nothing
    rescore_keys<NW, 8>(keys, m, X, ldx, qv, d >> 2, fin_term(bo, q));
    // (8192 keys of LDS: the run sort's source and destination both fit)
    const unsigned long long* sorted = sort_keys_desc<NT>(keys, keys + (m <= 1024 ? 1024 : 2048), m, 0);
    if (!certify_or_fail(sorted, need, (long long)c >= nrows, tau[q] + eps, fail, q, nq)) return;
    write_result(sorted, m, k, q, outD, outI, pos_offset);
}

// Small batches (<= FUSED_MAX_NQ queries), round 3: select -> prune -> re-score -> sort -> certificate in ONE launch of
// gridDim.x workgroups per query (the three kernels above cost 38 us at one query: 12.5 + 8 + 17, each of the small ones
// mostly launch-to-drain latency; they are gone).  Every workgroup of a query repeats the select + prune on the query's candidates (the same
// deterministic result in each: redundant, but in parallel), re-scores the survivors whose corpus position falls to it
// (pos % gridDim.x: a share that does not depend on the order in which a block's threads compacted the survivors), appends
// the exact keys to the query's list in the workspace, and takes a ticket; the workgroup that draws the LAST ticket sorts
// the list, certifies and writes the result.  Re-score, sort and certificate are finalize_mixed_kernel's: the same helpers.
#define AMDREC_FUSED_KERNEL finalize_fused_kernel
#define AMDREC_FUSED_PARAMS
#define AMDREC_FUSED_BOOST
#define AMDREC_FUSED_EPS(e) e
#define AMDREC_FUSED_TERM
#include "search_finalize_fused.hpp"
#undef AMDREC_FUSED_KERNEL
#undef AMDREC_FUSED_PARAMS
#undef AMDREC_FUSED_BOOST
#undef AMDREC_FUSED_EPS
#undef AMDREC_FUSED_TERM
// ... and its boosted sibling: fin_eps where eps is formed, fin_term in the re-score.  The name sorts behind every kernel
// the module already had (search_finalize_fused.hpp says why that matters).
#define AMDREC_FUSED_KERNEL finalize_fused_boosted_kernel
#define AMDREC_FUSED_PARAMS , const float* boost, const float* weight, float boost_max
#define AMDREC_FUSED_BOOST const Boosted bo{boost, weight, boost_max};
#define AMDREC_FUSED_EPS(e) fin_eps(e, d, q, bo)
#define AMDREC_FUSED_TERM , fin_term(bo, q)
#include "search_finalize_fused.hpp"
#undef AMDREC_FUSED_KERNEL
#undef AMDREC_FUSED_PARAMS
#undef AMDREC_FUSED_BOOST
#undef AMDREC_FUSED_EPS
#undef AMDREC_FUSED_TERM

__global__ void fill_f32_kernel(float* p, long long n, float v) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- plan ---------------------------------------------------------------------------
struct SearchPlan {
    long long n_sample;      // sample rows (multiple of SAMPLE_G), 0 => no sampling (tau = -inf)
    long long gstride;       // rows between sample blocks
    int rank;                // r
    int nslices;             // fix-up slices
    long long target;        // expected candidates per query (0: every row is a candidate)
    float *tau, *sample;     // the workspace: make_plan cuts it
    int *cnt, *ocnt, *ticket, *fcount, *fticket, *fail, *segcnt;   // cnt .. fail are cleared together: clear_bytes from cnt
    unsigned long long *cand, *fix, *exact;
    uint16_t* q16; size_t bytes, clear_bytes;
};

// dim16 > 0: the mixed-precision search, which also keeps a bf16 copy of the queries.  base: the workspace to cut, or nullptr to size it
static SearchPlan make_plan(long long nq, long long nrows, int k, int dim16, void* base) {
    SearchPlan pl;
    long long nt = (nrows + SAMPLE_G - 1) / SAMPLE_G;
    // expected candidates per query: far enough above k that an unlucky sample cannot undershoot it (the estimate's
    // sigma is ~target/8: k = 500 -> 1400 = k + 5.1 sigma), small enough that the finalize sort stays at 2048 keys for
    // k = 500.  Round 2 gave every k at least k + 900 - for the SHORT per-shard lists of the sharded search (128 of 500 at 8
    // ranks) that is 7 sigma and, on a shard an eighth the size, 8x the hit density of the single-GPU pass.  Now, for
    // batches whose corpus pass is compute-side bound (>= 256 queries; a small batch is HBM-bound and pays more for a larger
    // sample than its candidates cost): between the 5.1-sigma floor max(2.8 k, k + 256) and k + 900, the value that balances
    // the sample (rows ~ 64 nrows / target) against the per-hit work of the pass (~ target): ~0.6 sqrt(nrows), fitted to
    // same-box runs at 125k-row shards and 1M rows (profiles/r03_shard_search_target.log: per-rank search at the 8-rank
    // shape 0.766 -> 0.660 ms, k = 500 at 1M unchanged).
    long long t5 = k + 900ll;
    if (nq >= 256) {
        long long lo = (28ll * k + 9) / 10;
        if (lo < k + 256ll) lo = k + 256ll;
        long long opt = (long long)(0.6 * sqrt((double)(nrows > 0 ? nrows : 1)));
        if (opt < lo) opt = lo;
        if (opt < t5) t5 = opt;
    }
    long long target = (2ll * k > t5) ? 2ll * k : t5;
    pl.target = nrows <= CAND_CAP ? 0 : target;
    if (nrows <= CAND_CAP) {
        pl.n_sample = 0;                  // every row becomes a candidate
        pl.gstride = SAMPLE_G;
        pl.rank = 0;
    } else {
        long long n = (SAMPLE_RANK * nrows + target - 1) / target;
        long long st = (n + SAMPLE_G - 1) / SAMPLE_G;       // sample tiles
        if (st < 1) st = 1;
        if (st > nt) st = nt;
        long long stride = nt / st;
        pl.gstride = stride * SAMPLE_G;
        pl.n_sample = st * SAMPLE_G;
        pl.rank = SAMPLE_RANK;
    }
    int ns = CAND_CAP / (k > 0 ? k : 1);
    pl.nslices = ns < 1 ? 1 : (ns > 16 ? 16 : ns);
    Carver c(base);
    pl.tau = c.take<float>(nq);
    const size_t m = c.bytes();
    pl.cnt = c.take<int>(nq);
    pl.ocnt = c.take<int>(nq);
    pl.ticket = c.take<int>(nq);                        // fix-up: slices finished per query
    pl.fcount = c.take<int>(nq);                        // fused finalize (small batches): exact keys appended,
    pl.fticket = c.take<int>(nq);                       // blocks finished per query
    pl.fail = c.take<int>(nq + 1);
    pl.clear_bytes = c.bytes_since(m);
    pl.segcnt = c.take<int>((size_t)(dim16 ? nq : 0) * 256);                     // streaming pass: hits per (query, segment)
    pl.cand = c.take<unsigned long long>((size_t)nq * CAND_CAP * (dim16 ? 2 : 1));   // mixed: + overflow block
    pl.sample = c.take<float>((size_t)nq * (size_t)pl.n_sample);
    pl.fix = c.take<unsigned long long>((size_t)nq * pl.nslices * k);
    pl.q16 = c.take<uint16_t>((size_t)nq * (size_t)dim16);
    pl.exact = c.take<unsigned long long>((size_t)(dim16 && nq <= FUSED_MAX_NQ ? nq : 0) * CAND_CAP);   // fused finalize: re-scored keys
    pl.bytes = c.bytes();
    return pl;
}

// X / Q / ldx / ldq / d are in staged floats: for a BF16 shape the bf16 matrices viewed as float matrices of
// half the columns (d_alg = the un-halved dimension, for the profiling hook's FLOP count)
template <class S, class EL = NoElig>
static hipError_t run_passes(const float* X, long long ldx, long long nrows, int d, const float* Q, long long ldq,
                             int nq, const SearchPlan& pl, hipStream_t st, int d_alg = 0,
                             bool filter = true, long long cand_stride = CAND_CAP, EL el = EL{}) {
    using Store = std::conditional_t<EL::on || EL::boosted, EpiStoreScoresT<EL>, EpiStoreScores>;
    using Filter = std::conditional_t<EL::on || EL::boosted, EpiFilterT<EL>, EpiFilter>;
    DenseRows lq{Q, nq, (int)ldq, d, 30, 1ll << 30};
    if (pl.n_sample > 0) {
        int gshift = 8;   // SAMPLE_G == 256
        DenseRows lps{X, nrows, (int)ldx, d, gshift, pl.gstride};
        Store es{};
        static_cast<EpiStoreScoresT<EL>&>(es) = EpiStoreScoresT<EL>{pl.sample, pl.n_sample, nq, pl.n_sample, lps, el};
        hipError_t e = launch_gemm<S, false>(lps, lq, es, d, pl.n_sample, nq, st, d_alg);
        if (e != hipSuccess) return e;
        ProfScope prof("search_threshold", 0.0, 4.0 * (double)nq * (double)pl.n_sample, st);
        hipLaunchKernelGGL(sample_threshold_kernel, dim3(nq), dim3(THR_NT), 0, st, pl.sample, pl.n_sample, pl.n_sample,
                           pl.rank, pl.tau);
    } else {
        hipLaunchKernelGGL(fill_f32_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, pl.tau, (long long)nq,
                           -INFINITY);
    }
    if (!filter) return hipGetLastError();
    DenseRows lp{X, nrows, (int)ldx, d, 30, 1ll << 30};
    Filter ef{};
    static_cast<EpiFilterT<EL>&>(ef) = EpiFilterT<EL>{pl.tau, pl.cand, pl.cnt, CAND_CAP, nq, nrows, cand_stride, el};
    return launch_gemm<S, false>(lp, lq, ef, d, nrows, nq, st, d_alg);
}

// corpus tile 256 rows x query tile 128 / 64 / 32 (4 waves each): f(Shape<...>{})
template <bool BF16, class F>
static hipError_t dispatch_query_tile(long long nq, F&& f) {
    if (nq > 64) return f(Shape<2, 2, 4, 2, false, BF16>{});
    if (nq > 32) return f(Shape<4, 1, 2, 2, false, BF16>{});
    return f(Shape<4, 1, 2, 1, false, BF16>{});
}

// the streaming kernels' K-steps per row for the dims they are instantiated for (32 / 64 / 128 / 256): f(integral_constant<int, KS>{})
template <class F>
static hipError_t dispatch_ks(int dim, F&& f) {
    if (dim == 256) return f(std::integral_constant<int, 16>{});
    if (dim == 128) return f(std::integral_constant<int, 8>{});
    if (dim == 64) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 2>{});
}

}  // namespace amdrec

using namespace amdrec;

static int topk_merge_impl(const float* scores, const int32_t* pos, int n_lists, int list_k, int64_t list_stride_bytes,
                           int64_t q0, int64_t nq, int k, float* out_scores, int64_t* out_pos, int32_t* n_inexact,
                           void* stream) {
    REQUIRE(n_lists >= 1 && list_k >= 1 && k >= 1 && (long long)n_lists * list_k <= 16384 && k <= 16384,
            "n_lists*list_k and k must be in [1,16384]");
    REQUIRE(list_stride_bytes % 4 == 0 && q0 >= 0, "bad stride/offset");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(scores && pos && out_scores && out_pos, "null pointer");
    int P = 2;
    while (P < n_lists * list_k) P <<= 1;
    static PerDeviceOnce attr_done;
    if (attr_done.pending()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(topk_merge_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 8));
        attr_done.mark();
    }
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)nq), dim3(512), (size_t)P * 8,
                       reinterpret_cast<hipStream_t>(stream), (const char*)scores, (const char*)pos, n_lists, list_k,
                       (long long)list_stride_bytes, (long long)q0, k, out_scores, (long long*)out_pos, (int*)n_inexact);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_topk_merge(const float* scores, const int32_t* pos, int n_lists, int64_t list_stride_bytes,
                                 int64_t q0, int64_t nq, int k, float* out_scores, int64_t* out_pos,
                                 void* stream) {
    return topk_merge_impl(scores, pos, n_lists, k, list_stride_bytes, q0, nq, k, out_scores, out_pos, nullptr, stream);
}

extern "C" int amdrec_topk_merge_partial(const float* scores, const int32_t* pos, int n_lists, int list_k,
                                         int64_t list_stride_bytes, int64_t q0, int64_t nq, int k, float* out_scores,
                                         int64_t* out_pos, int32_t* n_inexact, void* stream) {
    REQUIRE(n_inexact != nullptr, "n_inexact is null");
    return topk_merge_impl(scores, pos, n_lists, list_k, list_stride_bytes, q0, nq, k, out_scores, out_pos, n_inexact,
                           stream);
}

// both flat-search entries' argument checks (mixed: + the corpus's bf16 shadow and row norms); nq == 0 ends them early
static int search_check(bool mixed, const float* corpus, int64_t nrows, int64_t ld_corpus, int dim, const uint16_t* corpus_bf16,
                        int64_t ld_bf16, const float* max_norm, const float* queries, int64_t nq, int64_t ld_queries, int k,
                        const float* out_scores, const int64_t* out_pos) {
    const int mult = mixed ? 8 : 4;
    REQUIRE(k >= 1 && k <= KMAX, "k=%d outside [1,%d]", k, KMAX);
    REQUIRE(dim >= mult && dim % mult == 0 && dim <= 2048, "dim=%d must be a multiple of %d in [%d,2048]", dim, mult, mult);
    REQUIRE(nrows >= 0 && nrows < (1ll << 31) - 1024, "nrows out of range");
    REQUIRE(nq >= 0 && nq < (1ll << 24), "nq out of range");
    if (nq == 0) return AMDREC_OK;
    REQUIRE((nrows == 0 || (ld_corpus >= dim && ld_corpus % 4 == 0 &&
                            (!mixed || (ld_bf16 >= dim && ld_bf16 % 8 == 0 && ld_bf16 < (1 << 20))))) &&
                ld_queries >= dim && ld_queries % 4 == 0,
            "%s", mixed ? "leading dimensions must be >= dim; fp32 multiples of 4, bf16 multiples of 8"
                        : "leading dimensions must be >= dim and multiples of 4");
    REQUIRE((corpus && (!mixed || corpus_bf16)) || nrows == 0, "corpus is null");
    REQUIRE(queries && out_scores && out_pos && (!mixed || max_norm), "null pointer");
    REQUIRE(((uintptr_t)corpus % 16) == 0 && ((uintptr_t)corpus_bf16 % 16) == 0 && ((uintptr_t)queries % 16) == 0,
            "corpus/queries must be 16-byte aligned");
    return AMDREC_OK;
}

// every finalize / fix-up kernel's dynamic LDS limit, once per device
static int set_lds_limits() {
    static PerDeviceOnce attr_done;
    if (!attr_done.pending()) return AMDREC_OK;
    const struct { const void* kernel; int bytes; } limits[] = {
        {reinterpret_cast<const void*>(finalize_kernel), CAND_CAP * 8},
        {reinterpret_cast<const void*>(finalize_mixed_kernel<512, CAND_CAP>), CAND_CAP * 8 + 2048 * 4},
        {reinterpret_cast<const void*>(finalize_fused_kernel), CAND_CAP * 8 + 2048 * 4},
        {reinterpret_cast<const void*>(ScanKernels<NoElig>::fixup()), CAND_CAP * 8},
        {reinterpret_cast<const void*>(ScanKernels<Elig>::fixup()), CAND_CAP * 8},
        {reinterpret_cast<const void*>(ScanKernels<Boosted>::fixup()), CAND_CAP * 8},
        {reinterpret_cast<const void*>(finalize_mixed_kernel<512, CAND_CAP, AMDREC_BOOST_FIN>), CAND_CAP * 8 + 2048 * 4},
        {reinterpret_cast<const void*>(finalize_fused_boosted_kernel), CAND_CAP * 8 + 2048 * 4}};
    for (const auto& l : limits) HIP_TRY(hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, l.bytes));
    attr_done.mark();
    return AMDREC_OK;
}

// the exact re-scan of the queries that the finalize kernel could not certify, and their count for the caller
template <class EL = NoElig>
static int launch_fixup(const float* corpus, int64_t ld_corpus, int64_t nrows, int dim, const float* queries, int64_t nq,
                        int64_t ld_queries, int k, const SearchPlan& pl, float* out_scores, int64_t* out_pos, int64_t pos_offset,
                        int* n_fixup, hipStream_t st, EL el = EL{}) {
    launch_with(el, ScanKernels<EL>::fixup(), dim3((unsigned)(pl.nslices * (nq < FIX_GRID_Q ? nq : FIX_GRID_Q))), dim3(512),
                (size_t)CAND_CAP * 8, st, corpus, (long long)ld_corpus, (long long)nrows, dim, queries, (long long)ld_queries,
                (const int*)pl.fail, (int)nq, k, pl.nslices, pl.fix, pl.ticket, out_scores, (long long*)out_pos,
                (long long)pos_offset);
    HIP_TRY(hipGetLastError());
    if (n_fixup) HIP_TRY(hipMemcpyAsync(n_fixup, pl.fail + nq, sizeof(int), hipMemcpyDeviceToDevice, st));
    return AMDREC_OK;
}

extern "C" int amdrec_flat_search_workspace(int64_t nq, int64_t nrows, int k, size_t* bytes) {
    REQUIRE(bytes != nullptr, "bytes is null");
    REQUIRE(nq >= 0 && nrows >= 0, "negative size");
    REQUIRE(k >= 1 && k <= KMAX, "k=%d outside [1,%d]", k, KMAX);
    *bytes = make_plan(nq, nrows, k, 0, nullptr).bytes;
    return AMDREC_OK;
}

// the eligibility pointers of the *_eligible entries: all three are required (checked with the other arguments, before
// the first HIP call)
static int elig_check(const uint64_t* tags, const uint64_t* require_all, const uint64_t* require_any, int64_t nrows) {
    REQUIRE(tags || nrows == 0, "tags is null");
    REQUIRE(require_all && require_any, "require_all / require_any is null");
    // (tags: the streaming pass reads the eight tags of a row group with one 64-byte scalar load)
    REQUIRE(((uintptr_t)tags % 64) == 0 && ((uintptr_t)require_all % 8) == 0 && ((uintptr_t)require_any % 8) == 0,
            "tags must be 64-byte aligned, require_all / require_any 8-byte aligned");
    return AMDREC_OK;
}
static int elig_check(NoElig, int64_t) { return AMDREC_OK; }
static int elig_check(Elig el, int64_t nrows) { return elig_check(el.tags, el.all, el.any, nrows); }
// ... and the boost arguments of the *_boosted entries: both pointers are required
static int elig_check(Boosted bo, int64_t nrows) {
    REQUIRE(bo.boost || nrows == 0, "boost is null");
    REQUIRE(bo.weight, "weight is null");
    // (boost: the streaming passes read the 32 boosts of a row quarter with two 64-byte scalar loads)
    REQUIRE(((uintptr_t)bo.boost % 64) == 0 && ((uintptr_t)bo.weight % 4) == 0,
            "boost must be 64-byte aligned, weight 4-byte aligned");
    REQUIRE(bo.boost_max >= 0.f && bo.boost_max < INFINITY, "boost_max must be a finite bound of max |boost|");
    return AMDREC_OK;
}

// finalize_mixed_kernel with the boost's arguments after the ones every instantiation takes
template <int NT, int CAPK, class... A>
static void launch_finalize_mixed(NoElig, dim3 grid, size_t lds, hipStream_t st, A... a) {
    hipLaunchKernelGGL((finalize_mixed_kernel<NT, CAPK>), grid, dim3(NT), lds, st, a...);
}
template <int NT, int CAPK, class... A>
static void launch_finalize_mixed(Elig, dim3 grid, size_t lds, hipStream_t st, A... a) {
    hipLaunchKernelGGL((finalize_mixed_kernel<NT, CAPK>), grid, dim3(NT), lds, st, a...);
}
template <int NT, int CAPK, class... A>
static void launch_finalize_mixed(Boosted bo, dim3 grid, size_t lds, hipStream_t st, A... a) {
    hipLaunchKernelGGL((finalize_mixed_kernel<NT, CAPK, AMDREC_BOOST_FIN>), grid, dim3(NT), lds, st, a..., bo.boost, bo.weight,
                       bo.boost_max);
}

template <class EL>
static int flat_search_impl(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                            const float* queries, int64_t nq, int64_t ld_queries, int k,
                            int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                            size_t workspace_bytes, int* n_fixup, void* stream, EL el) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc = search_check(false, corpus, nrows, ld_corpus, dim, nullptr, 0, nullptr, queries, nq, ld_queries, k, out_scores, out_pos);
    if (rc || nq == 0) return rc;
    if ((rc = elig_check(el, nrows))) return rc;
    const SearchPlan pl = make_plan(nq, nrows, k, 0, workspace);
    if ((rc = require_workspace(workspace, workspace_bytes, pl.bytes, 256))) return rc;
    HIP_TRY(hipMemsetAsync(pl.cnt, 0, pl.clear_bytes, st));

    hipError_t e = nrows <= 0 ? hipSuccess : dispatch_query_tile<false>(nq, [&](auto shape) {
        return run_passes<decltype(shape), EL>(corpus, ld_corpus, nrows, dim, queries, ld_queries, (int)nq, pl, st, 0, true,
                                               CAND_CAP, el);
    });
    HIP_TRY(e);
    if ((rc = set_lds_limits())) return rc;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)nq), dim3(512), CAND_CAP * 8, st, pl.cand, pl.cnt, CAND_CAP, k,
                       (long long)nrows, pl.fail, out_scores, (long long*)out_pos, (long long)pos_offset);
    return launch_fixup(corpus, ld_corpus, nrows, dim, queries, nq, ld_queries, k, pl, out_scores, out_pos, pos_offset, n_fixup, st,
                        el);
}

extern "C" int amdrec_flat_search(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                  const float* queries, int64_t nq, int64_t ld_queries, int k,
                                  int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                  size_t workspace_bytes, int* n_fixup, void* stream) {
    return flat_search_impl(corpus, nrows, ld_corpus, dim, queries, nq, ld_queries, k, pos_offset, out_scores, out_pos, workspace,
                            workspace_bytes, n_fixup, stream, NoElig{});
}

extern "C" int amdrec_flat_search_eligible(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                           const float* queries, int64_t nq, int64_t ld_queries, int k,
                                           int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                           size_t workspace_bytes, int* n_fixup, void* stream, const uint64_t* tags,
                                           const uint64_t* require_all, const uint64_t* require_any) {
    return flat_search_impl(corpus, nrows, ld_corpus, dim, queries, nq, ld_queries, k, pos_offset, out_scores, out_pos, workspace,
                            workspace_bytes, n_fixup, stream, Elig{tags, require_all, require_any});
}

extern "C" int amdrec_bf16_rows(const float* x, int64_t rows, int64_t ld, int dim, uint16_t* out, int64_t ld_out,
                                float* max_norm, void* stream) {
    REQUIRE(dim >= 4 && dim % 4 == 0 && dim <= 2048, "dim=%d must be a multiple of 4 in [4,2048]", dim);
    if (rows <= 0) return AMDREC_OK;
    REQUIRE(x && out, "null pointer");
    REQUIRE(ld >= dim && ld % 4 == 0 && ld_out >= dim && ld_out % 4 == 0, "leading dimensions must be >= dim and multiples of 4");
    REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 8) == 0, "x must be 16-byte and out 8-byte aligned");
    hipLaunchKernelGGL(bf16_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, (long long)rows, (long long)ld, dim, out,
                       (long long)ld_out, max_norm, (int*)nullptr, 0ll);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_flat_search_mixed_workspace(int64_t nq, int64_t nrows, int k, int dim, size_t* bytes) {
    REQUIRE(bytes != nullptr, "bytes is null");
    REQUIRE(nq >= 0 && nrows >= 0, "negative size");
    REQUIRE(k >= 1 && k <= KMAX, "k=%d outside [1,%d]", k, KMAX);
    REQUIRE(dim >= 8 && dim % 8 == 0 && dim <= 2048, "dim=%d must be a multiple of 8 in [8,2048]", dim);
    *bytes = make_plan(nq, nrows, k, dim, nullptr).bytes;
    return AMDREC_OK;
}

template <class EL>
static int flat_search_mixed_impl(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                  const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                                  const float* queries, int64_t nq, int64_t ld_queries, int k,
                                  int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                  size_t workspace_bytes, int* n_fixup, void* stream, EL el) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc = search_check(true, corpus, nrows, ld_corpus, dim, corpus_bf16, ld_bf16, max_norm, queries, nq, ld_queries, k,
                          out_scores, out_pos);
    if (rc || nq == 0) return rc;
    if ((rc = elig_check(el, nrows))) return rc;
    const SearchPlan pl = make_plan(nq, nrows, k, dim, workspace);
    if ((rc = require_workspace(workspace, workspace_bytes, pl.bytes, 256))) return rc;
    // cnt .. fail are cleared by the query-conversion kernel below (no separate fill launch: a launch costs ~5 us, a
    // 32-query search 170)
    const long long n_zero = (long long)(pl.clear_bytes / 4);
    if (nrows <= 0) HIP_TRY(hipMemsetAsync(pl.cnt, 0, pl.clear_bytes, st));
    constexpr long long CSTRIDE = CAND_STRIDE;
    // corpus pass: the streaming kernel for the power-of-two dims it is instantiated for, else the generic tiles
    const bool streaming = nrows > 0 && (dim == 32 || dim == 64 || dim == 128 || dim == 256);
    const int nseg = streaming ? scan_segments(nrows, nq) : 1;
    const int seg_cap = CAND_CAP / nseg;
    const int* segcnt = streaming ? pl.segcnt : pl.cnt;

    if (streaming && pl.n_sample > 0) {
        // conversion + sample in ONE launch (group maxima only), tau from the maxima: inside the corpus pass for <= 8
        // queries (no threshold launch), one wave per query otherwise
        const SamplePlan sp = sample_plan(nrows, pl.n_sample);
        REQUIRE(sp.cols <= pl.n_sample, "internal: sample maxima do not fit their workspace");
        const bool tau_in_scan = nq <= 8;
        hipError_t e = dispatch_ks(dim, [&](auto ks_tag) -> hipError_t {
            constexpr int KS = decltype(ks_tag)::value;
            hipError_t e2 = launch_sample<KS, EL>(corpus_bf16, ld_bf16, sp, queries, ld_queries, (int)nq, pl.q16, pl.sample, pl.cnt,
                                                  n_zero, st, el);
            if (e2 != hipSuccess) return e2;
            if (!tau_in_scan) {
                ProfScope prof("search_threshold", 0.0, 4.0 * (double)nq * (double)sp.cols, st);
                hipLaunchKernelGGL(tau_from_maxima_kernel, dim3((unsigned)((nq + 7) / 8)), dim3(512), 0, st, pl.sample,
                                   sp.cols, sp.cols, pl.rank, (int)nq, pl.tau);
            }
            return launch_scan<KS, EL>(corpus_bf16, ld_bf16, nrows, pl.q16, (int)nq, pl.tau, pl.cand, pl.segcnt, pl.ocnt, st,
                                       tau_in_scan ? pl.sample : nullptr, sp.cols, sp.cols, pl.rank, el);
        });
        HIP_TRY(e);
    } else if (nrows > 0) {
        hipLaunchKernelGGL(bf16_rows_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, queries, (long long)nq,
                           (long long)ld_queries, dim, pl.q16, (long long)dim, (float*)nullptr, pl.cnt, n_zero);
        // the bf16 matrices as float matrices of dim/2 columns (gemm_core.hpp, Shape::BF16)
        const float* X = reinterpret_cast<const float*>(corpus_bf16);
        const float* Q = reinterpret_cast<const float*>(pl.q16);
        const long long ldx = ld_bf16 / 2, ldq = dim / 2;
        const int dh = dim / 2;
        hipError_t e = dispatch_query_tile<true>(nq, [&](auto shape) {
            return run_passes<decltype(shape), EL>(X, ldx, nrows, dh, Q, ldq, (int)nq, pl, st, dim, !streaming, CSTRIDE, el);
        });
        HIP_TRY(e);
        if (streaming) {
            e = dispatch_ks(dim, [&](auto ks_tag) {
                return launch_scan<decltype(ks_tag)::value, EL>(corpus_bf16, ld_bf16, nrows, pl.q16, (int)nq, pl.tau, pl.cand,
                                                                pl.segcnt, pl.ocnt, st, nullptr, 0, 0, 0, el);
            });
            HIP_TRY(e);
        }
    }
    if ((rc = set_lds_limits())) return rc;
    {
        ProfScope prof(EL::boosted ? "search_finalize_mixed_boost" : "search_finalize_mixed", 0.0, 0.0, st);
        if (nq <= FUSED_MAX_NQ) {
            int slices = (int)(512 / nq);                           // ~512 workgroups in all: the chip once
            slices = slices < 1 ? 1 : (slices > 16 ? 16 : slices);
            if constexpr (EL::boosted)
                hipLaunchKernelGGL(finalize_fused_boosted_kernel, dim3((unsigned)slices, (unsigned)nq), dim3(512),
                                   (size_t)CAND_CAP * 8 + (size_t)dim * 4, st, pl.cand, CSTRIDE, segcnt, nseg, seg_cap, pl.ocnt,
                                   CAND_CAP, k, (long long)nrows, pl.tau, max_norm, corpus, (long long)ld_corpus, dim, queries,
                                   (long long)ld_queries, pl.fail, out_scores, (long long*)out_pos, (long long)pos_offset,
                                   pl.exact, pl.fcount, pl.fticket, el.boost, el.weight, el.boost_max);
            else
            hipLaunchKernelGGL(finalize_fused_kernel, dim3((unsigned)slices, (unsigned)nq), dim3(512), (size_t)CAND_CAP * 8 + (size_t)dim * 4, st, pl.cand, CSTRIDE,
                               segcnt, nseg, seg_cap, pl.ocnt, CAND_CAP, k, (long long)nrows, pl.tau, max_norm, corpus,
                               (long long)ld_corpus, dim, queries, (long long)ld_queries, pl.fail, out_scores,
                               (long long*)out_pos, (long long)pos_offset, pl.exact, pl.fcount, pl.fticket);
        } else {
            // one workgroup per query; short lists of many queries (the sharded search) on the small shapes: twice the
            // expected candidate count must fit (10 sigma of the threshold estimate; beyond it the query takes the fix-up scan)
#define AMDREC_FINALIZE(NT_, CAPK_)                                                                                          \
    launch_finalize_mixed<NT_, CAPK_>(el, dim3((unsigned)nq), (size_t)(CAPK_) * 8 + (size_t)dim * 4, st,                      \
                                      (const unsigned long long*)pl.cand, CSTRIDE, segcnt, nseg, seg_cap, (const int*)pl.ocnt, k, \
                                      (long long)nrows, (const float*)pl.tau, max_norm, corpus, (long long)ld_corpus, dim,     \
                                      queries, (long long)ld_queries, pl.fail, out_scores, (long long*)out_pos,                \
                                      (long long)pos_offset)
            if (pl.target > 0 && 2 * pl.target <= 1024 && dim <= 2048) AMDREC_FINALIZE(128, 1024);
            else if (pl.target > 0 && 2 * pl.target <= 2048 && dim <= 2048) AMDREC_FINALIZE(256, 2048);
            else AMDREC_FINALIZE(512, CAND_CAP);
#undef AMDREC_FINALIZE
        }
    }
    ProfScope prof_fix(tag_for<EL>("search_fixup", "search_fixup_elig", "search_fixup_boost"), 0.0, 0.0, st);
    return launch_fixup(corpus, ld_corpus, nrows, dim, queries, nq, ld_queries, k, pl, out_scores, out_pos, pos_offset, n_fixup, st,
                        el);
}

extern "C" int amdrec_flat_search_mixed(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                        const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                                        const float* queries, int64_t nq, int64_t ld_queries, int k,
                                        int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                        size_t workspace_bytes, int* n_fixup, void* stream) {
    return flat_search_mixed_impl(corpus, nrows, ld_corpus, dim, corpus_bf16, ld_bf16, max_norm, queries, nq, ld_queries, k,
                                  pos_offset, out_scores, out_pos, workspace, workspace_bytes, n_fixup, stream, NoElig{});
}

extern "C" int amdrec_flat_search_mixed_eligible(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                                 const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                                                 const float* queries, int64_t nq, int64_t ld_queries, int k,
                                                 int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                                 size_t workspace_bytes, int* n_fixup, void* stream, const uint64_t* tags,
                                                 const uint64_t* require_all, const uint64_t* require_any) {
    return flat_search_mixed_impl(corpus, nrows, ld_corpus, dim, corpus_bf16, ld_bf16, max_norm, queries, nq, ld_queries, k,
                                  pos_offset, out_scores, out_pos, workspace, workspace_bytes, n_fixup, stream,
                                  Elig{tags, require_all, require_any});
}

extern "C" int amdrec_flat_search_boosted(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                          const float* queries, int64_t nq, int64_t ld_queries, int k,
                                          int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                          size_t workspace_bytes, int* n_fixup, void* stream, const float* boost,
                                          const float* weight, float boost_max) {
    return flat_search_impl(corpus, nrows, ld_corpus, dim, queries, nq, ld_queries, k, pos_offset, out_scores, out_pos, workspace,
                            workspace_bytes, n_fixup, stream, Boosted{boost, weight, boost_max});
}

extern "C" int amdrec_flat_search_mixed_boosted(const float* corpus, int64_t nrows, int64_t ld_corpus, int dim,
                                                const uint16_t* corpus_bf16, int64_t ld_bf16, const float* max_norm,
                                                const float* queries, int64_t nq, int64_t ld_queries, int k,
                                                int64_t pos_offset, float* out_scores, int64_t* out_pos, void* workspace,
                                                size_t workspace_bytes, int* n_fixup, void* stream, const float* boost,
                                                const float* weight, float boost_max) {
    return flat_search_mixed_impl(corpus, nrows, ld_corpus, dim, corpus_bf16, ld_bf16, max_norm, queries, nq, ld_queries, k,
                                  pos_offset, out_scores, out_pos, workspace, workspace_bytes, n_fixup, stream,
                                  Boosted{boost, weight, boost_max});
}
#undef AMDREC_BOOST_FIN
