// Per-request must-consider lists (behind FAISSIndex.search_device(..., include=) and AdRecommenderInference's
// include_ad_ids): the search ran as it is for k entries per query; this step scores the query's listed rows exactly and
// merges those that the result does not hold into it, evicting from the result's tail (amdrec/include.py has the rule).
//   include_merge : one workgroup of 512 per query.
//     1. the query goes to LDS; lane i of wave 0 takes list entry i (I <= 64): a position outside [0, n_rows), a position
//        that an earlier entry holds, or a row that fails the query's masks drops the entry.  The exclusion block is walked
//        by all threads, each of its entries against the (at most 64) listed rows' ids in LDS: a match drops the entry.
//     2. the survivors, compacted, are scored by rescore_keys (the searches' re-score chain; 8 rows in flight per wave: the
//        reads are random 1 KB rows, latency-bound); a NaN score leaves key 0.  bitonic_desc orders the 64 keys.
//     3. a second 64-entry list, (position + 1) << 8 | rank, ordered the same way: every result column finds its position
//        in it by ONE binary search (not k x I compares) and flags the list entry it met; what is not flagged is N, the
//        entries to inject, compacted in their order.
//     4. f + m - k of the result's filled columns that are not listed leave, from the tail: two prefix counts (filled
//        columns, unlisted filled columns) behind one barrier give each kept column its rank among the kept.
//     5. both lists are ordered by key, so an element's slot is its rank in its own list plus the elements of the other
//        list that precede it: one binary search each.  The kept columns are written as the search wrote them.
#include "common.hpp"
#include "topk_utils.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int IN_NT = 512;                        // threads per workgroup
constexpr int IN_ROUNDS = AMDREC_MAX_K / IN_NT;   // result columns per thread at most
constexpr int IN_MAX = AMDREC_MAX_INCLUDE;        // list entries per query at most: one wave's lanes
static_assert(IN_MAX == 64, "one list entry per lane of a wave");

// keys of `list`[0 .. n) (descending) that are greater than `key`
__device__ __forceinline__ int count_greater(const unsigned long long* list, int n, unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] > key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <class Term>
__global__ __launch_bounds__(IN_NT) void include_merge_kernel(
    const long long* pos, const float* scores, int k, const long long* incl, int I, long long ld_incl, const float* X,
    long long ldx, long long n_rows, int d, const float* Q, long long ldq, const long long* tags, const long long* req_all,
    const long long* req_any, const long long* excl, int E, long long ld_excl, const long long* ids, const float* boosts,
    const float* weights, long long* out_pos, float* out_scores, unsigned char* out_injected) {
    __shared__ __attribute__((aligned(16))) float qv[2048];
    __shared__ __attribute__((aligned(16))) unsigned long long rk[AMDREC_MAX_K];    // kept result keys, in rank order
    __shared__ __attribute__((aligned(16))) unsigned long long vkeys[IN_MAX];       // listed rows: (score, position), descending
    __shared__ __attribute__((aligned(16))) unsigned long long vpos[IN_MAX];        // (position + 1) << 8 | rank in vkeys, descending
    __shared__ __attribute__((aligned(16))) unsigned long long nkeys[IN_MAX];       // N: vkeys without those the result holds
    __shared__ long long lpos[IN_MAX], lid[IN_MAX];                                 // the list as given: positions, their ids
    __shared__ int dead[IN_MAX], in_result[IN_MAX];
    __shared__ int wave_total[2][IN_ROUNDS][IN_NT / 64];
    __shared__ int n_valid_sh, m_sh;
    const long long q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    // 1. query and list
    for (int i = tid; i < d; i += IN_NT) qv[i] = Q[q * ldq + i];
    if (tid < IN_MAX) {
        const long long p = tid < I ? incl[q * ld_incl + tid] : -1ll;
        const bool ok = p >= 0 && p < n_rows;
        lpos[tid] = ok ? p : -1ll;
        lid[tid] = ok ? (ids ? ids[p] : p) : -1ll;
        dead[tid] = 0;
        in_result[tid] = 0;
        vkeys[tid] = 0ull;
        vpos[tid] = 0ull;
    }
    __syncthreads();
    if (excl) {                                   // exclusion wins: an entry of the block that equals a listed row's id
        for (int e = tid; e < E; e += IN_NT) {
            const long long x = excl[q * ld_excl + e];
            if (x < 0) continue;
            for (int i = 0; i < I; ++i)
                if (lid[i] == x) dead[i] = 1;     // (several threads may write the same 1)
        }
        __syncthreads();
    }
    if (w == 0) {
        const long long p = lpos[lane];
        bool ok = p >= 0 && !dead[lane];
        for (int j = 0; j < lane; ++j) ok = ok && lpos[j] != p;      // the first occurrence stands
        if (ok && tags) {
            const unsigned long long t = (unsigned long long)tags[p], a = (unsigned long long)req_all[q],
                                     y = (unsigned long long)req_any[q];
            ok = (t & a) == a && (y == 0ull || (t & y) != 0ull);
        }
        const unsigned long long mk = __ballot(ok);
        if (ok) vkeys[__popcll(mk & ((1ull << lane) - 1ull))] = make_key(0.f, (uint32_t)p);
        if (lane == 0) n_valid_sh = __popcll(mk);
    }
    __syncthreads();

    // 2. exact scores, then order
    const int n_listed = n_valid_sh;
    if constexpr (Term::boosted) rescore_keys<IN_NT / 64, 8, Term>(vkeys, n_listed, X, ldx, qv, d >> 2, Term{boosts, weights[q]});
    else rescore_keys<IN_NT / 64, 8, Term>(vkeys, n_listed, X, ldx, qv, d >> 2);
    bitonic_desc(vkeys, IN_MAX);                  // NaN rows (key 0) go last; (ends behind a block barrier)

    // 3. which listed rows does the result hold already?
    if (tid < IN_MAX) {
        const unsigned long long key = vkeys[tid];
        vpos[tid] = key ? (((unsigned long long)key_pos(key) + 1ull) << 8) | (unsigned long long)tid : 0ull;
    }
    __syncthreads();
    bitonic_desc(vpos, IN_MAX);
    long long rp[IN_ROUNDS];
    float rs[IN_ROUNDS];
    bool filled[IN_ROUNDS], unlisted[IN_ROUNDS];
#pragma unroll
    for (int r = 0; r < IN_ROUNDS; ++r) {
        const int c = r * IN_NT + tid;
        const bool in = c < k;
        rp[r] = in ? pos[q * k + c] : -1ll;
        rs[r] = in ? scores[q * k + c] : 0.f;
        filled[r] = rp[r] >= 0;
        bool listed = false;
        if (filled[r]) {
            const unsigned long long want = (unsigned long long)rp[r] + 1ull;
            int lo = 0, hi = IN_MAX;              // first entry whose position part is <= want (descending list)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((vpos[mid] >> 8) > want) lo = mid + 1; else hi = mid;
            }
            if (lo < IN_MAX && (vpos[lo] >> 8) == want) {
                listed = true;
                in_result[(int)(vpos[lo] & 255ull)] = 1;
            }
        }
        unlisted[r] = filled[r] && !listed;
    }
    // the two prefix counts of step 4 ride behind the same barrier
    int filled_before[IN_ROUNDS], unlisted_before[IN_ROUNDS];
#pragma unroll
    for (int r = 0; r < IN_ROUNDS; ++r) {
        const unsigned long long mf = __ballot(filled[r]), mu = __ballot(unlisted[r]);
        const unsigned long long below = (1ull << lane) - 1ull;
        filled_before[r] = __popcll(mf & below);
        unlisted_before[r] = __popcll(mu & below);
        if (lane == 0) {
            wave_total[0][r][w] = __popcll(mf);
            wave_total[1][r][w] = __popcll(mu);
        }
    }
    __syncthreads();
    if (w == 0) {
        const unsigned long long key = vkeys[lane];
        const bool inject = key != 0ull && !in_result[lane];
        const unsigned long long mk = __ballot(inject);
        if (inject) nkeys[__popcll(mk & ((1ull << lane) - 1ull))] = key;
        if (lane == 0) m_sh = __popcll(mk);
    }
    int f = 0, n_unlisted = 0;
#pragma unroll
    for (int r = 0; r < IN_ROUNDS; ++r) {
        filled_before[r] += f;
        unlisted_before[r] += n_unlisted;
#pragma unroll
        for (int x = 0; x < IN_NT / 64; ++x) {
            const int tf = wave_total[0][r][x], tu = wave_total[1][r][x];
            if (x < w) { filled_before[r] += tf; unlisted_before[r] += tu; }
            f += tf;
            n_unlisted += tu;
        }
    }
    __syncthreads();

    // 4. evict from the tail
    const int m = m_sh;
    const int evict = max(0, f + m - k);          // <= n_unlisted: I <= k
    const int first_out = n_unlisted - evict;     // unlisted filled columns from this index on leave
    bool keep[IN_ROUNDS];
    int rank[IN_ROUNDS];
    unsigned long long rkey[IN_ROUNDS];
#pragma unroll
    for (int r = 0; r < IN_ROUNDS; ++r) {
        keep[r] = filled[r] && !(unlisted[r] && unlisted_before[r] >= first_out);
        rank[r] = filled_before[r] - max(0, unlisted_before[r] - first_out);
        rkey[r] = make_key(rs[r], (uint32_t)rp[r]);
        if (keep[r]) rk[rank[r]] = rkey[r];
    }
    const int n_kept = f - evict;
    __syncthreads();

    // 5. merge by rank
#pragma unroll
    for (int r = 0; r < IN_ROUNDS; ++r) {
        if (!keep[r]) continue;
        const int slot = rank[r] + count_greater(nkeys, m, rkey[r]);
        if (slot < k) {
            out_pos[q * k + slot] = rp[r];
            out_scores[q * k + slot] = rs[r];
            if (out_injected) out_injected[q * k + slot] = 0;
        }
    }
    if (tid < m) {
        const unsigned long long key = nkeys[tid];
        const int slot = tid + count_greater(rk, n_kept, key);
        if (slot < k) {
            out_pos[q * k + slot] = (long long)key_pos(key);
            out_scores[q * k + slot] = key_score(key);
            if (out_injected) out_injected[q * k + slot] = 1;
        }
    }
    for (int i = n_kept + m + tid; i < k; i += IN_NT) {
        out_pos[q * k + i] = -1ll;
        out_scores[q * k + i] = -INFINITY;
        if (out_injected) out_injected[q * k + i] = 0;
    }
}

}  // namespace amdrec

using namespace amdrec;

extern "C" int amdrec_include_merge(const int64_t* pos, const float* scores, int64_t nq, int k, const int64_t* include,
                                    int n_include, int64_t ld_include, const float* X, int64_t ldx, int64_t n_rows, int d,
                                    const float* Q, int64_t ldq, const int64_t* tags, const int64_t* require_all,
                                    const int64_t* require_any, const int64_t* exclude, int n_exclude, int64_t ld_exclude,
                                    const int64_t* ids, const float* boosts, const float* boost_w, int64_t* out_pos,
                                    float* out_scores, uint8_t* out_injected, void* stream) {
    REQUIRE(k >= 1 && k <= AMDREC_MAX_K, "k=%d out of range [1, %d]", k, AMDREC_MAX_K);
    REQUIRE(n_include >= 1 && n_include <= AMDREC_MAX_INCLUDE && n_include <= k,
            "n_include=%d out of range [1, min(k=%d, %d)]", n_include, k, AMDREC_MAX_INCLUDE);
    REQUIRE(ld_include >= n_include, "ld_include=%lld is smaller than n_include=%d", (long long)ld_include, n_include);
    REQUIRE(d >= 4 && d <= 2048 && d % 4 == 0, "d=%d: a multiple of 4 in [4, 2048]", d);
    REQUIRE(ldx >= d && ldx % 4 == 0, "ldx=%lld: a multiple of 4, at least d=%d", (long long)ldx, d);
    REQUIRE(ldq >= d, "ldq=%lld is smaller than d=%d", (long long)ldq, d);
    REQUIRE(n_rows >= 0 && n_rows <= 4294967295ll, "n_rows=%lld out of range [0, 2^32 - 1]", (long long)n_rows);
    REQUIRE((require_all == nullptr) == (tags == nullptr) && (require_any == nullptr) == (tags == nullptr),
            "tags, require_all and require_any go together (all three, or all NULL)");
    REQUIRE(exclude != nullptr || n_exclude == 0, "n_exclude=%d without an exclusion block", n_exclude);
    REQUIRE(exclude == nullptr || (n_exclude >= 1 && n_exclude < AMDREC_MAX_K), "n_exclude=%d out of range [1, %d]",
            n_exclude, AMDREC_MAX_K - 1);
    REQUIRE(exclude == nullptr || ld_exclude >= n_exclude, "ld_exclude=%lld is smaller than n_exclude=%d",
            (long long)ld_exclude, n_exclude);
    REQUIRE(ids == nullptr || exclude != nullptr, "ids without an exclusion block (they only serve the exclusion test)");
    REQUIRE((boosts == nullptr) == (boost_w == nullptr), "boosts and boost_w go together (both, or both NULL)");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq <= 2147483647ll, "nq=%lld: at most 2^31 - 1 queries per call", (long long)nq);
    REQUIRE(pos != nullptr && scores != nullptr, "null pointer: pos / scores");
    REQUIRE(include != nullptr, "null pointer: include");
    REQUIRE(X != nullptr || n_rows == 0, "null pointer: X");
    REQUIRE(Q != nullptr, "null pointer: Q");
    REQUIRE(out_pos != nullptr && out_scores != nullptr, "null pointer: out_pos / out_scores");
    REQUIRE(((uintptr_t)X & 15) == 0, "X must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("include_merge", 2.0 * (double)nq * n_include * d,
                   (double)nq * ((double)k * 25 + (double)n_include * (8 + 4.0 * d) + 4.0 * d + (double)n_exclude * 8), st);
    const dim3 grid((unsigned)nq), block(IN_NT);
    if (boosts)
        hipLaunchKernelGGL(include_merge_kernel<RowBoost>, grid, block, 0, st, (const long long*)pos, scores, k,
                           (const long long*)include, n_include, (long long)ld_include, X, (long long)ldx, (long long)n_rows,
                           d, Q, (long long)ldq, (const long long*)tags, (const long long*)require_all,
                           (const long long*)require_any, (const long long*)exclude, n_exclude, (long long)ld_exclude,
                           (const long long*)ids, boosts, boost_w, (long long*)out_pos, out_scores, out_injected);
    else
        hipLaunchKernelGGL(include_merge_kernel<NoTerm>, grid, block, 0, st, (const long long*)pos, scores, k,
                           (const long long*)include, n_include, (long long)ld_include, X, (long long)ldx, (long long)n_rows,
                           d, Q, (long long)ldq, (const long long*)tags, (const long long*)require_all,
                           (const long long*)require_any, (const long long*)exclude, n_exclude, (long long)ld_exclude,
                           (const long long*)ids, boosts, boost_w, (long long*)out_pos, out_scores, out_injected);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
