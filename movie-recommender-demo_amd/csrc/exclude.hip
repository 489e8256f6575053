// Per-request exclusion lists (behind FAISSIndex.search_device(..., exclude=) and AdRecommenderInference's exclude_ad_ids):
// the search ran unfiltered for kc = k + E candidates per query; this step drops every candidate whose key is in the
// query's exclusion list and closes the gaps, order kept.
//   exclude_compact : one workgroup of 512 per query.  The E list entries go to LDS as id + 1 (negative = padding = 0, the
//            smallest key), padded with zeros to a power of two, and are ordered with bitonic_desc (duplicates are fine
//            there; sort_desc_runs wants unique keys).  Thread t owns candidate columns t, t + 512, ...: a binary search
//            of the column's key in the sorted list decides whether it stays.  A column that is already unfilled (its
//            position, or its key where no position block travels along, is negative) is never matched and stays where it
//            is: behind every filled one, as the searches write them.  The output slot of a survivor is the number of
//            survivors in the columns before it: wave ballot + popcount of the lower lanes, wave totals of all (at most
//            four) rounds through LDS behind ONE barrier.  Slots past the last survivor get the caller's fill values.
#include "common.hpp"
#include "topk_utils.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int EX_NT = 512;                        // threads per workgroup
constexpr int EX_ROUNDS = AMDREC_MAX_K / EX_NT;   // candidate columns per thread at most

__global__ __launch_bounds__(EX_NT) void exclude_compact_kernel(
    const long long* keys, const float* scores, const long long* carry, int kc, const long long* excl, int E,
    long long ld_excl, int k, long long fill_key, float fill_score, long long fill_carry, long long* out_keys,
    float* out_scores, long long* out_carry) {
    __shared__ __attribute__((aligned(16))) unsigned long long list[AMDREC_MAX_K];
    __shared__ int wave_total[EX_ROUNDS][EX_NT / 64];
    const long long q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int P = 2;
    while (P < E) P <<= 1;
    const long long* eq = excl + q * ld_excl;
    for (int i = tid; i < P; i += EX_NT) {
        const long long id = i < E ? eq[i] : -1ll;
        list[i] = id >= 0 ? (unsigned long long)id + 1ull : 0ull;
    }
    __syncthreads();
    bitonic_desc(list, P);                        // (ends behind a block barrier)

    const long long* kq = keys + q * kc;
    long long key[EX_ROUNDS], car[EX_ROUNDS];
    float sc[EX_ROUNDS];
    bool keep[EX_ROUNDS];
    int before[EX_ROUNDS];                        // survivors in lower lanes of my wave, this round
#pragma unroll
    for (int r = 0; r < EX_ROUNDS; ++r) {
        const int c = r * EX_NT + tid;
        const bool in = c < kc;
        key[r] = in ? kq[c] : -1ll;
        sc[r] = in ? scores[q * kc + c] : 0.f;
        car[r] = in && carry ? carry[q * kc + c] : 0ll;
        const bool filled = (carry ? car[r] : key[r]) >= 0;
        bool hit = false;
        if (in && filled && key[r] >= 0) {
            const unsigned long long want = (unsigned long long)key[r] + 1ull;
            int lo = 0, hi = P;                   // first index whose entry is <= want (descending list)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (list[mid] > want) lo = mid + 1; else hi = mid;
            }
            hit = lo < P && list[lo] == want;
        }
        keep[r] = in && !hit;
        const unsigned long long m = __ballot(keep[r]);
        before[r] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[r][w] = __popcll(m);
    }
    __syncthreads();
    int base = 0;                                 // survivors in the rounds before this one
#pragma unroll
    for (int r = 0; r < EX_ROUNDS; ++r) {
        int slot = base + before[r];
#pragma unroll
        for (int x = 0; x < EX_NT / 64; ++x) {
            const int t = wave_total[r][x];
            if (x < w) slot += t;
            base += t;
        }
        if (keep[r] && slot < k) {
            if (out_keys) out_keys[q * k + slot] = key[r];
            out_scores[q * k + slot] = sc[r];
            if (out_carry) out_carry[q * k + slot] = car[r];
        }
    }
    for (int i = base + tid; i < k; i += EX_NT) {  // base = all survivors of the query
        if (out_keys) out_keys[q * k + i] = fill_key;
        out_scores[q * k + i] = fill_score;
        if (out_carry) out_carry[q * k + i] = fill_carry;
    }
}

}  // namespace amdrec

using namespace amdrec;

extern "C" int amdrec_exclude_compact(const int64_t* keys, const float* scores, const int64_t* carry, int64_t nq, int kc,
                                      const int64_t* exclude, int n_exclude, int64_t ld_exclude, int k, int64_t fill_key,
                                      float fill_score, int64_t fill_carry, int64_t* out_keys, float* out_scores,
                                      int64_t* out_carry, void* stream) {
    REQUIRE(kc >= 1 && kc <= AMDREC_MAX_K, "kc=%d out of range [1, %d]", kc, AMDREC_MAX_K);
    REQUIRE(k >= 1 && k <= kc, "k=%d out of range [1, kc=%d]", k, kc);
    REQUIRE(n_exclude >= 1 && n_exclude < AMDREC_MAX_K, "n_exclude=%d out of range [1, %d]", n_exclude, AMDREC_MAX_K - 1);
    REQUIRE(ld_exclude >= n_exclude, "ld_exclude=%lld is smaller than n_exclude=%d", (long long)ld_exclude, n_exclude);
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq <= 2147483647ll, "nq=%lld: at most 2^31 - 1 queries per call", (long long)nq);
    REQUIRE(keys != nullptr && scores != nullptr, "null pointer: keys / scores");
    REQUIRE(exclude != nullptr, "null pointer: exclude");
    REQUIRE(out_scores != nullptr, "null pointer: out_scores");
    REQUIRE(out_keys != nullptr || (carry != nullptr && out_carry != nullptr),
            "null pointer: out_keys (it may be NULL only when carry and out_carry are given)");
    REQUIRE((carry == nullptr) == (out_carry == nullptr), "carry and out_carry go together (one of them is NULL)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("exclude_compact", 0.0, (double)nq * ((double)kc * (carry ? 20 : 12) + (double)n_exclude * 8), st);
    hipLaunchKernelGGL(exclude_compact_kernel, dim3((unsigned)nq), dim3(EX_NT), 0, st, (const long long*)keys, scores,
                       (const long long*)carry, kc, (const long long*)exclude, n_exclude, (long long)ld_exclude, k,
                       (long long)fill_key, fill_score, (long long)fill_carry, (long long*)out_keys, out_scores,
                       (long long*)out_carry);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
