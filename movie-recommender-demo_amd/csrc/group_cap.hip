// Per-group caps on a search result (behind FAISSIndex.search_device(..., max_per_group=)): the search ran for kc positions per
// query; this step keeps an entry iff fewer than max_per_group earlier filled entries of its row share its non-negative group
// key (group_of[position]; a position outside the array counts as ungrouped), closes the gaps, order kept, and cuts to k.
//   group_cap_compact : one workgroup of 512 per query, built like exclude_compact.  Thread t owns columns t, t + 512, ...;
//            the columns' groups go to LDS (an unfilled column as -1, so that it is never counted), each thread decides its
//            columns with below_group_cap and the survivors' output slots come from compact_slots - the two pieces the capped
//            stage-2 selection (select.hip) uses as well.  An unfilled column (position < 0) is never dropped and keeps its
//            place: behind every filled one, as the searches write them.  Slots past the last survivor get -1 / fill_score.
#include "common.hpp"
#include "topk_utils.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int GC_NT = 512;                        // threads per workgroup
constexpr int GC_ROUNDS = AMDREC_MAX_K / GC_NT;   // columns per thread at most

__global__ __launch_bounds__(GC_NT) void group_cap_compact_kernel(const long long* pos, const float* scores, int kc,
                                                                  const long long* group_of, long long n_group_rows, int cap,
                                                                  int k, float fill_score, long long* out_pos,
                                                                  float* out_scores) {
    __shared__ __attribute__((aligned(16))) long long grp[AMDREC_MAX_K];
    __shared__ int wave_total[GC_ROUNDS][GC_NT / 64];
    const long long q = blockIdx.x;
    const int tid = threadIdx.x;
    long long p[GC_ROUNDS], g[GC_ROUNDS];
    float sc[GC_ROUNDS];
#pragma unroll
    for (int r = 0; r < GC_ROUNDS; ++r) {
        const int c = r * GC_NT + tid;
        const bool in = c < kc;
        p[r] = in ? pos[q * kc + c] : -1ll;
        sc[r] = in ? scores[q * kc + c] : 0.f;
        g[r] = group_at(group_of, n_group_rows, p[r]);
        if (in) grp[c] = g[r];
    }
    __syncthreads();
    bool keep[GC_ROUNDS];
    int slot[GC_ROUNDS];
#pragma unroll
    for (int r = 0; r < GC_ROUNDS; ++r) {
        const int c = r * GC_NT + tid;
        keep[r] = c < kc && (g[r] < 0 || below_group_cap(grp, c, g[r], cap));
    }
    const int kept = compact_slots<GC_NT, GC_ROUNDS>(keep, slot, wave_total);
#pragma unroll
    for (int r = 0; r < GC_ROUNDS; ++r)
        if (keep[r] && slot[r] < k) {
            out_pos[q * k + slot[r]] = p[r];
            out_scores[q * k + slot[r]] = sc[r];
        }
    for (int i = kept + tid; i < k; i += GC_NT) {
        out_pos[q * k + i] = -1ll;
        out_scores[q * k + i] = fill_score;
    }
}

}  // namespace amdrec

using namespace amdrec;

extern "C" int amdrec_group_cap_compact(const int64_t* pos, const float* scores, int64_t nq, int kc, const int64_t* group_of,
                                        int64_t n_group_rows, int max_per_group, int k, float fill_score, int64_t* out_pos,
                                        float* out_scores, void* stream) {
    REQUIRE(kc >= 1 && kc <= AMDREC_MAX_K, "kc=%d out of range [1, %d]", kc, AMDREC_MAX_K);
    REQUIRE(k >= 1 && k <= kc, "k=%d out of range [1, kc=%d]", k, kc);
    REQUIRE(max_per_group >= 1 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [1, %d]", max_per_group,
            AMDREC_MAX_K);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq <= 2147483647ll, "nq=%lld: at most 2^31 - 1 queries per call", (long long)nq);
    REQUIRE(pos != nullptr && scores != nullptr, "null pointer: pos / scores");
    REQUIRE(group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    REQUIRE(out_pos != nullptr && out_scores != nullptr, "null pointer: out_pos / out_scores");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("group_cap_compact", 0.0, (double)nq * ((double)kc * 20 + (double)k * 12), st);
    hipLaunchKernelGGL(group_cap_compact_kernel, dim3((unsigned)nq), dim3(GC_NT), 0, st, (const long long*)pos, scores, kc,
                       (const long long*)group_of, (long long)n_group_rows, max_per_group, k, fill_score, (long long*)out_pos,
                       out_scores);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
