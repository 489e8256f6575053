// Small per-row kernels around the GEMM-shaped stages (HBM-bound, coalesced float4 traffic).
#include "../../include/amdrec.h"
#include "common.hpp"
#include "topk_utils.hpp"

namespace amdrec {

// faiss.normalize_L2 (faiss_retrieval.py:115, :147): x *= 1/sqrt(sum x^2) for rows with
// non-zero norm.  One wave per row, float4 lanes; out may alias in.
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* in, long long ldi, float* out,
                                                           long long ldo, long long rows, int d) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(in + row * ldi);
    f32x4* dst = reinterpret_cast<f32x4*>(out + row * ldo);
    const int d4 = d >> 2;
    float ss = 0.f;
    for (int c = lane; c < d4; c += 64) {
        f32x4 v = src[c];
        ss += sumsq4(v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float inv = ss > 0.f ? 1.0f / sqrtf(ss) : 1.0f;
    for (int c = lane; c < d4; c += 64) {
        f32x4 v = src[c];
        dst[c] = f32x4{v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv};
    }
}

// FAISSIndex.search id remap (faiss_retrieval.py:159-160): ids[i] = id_map[pos[i]];
// pos == -1 (unfilled slot) reads id_map[n-1], exactly like Python's id_map[-1].
__global__ void remap_ids_kernel(const long long* pos, const long long* id_map, long long n_map, long long* out,
                                 long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long p = pos[i];
    if (p < 0) p += n_map;
    out[i] = (p >= 0 && p < n_map) ? id_map[p] : -1;
}

// Request-side numerical feature prep (inference.py:186-195 / data_preprocessing.py: log1p(|x|) then
// StandardScaler.transform): out = (log1p(|x|) - mean[c]) / scale[c], float32 out (the reference's float64
// result crashes its own float32 model).
__global__ void prep_numerical_kernel(const float* x, const float* mean, const float* scale, float* out, long long rows,
                                      int cols) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int c = (int)(i % cols);
    out[i] = (log1pf(fabsf(x[i])) - mean[c]) / scale[c];
}

// Stage-2 selection (inference.py:258-263, faiss_retrieval.py:355-358): per user, the top_k of
// its k_c candidates by the ranking task's LOGIT (sigmoid is monotone; ranking on logits avoids
// the ties of saturated sigmoids), order (logit desc, candidate slot asc); then sigmoid of every
// task's logit at the winners and the winners' ad ids.  cand_pos (nullable): the candidates' stage-1 positions; a slot whose
// position is negative was never filled by the search and is no candidate: it gets the empty key 0 (below every real key,
// NaN logits included), so it can only appear behind all real candidates, where it reads id -1 / probability 0 like the
// tail of a list shorter than top_k.  One block per user, bitonic sort of 64-bit (logit, ~slot) keys in LDS.
__global__ __launch_bounds__(256) void select_topk_kernel(const float* logits, long long ld, int n_tasks,
                                                          int rank_task, const long long* cand_ids,
                                                          const long long* cand_pos, int k_c, int top_k,
                                                          long long* out_ids, float* out_scores, int* out_slots,
                                                          long long n_users) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    const long long u = blockIdx.x;
    int P = 2;
    while (P < k_c) P <<= 1;
    const float* lr = logits + (long long)rank_task * ld + u * k_c;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        unsigned long long key = 0ull;
        if (i < k_c && !(cand_pos && cand_pos[u * k_c + i] < 0)) {
            float v = lr[i];
            if (v == v) key = make_key(v, (uint32_t)i);     // NaN logits rank last
            else key = (unsigned long long)(~(uint32_t)i) | (1ull << 32);
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int sz = 2; sz <= P; sz <<= 1)
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int i = threadIdx.x; i < P; i += blockDim.x) {
                int j = i ^ st;
                if (j > i) {
                    unsigned long long a = keys[i], b = keys[j];
                    bool desc = (i & sz) == 0;
                    if (desc ? (a < b) : (a > b)) { keys[i] = b; keys[j] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < top_k; i += blockDim.x) {
        const bool valid = i < k_c && keys[i] != 0ull;           // (0 = empty: padding, or a slot stage 1 left unfilled)
        const int slot = valid ? (int)key_pos(keys[i]) : -1;
        out_ids[u * top_k + i] = valid ? cand_ids[u * k_c + slot] : -1;
        if (out_slots) out_slots[u * top_k + i] = slot;
        for (int t = 0; t < n_tasks; ++t) {
            float x = valid ? logits[(long long)t * ld + u * k_c + slot] : -INFINITY;
            out_scores[((long long)t * n_users + u) * top_k + i] = sigmoid_prob(x);
        }
    }
}

// The same for small top_k (<= 32: the serving path's top-10 of 500) without a sort: ONE WAVE per user holds the user's
// keys in registers (KPL per lane, k_c <= 64 * KPL) and extracts the maximum top_k times (wave max by lane exchange, the
// unique holder retires its key).  Keys are unique (the slot is part of the key), so the order is the sort's.  The
// 512-key bitonic sort above takes ~20 us of barriers whatever the batch; this takes ~3.
template <int KPL>
__global__ __launch_bounds__(256) void select_topk_small_kernel(const float* logits, long long ld, int n_tasks, int rank_task,
                                                                const long long* cand_ids, const long long* cand_pos,
                                                                int k_c, int top_k, long long* out_ids, float* out_scores,
                                                                int* out_slots, long long n_users) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;                                  // wave-uniform
    const float* lr = logits + (long long)rank_task * ld + u * k_c;
    unsigned long long key[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i = lane + 64 * j;
        unsigned long long kk = 0ull;
        if (i < k_c && !(cand_pos && cand_pos[u * k_c + i] < 0)) {
            const float v = lr[i];
            kk = (v == v) ? make_key(v, (uint32_t)i) : ((unsigned long long)(~(uint32_t)i) | (1ull << 32));   // NaN ranks last
        }
        key[j] = kk;
    }
    unsigned long long mine = 0ull;                            // lane r keeps winner r: the dependent loads (candidate id, the
    for (int r = 0; r < top_k; ++r) {                          // tasks' logits) go out together after the loop, one latency
        unsigned long long m = key[0];                         // instead of one per rank (they were 10 of the kernel's 15 us)
#pragma unroll
        for (int j = 1; j < KPL; ++j) m = key[j] > m ? key[j] : m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, 64);
            m = other > m ? other : m;
        }
#pragma unroll
        for (int j = 0; j < KPL; ++j) key[j] = key[j] == m ? 0ull : key[j];      // retire the winner (0 = empty)
        if (lane == r) mine = m;
    }
    if (lane < top_k) {
        const int r = lane;
        const bool valid = r < k_c && mine != 0ull;
        const int slot = valid ? (int)key_pos(mine) : -1;
        out_ids[u * top_k + r] = valid ? cand_ids[u * k_c + slot] : -1;
        if (out_slots) out_slots[u * top_k + r] = slot;
        for (int t = 0; t < n_tasks; ++t) {
            const float x = valid ? logits[(long long)t * ld + u * k_c + slot] : -INFINITY;
            out_scores[((long long)t * n_users + u) * top_k + r] = sigmoid_prob(x);
        }
    }
}

// ---- the same selection under a per-group cap (amdrec_select_topk_capped) ---------------------------------------------
// The key of candidate slot i of a user, exactly as the two kernels above build it (0 = no candidate).
__device__ __forceinline__ unsigned long long select_key(const float* lr, const long long* cand_pos_u, int i, int k_c) {
    if (i >= k_c || cand_pos_u[i] < 0) return 0ull;
    const float v = lr[i];
    return (v == v) ? make_key(v, (uint32_t)i) : ((unsigned long long)(~(uint32_t)i) | (1ull << 32));   // NaN ranks last
}

// what both capped kernels write for result slot r of user u (key 0: the unfilled tail)
__device__ __forceinline__ void write_winner(unsigned long long key, long long u, int r, const float* logits, long long ld,
                                             int n_tasks, const long long* cand_ids, int k_c, int top_k, long long* out_ids,
                                             float* out_scores, int* out_slots, long long n_users) {
    const bool valid = key != 0ull;
    const int slot = valid ? (int)key_pos(key) : -1;
    out_ids[u * top_k + r] = valid ? cand_ids[u * k_c + slot] : -1;
    if (out_slots) out_slots[u * top_k + r] = slot;
    for (int t = 0; t < n_tasks; ++t) {
        const float x = valid ? logits[(long long)t * ld + u * k_c + slot] : -INFINITY;
        out_scores[((long long)t * n_users + u) * top_k + r] = sigmoid_prob(x);
    }
}

// Serving shape: select_topk_small_kernel with the group of every key next to it (one gather through cand_pos per key, issued
// with the logit loads).  The greedy rule in this form: a round's winner belongs to a group that is not saturated, so it is
// accepted; the wave then counts the accepted winners of that group (lanes 0 .. r hold them: a ballot and a popcount), and
// when the count reaches the cap every lane retires its remaining keys of the group - a saturated group never wins a later
// round, and the loop still runs exactly top_k rounds.
template <int KPL>
__global__ __launch_bounds__(256) void select_topk_capped_small_kernel(const float* logits, long long ld, int n_tasks,
                                                                       int rank_task, const long long* cand_ids,
                                                                       const long long* cand_pos, int k_c, int top_k,
                                                                       long long* out_ids, float* out_scores, int* out_slots,
                                                                       long long n_users, const long long* group_of,
                                                                       long long n_group_rows, int cap) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;                                  // wave-uniform
    const float* lr = logits + (long long)rank_task * ld + u * k_c;
    const long long* pu = cand_pos + u * k_c;
    unsigned long long key[KPL];
    long long grp[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i = lane + 64 * j;
        key[j] = select_key(lr, pu, i, k_c);
        grp[j] = i < k_c ? group_at(group_of, n_group_rows, pu[i]) : -1ll;
    }
    unsigned long long mine = 0ull;                            // lane r keeps winner r and its group
    long long mine_g = -1ll;
    for (int r = 0; r < top_k; ++r) {
        unsigned long long m = key[0];
#pragma unroll
        for (int j = 1; j < KPL; ++j) m = key[j] > m ? key[j] : m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, 64);
            m = other > m ? other : m;
        }
        if (m == 0ull) continue;                               // wave-uniform: no candidate is left, the tail stays empty
        long long g = -1ll;                                    // the winner's group, from its unique holder
        bool holder = false;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const bool hit = key[j] == m;
            g = hit ? grp[j] : g;
            holder = holder || hit;
            key[j] = hit ? 0ull : key[j];                      // retire the winner (0 = empty)
        }
        const int src = __ffsll((long long)__ballot(holder)) - 1;
        g = __shfl(g, src, 64);
        if (lane == r) { mine = m; mine_g = g; }
        if (g >= 0) {                                          // wave-uniform
            const int taken = __popcll(__ballot(lane <= r && mine != 0ull && mine_g == g));
            if (taken >= cap) {
#pragma unroll
                for (int j = 0; j < KPL; ++j) key[j] = grp[j] == g ? 0ull : key[j];
            }
        }
    }
    // after a skipped round (fewer accepted candidates than top_k) the winners sit in lanes 0 .. n - 1 without a gap: a round
    // is skipped only once no key is left, and then every later round is skipped too
    if (lane < top_k)
        write_winner(mine, u, lane, logits, ld, n_tasks, cand_ids, k_c, top_k, out_ids, out_scores, out_slots, n_users);
}

// General shape (up to AMDREC_MAX_K candidates): the LDS bitonic sort of the keys, the sorted entries' groups next to them,
// keep = "fewer than cap earlier entries of my group" (below_group_cap), a block prefix sum over the keep flags
// (compact_slots), and the first top_k kept entries go out.  One workgroup of 512 per user.
constexpr int CAP_NT = 512;
constexpr int CAP_ROUNDS = AMDREC_MAX_K / CAP_NT;

__global__ __launch_bounds__(CAP_NT) void select_topk_capped_kernel(const float* logits, long long ld, int n_tasks,
                                                                    int rank_task, const long long* cand_ids,
                                                                    const long long* cand_pos, int k_c, int top_k,
                                                                    long long* out_ids, float* out_scores, int* out_slots,
                                                                    long long n_users, const long long* group_of,
                                                                    long long n_group_rows, int cap) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[AMDREC_MAX_K];
    __shared__ __attribute__((aligned(16))) long long grp[AMDREC_MAX_K];
    __shared__ int wave_total[CAP_ROUNDS][CAP_NT / 64];
    const long long u = blockIdx.x;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < k_c) P <<= 1;
    const float* lr = logits + (long long)rank_task * ld + u * k_c;
    const long long* pu = cand_pos + u * k_c;
    for (int i = tid; i < P; i += CAP_NT) keys[i] = select_key(lr, pu, i, k_c);
    __syncthreads();
    bitonic_desc(keys, P);                                     // (ends behind a block barrier)
    unsigned long long key[CAP_ROUNDS];
    long long g[CAP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CAP_ROUNDS; ++r) {
        const int i = r * CAP_NT + tid;
        key[r] = i < P ? keys[i] : 0ull;
        g[r] = key[r] != 0ull ? group_at(group_of, n_group_rows, pu[key_pos(key[r])]) : -1ll;
        if (i < P) grp[i] = g[r];
    }
    __syncthreads();
    bool keep[CAP_ROUNDS];
    int slot[CAP_ROUNDS];
#pragma unroll
    for (int r = 0; r < CAP_ROUNDS; ++r)
        keep[r] = key[r] != 0ull && (g[r] < 0 || below_group_cap(grp, r * CAP_NT + tid, g[r], cap));
    const int kept = compact_slots<CAP_NT, CAP_ROUNDS>(keep, slot, wave_total);
#pragma unroll
    for (int r = 0; r < CAP_ROUNDS; ++r)
        if (keep[r] && slot[r] < top_k)
            write_winner(key[r], u, slot[r], logits, ld, n_tasks, cand_ids, k_c, top_k, out_ids, out_scores, out_slots, n_users);
    for (int i = kept + tid; i < top_k; i += CAP_NT)
        write_winner(0ull, u, i, logits, ld, n_tasks, cand_ids, k_c, top_k, out_ids, out_scores, out_slots, n_users);
}

}  // namespace amdrec

using namespace amdrec;

extern "C" int amdrec_prep_numerical(const float* x, const float* mean, const float* scale, float* out, int64_t rows,
                                     int cols, void* stream) {
    REQUIRE(cols >= 1, "cols must be >= 1");
    if (rows <= 0) return AMDREC_OK;
    REQUIRE(x && mean && scale && out, "null pointer");
    const long long n = rows * cols;
    hipLaunchKernelGGL(prep_numerical_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, mean, scale, out, (long long)rows, cols);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_select_topk(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                  const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                  int64_t* out_ids, float* out_scores, int32_t* out_slots, void* stream) {
    REQUIRE(n_tasks >= 1 && rank_task >= 0 && rank_task < n_tasks, "bad task index");
    REQUIRE(k_c >= 1 && k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(top_k >= 1 && top_k <= AMDREC_MAX_K, "top_k out of range");
    if (n_users <= 0) return AMDREC_OK;
    REQUIRE(logits && cand_ids && out_ids && out_scores, "null pointer");
    REQUIRE(ld_logits >= n_users * k_c, "ld_logits too small");
    if (top_k <= 32 && k_c <= 512) {                            // one wave per user, no sort
        const dim3 grid((unsigned)((n_users + 3) / 4));
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        if (k_c <= 128)
            hipLaunchKernelGGL(select_topk_small_kernel<2>, grid, dim3(256), 0, st, logits, (long long)ld_logits, n_tasks, rank_task,
                               (const long long*)cand_ids, (const long long*)cand_pos, k_c, top_k, (long long*)out_ids, out_scores, out_slots, (long long)n_users);
        else
            hipLaunchKernelGGL(select_topk_small_kernel<8>, grid, dim3(256), 0, st, logits, (long long)ld_logits, n_tasks, rank_task,
                               (const long long*)cand_ids, (const long long*)cand_pos, k_c, top_k, (long long*)out_ids, out_scores, out_slots, (long long)n_users);
        HIP_TRY(hipGetLastError());
        return AMDREC_OK;
    }
    int P = 2;
    while (P < k_c) P <<= 1;
    hipLaunchKernelGGL(select_topk_kernel, dim3((unsigned)n_users), dim3(256), (size_t)P * 8,
                       reinterpret_cast<hipStream_t>(stream), logits, (long long)ld_logits, n_tasks, rank_task,
                       (const long long*)cand_ids, (const long long*)cand_pos, k_c, top_k, (long long*)out_ids, out_scores, out_slots,
                       (long long)n_users);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_select_topk_capped(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                         const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                         int64_t* out_ids, float* out_scores, int32_t* out_slots, const int64_t* group_of,
                                         int64_t n_group_rows, int max_per_group, void* stream) {
    REQUIRE(n_tasks >= 1 && rank_task >= 0 && rank_task < n_tasks, "bad task index");
    REQUIRE(k_c >= 1 && k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(top_k >= 1 && top_k <= AMDREC_MAX_K, "top_k out of range");
    REQUIRE(max_per_group >= 1 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [1, %d]", max_per_group,
            AMDREC_MAX_K);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (n_users <= 0) return AMDREC_OK;
    REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
    REQUIRE(logits && cand_ids && out_ids && out_scores, "null pointer");
    REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the capped selection reads every candidate's group through it)");
    REQUIRE(group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    REQUIRE(ld_logits >= n_users * k_c, "ld_logits too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("select_topk_capped", 0.0, (double)n_users * k_c * 20.0, st);
    if (top_k <= 32 && k_c <= 512) {                            // one wave per user, no sort
        const dim3 grid((unsigned)((n_users + 3) / 4));
        if (k_c <= 128)
            hipLaunchKernelGGL(select_topk_capped_small_kernel<2>, grid, dim3(256), 0, st, logits, (long long)ld_logits, n_tasks,
                               rank_task, (const long long*)cand_ids, (const long long*)cand_pos, k_c, top_k, (long long*)out_ids,
                               out_scores, out_slots, (long long)n_users, (const long long*)group_of, (long long)n_group_rows,
                               max_per_group);
        else
            hipLaunchKernelGGL(select_topk_capped_small_kernel<8>, grid, dim3(256), 0, st, logits, (long long)ld_logits, n_tasks,
                               rank_task, (const long long*)cand_ids, (const long long*)cand_pos, k_c, top_k, (long long*)out_ids,
                               out_scores, out_slots, (long long)n_users, (const long long*)group_of, (long long)n_group_rows,
                               max_per_group);
    } else {
        hipLaunchKernelGGL(select_topk_capped_kernel, dim3((unsigned)n_users), dim3(CAP_NT), 0, st, logits, (long long)ld_logits,
                           n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos, k_c, top_k,
                           (long long*)out_ids, out_scores, out_slots, (long long)n_users, (const long long*)group_of,
                           (long long)n_group_rows, max_per_group);
    }
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_l2_normalize(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows,
                                   int dim, void* stream) {
    REQUIRE(dim >= 4 && dim % 4 == 0, "dim=%d must be a positive multiple of 4", dim);
    if (rows <= 0) return AMDREC_OK;
    REQUIRE(ld_in % 4 == 0 && ld_out % 4 == 0 && ld_in >= dim && ld_out >= dim, "bad leading dimension");
    REQUIRE(in && out, "null pointer");
    REQUIRE(((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0, "pointers must be 16-byte aligned");
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), in, (long long)ld_in, out, (long long)ld_out,
                       (long long)rows, dim);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_remap_ids(const int64_t* pos, const int64_t* id_map, int64_t n_map, int64_t* out,
                                int64_t n, void* stream) {
    if (n <= 0) return AMDREC_OK;
    REQUIRE(pos && out && (id_map || n_map == 0), "null pointer");
    hipLaunchKernelGGL(remap_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), (const long long*)pos, (const long long*)id_map,
                       (long long)n_map, (long long*)out, (long long)n);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
