// IVFPQ refine (faiss IndexRefineFlat over IndexIVFPQ; behind FAISSIndex(index_type='IVFPQ', refine=...)): the code scan's
// kc candidates of every query re-ranked by their exact squared L2 distance to the kept row (fp32, or bf16 widened to fp32).
//   rerank : gridDim.x workgroups per query (blockIdx.y) share its kc candidate slots.  A wave takes one candidate row at a
//            time, RR_RU rows in flight (a candidate is a random 1 KiB / 512 B read at d = 256: latency-bound, as the flat
//            search's re-score), 16-byte loads.  A row's distance has ONE fixed evaluation order whatever workgroup, wave or
//            batch handles it: lane l sums (q_i - x_i)^2 over its 16-byte chunks l, l + 64, ... as one fma chain in element
//            order, then the 64 partial sums fold through the xor butterfly 32, 16, ... 1 (every lane ends with the same
//            bits).  Keys (orderable -distance, ~position) as the pool keys; a row flagged non-finite, or whose distance is
//            NaN, gets -inf (after every finite row, by position); an unfilled slot (-1) or a position outside the rows gets
//            no key.  The workgroup that draws the query's last ticket sorts the keys and writes the best k.
#include "common.hpp"
#include "topk_utils.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int RR_RU = 8;             // candidate rows in flight per wave
constexpr int RR_MAX_SLICES = 32;    // workgroups per query at most
constexpr int RR_SLICE_ROWS = 64;    // ... each with at least one full round of its 8 waves

template <bool BF16>
__global__ __launch_bounds__(512) void rerank_kernel(const void* rows_, long long nrows, long long ldr, int dim,
                                                     const unsigned char* finite, const float* Q, long long ldq,
                                                     const long long* cand, int kc, long long pos_offset, int k,
                                                     unsigned long long* part, int* tickets, float* outD, long long* outI) {
    __shared__ __attribute__((aligned(16))) float qv[2048];
    __shared__ __attribute__((aligned(16))) unsigned long long keys[2048];
    __shared__ __attribute__((aligned(16))) unsigned long long sorted[2048];
    const long long q = blockIdx.y;
    const int s = blockIdx.x, S = gridDim.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (kc + S - 1) / S;
    const int lo = s * per < kc ? s * per : kc, hi = lo + per < kc ? lo + per : kc;
    for (int c = tid; c < (dim >> 2); c += 512)
        reinterpret_cast<f32x4*>(qv)[c] = *reinterpret_cast<const f32x4*>(Q + q * ldq + 4 * c);
    __syncthreads();
    const long long* cq = cand + q * kc;
    constexpr int EPC = BF16 ? 8 : 4;                        // elements per 16-byte chunk
    const int nchunk = dim / EPC;
    for (int i0 = lo + w; i0 < hi; i0 += 8 * RR_RU) {
        float a[RR_RU];
        long long pos[RR_RU];
        bool live[RR_RU];
        const uint4* xr[RR_RU];
#pragma unroll
        for (int u = 0; u < RR_RU; ++u) {
            const int i = i0 + 8 * u;
            const long long p = i < hi ? cq[i] : -1ll;
            pos[u] = p;
            live[u] = p >= 0 && p < nrows && (finite == nullptr || finite[p] != 0);   // wave-uniform
            a[u] = 0.f;
            const long long r = live[u] ? p : 0;             // (a dead slot reads row 0's address, never dereferenced)
            xr[u] = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(rows_) + r * ldr * (BF16 ? 2 : 4));
        }
        for (int cc = lane; cc < nchunk; cc += 64) {
            uint4 x[RR_RU];
#pragma unroll
            for (int u = 0; u < RR_RU; ++u) x[u] = live[u] ? xr[u][cc] : make_uint4(0u, 0u, 0u, 0u);
            const float* y = &qv[EPC * cc];
            if constexpr (BF16) {
                const f32x4 y0 = *reinterpret_cast<const f32x4*>(y), y1 = *reinterpret_cast<const f32x4*>(y + 4);
#pragma unroll
                for (int u = 0; u < RR_RU; ++u) {
                    const uint32_t wd[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {            // elements 2e (low half) and 2e + 1 (high half), in order
                        const float ya = e < 2 ? y0[2 * e] : y1[2 * e - 4], yb = e < 2 ? y0[2 * e + 1] : y1[2 * e - 3];
                        const float d0 = ya - __uint_as_float(wd[e] << 16);
                        a[u] = __builtin_fmaf(d0, d0, a[u]);
                        const float d1 = yb - __uint_as_float(wd[e] & 0xffff0000u);
                        a[u] = __builtin_fmaf(d1, d1, a[u]);
                    }
                }
            } else {
                const f32x4 yv = *reinterpret_cast<const f32x4*>(y);
#pragma unroll
                for (int u = 0; u < RR_RU; ++u) {
                    const uint32_t wd[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float df = yv[e] - __uint_as_float(wd[e]);
                        a[u] = __builtin_fmaf(df, df, a[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RR_RU; ++u) {
            float v = a[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            const int i = i0 + 8 * u;
            if (lane == 0 && i < hi) {
                const bool slot = pos[u] >= 0 && pos[u] < nrows;
                float sc = live[u] ? -v : -INFINITY;
                if (!(sc == sc)) sc = -INFINITY;             // a NaN distance (non-finite query or row) ranks last
                keys[i] = slot ? make_key(sc, (uint32_t)pos[u]) : 0ull;
            }
        }
    }
    __syncthreads();
    if (S > 1) {
        unsigned long long* list = part + q * kc;
        for (int i = lo + tid; i < hi; i += 512) list[i] = keys[i];
        if (!last_workgroup(&tickets[q], S, true)) return;
        for (int i = tid; i < kc; i += 512) keys[i] = list[i];
        __syncthreads();
    }
    // kc keys, zeros = slots without a key: descending = distance ascending, then -inf keys by position, then the zeros
    const unsigned long long* res = sort_keys_desc<512>(keys, sorted, kc, 512);
    for (int i = tid; i < k; i += 512) {
        const unsigned long long key = res[i];
        outD[q * k + i] = key != 0ull ? 0.f - key_score(key) : INFINITY;
        outI[q * k + i] = key != 0ull ? (long long)key_pos(key) + pos_offset : -1ll;
    }
}

}  // namespace amdrec

using namespace amdrec;

// (amdrec/ivfpq.py RERANK_SPLIT_MAX_QUERIES states the same limit: more than 512 queries are never split)
static int rerank_slices(int64_t nq, int kc) {
    int64_t s = kc / RR_SLICE_ROWS;
    s = s < 1024 / nq ? s : 1024 / nq;
    s = s < RR_MAX_SLICES ? s : RR_MAX_SLICES;
    return s < 2 ? 1 : (int)s;
}

extern "C" int amdrec_ivfpq_rerank(const void* rows, int rows_bf16, int64_t nrows, int64_t ld_rows, int dim,
                                   const uint8_t* finite, const float* queries, int64_t nq, int64_t ld_queries,
                                   const int64_t* cand_pos, int kc, int64_t pos_offset, int k, float* out_dist,
                                   int64_t* out_pos, void* workspace, size_t workspace_bytes, int32_t* tickets,
                                   void* stream) {
    REQUIRE(rows_bf16 == 0 || rows_bf16 == 1, "rows_bf16=%d must be 0 or 1", rows_bf16);
    REQUIRE(kc >= 1 && kc <= AMDREC_MAX_K, "kc=%d out of range [1, %d]", kc, AMDREC_MAX_K);
    REQUIRE(k >= 1 && k <= kc, "k=%d out of range [1, kc=%d]", k, kc);
    REQUIRE(dim >= 4 && dim <= 2048 && dim % (rows_bf16 ? 8 : 4) == 0, "dim=%d must be a multiple of %d in [4, 2048]", dim,
            rows_bf16 ? 8 : 4);
    REQUIRE(nrows >= 0 && nrows < (1ll << 32), "nrows=%lld out of range", (long long)nrows);
    REQUIRE(ld_rows >= dim && ld_rows % (rows_bf16 ? 8 : 4) == 0 && ld_queries >= dim && ld_queries % 4 == 0,
            "bad leading dimension (ld_rows=%lld, ld_queries=%lld)", (long long)ld_rows, (long long)ld_queries);
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq <= 65535, "nq=%lld: at most 65535 queries per call", (long long)nq);
    REQUIRE(nrows == 0 || rows != nullptr, "null pointer: rows");
    REQUIRE(queries != nullptr, "null pointer: queries");
    REQUIRE(cand_pos != nullptr, "null pointer: cand_pos");
    REQUIRE(out_dist != nullptr && out_pos != nullptr, "null pointer: out_dist / out_pos");
    REQUIRE(((uintptr_t)rows % 16) == 0 && ((uintptr_t)queries % 16) == 0, "rows / queries must be 16-byte aligned");
    // several workgroups per query only with the caller's scratch (one key per candidate slot) and tickets; without: one
    int slices = workspace && tickets ? rerank_slices(nq, kc) : 1;
    if (slices > 1) {
        const size_t need = (size_t)nq * kc * 8;
        if (int rc = require_workspace(workspace, workspace_bytes, need, 8)) return rc;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("ivfpq_rerank", 3.0 * nq * kc * dim, (double)nq * kc * dim * (rows_bf16 ? 2 : 4), st);
#define AMDREC_RERANK(B)                                                                                                   \
    hipLaunchKernelGGL(rerank_kernel<B>, dim3((unsigned)slices, (unsigned)nq), dim3(512), 0, st, rows, (long long)nrows,   \
                       (long long)ld_rows, dim, finite, queries, (long long)ld_queries, (const long long*)cand_pos, kc,    \
                       (long long)pos_offset, k, reinterpret_cast<unsigned long long*>(workspace), tickets, out_dist,      \
                       (long long*)out_pos)
    if (rows_bf16) AMDREC_RERANK(true);
    else AMDREC_RERANK(false);
#undef AMDREC_RERANK
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
