// IVFPQ (replaces faiss IndexIVFPQ(IndexFlatIP quantizer, d, nlist, m, 8), metric L2, by_residual, behind
// FAISSIndex(index_type='IVFPQ'), faiss_retrieval.py:56-63).  The coarse level is the IVF index's (ivf.hip); here:
//   pq_encode  : code[r][s] = argmin_j |r_s - C_s[j]|^2 of the residual r = x - c[assign(x)], formed in registers /
//                LDS.  A tiled VALU GEMM per (64 rows, sub-space) against the sub-space's 256 codewords with an arg-min
//                epilogue (argmax <r,C> - |C|^2/2; ties -> lower j).  Also the assignment step of PQ training.
//   pq_accumulate / pq_finish : Lloyd update of the codebooks with 64-bit fixed-point sums (order-independent: training is
//                bit-reproducible, like amdrec_ivf_kmeans_step); an empty codeword keeps its value.
//   pq_tables  : per (query, probed list) the distance tables LUT[s][j] = |(q - c_l)_s - C_s[j]|^2, [m][256] fp32.
//   pq_scan    : one workgroup per (list, query tile of amdrec_ivf_group) x row range: the tile's tables staged in LDS, one
//                code load per row, m LDS lookups per (row, query), pool keys (score = -distance) in amdrec_ivf_select's
//                format - the existing select then yields (distance asc, position asc).
#include "invlists.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int PQ_KSUB = 256;
constexpr int ENC_ROWS = 64;         // rows per encode workgroup (8 per thread row group)
constexpr int ENC_KC = 32;           // sub-space dimensions staged per step
constexpr int TAB_P = 16;            // (query, probe) pairs per table workgroup
constexpr int PQ_MAX_DSUB = 512;     // d <= 2048, m >= 4
constexpr float PQ_FIX = 1099511627776.0f;   // 2^40: |residual coordinate| <= 2, <= 2^20 rows -> |sum| < 2^61

// ---- encode / assignment ------------------------------------------------------------------------------------------------
// Thread t: codes cg*8 .. cg*8+7 (cg = t % 32) of rows rg*8 .. rg*8+7 (rg = t / 32): 64 fp32 accumulators; per staged
// dimension 2 + 2 ds_read_b128 (the row values are a broadcast) feed 64 FMAs.
__global__ __launch_bounds__(256) void pq_encode_kernel(const float* x, long long rows, long long ld, int dsub, int m,
                                                        const long long* assign, const float* cent, long long ldc,
                                                        int nlist, const float* cb, unsigned char* codes) {
    __shared__ __attribute__((aligned(16))) float cs[ENC_KC][PQ_KSUB];
    __shared__ __attribute__((aligned(16))) float rs[ENC_KC][ENC_ROWS];
    __shared__ float cn[PQ_KSUB];
    const int s = blockIdx.y, t = threadIdx.x, cg = t & 31, rg = t >> 5;
    const long long row0 = (long long)blockIdx.x * ENC_ROWS;
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    float nrm = 0.f;                                    // |C_s[t]|^2, summed in dimension order
    const float* cw = cb + ((long long)s * PQ_KSUB + t) * dsub;
    const int rr = t >> 2, c0 = (t & 3) * 8;            // staging: row rr of the tile, dimensions c0 .. c0+7 of the step
    long long r = row0 + rr;
    r = r < rows ? r : rows - 1;                        // clamped: the row's result is dropped below
    long long a = assign[r];
    a = a < 0 ? 0 : (a >= nlist ? nlist - 1 : a);       // (a row of an invalid list reads list 0 / the last: never out of bounds)
    const float* xr = x + r * ld + (long long)s * dsub;
    const float* cr = cent + a * ldc + (long long)s * dsub;
    for (int k0 = 0; k0 < dsub; k0 += ENC_KC) {
        const int kc = dsub - k0 < ENC_KC ? dsub - k0 : ENC_KC;   // a multiple of 4
        __syncthreads();
        for (int kk = 0; kk < kc; kk += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(cw + k0 + kk);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cs[kk + e][t] = v[e];
                nrm = __builtin_fmaf(v[e], v[e], nrm);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j += 4) {
            if (c0 + j < kc) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + k0 + c0 + j);
                const f32x4 cv = *reinterpret_cast<const f32x4*>(cr + k0 + c0 + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) rs[c0 + j + e][rr] = xv[e] - cv[e];
            }
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
            const f32x4 r0v = *reinterpret_cast<const f32x4*>(&rs[kk][rg * 8]);
            const f32x4 r1v = *reinterpret_cast<const f32x4*>(&rs[kk][rg * 8 + 4]);
            const f32x4 c0v = *reinterpret_cast<const f32x4*>(&cs[kk][cg * 8]);
            const f32x4 c1v = *reinterpret_cast<const f32x4*>(&cs[kk][cg * 8 + 4]);
            const float rv[8] = {r0v[0], r0v[1], r0v[2], r0v[3], r1v[0], r1v[1], r1v[2], r1v[3]};
            const float cv[8] = {c0v[0], c0v[1], c0v[2], c0v[3], c1v[0], c1v[1], c1v[2], c1v[3]};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_fmaf(rv[i], cv[j], acc[i][j]);
        }
    }
    cn[t] = nrm;
    __syncthreads();
    float hn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) hn[j] = 0.5f * cn[cg * 8 + j];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float best = -INFINITY;
        int bj = cg * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                   // ascending code: a tie keeps the lower one
            const float sc = acc[i][j] - hn[j];
            if (sc > best) { best = sc; bj = cg * 8 + j; }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {              // across the 32 lanes of the row group (a half wave)
            const float ob = __shfl_xor(best, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        const long long row = row0 + rg * 8 + i;
        if (cg == 0 && row < rows) codes[row * m + s] = (unsigned char)bj;
    }
}

// ---- PQ training: fixed-point per-codeword sums of the residuals, then the means ----------------------------------------
__global__ __launch_bounds__(256) void pq_accumulate_kernel(const float* x, long long rows, long long ld, int d, int dsub,
                                                            int m, const long long* assign, const float* cent, long long ldc,
                                                            int nlist, const unsigned char* codes, long long* sums, int* counts) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    // a row with any non-finite coordinate adds neither sums nor counts (its codes are meaningless): one wave per row
    bool bad = false;
    for (int c = lane; c < d; c += 64) bad |= !__builtin_isfinite(x[r * ld + c]);
    if (__ballot(bad)) return;
    long long a = assign[r];
    a = a < 0 ? 0 : (a >= nlist ? nlist - 1 : a);
    for (int c = lane; c < d; c += 64) {
        const int s = c / dsub;
        const int j = codes[r * m + s];
        const float v = x[r * ld + c] - cent[a * ldc + c];
        if (v == v)
            atomicAdd(reinterpret_cast<unsigned long long*>(&sums[((long long)s * PQ_KSUB + j) * dsub + (c - s * dsub)]),
                      (unsigned long long)__float2ll_rn(v * PQ_FIX));
        if (c == s * dsub) atomicAdd(&counts[s * PQ_KSUB + j], 1);
    }
}

__global__ __launch_bounds__(256) void pq_finish_kernel(const long long* sums, const int* counts, int m, int dsub, float* cb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)m * PQ_KSUB * dsub) return;
    const int n = counts[i / dsub];
    if (n > 0) cb[i] = (float)((double)sums[i] / ((double)PQ_FIX * (double)n));
}

// ---- distance tables --------------------------------------------------------------------------------------------------
// Workgroup (TAB_P pairs, sub-space s); thread t = codeword t: LUT[pair][s][t] = sum_i ((q - c_l)_i - C_s[t]_i)^2 (one
// fma chain in dimension order).  The residuals sit in LDS (broadcast reads), the codeword in registers for all pairs.
__global__ __launch_bounds__(256) void pq_tables_kernel(const float* Q, long long ldq, long long npairs, int nprobe,
                                                        const long long* probes, long long ldp, const float* cent,
                                                        long long ldc, int nlist, const float* cb, int dsub, int m,
                                                        float* tables) {
    __shared__ __attribute__((aligned(16))) float res[TAB_P * PQ_MAX_DSUB];
    const int s = blockIdx.y, t = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * TAB_P;
    for (int e = t; e < TAB_P * dsub; e += 256) {
        const int p = e / dsub, c = e - p * dsub;
        const long long i = i0 + p;
        float v = 0.f;
        if (i < npairs) {
            const long long q = i / nprobe, pr = i - q * nprobe;
            const long long l = probes[q * ldp + pr];
            if (l >= 0 && l < nlist) v = Q[q * ldq + (long long)s * dsub + c] - cent[l * ldc + (long long)s * dsub + c];
        }
        res[e] = v;
    }
    __syncthreads();
    float acc[TAB_P];
#pragma unroll
    for (int p = 0; p < TAB_P; ++p) acc[p] = 0.f;
    const float* cw = cb + ((long long)s * PQ_KSUB + t) * dsub;
    for (int c = 0; c < dsub; c += 4) {
        const f32x4 cv = *reinterpret_cast<const f32x4*>(cw + c);
#pragma unroll
        for (int p = 0; p < TAB_P; ++p) {
            const f32x4 rv = *reinterpret_cast<const f32x4*>(&res[p * dsub + c]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float df = rv[e] - cv[e];
                acc[p] = __builtin_fmaf(df, df, acc[p]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < TAB_P; ++p)
        if (i0 + p < npairs) tables[((i0 + p) * m + s) * PQ_KSUB + t] = acc[p];
}

// ---- the table-lookup scan ------------------------------------------------------------------------------------------------
// blockIdx.y = one (list, query tile) of amdrec_ivf_group (qtile_prefix), blockIdx.x = a share of the list's rows (gridDim.x
// workgroups split a long list).  The tile's queries are taken QS at a time: their tables (m KiB each) fill 64 KiB of LDS
// (two workgroups per CU); each thread then owns a row: one code load (m bytes), and per query m LDS lookups summed in
// sub-space order and one 8-byte key store (consecutive rows: consecutive keys of the query's pool row).  A list keeps its
// rows with a non-finite coordinate after its list_fin[l] finite ones: their keys are -inf (after every finite row).
// list_fin == nullptr: every row is finite.
// EL (ListNoElig or ListElig, invlists.hpp): the eligibility predicate; EP: its pointers as trailing kernel arguments (none
// for ListNoElig: the kernel it always was).  A thread reads its row's tag once, next to the code word, and stores key 0 -
// the select's empty-slot value - for an ineligible (query, row) in both loops: stored, not skipped, the pool is not cleared
// between searches.  The sub-tile's mask words sit in LDS next to its pool offsets.
template <int M, class EL = ListNoElig, class... EP>
__global__ __launch_bounds__(256) void pq_scan_kernel(const unsigned char* codes, const long long* spos,
                                                      const long long* list_off, const long long* list_fin, int nlist, const float* tables, int nprobe,
                                                      const long long* goff, const long long* qt_prefix, int qtile,
                                                      const long long* pair_q, const long long* pair_p, const long long* base,
                                                      unsigned long long* keys, long long pool_ld, long long pos_offset,
                                                      EP... elig) {
    constexpr int QS = 64 / M;                                           // queries per LDS sub-tile
    __shared__ __attribute__((aligned(16))) float lut[QS * M * PQ_KSUB];
    __shared__ long long dst[QS];
    __shared__ typename EL::Mask msk[QS];
    const EL el{elig...};
    const long long y = blockIdx.y;
    if (y >= qt_prefix[nlist]) return;
    const int l = tile_list(y, qt_prefix, nlist);
    const long long r0 = list_off[l], len = list_off[l + 1] - r0, nfin = list_fin ? list_fin[l] : len;
    if ((long long)blockIdx.x * 256 >= len) return;
    const long long g0 = goff[l], g = goff[l + 1] - g0;
    const long long p0 = (y - qt_prefix[l]) * qtile;
    const long long pend = p0 + qtile < g ? p0 + qtile : g;
    const int t = threadIdx.x;
    for (long long sp = p0; sp < pend; sp += QS) {
        const int nsub = (int)(pend - sp < QS ? pend - sp : QS);
        __syncthreads();                                                 // the previous sub-tile's lookups are done
        for (int e = t; e < nsub * M * 64; e += 256) {
            const int j = e / (M * 64), w = e - j * (M * 64);
            const long long pi = pair_q[g0 + sp + j] * nprobe + pair_p[g0 + sp + j];
            reinterpret_cast<f32x4*>(lut)[e] = reinterpret_cast<const f32x4*>(tables + pi * (M * PQ_KSUB))[w];
        }
        if (t < nsub) {
            const long long q = pair_q[g0 + sp + t];
            dst[t] = q * pool_ld + base[q * nprobe + pair_p[g0 + sp + t]];
            if constexpr (EL::on) msk[t] = el.mask(q);
        }
        __syncthreads();
        const long long stride = (long long)gridDim.x * 256, row0 = (long long)blockIdx.x * 256 + t;
        for (long long row = row0; row < nfin; row += stride) {          // the list's finite rows
            uint32_t cw[M / 4];
            const uint32_t* src = reinterpret_cast<const uint32_t*>(codes + (r0 + row) * M);
            if constexpr (M == 4) {
                cw[0] = src[0];
            } else if constexpr (M == 8) {
                const uint2 v = *reinterpret_cast<const uint2*>(src);
                cw[0] = v.x; cw[1] = v.y;
            } else {
#pragma unroll
                for (int h = 0; h < M / 16; ++h) {
                    const uint4 v = reinterpret_cast<const uint4*>(src)[h];
                    cw[4 * h] = v.x; cw[4 * h + 1] = v.y; cw[4 * h + 2] = v.z; cw[4 * h + 3] = v.w;
                }
            }
            const uint32_t pos = (uint32_t)(spos[r0 + row] + pos_offset);
            const typename EL::Tag tg = el.tag(r0 + row);
            for (int j = 0; j < nsub; ++j) {
                const float* lt = lut + j * (M * PQ_KSUB);
                float dist = lt[cw[0] & 0xff];
#pragma unroll
                for (int s = 1; s < M; ++s) dist += lt[s * PQ_KSUB + ((cw[s >> 2] >> (8 * (s & 3))) & 0xff)];
                if constexpr (EL::on)
                    keys[dst[j] + row] = EL::ok(tg, msk[j]) ? make_key(rank_last(-dist), pos) : 0ull;
                else
                    keys[dst[j] + row] = make_key(rank_last(-dist), pos);           // NaN distances rank last
            }
        }
        // its rows with a non-finite coordinate (rare; none when list_fin is null): -inf keys, no lookups.  A loop of
        // their own keeps the per-(row, query) path above as it is
        const long long skip = row0 < nfin ? (nfin - row0 + stride - 1) / stride : 0;
        for (long long row = row0 + skip * stride; row < len; row += stride) {
            const uint32_t pos = (uint32_t)(spos[r0 + row] + pos_offset);
            if constexpr (EL::on) {
                const typename EL::Tag tg = el.tag(r0 + row);
                for (int j = 0; j < nsub; ++j) keys[dst[j] + row] = EL::ok(tg, msk[j]) ? make_key(-INFINITY, pos) : 0ull;
            } else {
                for (int j = 0; j < nsub; ++j) keys[dst[j] + row] = make_key(-INFINITY, pos);
            }
        }
    }
}

__global__ void pq_negate_kernel(const float* in, long long n, float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = -in[i];
}

}  // namespace amdrec

using namespace amdrec;

static bool pq_m_ok(int m) { return m == 4 || m == 8 || m == 16 || m == 32; }

static int pq_check(int dim, int m) {
    REQUIRE(pq_m_ok(m), "m=%d must be 4, 8, 16 or 32", m);
    REQUIRE(dim >= 4 && dim <= 2048 && dim % m == 0 && (dim / m) % 4 == 0,
            "dim=%d must be in [4,2048] with dim %% m == 0 and (dim / m) %% 4 == 0 (m=%d)", dim, m);
    return AMDREC_OK;
}

static int rows_check(const float* x, int64_t rows, int64_t ld, int dim, const int64_t* assign, const float* cent,
                      int64_t ldc, int nlist, const float* cb) {
    REQUIRE(rows >= 0 && rows < (1ll << 31), "rows out of range");
    REQUIRE(nlist >= 1 && nlist <= (1 << 20), "nlist out of range");
    REQUIRE(ld >= dim && ld % 4 == 0 && ldc >= dim && ldc % 4 == 0, "bad leading dimension");
    REQUIRE(rows == 0 || (x && assign && cent && cb), "null pointer");
    REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)cent % 16) == 0 && ((uintptr_t)cb % 16) == 0,
            "x / centroids / codebooks must be 16-byte aligned");
    return AMDREC_OK;
}

static int encode_impl(const float* x, long long rows, long long ld, int dim, const long long* assign, const float* cent,
                       long long ldc, int nlist, const float* cb, int m, unsigned char* codes, hipStream_t st) {
    ProfScope prof("ivfpq_encode", 2.0 * rows * PQ_KSUB * dim, 0.0, st);
    hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)((rows + ENC_ROWS - 1) / ENC_ROWS), (unsigned)m), dim3(256), 0, st, x,
                       rows, ld, dim / m, m, assign, cent, ldc, nlist, cb, codes);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivfpq_encode(const float* x, int64_t rows, int64_t ld, int dim, const int64_t* assign,
                                   const float* centroids, int64_t ld_centroids, int nlist, const float* codebooks, int m,
                                   uint8_t* codes, void* stream) {
    int rc = pq_check(dim, m);
    if (rc) return rc;
    rc = rows_check(x, rows, ld, dim, assign, centroids, ld_centroids, nlist, codebooks);
    if (rc) return rc;
    if (rows == 0) return AMDREC_OK;
    REQUIRE(codes != nullptr, "codes is null");
    return encode_impl(x, rows, ld, dim, (const long long*)assign, centroids, ld_centroids, nlist, codebooks, m, codes,
                       reinterpret_cast<hipStream_t>(stream));
}

// codebook training step: codes | sums | counts, the last two cleared together
struct TrainWs : Carver {
    unsigned char* codes; long long* sums; int* counts;
    size_t clear_bytes;
    TrainWs(int64_t rows, int dim, int m, void* ws) : Carver(ws) {
        codes = take<unsigned char>((size_t)rows * m);
        const size_t mk = bytes();
        sums = take<long long>((size_t)PQ_KSUB * dim);
        counts = take<int>((size_t)m * PQ_KSUB);
        clear_bytes = bytes_since(mk);
    }
};

extern "C" int amdrec_ivfpq_train_workspace(int64_t rows, int dim, int m, size_t* bytes) {
    REQUIRE(bytes != nullptr, "null pointer");
    int rc = pq_check(dim, m);
    if (rc) return rc;
    REQUIRE(rows >= 0 && rows <= (1ll << 20), "rows=%lld out of range [0, 2^20]", (long long)rows);
    *bytes = TrainWs(rows, dim, m, nullptr).bytes();
    return AMDREC_OK;
}

extern "C" int amdrec_ivfpq_train_step(const float* x, int64_t rows, int64_t ld, int dim, const int64_t* assign,
                                       const float* centroids, int64_t ld_centroids, int nlist, float* codebooks, int m, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    size_t need = 0;
    int rc = amdrec_ivfpq_train_workspace(rows, dim, m, &need);
    if (rc) return rc;
    rc = rows_check(x, rows, ld, dim, assign, centroids, ld_centroids, nlist, codebooks);
    if (rc) return rc;
    if (rows == 0) return AMDREC_OK;
    if ((rc = require_workspace(workspace, workspace_bytes, need))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const TrainWs w(rows, dim, m, workspace);
    rc = encode_impl(x, rows, ld, dim, (const long long*)assign, centroids, ld_centroids, nlist, codebooks, m, w.codes, st);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(w.sums, 0, w.clear_bytes, st));
    hipLaunchKernelGGL(pq_accumulate_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, (long long)rows,
                       (long long)ld, dim, dim / m, m, (const long long*)assign, centroids, (long long)ld_centroids, nlist, w.codes,
                       w.sums, w.counts);
    const long long ncb = (long long)PQ_KSUB * dim;
    hipLaunchKernelGGL(pq_finish_kernel, dim3((unsigned)((ncb + 255) / 256)), dim3(256), 0, st, w.sums, w.counts, m, dim / m,
                       codebooks);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivfpq_tables(const float* queries, int64_t nq, int64_t ld_queries, int dim, const int64_t* probes,
                                   int64_t ld_probes, int nprobe, const float* centroids, int64_t ld_centroids, int nlist,
                                   const float* codebooks, int m, float* tables, void* stream) {
    int rc = pq_check(dim, m);
    if (rc) return rc;
    REQUIRE(nprobe >= 1 && nlist >= 1 && ld_probes >= nprobe, "bad nlist/nprobe");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq * (int64_t)nprobe < (1ll << 31), "too many (query, probe) pairs for one call");
    REQUIRE(queries && probes && centroids && codebooks && tables, "null pointer");
    REQUIRE(ld_queries >= dim && ld_centroids >= dim, "bad leading dimension");
    REQUIRE(((uintptr_t)codebooks % 16) == 0, "codebooks must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long npairs = nq * nprobe;
    ProfScope prof("ivfpq_tables", 3.0 * npairs * PQ_KSUB * dim, (double)npairs * m * PQ_KSUB * 4, st);
    hipLaunchKernelGGL(pq_tables_kernel, dim3((unsigned)((npairs + TAB_P - 1) / TAB_P), (unsigned)m), dim3(256), 0, st,
                       queries, (long long)ld_queries, npairs, nprobe, (const long long*)probes, (long long)ld_probes,
                       centroids, (long long)ld_centroids, nlist, codebooks, dim / m, m, tables);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

// The eligibility pointers of amdrec_ivfpq_scan_finite_eligible: all three required and 8-byte aligned, checked with the other
// arguments before the first HIP call.  The plain scans and the eligible one are ONE host template over the predicate.
static int elig_check(ListNoElig) { return AMDREC_OK; }
static int elig_check(ListElig el) {
    REQUIRE(el.tags != nullptr, "list_tags is null");
    REQUIRE(el.all != nullptr, "require_all is null");
    REQUIRE(el.any != nullptr, "require_any is null");
    REQUIRE(((uintptr_t)el.tags % 8) == 0, "list_tags must be 8-byte aligned");
    REQUIRE(((uintptr_t)el.all % 8) == 0, "require_all must be 8-byte aligned");
    REQUIRE(((uintptr_t)el.any % 8) == 0, "require_any must be 8-byte aligned");
    return AMDREC_OK;
}
template <class Kern, class... Args>
static void launch_with(ListNoElig, Kern kern, dim3 grid, dim3 block, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(kern, grid, block, 0, st, args...);
}
template <class Kern, class... Args>
static void launch_with(ListElig el, Kern kern, dim3 grid, dim3 block, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(kern, grid, block, 0, st, args..., el.tags, el.all, el.any);
}
template <int M, class EL>
static constexpr auto pq_scan_for() {
    if constexpr (EL::on) return pq_scan_kernel<M, ListElig, const uint64_t*, const uint64_t*, const uint64_t*>;
    else return pq_scan_kernel<M>;
}

template <class EL>
static int scan_impl(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off,
                     const int64_t* list_finite, int nlist, int64_t max_list_rows, const float* tables, int nprobe,
                     const int64_t* group_off, const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                     const int64_t* pair_query, const int64_t* pair_probe, const int64_t* pool_base, int64_t npairs,
                     uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset, void* stream, EL el) {
    REQUIRE(pq_m_ok(m), "m=%d must be 4, 8, 16 or 32", m);
    REQUIRE(nlist >= 1 && nprobe >= 1, "bad nlist/nprobe");
    REQUIRE(qtile == 32 || qtile == 64, "qtile must be 32 or 64 (the value given to amdrec_ivf_group)");
    if (qtile_bound <= 0 || max_list_rows <= 0 || npairs <= 0) return AMDREC_OK;
    REQUIRE(qtile_bound <= 65535, "too many (list, query-tile) groups for one launch: chunk the queries");
    REQUIRE(codes && row_pos && list_off && tables && group_off && qtile_prefix && pair_query && pair_probe && pool_base &&
                pool_keys, "null pointer");
    REQUIRE(((uintptr_t)codes % 16) == 0 && ((uintptr_t)tables % 16) == 0, "codes / tables must be 16-byte aligned");
    if (int rc = elig_check(el)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // row shares per (list, tile): ~2048 workgroups in all over the tiles that can be non-empty, but at least ~1024 rows each
    // of the longest list: every share re-stages its tile's tables (64 KiB per sub-tile).  One 256-row share per 256-row block
    // (8192 workgroups) read 2.2 GB of tables at 512 queries against nlist 100 / nprobe 10 (scan 0.46 ms)
    const long long tiles = npairs < qtile_bound ? npairs : qtile_bound;
    long long gx = (2048 + tiles - 1) / tiles;
    const long long gmax = (max_list_rows + 1023) / 1024;
    gx = gx > gmax ? gmax : gx;
    gx = gx < 1 ? 1 : gx;
    ProfScope prof(EL::on ? "ivfpq_scan_elig" : "ivfpq_scan", 0.0, 0.0, st);
#define AMDREC_PQ_SCAN(MM)                                                                                                  \
    launch_with(el, pq_scan_for<MM, EL>(), dim3((unsigned)gx, (unsigned)qtile_bound), dim3(256), st, codes,                 \
                (const long long*)row_pos, (const long long*)list_off, (const long long*)list_finite, nlist,               \
                tables, nprobe, (const long long*)group_off, (const long long*)qtile_prefix, qtile,                        \
                (const long long*)pair_query,                                                                              \
                (const long long*)pair_probe, (const long long*)pool_base, (unsigned long long*)pool_keys, (long long)pool_ld, \
                (long long)pos_offset)
    switch (m) {
        case 4: AMDREC_PQ_SCAN(4); break;
        case 8: AMDREC_PQ_SCAN(8); break;
        case 16: AMDREC_PQ_SCAN(16); break;
        default: AMDREC_PQ_SCAN(32); break;
    }
#undef AMDREC_PQ_SCAN
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivfpq_scan(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off, int nlist,
                                 int64_t max_list_rows, const float* tables, int nprobe, const int64_t* group_off,
                                 const int64_t* qtile_prefix, int64_t qtile_bound, int qtile, const int64_t* pair_query,
                                 const int64_t* pair_probe, const int64_t* pool_base, int64_t npairs, uint64_t* pool_keys,
                                 int64_t pool_ld, int64_t pos_offset, void* stream) {
    return scan_impl(codes, m, row_pos, list_off, nullptr, nlist, max_list_rows, tables, nprobe, group_off, qtile_prefix,
                     qtile_bound, qtile, pair_query, pair_probe, pool_base, npairs, pool_keys, pool_ld, pos_offset, stream,
                     ListNoElig{});
}

extern "C" int amdrec_ivfpq_scan_finite(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off,
                                        const int64_t* list_finite, int nlist, int64_t max_list_rows, const float* tables,
                                        int nprobe, const int64_t* group_off, const int64_t* qtile_prefix,
                                        int64_t qtile_bound, int qtile, const int64_t* pair_query, const int64_t* pair_probe,
                                        const int64_t* pool_base, int64_t npairs, uint64_t* pool_keys, int64_t pool_ld,
                                        int64_t pos_offset, void* stream) {
    REQUIRE(list_finite != nullptr, "null pointer: list_finite");
    return scan_impl(codes, m, row_pos, list_off, list_finite, nlist, max_list_rows, tables, nprobe, group_off,
                     qtile_prefix, qtile_bound, qtile, pair_query, pair_probe, pool_base, npairs, pool_keys, pool_ld,
                     pos_offset, stream, ListNoElig{});
}

extern "C" int amdrec_ivfpq_scan_finite_eligible(const uint8_t* codes, int m, const int64_t* row_pos, const int64_t* list_off,
                                                 const int64_t* list_finite, int nlist, int64_t max_list_rows,
                                                 const float* tables, int nprobe, const int64_t* group_off,
                                                 const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                                                 const int64_t* pair_query, const int64_t* pair_probe,
                                                 const int64_t* pool_base, int64_t npairs, uint64_t* pool_keys,
                                                 int64_t pool_ld, int64_t pos_offset, void* stream,
                                                 const uint64_t* list_tags, const uint64_t* require_all,
                                                 const uint64_t* require_any) {
    REQUIRE(list_finite != nullptr, "null pointer: list_finite");
    return scan_impl(codes, m, row_pos, list_off, list_finite, nlist, max_list_rows, tables, nprobe, group_off,
                     qtile_prefix, qtile_bound, qtile, pair_query, pair_probe, pool_base, npairs, pool_keys, pool_ld,
                     pos_offset, stream, ListElig{list_tags, require_all, require_any});
}

extern "C" int amdrec_ivfpq_distances(const float* scores, int64_t nq, int k, float* distances, void* stream) {
    REQUIRE(k >= 1 && k <= AMDREC_MAX_K, "k=%d out of range [1, %d]", k, AMDREC_MAX_K);
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(scores && distances, "null pointer");
    const long long n = nq * (long long)k;
    hipLaunchKernelGGL(pq_negate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       scores, n, distances);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
