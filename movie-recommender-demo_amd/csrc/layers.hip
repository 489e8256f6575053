// Tower and ranker forward passes (eval mode) as chains of fp32-MFMA GEMMs with fused
// epilogues.  Orientation: P = weights [out_features][K] (the "small" operand, re-read from
// L2 by every block), Q = data rows [rows][K] (streamed once).  In the accumulator a LANE
// holds one data row and its REGISTERS hold output features, so per-row reductions
// (LayerNorm, L2 norm) are in-lane + one lane-half exchange + one 2-wave LDS exchange.
//
//   tower  (two_tower_model.py:98-121 / :167-184): gather+concat -> [Linear+BN(folded)+ReLU]*n
//                                                  -> Linear -> L2 normalise
//   ranker (transformer_ranker.py:332-380): gather+concat -> Linear(+pos[0]) ->
//          3x { x = LN(x + W_o(W_v x)) ; x = LN(x + W_2 relu(W_1 x)) } -> 3x cross -> 3 heads
//          (seq_len == 1, :358, makes the attention exactly W_o(W_v x + b_v) + b_o: SURVEY fact 1)
#include <type_traits>
#include "gemm_core.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

using ShapeWide = Shape<2, 2, 4, 2>;    // 256 features x 128 rows per workgroup (4 waves)
using ShapeNarrow = Shape<2, 2, 1, 4>;  //  64 features x 256 rows per workgroup
// Small batches (a single request = 500 candidate rows): with the shapes above a layer occupies 4 CUs and
// every wave runs a 128-MFMA chain per K-step (~40 us per 256x256 layer).  These shapes give each of 8
// waves ONE 32x32 tile: 16 workgroups for 500 rows and a 16-MFMA chain per K-step.
using ShapeSmall = Shape<8, 1, 1, 1>;        // 256 features x 32 rows, 8 waves
using ShapeSmallNarrow = Shape<2, 4, 1, 1>;  //  64 features x 128 rows, 8 waves
constexpr long long SMALL_ROWS = 8192;       // rows <= this use the small shapes

// Epilogue data movement.  In the accumulator a lane owns row q(j) and, per tile i and register group g,
// the 4 consecutive features 32*i + 8*g + 4*(lane>>5) + {0..3}: a direct store instruction would cover
// 32 rows x 32 bytes (quarter cache lines).  Instead every 32x32 tile goes through a wave-private 4 KB
// LDS tile (16-byte chunk index XOR (row & 7): conflict-free both ways) so that each global store / load
// instruction moves 8 rows x 128 bytes = whole cache lines (measured on the layer shapes: +4.5 % at
// K = 1024, +5 % at K = 256, +7.5 % for the 1024-wide FFN output; tools/gemm_probe.hip).
// LDS instructions of one wave execute in order, so the tile needs no barrier.
#define AMDREC_EPI_FENCE() asm volatile("" ::: "memory")   // bounds the loads in flight (register pressure)
#define FOFF(i, g) ((i) * 32 + (g) * 8)
constexpr int EPI_TILE_FLOATS = 1024;        // 32 rows x 32 floats per wave
constexpr int EPI_TILE_BASE = 1024;          // floats reserved below the tiles for row reductions
constexpr size_t epi_lds_bytes(int nwaves) { return (size_t)(EPI_TILE_BASE + nwaves * EPI_TILE_FLOATS) * sizeof(float); }

struct WaveTile {
    float* t;
    int r, h, lr, lc;                         // acc view: row r, half h;  line view: row lr (+8*pass), chunk lc
    __device__ __forceinline__ WaveTile(float* smem, int lane)
        : t(smem + EPI_TILE_BASE + (threadIdx.x >> 6) * EPI_TILE_FLOATS), r(lane & 31), h(lane >> 5), lr(lane >> 3),
          lc(lane & 7) {}
    __device__ __forceinline__ void put_acc(const f32x4 (&v)[4]) {
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(t + r * 32 + (((2 * g + h) ^ (r & 7)) << 2)) = v[g];
    }
    __device__ __forceinline__ void get_acc(f32x4 (&v)[4]) const {
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = *reinterpret_cast<const f32x4*>(t + r * 32 + (((2 * g + h) ^ (r & 7)) << 2));
    }
    __device__ __forceinline__ f32x4 get_line(int pass) const {
        const int row = lr + 8 * pass;
        return *reinterpret_cast<const f32x4*>(t + row * 32 + ((lc ^ (row & 7)) << 2));
    }
    __device__ __forceinline__ void put_line(int pass, f32x4 v) {
        const int row = lr + 8 * pass;
        *reinterpret_cast<f32x4*>(t + row * 32 + ((lc ^ (row & 7)) << 2)) = v;
    }
};

// full-line store of one 32x32 tile held in acc layout `v`: rows row0.., features feat0..
template <bool FULL>
__device__ __forceinline__ void tile_store(WaveTile& wt, const f32x4 (&v)[4], float* out, long long ld, long long row0,
                                           long long rows, int feat0, int nout) {
    wt.put_acc(v);
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const f32x4 line = wt.get_line(pass);
        const long long row = row0 + wt.lr + 8 * pass;
        const int f = feat0 + wt.lc * 4;
        if (row < rows && (FULL || f < nout)) *reinterpret_cast<f32x4*>(out + row * ld + f) = line;
    }
}
// full-line load of one 32x32 tile into acc layout (rows past the end are clamped, features masked)
template <bool FULL>
__device__ __forceinline__ void tile_load(WaveTile& wt, f32x4 (&v)[4], const float* src, long long ld, long long row0,
                                          long long rows, int feat0, int nout) {
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        long long row = row0 + wt.lr + 8 * pass;
        row = row < rows ? row : rows - 1;
        const int f = feat0 + wt.lc * 4;
        const f32x4 line = (FULL || f < nout) ? *reinterpret_cast<const f32x4*>(src + row * ld + f)
                                              : f32x4{0.f, 0.f, 0.f, 0.f};
        wt.put_line(pass, line);
    }
    wt.get_acc(v);
}

// what launch_gemm asks of these epilogues: each writes one fp32 per output element through the wave tiles above
struct EpiTiled {
    static constexpr double out_bytes_per_elem = 1.0;
    static constexpr size_t lds_bytes(int nwaves) { return epi_lds_bytes(nwaves); }
};
// Every epilogue EpiXT<FULL> derives from a plain struct XArgs: the kernel arguments, which a call site of linear() names
// field by field (rows and nout apart: the dispatcher fills those in), and the epilogue template the dispatcher instantiates.
template <bool> struct EpiLinearT;   template <bool> struct EpiRowBiasT;   template <bool> struct EpiCrossT;
template <bool> struct EpiResidualLNT;   template <bool> struct EpiL2NormT;

struct LinearArgs {
    template <bool FULL> using Epi = EpiLinearT<FULL>;
    const float* bias;
    float* out;
    long long ldo;
    long long rows;
    int nout;
    int relu;
};
// out[row][f] = act(acc + bias[f])
template <bool FULL>
struct EpiLinearT : LinearArgs, EpiTiled {
    static constexpr const char* name = "linear";
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
        WaveTile wt(smem, lane);
        const int f0 = acc.p(0, 0, lane);
        const float* bp = bias + f0;
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            f32x4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = (FULL || f0 + FOFF(i, g) < nout) ? *reinterpret_cast<const f32x4*>(bp + FOFF(i, g))
                                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                f32x4 v[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = acc.v[i][j][4 * g + e] + b[g][e];
                        v[g][e] = relu ? relu_keep_nan(x) : x;
                    }
                tile_store<FULL>(wt, v, out, ldo, (long long)acc.q0 + j * 32, rows, acc.p0 + i * 32, nout);
            }
        }
    }
};

// out[row][f] = acc + ubias[row / rowdiv][f]: the candidate (ad) half of the feature projection plus its
// user's precomputed half (which already carries the bias and positional row)
struct RowBiasArgs {
    template <bool FULL> using Epi = EpiRowBiasT<FULL>;
    const float* ubias;     // [n_users][ld]
    float* out;
    long long ld;
    long long rows;
    long long row_base;     // global index of the chunk's first row
    int rowdiv;
    int nout;
};
template <bool FULL>
struct EpiRowBiasT : RowBiasArgs, EpiTiled {
    static constexpr const char* name = "linear";
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
        WaveTile wt(smem, lane);
        const int f0 = acc.p(0, 0, lane);
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            long long row = acc.q(j, lane);
            row = row < rows ? row : rows - 1;
            const float* up = ubias + ((row_base + row) / rowdiv) * ld + f0;
#pragma unroll
            for (int i = 0; i < TP; ++i) {
                f32x4 v[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 u = (FULL || f0 + FOFF(i, g) < nout) ? *reinterpret_cast<const f32x4*>(up + FOFF(i, g))
                                                                     : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[g][e] = acc.v[i][j][4 * g + e] + u[e];
                }
                tile_store<FULL>(wt, v, out, ld, (long long)acc.q0 + j * 32, rows, acc.p0 + i * 32, nout);
            }
        }
    }
};

// out[row][f] = x0[row][f] * (acc + bias[f]) + xl[row][f]     (FeatureInteractionLayer :201)
struct CrossArgs {
    template <bool FULL> using Epi = EpiCrossT<FULL>;
    const float* bias;
    const float* x0;
    const float* xl;
    float* out;
    long long ld;
    long long rows;
    int nout;
};
template <bool FULL>
struct EpiCrossT : CrossArgs, EpiTiled {
    static constexpr const char* name = "cross";
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
        WaveTile wt(smem, lane);
        const int f0 = acc.p(0, 0, lane);
        const float* bp = bias + f0;
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            f32x4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = (FULL || f0 + FOFF(i, g) < nout) ? *reinterpret_cast<const f32x4*>(bp + FOFF(i, g))
                                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                const long long row0 = (long long)acc.q0 + j * 32;
                f32x4 a0[4], al[4], v[4];
                tile_load<FULL>(wt, a0, x0, ld, row0, rows, acc.p0 + i * 32, nout);
                tile_load<FULL>(wt, al, xl, ld, row0, rows, acc.p0 + i * 32, nout);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[g][e] = a0[g][e] * (acc.v[i][j][4 * g + e] + b[g][e]) + al[g][e];
                tile_store<FULL>(wt, v, out, ld, row0, rows, acc.p0 + i * 32, nout);
                AMDREC_EPI_FENCE();
            }
        }
    }
};

// Row statistics over the nout (<= 256) features of a row.  The workgroup is one P tile wide
// (ShapeWide: 2 waves x 128 features), so: in-lane sum over the lane's 64 values, exchange
// with lane^32 (other row-group half of the same tiles), exchange between the 2 feature
// waves through LDS.  `red` is [2 phases][WP][BQ rows] (<= EPI_TILE_BASE floats).
template <int TQ, int BQ, int WP>
__device__ __forceinline__ void row_allreduce(float (&part)[TQ], float* red, int phase, int wp, int wq, int lane) {
    static_assert(2 * WP * BQ <= EPI_TILE_BASE, "reduction scratch overlaps the epilogue tiles");
#pragma unroll
    for (int j = 0; j < TQ; ++j) part[j] += __shfl_xor(part[j], 32, 64);
    float* r = red + phase * WP * BQ;
    if (lane < 32) {
#pragma unroll
        for (int j = 0; j < TQ; ++j) r[wp * BQ + wq * TQ * 32 + j * 32 + lane] = part[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
        const int idx = wq * TQ * 32 + j * 32 + (lane & 31);
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < WP; ++w) a += r[w * BQ + idx];     // fixed order: deterministic
        part[j] = a;
    }
}

// out = LayerNorm(resid + acc + bias) * gamma + beta   (transformer_ranker.py:149, :153; eps 1e-5)
struct ResidualLNArgs {
    template <bool FULL> using Epi = EpiResidualLNT<FULL>;
    const float* bias;
    const float* resid;
    const float* gamma;
    const float* beta;
    float* out;
    long long ld;
    long long rows;
    int nout;
    float eps;
};
template <bool FULL>
struct EpiResidualLNT : ResidualLNArgs, EpiTiled {
    static constexpr const char* name = "residual_ln";
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        static_assert(A::WP * TP * 32 == 256, "LayerNorm epilogue: the workgroup spans one 256-feature P tile");
        const int lane = threadIdx.x & 63;
        const int wp = acc.wp, wq = acc.wq;
        WaveTile wt(smem, lane);
        const int f0 = acc.p(0, 0, lane);
        const float* bp = bias + f0;
        float s[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) s[j] = 0.f;
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            f32x4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = (FULL || f0 + FOFF(i, g) < nout) ? *reinterpret_cast<const f32x4*>(bp + FOFF(i, g))
                                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                f32x4 rs[4];
                tile_load<FULL>(wt, rs, resid, ld, (long long)acc.q0 + j * 32, rows, acc.p0 + i * 32, nout);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bool fv = FULL || f0 + FOFF(i, g) < nout;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = fv ? acc.v[i][j][4 * g + e] + b[g][e] + rs[g][e] : 0.f;
                        acc.v[i][j][4 * g + e] = x;
                        s[j] += x;
                    }
                }
            }
            AMDREC_EPI_FENCE();
        }
        row_allreduce<TQ, A::BQ, A::WP>(s, smem, 0, wp, wq, lane);
        const float inv_n = 1.0f / (float)nout;
        float mean[TQ], q2[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            mean[j] = s[j] * inv_n;
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bool fv = FULL || f0 + FOFF(i, g) < nout;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float dlt = fv ? acc.v[i][j][4 * g + e] - mean[j] : 0.f;
                        a += dlt * dlt;
                    }
                }
            q2[j] = a;
        }
        row_allreduce<TQ, A::BQ, A::WP>(q2, smem, 1, wp, wq, lane);
        float rstd[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) rstd[j] = 1.0f / sqrtf(q2[j] * inv_n + eps);
        const float* gp = gamma + f0;
        const float* tp = beta + f0;
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            f32x4 ga[4], be[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bool fv = FULL || f0 + FOFF(i, g) < nout;
                ga[g] = fv ? *reinterpret_cast<const f32x4*>(gp + FOFF(i, g)) : f32x4{0.f, 0.f, 0.f, 0.f};
                be[g] = fv ? *reinterpret_cast<const f32x4*>(tp + FOFF(i, g)) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                f32x4 v[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        v[g][e] = (acc.v[i][j][4 * g + e] - mean[j]) * rstd[j] * ga[g][e] + be[g][e];
                tile_store<FULL>(wt, v, out, ld, (long long)acc.q0 + j * 32, rows, acc.p0 + i * 32, nout);
            }
            AMDREC_EPI_FENCE();
        }
    }
};

// out = (acc + bias) / max(||acc + bias||_2, eps)      (F.normalize, two_tower_model.py:119)
struct L2NormArgs {
    template <bool FULL> using Epi = EpiL2NormT<FULL>;
    const float* bias;
    float* out;
    long long ldo;
    long long rows;
    int nout;
    float eps;
};
template <bool FULL>
struct EpiL2NormT : L2NormArgs, EpiTiled {
    static constexpr const char* name = "l2norm";
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        static_assert(A::WP * TP * 32 == 256, "L2-norm epilogue: the workgroup spans one 256-feature P tile");
        const int lane = threadIdx.x & 63;
        const int wp = acc.wp, wq = acc.wq;
        WaveTile wt(smem, lane);
        const int f0 = acc.p(0, 0, lane);
        const float* bp = bias + f0;
        float s[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) s[j] = 0.f;
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            f32x4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = (FULL || f0 + FOFF(i, g) < nout) ? *reinterpret_cast<const f32x4*>(bp + FOFF(i, g))
                                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < TQ; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bool fv = FULL || f0 + FOFF(i, g) < nout;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = fv ? acc.v[i][j][4 * g + e] + b[g][e] : 0.f;
                        acc.v[i][j][4 * g + e] = x;
                        s[j] += x * x;
                    }
                }
            AMDREC_EPI_FENCE();
        }
        row_allreduce<TQ, A::BQ, A::WP>(s, smem, 0, wp, wq, lane);
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const float inv = 1.0f / fmaxf(sqrtf(s[j]), eps);
#pragma unroll
            for (int i = 0; i < TP; ++i) {
                f32x4 v[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[g][e] = acc.v[i][j][4 * g + e] * inv;
                tile_store<FULL>(wt, v, out, ldo, (long long)acc.q0 + j * 32, rows, acc.p0 + i * 32, nout);
            }
        }
    }
};

// out[row] = dot(h[row][0..n), w) + b   (last Linear(64,1) of a prediction head + squeeze)
__global__ __launch_bounds__(256) void rowdot_kernel(const float* h, long long ldh, int n, const float* w,
                                                     const float* b, float* out, long long rows) {
    // 16 lanes per row, float4 each
    const long long row = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int sub = threadIdx.x & 15;
    float a = 0.f;
    if (row < rows) {
        for (int c = sub * 4; c < n; c += 64) {
            f32x4 x = *reinterpret_cast<const f32x4*>(h + row * ldh + c);
            f32x4 y = *reinterpret_cast<const f32x4*>(w + c);
            a += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (row < rows && sub == 0) out[row] = a + b[0];
}

// Validate categorical indices (torch raises IndexError; a kernel must not fault): flag = 1
// if any index is outside [0, card).  The loaders clamp, so nothing reads out of bounds.
__global__ void check_index_kernel(const long long* cat, long long rows, int F, const int* card, int* flag) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * F) return;
    long long v = cat[i];
    if (v < 0 || v >= card[i % F]) *flag = 1;
}

static void launch_check_index(const int64_t* cat, long long rows, int F, const int* card, int* flag, hipStream_t st) {
    hipLaunchKernelGGL(check_index_kernel, dim3((unsigned)((rows * F + 255) / 256)), dim3(256), 0, st, (const long long*)cat,
                       rows, F, card, flag);
}

// ad_rowmap against the ad table on the checked path: a row >= n_rows is out of range (the reference's ad_table[cand] raises);
// a negative row means "no candidate" (an unfilled search slot) and is not an error
__global__ void check_rowmap_kernel(const long long* rowmap, long long n, long long n_rows, int* flag) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (rowmap[i] >= n_rows) *flag = 1;
}

static inline DenseRows dense(const float* p, long long rows, long long ld, int K) {
    return DenseRows{p, rows, (int)ld, K, 30, 1ll << 30};
}
// the un-padded K of a row source (the profile hook's FLOP count)
static inline int k_of(const DenseRows& r) { return r.K; }
static inline int k_of(const EmbConcatRows& g) { return g.F * g.E + g.n_num; }

// The weights of one layer, [nout][ld] fp32.  WeightsX6 adds the host-split bf16 planes of the error-compensated path
// (gemm_core.hpp "x6"; null when the engine is fp32): only a call that passes this type has x6 kernels at all.
struct Weights { const float* w; int ld; };
struct WeightsX6 { const float* w; const uint16_t* x6; int ld; };
// narrow outputs (<= 64 features) may use the 64-feature shapes, unless the call wants a whole 256-feature row in one
// workgroup whatever nout is (the projections; the LayerNorm and L2-norm epilogues, which need it)
enum Tiles { ANY_WIDTH, WIDE_ONLY };

// FULL = the width fills whole P tiles, so the epilogue needs no feature-bound checks (true for every layer of the default
// architecture): launch(EpiXT<full>{a})
template <class Args, class Launch>
static hipError_t with_epilogue(bool full, const Args& a, Launch launch) {
    return full ? launch(typename Args::template Epi<true>{a}) : launch(typename Args::template Epi<false>{a});
}
template <class S, class LoadQ, class Args>
static hipError_t linear_tiles(const float* W, int ldw, const LoadQ& lq, const Args& a, hipStream_t st) {
    return with_epilogue(a.nout % S::BP == 0, a, [&](const auto& epi) {
        return launch_gemm<S, true>(dense(W, a.nout, ldw, ldw), lq, epi, ldw, a.nout, a.rows, st, k_of(lq));
    });
}
// y = epilogue(x W^T) for the rows of `lq`: the epilogue's arguments by name, rows and nout filled in here.  Dispatch on the
// row count (small shapes up to SMALL_ROWS), the output width and - with planes, a dense fp32 row operand and at least one
// full 256-feature tile - the x6 path for the big passes.
template <Tiles TILES, class W, class LoadQ, class Args>
static hipError_t linear(const W& w, int nout, const LoadQ& lq, hipStream_t st, Args a) {
    a.rows = lq.rows;
    a.nout = nout;
    if constexpr (std::is_same<W, WeightsX6>::value) {
        static_assert(std::is_same<LoadQ, DenseRows>::value, "the x6 kernels stage dense fp32 rows");
        if (w.x6 != nullptr && a.rows > SMALL_ROWS && nout >= 256)
            return with_epilogue(nout % 256 == 0, a, [&](const auto& epi) {
                return launch_gemm_x6(w.x6, nout, lq, epi, w.ld, a.rows, st, k_of(lq));
            });
    }
    if constexpr (TILES == ANY_WIDTH) {
        if (nout <= 64)
            return a.rows <= SMALL_ROWS ? linear_tiles<ShapeSmallNarrow>(w.w, w.ld, lq, a, st)
                                        : linear_tiles<ShapeNarrow>(w.w, w.ld, lq, a, st);
    }
    return a.rows <= SMALL_ROWS ? linear_tiles<ShapeSmall>(w.w, w.ld, lq, a, st) : linear_tiles<ShapeWide>(w.w, w.ld, lq, a, st);
}

// Rows per pass.  A 256-feature layer launches rows/256 workgroups, so a pass must be >= 65536 rows to
// give every one of the 256 CUs a block and several times that to keep the last wave of blocks full
// (measured: 32768-row passes left half the chip idle, 45-74 TF; fp32 GEMMs are MFMA-bound, not
// HBM-bound, so keeping a pass inside the Infinity Cache buys nothing here).
constexpr long long ROW_CHUNK = 262144;

}  // namespace amdrec

using namespace amdrec;

// ============================== towers ==============================================
static int tower_check(const amdrec_tower_params* p) {
    REQUIRE(p != nullptr, "params is null");
    REQUIRE(p->n_feat >= 1 && p->n_feat <= 64, "n_feat out of range");
    REQUIRE(p->emb_dim >= 4 && (p->emb_dim & (p->emb_dim - 1)) == 0, "emb_dim must be a power of two >= 4");
    REQUIRE(p->n_num >= 0, "n_num < 0");
    REQUIRE(p->n_layers >= 1 && p->n_layers <= AMDREC_MAX_LAYERS, "n_layers out of range");
    REQUIRE(p->dims[0] == p->n_feat * p->emb_dim + p->n_num, "dims[0] != n_feat*emb_dim + n_num");
    for (int l = 0; l < p->n_layers; ++l) {
        REQUIRE(p->dims[l + 1] >= 4 && p->dims[l + 1] % 4 == 0, "layer width must be a multiple of 4");
        REQUIRE(p->ldw[l] % 32 == 0 && p->ldw[l] >= p->dims[l], "ldw must be a multiple of 32 and >= K");
        REQUIRE(p->w[l] && p->b[l], "null weight pointer");
    }
    REQUIRE(p->dims[p->n_layers] <= 256, "output_dim > 256 is not supported by the fused L2-norm epilogue");
    REQUIRE(p->tables && p->table_off && p->cards, "null table pointer");
    return AMDREC_OK;
}

// two ping-pong buffers of one row chunk at the widest hidden layer
struct TowerWs : Carver {
    float* bufs[2]; long long chunk;
    TowerWs(const amdrec_tower_params* p, long long rows, void* ws) : Carver(ws) {
        chunk = rows < ROW_CHUNK ? rows : ROW_CHUNK;
        int wmax = 4;
        for (int l = 1; l < p->n_layers; ++l) wmax = p->dims[l] > wmax ? p->dims[l] : wmax;
        for (float*& b : bufs) b = take<float>((size_t)chunk * wmax);
    }
};

extern "C" int amdrec_tower_workspace(const amdrec_tower_params* p, int64_t rows, size_t* bytes) {
    int rc = tower_check(p);
    if (rc) return rc;
    REQUIRE(bytes && rows >= 0, "bad arguments");
    *bytes = TowerWs(p, rows, nullptr).bytes();
    return AMDREC_OK;
}

namespace amdrec {   // tower_small.hip: the whole tower in one launch for batches of <= 4096 rows
bool tower_small_ok(const amdrec_tower_params* p, long long rows);
hipError_t tower_small_run(const amdrec_tower_params* p, const long long* cat, const float* num, long long rows, float* out,
                           long long ld_out, hipStream_t st);
}

extern "C" int amdrec_tower_forward(const amdrec_tower_params* p, const int64_t* cat, const float* num,
                                    int64_t rows, float* out, int64_t ld_out, int* bad_index_flag,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    int rc = tower_check(p);
    if (rc) return rc;
    if (rows <= 0) return AMDREC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    REQUIRE(cat && out && (num || p->n_num == 0), "null pointer");
    REQUIRE(ld_out % 4 == 0 && ld_out >= p->dims[p->n_layers], "bad ld_out");
    const TowerWs w(p, rows, workspace);
    if ((rc = require_workspace(workspace, workspace_bytes, w.bytes()))) return rc;
    if (bad_index_flag) launch_check_index(cat, rows, p->n_feat, p->cards, bad_index_flag, st);
    if (tower_small_ok(p, rows)) {                      // serving batches: one launch for the whole tower
        HIP_TRY(tower_small_run(p, (const long long*)cat, num, rows, out, (long long)ld_out, st));
        return AMDREC_OK;
    }
    for (long long r0 = 0; r0 < rows; r0 += w.chunk) {
        const long long m = rows - r0 < w.chunk ? rows - r0 : w.chunk;
        for (int l = 0; l < p->n_layers; ++l) {
            const int nout = p->dims[l + 1];
            const Weights W{p->w[l], p->ldw[l]};
            // a hidden layer writes relu(.) to its ping-pong buffer, the last layer the normalised rows to `out`
            auto layer = [&](const auto& in) {
                if (l == p->n_layers - 1)
                    return linear<WIDE_ONLY>(W, nout, in, st,
                                             L2NormArgs{.bias = p->b[l], .out = out + r0 * ld_out, .ldo = ld_out, .eps = 1e-12f});
                return linear<ANY_WIDTH>(W, nout, in, st,
                                         LinearArgs{.bias = p->b[l], .out = w.bufs[l & 1], .ldo = nout, .relu = 1});
            };
            // layer 0 gathers its rows from the tables, every other layer reads the previous one's buffer
            if (l == 0) HIP_TRY(layer(EmbConcatRows::tower_rows(p, (const long long*)cat, num, r0, m)));
            else HIP_TRY(layer(dense(w.bufs[(l - 1) & 1], m, p->dims[l], p->dims[l])));
        }
    }
    if (p->renormalize)                                   // the general path: a second launch (amdrec_l2_normalize in place)
        return amdrec_l2_normalize(out, ld_out, out, ld_out, rows, p->dims[p->n_layers], stream);
    return AMDREC_OK;
}

// ============================== ranker ==============================================
namespace amdrec {   // ranker_x3.hip: the fp16x3 row-owner engine (everything after the feature projection in one kernel)
bool ranker_x3_wanted(const amdrec_ranker_params* p, long long rows);
bool ranker_x3_folded(const amdrec_ranker_params* p);
bool ranker_x3_hidden_cache(const amdrec_ranker_params* p, long long rows);
bool ranker_x3_ctr_first_supported(const amdrec_ranker_params* p, long long rows, long long row_chunk);
size_t ranker_x3_winner_workspace(const amdrec_ranker_params* p, long long rows);
int ranker_x3_run(const amdrec_ranker_params* p, const float* X, long long ldx, const float* U, long long ldu,
                  const long long* rowmap, long long row_base, int rowdiv, long long n_cache, long long rows, float* scratch,
                  float* logits, long long ld_logits, hipStream_t st, bool ctr_first = false, float* x_out = nullptr,
                  long long ld_xout = 0);
}
static int ranker_check(const amdrec_ranker_params* p) {
    REQUIRE(p != nullptr, "params is null");
    REQUIRE(p->n_user_feat >= 0 && p->n_ad_feat >= 0 && p->n_user_feat + p->n_ad_feat >= 1 &&
                p->n_user_feat + p->n_ad_feat <= 128, "feature counts out of range");
    REQUIRE(p->emb_dim >= 4 && (p->emb_dim & (p->emb_dim - 1)) == 0, "emb_dim must be a power of two >= 4");
    REQUIRE(p->d_model >= 4 && p->d_model % 4 == 0 && p->d_model <= 256, "d_model must be a multiple of 4, <= 256");
    REQUIRE(p->d_ff >= 4 && p->d_ff % 4 == 0, "d_ff must be a multiple of 4");
    REQUIRE(p->n_layers >= 0 && p->n_layers <= AMDREC_MAX_LAYERS, "n_layers out of range");
    REQUIRE(p->n_cross >= 0 && p->n_cross <= AMDREC_MAX_LAYERS, "n_cross out of range");
    REQUIRE(p->n_tasks >= 1 && p->n_tasks <= AMDREC_MAX_TASKS, "n_tasks out of range");
    REQUIRE(p->head_h1 % 4 == 0 && p->head_h2 % 4 == 0 && p->head_h1 >= 4 && p->head_h2 >= 4, "bad head widths");
    REQUIRE(p->tables && p->table_off && p->cards && p->w_proj && p->b_proj, "null pointer in params");
    return AMDREC_OK;
}

struct RankerWs : Carver {
    float *X, *T, *X0, *H, *U; long long chunk;
    RankerWs(const amdrec_ranker_params* p, long long rows, void* ws) : Carver(ws) {
        chunk = rows < ROW_CHUNK ? rows : ROW_CHUNK;
        if (chunk < 1) chunk = 1;
        const size_t dm = (size_t)chunk * p->d_model;
        long long hw = p->d_ff;
        long long headw = (long long)p->n_tasks * (p->head_h1 + p->head_h2);
        if (headw > hw) hw = headw;
        X = take<float>(dm);
        T = take<float>(dm);
        // X0 doubles as the row-owner engine's x0 scratch, which is addressed in whole 128-row workgroups
        X0 = take<float>((size_t)((chunk + 127) / 128 * 128) * p->d_model);
        H = take<float>((size_t)chunk * hw);
        U = take<float>((size_t)(rows > 0 ? rows : 0) * p->d_model);   // upper bound: one user row per batch row
    }
};

extern "C" int amdrec_ranker_workspace(const amdrec_ranker_params* p, int64_t rows, size_t* bytes) {
    int rc = ranker_check(p);
    if (rc) return rc;
    REQUIRE(bytes && rows >= 0, "bad arguments");
    *bytes = RankerWs(p, rows, nullptr).bytes();
    return AMDREC_OK;
}

// x0[r] = ad_proj_cache[ad row of r] + U[user of r]  (the cached form of the EpiRowBiasT projection: same addends,
// same order).  One wave per row.
__global__ __launch_bounds__(256) void proj_gather_kernel(const float* cache, long long ldc, long long n_cache,
                                                          const long long* rowmap, long long row_base, const float* U,
                                                          int dm, int rowdiv, float* X, long long m) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= m) return;
    const long long gr = row_base + r;
    long long a = rowmap ? rowmap[gr] : gr;
    a = a < 0 ? 0 : (a >= n_cache ? n_cache - 1 : a);        // clamped like the gather loader (a negative row = no candidate:
                                                             // amdrec_select_topk drops it; >= n_cache: check_rowmap_kernel)
    const f32x4* cp = reinterpret_cast<const f32x4*>(cache + a * ldc);
    const f32x4* up = reinterpret_cast<const f32x4*>(U + (gr / rowdiv) * dm);
    f32x4* xp = reinterpret_cast<f32x4*>(X + r * dm);
    for (int c = lane; c < (dm >> 2); c += 64) {
        const f32x4 a4 = cp[c], u4 = up[c];
        xp[c] = f32x4{a4[0] + u4[0], a4[1] + u4[1], a4[2] + u4[2], a4[3] + u4[3]};
    }
}

// out[a] = W . emb(ad_cat[a]) for a [nout][ldw_proj_ad] matrix over the ad embeddings (no bias)
static int project_ads(const amdrec_ranker_params* p, const float* W, int nout, const int64_t* ad_cat, int64_t n_ads,
                       float* out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = ranker_check(p);
    if (rc) return rc;
    if (n_ads <= 0) return AMDREC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int dm = nout;
    REQUIRE(W && p->n_ad_feat > 0, "params carry no split projection (w_proj_ad / x3.w_hidden_ad)");
    REQUIRE(ad_cat && out, "null pointer");
    REQUIRE(ld_out >= dm && ld_out % 4 == 0 && ((uintptr_t)out % 16) == 0, "bad output layout");
    REQUIRE(n_ads < (1ll << 31) - 1024, "n_ads out of range");
    if ((rc = require_workspace(workspace, workspace_bytes, align_up((size_t)dm * 4, 256)))) return rc;
    float* zero = static_cast<float*>(workspace);
    HIP_TRY(hipMemsetAsync(zero, 0, (size_t)dm * 4, st));
    // the same GEMM (shape, K order) as the uncached candidate half, with an all-zero "user row"
    const EmbConcatRows ga = EmbConcatRows::ranker_ad_rows(p, (const long long*)ad_cat, nullptr, n_ads, 0, n_ads);
    HIP_TRY(linear<WIDE_ONLY>(Weights{W, p->ldw_proj_ad}, dm, ga, st,
                              RowBiasArgs{.ubias = zero, .out = out, .ld = ld_out, .row_base = 0, .rowdiv = 0x7fffffff}));
    return AMDREC_OK;
}

extern "C" int amdrec_ranker_project_ads(const amdrec_ranker_params* p, const int64_t* ad_cat, int64_t n_ads,
                                         float* out, int64_t ld_out, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    REQUIRE(p != nullptr, "params is null");
    return project_ads(p, p->w_proj_ad, p->d_model, ad_cat, n_ads, out, ld_out, workspace, workspace_bytes, stream);
}

extern "C" int amdrec_ranker_project_ads_hidden(const amdrec_ranker_params* p, const int64_t* ad_cat, int64_t n_ads,
                                                float* out, int64_t ld_out, void* workspace, size_t workspace_bytes,
                                                void* stream) {
    REQUIRE(p != nullptr, "params is null");
    return project_ads(p, p->x3.w_hidden_ad, p->d_ff, ad_cat, n_ads, out, ld_out, workspace, workspace_bytes, stream);
}

// The user half of the projection for a handful of requests (hoisted form: U[u] = W_user [user emb | numerical] + b).  The tile
// GEMM spends 18 us on ONE user row (7 dependent k-steps of global load -> LDS -> MFMA on four workgroups).  Here a workgroup
// stages the user's 205 features in LDS and computes 32 output features, eight lanes per feature: the eight read 128
// contiguous bytes of the weight row per step (7 steps, all in flight), fp32 FMA chains, then a three-step lane reduction.
// (One thread per output feature reads its row alone: 64 cache lines per load instruction, 12 us on one CU.)
constexpr int USER_PROJ_SMALL_MAX = 64, USER_PROJ_SMALL_K = 256;     // users per call; features (8 steps of 32)
__global__ __launch_bounds__(256) void user_proj_small_kernel(EmbConcatRows g, const float* W, int ldw, int K, const float* bias,
                                                              float* U, int dm) {
    __shared__ __attribute__((aligned(16))) float feat[USER_PROJ_SMALL_K];
    const long long u = blockIdx.x;
    const int K4 = (K + 3) / 4 * 4;
    const int n = blockIdx.y * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
    const float* w = W + (long long)(n < dm ? n : dm - 1) * ldw;
    f32x4 wv[USER_PROJ_SMALL_K / 32];                              // the weight loads go out first: they do not depend on the
#pragma unroll                                                     // features, whose gather is two dependent loads deep
    for (int i = 0; i < USER_PROJ_SMALL_K / 32; ++i) {
        const int k = 4 * j + 32 * i;
        wv[i] = k < K4 ? *reinterpret_cast<const f32x4*>(w + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const EmbConcatRows::RowState rs = g.row_state(u);
    for (int k = threadIdx.x * 4; k < K4; k += 1024) *reinterpret_cast<f32x4*>(feat + k) = g.load(rs, k);
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < USER_PROJ_SMALL_K / 32; ++i) {
        const int k = 4 * j + 32 * i;
        const f32x4 x = k < K4 ? *reinterpret_cast<const f32x4*>(feat + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        a0 = __builtin_fmaf(wv[i][0], x[0], a0);
        a1 = __builtin_fmaf(wv[i][1], x[1], a1);
        a2 = __builtin_fmaf(wv[i][2], x[2], a2);
        a3 = __builtin_fmaf(wv[i][3], x[3], a3);
    }
    float a = (a0 + a1) + (a2 + a3);
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    a += __shfl_xor(a, 4, 64);
    if (j == 0 && n < dm) U[u * dm + n] = a + bias[n];
}

// What the parts of amdrec_ranker_forward share
struct RankerCtx {
    const amdrec_ranker_params* p;
    hipStream_t st;
    float *X, *T, *X0, *H, *U;     // RankerWs
    int dm;
    bool hoist;                    // split projection: the user half once per user row (U), the ad half per candidate
    int du;                        // width and leading dimension of U's rows
};

// U[u] = W_user [user emb(u) | numerical(u)] + b_proj (+ pos[0]): once per user row; rows [U | Q] when du == dm + d_ff
static int ranker_user_projection(const RankerCtx& c, const int64_t* user_cat, const float* numerical, long long n_users) {
    const amdrec_ranker_params* p = c.p;
    const bool with_q = c.du != c.dm;
    const float* w_user = with_q ? p->x3.w_user_uq : p->w_proj_user;
    const float* b_user = with_q ? p->x3.b_user_uq : p->b_proj;
    const EmbConcatRows gu = EmbConcatRows::ranker_user_rows(p, (const long long*)user_cat, numerical, n_users);
    const int Ku = k_of(gu), K4 = (Ku + 3) / 4 * 4;
    if (n_users <= USER_PROJ_SMALL_MAX && K4 <= USER_PROJ_SMALL_K && p->ldw_proj_user >= K4) {
        ProfScope prof("user_proj_small", 2.0 * n_users * c.du * Ku, (double)c.du * Ku * 4, c.st);
        hipLaunchKernelGGL(user_proj_small_kernel, dim3((unsigned)n_users, (unsigned)((c.du + 31) / 32)), dim3(256), 0, c.st, gu,
                           w_user, (int)p->ldw_proj_user, Ku, b_user, c.U, c.du);
        HIP_TRY(hipGetLastError());
        return AMDREC_OK;
    }
    HIP_TRY(linear<WIDE_ONLY>(Weights{w_user, p->ldw_proj_user}, c.du, gu, c.st,
                              LinearArgs{.bias = b_user, .out = c.U, .ldo = c.du, .relu = 0}));
    return AMDREC_OK;
}

// X = the feature projection (+ pos[0], folded into b_proj on the host) of one pass's rows `g`
static int ranker_project_rows(const RankerCtx& c, const EmbConcatRows& g) {
    const amdrec_ranker_params* p = c.p;
    if (c.hoist && p->ad_proj_cache) {
        hipLaunchKernelGGL(proj_gather_kernel, dim3((unsigned)((g.rows + 3) / 4)), dim3(256), 0, c.st, p->ad_proj_cache,
                           (long long)p->ld_ad_proj_cache, g.rows1, g.rowmap1, g.row_base, (const float*)c.U, c.dm,
                           g.cat0_rowdiv, c.X, g.rows);
    } else if (c.hoist) {
        // candidate half: ad embeddings only (K = n_ad_feat * emb_dim), plus the user's row of U
        HIP_TRY(linear<WIDE_ONLY>(Weights{p->w_proj_ad, p->ldw_proj_ad}, c.dm,
                                  EmbConcatRows::ranker_ad_rows(p, g.cat1, g.rowmap1, g.rows1, g.row_base, g.rows), c.st,
                                  RowBiasArgs{.ubias = c.U, .out = c.X, .ld = c.dm, .row_base = g.row_base,
                                              .rowdiv = g.cat0_rowdiv}));
    } else {
        HIP_TRY(linear<WIDE_ONLY>(Weights{p->w_proj, p->ldw_proj}, c.dm, g, c.st,
                                  LinearArgs{.bias = p->b_proj, .out = c.X, .ldo = c.dm, .relu = 0}));
    }
    return AMDREC_OK;
}

// The layer-by-layer engine on the m projected rows in X: encoder layers, cross layers, heads -> logits[t * ld_logits + row]
static int ranker_layer_chain(const RankerCtx& c, long long m, float* logits, long long ld_logits) {
    const amdrec_ranker_params* p = c.p;
    const hipStream_t st = c.st;
    const int dm = c.dm, dff = p->d_ff;
    float *X = c.X, *T = c.T;
    for (int l = 0; l < p->n_layers; ++l) {
        const amdrec_encoder_layer& L = p->layers[l];
        const WeightsX6 w_o{L.w_o, L.w_o_x6, L.ldw_dm};
        ResidualLNArgs ln1{.bias = L.b_o, .resid = X, .gamma = L.ln1_g, .beta = L.ln1_b, .out = X, .ld = dm, .eps = p->ln_eps};
        if (L.w_v != nullptr) {
            // T = W_v x + b_v ; X = LN1(X + W_o T + b_o)
            HIP_TRY(linear<WIDE_ONLY>(Weights{L.w_v, L.ldw_dm}, dm, dense(X, m, dm, dm), st,
                                      LinearArgs{.bias = L.b_v, .out = T, .ldo = dm, .relu = 0}));
            HIP_TRY(linear<WIDE_ONLY>(w_o, dm, dense(T, m, dm, dm), st, ln1));
        } else {
            // host pre-multiplied W_ov = W_o W_v: LN1(X + W_ov X + b_ov), written to the spare buffer
            ln1.out = T;
            HIP_TRY(linear<WIDE_ONLY>(w_o, dm, dense(X, m, dm, dm), st, ln1));
            float* tmp = X; X = T; T = tmp;
        }
        // H = relu(W_1 X + b_1)
        HIP_TRY(linear<ANY_WIDTH>(WeightsX6{L.w_1, L.w_1_x6, L.ldw_dm}, dff, dense(X, m, dm, dm), st,
                                  LinearArgs{.bias = L.b_1, .out = c.H, .ldo = dff, .relu = 1}));
        // X = LN2(X + W_2 H + b_2)
        HIP_TRY(linear<WIDE_ONLY>(WeightsX6{L.w_2, L.w_2_x6, L.ldw_ff}, dm, dense(c.H, m, dff, dff), st,
                                  ResidualLNArgs{.bias = L.b_2, .resid = X, .gamma = L.ln2_g, .beta = L.ln2_b, .out = X, .ld = dm,
                                                 .eps = p->ln_eps}));
    }
    // ---- cross layers: xl <- x0 * (xl W_i + b_i) + xl ; x0 = X ----
    const float* xl = X;
    for (int i = 0; i < p->n_cross; ++i) {
        float* dst = (i & 1) ? c.X0 : T;
        HIP_TRY(linear<WIDE_ONLY>(WeightsX6{p->cross_wt[i], p->cross_wt_x6[i], p->ldw_cross}, dm, dense(xl, m, dm, dm), st,
                                  CrossArgs{.bias = p->cross_b[i], .x0 = X, .xl = xl, .out = dst, .ld = dm}));
        xl = dst;
    }
    // ---- heads ----
    const int h1 = p->head_h1, h2 = p->head_h2, nt = p->n_tasks;
    float* H1 = c.H;                                 // [m][nt*h1]
    float* H2 = c.H + (size_t)m * nt * h1;           // [m][nt*h2]
    HIP_TRY(linear<ANY_WIDTH>(WeightsX6{p->head_w1, p->head_w1_x6, p->ldw_head1}, nt * h1, dense(xl, m, dm, dm), st,
                              LinearArgs{.bias = p->head_b1, .out = H1, .ldo = nt * h1, .relu = 1}));
    for (int t = 0; t < nt; ++t) {
        HIP_TRY(linear<ANY_WIDTH>(Weights{p->head_w2[t], p->ldw_head2}, h2, dense(H1 + t * h1, m, (long long)nt * h1, h1), st,
                                  LinearArgs{.bias = p->head_b2[t], .out = H2 + t * h2, .ldo = nt * h2, .relu = 1}));
        hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)((m * 16 + 255) / 256)), dim3(256), 0, st, H2 + t * h2, (long long)nt * h2,
                           h2, p->head_w3[t], p->head_b3[t], logits + (long long)t * ld_logits, m);
    }
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

// amdrec_ranker_forward, and (ctr_first) amdrec_ranker_forward_ctr_first: the same pass loop, hoisted user projection, cached
// gather and program selection; the CTR-first form runs the trunk and the head of task 0 alone on every pass (out_logits:
// that one row) and keeps each row's trunk state in trunk_out
static int ranker_forward(const amdrec_ranker_params* p, const int64_t* user_cat, const float* numerical,
                          int64_t user_rowdiv, const int64_t* ad_cat, const int64_t* ad_rowmap, int64_t rows,
                          float* out_logits, int64_t ld_logits, int* bad_index_flag, int64_t n_user_rows, int64_t n_ad_rows,
                          void* workspace, size_t workspace_bytes, void* stream, bool ctr_first, float* trunk_out,
                          int64_t ld_trunk) {
    int rc = ranker_check(p);
    if (rc) return rc;
    if (rows <= 0) return AMDREC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    REQUIRE(user_rowdiv >= 1, "user_rowdiv must be >= 1");
    if (ctr_first) {
        REQUIRE(trunk_out != nullptr && ld_trunk >= 256 && ld_trunk % 4 == 0 && ((uintptr_t)trunk_out % 16) == 0,
                "bad trunk_out layout (ld_trunk >= 256, 16-byte aligned)");
        REQUIRE(ranker_x3_ctr_first_supported(p, rows, ROW_CHUNK), "these parameters cannot run the CTR-first program on %lld "
                "rows (amdrec_ranker_ctr_first_supported)", (long long)rows);
    }
    REQUIRE((user_cat || p->n_user_feat == 0) && (ad_cat || p->n_ad_feat == 0) && out_logits, "null pointer");
    REQUIRE(numerical || p->n_num == 0, "numerical is null");
    REQUIRE(ld_logits >= rows, "ld_logits < rows");
    REQUIRE(p->n_ad_feat == 0 || n_ad_rows >= 1, "n_ad_rows must be >= 1");
    REQUIRE(ad_rowmap != nullptr || p->n_ad_feat == 0 || n_ad_rows >= rows, "ad_cat has fewer rows than the batch");
    REQUIRE(p->n_user_feat == 0 || n_user_rows * user_rowdiv >= rows, "user_cat has too few rows");
    const bool hoist = user_rowdiv > 1 && p->w_proj_user && p->w_proj_ad && p->n_ad_feat > 0 &&
                       (p->n_user_feat > 0 || p->n_num > 0);
    const long long n_users = hoist ? (rows + user_rowdiv - 1) / user_rowdiv : 0;
    const RankerWs w(p, rows, workspace);
    if ((rc = require_workspace(workspace, workspace_bytes, w.bytes()))) return rc;
    const int dm = p->d_model, F0 = p->n_user_feat, F = p->n_user_feat + p->n_ad_feat;

    if (bad_index_flag) {
        if (F0 && n_user_rows > 0) launch_check_index(user_cat, n_user_rows, F0, p->cards, bad_index_flag, st);
        if (F - F0 && n_ad_rows > 0) launch_check_index(ad_cat, n_ad_rows, F - F0, p->cards + F0, bad_index_flag, st);
        if (F - F0 && ad_rowmap)
            hipLaunchKernelGGL(check_rowmap_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st,
                               (const long long*)ad_rowmap, (long long)rows, (long long)n_ad_rows, bad_index_flag);
    }

    // First-FFN hidden cache (amdrec_x3_weights.stream_hc): when the largest pass of this call takes it, the user projection
    // also writes Q[u] = W_1c U[u] - rows [U | Q] of dm + d_ff floats from the stacked weights, in the same launch.  They
    // share U's workspace region (rows * dm floats), which holds them from five candidates per user on.
    const bool with_q = hoist && ranker_x3_hidden_cache(p, w.chunk) && n_users * (long long)(dm + p->d_ff) <= rows * (long long)dm;
    const RankerCtx c{p, st, w.X, w.T, w.X0, w.H, w.U, dm, hoist, with_q ? dm + p->d_ff : dm};
    if (hoist && (rc = ranker_user_projection(c, user_cat, numerical, n_users))) return rc;
    const long long n_cache = n_ad_rows > 0 ? n_ad_rows : 1;
    for (long long r0 = 0; r0 < rows; r0 += w.chunk) {
        const long long m = rows - r0 < w.chunk ? rows - r0 : w.chunk;
        // fp16x3 row-owner engine: the rest of the chain is one kernel; with the candidate-side cache it also does the
        // gather (x0 = cache row + user half).  Its x0 scratch is the X0 region (sized in whole 128-row workgroups).
        const bool use_x3 = ranker_x3_wanted(p, m);
        float* trunk_r0 = ctr_first ? trunk_out + r0 * ld_trunk : nullptr;
        // the folded projection (x3.fold_attn1) already contains layer 1's attention block: only the engine's chain, which
        // starts with LN1 alone, may follow it
        REQUIRE(use_x3 || !ranker_x3_folded(p), "x3.fold_attn1 is set but a pass of %lld rows would not run the row-owner "
                                                "engine (the fold needs n_layers >= 1 and x3.min_rows == 1)", m);
        if (use_x3 && hoist && p->ad_proj_cache) {
            rc = ranker_x3_run(p, nullptr, 0, c.U, c.du, (const long long*)ad_rowmap, r0, (int)user_rowdiv, n_cache, m, c.X0,
                               out_logits + r0, (long long)ld_logits, st, ctr_first, trunk_r0, ld_trunk);
        } else {
            rc = ranker_project_rows(c, EmbConcatRows::ranker_rows(p, (const long long*)user_cat, numerical, user_rowdiv,
                                                                   (const long long*)ad_cat, (const long long*)ad_rowmap,
                                                                   n_ad_rows, r0, m));
            if (rc) return rc;
            rc = use_x3 ? ranker_x3_run(p, c.X, dm, nullptr, 0, nullptr, 0, 1, 0, m, c.X0, out_logits + r0, ld_logits, st, ctr_first,
                                        trunk_r0, ld_trunk)
                        : ranker_layer_chain(c, m, out_logits + r0, ld_logits);
        }
        if (rc) return rc;
    }
    return AMDREC_OK;
}

extern "C" int amdrec_ranker_forward(const amdrec_ranker_params* p, const int64_t* user_cat, const float* numerical,
                                     int64_t user_rowdiv, const int64_t* ad_cat, const int64_t* ad_rowmap,
                                     int64_t rows, float* out_logits, int64_t ld_logits, int* bad_index_flag,
                                     int64_t n_user_rows, int64_t n_ad_rows, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return ranker_forward(p, user_cat, numerical, user_rowdiv, ad_cat, ad_rowmap, rows, out_logits, ld_logits, bad_index_flag,
                          n_user_rows, n_ad_rows, workspace, workspace_bytes, stream, false, nullptr, 0);
}

extern "C" int amdrec_ranker_forward_ctr_first(const amdrec_ranker_params* p, const int64_t* user_cat, const float* numerical,
                                               int64_t user_rowdiv, const int64_t* ad_cat, const int64_t* ad_rowmap,
                                               int64_t rows, float* out_logits, int64_t ld_logits, int* bad_index_flag,
                                               int64_t n_user_rows, int64_t n_ad_rows, float* trunk_out, int64_t ld_trunk,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    return ranker_forward(p, user_cat, numerical, user_rowdiv, ad_cat, ad_rowmap, rows, out_logits, ld_logits, bad_index_flag,
                          n_user_rows, n_ad_rows, workspace, workspace_bytes, stream, true, trunk_out, ld_trunk);
}

extern "C" int amdrec_ranker_ctr_first_supported(const amdrec_ranker_params* p, int64_t rows) {
    return p != nullptr && ranker_check(p) == AMDREC_OK && rows >= 1 && ranker_x3_ctr_first_supported(p, rows, ROW_CHUNK) ? 1 : 0;
}

extern "C" int amdrec_ranker_ctr_first_workspace(const amdrec_ranker_params* p, int64_t rows, int64_t n_winner_rows,
                                                 size_t* bytes) {
    int rc = ranker_check(p);
    if (rc) return rc;
    REQUIRE(bytes && rows >= 0 && n_winner_rows >= 0, "bad arguments");
    const size_t pass1 = rows > 0 ? RankerWs(p, rows, nullptr).bytes() : 0, pass2 = ranker_x3_winner_workspace(p, n_winner_rows);
    *bytes = pass1 > pass2 ? pass1 : pass2;
    return AMDREC_OK;
}
