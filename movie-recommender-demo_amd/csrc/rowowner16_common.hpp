// What the 16-rows-per-wave kernels share whatever their workgroup shape (x3b, x3b4: rowowner16_impl.hpp; x3c:
// rowowner16c.hpp): the MFMA group, row statistics, the plane split, LayerNorm, the hidden-tile conversion and row I/O on
// the lane layout of rowowner16.hpp (lane l: row q = l & 15, group g = l >> 4; x[T][r] = feature 16 T + 4 g + r).
#pragma once
#include "x3_common.hpp"

namespace amdrec {
namespace x16 {

using x3::DBG, x3::f16x8, x3::lds_cfloat, x3::TARGET_EXP;

__device__ __forceinline__ f32x4 mfma(const f16x8& a, const f16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// one group of 4 fragment sets {Ah(t0), Al(t0), Ah(t1), Al(t1)} against one B k-step (bh, bl): 6 MFMAs, two accumulators interleaved
// NP (here and below): products per MAC.  3 = the fp16x3 arithmetic; 1 = the single-product engine (rowowner16.hpp): the
// high-by-high MFMAs alone, no low plane is formed (`bl` / `l` are never written) and a[1], a[3] are never read
template <int NP = 3>
__device__ __forceinline__ void group6(const f16x8 (&a)[4], const f16x8& bh, const f16x8& bl, f32x4& c0, f32x4& c1) {
    static_assert(NP == 3 || NP == 1, "three products or one");
    if constexpr (NP == 3) {
        c0 = mfma(a[0], bl, c0);
        c1 = mfma(a[2], bl, c1);
        c0 = mfma(a[1], bh, c0);
        c1 = mfma(a[3], bh, c1);
    }
    c0 = mfma(a[0], bh, c0);
    c1 = mfma(a[2], bh, c1);
}

__device__ __forceinline__ float reduce_max4(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float reduce_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

__device__ __forceinline__ void row_scale(const f32x4 (&x)[16], float& s, float& inv) {
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, __builtin_fabsf(x[t][r]));
    m = reduce_max4(m);
    int eb = (int)((__float_as_uint(m) >> 23) & 0xffu);
    eb = eb < 87 ? 87 : (eb > 250 ? 250 : eb);                  // as rowowner.hpp row_scale
    s = __uint_as_float((uint32_t)(127 + TARGET_EXP + 127 - eb) << 23);
    inv = __uint_as_float((uint32_t)(eb - TARGET_EXP) << 23);
}

// planes of one k-step from two adjacent tiles (elements 0..3 from `a`, 4..7 from `b`), scaled by s
template <int NP = 3>
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, float s, f16x8& h, f16x8& l) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = (j < 4 ? a[j & 3] : b[j & 3]) * s;
        const _Float16 hh = (_Float16)v;
        h[j] = hh;
        if constexpr (NP == 3) l[j] = (_Float16)(v - (float)hh);
    }
}

__device__ __forceinline__ f32x4 param4(lds_cfloat* pb, int off, int tile) {      // features 16 tile + 4 g + {0..3} (pb carries 4 g)
    return *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(pb + off + 16 * tile);
}

// planes + initial accumulators, tile pair by tile pair (x[2ks], x[2ks+1] die as they are consumed)
template <bool WITH_X, int NP = 3>
__device__ __forceinline__ void prepare(const f32x4 (&x)[16], float s, lds_cfloat* pb, int bias, float scale,
                                        f16x8 (&xh)[8], f16x8 (&xl)[8], f32x4 (&acc)[16]) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        split8<NP>(x[2 * ks], x[2 * ks + 1], s, xh[ks], xl[ks]);
#pragma unroll
        for (int t = 2 * ks; t < 2 * ks + 2; ++t) {
            const f32x4 b = param4(pb, bias, t);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] = ((WITH_X ? x[t][r] : 0.f) + b[r]) * scale;
        }
    }
}

// (returns the row's 1 / sqrt(var + eps): PH_FFN_LN_CACHED scales the cached hidden rows with it)
__device__ __forceinline__ float layer_norm(f32x4 (&y)[16], lds_cfloat* pb, int gamma, int beta, float eps) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += y[t][r];
    const float mean = reduce_sum4(s) * (1.0f / 256.0f);
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = y[t][r] - mean;
            q += d * d;
        }
    const float rstd = 1.0f / sqrtf(reduce_sum4(q) * (1.0f / 256.0f) + eps);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x4 ga = param4(pb, gamma, t), be = param4(pb, beta, t);
#pragma unroll
        for (int r = 0; r < 4; ++r) y[t][r] = (y[t][r] - mean) * rstd * ga[r] + be[r];
    }
    return rstd;
}

// LayerNorm of y = acc * un (un a power of two: acc * un is exact, and so is sum(acc) * un == sum(acc * un) barring fp32
// denormals): the unscale rides in the mean and in the deviation's fma, the deviation is kept in place
__device__ __forceinline__ void layer_norm_scaled(const f32x4 (&acc)[16], float un, f32x4 (&y)[16], lds_cfloat* pb, int gamma,
                                                  int beta, float eps) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += acc[t][r];
    const float mean = reduce_sum4(s) * un * (1.0f / 256.0f);
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = __builtin_fmaf(acc[t][r], un, -mean);
            y[t][r] = d;
            q += d * d;
        }
    const float rstd = 1.0f / sqrtf(reduce_sum4(q) * (1.0f / 256.0f) + eps);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x4 ga = param4(pb, gamma, t), be = param4(pb, beta, t);
#pragma unroll
        for (int r = 0; r < 4; ++r) y[t][r] = y[t][r] * rstd * ga[r] + be[r];
    }
}

// hidden tile (two 16-feature accumulators = one k-step of stage 2) -> planes
// `lim` = 60000 / c (exact: c is a power of two)
template <int NP = 3>
__device__ __forceinline__ void hidden_planes(const f32x4& a0, const f32x4& a1, float c, float lim, f16x8& hh, f16x8& hl) {
    if (DBG & 8) {
        asm volatile("" : "+v"(hh), "+v"(hl) : "v"(a0), "v"(a1));
        return;
    }
    // min(max(a, 0) * c, 60000) == med3(a, 0, 60000 / c) * c for a power-of-two c: relu and clamp are one instruction in
    // the unscaled domain and the scale rides in the split's fma_mix instructions (3 vector instructions per element)
    f32x4 t0, t1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        t0[r] = __builtin_amdgcn_fmed3f(a0[r], 0.f, lim);
        t1[r] = __builtin_amdgcn_fmed3f(a1[r], 0.f, lim);
    }
    split8<NP>(t0, t1, c, hh, hl);
}
__device__ __forceinline__ void init_pair(f32x4& a0, f32x4& a1, lds_cfloat* pb, int bias, int tile0, float scale) {
    const f32x4 b0 = param4(pb, bias, tile0), b1 = param4(pb, bias, tile0 + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        a0[r] = b0[r] * scale;
        a1[r] = b1[r] * scale;
    }
}

// row I/O: lane (q, g) moves the 16-byte groups [16 T + 4 g, +4) of row q (64 contiguous bytes per row and instruction)
__device__ __forceinline__ void load_rows(f32x4 (&x)[16], const float* row_ptr, int g) {
#pragma unroll
    for (int t = 0; t < 16; ++t) x[t] = *reinterpret_cast<const f32x4*>(row_ptr + 16 * t + 4 * g);
}
__device__ __forceinline__ void add_rows(f32x4 (&x)[16], const float* row_ptr, int g) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row_ptr + 16 * t + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[t][r] += v[r];
    }
}
__device__ __forceinline__ void store_rows(const f32x4 (&x)[16], float* row_ptr, int g) {
#pragma unroll
    for (int t = 0; t < 16; ++t) *reinterpret_cast<f32x4*>(row_ptr + 16 * t + 4 * g) = x[t];
}

}  // namespace x16
}  // namespace amdrec
