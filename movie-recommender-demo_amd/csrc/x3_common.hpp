// "Row-owner" fp16x3 engine of the TransformerRanker forward (transformer_ranker.py:332-380, eval mode) for gfx950: what
// all of its kernels share - numerics, the weight stream's geometry, the program a launch runs and its input rows.
// Kernels: rowowner16.hpp (16 rows per wave, the default), rowowner16c.hpp (column-split, small passes), rowowner.hpp
// (32 rows per wave).
//
// WHAT.  One kernel runs the whole chain  gather/x0 -> n x { x = LN(x + W_ov x + b) ; x = LN(x + W_2 relu(W_1 x + b_1)
// + b_2) } -> 3 x cross -> 3 heads -> logits  with every activation living in REGISTERS between the GEMMs: nothing but
// the input rows and the logits touches HBM.  (With layer 1's attention folded into the projection,
// amdrec_x3_weights.fold_attn1, the input rows are z = x0 + W_ov x0 + b_ov and the first phase is x = LN(z) alone: PH_LN.)
//
// ARITHMETIC ("x3": fp32 in, fp32 out, fp32-level error on the 16-bit matrix pipe).  Every fp32 operand is multiplied
// by a power of two (exact) and split into two fp16 planes  v = h + l + e,  h = RN16(v), l = RN16(v - h),
// |e| <= 2^-22 |v|  (fp16 has 11 significant bits; the second rounding is taken of an exact fp32 difference).  A product
// a*b is evaluated as  ah*bh + ah*bl + al*bh  by three fp16 MFMAs (an fp16 x fp16 product is exact in
// fp32; the MFMA accumulates in fp32); the dropped al*bl term is <= 2^-22 |ab|.  Split error measured on the host
// against float64 (tools/split_accuracy.py): rms 7.6e-8 of a K = 256 dot product whose fp32 fma-chain evaluation
// itself is off by rms 2.9e-7 - the same level as the round-1 six-product bf16 split (6.0e-8), at half the MFMAs.
//  * scaling: weights carry one power of two per matrix (host, max |w| -> [2^12, 2^13)); activations one power of two
//    per ROW, from the row's own max |x| (-> [2^12, 2^13)), recomputed in registers before each GEMM; a hidden tile
//    (FFN, heads) one power of two per row from the bound |relu(w_j . x + b_j)| <= ||w_j||_2 ||x||_2 + |b_j| with
//    ||x||_2 <= 16 max|x| (-> below 2^14).  fp16 overflow (65504) is therefore impossible for finite inputs; elements
//    more than 2^15 below the row maximum lose RELATIVE precision only (absolute error <= 2^-25 of a scaled unit:
//    2^-37 of the row maximum).
//
// WEIGHT STREAM.  The host packs all weights of the chain as ONE linear stream of 1 KB "fragment sets" (64 lanes x
// 16 B = the A operand of one MFMA k-step of one output tile and plane, already in lane order) in exactly the order the
// kernel consumes them.  The stream flows through an LDS ring of 16 KB chunks filled by LDS-DMA (1 KB per wave
// instruction, source and destination both linear: no swizzle needed, a fragment read is a conflict-free ds_read_b128
// at base + lane * 16); the parameter blob sits in LDS behind the ring.
#pragma once
#include "common.hpp"

namespace amdrec {
namespace x3 {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) const float lds_cfloat;
typedef __attribute__((address_space(3))) unsigned char lds_byte;

constexpr int FRAG_BYTES = 1024;                 // one fragment set: 64 lanes x 8 fp16
constexpr int CHUNK_FRAGS = 16;
constexpr int CHUNK_BYTES = CHUNK_FRAGS * FRAG_BYTES;
#ifndef AMDREC_X3_NBUF
#define AMDREC_X3_NBUF 7
#endif
constexpr int NBUF = AMDREC_X3_NBUF;             // ring chunks (7 x 16 KB = 112 KB; 6, 8 and 9 measured the same; the 16-row kernel's
                                                 // 128-row shape runs on NBUF - 1 and hands hidden tiles over in the last slot)
constexpr int PARAM_FLOATS = 11264;              // LDS parameter area behind the ring: 44 KB (the reference architecture needs 41.5)
constexpr int RING_BYTES = NBUF * CHUNK_BYTES;
constexpr int DEPTH = NBUF - 3;                  // chunks in flight beyond the certified one (NBUF >= DEPTH + 3)
constexpr int TARGET_EXP = 12;                   // scaled row / matrix maxima lie in [2^12, 2^13)

// PH_LN: LayerNorm alone (gamma / beta), no weights and no stream chunks - layer 1's LN1 when its attention block is
// folded into the feature projection (amdrec_x3_weights.fold_attn1: the input rows are z = x0 + W_ov x0 + b_ov already)
// PH_FFN_LN_CACHED (16-row kernel, 128-row shape only; must follow PH_LN): layer 1's FFN with stage 1 served from the
// hidden cache - the hidden tile is relu((P[ad] + Q[user]) * rstd + c) from two row loads (Input::hcache / Q, rstd handed
// on by PH_LN, c in the place of b_1 in the blob), the stream holds the stage-2 groups only (amdrec_x3_weights.stream_hc)
enum PhaseType { PH_ATTN_LN = 0, PH_FFN_LN = 1, PH_CROSS = 2, PH_HEADS = 3, PH_LN = 4, PH_FFN_LN_CACHED = 5 };

struct Phase {
    int type;
    int n_steps;            // FFN: d_ff / 32 hidden tiles; HEADS: head_h1 / 32 hidden tiles per task
    int n_tasks;            // HEADS
    int pad_;
    // offsets (in floats) into the parameter blob, which is DMA'd into LDS once per workgroup (see Program::params)
    int b1;                 // ATTN/CROSS: bias [256]; FFN: b_1 [d_ff]; HEADS: stacked b_1 [n_tasks * head_h1]
    int b2;                 // FFN: b_2 [256]
    int gamma;              // LayerNorm weight / bias [256] (ATTN, FFN, LN)
    int beta;
    float sw1, sw2;         // power-of-two scales of the packed weight planes (W_ov / W_1 / W_c / head W_1; W_2 / head W_2)
    float hn, hb;           // FFN / HEADS hidden bound: |relu(w_j . x + b_j)| <= hn * (2^13 / row scale) + hb, with
                            // hn = 16 max_j ||w_j||_2 (||x||_2 <= 16 max|x| over 256 features), hb = max_j |b_j|
    float ln_eps;
    float pad2_;
};
constexpr int MAX_PHASES = 20;          // 8 encoder layers x 2 + 3 cross + heads; the whole Program travels as a kernel argument
struct Program {
    int n_phases;
    int total_chunks;                   // length of the weight stream in 16 KB chunks
    const unsigned char* stream;        // packed fragment sets
    // All biases / LayerNorm weights / head vectors of the chain as ONE float blob (amdrec/weights.py pack_x3_params:
    // per layer b_ov, gamma1, beta1, b_1, b_2, gamma2, beta2; per cross layer its bias; heads b_1, then per task b_2, w_3,
    // b_3 padded to 4).  The kernel copies it into LDS behind the ring at start; a lane then reads the 4 parameters of
    // its features with ONE ds_read_b128 (lanes of a half share the address: a broadcast) - scalar loads needed a select
    // per element for the lane half and so many SGPRs that ~600 of them spilled at every phase transition.
    const float* params;
    int n_params;                       // floats, multiple of 1024 (padded), <= PARAM_FLOATS
    int hb2[4];                         // HEADS, per task: offsets of b_2 [64], w_3 [64], b_3 [4]
    int hw3[4];
    int hb3[4];
    Phase ph[MAX_PHASES];
};

// input rows: either a dense fp32 matrix X[rows][256] (the projection GEMM's output) or the cached form
// x0[r] = ad_proj_cache[ad row of r] + U[user of r]  (layers.hip proj_gather_kernel: same addends, same order)
struct Input {
    const float* X;            // dense [rows][ldx] or nullptr
    long long ldx;
    const float* cache;        // [n_cache][ldc]
    long long ldc, n_cache;
    const long long* rowmap;   // candidate -> cache row (may be nullptr: identity)
    const float* U;            // [n_users][ldu], 256 used
    long long row_base;        // global index of row 0 of this launch (for the user index)
    int rowdiv;
    long long ldu;             // 256, or 256 + d_ff when the user projection wrote [U | Q] rows
    const float* hcache;       // PH_FFN_LN_CACHED: P [n_cache][ldh] (rows as in `cache`) and Q [n_users][ldu] (= U + 256)
    long long ldh;
    const float* Q;
    // gathered dense form (16-row kernels only; X set): row r reads X[(r / top_k) * k_c + slots[r]] - the winners of a
    // selection (amdrec_select_topk's out_slots) out of the rows it selected from; clamped into [0, n_x), a negative slot
    // (no winner: its result is discarded) reads row 0.  slots == nullptr: row r reads X[r].
    const int* slots;          // [rows]
    int top_k, k_c;
    long long n_x;             // rows of X
};

// the row of X that row r of the launch reads (r < 2^31 with slots: amdrec_ranker_winner_heads)
__device__ __forceinline__ long long dense_row(const Input& in, long long r) {
    if (in.slots == nullptr) return r;
    const int s = in.slots[r];
    const long long a = (long long)((uint32_t)r / (uint32_t)in.top_k) * in.k_c + s;
    return s < 0 ? 0 : (a >= in.n_x ? in.n_x - 1 : a);
}

// The heads' ReLUs (med3 in hidden_planes, fmaxf before w_3) are one instruction per element and drop a NaN, and unlike the
// FFN no residual carries it past them: a row whose trunk state is NaN or infinite would leave with finite logits built from
// the biases, where the reference's torch.relu keeps the NaN.  So every heads phase takes ONE value per row, `probe` - an
// element of the row's first stage-1 accumulator, which the MFMA makes NaN exactly when the row's planes hold a NaN (a NaN
// anywhere in the row; an infinity gives a NaN low plane) - and applies it where a logit is stored: one select per row and
// task, nothing per hidden element, and the bits of every finite row stay what they were.
__device__ __forceinline__ float keep_nan(float logit, float probe) {
    const float z = probe * 0.f;                 // 0 for a finite probe, NaN for a NaN or infinite one
    return z != z ? z : logit;
}

// Elimination switches for tools/x3_probe.hip (0 in the product): 1 = no weight DMA and no wait for it, 2 = no
// per-chunk barrier, 4 = no fragment reads from LDS (stale registers), 8 = no hidden-tile conversion (stale planes);
// 16-row kernels only: 16 = cycle stamps (DMA wait / barrier) per wave into the logits buffer's tail, 32 (with 16) =
// stamps of the waits for a group's fragments instead, 64 / 128 = fragment reads for one group in four / in two;
// 128-row shape of the 16-row kernel only (rowowner16_impl.hpp, profiles/x3_paired_ffn_bound.log): 256 = PH_FFN_LN as the
// UNPAIRED phase on the 7-slot ring, without the fragment reads of its odd groups, 512 = that and without its hidden-tile
// conversions (the two bound the paired phase from below), 1024 = the paired phase without the exchanges at its ends.
#ifndef AMDREC_X3_DBG
#define AMDREC_X3_DBG 0
#endif
constexpr int DBG = AMDREC_X3_DBG;

// power of two sh with bound * sh in [2^13, 2^14)  (bound > 0 finite; tiny bounds clamped)
__device__ __forceinline__ float hidden_scale(float bound) {
    int eb = (int)((__float_as_uint(bound) >> 23) & 0xffu);
    eb = eb < 40 ? 40 : (eb > 250 ? 250 : eb);
    return __uint_as_float((uint32_t)(127 + 13 + 127 - eb) << 23);
}

}  // namespace x3
}  // namespace amdrec
