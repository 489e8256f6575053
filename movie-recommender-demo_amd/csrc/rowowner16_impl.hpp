// Body of the 16-rows-per-wave row-owner kernel (design and geometry: rowowner16.hpp; helpers that do not depend on the
// workgroup shape: rowowner16_common.hpp): the ring, the step and phase drivers and the kernel, included once per
// workgroup shape and product count with AMDREC_X3B_NAMESPACE / AMDREC_X3B_WAVES / AMDREC_X3B_PRODUCTS set - x3b: 8 waves =
// 128 rows per workgroup (two waves per SIMD, the throughput shape), x3b4: 4 waves = 64 rows (one wave per SIMD: a pass
// of <= 16384 rows spreads over twice the CUs and a wave has its SIMD to itself - 0.20 instead of 0.28 ms for one
// request's 500 rows, tools/x3_probe.hip);
// x1b / x1b4: the same two shapes with ONE product per MAC (rowowner16.hpp "SINGLE PRODUCT").
// No include guard.  What was tried here and not adopted: profiles/HISTORY.md "Row-owner 16-row kernel: switches".

// (a step without stage 2 is passed the not-yet-written hidden planes by reference and never reads them)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wuninitialized-const-reference"
namespace amdrec {
namespace AMDREC_X3B_NAMESPACE {

using x3::CHUNK_BYTES, x3::CHUNK_FRAGS, x3::DBG, x3::f16x8, x3::FRAG_BYTES, x3::Input, x3::lds_byte, x3::lds_cfloat, x3::Phase,
    x3::Program, x3::RING_BYTES;
using x16::add_rows, x16::init_pair, x16::layer_norm, x16::layer_norm_scaled, x16::load_rows, x16::param4, x16::reduce_sum4,
    x16::row_scale, x16::store_rows;

#if !defined(AMDREC_X3B_WAVES) || !defined(AMDREC_X3B_NAMESPACE) || !defined(AMDREC_X3B_PRODUCTS)
#error "include rowowner16.hpp, not this file"
#endif
constexpr int WAVES = AMDREC_X3B_WAVES, ROWS_PER_WAVE = 16, ROWS_PER_WG = WAVES * ROWS_PER_WAVE;
// Products per MAC: 3, or 1 = high planes only.  With 1 no low plane exists: the `xl` / `hl` / `bl` operands below are
// declared and handed on as before but never written, read, or exchanged between the waves of a pair, and a group's low
// fragment sets (1 and 3) are never read from LDS.  Ring, DMA, waits and barriers do not depend on it.
constexpr int PRODUCTS = AMDREC_X3B_PRODUCTS;
constexpr bool LOW = PRODUCTS == 3;
__device__ __forceinline__ void group6(const f16x8 (&a)[4], const f16x8& bh, const f16x8& bl, f32x4& c0, f32x4& c1) {
    x16::group6<PRODUCTS>(a, bh, bl, c0, c1);
}
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, float s, f16x8& h, f16x8& l) {
    x16::split8<PRODUCTS>(a, b, s, h, l);
}
template <bool WITH_X>
__device__ __forceinline__ void prepare(const f32x4 (&x)[16], float s, lds_cfloat* pb, int bias, float scale, f16x8 (&xh)[8],
                                        f16x8 (&xl)[8], f32x4 (&acc)[16]) {
    x16::prepare<WITH_X, PRODUCTS>(x, s, pb, bias, scale, xh, xl, acc);
}
__device__ __forceinline__ void hidden_planes(const f32x4& a0, const f32x4& a1, float c, float lim, f16x8& hh, f16x8& hl) {
    x16::hidden_planes<PRODUCTS>(a0, a1, c, lim, hh, hl);
}
constexpr int DMA_PER_WAVE = CHUNK_FRAGS / WAVES;     // 2 fragment sets per wave and chunk
// The 128-row shape runs PH_FFN_LN split by STAGE over pairs of waves (phase_ffn_ln_role_a, phase_ffn_ln_role_b below).  Its hand-off area is
// the ring's last slot: the ring is one chunk shorter there (NBUF 6 and 7 measured the same,
// profiles/x3_paired_ffn_bound.log), the parameter blob stays where it is and the host's LDS size does not change.
// (DBG & 256 / 512: the unpaired phase with its elimination switches, on the unshortened ring.)
constexpr bool PAIRED = WAVES == 8 && !(DBG & (256 | 512));
constexpr int NBUF = PAIRED ? x3::NBUF - 1 : x3::NBUF, DEPTH = NBUF - 3;
constexpr int PAIR_BYTES = CHUNK_BYTES / 4;           // per pair of waves: 4 KB = four 16-byte pieces per lane
// A chunk's DMA pieces are issued behind the fragment reads of this group of the chunk in front of it (not at the chunk's
// barrier, group 0): the matrix pipe has the first group's MFMAs queued while the waves of a SIMD sit in the
// memory-instruction issue.
constexpr int DMA_GROUP = 1;

// The weight stream's LDS ring.  DMA by buffer_load ... lds with an SGPR chunk offset: no per-lane 64-bit address add, M0
// written once per chunk (the instruction's immediate offset advances source and LDS destination together).
struct Ring {
    lds_byte* lds_dma;
    lds_byte* lds_rd;
    int issued, total;
    int slot;                    // ring slot of the chunk being read
    __amdgpu_buffer_rsrc_t rsrc; // the whole stream as a raw buffer
    uint32_t voff, soff0;        // lane * 16; wave * DMA_PER_WAVE * FRAG_BYTES
    const lds_byte* cbase;       // its address for this lane (lds_rd + slot * CHUNK_BYTES)
    unsigned long long t_wait, t_bar, t_dma;     // DBG & 16 (diagnostic build only): cycles in the DMA wait / barrier / DMA issue
    unsigned long long t_lds, t_cal;             // DBG & 32: cycles waiting for a group's fragments; stamp-pair calibration
    // DBG & 32: wait for the fragments of the group about to be multiplied, timed
    __device__ __forceinline__ void timed_landed(f16x8 (&f)[4]) {
        if (!(DBG & 32)) return;
        const unsigned long long a = __builtin_amdgcn_s_memtime();
        if constexpr (LOW) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[2]));
        const unsigned long long b = __builtin_amdgcn_s_memtime();
        t_lds += b - a;
    }

    // the 12-bit immediate covers four pieces; beyond that the SGPR offset and the LDS base move
    template <int U>
    __device__ __forceinline__ void dma_pieces(lds_byte* dst, uint32_t so) {
        if constexpr (U < DMA_PER_WAVE) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(dst + (U >> 2) * 4 * FRAG_BYTES),
                                                     16, voff, so + (U >> 2) * 4 * FRAG_BYTES, (U & 3) * FRAG_BYTES, 0);
            dma_pieces<U + 1>(dst, so);
        }
    }
    // this wave's pieces of the chunk `issued` (past the stream's end: a harmless re-load of the last chunk into a free slot)
    __device__ __forceinline__ void issue() {
        if (DBG & 1) { ++issued; return; }
        const int c = issued < total ? issued : total - 1;
        lds_byte* dst = lds_dma + (uint32_t)(issued % NBUF) * CHUNK_BYTES;
        const uint32_t so = __builtin_amdgcn_readfirstlane(soff0 + (uint32_t)c * CHUNK_BYTES);
        dma_pieces<0>(dst, so);
        ++issued;
    }
    // Certify the chunk after the one whose first fragments are about to be read: my share of it has landed (all younger
    // DMAs may still be in flight), everyone's share after the barrier.
    // EXTRA: vector-memory loads of the phase's own (PH_FFN_LN_CACHED: hidden-cache rows) that are known to have been
    // issued AFTER the DMA pieces of the chunk being certified - they sit in the same in-order counter, so the counted wait
    // leaves room for them too (an EXTRA below the true number only waits longer; above it would certify too early)
    template <int EXTRA = 0>
    __device__ __forceinline__ void certify_next() {
        if (DBG & 16) {
            const unsigned long long a = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_WAVE * (DEPTH - 1)) : "memory");
            const unsigned long long b = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_barrier();
            const unsigned long long c = __builtin_amdgcn_s_memtime();
            const unsigned long long d = __builtin_amdgcn_s_memtime();       // (the DMA issue itself sits behind group DMA_GROUP)
            t_wait += b - a; t_bar += c - b; t_dma += d - c;
            return;
        }
        if (!(DBG & 1)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_WAVE * (DEPTH - 1) + EXTRA) : "memory");
        if (!(DBG & 2)) __builtin_amdgcn_s_barrier();
    }
    __device__ __forceinline__ void start(const unsigned char* stream, int total_chunks, lds_byte* lds, int wave, int lane) {
        voff = (uint32_t)lane * 16;
        soff0 = (uint32_t)wave * DMA_PER_WAVE * FRAG_BYTES;
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(stream), 0, (uint32_t)total_chunks * CHUNK_BYTES,
                                                 0x00020000);
        lds_dma = lds + wave * DMA_PER_WAVE * FRAG_BYTES;
        lds_rd = lds + lane * 16;
        issued = 0;
        total = total_chunks;
        slot = -1;
        cbase = lds_rd;
        t_wait = t_bar = t_dma = t_lds = 0;
        t_cal = 0;
        if (DBG & 32) {
            const unsigned long long a = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const unsigned long long b = __builtin_amdgcn_s_memtime();
            t_cal = b - a;
        }
#pragma unroll
        for (int c = 0; c < DEPTH + 1; ++c) issue();
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_WAVE * DEPTH) : "memory");
        __builtin_amdgcn_s_barrier();
    }
    // Fragment group G (0..3, a compile-time constant) of the current chunk: a chunk is 4 groups of 4 fragment sets, every
    // GEMM / FFN step starts on a chunk boundary and its loops are unrolled, so the position inside the chunk is known
    // at compile time: the four reads are one base register + immediate offsets, and the ring bookkeeping (slot
    // wrap-around, barrier, DMA) runs once per chunk instead of the per-group address arithmetic and boundary test.
    // Group 0 certifies the chunk after this one and moves to this chunk's slot; group DMA_GROUP refills a free slot
    // (chunk + DEPTH + 1 into the slot of chunk - 2, which every wave has left).
    // the chunk's barrier: certify the chunk after this one, move to this chunk's slot
    template <int EXTRA = 0>
    __device__ __forceinline__ void advance() {
        certify_next<EXTRA>();
        slot = slot + 1 == NBUF ? 0 : slot + 1;
        cbase = lds_rd + (uint32_t)slot * CHUNK_BYTES;
    }
    // HALF (PH_FFN_LN, diagnostic build only, DBG & 256 / 512): no reads for the odd groups - the stage-2 groups there
    template <int G, bool HALF = false>
    __device__ __forceinline__ void frag4(f16x8 (&f)[4]) {
        static_assert(G >= 0 && G < 4 && CHUNK_FRAGS == 16, "four groups of four fragment sets per chunk");
        // DBG & 64 (diagnostic build only): fragment reads for ONE group in four - the LDS -> VGPR traffic a kernel would
        // have in which a fragment set feeds four row tiles (the hybrid row-tile-owner / column-split proposal)
        if ((DBG & 4) || ((DBG & 64) && G != 0) || ((DBG & 128) && (G & 1)) ||        // 128: one group in TWO (pairs of waves sharing)
            (HALF && (DBG & (256 | 512)) && (G & 1))) {
#pragma unroll
            for (int u = 0; u < 4; u += LOW ? 1 : 2) asm volatile("" : "+v"(f[u]));
        } else {
            // (one product: the high sets 0 and 2 alone - the low sets arrive with the chunk and stay in LDS)
#pragma unroll
            for (int u = 0; u < 4; u += LOW ? 1 : 2)
                f[u] = *reinterpret_cast<const __attribute__((address_space(3))) f16x8*>(cbase + (4 * G + u) * FRAG_BYTES);
        }
    }
    template <int G, int EXTRA = 0, bool HALF = false>
    __device__ __forceinline__ void read4(f16x8 (&f)[4]) {
        if (G == 0) advance<EXTRA>();
        frag4<G, HALF>(f);
        if (G == DMA_GROUP) issue();
    }
    __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// groups I .. 63 of one 256 x 256 GEMM (group I = k-step I / 8, tile pair I % 8); `cur` holds group I's fragments
template <int I>
__device__ __forceinline__ void gemm256_groups(Ring& ring, f16x8 (&cur)[4], const f16x8 (&xh)[8], const f16x8 (&xl)[8],
                                               f32x4 (&acc)[16]) {
    constexpr int ks = I >> 3, tp = I & 7;
    f16x8 nxt[4];
    if constexpr (I < 63) ring.read4<(I + 1) & 3>(nxt);
    ring.timed_landed(cur);
    group6(cur, xh[ks], xl[ks], acc[2 * tp], acc[2 * tp + 1]);
    if constexpr (I < 63) gemm256_groups<I + 1>(ring, nxt, xh, xl, acc);
}
template <int I0>
__device__ __forceinline__ void gemm256_from(Ring& ring, const f16x8 (&xh)[8], const f16x8 (&xl)[8], f32x4 (&acc)[16]) {
    f16x8 cur[4];
    ring.read4<0>(cur);
    gemm256_groups<I0>(ring, cur, xh, xl, acc);
}

__device__ __forceinline__ void gemm256(Ring& ring, const f16x8 (&xh)[8], const f16x8 (&xl)[8], f32x4 (&acc)[16]) {
    gemm256_from<0>(ring, xh, xl, acc);
}
__device__ __forceinline__ void phase_attn_ln(Ring& ring, const Phase& P, f32x4 (&x)[16], lds_cfloat* pb) {
    float s, inv;
    row_scale(x, s, inv);
    f16x8 xh[8], xl[8];
    f32x4 acc[16];
    prepare<true>(x, s, pb, P.b1, s * P.sw1, xh, xl, acc);
    gemm256(ring, xh, xl, acc);
    layer_norm_scaled(acc, inv / P.sw1, x, pb, P.gamma, P.beta, P.ln_eps);
}

template <bool S1, bool S2, int GI, int EXTRA = 0, bool HALF = false>
__device__ __forceinline__ void ffn_groups(Ring& ring, f16x8 (&cur)[4], const f16x8 (&xh)[8], const f16x8 (&xl)[8],
                                           f32x4& a10, f32x4& a11, f32x4 (&acc2)[16], const f16x8& hh, const f16x8& hl) {
    constexpr int NG = (S1 ? 8 : 0) + (S2 ? 8 : 0);          // groups in this step (a multiple of 4: whole chunks)
    constexpr bool is1 = S1 && (!S2 || (GI & 1) == 0);
    constexpr int u = (S1 && S2) ? GI >> 1 : GI;
    f16x8 nxt[4];
    if constexpr (GI < NG - 1) ring.read4<(GI + 1) & 3, EXTRA, HALF>(nxt);
    ring.timed_landed(cur);
    if constexpr (is1) group6(cur, xh[u], xl[u], a10, a11);
    else group6(cur, hh, hl, acc2[2 * u], acc2[2 * u + 1]);
    if constexpr (GI < NG - 1) ffn_groups<S1, S2, GI + 1, EXTRA, HALF>(ring, nxt, xh, xl, a10, a11, acc2, hh, hl);
}

// One FFN step: 8 x { stage-1 group (W_1 tiles 2t, 2t+1 at ks = u), stage-2 group (W_2 tiles 2u, 2u+1 at k-step t-1) }
template <bool S1, bool S2, int EXTRA = 0, bool HALF = false>
__device__ __forceinline__ void ffn_step(Ring& ring, const f16x8 (&xh)[8], const f16x8 (&xl)[8], f32x4& a10, f32x4& a11,
                                         f32x4 (&acc2)[16], const f16x8& hh, const f16x8& hl) {
    f16x8 cur[4];
    ring.read4<0, EXTRA, HALF>(cur);
    ffn_groups<S1, S2, 0, EXTRA, HALF>(ring, cur, xh, xl, a10, a11, acc2, hh, hl);
}

// (diagnostic build only, DBG & 512: PH_FFN_LN without its hidden-tile conversions - stale planes)
__device__ __forceinline__ void ffn_hidden(const f32x4& a0, const f32x4& a1, float c, float lim, f16x8& hh, f16x8& hl) {
    if (DBG & 512) asm volatile("" : "+v"(hh), "+v"(hl) : "v"(a0), "v"(a1));
    else hidden_planes(a0, a1, c, lim, hh, hl);
}
__device__ __forceinline__ void phase_ffn_ln(Ring& ring, const Phase& P, f32x4 (&x)[16], lds_cfloat* pb) {
    float s, inv;
    row_scale(x, s, inv);
    f16x8 xh[8], xl[8];
    const float sh = x3::hidden_scale(fmaf(P.hn * 8192.0f, inv, P.hb));
    f32x4 acc2[16];
    prepare<true>(x, s, pb, P.b2, P.sw2 * sh, xh, xl, acc2);
    const float b1s = s * P.sw1, c1 = sh * inv / P.sw1, lim1 = 60000.f / c1;
    f32x4 a10, a11;
    f16x8 hh, hl;
    init_pair(a10, a11, pb, P.b1, 0, b1s);
    ffn_step<true, false, 0, true>(ring, xh, xl, a10, a11, acc2, hh, hl);
    for (int t = 1; t < P.n_steps; ++t) {
        ffn_hidden(a10, a11, c1, lim1, hh, hl);
        init_pair(a10, a11, pb, P.b1, 2 * t, b1s);
        ffn_step<true, true, 0, true>(ring, xh, xl, a10, a11, acc2, hh, hl);
    }
    ffn_hidden(a10, a11, c1, lim1, hh, hl);
    ffn_step<false, true, 0, true>(ring, xh, xl, a10, a11, acc2, hh, hl);
    layer_norm_scaled(acc2, 1.0f / (P.sw2 * sh), x, pb, P.gamma, P.beta, P.ln_eps);
}

// ---- PH_FFN_LN split by STAGE over pairs of waves (the 128-row shape) ----
// Waves w ("role A") and w + 4 ("role B") share a SIMD and form a pair; tile 0 is A's 16 rows, tile 1 B's.  A holds the x
// planes of BOTH tiles and runs every stage-1 group against both; B holds the stage-2 accumulators of both tiles and runs
// every stage-2 group against both: a fragment set read from LDS feeds 12 MFMAs instead of 6, every wave reads the
// fragments of half the groups (the stream alternates stage-1 and stage-2 groups: A reads groups 0 and 2 of a chunk, B 1
// and 3), and the two waves of a SIMD no longer convert their hidden tiles at the same moment (pair_publish).
// Every output element sees the MFMAs it sees in phase_ffn_ln, in the same order and scaled alike: results are bit-identical.
//  * hidden tiles: A writes the planes of its tile and the finished accumulators of B's (4 x 16 bytes per lane: the
//    accumulator layout IS the B-operand layout, so lane l writes what lane l of B reads) into the pair's area, waits lgkmcnt(0) and passes the next chunk's barrier
//    (Ring::advance); B reads them behind that barrier.  One buffer is enough: B's reads have landed before the MFMAs of
//    its first group, i.e. before its next barrier, and A writes again three barriers later.
//  * phase entry / exit: B's planes and stage-1 bias scale go to A, A's initial stage-2 accumulator and hidden scale to B, and at
//    the end A's LayerNorm output comes back - 16 KB each through the 4 KB area, in slices of { write, wait, barrier, read,
//    wait, barrier }: 18 barriers at entry, 8 at exit, beside the phase's 4 n_steps.
//  * workgroup barriers only, and both roles pass the same number on every path: a role without groups in a step (B in the
//    first, A in the last) still passes every chunk's barrier and issues its DMA pieces.
template <int K, class V>
__device__ __forceinline__ void pair_put(lds_byte* box, const V& v) {
    static_assert(sizeof(V) == 16 && K >= 0 && K < PAIR_BYTES / FRAG_BYTES, "a 16-byte piece per lane");
    *reinterpret_cast<__attribute__((address_space(3))) V*>(box + K * FRAG_BYTES) = v;
}
template <int K, class V>
__device__ __forceinline__ void pair_get(const lds_byte* box, V& v) {
    static_assert(sizeof(V) == 16 && K >= 0 && K < PAIR_BYTES / FRAG_BYTES, "a 16-byte piece per lane");
    v = *reinterpret_cast<const __attribute__((address_space(3))) V*>(box + K * FRAG_BYTES);
}
__device__ __forceinline__ void pair_landed() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void pair_sync() {        // my accesses to the area are done; everyone's behind the barrier
    pair_landed();
    __builtin_amdgcn_s_barrier();
}
// one fragment set against one B k-step of both tiles: per accumulator the MFMAs of group6, in its order
__device__ __forceinline__ void group12(const f16x8 (&a)[4], const f16x8& bh0, const f16x8& bl0, const f16x8& bh1,
                                        const f16x8& bl1, f32x4& c00, f32x4& c01, f32x4& c10, f32x4& c11) {
    if constexpr (LOW) {
        c00 = x16::mfma(a[0], bl0, c00);
        c01 = x16::mfma(a[2], bl0, c01);
        c10 = x16::mfma(a[0], bl1, c10);
        c11 = x16::mfma(a[2], bl1, c11);
        c00 = x16::mfma(a[1], bh0, c00);
        c01 = x16::mfma(a[3], bh0, c01);
        c10 = x16::mfma(a[1], bh1, c10);
        c11 = x16::mfma(a[3], bh1, c11);
    }
    c00 = x16::mfma(a[0], bh0, c00);
    c01 = x16::mfma(a[2], bh0, c01);
    c10 = x16::mfma(a[0], bh1, c10);
    c11 = x16::mfma(a[2], bh1, c11);
}
// A role's J-th group of a step.  MODE 0: a single-stage step, all four groups of its 2 chunks are this role's;
// MODE 1: role A in a full step (groups 0 and 2 of its 4 chunks); MODE 2: role B there (groups 1 and 3).
// The role's first group of a chunk passes the chunk's barrier, one of its groups issues the wave's DMA pieces.
template <int MODE, int J>
__device__ __forceinline__ void pair_read(Ring& ring, f16x8 (&f)[4]) {
    constexpr int G = MODE == 0 ? (J & 3) : 2 * (J & 1) + (MODE == 2 ? 1 : 0);
    if constexpr (G == (MODE == 2 ? 1 : 0)) ring.advance();
    ring.frag4<G>(f);
    if constexpr (G == (MODE == 1 ? 2 : DMA_GROUP)) ring.issue();
}
template <int MODE, int J>
__device__ __forceinline__ void pair_groups1(Ring& ring, f16x8 (&cur)[4], const f16x8 (&xh)[2][8], const f16x8 (&xl)[2][8],
                                             f32x4 (&a)[2][2]) {
    f16x8 nxt[4];
    if constexpr (J < 7) pair_read<MODE, J + 1>(ring, nxt);
    ring.timed_landed(cur);
    group12(cur, xh[0][J], xl[0][J], xh[1][J], xl[1][J], a[0][0], a[0][1], a[1][0], a[1][1]);
    if constexpr (J < 7) pair_groups1<MODE, J + 1>(ring, nxt, xh, xl, a);
}
template <int MODE, int J>
__device__ __forceinline__ void pair_groups2(Ring& ring, f16x8 (&cur)[4], const f16x8 (&hh)[2], const f16x8 (&hl)[2],
                                             f32x4 (&acc2)[2][16]) {
    f16x8 nxt[4];
    if constexpr (J < 7) pair_read<MODE, J + 1>(ring, nxt);
    ring.timed_landed(cur);
    group12(cur, hh[0], hl[0], hh[1], hl[1], acc2[0][2 * J], acc2[0][2 * J + 1], acc2[1][2 * J], acc2[1][2 * J + 1]);
    if constexpr (J < 7) pair_groups2<MODE, J + 1>(ring, nxt, hh, hl, acc2);
}
// the 2 chunks of a single-stage step for the role without groups in it
__device__ __forceinline__ void pair_idle_step(Ring& ring) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        ring.advance();
        ring.issue();
    }
}

// A: the finished hidden tile goes to the pair's area - its own tile's as planes, B's tile's as the two accumulators it
// is (B converts that one: each wave converts one tile per step, as in the unpaired phase, but not at the same time - A in
// front of the barrier, under B's last MFMAs of the step, B behind it, under A's first); the next chunk's barrier hands
// them to B
__device__ __forceinline__ void pair_publish(const f32x4 (&a)[2][2], float c1, float lim1, lds_byte* box) {
    f16x8 hh, hl;
    hidden_planes(a[0][0], a[0][1], c1, lim1, hh, hl);
    pair_put<0>(box, hh);
    if constexpr (LOW) pair_put<1>(box, hl);
    pair_put<2>(box, a[1][0]);
    pair_put<3>(box, a[1][1]);
    pair_landed();
}
// B, behind a step's first barrier: what A published in front of it
__device__ __forceinline__ void pair_fetch(const lds_byte* box, float c1, float lim1, f16x8 (&hh)[2], f16x8 (&hl)[2]) {
    f32x4 a0, a1;
    pair_get<0>(box, hh[0]);
    if constexpr (LOW) pair_get<1>(box, hl[0]);
    pair_get<2>(box, a0);
    pair_get<3>(box, a1);
    hidden_planes(a0, a1, c1, lim1, hh[1], hl[1]);
}

__device__ __forceinline__ void phase_ffn_ln_role_a(Ring& ring, const Phase& P, f32x4 (&x)[16], lds_cfloat* pb, lds_byte* box) {
    float s, inv;
    row_scale(x, s, inv);
    const float sh = x3::hidden_scale(fmaf(P.hn * 8192.0f, inv, P.hb));
    float b1s[2];
    b1s[0] = s * P.sw1;
    const float c1 = sh * inv / P.sw1, lim1 = 60000.f / c1;
    f16x8 xh[2][8], xl[2][8];
    {
        f32x4 acc2[16];
        prepare<true>(x, s, pb, P.b2, P.sw2 * sh, xh[0], xl[0], acc2);
        // pieces 0, 1: B -> A; pieces 2, 3: A -> B
        f32x4 sc = {P.sw2 * sh, 0.f, 0.f, 0.f};
        if (DBG & 1024) {           // diagnostic build only: no exchange at the phase's ends (its cost by difference)
            sc[0] = b1s[0];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                asm volatile("" ::"v"(acc2[2 * i]), "v"(acc2[2 * i + 1]));
                xh[1][i] = xh[0][i], xl[1][i] = xl[0][i];
                asm volatile("" : "+v"(xh[1][i]), "+v"(xl[1][i]));
            }
        } else {
            pair_put<2>(box, sc);
            pair_sync();
            pair_get<0>(box, sc);
            pair_sync();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pair_put<2>(box, acc2[2 * i]);
                pair_put<3>(box, acc2[2 * i + 1]);
                pair_sync();
                pair_get<0>(box, xh[1][i]);
                if constexpr (LOW) pair_get<1>(box, xl[1][i]);
                pair_sync();
            }
        }
        b1s[1] = sc[0];
    }
    f32x4 a[2][2];
    f16x8 cur[4];
    init_pair(a[0][0], a[0][1], pb, P.b1, 0, b1s[0]);
    init_pair(a[1][0], a[1][1], pb, P.b1, 0, b1s[1]);
    pair_read<0, 0>(ring, cur);
    pair_groups1<0, 0>(ring, cur, xh, xl, a);
    for (int t = 1; t < P.n_steps; ++t) {
        pair_publish(a, c1, lim1, box);         // tile t - 1
        init_pair(a[0][0], a[0][1], pb, P.b1, 2 * t, b1s[0]);
        init_pair(a[1][0], a[1][1], pb, P.b1, 2 * t, b1s[1]);
        pair_read<1, 0>(ring, cur);
        pair_groups1<1, 0>(ring, cur, xh, xl, a);
    }
    pair_publish(a, c1, lim1, box);
    pair_idle_step(ring);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (DBG & 1024) {
            asm volatile("" : "+v"(x[4 * k]), "+v"(x[4 * k + 1]), "+v"(x[4 * k + 2]), "+v"(x[4 * k + 3]));
            continue;
        }
        pair_sync();
        pair_get<0>(box, x[4 * k]);
        pair_get<1>(box, x[4 * k + 1]);
        pair_get<2>(box, x[4 * k + 2]);
        pair_get<3>(box, x[4 * k + 3]);
        pair_sync();
    }
}

__device__ __forceinline__ void phase_ffn_ln_role_b(Ring& ring, const Phase& P, f32x4 (&x)[16], lds_cfloat* pb, lds_byte* box) {
    float s, inv;
    row_scale(x, s, inv);
    const float sh = x3::hidden_scale(fmaf(P.hn * 8192.0f, inv, P.hb));
    float k2[2];
    k2[1] = P.sw2 * sh;
    const float c1 = sh * inv / P.sw1, lim1 = 60000.f / c1;
    f32x4 acc2[2][16];
    {
        f16x8 xh[8], xl[8];
        prepare<true>(x, s, pb, P.b2, k2[1], xh, xl, acc2[1]);
        f32x4 sc = {s * P.sw1, 0.f, 0.f, 0.f};
        if (DBG & 1024) {
            sc[0] = k2[1];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                asm volatile("" ::"v"(xh[i]), "v"(xl[i]));
                acc2[0][2 * i] = acc2[1][2 * i], acc2[0][2 * i + 1] = acc2[1][2 * i + 1];
                asm volatile("" : "+v"(acc2[0][2 * i]), "+v"(acc2[0][2 * i + 1]));
            }
        } else {
            pair_put<0>(box, sc);
            pair_sync();
            pair_get<2>(box, sc);
            pair_sync();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                pair_put<0>(box, xh[i]);
                if constexpr (LOW) pair_put<1>(box, xl[i]);
                pair_sync();
                pair_get<2>(box, acc2[0][2 * i]);
                pair_get<3>(box, acc2[0][2 * i + 1]);
                pair_sync();
            }
        }
        k2[0] = sc[0];
    }
    pair_idle_step(ring);
    f16x8 hh[2], hl[2], cur[4];
    for (int t = 1; t < P.n_steps; ++t) {
        pair_read<2, 0>(ring, cur);
        pair_fetch(box, c1, lim1, hh, hl);                // tile t - 1
        pair_groups2<2, 0>(ring, cur, hh, hl, acc2);
    }
    pair_read<0, 0>(ring, cur);
    pair_fetch(box, c1, lim1, hh, hl);
    pair_groups2<0, 0>(ring, cur, hh, hl, acc2);
    {
        f32x4 y[16];
        layer_norm_scaled(acc2[0], 1.0f / k2[0], y, pb, P.gamma, P.beta, P.ln_eps);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (DBG & 1024) {
                asm volatile("" ::"v"(y[4 * k]), "v"(y[4 * k + 1]), "v"(y[4 * k + 2]), "v"(y[4 * k + 3]));
                continue;
            }
            pair_put<0>(box, y[4 * k]);
            pair_put<1>(box, y[4 * k + 1]);
            pair_put<2>(box, y[4 * k + 2]);
            pair_put<3>(box, y[4 * k + 3]);
            pair_sync();
            pair_sync();
        }
    }
    layer_norm_scaled(acc2[1], 1.0f / k2[1], x, pb, P.gamma, P.beta, P.ln_eps);
}

// ---- PH_FFN_LN_CACHED: layer 1's FFN with stage 1 from the hidden cache (amdrec_x3_weights.stream_hc) ----
// W_1 x1 + b_1 = rstd * W_1c z + c with W_1c z = P[ad] + Q[user]: hidden tile t (features 32 t .. 32 t + 31) is two 16-byte
// groups of each row per lane - floats 32 t + 4 g and 32 t + 16 + 4 g, the accumulator layout of the two stage-1 tiles it
// replaces (row I/O pattern of load_rows: 64 contiguous bytes per row and instruction).
struct HiddenRows {
    f32x4 p0, p1, q0, q1;
};
// The loads stay in flight across two steps (and the loop's back edge), where the compiler's own wait insertion falls back
// to vmcnt(0) - which would also drain the ring's DMA once per step.  So they are issued as inline assembly, invisible to
// it, and waited for by count (wait_hidden) like the ring's DMA pieces.
__device__ __forceinline__ void load_hidden(HiddenRows& h, const float* prow, const float* qrow, int t) {
    const float* pp = prow + 32 * t;
    const float* qq = qrow + 32 * t;
    asm volatile("global_load_dwordx4 %0, %4, off\n\t"
                 "global_load_dwordx4 %1, %4, off offset:64\n\t"
                 "global_load_dwordx4 %2, %5, off\n\t"
                 "global_load_dwordx4 %3, %5, off offset:64"
                 : "=&v"(h.p0), "=&v"(h.p1), "=&v"(h.q0), "=&v"(h.q1)
                 : "v"(pp), "v"(qq)
                 : "memory");
}
// N = vector-memory operations issued after the four loads of `h` (DMA pieces and younger loads of this phase)
template <int N>
__device__ __forceinline__ void wait_hidden(HiddenRows& h) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(h.p0), "+v"(h.p1), "+v"(h.q0), "+v"(h.q1) : "n"(N) : "memory");
}
// step t: hidden tile t from `h` (WAIT: see wait_hidden) -> planes, then (LOAD) h <- the rows of step t + 2, then the 8
// stage-2 groups (2 chunks).  The four loads are issued in front of the step's first chunk barrier; EXTRA: see
// Ring::certify_next.
template <int EXTRA, int WAIT, bool LOAD>
__device__ __forceinline__ void cached_step(Ring& ring, const Phase& P, HiddenRows& h, const float* prow, const float* qrow,
                                            int t, float rstd, float sh, float lim, lds_cfloat* pb, f32x4 (&acc2)[16]) {
    const f32x4 c0 = param4(pb, P.b1, 2 * t), c1 = param4(pb, P.b1, 2 * t + 1);
    wait_hidden<WAIT>(h);
    f32x4 a0, a1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        a0[r] = __builtin_fmaf(h.p0[r] + h.q0[r], rstd, c0[r]);
        a1[r] = __builtin_fmaf(h.p1[r] + h.q1[r], rstd, c1[r]);
    }
    f16x8 hh, hl, xh[8], xl[8];               // (no stage 1: the x planes are never read)
    hidden_planes(a0, a1, sh, lim, hh, hl);
    if (LOAD) load_hidden(h, prow, qrow, t + 2);
    ffn_step<false, true, EXTRA>(ring, xh, xl, a0, a1, acc2, hh, hl);
}
// x = LN1's output, rstd = its 1 / sqrt(var(z) + eps).  Two steps' rows are in flight (two register sets, refilled as they
// are consumed): 4 loads per step beside the ring's 4 DMA pieces (2 per chunk, always issued: past the stream's end the
// ring re-loads its last chunk).  All of them sit in ONE in-order counter, so every wait of the phase is by count:
//  * a step's rows (WAIT): issued two steps = 8 DMA pieces and one younger set of loads earlier: 12; the first two sets go
//    out together at the start of the phase (4, 8), and no set follows the one that the last step consumes (8);
//  * a chunk's DMA (EXTRA, Ring::certify_next): when chunk k + 1 is certified in front of chunk k of step t = k / 2, the
//    loads issued at the start of steps t - 1 and t are younger than its DMA pieces, which went out four chunks earlier:
//    8 while both sets exist, 4 in step T - 2, 0 in step T - 1.
__device__ __forceinline__ void phase_ffn_ln_cached(Ring& ring, const Phase& P, f32x4 (&x)[16], float rstd, const float* prow,
                                                    const float* qrow, lds_cfloat* pb) {
    HiddenRows ha, hb;
    load_hidden(ha, prow, qrow, 0);
    load_hidden(hb, prow, qrow, 1);
    float s, inv;
    row_scale(x, s, inv);
    const float sh = x3::hidden_scale(fmaf(P.hn * 8192.0f, inv, P.hb));
    const float k2 = P.sw2 * sh, lim = 60000.f / sh;
    f32x4 acc2[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x4 b = param4(pb, P.b2, t);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc2[t][r] = (x[t][r] + b[r]) * k2;
    }
    const int T = P.n_steps;                   // even, >= 4 (x3_build)
    cached_step<8, 4, true>(ring, P, ha, prow, qrow, 0, rstd, sh, lim, pb, acc2);
    cached_step<8, 8, true>(ring, P, hb, prow, qrow, 1, rstd, sh, lim, pb, acc2);
    for (int t = 2; t < T - 2; t += 2) {
        cached_step<8, 12, true>(ring, P, ha, prow, qrow, t, rstd, sh, lim, pb, acc2);
        cached_step<8, 12, true>(ring, P, hb, prow, qrow, t + 1, rstd, sh, lim, pb, acc2);
    }
    cached_step<4, 12, false>(ring, P, ha, prow, qrow, T - 2, rstd, sh, lim, pb, acc2);
    cached_step<0, 8, false>(ring, P, hb, prow, qrow, T - 1, rstd, sh, lim, pb, acc2);
    layer_norm_scaled(acc2, 1.0f / k2, x, pb, P.gamma, P.beta, P.ln_eps);
}

// one QUARTER of a cross layer's 256 x 256 GEMM: output tiles 4 Q4 .. 4 Q4 + 3 (two tile pairs), 16 groups = 4 chunks,
// k-step major (amdrec/weights.py x3b_stream_cross); `cur` holds group I's fragments
template <int I>
__device__ __forceinline__ void cross_quarter_groups(Ring& ring, f16x8 (&cur)[4], const f16x8 (&xh)[8], const f16x8 (&xl)[8],
                                                     f32x4 (&acc)[4]) {
    constexpr int ks = I >> 1, pr = I & 1;
    f16x8 nxt[4];
    if constexpr (I < 15) ring.read4<(I + 1) & 3>(nxt);
    ring.timed_landed(cur);
    group6(cur, xh[ks], xl[ks], acc[2 * pr], acc[2 * pr + 1]);
    if constexpr (I < 15) cross_quarter_groups<I + 1>(ring, nxt, xh, xl, acc);
}

// xl <- x0 * (xl W + b) + xl with x0 IN REGISTERS (round 2 wrote the trunk's output to HBM once and read it back in each of
// the three cross layers: 1.05 of the launch's 1.99 GB of HBM traffic).  x0 (64 registers) + the residual xl (64) + the
// planes of xl (64) leave room for a 16-register accumulator, so the GEMM runs in four quarters of the output features;
// a quarter's epilogue updates its own four tiles of xl in place - the planes were taken from the old xl, and a tile's
// residual is its own old value.  Same MFMAs in the same order per output element as the undivided GEMM: bit-identical.
__device__ __forceinline__ void phase_cross(Ring& ring, const Phase& P, f32x4 (&xl_)[16], const f32x4 (&x0)[16], lds_cfloat* pb) {
    float s, inv;
    row_scale(xl_, s, inv);
    f16x8 xh[8], xl[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) split8(xl_[2 * ks], xl_[2 * ks + 1], s, xh[ks], xl[ks]);
    const float bs = s * P.sw1, un = inv / P.sw1;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        f32x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 b = param4(pb, P.b1, 4 * q4 + i);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = b[r] * bs;
        }
        f16x8 cur[4];
        ring.read4<0>(cur);
        cross_quarter_groups<0>(ring, cur, xh, xl, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) xl_[4 * q4 + i][r] = x0[4 * q4 + i][r] * (acc[i][r] * un) + xl_[4 * q4 + i][r];
    }
}

// One step of the heads, software-pipelined like the FFN (round 3; the heads used to finish a hidden tile's stage 1, convert
// it and only then run its stage 2: a dependency bubble per tile and two fragment reads with nothing to hide behind - 5.45 us
// per chunk against the FFN's 4.55): the stage-1 groups of hidden tile tt (8: W_1 tiles 2tt, 2tt+1 at ks = u) with the two
// stage-2 groups of tile tt - 1 (W_2 tile pairs 0 and 1 of that tile's task, at k-step = its index in the task) riding behind
// u = 3 and u = 7.  Stream order: amdrec/weights.py x3b_stream_heads.  P0 = position of the step's first group in its
// chunk (0 or 2: a full step is 10 groups = 2.5 chunks).
template <bool S1, bool S2, int P0, int GI>
__device__ __forceinline__ void heads_groups(Ring& ring, f16x8 (&cur)[4], const f16x8 (&xh)[8], const f16x8 (&xl)[8],
                                             f32x4& a10, f32x4& a11, f32x4 (&acc2)[4], const f16x8& hh, const f16x8& hl) {
    constexpr int NG = (S1 ? 8 : 0) + (S2 ? 2 : 0);
    // (S1 && S2): u0 u1 u2 u3 p0 u4 u5 u6 u7 p1
    constexpr bool is2 = S2 && (!S1 || GI == 4 || GI == 9);
    constexpr int u = !S1 ? 0 : (S2 ? (GI < 4 ? GI : GI - 1) : GI);
    constexpr int pr = !S1 ? GI : (GI == 9 ? 1 : 0);
    f16x8 nxt[4];
    if constexpr (GI < NG - 1) ring.read4<(P0 + GI + 1) & 3>(nxt);
    ring.timed_landed(cur);
    if constexpr (is2) group6(cur, hh, hl, acc2[2 * pr], acc2[2 * pr + 1]);
    else group6(cur, xh[u], xl[u], a10, a11);
    if constexpr (GI < NG - 1) heads_groups<S1, S2, P0, GI + 1>(ring, nxt, xh, xl, a10, a11, acc2, hh, hl);
}
template <bool S1, bool S2, int P0>
__device__ __forceinline__ void heads_step(Ring& ring, const f16x8 (&xh)[8], const f16x8 (&xl)[8], f32x4& a10, f32x4& a11,
                                           f32x4 (&acc2)[4], const f16x8& hh, const f16x8& hl) {
    f16x8 cur[4];
    ring.read4<P0>(cur);
    heads_groups<S1, S2, P0, 0>(ring, cur, xh, xl, a10, a11, acc2, hh, hl);
}

__device__ __forceinline__ void phase_heads(Ring& ring, const Program& G, const Phase& P, const f32x4 (&x)[16], float* out,
                                            long long ld_out, long long row, bool row_ok, int g, lds_cfloat* pb) {
    float s, inv;
    row_scale(x, s, inv);
    f16x8 xh[8], xl[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) split8(x[2 * ks], x[2 * ks + 1], s, xh[ks], xl[ks]);
    const float sh = x3::hidden_scale(fmaf(P.hn * 8192.0f, inv, P.hb));
    const float b1s = s * P.sw1, c1 = sh * inv / P.sw1, un2 = 1.0f / (P.sw2 * sh), lim1 = 60000.f / c1;
    const int T = P.n_steps, NT = P.n_tasks * T;               // hidden tiles per task / in all (NT even: x3_build)
    f32x4 acc2[4], a10, a11;
    f16x8 hh, hl;
    init_pair(acc2[0], acc2[1], pb, G.hb2[0], 0, P.sw2 * sh);
    init_pair(acc2[2], acc2[3], pb, G.hb2[0], 2, P.sw2 * sh);
    init_pair(a10, a11, pb, P.b1, 0, b1s);
    heads_step<true, false, 0>(ring, xh, xl, a10, a11, acc2, hh, hl);                   // tile 0: stage 1 only
    const float probe = a10[0];                                // NaN iff the row's state is not finite (x3_common.hpp keep_nan)
    int task = 0, t_in = 0;                                    // task / index of the tile whose stage 2 runs in step tt
    for (int tt = 1; tt <= NT; ++tt) {
        hidden_planes(a10, a11, c1, lim1, hh, hl);             // tile tt - 1
        if (tt < NT) {
            init_pair(a10, a11, pb, P.b1, 2 * tt, b1s);        // stacked b_1: tile tt of all tasks' hidden units
            if (tt & 1) heads_step<true, true, 0>(ring, xh, xl, a10, a11, acc2, hh, hl);
            else heads_step<true, true, 2>(ring, xh, xl, a10, a11, acc2, hh, hl);
        } else {
            heads_step<false, true, 2>(ring, xh, xl, a10, a11, acc2, hh, hl);           // NT even: the last step starts at 2
        }
        if (++t_in == T) {                                     // that was the task's last hidden tile: its 64 outputs are complete
            float dot = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 w = param4(pb, G.hw3[task], t);
#pragma unroll
                for (int r = 0; r < 4; ++r) dot += fmaxf(acc2[t][r] * un2, 0.f) * w[r];
            }
            dot = reduce_sum4(dot);
            if (g == 0 && row_ok) out[(long long)task * ld_out + row] = x3::keep_nan(dot + pb[G.hb3[task]], probe);  // g == 0: pb carries no offset
            t_in = 0;
            if (++task < P.n_tasks) {
                init_pair(acc2[0], acc2[1], pb, G.hb2[task], 0, P.sw2 * sh);
                init_pair(acc2[2], acc2[3], pb, G.hb2[task], 2, P.sw2 * sh);
            }
        }
    }
}

// everything after the parameter blob is in LDS: ring start, row load, the phases, logits
__device__ __forceinline__ void run_chain(const Program& G, const Input& in, long long rows, float* scratch, float* x_out,
                                          long long ld_xout, float* logits, long long ld_logits, unsigned char* smem, int wave,
                                          int lane, lds_cfloat* pb) {
    const int g = lane >> 4, q = lane & 15;
    const long long row = (long long)blockIdx.x * ROWS_PER_WG + wave * ROWS_PER_WAVE + q;
    const bool row_ok = row < rows;
    const long long rowc = row_ok ? row : rows - 1;
    Ring ring;
    const unsigned long long t_begin = (DBG & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
    ring.start(G.stream, G.total_chunks, (lds_byte*)smem, wave, lane);

    f32x4 x[16];
    if (in.X != nullptr) {
        load_rows(x, in.X + x3::dense_row(in, rowc) * in.ldx, g);
    } else {
        const long long gr = in.row_base + rowc;
        long long a = in.rowmap ? in.rowmap[gr] : gr;
        a = a < 0 ? 0 : (a >= in.n_cache ? in.n_cache - 1 : a);
        load_rows(x, in.cache + a * in.ldc, g);
        add_rows(x, in.U + (gr / in.rowdiv) * in.ldu, g);
    }
    // The chain is [encoder phases] [cross phases] [heads] (ranker_x3.hip x3_build), walked as three loops so that x0 - the
    // trunk's output, 64 registers - is live only across the cross layers.
    int p = 0;
    float rstd = 0.f;                              // of PH_LN, for the PH_FFN_LN_CACHED that follows it
    for (; p < G.n_phases; ++p) {
        const Phase& P = G.ph[p];
        const int type = __builtin_amdgcn_readfirstlane(P.type);
        if (type == x3::PH_ATTN_LN) phase_attn_ln(ring, P, x, pb);
        else if (type == x3::PH_FFN_LN) {
            if constexpr (PAIRED) {
                lds_byte* box = (lds_byte*)smem + NBUF * CHUNK_BYTES + (wave & 3) * PAIR_BYTES + lane * 16;
                if (wave < 4) phase_ffn_ln_role_a(ring, P, x, pb, box);
                else phase_ffn_ln_role_b(ring, P, x, pb, box);
            } else {
                phase_ffn_ln(ring, P, x, pb);
            }
        }
        else if (type == x3::PH_LN) rstd = layer_norm(x, pb, P.gamma, P.beta, P.ln_eps);     // folded layer-1 attention
        else if (WAVES == 8 && type == x3::PH_FFN_LN_CACHED) {                         // the 128-row shape only (x3_build)
            if constexpr (WAVES == 8) {
                const long long gr = in.row_base + rowc;
                long long a = in.rowmap ? in.rowmap[gr] : gr;
                a = a < 0 ? 0 : (a >= in.n_cache ? in.n_cache - 1 : a);            // clamped as for the projection cache
                phase_ffn_ln_cached(ring, P, x, rstd, in.hcache + a * in.ldh + 4 * g, in.Q + (gr / in.rowdiv) * in.ldu + 4 * g,
                                    pb);
            }
        } else break;
    }
    if (p < G.n_phases && __builtin_amdgcn_readfirstlane(G.ph[p].type) == x3::PH_CROSS) {
        f32x4 x0[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) x0[t] = x[t];
        for (; p < G.n_phases && __builtin_amdgcn_readfirstlane(G.ph[p].type) == x3::PH_CROSS; ++p)
            phase_cross(ring, G.ph[p], x, x0, pb);
    }
    if (p < G.n_phases) phase_heads(ring, G, G.ph[p], x, logits, ld_logits, row, row_ok, g, pb);
    if (x_out != nullptr && row_ok) store_rows(x, x_out + row * ld_xout, g);
    ring.drain();
    if ((DBG & 16) && lane == 0) {            // diagnostic build: cycle stamps into the unused tail of the logits buffer
        float* dbg = logits + 3 * ld_logits + ((long long)blockIdx.x * WAVES + wave) * 4;
        dbg[0] = (float)(__builtin_amdgcn_s_memtime() - t_begin);
        dbg[1] = (DBG & 32) ? (float)ring.t_lds : (float)ring.t_wait;
        dbg[2] = (DBG & 32) ? (float)ring.t_cal : (float)ring.t_bar;
        dbg[3] = (float)ring.t_dma;
    }
}

// (the 4-wave shape could take 512 registers per wave; bounded to 256 like the 8-wave shape it ran 3 % FASTER: no AGPR traffic)
__global__ __launch_bounds__(64 * WAVES, 2) void ranker_x3b_kernel(Program G, Input in, long long rows, float* scratch,
                                                            float* x_out, long long ld_xout, float* logits,
                                                            long long ld_logits) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;

    lds_byte* pbase = (lds_byte*)smem + RING_BYTES;
    for (int o = 0; o + wave * 1024 < G.n_params * 4; o += WAVES * 1024)  // WAVES x 1 KB per pass; n_params % 1024 == 0
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(
                                             reinterpret_cast<const unsigned char*>(G.params) + o + tid * 16),
                                         (__attribute__((address_space(3))) void*)(pbase + o + wave * 1024), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_cfloat* pb = reinterpret_cast<lds_cfloat*>(pbase) + 4 * g;

    run_chain(G, in, rows, scratch, x_out, ld_xout, logits, ld_logits, smem, wave, lane, pb);
}

}  // namespace AMDREC_X3B_NAMESPACE
}  // namespace amdrec
#pragma clang diagnostic pop