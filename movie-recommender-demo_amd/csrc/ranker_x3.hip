// The fp16x3 row-owner engine of amdrec_ranker_forward (numerics, stream and program: x3_common.hpp; kernels: rowowner*.hpp).
//   ranker_x3*_kernel : input rows (dense X or cached-projection gather) -> all phases of the chain -> logits
//   amdrec_ranker_x3_prefix : debugging / test entry: run the first n phases on a dense X and return the rows
#include "rowowner.hpp"
#include "rowowner16.hpp"
#include "rowowner16c.hpp"
#include "../../include/amdrec.h"

using namespace amdrec;

// Parameter blob layout (floats; amdrec/weights.py pack_x3_params writes exactly this): per encoder layer
// [b_ov 256 | gamma1 256 | beta1 256 | b_1 d_ff | b_2 256 | gamma2 256 | beta2 256], per cross layer [bias 256], heads
// [b_1 n_tasks*h1] then per task [b_2 64 | w_3 64 | b_3 4]; padded to a multiple of 1024.  With fold_attn1 layer 1's b_ov
// is absent (the folded projection bias carries it): that layer's block starts at gamma1.
static bool x3_folded(const amdrec_ranker_params* p) { return p->x3.fold_attn1 != 0; }
static long long x3_param_floats(const amdrec_ranker_params* p) {
    const long long n = (long long)p->n_layers * (6 * 256 + p->d_ff) + 256ll * p->n_cross + (long long)p->n_tasks * (p->head_h1 + 132) -
                        (x3_folded(p) ? 256 : 0);
    return (n + 1023) / 1024 * 1024;
}

// eligibility of the engine for these parameters (the reference architecture: d_model 256, 64-wide head layer 2)
static bool x3_eligible(const amdrec_ranker_params* p) {
    if (p->x3.stream == nullptr || p->x3.chunks <= 0 || p->x3.params == nullptr) return false;
    if (p->x3.variant != 16 && p->x3.variant != 32) return false;
    if (p->x3.products != 0 && p->x3.products != 1 && p->x3.products != 3) return false;
    if (p->x3.products == 1 && p->x3.variant != 16) return false;     // the single-product kernels are 16-row kernels
    if (x3_param_floats(p) > x3::PARAM_FLOATS) return false;      // the parameter blob must fit its LDS area
    // d_ff is a placeholder without encoder layers (amdrec/weights.py pack_ranker)
    if (p->d_model != 256 || (p->n_layers > 0 && p->d_ff % 32 != 0) || p->head_h1 % 32 != 0 || p->head_h2 != 64) return false;
    if (2 * p->n_layers + p->n_cross + 1 > x3::MAX_PHASES || p->n_tasks > 4) return false;
    for (int l = 0; l < p->n_layers; ++l)
        if (p->layers[l].w_v != nullptr) return false;              // needs the pre-multiplied W_ov form
    if (x3_folded(p) && (p->n_layers < 1 || p->x3.min_rows != 1)) return false;   // see amdrec_x3_weights.fold_attn1
    return true;
}

// the column-split stream (rowowner16c.hpp) is present and the architecture fits its super-steps of four hidden tiles
static bool x3c_available(const amdrec_ranker_params* p) {
    return p->x3.variant == 16 && p->x3.stream_cs != nullptr && p->x3.chunks_cs > 0 &&
           (p->n_layers == 0 || p->d_ff % 128 == 0) && p->head_h1 % 128 == 0;
}

constexpr long long X3B4_MAX_ROWS = 256ll * 64;      // one 64-row workgroup per CU

// The kernel a pass of `rows` rows runs on.  ColSplit (rowowner16c.hpp, 16 rows per workgroup): one request's pass, <= 4096
// rows by default.  16-row variant otherwise: 64-row workgroups of four waves (one per SIMD) while the pass fits the chip
// once in that shape (<= 256 CUs x 64 rows) - it finishes in ~0.7 of the 128-row shape's time (one request's 500 rows: 0.20
// against 0.28 ms, profiles/r03_x3b_waves.log); beyond it the 128-row shape's two waves per SIMD win.
// amdrec_x3_weights.products == 1 (the single-product engine: x1b / x1b4 of rowowner16.hpp) has the two row-owner shapes of
// the 16-row kernel and nothing else: never ColSplit, never Rows32x128 (x3_eligible).
enum class X3Shape { Rows32x128, Rows16x128, Rows16x64, ColSplit };
static bool x3_single_product(const amdrec_ranker_params* p) { return p->x3.products == 1; }
static X3Shape x3_shape(const amdrec_ranker_params* p, long long rows) {
    if (x3_single_product(p)) return rows <= X3B4_MAX_ROWS ? X3Shape::Rows16x64 : X3Shape::Rows16x128;
    const long long cs_rows = p->x3.cs_max_rows > 0 ? p->x3.cs_max_rows : (p->x3.cs_max_rows < 0 ? 0 : x3c::MAX_ROWS);
    if (x3c_available(p) && rows <= cs_rows) return X3Shape::ColSplit;
    if (p->x3.variant != 16) return X3Shape::Rows32x128;
    return rows <= X3B4_MAX_ROWS ? X3Shape::Rows16x64 : X3Shape::Rows16x128;
}

// the first-FFN hidden cache (amdrec_x3_weights.stream_hc) serves this pass: everything it needs is packed, both caches
// are set, and the pass takes the 128-row shape of the 16-row kernel
static bool x3_hidden_cache(const amdrec_ranker_params* p, X3Shape shape) {
    return x3_folded(p) && shape == X3Shape::Rows16x128 && p->x3.stream_hc != nullptr && p->x3.chunks_hc > 0 &&
           p->x3.params_hc != nullptr && p->x3.w_user_uq != nullptr && p->x3.b_user_uq != nullptr &&
           p->ad_proj_cache != nullptr && p->ad_hidden_cache != nullptr && p->ld_ad_hidden_cache >= p->d_ff &&
           p->d_ff % 64 == 0 && p->d_ff >= 128;
}

// The heads a program runs: tasks first_task .. first_task + n_tasks - 1 (n_tasks < 0: all of them), behind the trunk or -
// heads_only - as the whole program [PH_HEADS], on rows that are trunk states already.  Each window has its own stream
// (amdrec_x3_weights.stream_ctr* / stream_win*); the parameter blob is the one blob, read at shifted offsets.
struct X3Window {
    int first_task = 0, n_tasks = -1;
    bool heads_only = false;
};
static X3Window x3_ctr_first_window() { return X3Window{0, 1, false}; }
static X3Window x3_winner_window(const amdrec_ranker_params* p) { return X3Window{1, p->n_tasks - 1, true}; }

// n_phases < 0: the whole chain; cs: the column-split kernel's stream; hc: the hidden-cache program (x3_hidden_cache)
static int x3_build(const amdrec_ranker_params* p, int n_phases, x3::Program& G, bool cs = false, bool hc = false,
                    X3Window win = X3Window{}) {
    memset(&G, 0, sizeof(G));
    if (win.n_tasks < 0) win.n_tasks = p->n_tasks - win.first_task;
    const bool all_tasks = win.first_task == 0 && win.n_tasks == p->n_tasks && !win.heads_only;
    const bool ctr_first = win.first_task == 0 && win.n_tasks == 1 && !win.heads_only && !all_tasks;
    const bool winners = win.first_task == 1 && win.n_tasks == p->n_tasks - 1 && win.n_tasks >= 1 && win.heads_only;
    REQUIRE(all_tasks || ctr_first || winners, "x3: no stream is packed for tasks %d .. %d%s", win.first_task,
            win.first_task + win.n_tasks - 1, win.heads_only ? " (heads only)" : "");
    REQUIRE(!(winners && hc), "x3: the heads-only program has no hidden-cache form");
    int n = 0, o = 0;                                               // o: running offset into the parameter blob (floats)
    const bool fold = x3_folded(p);
    for (int l = 0; l < p->n_layers; ++l) {
        if (win.heads_only) {                                       // no trunk phases: only the blob offset moves
            o += (l == 0 && fold ? 512 : 768) + p->d_ff + 768;
            continue;
        }
        x3::Phase& A = G.ph[n++];
        if (l == 0 && fold) {                                       // the input rows are z = x0 + W_ov x0 + b_ov: LN1 alone
            A.type = x3::PH_LN; A.gamma = o; A.beta = o + 256; A.sw1 = 1.f; A.sw2 = 1.f; A.ln_eps = p->ln_eps;
            o += 512;
        } else {
            A.type = x3::PH_ATTN_LN; A.b1 = o; A.gamma = o + 256; A.beta = o + 512; A.sw1 = p->x3.sw_ov[l];
            A.sw2 = 1.f; A.ln_eps = p->ln_eps;
            o += 768;
        }
        x3::Phase& F = G.ph[n++];
        F.type = hc && l == 0 ? x3::PH_FFN_LN_CACHED : x3::PH_FFN_LN; F.n_steps = p->d_ff / 32; F.b1 = o; F.b2 = o + p->d_ff; F.gamma = o + p->d_ff + 256;
        F.beta = o + p->d_ff + 512;
        F.sw1 = p->x3.sw_1[l]; F.sw2 = p->x3.sw_2[l]; F.hn = p->x3.hn[l]; F.hb = p->x3.hb[l]; F.ln_eps = p->ln_eps;
        o += p->d_ff + 768;
    }
    for (int c = 0; c < p->n_cross; ++c) {
        if (win.heads_only) { o += 256; continue; }
        x3::Phase& C = G.ph[n++];
        C.type = x3::PH_CROSS; C.b1 = o; C.sw1 = p->x3.sw_cross[c]; C.sw2 = 1.f;
        o += 256;
    }
    x3::Phase& H = G.ph[n++];
    // the window's part of the stacked b_1 and its tasks' vectors; the scales and the hidden bound stay those of the STACKED
    // heads (a row's hidden scale depends on them: a per-task bound would change bits)
    H.type = x3::PH_HEADS; H.n_steps = p->head_h1 / 32; H.n_tasks = win.n_tasks; H.b1 = o + win.first_task * p->head_h1;
    H.sw1 = p->x3.sw_h1; H.sw2 = p->x3.sw_h2; H.hn = p->x3.hn_head; H.hb = p->x3.hb_head;
    o += p->n_tasks * p->head_h1;
    for (int t = 0; t < p->n_tasks; ++t) {
        const int i = t - win.first_task;
        if (i >= 0 && i < win.n_tasks) { G.hb2[i] = o; G.hw3[i] = o + 64; G.hb3[i] = o + 128; }
        o += 132;
    }
    REQUIRE(p->x3.n_params == x3_param_floats(p), "x3: parameter blob has %lld floats, the architecture needs %lld",
            (long long)p->x3.n_params, x3_param_floats(p));
    G.params = hc ? p->x3.params_hc : p->x3.params;
    G.n_params = (int)p->x3.n_params;
    // chunks consumed by a prefix of the chain (the ring only needs to know where the stream ends)
    const long long per_layer = 16 + 4ll * (p->d_ff / 32);          // W_ov: 16 chunks; FFN: 64 fragment sets per hidden tile
    // heads: 8 stage-1 + 2 stage-2 groups per hidden tile; column-split: per 4 hidden tiles 8 + 4 chunks (stage 2 half empty)
    const long long hidden_tiles = (long long)win.n_tasks * (p->head_h1 / 32);
    const long long heads = cs ? hidden_tiles * 3 : hidden_tiles * 40 / 16;
    REQUIRE(cs || hidden_tiles * 40 % 16 == 0, "x3: head stream is not a whole number of chunks");
    REQUIRE(!cs || hidden_tiles % 4 == 0, "x3: column-split head stream is not a whole number of super-steps");
    // fold: no layer-1 W_ov; hc: no stage 1 of layer 1's FFN (32 of a hidden tile's 64 fragment sets)
    const long long trunk = p->n_layers * per_layer - (fold ? 16 : 0) - (hc ? 2ll * (p->d_ff / 32) : 0) + 16ll * p->n_cross;
    const long long total = (win.heads_only ? 0 : trunk) + heads;
    const amdrec_x3_weights& w = p->x3;
    const void* stream = all_tasks ? (cs ? w.stream_cs : (hc ? w.stream_hc : w.stream))
                         : ctr_first ? (cs ? w.stream_ctr_cs : (hc ? w.stream_ctr_hc : w.stream_ctr))
                                     : (cs ? w.stream_win_cs : w.stream_win);
    const long long have = all_tasks ? (cs ? w.chunks_cs : (hc ? w.chunks_hc : w.chunks))
                           : ctr_first ? (cs ? w.chunks_ctr_cs : (hc ? w.chunks_ctr_hc : w.chunks_ctr))
                                       : (cs ? w.chunks_win_cs : w.chunks_win);
    REQUIRE(stream != nullptr, "x3: the stream of this program is not packed");
    REQUIRE(total == have, "x3: stream length %lld chunks does not match the architecture (%lld)", have, total);
    G.n_phases = n_phases < 0 || n_phases > n ? n : n_phases;
    G.total_chunks = (int)total;
    G.stream = reinterpret_cast<const unsigned char*>(stream);
    return AMDREC_OK;
}

// weight elements a row is multiplied with in the program's phases (the LayerNorm-only phase has none)
static double x3_weight_elements(const x3::Program& G) {
    double w = 0;
    for (int i = 0; i < G.n_phases; ++i) {
        const x3::Phase& P = G.ph[i];
        if (P.type == x3::PH_ATTN_LN || P.type == x3::PH_CROSS) w += 256.0 * 256.0;
        else if (P.type == x3::PH_FFN_LN) w += 2.0 * 256.0 * 32.0 * P.n_steps;
        else if (P.type == x3::PH_FFN_LN_CACHED) w += 256.0 * 32.0 * P.n_steps;          // stage 2 only
        else if (P.type == x3::PH_HEADS) w += (double)P.n_tasks * (256.0 * 32.0 * P.n_steps + 64.0 * 32.0 * P.n_steps + 64.0);
    }
    return w;
}

static size_t x3_scratch_bytes(long long rows) {
    return (size_t)((rows + x3::ROWS_PER_WG - 1) / x3::ROWS_PER_WG) * x3::ROWS_PER_WG * 256 * 4;
}

// tag: the launch's profile tag, where it is not the kernel shape's own; single: the single-product kernels (Rows16x128 /
// Rows16x64 only)
static int x3_launch(const x3::Program& G, const x3::Input& in, long long rows, float* scratch, float* x_out,
                     long long ld_xout, float* logits, long long ld_logits, hipStream_t st, X3Shape shape,
                     const char* tag = nullptr, bool single = false) {
    static PerDeviceOnce attr_done;
    if (attr_done.pending()) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(x3::ranker_x3_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, x3::RING_BYTES + x3::PARAM_FLOATS * 4));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(x3b::ranker_x3b_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, x3::RING_BYTES + x3::PARAM_FLOATS * 4));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(x3b4::ranker_x3b_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, x3::RING_BYTES + x3::PARAM_FLOATS * 4));
        attr_done.mark();
    }
    if (single) {
        REQUIRE(shape == X3Shape::Rows16x128 || shape == X3Shape::Rows16x64, "x3: the single-product engine has the 16-row "
                "row-owner shapes only");
        static PerDeviceOnce attr_single;
        if (attr_single.pending()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(x1b::ranker_x3b_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, x3::RING_BYTES + x3::PARAM_FLOATS * 4));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(x1b4::ranker_x3b_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, x3::RING_BYTES + x3::PARAM_FLOATS * 4));
            attr_single.mark();
        }
    }
    if (shape == X3Shape::ColSplit) {                  // (the caller built G on that kernel's stream)
        static PerDeviceOnce attr_cs;
        if (attr_cs.pending()) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(x3c::ranker_x3c_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, x3c::LDS_BYTES));
            attr_cs.mark();
        }
        ProfScope prof(tag ? tag : "ranker_colsplit16_x3", 2.0 * (double)rows * x3_weight_elements(G), (double)rows * (1024.0 + 12.0), st);
        const int n_pre = x3c::PREFETCH_WGS;           // (A/B against 0: profiles/r03_x3c_prefetch_ab.log)
        const int n_row_wgs = (int)((rows + x3c::ROWS_PER_WG - 1) / x3c::ROWS_PER_WG);
        hipLaunchKernelGGL(x3c::ranker_x3c_kernel, dim3((unsigned)(n_row_wgs + (n_pre > 0 ? n_pre : 0))), dim3(64 * x3c::WAVES),
                           x3c::LDS_BYTES, st, G, in, rows, n_row_wgs, x_out, ld_xout, logits, ld_logits);
        HIP_TRY(hipGetLastError());
        return AMDREC_OK;
    }
    const bool small = shape == X3Shape::Rows16x64;
    const int rows_wg = small ? x3b4::ROWS_PER_WG : x3::ROWS_PER_WG;
    const unsigned grid = (unsigned)((rows + rows_wg - 1) / rows_wg);
    {
        // algorithmic FLOPs: 2 * rows * sum over the phases' weight elements (bench.py prices them against bf16 MFMA / 3)
        const double w = x3_weight_elements(G);
        const double hidden_bytes = in.hcache != nullptr ? 4.0 * 32.0 * G.ph[1].n_steps : 0.0;   // a row of P (Q: one per user)
        ProfScope prof(tag ? tag : single ? (small ? "ranker_rowowner16_64_f16" : "ranker_rowowner16_128_f16")
                       : small ? "ranker_rowowner16_64_x3" : (shape == X3Shape::Rows16x128 ? "ranker_rowowner16_128_x3" : "ranker_rowowner_128_x3"),
                       2.0 * (double)rows * w, (double)rows * (1024.0 + 12.0 + hidden_bytes), st);
        if (single && small)
            hipLaunchKernelGGL(x1b4::ranker_x3b_kernel, dim3(grid), dim3(64 * x1b4::WAVES), x3::RING_BYTES + x3::PARAM_FLOATS * 4, st,
                               G, in, rows, scratch, x_out, ld_xout, logits, ld_logits);
        else if (single)
            hipLaunchKernelGGL(x1b::ranker_x3b_kernel, dim3(grid), dim3(512), x3::RING_BYTES + x3::PARAM_FLOATS * 4, st, G, in,
                               rows, scratch, x_out, ld_xout, logits, ld_logits);
        else if (small)
            hipLaunchKernelGGL(x3b4::ranker_x3b_kernel, dim3(grid), dim3(64 * x3b4::WAVES), x3::RING_BYTES + x3::PARAM_FLOATS * 4, st,
                               G, in, rows, scratch, x_out, ld_xout, logits, ld_logits);
        else if (shape == X3Shape::Rows16x128)
            hipLaunchKernelGGL(x3b::ranker_x3b_kernel, dim3(grid), dim3(512), x3::RING_BYTES + x3::PARAM_FLOATS * 4, st, G, in,
                               rows, scratch, x_out, ld_xout, logits, ld_logits);
        else
            hipLaunchKernelGGL(x3::ranker_x3_kernel, dim3(grid), dim3(256), x3::RING_BYTES + x3::PARAM_FLOATS * 4, st, G, in,
                               rows, scratch, x_out, ld_xout, logits, ld_logits);
    }
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

// used by amdrec_ranker_forward (layers.hip)
namespace amdrec {
bool ranker_x3_wanted(const amdrec_ranker_params* p, long long rows) {
    const long long min_rows = p->x3.min_rows > 0 ? p->x3.min_rows : 8193;
    return rows >= min_rows && x3_eligible(p);
}
bool ranker_x3_folded(const amdrec_ranker_params* p) { return x3_folded(p); }
size_t ranker_x3_scratch_bytes(long long rows) { return x3_scratch_bytes(rows); }
bool ranker_x3_hidden_cache(const amdrec_ranker_params* p, long long rows) {
    return x3_eligible(p) && x3_hidden_cache(p, x3_shape(p, rows));
}
// Every pass of a `rows`-row call (layers.hip splits it at ROW_CHUNK rows) and a winner pass of that many rows would run a
// 16-row kernel on a packed CTR-first / winner stream, with the hidden-cache program wherever the all-heads call takes it.
bool ranker_x3_ctr_first_supported(const amdrec_ranker_params* p, long long rows, long long row_chunk) {
    const amdrec_x3_weights& w = p->x3;
    if (!x3_eligible(p) || w.variant != 16 || p->n_tasks < 2) return false;
    if (w.stream_ctr == nullptr || w.chunks_ctr <= 0 || w.stream_win == nullptr || w.chunks_win <= 0) return false;
    const long long pass[2] = {rows < row_chunk ? rows : row_chunk, rows > row_chunk ? rows % row_chunk : 0};
    for (long long m : pass) {
        if (m <= 0) continue;
        if (!ranker_x3_wanted(p, m)) return false;
        const X3Shape shape = x3_shape(p, m);
        if (shape == X3Shape::ColSplit && (w.stream_ctr_cs == nullptr || w.chunks_ctr_cs <= 0 || w.stream_win_cs == nullptr ||
                                           w.chunks_win_cs <= 0))
            return false;
        if (x3_hidden_cache(p, shape) && (w.stream_ctr_hc == nullptr || w.chunks_ctr_hc <= 0)) return false;
    }
    return true;
}
// ldu: leading dimension of U; > 256 = the user projection wrote [U | Q] rows (Q = W_1c u_user at U + 256).
// ctr_first: the trunk and the head of task 0 only (logits: that one row), each row's trunk state to x_out (may be nullptr).
int ranker_x3_run(const amdrec_ranker_params* p, const float* X, long long ldx, const float* U, long long ldu,
                  const long long* rowmap, long long row_base, int rowdiv, long long n_cache, long long rows, float* scratch,
                  float* logits, long long ld_logits, hipStream_t st, bool ctr_first, float* x_out, long long ld_xout) {
    const X3Shape shape = x3_shape(p, rows);
    const bool hc = X == nullptr && ldu >= 256 + p->d_ff && x3_hidden_cache(p, shape);
    REQUIRE(!ctr_first || shape != X3Shape::Rows32x128, "x3: the CTR-first program needs the 16-row kernels (x3.variant 16)");
    x3::Program G;
    int rc = x3_build(p, -1, G, shape == X3Shape::ColSplit, hc, ctr_first ? x3_ctr_first_window() : X3Window{});
    if (rc) return rc;
    x3::Input in{};
    in.ldu = 256;
    if (X != nullptr) {
        in.X = X; in.ldx = ldx;
    } else {
        in.cache = p->ad_proj_cache; in.ldc = p->ld_ad_proj_cache; in.n_cache = n_cache; in.rowmap = rowmap; in.U = U;
        in.row_base = row_base; in.rowdiv = rowdiv; in.ldu = ldu;
        if (hc) { in.hcache = p->ad_hidden_cache; in.ldh = p->ld_ad_hidden_cache; in.Q = U + 256; }
    }
    return x3_launch(G, in, rows, scratch, x_out, ld_xout, logits, ld_logits, st, shape, nullptr, x3_single_product(p));
}
}  // namespace amdrec

// ---- CTR-first ranking, pass 2: the other heads on the winners' stored trunk rows (amdrec.h) ----
namespace {
struct WinnerWs : Carver {
    float* logits;             // [n_tasks - 1][rows] (the 16-row kernels use no scratch rows)
    WinnerWs(const amdrec_ranker_params* p, long long rows, void* ws) : Carver(ws) {
        logits = take<float>((size_t)(p->n_tasks - 1) * (size_t)rows);
    }
};
}  // namespace
namespace amdrec {
size_t ranker_x3_winner_workspace(const amdrec_ranker_params* p, long long rows) {
    return WinnerWs(p, rows > 0 ? rows : 0, nullptr).bytes();
}
}  // namespace amdrec

// out[t + 1][i] = sigmoid(logits[t][i]) for the winner rows i, 0.0 where the selection left the slot empty - the value
// amdrec_select_topk writes there for the ranking task
__global__ __launch_bounds__(256) void winner_scores_kernel(const float* logits, const int* slots, long long n, int n_planes,
                                                            float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool valid = slots[i] >= 0;
    for (int t = 0; t < n_planes; ++t) out[(long long)(t + 1) * n + i] = valid ? sigmoid_prob(logits[(long long)t * n + i]) : 0.0f;
}

extern "C" int amdrec_ranker_winner_heads(const amdrec_ranker_params* p, const float* trunk, int64_t ld_trunk,
                                          int64_t n_trunk_rows, const int32_t* slots, int64_t n_users, int k_c, int top_k,
                                          float* out_scores, void* workspace, size_t workspace_bytes, void* stream) {
    REQUIRE(p != nullptr, "params is null");
    REQUIRE(k_c >= 1 && k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(top_k >= 1 && top_k <= AMDREC_MAX_K, "top_k out of range");
    if (n_users <= 0) return AMDREC_OK;
    const long long rows = (long long)n_users * top_k;
    REQUIRE(rows < (1ll << 31), "n_users * top_k out of range");
    REQUIRE(trunk && slots && out_scores, "null pointer");
    REQUIRE(ld_trunk >= 256 && ld_trunk % 4 == 0 && ((uintptr_t)trunk % 16) == 0, "bad trunk layout");
    REQUIRE(n_trunk_rows >= (long long)n_users * k_c, "trunk has fewer rows than n_users * k_c");
    REQUIRE(ranker_x3_ctr_first_supported(p, rows, rows), "these parameters cannot run the heads-only program on %lld rows (no "
            "winner stream packed, or not the 16-row fp16x3 engine)", rows);
    const WinnerWs w(p, rows, workspace);
    int rc = require_workspace(workspace, workspace_bytes, w.bytes());
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const X3Shape shape = x3_shape(p, rows);
    x3::Program G;
    if ((rc = x3_build(p, -1, G, shape == X3Shape::ColSplit, false, x3_winner_window(p)))) return rc;
    x3::Input in{};
    in.X = trunk; in.ldx = ld_trunk; in.ldu = 256;
    in.slots = slots; in.top_k = top_k; in.k_c = k_c; in.n_x = n_trunk_rows;
    if ((rc = x3_launch(G, in, rows, nullptr, nullptr, 0, w.logits, rows, st, shape,
                        x3_single_product(p) ? "ranker_winner_heads_f16" : "ranker_winner_heads_x3", x3_single_product(p)))) return rc;
    hipLaunchKernelGGL(winner_scores_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, w.logits, slots, rows,
                       p->n_tasks - 1, out_scores);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

// test / debugging entry only: z[r] = x0[r] + (W_ov x0[r] + b_ov), one workgroup per row, thread f = output feature (fp32 fma
// chain over k ascending, the generic path's order of the bias and the residual)
__global__ __launch_bounds__(256) void x3_fold_rows_kernel(const float* X, long long ldx, const float* W, long long ldw,
                                                           const float* b, float* Z) {
    __shared__ float xr[256];
    const long long r = blockIdx.x;
    const int f = threadIdx.x;
    xr[f] = X[r * ldx + f];
    __syncthreads();
    const float* w = W + f * ldw;
    float acc = 0.f;
    for (int k = 0; k < 256; ++k) acc = __builtin_fmaf(w[k], xr[k], acc);
    Z[r * 256 + f] = xr[f] + (acc + b[f]);
}

extern "C" int amdrec_ranker_x3_prefix(const amdrec_ranker_params* p, const float* X, int64_t ldx, int64_t rows,
                                       int n_phases, float* x_out, int64_t ld_out, float* logits, int64_t ld_logits,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    REQUIRE(p != nullptr && X != nullptr, "null pointer");
    REQUIRE(x3_eligible(p), "these parameters are not eligible for the fp16x3 engine (or carry no x3 stream)");
    if (rows <= 0) return AMDREC_OK;
    REQUIRE(ldx >= 256 && ldx % 4 == 0 && ((uintptr_t)X % 16) == 0, "bad X layout");
    REQUIRE(x_out == nullptr || (ld_out >= 256 && ld_out % 4 == 0 && ((uintptr_t)x_out % 16) == 0), "bad x_out layout");
    const X3Shape shape = x3_shape(p, rows);
    x3::Program G;
    int rc = x3_build(p, n_phases, G, shape == X3Shape::ColSplit);
    if (rc) return rc;
    const bool heads = G.n_phases == 2 * p->n_layers + p->n_cross + 1;
    REQUIRE(!heads || (logits != nullptr && ld_logits >= rows), "the full chain needs a logits buffer");
    const size_t need = x3_scratch_bytes(rows);
    if ((rc = require_workspace(workspace, workspace_bytes, need))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* scratch = reinterpret_cast<float*>(workspace);
    x3::Input in{};
    in.X = X; in.ldx = ldx; in.ldu = 256;
    if (x3_folded(p)) {
        // X is x0; the folded chain wants z = x0 + W_ov x0 + b_ov.  z goes to the scratch rows (row r at r * 256): the
        // 32-row kernel later stores a row's x0 of the cross layers over that same row, after its own lane has read it
        const amdrec_encoder_layer& L = p->layers[0];
        REQUIRE(L.w_o != nullptr && L.b_o != nullptr && L.ldw_dm >= 256, "x3: folded parameters without layer 1's W_ov / b_ov");
        hipLaunchKernelGGL(x3_fold_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, X, (long long)ldx, L.w_o,
                           (long long)L.ldw_dm, L.b_o, scratch);
        HIP_TRY(hipGetLastError());
        in.X = scratch; in.ldx = 256;
    }
    return x3_launch(G, in, rows, scratch, x_out, ld_out, logits, ld_logits, st, shape, nullptr, x3_single_product(p));
}
