// IVF-Flat search (replaces faiss IndexIVFFlat(METRIC_INNER_PRODUCT).search behind FAISSIndex.search,
// faiss_retrieval.py:50-55, :150-155).  The coarse step (nprobe best centroids by inner product)
// reuses amdrec_flat_search on the centroid table; here:
//   ivf_scan   : one workgroup per (query, probed list): inner product of the query with every row
//                of the list (rows stored list-contiguous), written as 64-bit (score, ~position)
//                keys into the query's pool.  Wave-per-row float4 streaming: HBM/L2-bound.
//   ivf_select : per query, exact k largest keys of its pool: 64-bit LDS-histogram radix select
//                (6 passes), compaction, bitonic sort.  Keys are unique (lists are disjoint), so the
//                selection is exact and deterministic for every input - no sampling, no fix-up.
#include <tuple>
#include "gemm_core.hpp"
#include "topk_utils.hpp"
#include "invlists.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

// EL (ListNoElig or ListElig, invlists.hpp): the eligibility predicate; EP: its pointers as trailing kernel arguments - none
// for ListNoElig, whose instantiation takes the arguments the kernel always took and compiles to the code it always was;
// (list_tags, all, any) for ListElig.  The scans below take them the same way.  This scan is a slot mode: an ineligible
// (query, row) slot is stored as key 0, the select's EMPTY-slot value - stored, not skipped: the pool is not cleared
// between searches.
// BO (ListNoBoost or ListBoost, invlists.hpp): the stage-1 score boost, taken the same way - its pointers (list_boosts,
// weight) follow the eligibility pointers; ListNoBoost adds none.  A boosted scan files s = ip + w_q * boost[r] (boost_add /
// boost_term: two rounded operations) where the plain one files ip, under the same rules (rank_last, key 0 when ineligible).
template <class EL = ListNoElig, class BO = ListNoBoost, class... EP>
__global__ __launch_bounds__(256) void ivf_scan_kernel(const float* xs, long long ld, int d, const long long* spos,
                                                       const long long* list_off, const float* Q, long long ldq,
                                                       const long long* probes, const long long* base, int nprobe,
                                                       unsigned long long* keys, long long pool_ld,
                                                       long long pos_offset, EP... tail) {
    __shared__ __attribute__((aligned(16))) float qv[2048];
    const ListPreds<EL, BO> preds = list_preds(tail...);
    const EL el = preds.el;
    [[maybe_unused]] const BO bo = preds.bo;
    const int q = blockIdx.y, p = blockIdx.x;
    const long long l = probes[(long long)q * nprobe + p];
    if (l < 0) return;
    const long long r0 = list_off[l];
    long long r1 = list_off[l + 1];
    if (r1 <= r0) return;
    // gridDim.z workgroups share the list's rows (whole 32-row rounds each): one request against the reference's default
    // index (nlist 100, nprobe 10: ten lists of 10 000 rows at 1M ads) was ten workgroups streaming 10 MB each - 1 ms
    long long rb = r0;
    if (gridDim.z > 1) {
        const long long per = ((r1 - r0 + gridDim.z - 1) / gridDim.z + 31) / 32 * 32;
        rb = r0 + (long long)blockIdx.z * per;
        if (rb >= r1) return;
        if (rb + per < r1) r1 = rb + per;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < d; i += 256) qv[i] = Q[(long long)q * ldq + i];
    __syncthreads();
    unsigned long long* dst = keys + (long long)q * pool_ld + base[(long long)q * nprobe + p];
    const int d4 = d >> 2;
    constexpr int NW = 4, U = 8;
    const typename EL::Mask mq = el.mask(q);
    [[maybe_unused]] const typename BO::Weight wq = bo.w(q);
    for (long long row0 = rb; row0 < r1; row0 += NW * U) {
        float part[U];
        const f32x4* xr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long r = row0 + w * U + u;
            r = r < r1 ? r : r1 - 1;                           // clamped: branch-free loads, result dropped below
            xr[u] = reinterpret_cast<const f32x4*>(xs + r * ld);
            part[u] = 0.f;
        }
        // column chunk outermost so that the U row loads of a chunk are in flight together (with the row loop
        // outside, each row's load had to return before the next row's was issued)
        for (int c = lane; c < d4; c += 64) {
            const f32x4 y = *reinterpret_cast<const f32x4*>(&qv[4 * c]);
            f32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = xr[u][c];
#pragma unroll
            for (int u = 0; u < U; ++u)        // fma4's chain written out (through the helper the eight slots compile to another
                                               // instruction order): the same rounding sequence in every slot u
                part[u] = __builtin_fmaf(x[u][3], y[3], __builtin_fmaf(x[u][2], y[2], __builtin_fmaf(x[u][1], y[1],
                                         __builtin_fmaf(x[u][0], y[0], part[u]))));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a = part[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            const long long r = row0 + w * U + u;
            if constexpr (BO::on) {
                if (lane == 0 && r < r1) {
                    const float s = BO::apply(a, wq, bo.row(r));
                    dst[r - r0] = EL::ok(el.tag(r), mq) ? make_key(rank_last(s), (uint32_t)(spos[r] + pos_offset)) : 0ull;
                }
            } else if constexpr (EL::on) {
                if (lane == 0 && r < r1)
                    dst[r - r0] = EL::ok(el.tag(r), mq) ? make_key(rank_last(a), (uint32_t)(spos[r] + pos_offset)) : 0ull;
            } else {
                if (lane == 0 && r < r1) dst[r - r0] = make_key(rank_last(a), (uint32_t)(spos[r] + pos_offset));
            }
        }
    }
}

// ---- batched scan: queries grouped by list, one fp32-MFMA GEMM tile per (list, 64 queries, 256 rows) ----
// The per-pair scan above re-reads a list once per probing query; with hundreds of queries per
// batch every list is probed by many of them, so the (query, probe) pairs are sorted by list (host-side
// integer plumbing) and each list is read ONCE per 64-query group: P = gathered queries (registers),
// Q = list rows (lanes -> a store instruction writes 2 x 32 consecutive keys of two queries' pools).
struct GatherRows {
    const float* base;
    const long long* idx;   // row r of the group -> base[idx[r]]
    long long n;
    int ld, K;
    using RowState = int;                     // the gathered row, resolved once per staged row
    __device__ __forceinline__ RowState row_state(long long r) const { return (int)idx[r < n ? r : n - 1]; }
    __device__ __forceinline__ bool k_valid(int k) const { return k < K; }
    __device__ __forceinline__ f32x4 load(RowState row, int k) const {
        return *reinterpret_cast<const f32x4*>(base + (long long)row * ld + k);
    }
};

template <class EL, class BO = ListNoBoost>
struct EpiIvfKeysT {
    static constexpr const char* name = BO::on ? (EL::on ? "ivf_scan_elig_boost" : "ivf_scan_boost") : (EL::on ? "ivf_scan_elig" : "ivf_scan");
    static constexpr double out_bytes_per_elem = 2.0;
    static constexpr size_t lds_bytes(int) { return 0; }
    const long long* spos;      // positions of this list's rows
    long long list_rows;
    const long long* pair_q;    // this list's group: query of member j
    const long long* pair_p;    //                    probe slot of member j
    long long g;
    const long long* base;      // [nq][nprobe] pool offsets
    int nprobe;
    unsigned long long* keys;
    long long pool_ld, pos_offset;
    // filter mode (tau != nullptr): only rows with score >= tau[q * ld_tau] are kept, appended at fill[q]++ (the caller
    // seeds fill[q] with the keys already in the query's pool row); base / pair_p are not used
    const float* tau;
    long long ld_tau;
    unsigned long long* fill;
    // eligibility (rows counted from the list's first, as spos): slot mode stores key 0, the select's empty-slot value, for
    // an ineligible (query, row) element; filter mode tests the predicate with the threshold and does not append the row
    [[no_unique_address]] EL el;
    // boost (rows counted from the list's first, as spos): both modes see s = BO::apply(ip, w_q, boost[row]) where the plain
    // scan sees ip - the slot's key, and the value compared with tau (the k-th BOOSTED score of the first phase)
    [[no_unique_address]] BO bo;
    template <class A>
    __device__ void operator()(A& acc, float*) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
        // Everything the 16 accumulator rows of a tile need from memory - the member's query, its threshold or pool offset -
        // is fetched for all 16 FIRST (independent loads, in flight together), then the rows' positions; round 3 resolved
        // pair_q -> tau / pair_p -> base row by row inside the store loop: 32-48 dependent round trips per workgroup,
        // longer than the tile's MFMAs on short lists.
        long long rowq[TQ], posq[TQ];
        typename EL::Tag tagq[TQ];
        [[maybe_unused]] typename BO::Row bq[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            rowq[j] = acc.q(j, lane);                             // row inside the list
            posq[j] = rowq[j] < list_rows ? spos[rowq[j]] + pos_offset : -1;
            tagq[j] = rowq[j] < list_rows ? el.tag(rowq[j]) : typename EL::Tag{};
            if constexpr (BO::on) bq[j] = rowq[j] < list_rows ? bo.row(rowq[j]) : typename BO::Row{};
        }
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            long long qv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long jj = acc.p(i, r, lane);          // member of the group (depends on the lane half)
                qv[r] = jj < g ? pair_q[jj] : -1;
            }
            // the queries' two mask words, fetched with the tau / base loads, folded with the rows' tags into one bit per
            // element (r * TQ + j) at once: the sixteen mask pairs are dead before the store loop (held through it they
            // took the 64 x 256 tiles to the register limit)
            uint64_t okb = 0ull;
            if constexpr (EL::on) {
                static_assert(16 * TQ <= 64, "one eligibility bit per accumulator element of a tile row");
                typename EL::Mask mv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) mv[r] = el.mask(qv[r]);
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int j = 0; j < TQ; ++j) okb |= (uint64_t)EL::ok(tagq[j], mv[r]) << (r * TQ + j);
            }
            (void)okb;
            // the queries' weights, with the tau / base loads
            [[maybe_unused]] typename BO::Weight wv[16];
            if constexpr (BO::on) {
#pragma unroll
                for (int r = 0; r < 16; ++r) wv[r] = bo.w(qv[r]);
            }
            if (tau != nullptr) {
                float tv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) tv[r] = qv[r] >= 0 ? tau[qv[r] * ld_tau] : __builtin_nanf("");   // NaN: no score passes
#pragma unroll
                for (int r = 0; r < 16; ++r) {
#pragma unroll
                    for (int j = 0; j < TQ; ++j) {
                        const float sc = rank_last(BO::apply(acc.v[i][j][r], wv[r], bq[j]));
                        if (sc >= tv[r] && posq[j] >= 0 && (!EL::on || ((okb >> (r * TQ + j)) & 1ull)))
                            (keys + qv[r] * pool_ld)[atomicAdd(&fill[qv[r]], 1ull)] = make_key(sc, (uint32_t)posq[j]);
                    }
                }
                continue;
            }
            long long off[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long jj = acc.p(i, r, lane);
                off[r] = qv[r] >= 0 ? pair_p[jj] : 0;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) off[r] = qv[r] >= 0 ? qv[r] * pool_ld + base[qv[r] * nprobe + off[r]] : -1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (off[r] < 0) continue;
                unsigned long long* dst = keys + off[r];
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    if (posq[j] < 0) continue;
                    if constexpr (EL::on)
                        dst[rowq[j]] = ((okb >> (r * TQ + j)) & 1ull)
                                           ? make_key(rank_last(BO::apply(acc.v[i][j][r], wv[r], bq[j])), (uint32_t)posq[j]) : 0ull;
                    else
                        dst[rowq[j]] = make_key(rank_last(BO::apply(acc.v[i][j][r], wv[r], bq[j])), (uint32_t)posq[j]);
                }
            }
        }
    }
};

// ---- filter mode with a bf16 PREFILTER (round 4) ------------------------------------------------------------------------
// The second phase of the two-phase scan keeps only rows with score >= tau_q and most of a batch's (query, probe) pairs are
// second-phase pairs: 0.64 of the 0.80 ms scan at the per-rank shape of an 8-way sharded 10M index, fp32-MFMA-bound (64
// queries per list).  Their GEMM runs here on a bf16 shadow of the lists and bf16 queries (v_mfma_f32_32x32x16_bf16: 16x the
// fp32 MFMA rate, half the list bytes) and decides only which rows MAY pass: a row with fp32 score >= tau has a bf16 score
// >= tau - eps_q (eps_bound: the flat search's measured-rounding-error bound, with M / D of the list shadow), so every row
// with approx >= tau_lo[q] = tau[q] - eps_q is RE-SCORED in fp32 from the fp32 list row - one wave per row, one explicit
// fma chain per lane and a fixed reduction order, so a row's score does not depend on which workgroup handled it - and
// appended if that exact score passes tau.  The pool holds exact fp32 keys as before; nothing downstream changes.
// Hits of a whole tile are collected in one list in LDS (the staging area, free after the K loop), then the workgroup's
// waves share them; a hit that finds the list full is re-scored by its own lane, in the same summation order (rescore1).
template <class EL, class BO = ListNoBoost>
struct EpiIvfPrefilterT {
    static constexpr const char* name = BO::on ? (EL::on ? "ivf_scan_bf16_elig_boost" : "ivf_scan_bf16_boost")
                                               : (EL::on ? "ivf_scan_bf16_elig" : "ivf_scan_bf16");
    static constexpr double out_bytes_per_elem = 0.0;
    static constexpr size_t lds_bytes(int) { return 0; }        // reuses the staging tiles (checked against their size below)
    const long long* spos;      // positions of this list's rows
    long long list_rows;
    const long long* pair_q;    // this list's group: query of member j
    long long g;
    unsigned long long* keys;
    long long pool_ld, pos_offset;
    const float* tau;           // exact filter: fp32 score >= tau[q * ld_tau] (minus the slack below)
    long long ld_tau;
    const float* tau_lo;        // prefilter: bf16 score >= tau_lo[q]
    unsigned long long* fill;
    const float* xs;            // this list's fp32 rows
    long long ld;
    const float* Q;             // fp32 queries
    long long ldq;
    int d;
    // eligibility (rows counted from the list's first, as spos): tested at nomination, BEFORE the hit enters the LDS list -
    // an ineligible row costs neither a list slot nor the fp32 row read of the re-score; rescore16 / rescore1 / keep only
    // ever see eligible rows
    [[no_unique_address]] EL el;
    // boost (rows counted from the list's first, as spos): nomination compares boost_add(bf16 score, t) with tau_lo - the
    // bound widened for the two roundings, ivf_filter_bounds_kernel -; keep files boost_add(fp32 re-score, t) with the
    // same t (an overflow hit passes its own, a listed hit reads the row's boost and the query's weight again), so
    // rescore16 and rescore1 hits file the same value
    [[no_unique_address]] BO bo;
    // fp32 score of (list row, query) by the 16 lanes of a quarter wave (sub = lane & 15); every lane returns the sum
    __device__ __forceinline__ float rescore16(long long row, long long q, int sub) const {
        const f32x4* xr = reinterpret_cast<const f32x4*>(xs + row * ld);
        const f32x4* qr = reinterpret_cast<const f32x4*>(Q + q * ldq);
        float part = 0.f;
        for (int c = sub; c < (d >> 2); c += 16) {
            const f32x4 x = xr[c], y = qr[c];
            part = fma4(x, y, part);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        return part;
    }
    // the same score, bit for bit, by ONE lane.  Which nominations of a crowded tile miss the list is decided by a race for
    // its slots, so the two must agree or a row's score would change from run to run.  rescore16's xor butterfly, seen from
    // lane 0, is a balanced tree whose leaves in order are the sixteen chains in bit-reversed order: sum them pairwise with
    // one pending value per level.  Kept a rolled loop: it is expanded once per accumulator element of the caller.
    __device__ __forceinline__ float rescore1(long long row, long long q) const {
        const f32x4* xr = reinterpret_cast<const f32x4*>(xs + row * ld);
        const f32x4* qr = reinterpret_cast<const f32x4*>(Q + q * ldq);
        float l1 = 0.f, l2 = 0.f, l4 = 0.f, l8 = 0.f, sum = 0.f;          // pending sums of 1, 2, 4, 8 chains
#pragma clang loop unroll(disable)
        for (int t = 0; t < 16; ++t) {
            float v = 0.f;
            for (int c = (int)(__brev((unsigned)t) >> 28); c < (d >> 2); c += 16) {
                const f32x4 x = xr[c], y = qr[c];
                v = fma4(x, y, v);
            }
            if (!(t & 1)) { l1 = v; continue; }
            v = l1 + v;
            if (!(t & 2)) { l2 = v; continue; }
            v = l2 + v;
            if (!(t & 4)) { l4 = v; continue; }
            v = l4 + v;
            if (!(t & 8)) { l8 = v; continue; }
            sum = l8 + v;
        }
        return sum;
    }
    // the threshold is the k-th score of the first phase, computed by the fp32 MFMA; the re-score sums in another order
    // (1e-7-level differences): a slack towards KEEPING never costs exactness, the select decides
    // (bt: the pair's boost term, the one its nomination added to the bf16 score)
    __device__ __forceinline__ void keep(float sc, long long row, long long q, typename BO::Term bt = {}) const {
        if constexpr (BO::on) sc = BO::add(sc, bt);
        sc = rank_last(sc);
        const float t = tau[q * ld_tau];
        if (sc >= t - 1e-6f * fmaxf(1.f, fabsf(t)) || t == -INFINITY)
            (keys + q * pool_ld)[atomicAdd(&fill[q], 1ull)] = make_key(sc, (uint32_t)(spos[row] + pos_offset));
    }
    template <class A>
    __device__ void operator()(A& acc, float* smem) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        constexpr int NWAVES = A::WP * A::WQ;
        // the nominations of the whole tile in ONE list over the staging tiles; a nomination that does not fit is re-scored
        // by its own lane on the spot (a tile with thousands of nominations: tau is not selective there)
        constexpr int BP = A::WP * TP * 32;
        constexpr size_t STAGE_BYTES = (size_t)(A::WP * TP + A::WQ * TQ) * 32 * BK * sizeof(float);
        constexpr int CAP = (int)((STAGE_BYTES - 16 - (EL::on ? (size_t)BP * 16 : 0)) / 8);
        static_assert(BP <= NWAVES * 64 && CAP >= 256, "one query's masks per thread; room for a tile's nominations");
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        int* cnt = reinterpret_cast<int*>(smem);
        unsigned long long* hits = reinterpret_cast<unsigned long long*>(smem + 4);     // (query << 32) | row in the list
        long long rowq[TQ];
        typename EL::Tag tagq[TQ];
        [[maybe_unused]] typename BO::Row bq[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            rowq[j] = acc.q(j, lane);
            tagq[j] = rowq[j] < list_rows ? el.tag(rowq[j]) : typename EL::Tag{};
            if constexpr (BO::on) bq[j] = rowq[j] < list_rows ? bo.row(rowq[j]) : typename BO::Row{};
        }
        // member -> query -> prefilter threshold for all of this lane's accumulator rows at once: two dependent round
        // trips per tile (fetched round by round they were eight)
        int qv[TP][16];
        float tv[TP][16];
#pragma unroll
        for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long jj = acc.p(i, r, lane);
                qv[i][r] = jj < g ? (int)pair_q[jj] : -1;
            }
#pragma unroll
        for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) tv[i][r] = qv[i][r] >= 0 ? tau_lo[qv[i][r]] : __builtin_nanf("");
        [[maybe_unused]] typename BO::Weight wv[TP][16];                   // the queries' weights, with the tau_lo loads
        if constexpr (BO::on) {
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) wv[i][r] = bo.w(qv[i][r]);
        }
        // eligibility: the two mask words of the tile's BP queries go to the END of the staging area (one query per thread:
        // pair_q -> all / any, in flight with the pair_q -> tau_lo loads above; the nomination list gives up BP * 16 bytes)
        // and a hit reads its query's pair from there.  Held in registers - sixteen pairs per lane, or folded into a bit
        // per accumulator element - they spilled the 64 x 256 tile.
        const uint64_t* lmask = nullptr;
        if constexpr (EL::on) {
            uint64_t* lm = reinterpret_cast<uint64_t*>(smem) + (STAGE_BYTES / 8 - 2 * BP);
            const long long jj = (long long)(acc.p0 - acc.wp * TP * 32) + tid;
            if (tid < BP) {
                const typename EL::Mask m = el.mask(jj < g ? pair_q[jj] : -1);
                lm[2 * tid] = m.all;
                lm[2 * tid + 1] = m.any;
            }
            lmask = lm;
        }
        (void)lmask;
        if (tid == 0) *cnt = 0;
        __syncthreads();                                                  // (also: every wave has left the staging tiles)
#pragma unroll
        for (int i = 0; i < TP; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int j = 0; j < TQ; ++j) {
                    [[maybe_unused]] const typename BO::Term t = BO::term(wv[i][r], bq[j]);
                    const float a = BO::add(acc.v[i][j][r], t);
                    // NaN approx (NaN rows / queries): re-score, the exact path decides; NaN threshold: member absent
                    if ((a >= tv[i][r] || (!(a == a) && tv[i][r] == tv[i][r])) && rowq[j] < list_rows) {
                        if constexpr (EL::on) {
                            const int m = acc.wp * TP * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);   // acc.p() inside the tile
                            if (!EL::ok(tagq[j], typename EL::Mask{lmask[2 * m], lmask[2 * m + 1]})) continue;
                        }
                        const int slot = atomicAdd(cnt, 1);
                        if (slot < CAP) {
                            hits[slot] = ((unsigned long long)(uint32_t)qv[i][r] << 32) | (unsigned long long)rowq[j];
                        } else {
                            if constexpr (BO::on) keep(rescore1(rowq[j], qv[i][r]), rowq[j], qv[i][r], t);
                            else keep(rescore1(rowq[j], qv[i][r]), rowq[j], qv[i][r]);
                        }
                    }
                }
        __syncthreads();
        const int n = *cnt < CAP ? *cnt : CAP;
        // four nominations per wave at a time (a quarter wave each), two rounds in flight
        const int grp = lane >> 4, sub = lane & 15;
        int h = wave * 4 + grp;
        for (; h + NWAVES * 4 < n; h += 2 * NWAVES * 4) {
            const unsigned long long e0 = hits[h], e1 = hits[h + NWAVES * 4];
            const long long q0 = (long long)(e0 >> 32), r0 = (long long)(e0 & 0xffffffffull);
            const long long q1 = (long long)(e1 >> 32), r1 = (long long)(e1 & 0xffffffffull);
            const float s0 = rescore16(r0, q0, sub), s1 = rescore16(r1, q1, sub);
            if constexpr (BO::on) {
                if (sub == 0) { keep(s0, r0, q0, BO::term(bo.w(q0), bo.row(r0))); keep(s1, r1, q1, BO::term(bo.w(q1), bo.row(r1))); }
            } else {
                if (sub == 0) { keep(s0, r0, q0); keep(s1, r1, q1); }
            }
        }
        if (h < n) {
            const unsigned long long e0 = hits[h];
            const long long q0 = (long long)(e0 >> 32), r0 = (long long)(e0 & 0xffffffffull);
            const float s0 = rescore16(r0, q0, sub);
            if constexpr (BO::on) {
                if (sub == 0) keep(s0, r0, q0, BO::term(bo.w(q0), bo.row(r0)));
            } else {
                if (sub == 0) keep(s0, r0, q0);
            }
        }
        __syncthreads();                                                  // the staging tiles are the next row tile's again
    }
};

// tau_lo[q] = tau[q] - eps_q for the prefilter above: one wave per query (||q||, ||bf16(q) - q|| from the two copies of the
// query, M / D from the list shadow's max_norm).  tau = -inf (fewer than k rows in the first phase) stays -inf.
//
// BOOSTED scans (BP = weight [nq], boost_max): nomination compares fl(a + t) with tau_lo, where a is the bf16 score, t =
// fl(w_q * boost[r]) the term both sides share, and a row must be nominated whenever its exact key s = fl(ip + t) >= tau.
// With u = 2^-24, fl(x) >= x - u |x| and |ip - a| <= eps_q:
//     fl(a + t) >= (a + t) - u |a + t| >= (ip + t) - eps_q - u |a + t| >= s - u |ip + t| - eps_q - u |a + t|
//               >= tau - eps_q - u (|ip + t| + |a + t|),
// and |ip + t| <= P, |a + t| <= P + eps_q for P = |w_q| boost_max + ||q|| (M + D)  (|t| <= |w_q| boost_max (1 + u), folded
// into the factor below).  So tau_lo = tau - eps_q - 2u (P + eps_q) nominates every such row; the kernel takes 5u for 2u: the
// two subtractions that form tau_lo round too (each by at most u times a value no larger than P + eps_q), and a bound that
// is too low costs re-scores, never a row.  A non-finite P (a NaN / inf weight) re-scores everything, like a non-finite eps.
__device__ __forceinline__ float boost_bound_slack(long long q, float qn, float eps, float md, const float* weight, float boost_max) {
    return 3.0e-7f * (fabsf(weight[q]) * boost_max + qn * md + eps);
}
template <class... BP>
__global__ __launch_bounds__(256) void ivf_filter_bounds_kernel(const float* Q, long long ldq, const uint16_t* Q16, long long ldq16,
                                                                int d, long long nq, const float* max_norm, const float* tau,
                                                                long long ld_tau, float* tau_lo, BP... bp) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    float qn = 0.f, dqn = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float v = Q[q * ldq + c];
        const float b = __uint_as_float((uint32_t)Q16[q * ldq16 + c] << 16);
        qn += v * v;
        dqn += (b - v) * (b - v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { qn += __shfl_xor(qn, o, 64); dqn += __shfl_xor(dqn, o, 64); }
    if (lane == 0) {
        const float eps = eps_bound(sqrtf(qn), sqrtf(dqn) * 1.0001f, max_norm[0], max_norm[1], d);
        const float t = tau[q * ld_tau];
        if constexpr (sizeof...(BP) == 0) {
            tau_lo[q] = (eps < INFINITY) ? t - eps : -INFINITY;           // NaN / inf norms: everything is re-scored
        } else {
            const float slack = boost_bound_slack(q, sqrtf(qn), eps, max_norm[0] + max_norm[1], bp...);
            tau_lo[q] = (eps < INFINITY && slack < INFINITY) ? t - eps - slack : -INFINITY;
        }
    }
}

template <class S, class EL = ListNoElig, class BO = ListNoBoost, class... EP>
__global__ __launch_bounds__(S::NT, 2) void ivf_group_scan_mixed_kernel(
    const float* xs, long long ld, const uint16_t* xs16, long long ld16, int d, int ksteps, const long long* spos,
    const long long* list_off, const float* Q, long long ldq, const uint16_t* Q16, long long ldq16, const long long* goff,
    const long long* qt_prefix, int nlist, const long long* pair_q, unsigned long long* keys, long long pool_ld,
    long long pos_offset, const float* tau, long long ld_tau, const float* tau_lo, unsigned long long* fill, EP... tail) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ListPreds<EL, BO> preds = list_preds(tail...);
    const EL el = preds.el;
    const BO bo = preds.bo;
    const long long y = blockIdx.y;
    if (y >= qt_prefix[nlist]) return;
    const int l = tile_list(y, qt_prefix, nlist);
    const long long r0 = list_off[l], len = list_off[l + 1] - r0;
    if ((long long)blockIdx.x * S::BQ >= len) return;
    const long long g0 = goff[l], g = goff[l + 1] - g0;
    // the bf16 matrices as float matrices of d / 2 columns (gemm_core.hpp, Shape::BF16)
    GatherRows lp{reinterpret_cast<const float*>(Q16), pair_q + g0, g, (int)(ldq16 / 2), d / 2};
    DenseRows lq{reinterpret_cast<const float*>(xs16 + r0 * ld16), len, (int)(ld16 / 2), d / 2, 30, 1ll << 30};
    EpiIvfPrefilterT<EL, BO> epi{spos + r0, len, pair_q + g0, g, keys, pool_ld, pos_offset, tau, ld_tau, tau_lo, fill,
                                 xs + r0 * ld, ld, Q, ldq, d, el.at(r0), bo.at(r0)};
    const long long p0 = (y - qt_prefix[l]) * S::BP;
    for (long long row0 = (long long)blockIdx.x * S::BQ; row0 < len; row0 += (long long)gridDim.x * S::BQ)
        gemm_block<S>(lp, lq, epi, ksteps, p0, row0, smem);
}

// Coarse quantizer as a dense key table (round 3): scores of every query against every centroid -> keys[nq][ld] (64-bit
// (score, ~centroid), the pool format of ivf_select).  The probes used to come from the general exact search
// (amdrec_flat_search over the centroid table): with nlist <= 8192 rows that path files EVERY row as a candidate through
// atomics and sorts 4096 keys per query - 0.27 ms of a 4.6 ms step at nlist 4096 / 512 queries.  Same mainloop, same
// operand roles (lane <-> query, registers <-> centroids) as that search's filter pass, so the scores - and with
// ivf_select's order rule (score desc, position asc) the probes - are bit-identical to it.
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
struct EpiCoarseKeys {
    static constexpr const char* name = "ivf_coarse";
    static constexpr double out_bytes_per_elem = 2.0;
    static constexpr size_t lds_bytes(int) { return 0; }
    unsigned long long* keys;   // [nq][ld]
    long long ld;
    int nq;
    long long nlist;
    template <class A>
    __device__ void operator()(A& acc, float*) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const int q = acc.q(j, lane);
            if (q >= nq) continue;
            unsigned long long* dst = keys + (long long)q * ld;
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const long long p = acc.p(i, 4 * g, lane);     // 4 consecutive centroids p .. p+3
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {
                        if (p + e >= nlist) continue;
                        u64x2 kk;
                        kk[0] = make_key(rank_last(acc.v[i][j][4 * g + e]), (uint32_t)(p + e));
                        kk[1] = make_key(rank_last(acc.v[i][j][4 * g + e + 1]), (uint32_t)(p + e + 1));   // p+e+1 == nlist (odd nlist): lands in the ld padding
                        *reinterpret_cast<u64x2*>(dst + p + e) = kk;
                    }
                }
        }
    }
};

// ---- aware probes: the coarse step that sees the request's masks and boost weight (amdrec/probes.py has the rule) ------------
// Per list l the index keeps a SUMMARY of its rows next to list_tags / list_boosts: tag_or[l] = OR of the rows' tag words,
// boost_hi[l] / boost_lo[l] = max / min of the rows' boosts.  The coarse GEMM's epilogue then files, where EpiCoarseKeys files
// make_key(rank_last(c), l):  0 (the empty slot ivf_select skips) when no row of l can pass the query's masks or l is empty,
// else make_key(rank_last(c + w_q * b), l) with b = boost_hi[l] (w_q >= 0) or boost_lo[l] (w_q < 0): an upper bound of the
// boosted key of any row at the centroid's similarity.  The two predicates are types, as in the scans: four epilogues.
struct CoarseNoElig {
    static constexpr bool on = false;
    struct Mask {};
    struct Or2 {};
    __device__ __forceinline__ Mask mask(long long) const { return {}; }
    __device__ __forceinline__ Or2 load2(long long, bool) const { return {}; }
    static __device__ __forceinline__ bool ok(Or2, int, Mask) { return true; }
};
struct CoarseElig {
    static constexpr bool on = true;
    const unsigned long long* tag_or;   // [nlist]
    const uint64_t* all;                // [nq]
    const uint64_t* any;                // [nq]
    struct Mask { unsigned long long all, any; };
    using Or2 = u64x2;
    __device__ __forceinline__ Mask mask(long long q) const { return {all[q], any[q]}; }
    // the words of lists p, p+1 (p even): one 16-byte load; `both` false: p is the table's last list, p+1 is not read
    __device__ __forceinline__ Or2 load2(long long p, bool both) const {
        if (both) return *reinterpret_cast<const u64x2*>(tag_or + p);
        Or2 o;
        o[0] = tag_or[p], o[1] = 0ull;
        return o;
    }
    static __device__ __forceinline__ bool ok(Or2 o, int h, Mask m) {
        return (o[h] & m.all) == m.all && (m.any == 0ull || (o[h] & m.any) != 0ull);
    }
};
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct CoarseNoBoost {
    static constexpr bool on = false;
    struct Weight {};
    struct B2 {};
    __device__ __forceinline__ Weight w(long long) const { return {}; }
    __device__ __forceinline__ B2 load2(long long, bool, Weight) const { return {}; }
    static __device__ __forceinline__ float apply(float c, Weight, B2, int) { return c; }
};
struct CoarseBoost {
    static constexpr bool on = true;
    const float* hi;        // [nlist]
    const float* lo;        // [nlist]
    const float* weight;    // [nq]
    using Weight = float;
    using B2 = f32x2;
    __device__ __forceinline__ Weight w(long long q) const { return weight[q]; }
    // the bound of lists p, p+1 for this query's sign: ONE 8-byte load (hi or lo, never both)
    __device__ __forceinline__ B2 load2(long long p, bool both, Weight wq) const {
        const float* src = wq >= 0.f ? hi : lo;
        if (both) return *reinterpret_cast<const f32x2*>(src + p);
        B2 o;
        o[0] = src[p], o[1] = 0.f;
        return o;
    }
    static __device__ __forceinline__ float apply(float c, Weight wq, B2 o, int h) { return boost_add(c, boost_term(wq, o[h])); }
};

// The summaries are read per PAIR of lists, where the pair's two keys are made and stored (16-byte loads of len and tag_or,
// 8 bytes of the boost bound; nlist * 24 bytes in all: L2-resident): a group of four at a time keeps eight more registers
// live across the pair loop and the 256 x 128 tile, at its 244-VGPR budget, spills.
typedef long long i64x2 __attribute__((ext_vector_type(2)));
template <class EL, class BO>
struct EpiCoarseKeysAwareT {
    static constexpr const char* name = "ivf_coarse_aware";
    static constexpr double out_bytes_per_elem = 2.0;
    static constexpr size_t lds_bytes(int) { return 0; }
    unsigned long long* keys;   // [nq][ld]
    long long ld;
    int nq;
    long long nlist;
    const long long* len;       // [nlist] rows per list
    EL el;
    BO bo;
    // (forced: left to the inliner's budget, the masked + boosted form on the 256 x 128 tile became a call whose
    // accumulator argument - 128 registers - went through scratch)
    template <class A>
    __device__ __forceinline__ void operator()(A& acc, float*) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            const int q = acc.q(j, lane);
            if (q >= nq) continue;
            unsigned long long* dst = keys + (long long)q * ld;
            const typename EL::Mask m = el.mask(q);
            const typename BO::Weight wq = bo.w(q);
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const long long p = acc.p(i, 4 * g, lane);     // 4 consecutive lists p .. p+3, p % 4 == 0
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {
                        const long long l = p + e;
                        if (l >= nlist) continue;
                        const bool both = l + 1 < nlist;           // false: l + 1 == nlist (odd nlist), the ld padding: nothing is read there
                        i64x2 n2;
                        if (both) n2 = *reinterpret_cast<const i64x2*>(len + l);
                        else n2[0] = len[l], n2[1] = 0;            // ... and its key is written as 0
                        const typename EL::Or2 t2 = el.load2(l, both);
                        const typename BO::B2 b2 = bo.load2(l, both, wq);
                        u64x2 kk;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const bool feasible = n2[h] > 0 && EL::ok(t2, h, m);
                            const float s = BO::apply(acc.v[i][j][4 * g + e + h], wq, b2, h);
                            kk[h] = feasible ? make_key(rank_last(s), (uint32_t)(l + h)) : 0ull;
                        }
                        *reinterpret_cast<u64x2*>(dst + l) = kk;
                    }
                }
        }
    }
};

// Per-list summaries for the aware coarse step: one wave per list (grid-stride over lists), the lanes stride the list's
// contiguous rows (coalesced), a butterfly reduces.  OR / max / min do not depend on the order: exact, no atomics.  An empty
// list writes 0 / 0.0 / 0.0 (it is never feasible: the epilogue tests its length).
__global__ __launch_bounds__(256) void ivf_list_summaries_kernel(const long long* off, int nlist, const unsigned long long* tags,
                                                                 const float* boosts, unsigned long long* tag_or,
                                                                 float* boost_hi, float* boost_lo) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long l = wave; l < nlist; l += nwaves) {                  // wave-uniform
        const long long r0 = off[l], r1 = off[l + 1];
        unsigned long long t = 0ull;
        float hi = -INFINITY, lo = INFINITY;
        for (long long r = r0 + lane; r < r1; r += 64) {
            if (tags) t |= tags[r];
            if (boosts) {
                const float b = boosts[r];
                hi = fmaxf(hi, b);
                lo = fminf(lo, b);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            t |= __shfl_xor(t, o, 64);
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
            lo = fminf(lo, __shfl_xor(lo, o, 64));
        }
        if (lane == 0) {
            const bool none = r1 <= r0;
            if (tags) tag_or[l] = t;
            if (boosts) {
                boost_hi[l] = none ? 0.f : hi;
                boost_lo[l] = none ? 0.f : lo;
            }
        }
    }
}

// The grouped scans' tiles; BF16: the bf16-prefilter form of the same tile (K-step = 64 bf16)
template <bool BF16> using ShapeIvf = Shape<2, 2, 1, 4, false, BF16>;     // 64 queries x 256 list rows per workgroup
// 32 queries x 256 list rows: for sparse groups (few probing queries per list: 512 x 64 probes over 4096 lists is 8 per list,
// a 64-query tile would be 12 % full)
template <bool BF16> using ShapeIvf32 = Shape<1, 4, 1, 2, false, BF16>;
// SHORT lists (round 4): a rank of an 8-way sharded 10M index holds ~305 rows of each of the 4096 lists - two 256-row tiles
// of which the second is 19 % full (68 % of the MFMAs multiply padding); 128-row tiles pad the same list to 384 rows.
template <bool BF16> using ShapeIvfS = Shape<2, 2, 1, 2, false, BF16>;    // 64 queries x 128 list rows
template <bool BF16> using ShapeIvf32S = Shape<1, 4, 1, 1, false, BF16>;  // 32 queries x 128 list rows
// (double-buffered staging - one barrier per K-step - measured at the per-rank shape: 0.817 against 0.799 ms, not kept)

template <class S, class EL = ListNoElig, class BO = ListNoBoost, class... EP>
__global__ __launch_bounds__(S::NT, 2) void ivf_group_scan_kernel(
    const float* xs, long long ld, int d, int ksteps, const long long* spos, const long long* list_off,
    const float* Q, long long ldq, const long long* goff, const long long* qt_prefix, int nlist,
    const long long* pair_q, const long long* pair_p, const long long* base, int nprobe, unsigned long long* keys,
    long long pool_ld, long long pos_offset, const float* tau, long long ld_tau, unsigned long long* fill, EP... tail) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ListPreds<EL, BO> preds = list_preds(tail...);
    const EL el = preds.el;
    const BO bo = preds.bo;
    const long long y = blockIdx.y;
    if (y >= qt_prefix[nlist]) return;
    const int l = tile_list(y, qt_prefix, nlist);
    const long long r0 = list_off[l], len = list_off[l + 1] - r0;
    if ((long long)blockIdx.x * S::BQ >= len) return;
    const long long g0 = goff[l], g = goff[l + 1] - g0;
    GatherRows lp{Q, pair_q + g0, g, (int)ldq, d};
    DenseRows lq{xs + r0 * ld, len, (int)ld, d, 30, 1ll << 30};
    EpiIvfKeysT<EL, BO> epi{spos + r0, len, pair_q + g0, pair_p + g0, g, base, nprobe, keys, pool_ld, pos_offset, tau, ld_tau, fill,
                            el.at(r0), bo.at(r0)};
    const long long p0 = (y - qt_prefix[l]) * S::BP;
    // gridDim.x workgroups share the list's row tiles (round 4: the host no longer launches one workgroup per row tile of
    // the LONGEST list - on short lists three of four workgroups found no rows after paying for the tile search)
    for (long long row0 = (long long)blockIdx.x * S::BQ; row0 < len; row0 += (long long)gridDim.x * S::BQ)
        gemm_block<S>(lp, lq, epi, ksteps, p0, row0, smem);     // (ends behind a barrier: the staging area is free)
}

// k largest of keys[q][0..n_q) -> sorted (score desc, position asc); fewer than k -> padded (-inf, -1).
// The k-th largest SCORE is found by a 3-pass radix select over the keys' high words (11 + 11 + 10 bits); every key at or
// above it is then gathered (the keys above it plus its ties) and the sort of the full 64-bit keys settles the
// ties by position.  Four reads of the pool instead of the seven of a select over the whole 64-bit key; only when the
// boundary score has so many ties that the gather would not fit (k + ties > 2048) does the kernel fall back to that
// 6-pass select of the exact k-th key.
// the k best (by 64-bit key, descending) of row[0 .. n): returns them sorted (in `buf` or in `other`, 2048 keys each),
// have = min(n, k) valid entries first (keys of value 0 = empty slots rank last and are reported invalid by write_result).
// All 512 threads call.
__device__ __forceinline__ const unsigned long long* select_sorted_keys(const unsigned long long* row, long long n, int k,
                                                                        int* hist, int* scratch, unsigned long long* buf,
                                                                        unsigned long long* other, int* count, int& have) {
    const int tid = threadIdx.x;
    // A key of value 0 is an EMPTY slot, never a row (make_key of a NaN-free score is non-zero): the split select's partial
    // lists are zero-padded, so a pool may hold S * k > k entries of which fewer than k are rows.  Empty slots are skipped
    // by the histograms and by the gather (kstar >= 1); when fewer than k rows exist everything non-empty is gathered.
    // (Round 3 counted the padding: the k-th largest of 300 rows + 7700 zeros was 0, the gather admitted all 8000 entries
    // and kept an arbitrary 2048 of them - ADVICE r3.)
    unsigned long long kstar = 1ull;          // gather every row by default (n <= k, or fewer than k non-empty keys)
    if (n > k) {
        // every key at or above the k-th largest score's (partial) prefix: the select stops once those fit the sort buffer.
        // Typical pools stop after the FIRST pass: two walks over the pool instead of four (the select of a large pool is
        // bound by those walks: 512 queries x 100 000 keys, 0.46 ms).
        const uint32_t prefix = select_prefix_desc<512, 3, 2048>(hist, scratch, k, [&](auto count_key) {
            for (long long i = tid; i < n; i += 512) count_key(row[i]);
        });
        kstar = prefix == 0u ? 1ull : (unsigned long long)prefix << 32;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (tid == 0) *count = 0;
        for (int i = tid; i < 2048; i += 512) buf[i] = 0ull;
        __syncthreads();
        for (long long i = tid; i < n; i += 512) {
            const unsigned long long key = row[i];
            if (key >= kstar) {
                const int pos = atomicAdd(count, 1);
                if (pos < 2048) buf[pos] = key;
            }
        }
        __syncthreads();
        if (*count <= 2048 || attempt == 1) break;        // block-uniform
        // too many ties at the boundary score: the exact k-th KEY by a 6-pass select over all 64 bits, then exactly k pass
        unsigned long long prefix = 0ull, pmask = 0ull;
        int rr = k;
        const int shifts[6] = {53, 42, 31, 20, 9, 0};
        const int bits[6] = {11, 11, 11, 11, 11, 9};
        for (int pass = 0; pass < 6; ++pass) {
            __syncthreads();
            for (int i = tid; i < 2048; i += 512) hist[i] = 0;
            __syncthreads();
            const unsigned long long bm = (1ull << bits[pass]) - 1;
            for (long long i = tid; i < n; i += 512) {
                const unsigned long long key = row[i];
                if (key != 0ull && (key & pmask) == prefix) atomicAdd(&hist[(int)((key >> shifts[pass]) & bm)], 1);
            }
            __syncthreads();
            const int bin = find_bin_desc<2048, 512>(hist, rr, scratch);
            prefix |= (unsigned long long)bin << shifts[pass];
            pmask |= bm << shifts[pass];
        }
        kstar = prefix ? prefix : 1ull;           // (more than 2048 non-empty keys were gathered: the k-th exists)
        __syncthreads();
    }
    const int have_all = *count < 2048 ? *count : 2048;
    have = have_all < k ? have_all : k;
    // the network up to 512 keys, the runs beyond (A/B of the two forms: profiles/r04_ivf_sort_ab.log)
    return sort_keys_desc<512>(buf, other, have_all, 512);
}

__global__ __launch_bounds__(512) void ivf_select_kernel(const unsigned long long* keys, long long pool_ld,
                                                         const long long* n_pool, int k, float* outD,
                                                         long long* outI) {
    __shared__ int hist[2048];
    __shared__ int scratch[514];
    __shared__ __attribute__((aligned(16))) unsigned long long buf[2048];
    __shared__ __attribute__((aligned(16))) unsigned long long other[2048];
    __shared__ int count;
    const long long q = blockIdx.x;
    int have;
    const unsigned long long* sorted = select_sorted_keys(keys + q * pool_ld, n_pool[q], k, hist, scratch, buf, other, &count, have);
    write_result(sorted, have, k, q, outD, outI, 0);
}

// Few queries with LARGE pools (one request against nlist 100 / nprobe 10 at 1M ads: 100 000 keys, one workgroup walking
// them four times: 0.14 ms): gridDim.x workgroups per query each select the k best of a slice of the pool into
// part[q][slice][k]; the workgroup that draws the query's last ticket selects the k best of those and writes the result.
// The k best of the pool are among the k best of the slices, and the order is the key order either way: the same result
// as ivf_select_kernel.  The ticket returns to 0.
__global__ __launch_bounds__(512) void ivf_select_split_kernel(const unsigned long long* keys, long long pool_ld,
                                                               const long long* n_pool, int k, unsigned long long* part,
                                                               int* tickets, float* outD, long long* outI) {
    __shared__ int hist[2048];
    __shared__ int scratch[514];
    __shared__ __attribute__((aligned(16))) unsigned long long buf[2048];
    __shared__ __attribute__((aligned(16))) unsigned long long other[2048];
    __shared__ int count;
    const long long q = blockIdx.y;
    const int s = blockIdx.x, S = gridDim.x, tid = threadIdx.x;
    const long long n = n_pool[q];
    const long long per = (n + S - 1) / S;
    const long long lo = s * per < n ? s * per : n, hi = lo + per < n ? lo + per : n;
    int have;
    const unsigned long long* sorted = select_sorted_keys(keys + q * pool_ld + lo, hi - lo, k, hist, scratch, buf, other, &count, have);
    unsigned long long* mine = part + (q * S + s) * k;
    for (int i = tid; i < k; i += 512) mine[i] = i < have ? sorted[i] : 0ull;
    if (!last_workgroup(&tickets[q], S, true)) return;
    sorted = select_sorted_keys(part + q * S * k, (long long)S * k, k, hist, scratch, buf, other, &count, have);
    write_result(sorted, have, k, q, outD, outI, 0);
}

// ---- index BUILD: max-inner-product assignment and Lloyd iterations (faiss_retrieval.py:83-95, :118: IndexIVFFlat with an
// IndexFlatIP quantizer trains k-means on first add and files every vector under the centroid of largest inner product) ----
// Assignment = the GEMM mainloop (P = centroids: registers, Q = rows: lanes, fp32 MFMA: exact fma chains, so a row's
// scores do not depend on tiling) with an arg-max epilogue: per row the best (score, centroid) key of the block's 256
// centroids, folded across the centroid tiles with one 64-bit atomicMax per (wave, row).  key = (orderable score << 32) |
// ~centroid: larger = better, equal scores -> LOWER centroid index (deterministic; NaN scores never win).
struct EpiArgmax {
    static constexpr const char* name = "ivf_assign";
    static constexpr double out_bytes_per_elem = 0.0;
    static constexpr size_t lds_bytes(int) { return 0; }
    unsigned long long* keys;   // [rows], zero-initialised
    long long rows;
    int nlist;
    template <class A>
    __device__ void operator()(A& acc, float*) const {
        constexpr int TP = A::TP, TQ = A::TQ;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
            unsigned long long best = 0ull;
#pragma unroll
            for (int i = 0; i < TP; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = acc.p(i, r, lane);
                    const float sc = acc.v[i][j][r];
                    if (p < nlist && sc == sc) {
                        const unsigned long long key = make_key(sc, (uint32_t)p);
                        best = key > best ? key : best;
                    }
                }
            const unsigned long long other = ((unsigned long long)__shfl_xor((unsigned)(best >> 32), 32, 64) << 32) |
                                             (unsigned long long)__shfl_xor((unsigned)best, 32, 64);
            best = other > best ? other : best;
            const long long q = acc.q(j, lane);
            if (lane < 32 && q < rows && best != 0ull) atomicMax(&keys[q], best);
        }
    }
};

__global__ void ivf_decode_assign_kernel(const unsigned long long* keys, long long rows, long long* assign, float* score) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const unsigned long long k = keys[i];
    assign[i] = k ? (long long)key_pos(k) : 0ll;          // a row whose scores are all NaN goes to list 0
    if (score) score[i] = k ? key_score(k) : -INFINITY;
}

// Centroid update, DETERMINISTIC: every coordinate is accumulated as a 64-bit fixed-point integer (x * 2^40, exact for
// fp32 unit-vector coordinates down to 2^-16; integer addition is associative, so the sum does not depend on the order
// the atomics land in - float atomics would make the trained centroids, and with them every IVF result, vary run to run).
constexpr float IVF_FIX = 1099511627776.0f;      // 2^40; up to 2^22 unit rows per centroid before 2^62
__global__ __launch_bounds__(256) void ivf_accumulate_kernel(const float* x, long long rows, long long ld, int d,
                                                             const long long* assign, long long* sums, int* counts) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const long long a = assign[r];
    for (int c = lane; c < d; c += 64) {
        const float v = x[r * ld + c];
        if (v == v) atomicAdd(reinterpret_cast<unsigned long long*>(&sums[a * d + c]), (unsigned long long)__float2ll_rn(v * IVF_FIX));
    }
    if (lane == 0) atomicAdd(&counts[a], 1);
}
// new centroid = sum / |sum| (spherical k-means: the quantizer compares inner products); empty clusters keep the old one
__global__ __launch_bounds__(256) void ivf_finish_centroids_kernel(const long long* sums, const int* counts, int nlist, int d,
                                                                   float* cent, long long ldc) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= nlist || counts[c] == 0) return;
    double ss = 0.0;
    for (int k = lane; k < d; k += 64) {
        const double v = (double)sums[(long long)c * d + k];
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (!(ss > 0.0)) return;
    const double inv = 1.0 / sqrt(ss);
    for (int k = lane; k < d; k += 64) cent[c * ldc + k] = (float)((double)sums[(long long)c * d + k] * inv);
}

// ---- query-time plumbing, sync-free (replaces torch argsort / bincount / cumsum per search call) ---------------------
// pool layout of every query + rank of every (query, probe) pair inside its list's group (counting sort, pass 1)
__global__ void ivf_group_count_kernel(const long long* probes, long long ldp, int nprobe, long long npairs, int nlist, int* cnt,
                                       int* rank) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const long long l = probes[(i / nprobe) * ldp + i % nprobe];
    rank[i] = atomicAdd(&cnt[(l < 0 || l >= nlist) ? nlist : (int)l], 1);
}
__global__ void ivf_pool_layout_kernel(const long long* probes, long long ldp, long long m, int nprobe, int nlist,
                                       const long long* list_len, long long* base, long long* n_pool) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    long long run = 0;
    for (int p = 0; p < nprobe; ++p) {
        const long long l = probes[q * ldp + p];
        base[q * nprobe + p] = run;
        run += (l >= 0 && l < nlist) ? list_len[l] : 0;
    }
    n_pool[q] = run;
}
// exclusive scans over the lists: group offsets and query-tile offsets (tiles of qtile queries; one block)
__global__ __launch_bounds__(1024) void ivf_group_prefix_kernel(const int* cnt, int nlist, int qtile, long long* goff,
                                                                 long long* qtp) {
    __shared__ long long sa[1024], sb[1024];
    const int tid = threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    const int lo = tid * per, hi = (lo + per < nlist) ? lo + per : nlist;
    long long a = 0, b = 0;
    for (int l = lo; l < hi; ++l) { a += cnt[l]; b += (cnt[l] + qtile - 1) / qtile; }
    sa[tid] = a; sb[tid] = b;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                  // Hillis-Steele inclusive scan of the 1024 partials
        const long long va = tid >= o ? sa[tid - o] : 0, vb = tid >= o ? sb[tid - o] : 0;
        __syncthreads();
        sa[tid] += va; sb[tid] += vb;
        __syncthreads();
    }
    long long ra = sa[tid] - a, rb = sb[tid] - b;         // exclusive prefix of this thread's range
    for (int l = lo; l < hi; ++l) {
        goff[l] = ra; qtp[l] = rb;
        ra += cnt[l]; rb += (cnt[l] + qtile - 1) / qtile;
    }
    if (tid == 1023) { goff[nlist] = sa[1023]; qtp[nlist] = sb[1023]; }
}
__global__ void ivf_group_scatter_kernel(const long long* probes, long long ldp, long long npairs, int nprobe, int nlist,
                                         const int* rank, const long long* goff, long long* pair_q, long long* pair_p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const long long l = probes[(i / nprobe) * ldp + i % nprobe];
    if (l < 0 || l >= nlist) return;
    const long long pos = goff[l] + rank[i];
    pair_q[pos] = i / nprobe;
    pair_p[pos] = i % nprobe;
}

}  // namespace amdrec

using namespace amdrec;

static int assign_impl(const float* x, long long rows, long long ld, int dim, const float* cent, int nlist, long long ldc,
                       long long* assign, float* score, unsigned long long* keys, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(keys, 0, (size_t)rows * 8, st));
    DenseRows lp{cent, nlist, (int)ldc, dim, 30, 1ll << 30};
    DenseRows lq{x, rows, (int)ld, dim, 30, 1ll << 30};
    EpiArgmax epi{keys, rows, nlist};
    HIP_TRY((launch_gemm<Shape<2, 2, 4, 2>, true>(lp, lq, epi, dim, nlist, rows, st)));
    hipLaunchKernelGGL(ivf_decode_assign_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, keys, rows, assign, score);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

static int assign_check(const float* x, int64_t rows, int64_t ld, int dim, const float* cent, int nlist, int64_t ldc) {
    REQUIRE(dim >= 4 && dim % 4 == 0 && dim <= 2048, "dim=%d must be a multiple of 4 in [4,2048]", dim);
    REQUIRE(nlist >= 1 && nlist <= (1 << 20), "nlist out of range");
    REQUIRE(rows >= 0 && rows < (1ll << 31) - 1024, "rows out of range");
    REQUIRE(ld >= dim && ld % 4 == 0 && ldc >= dim && ldc % 4 == 0 && ld < (1ll << 31) && ldc < (1ll << 31), "bad leading dimension");
    REQUIRE(rows == 0 || (x && cent), "null pointer");
    REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)cent % 16) == 0, "x / centroids must be 16-byte aligned");
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_assign(const float* x, int64_t rows, int64_t ld, int dim, const float* centroids, int nlist,
                                 int64_t ld_centroids, int64_t* assign, float* best_score, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    int rc = assign_check(x, rows, ld, dim, centroids, nlist, ld_centroids);
    if (rc) return rc;
    if (rows == 0) return AMDREC_OK;
    REQUIRE(assign != nullptr, "assign is null");
    if ((rc = require_workspace(workspace, workspace_bytes, align_up((size_t)rows * 8, 256)))) return rc;
    return assign_impl(x, rows, ld, dim, centroids, nlist, ld_centroids, (long long*)assign, best_score,
                       static_cast<unsigned long long*>(workspace), reinterpret_cast<hipStream_t>(stream));
}

// k-means step: xkeys | assign | sums | counts, the last two cleared together
struct KmeansWs : Carver {
    unsigned long long* keys; long long *assign, *sums; int* counts;
    size_t clear_bytes;
    KmeansWs(int64_t rows, int dim, int nlist, void* ws) : Carver(ws) {
        keys = take<unsigned long long>(rows);
        assign = take<long long>(rows);
        const size_t m = bytes();
        sums = take<long long>((size_t)nlist * dim);
        counts = take<int>(nlist);
        clear_bytes = bytes_since(m);
    }
};

extern "C" int amdrec_ivf_kmeans_workspace(int64_t rows, int dim, int nlist, size_t* bytes) {
    REQUIRE(bytes != nullptr && rows >= 0 && dim >= 4 && nlist >= 1, "bad arguments");
    *bytes = KmeansWs(rows, dim, nlist, nullptr).bytes();
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_kmeans_step(const float* x, int64_t rows, int64_t ld, int dim, float* centroids, int nlist,
                                      int64_t ld_centroids, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = assign_check(x, rows, ld, dim, centroids, nlist, ld_centroids);
    if (rc) return rc;
    if (rows == 0) return AMDREC_OK;
    const KmeansWs w(rows, dim, nlist, workspace);
    if ((rc = require_workspace(workspace, workspace_bytes, w.bytes()))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    rc = assign_impl(x, rows, ld, dim, centroids, nlist, ld_centroids, w.assign, nullptr, w.keys, st);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(w.sums, 0, w.clear_bytes, st));
    hipLaunchKernelGGL(ivf_accumulate_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, (long long)rows,
                       (long long)ld, dim, w.assign, w.sums, w.counts);
    hipLaunchKernelGGL(ivf_finish_centroids_kernel, dim3((unsigned)((nlist + 3) / 4)), dim3(256), 0, st, w.sums, w.counts, nlist,
                       dim, centroids, (long long)ld_centroids);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_group(const int64_t* probes, int64_t ld_probes, int64_t nq, int nprobe, int nlist, const int64_t* list_len,
                                int64_t* pool_base, int64_t* pool_count, int64_t* pair_query, int64_t* pair_probe,
                                int64_t* group_off, int64_t* qtile_prefix, int qtile, void* workspace,
                                size_t workspace_bytes, void* stream) {
    REQUIRE(nprobe >= 1 && nlist >= 1 && nlist <= (1 << 20), "bad nlist/nprobe");
    REQUIRE(qtile == 32 || qtile == 64, "qtile must be 32 or 64");
    REQUIRE(ld_probes >= nprobe, "ld_probes < nprobe");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq * (int64_t)nprobe < (1ll << 31), "too many (query, probe) pairs for one call");
    REQUIRE(probes && list_len && pool_base && pool_count && pair_query && pair_probe && group_off && qtile_prefix, "null pointer");
    const long long npairs = nq * nprobe;
    Carver c(workspace);
    int *cnt = c.take<int>((size_t)nlist + 1), *rank = c.take<int>(npairs);
    if (int rc = require_workspace(workspace, workspace_bytes, c.bytes())) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)(nlist + 1) * 4, st));
    hipLaunchKernelGGL(ivf_group_count_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st,
                       (const long long*)probes, (long long)ld_probes, nprobe, npairs, nlist, cnt, rank);
    hipLaunchKernelGGL(ivf_pool_layout_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, (const long long*)probes,
                       (long long)ld_probes, (long long)nq, nprobe, nlist, (const long long*)list_len, (long long*)pool_base,
                       (long long*)pool_count);
    hipLaunchKernelGGL(ivf_group_prefix_kernel, dim3(1), dim3(1024), 0, st, cnt, nlist, qtile, (long long*)group_off,
                       (long long*)qtile_prefix);
    hipLaunchKernelGGL(ivf_group_scatter_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st,
                       (const long long*)probes, (long long)ld_probes, npairs, nprobe, nlist, rank, (const long long*)group_off,
                       (long long*)pair_query, (long long*)pair_probe);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

// ---- the eligibility pointers of the *_eligible scans ----
// All three are required and 8-byte aligned, checked with the other arguments before the first HIP call.  A scan entry
// and its *_eligible twin are ONE host template over the predicate: ListNoElig checks and passes nothing.
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
// ---- the boost pointers of the *_boosted scans ----
// Both required and 4-byte aligned, checked with the other arguments before the first HIP call.  A scan entry and its
// *_boosted / *_eligible_boosted twins are the same host template: ListNoBoost checks and passes nothing.
static int boost_check(ListNoBoost) { return AMDREC_OK; }
static int boost_check(ListBoost bo) {
    REQUIRE(bo.boosts != nullptr, "list_boosts is null");
    REQUIRE(bo.weight != nullptr, "weight is null");
    REQUIRE(((uintptr_t)bo.boosts % 4) == 0, "list_boosts must be 4-byte aligned");
    REQUIRE(((uintptr_t)bo.weight % 4) == 0, "weight must be 4-byte aligned");
    return AMDREC_OK;
}
static int boost_max_check(float boost_max) {
    REQUIRE(boost_max >= 0.f && boost_max < INFINITY, "boost_max must be a finite bound of max |boost|");
    return AMDREC_OK;
}
// the kernel instantiation of (EL, BO) inside a host template over them: K<prefix..., EL, BO, EL's three pointers (ListElig),
// BO's two (ListBoost)>; the plain one is K<prefix...>.  The prefix ends in its comma (or is empty).
#define AMDREC_LIST_ELIG_PTRS const uint64_t*, const uint64_t*, const uint64_t*
#define AMDREC_LIST_BOOST_PTRS const float*, const float*
#define AMDREC_LIST_KERNEL(K, ...) [] { \
    if constexpr (EL::on && BO::on) return K<__VA_ARGS__ ListElig, ListBoost, AMDREC_LIST_ELIG_PTRS, AMDREC_LIST_BOOST_PTRS>; \
    else if constexpr (EL::on) return K<__VA_ARGS__ ListElig, ListNoBoost, AMDREC_LIST_ELIG_PTRS>; \
    else if constexpr (BO::on) return K<__VA_ARGS__ ListNoElig, ListBoost, AMDREC_LIST_BOOST_PTRS>; \
    else return K<__VA_ARGS__ ListNoElig, ListNoBoost>; }()
// launches `kern` with the eligibility pointers, then the boost pointers, after the arguments every instantiation takes
static std::tuple<> list_tail(ListNoElig) { return {}; }
static std::tuple<const uint64_t*, const uint64_t*, const uint64_t*> list_tail(ListElig el) { return {el.tags, el.all, el.any}; }
static std::tuple<> list_tail(ListNoBoost) { return {}; }
static std::tuple<const float*, const float*> list_tail(ListBoost bo) { return {bo.boosts, bo.weight}; }
template <class EL, class BO, class Kern, class... Args>
static void launch_with(EL el, BO bo, Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    std::apply([&](auto... tail) { hipLaunchKernelGGL(kern, grid, block, lds, st, args..., tail...); },
               std::tuple_cat(list_tail(el), list_tail(bo)));
}
// the ProfScope tag of a scan: base, base_elig, base_boost or base_elig_boost
#define AMDREC_LIST_TAG(base) \
    (BO::on ? (EL::on ? base "_elig_boost" : base "_boost") : (EL::on ? base "_elig" : base))

template <class EL, class BO = ListNoBoost>
static int ivf_scan_impl(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                         const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                         const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                         int64_t pool_ld, int64_t pos_offset, void* stream, EL el, BO bo = {}) {
    REQUIRE(dim >= 4 && dim % 4 == 0 && dim <= 2048, "dim=%d must be a multiple of 4 in [4,2048]", dim);
    REQUIRE(nprobe >= 1 && nprobe <= 65535, "nprobe out of range");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(nq <= 65535, "at most 65535 queries per call");
    REQUIRE(lists && row_pos && list_off && queries && probes && pool_base && pool_keys, "null pointer");
    REQUIRE(ld % 4 == 0 && ld >= dim && ld_queries >= dim, "bad leading dimension");
    if (int rc = elig_check(el)) return rc;
    if (int rc = boost_check(bo)) return rc;
    long long splits = 2048 / ((long long)nprobe * nq);            // ~2048 workgroups in all
    splits = splits < 1 ? 1 : (splits > 64 ? 64 : splits);
    ProfScope prof(AMDREC_LIST_TAG("ivf_scan_pairs"), 0.0, 0.0, reinterpret_cast<hipStream_t>(stream));
    auto kern = AMDREC_LIST_KERNEL(ivf_scan_kernel, );
    launch_with(el, bo, kern, dim3(nprobe, (unsigned)nq, (unsigned)splits), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                lists, (long long)ld, dim, (const long long*)row_pos, (const long long*)list_off, queries,
                (long long)ld_queries, (const long long*)probes, (const long long*)pool_base, nprobe,
                (unsigned long long*)pool_keys, (long long)pool_ld, (long long)pos_offset);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_scan(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                               const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                               const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                               int64_t pool_ld, int64_t pos_offset, void* stream) {
    return ivf_scan_impl(lists, ld, dim, row_pos, list_off, queries, nq, ld_queries, probes, pool_base, nprobe, pool_keys,
                         pool_ld, pos_offset, stream, ListNoElig{});
}

extern "C" int amdrec_ivf_scan_eligible(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                        const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                                        const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                                        int64_t pool_ld, int64_t pos_offset, void* stream, const uint64_t* list_tags,
                                        const uint64_t* require_all, const uint64_t* require_any) {
    return ivf_scan_impl(lists, ld, dim, row_pos, list_off, queries, nq, ld_queries, probes, pool_base, nprobe, pool_keys,
                         pool_ld, pos_offset, stream, ListElig{list_tags, require_all, require_any});
}

extern "C" int amdrec_ivf_scan_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                       const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                                       const int64_t* probes, const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                                       int64_t pool_ld, int64_t pos_offset, void* stream, const float* list_boosts,
                                       const float* weight) {
    return ivf_scan_impl(lists, ld, dim, row_pos, list_off, queries, nq, ld_queries, probes, pool_base, nprobe, pool_keys,
                         pool_ld, pos_offset, stream, ListNoElig{}, ListBoost{list_boosts, weight});
}

extern "C" int amdrec_ivf_scan_eligible_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                                const int64_t* list_off, const float* queries, int64_t nq, int64_t ld_queries,
                                                const int64_t* probes, const int64_t* pool_base, int nprobe,
                                                uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset, void* stream,
                                                const uint64_t* list_tags, const uint64_t* require_all,
                                                const uint64_t* require_any, const float* list_boosts, const float* weight) {
    return ivf_scan_impl(lists, ld, dim, row_pos, list_off, queries, nq, ld_queries, probes, pool_base, nprobe, pool_keys,
                         pool_ld, pos_offset, stream, ListElig{list_tags, require_all, require_any},
                         ListBoost{list_boosts, weight});
}

// Workgroup columns per (list, query tile): an eighth of the LONGEST list's row tiles, each looping over its share of the
// list's tiles.  Round 3 launched one workgroup per row tile of the longest list for every (list, query tile): list lengths
// spread 0 .. 4x the mean, so three of four workgroups found no rows - after paying for the tile search - and at the
// per-rank shape of an 8-way sharded 10M index (305-row lists) 48 000 of 61 000 workgroups were empty: scan 1.82 ->
// 0.80 ms (profiles/r04_shard_ivf_g8_after.log).
constexpr long long scan_columns(long long max_list_rows, int tile_rows) {
    return ((max_list_rows + tile_rows - 1) / tile_rows + 7) / 8;
}
static_assert(scan_columns(305, 128) == 1 && scan_columns(9767, 256) == 5, "the per-rank and the single-GPU shape of the 10M index");

// row tile: 128 rows when even the longest list is short (the tile count of a launch is sized by it), else 256
constexpr long long SHORT_LIST_ROWS = 1536;

// Both grouped kernels are launched here, so the two phases of one search cannot disagree about geometry; `args`: the
// kernel's arguments
template <class S, auto Kernel, class EL, class BO, class... Args>
static hipError_t launch_grouped(EL el, BO bo, const char* tag, long long max_list_rows, long long qtile_bound, hipStream_t st, Args... args) {
    static PerDeviceOnce attr_done;
    if (attr_done.pending()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)S::LDS_BYTES);
        if (e != hipSuccess) return e;
        attr_done.mark();
    }
    ProfScope prof(tag, 0.0, 0.0, st);
    launch_with(el, bo, Kernel, dim3((unsigned)scan_columns(max_list_rows, S::BQ), (unsigned)qtile_bound), dim3(S::NT),
                S::LDS_BYTES, st, args...);
    return hipGetLastError();
}

// f(shape, ProfScope tag) for the tile of (qtile, short_lists = the longest list has at most SHORT_LIST_ROWS rows)
// (the tags of the filtered instantiations end in _elig, of the boosted ones in _boost, of both in _elig_boost)
template <bool BF16, class EL, class BO, class F>
static hipError_t with_scan_shape(int qtile, bool short_lists, F&& f) {
#define AMDREC_SCAN_TAG(tile) \
    (BF16 ? AMDREC_LIST_TAG("ivf_scan_grouped_bf16_" tile) : AMDREC_LIST_TAG("ivf_scan_grouped_" tile))
    // fp32 scan with BOTH predicates: the 64 x 256 tile spills (255 VGPRs + 16 bytes of scratch; the filtered one alone sits
    // at 248), so long lists take the 64 x 128 tile too (220 VGPRs, no scratch) - twice the row tiles per list, same keys
    if (qtile == 64) {
        if constexpr (!BF16 && EL::on && BO::on)
            return f(ShapeIvfS<BF16>{}, AMDREC_SCAN_TAG("64x128"));
        else
            return short_lists ? f(ShapeIvfS<BF16>{}, AMDREC_SCAN_TAG("64x128")) : f(ShapeIvf<BF16>{}, AMDREC_SCAN_TAG("64x256"));
    }
    return short_lists ? f(ShapeIvf32S<BF16>{}, AMDREC_SCAN_TAG("32x128")) : f(ShapeIvf32<BF16>{}, AMDREC_SCAN_TAG("32x256"));
#undef AMDREC_SCAN_TAG
}

// The arguments the two grouped entries have in common and the refusals they share.  Each entry applies them in its own
// order with its own conditions in between; "null pointer" and "bad leading dimension" are one REQUIRE per entry (its own
// clauses and-ed to pointers() / leading_dims()), so which of them wins does not depend on the entry.
struct GroupedArgs {
    const float* lists; int64_t ld; int dim; const int64_t *row_pos, *list_off; int64_t max_list_rows;
    const float* queries; int64_t ld_queries; const int64_t *group_off, *qtile_prefix; int64_t qtile_bound; int qtile;
    const int64_t* pair_query; const uint64_t* pool_keys;
    int check_dim(int multiple) const {
        REQUIRE(dim >= multiple && dim % multiple == 0 && dim <= 2048, "dim=%d must be a multiple of %d in [%d,2048]", dim,
                multiple, multiple);
        return AMDREC_OK;
    }
    int check_qtile() const {
        REQUIRE(qtile == 32 || qtile == 64, "qtile must be 32 or 64 (the value given to amdrec_ivf_group)");
        return AMDREC_OK;
    }
    bool empty() const { return qtile_bound <= 0 || max_list_rows <= 0; }        // nothing to scan: AMDREC_OK
    int check_bound() const {
        REQUIRE(qtile_bound <= 65535, "too many (list, query-tile) groups for one launch: chunk the queries");
        return AMDREC_OK;
    }
    bool pointers() const { return lists && row_pos && list_off && queries && group_off && qtile_prefix && pair_query && pool_keys; }
    bool leading_dims() const { return ld % 4 == 0 && ld >= dim && ld_queries >= dim && ld_queries % 4 == 0; }
};

template <class EL, class BO = ListNoBoost>
static int scan_grouped_impl(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                             const int64_t* list_off, int nlist, int64_t max_list_rows,
                             const float* queries, int64_t ld_queries, const int64_t* group_off,
                             const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                             const int64_t* pair_query, const int64_t* pair_probe, const int64_t* pool_base,
                             int nprobe, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
                             const float* tau, int64_t ld_tau, int64_t* pool_fill, void* stream, EL el, BO bo = {}) {
    const GroupedArgs a{lists, ld, dim, row_pos, list_off, max_list_rows, queries, ld_queries, group_off, qtile_prefix, qtile_bound,
                        qtile, pair_query, pool_keys};
    if (int rc = a.check_dim(4)) return rc;
    REQUIRE(nlist >= 1 && nprobe >= 1, "bad nlist/nprobe");
    if (int rc = a.check_qtile()) return rc;
    REQUIRE((tau == nullptr) == (pool_fill == nullptr) && (tau == nullptr || ld_tau >= 1), "tau and pool_fill go together");
    if (a.empty()) return AMDREC_OK;
    if (int rc = a.check_bound()) return rc;
    REQUIRE(a.pointers() && pair_probe && (pool_base || tau), "null pointer");
    REQUIRE(a.leading_dims(), "bad leading dimension");
    if (int rc = elig_check(el)) return rc;
    if (int rc = boost_check(bo)) return rc;
    const hipError_t e = with_scan_shape<false, EL, BO>(qtile, max_list_rows <= SHORT_LIST_ROWS, [&](auto shape, const char* tag) {
        using S = decltype(shape);
        constexpr auto kern = AMDREC_LIST_KERNEL(ivf_group_scan_kernel, S,);
        return launch_grouped<S, kern>(
            el, bo, tag, max_list_rows, qtile_bound, reinterpret_cast<hipStream_t>(stream), lists, ld, dim, (dim + BK - 1) / BK,
            (const long long*)row_pos, (const long long*)list_off, queries, ld_queries, (const long long*)group_off,
            (const long long*)qtile_prefix, nlist, (const long long*)pair_query, (const long long*)pair_probe,
            (const long long*)pool_base, nprobe, (unsigned long long*)pool_keys, pool_ld, pos_offset, tau, ld_tau,
            (unsigned long long*)pool_fill);
    });
    HIP_TRY(e);
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_scan_grouped(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                       const int64_t* list_off, int nlist, int64_t max_list_rows,
                                       const float* queries, int64_t ld_queries, const int64_t* group_off,
                                       const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                                       const int64_t* pair_query, const int64_t* pair_probe, const int64_t* pool_base,
                                       int nprobe, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
                                       const float* tau, int64_t ld_tau, int64_t* pool_fill, void* stream) {
    return scan_grouped_impl(lists, ld, dim, row_pos, list_off, nlist, max_list_rows, queries, ld_queries, group_off,
                             qtile_prefix, qtile_bound, qtile, pair_query, pair_probe, pool_base, nprobe, pool_keys, pool_ld,
                             pos_offset, tau, ld_tau, pool_fill, stream, ListNoElig{});
}

extern "C" int amdrec_ivf_scan_grouped_eligible(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                                const int64_t* list_off, int nlist, int64_t max_list_rows,
                                                const float* queries, int64_t ld_queries, const int64_t* group_off,
                                                const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                                                const int64_t* pair_query, const int64_t* pair_probe,
                                                const int64_t* pool_base, int nprobe, uint64_t* pool_keys, int64_t pool_ld,
                                                int64_t pos_offset, const float* tau, int64_t ld_tau, int64_t* pool_fill,
                                                void* stream, const uint64_t* list_tags, const uint64_t* require_all,
                                                const uint64_t* require_any) {
    return scan_grouped_impl(lists, ld, dim, row_pos, list_off, nlist, max_list_rows, queries, ld_queries, group_off,
                             qtile_prefix, qtile_bound, qtile, pair_query, pair_probe, pool_base, nprobe, pool_keys, pool_ld,
                             pos_offset, tau, ld_tau, pool_fill, stream, ListElig{list_tags, require_all, require_any});
}

extern "C" int amdrec_ivf_scan_grouped_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                               const int64_t* list_off, int nlist, int64_t max_list_rows,
                                               const float* queries, int64_t ld_queries, const int64_t* group_off,
                                               const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                                               const int64_t* pair_query, const int64_t* pair_probe, const int64_t* pool_base,
                                               int nprobe, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
                                               const float* tau, int64_t ld_tau, int64_t* pool_fill, void* stream,
                                               const float* list_boosts, const float* weight) {
    return scan_grouped_impl(lists, ld, dim, row_pos, list_off, nlist, max_list_rows, queries, ld_queries, group_off,
                             qtile_prefix, qtile_bound, qtile, pair_query, pair_probe, pool_base, nprobe, pool_keys, pool_ld,
                             pos_offset, tau, ld_tau, pool_fill, stream, ListNoElig{}, ListBoost{list_boosts, weight});
}

extern "C" int amdrec_ivf_scan_grouped_eligible_boosted(const float* lists, int64_t ld, int dim, const int64_t* row_pos,
                                                        const int64_t* list_off, int nlist, int64_t max_list_rows,
                                                        const float* queries, int64_t ld_queries, const int64_t* group_off,
                                                        const int64_t* qtile_prefix, int64_t qtile_bound, int qtile,
                                                        const int64_t* pair_query, const int64_t* pair_probe,
                                                        const int64_t* pool_base, int nprobe, uint64_t* pool_keys,
                                                        int64_t pool_ld, int64_t pos_offset, const float* tau, int64_t ld_tau,
                                                        int64_t* pool_fill, void* stream, const uint64_t* list_tags,
                                                        const uint64_t* require_all, const uint64_t* require_any,
                                                        const float* list_boosts, const float* weight) {
    return scan_grouped_impl(lists, ld, dim, row_pos, list_off, nlist, max_list_rows, queries, ld_queries, group_off,
                             qtile_prefix, qtile_bound, qtile, pair_query, pair_probe, pool_base, nprobe, pool_keys, pool_ld,
                             pos_offset, tau, ld_tau, pool_fill, stream, ListElig{list_tags, require_all, require_any},
                             ListBoost{list_boosts, weight});
}

// BP: nothing, or (weight [nq], boost_max) of the boosted bound
template <class... BP>
static int filter_bounds_impl(const char* tag, const float* queries, int64_t nq, int64_t ld_queries, int dim,
                              const uint16_t* queries_bf16, int64_t ld_queries_bf16, const float* max_norm,
                              const float* tau, int64_t ld_tau, float* tau_lo, void* stream, BP... bp) {
    REQUIRE(dim >= 8 && dim % 8 == 0 && dim <= 2048, "dim=%d must be a multiple of 8 in [8,2048]", dim);
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(queries && queries_bf16 && max_norm && tau && tau_lo, "null pointer");
    REQUIRE(ld_queries >= dim && ld_queries_bf16 >= dim && ld_tau >= 1, "bad leading dimension");
    ProfScope prof(tag, 0.0, 0.0, reinterpret_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(ivf_filter_bounds_kernel<BP...>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       queries, (long long)ld_queries, queries_bf16, (long long)ld_queries_bf16, dim, (long long)nq, max_norm, tau,
                       (long long)ld_tau, tau_lo, bp...);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_filter_bounds(const float* queries, int64_t nq, int64_t ld_queries, int dim,
                                        const uint16_t* queries_bf16, int64_t ld_queries_bf16, const float* max_norm,
                                        const float* tau, int64_t ld_tau, float* tau_lo, void* stream) {
    return filter_bounds_impl("ivf_filter_bounds", queries, nq, ld_queries, dim, queries_bf16, ld_queries_bf16, max_norm, tau,
                              ld_tau, tau_lo, stream);
}

extern "C" int amdrec_ivf_filter_bounds_boosted(const float* queries, int64_t nq, int64_t ld_queries, int dim,
                                                const uint16_t* queries_bf16, int64_t ld_queries_bf16, const float* max_norm,
                                                const float* tau, int64_t ld_tau, float* tau_lo, void* stream,
                                                const float* weight, float boost_max) {
    if (nq > 0) {
        REQUIRE(weight != nullptr, "weight is null");
        REQUIRE(((uintptr_t)weight % 4) == 0, "weight must be 4-byte aligned");
    }
    if (int rc = boost_max_check(boost_max)) return rc;
    return filter_bounds_impl("ivf_filter_bounds_boost", queries, nq, ld_queries, dim, queries_bf16, ld_queries_bf16, max_norm,
                              tau, ld_tau, tau_lo, stream, weight, boost_max);
}

template <class EL, class BO = ListNoBoost>
static int scan_grouped_mixed_impl(const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim,
                                   const int64_t* row_pos, const int64_t* list_off, int nlist, int64_t max_list_rows,
                                   const float* queries, int64_t ld_queries, const uint16_t* queries_bf16,
                                   int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
                                   int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys,
                                   int64_t pool_ld, int64_t pos_offset, const float* tau, int64_t ld_tau,
                                   const float* tau_lo, int64_t* pool_fill, void* stream, EL el, BO bo = {}) {
    const GroupedArgs a{lists, ld, dim, row_pos, list_off, max_list_rows, queries, ld_queries, group_off, qtile_prefix, qtile_bound,
                        qtile, pair_query, pool_keys};
    if (int rc = a.check_dim(8)) return rc;
    REQUIRE(nlist >= 1, "bad nlist");
    if (int rc = a.check_qtile()) return rc;
    if (a.empty()) return AMDREC_OK;
    if (int rc = a.check_bound()) return rc;
    REQUIRE(a.pointers() && lists_bf16 && queries_bf16 && tau && tau_lo && pool_fill, "null pointer");
    REQUIRE(a.leading_dims() && ld_bf16 >= dim && ld_bf16 % 8 == 0 && ld_queries_bf16 >= dim && ld_queries_bf16 % 8 == 0 &&
                ld_tau >= 1, "bad leading dimension");
    REQUIRE(((uintptr_t)lists % 16) == 0 && ((uintptr_t)lists_bf16 % 16) == 0 && ((uintptr_t)queries % 16) == 0 &&
                ((uintptr_t)queries_bf16 % 16) == 0, "lists / queries must be 16-byte aligned");
    if (int rc = elig_check(el)) return rc;
    if (int rc = boost_check(bo)) return rc;
    const hipError_t e = with_scan_shape<true, EL, BO>(qtile, max_list_rows <= SHORT_LIST_ROWS, [&](auto shape, const char* tag) {
        using S = decltype(shape);
        constexpr auto kern = AMDREC_LIST_KERNEL(ivf_group_scan_mixed_kernel, S,);
        return launch_grouped<S, kern>(
            el, bo, tag, max_list_rows, qtile_bound, reinterpret_cast<hipStream_t>(stream), lists, ld, lists_bf16, ld_bf16, dim,
            (dim / 2 + BK - 1) / BK, (const long long*)row_pos, (const long long*)list_off, queries, ld_queries, queries_bf16,
            ld_queries_bf16, (const long long*)group_off, (const long long*)qtile_prefix, nlist, (const long long*)pair_query,
            (unsigned long long*)pool_keys, pool_ld, pos_offset, tau, ld_tau, tau_lo, (unsigned long long*)pool_fill);
    });
    HIP_TRY(e);
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_scan_grouped_mixed(const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim,
                                             const int64_t* row_pos, const int64_t* list_off, int nlist, int64_t max_list_rows,
                                             const float* queries, int64_t ld_queries, const uint16_t* queries_bf16,
                                             int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
                                             int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys,
                                             int64_t pool_ld, int64_t pos_offset, const float* tau, int64_t ld_tau,
                                             const float* tau_lo, int64_t* pool_fill, void* stream) {
    return scan_grouped_mixed_impl(lists, ld, lists_bf16, ld_bf16, dim, row_pos, list_off, nlist, max_list_rows, queries,
                                   ld_queries, queries_bf16, ld_queries_bf16, group_off, qtile_prefix, qtile_bound, qtile,
                                   pair_query, pool_keys, pool_ld, pos_offset, tau, ld_tau, tau_lo, pool_fill, stream,
                                   ListNoElig{});
}

extern "C" int amdrec_ivf_scan_grouped_mixed_eligible(
    const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim, const int64_t* row_pos,
    const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries, int64_t ld_queries,
    const uint16_t* queries_bf16, int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
    int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
    const float* tau, int64_t ld_tau, const float* tau_lo, int64_t* pool_fill, void* stream, const uint64_t* list_tags,
    const uint64_t* require_all, const uint64_t* require_any) {
    return scan_grouped_mixed_impl(lists, ld, lists_bf16, ld_bf16, dim, row_pos, list_off, nlist, max_list_rows, queries,
                                   ld_queries, queries_bf16, ld_queries_bf16, group_off, qtile_prefix, qtile_bound, qtile,
                                   pair_query, pool_keys, pool_ld, pos_offset, tau, ld_tau, tau_lo, pool_fill, stream,
                                   ListElig{list_tags, require_all, require_any});
}

extern "C" int amdrec_ivf_scan_grouped_mixed_boosted(
    const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim, const int64_t* row_pos,
    const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries, int64_t ld_queries,
    const uint16_t* queries_bf16, int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
    int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
    const float* tau, int64_t ld_tau, const float* tau_lo, int64_t* pool_fill, void* stream, const float* list_boosts,
    const float* weight) {
    return scan_grouped_mixed_impl(lists, ld, lists_bf16, ld_bf16, dim, row_pos, list_off, nlist, max_list_rows, queries,
                                   ld_queries, queries_bf16, ld_queries_bf16, group_off, qtile_prefix, qtile_bound, qtile,
                                   pair_query, pool_keys, pool_ld, pos_offset, tau, ld_tau, tau_lo, pool_fill, stream,
                                   ListNoElig{}, ListBoost{list_boosts, weight});
}

extern "C" int amdrec_ivf_scan_grouped_mixed_eligible_boosted(
    const float* lists, int64_t ld, const uint16_t* lists_bf16, int64_t ld_bf16, int dim, const int64_t* row_pos,
    const int64_t* list_off, int nlist, int64_t max_list_rows, const float* queries, int64_t ld_queries,
    const uint16_t* queries_bf16, int64_t ld_queries_bf16, const int64_t* group_off, const int64_t* qtile_prefix,
    int64_t qtile_bound, int qtile, const int64_t* pair_query, uint64_t* pool_keys, int64_t pool_ld, int64_t pos_offset,
    const float* tau, int64_t ld_tau, const float* tau_lo, int64_t* pool_fill, void* stream, const uint64_t* list_tags,
    const uint64_t* require_all, const uint64_t* require_any, const float* list_boosts, const float* weight) {
    return scan_grouped_mixed_impl(lists, ld, lists_bf16, ld_bf16, dim, row_pos, list_off, nlist, max_list_rows, queries,
                                   ld_queries, queries_bf16, ld_queries_bf16, group_off, qtile_prefix, qtile_bound, qtile,
                                   pair_query, pool_keys, pool_ld, pos_offset, tau, ld_tau, tau_lo, pool_fill, stream,
                                   ListElig{list_tags, require_all, require_any}, ListBoost{list_boosts, weight});
}

extern "C" int amdrec_ivf_coarse_keys(const float* centroids, int nlist, int64_t ld_centroids, int dim, const float* queries,
                                      int64_t nq, int64_t ld_queries, uint64_t* keys, int64_t ld_keys, void* stream) {
    REQUIRE(dim >= 4 && dim % 4 == 0 && dim <= 2048, "dim=%d must be a multiple of 4 in [4,2048]", dim);
    REQUIRE(nlist >= 1 && nlist <= (1 << 20), "nlist out of range");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(centroids && queries && keys, "null pointer");
    REQUIRE(ld_centroids >= dim && ld_centroids % 4 == 0 && ld_queries >= dim && ld_queries % 4 == 0 && ld_keys >= (nlist + 1) / 2 * 2 &&
                ld_keys % 2 == 0,
            "bad leading dimension");
    REQUIRE(((uintptr_t)centroids % 16) == 0 && ((uintptr_t)queries % 16) == 0, "centroids / queries must be 16-byte aligned");
    REQUIRE(((uintptr_t)keys % 16) == 0, "keys must be 16-byte aligned");
    REQUIRE(nq < (1ll << 24), "nq out of range");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DenseRows lp{centroids, nlist, (int)ld_centroids, dim, 30, 1ll << 30};
    DenseRows lq{queries, nq, (int)ld_queries, dim, 30, 1ll << 30};
    EpiCoarseKeys epi{reinterpret_cast<unsigned long long*>(keys), (long long)ld_keys, (int)nq, (long long)nlist};
    hipError_t e;                                       // the query-tile shapes of amdrec_flat_search's filter pass
    if (nq > 64)      e = launch_gemm<Shape<2, 2, 4, 2>, false>(lp, lq, epi, dim, nlist, nq, st);
    else if (nq > 32) e = launch_gemm<Shape<4, 1, 2, 2>, false>(lp, lq, epi, dim, nlist, nq, st);
    else              e = launch_gemm<Shape<4, 1, 2, 1>, false>(lp, lq, epi, dim, nlist, nq, st);
    HIP_TRY(e);
    return AMDREC_OK;
}

template <class EL, class BO>
static hipError_t coarse_keys_aware_launch(const DenseRows& lp, const DenseRows& lq, uint64_t* keys, int64_t ld_keys, int64_t nq,
                                           int nlist, int dim, const int64_t* list_len, EL el, BO bo, hipStream_t st) {
    EpiCoarseKeysAwareT<EL, BO> epi{reinterpret_cast<unsigned long long*>(keys), (long long)ld_keys, (int)nq, (long long)nlist,
                                    reinterpret_cast<const long long*>(list_len), el, bo};
    // amdrec_ivf_coarse_keys' shapes: c is that table's score bit for bit
    if (nq > 64) return launch_gemm<Shape<2, 2, 4, 2>, false>(lp, lq, epi, dim, nlist, nq, st);
    if (nq > 32) return launch_gemm<Shape<4, 1, 2, 2>, false>(lp, lq, epi, dim, nlist, nq, st);
    return launch_gemm<Shape<4, 1, 2, 1>, false>(lp, lq, epi, dim, nlist, nq, st);
}

extern "C" int amdrec_ivf_coarse_keys_aware(const float* centroids, int nlist, int64_t ld_centroids, int dim, const float* queries,
                                            int64_t nq, int64_t ld_queries, uint64_t* keys, int64_t ld_keys,
                                            const int64_t* list_len, const uint64_t* tag_or, const uint64_t* require_all,
                                            const uint64_t* require_any, const float* boost_hi, const float* boost_lo,
                                            const float* weight, void* stream) {
    REQUIRE(dim >= 4 && dim % 4 == 0 && dim <= 2048, "dim=%d must be a multiple of 4 in [4,2048]", dim);
    REQUIRE(nlist >= 1 && nlist <= (1 << 20), "nlist out of range");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(centroids && queries && keys && list_len, "null pointer");
    REQUIRE(ld_centroids >= dim && ld_centroids % 4 == 0 && ld_queries >= dim && ld_queries % 4 == 0 && ld_keys >= (nlist + 1) / 2 * 2 &&
                ld_keys % 2 == 0,
            "bad leading dimension");
    REQUIRE(((uintptr_t)centroids % 16) == 0 && ((uintptr_t)queries % 16) == 0, "centroids / queries must be 16-byte aligned");
    REQUIRE(((uintptr_t)keys % 16) == 0, "keys must be 16-byte aligned");
    REQUIRE(nq < (1ll << 24), "nq out of range");
    const bool masked = tag_or || require_all || require_any, boosted = boost_hi || boost_lo || weight;
    REQUIRE(!masked || (tag_or && require_all && require_any), "masks need tag_or, require_all and require_any");
    REQUIRE(!boosted || (boost_hi && boost_lo && weight), "a weight needs boost_hi, boost_lo and weight");
    REQUIRE(((uintptr_t)list_len % 16) == 0 && ((uintptr_t)tag_or % 16) == 0 && ((uintptr_t)boost_hi % 16) == 0 &&
                ((uintptr_t)boost_lo % 16) == 0,
            "the per-list arrays must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DenseRows lp{centroids, nlist, (int)ld_centroids, dim, 30, 1ll << 30};
    DenseRows lq{queries, nq, (int)ld_queries, dim, 30, 1ll << 30};
    const CoarseElig el{reinterpret_cast<const unsigned long long*>(tag_or), require_all, require_any};
    const CoarseBoost bo{boost_hi, boost_lo, weight};
    hipError_t e;
    if (masked && boosted) e = coarse_keys_aware_launch(lp, lq, keys, ld_keys, nq, nlist, dim, list_len, el, bo, st);
    else if (masked)       e = coarse_keys_aware_launch(lp, lq, keys, ld_keys, nq, nlist, dim, list_len, el, CoarseNoBoost{}, st);
    else if (boosted)      e = coarse_keys_aware_launch(lp, lq, keys, ld_keys, nq, nlist, dim, list_len, CoarseNoElig{}, bo, st);
    else                   e = coarse_keys_aware_launch(lp, lq, keys, ld_keys, nq, nlist, dim, list_len, CoarseNoElig{}, CoarseNoBoost{}, st);
    HIP_TRY(e);
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_list_summaries(const int64_t* list_off, int nlist, const uint64_t* list_tags, const float* list_boosts,
                                         uint64_t* tag_or, float* boost_hi, float* boost_lo, void* stream) {
    REQUIRE(nlist >= 1 && nlist <= (1 << 20), "nlist out of range");
    REQUIRE(list_off, "null pointer");
    REQUIRE(!list_tags || tag_or, "list_tags without tag_or");
    REQUIRE(!list_boosts || (boost_hi && boost_lo), "list_boosts without boost_hi / boost_lo");
    if (!list_tags && !list_boosts) return AMDREC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("ivf_list_summaries", 0.0, 0.0, st);
    const unsigned blocks = (unsigned)std::min<long long>(((long long)nlist + 3) / 4, 1024);   // 4096 waves; more lists: grid-stride
    hipLaunchKernelGGL(ivf_list_summaries_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const long long*>(list_off), nlist,
                       reinterpret_cast<const unsigned long long*>(list_tags), list_boosts,
                       reinterpret_cast<unsigned long long*>(tag_or), boost_hi, boost_lo);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}


extern "C" int amdrec_ivf_select(const uint64_t* pool_keys, int64_t pool_ld, const int64_t* pool_count, int64_t nq,
                                 int k, float* out_scores, int64_t* out_pos, void* stream) {
    REQUIRE(k >= 1 && k <= AMDREC_MAX_K, "k=%d outside [1,%d]", k, AMDREC_MAX_K);
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(pool_keys && pool_count && out_scores && out_pos, "null pointer");
    ProfScope prof("ivf_select", 0.0, 0.0, reinterpret_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)nq), dim3(512), 0, reinterpret_cast<hipStream_t>(stream),
                       (const unsigned long long*)pool_keys, (long long)pool_ld, (const long long*)pool_count, k,
                       out_scores, (long long*)out_pos);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_ivf_select_split(const uint64_t* pool_keys, int64_t pool_ld, const int64_t* pool_count, int64_t nq,
                                       int k, int slices, float* out_scores, int64_t* out_pos, void* workspace,
                                       size_t workspace_bytes, int32_t* tickets, void* stream) {
    REQUIRE(k >= 1 && k <= AMDREC_MAX_K, "k=%d outside [1,%d]", k, AMDREC_MAX_K);
    REQUIRE(slices >= 1 && slices <= 1024 && nq <= 65535, "slices / nq out of range");
    if (nq <= 0) return AMDREC_OK;
    REQUIRE(pool_keys && pool_count && out_scores && out_pos && tickets, "null pointer");
    const size_t need = (size_t)nq * slices * k * 8;
    if (int rc = require_workspace(workspace, workspace_bytes, need, 16)) return rc;
    ProfScope prof("ivf_select", 0.0, 0.0, reinterpret_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(ivf_select_split_kernel, dim3((unsigned)slices, (unsigned)nq), dim3(512), 0,
                       reinterpret_cast<hipStream_t>(stream), (const unsigned long long*)pool_keys, (long long)pool_ld,
                       (const long long*)pool_count, k, reinterpret_cast<unsigned long long*>(workspace), tickets, out_scores,
                       (long long*)out_pos);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
