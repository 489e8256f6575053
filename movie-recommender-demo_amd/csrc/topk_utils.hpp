// Block-wide helpers shared by the flat, IVF and IVFPQ-refine top-k kernels: radix select over LDS histograms, sorts of
// 64-bit keys, the last-workgroup hand-off, the fp32 re-score, the mixed search's error bound, candidate-list bookkeeping
// and certificate, result write-out.
#pragma once
#include "common.hpp"

namespace amdrec {

// ---- block-wide helpers -------------------------------------------------------------
// Find, scanning bins from the top, the bin that holds the r-th largest element.
// hist[NB] in LDS; returns bin and updates r to the rank inside that bin.  All threads call.
template <int NB, int NT>
__device__ inline int find_bin_desc(const int* hist, int& r, int* scratch /*[NT+2]*/) {
    // Thread t owns bins [t*PER, (t+1)*PER).  A suffix scan over the threads' sums (wave shuffles + one LDS round
    // over the wave totals) gives each thread the count of keys in bins above its own; exactly one thread's range
    // holds the r-th largest key.  (A serial scan by one lane cost ~25 us per call at NT = 512.)
    constexpr int PER = NB / NT;
    constexpr int NW = NT / 64;
    static_assert(NB % NT == 0 && NT % 64 == 0, "bins must split evenly over whole waves");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int local = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) local += hist[tid * PER + i];
    int incl = local;                               // inclusive suffix sum within the wave (lanes >= mine)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl += v;
    }
    if (lane == 0) scratch[wv] = incl;              // wave total
    if (tid == 0) scratch[NT] = -1;
    __syncthreads();
    int above = incl - local;                       // keys in higher bins of this wave ...
#pragma unroll
    for (int x = 0; x < NW; ++x)
        if (x > wv) above += scratch[x];            // ... and of the higher waves
    if (above < r && r <= above + local) {          // the r-th largest lies in my bins (exactly one thread)
        int bin = -1;
#pragma unroll
        for (int i = PER - 1; i >= 0; --i) {
            const int h = hist[tid * PER + i];
            if (bin < 0) {
                if (above + h >= r) bin = tid * PER + i;
                else above += h;
            }
        }
        scratch[NT] = bin;
        scratch[NT + 1] = r - above;
    }
    __syncthreads();
    const int bin = scratch[NT];
    r = scratch[NT + 1];
    __syncthreads();
    return bin;
}

// Bitonic sort of P (power of two) 64-bit keys in LDS, descending.  All threads call; blockDim.x must be a
// multiple of 64.  The network is indexed by compare-exchange PAIR (pair p -> elements i, i | st with the st
// bit spliced out of p), so every lane does useful work.  A pair with st < 32 lies inside the 64 consecutive
// elements owned by one wave's pair group, and a wave's LDS operations execute in order, so those stages need
// only a wave-level fence; block barriers are paid for st >= 32 and at the end of each outer stage.
// SITE (here and in the two sorts below): an instantiation of its own for a caller whose arrays are not the other callers'.
// The kernels of a translation unit that call one instantiation with the same LDS arrays get those arrays folded into it as
// constants; a further caller with other arrays would undo that for all of them, so it takes SITE != 0 and leaves theirs alone.
template <int SITE = 0>
__device__ inline void bitonic_desc(unsigned long long* buf, int P) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int half = P >> 1;
    for (int sz = 2; sz <= P; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int p = tid; p < half; p += nt) {
                const int i = ((p & ~(st - 1)) << 1) | (p & (st - 1));
                const int j = i | st;
                const unsigned long long a = buf[i], b = buf[j];
                const bool desc = (i & sz) == 0;
                if (desc ? (a < b) : (a > b)) { buf[i] = b; buf[j] = a; }
            }
            if (st >= 32 || st == 1) __syncthreads();
            else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
}

// Descending sort of m <= 512 R keys in LDS by a 512-thread block (R = 2 or 4 keys per lane), keys UNIQUE and non-zero
// (0 = padding): `src`[0 .. m) -> `dst`[0 .. m) (two different arrays of >= 512 R keys; `src` is overwritten; positions of
// `dst` that receive no key keep their contents: clear them first if zeros can occur among the m).  Each of the 8 waves
// sorts a run of 64 R keys in registers (a bitonic network on shuffles: 28 stages at R = 2, 36 at R = 4), the runs go back to
// `src`, and every key finds its final position as its index in its own run + the number of larger keys in each other run
// (a binary search per run: the runs are sorted and the keys unique).  ~4 us at 1024 keys against ~17 for the all-LDS
// bitonic network (66 stages, most of them behind a block barrier) - the single-query search's finalize was the sort.
template <int R, int SITE = 0>
__device__ inline void sort_desc_runs(unsigned long long* src, unsigned long long* dst, int m) {
    static_assert(R == 2 || R == 4, "two or four keys per lane");
    constexpr int RUN = 64 * R, STEPS = R == 2 ? 8 : 9;      // binary search over 0 .. RUN
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long key[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = RUN * w + 64 * r + lane;
        key[r] = i < m ? src[i] : 0ull;
    }
    __syncthreads();                                        // every key is in registers: `src` may be overwritten
#pragma unroll
    for (int k = 2; k <= RUN; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {                                   // the partner is another register of the same lane
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int pr = r ^ (j >> 6);
                    if (pr < r) continue;                    // each pair once, from its lower element
                    const bool desc = ((64 * r) & k) == 0;
                    const unsigned long long a = key[r], b = key[pr];
                    const bool swap = desc ? (a < b) : (a > b);
                    key[r] = swap ? b : a;
                    key[pr] = swap ? a : b;
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = 64 * r + lane;
                    const unsigned long long other = __shfl_xor(key[r], j, 64);
                    const bool lower = (lane & j) == 0;          // i < partner
                    const bool desc = (i & k) == 0;              // this k-block ends descending
                    const bool take_max = lower == desc;
                    const bool other_greater = other > key[r];
                    key[r] = (take_max == other_greater) ? other : key[r];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) src[RUN * w + 64 * r + lane] = key[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (key[r] == 0ull) continue;
        int rank = 64 * r + lane;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (v == w) continue;
            const unsigned long long* run = src + RUN * v;
            int lo = 0, hi = RUN;
#pragma unroll
            for (int it = 0; it < STEPS; ++it) {             // keys of the run greater than mine: 0 .. RUN (zeros are smaller than any key)
                const int mid = (lo + hi) >> 1;
                if (lo < hi && run[mid] > key[r]) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        dst[rank] = key[r];
    }
    __syncthreads();
}

// |bf16 inner product - fp32 inner product| of a query against any corpus row (derivation: search.hip, "Error bound of the
// bf16 pass"): qn = ||q||, dqn = ||bf16(q) - q||, M / D = largest row norm / largest row rounding-error norm of the corpus.
__device__ __forceinline__ float eps_bound(float qn, float dqn, float M, float D, int d) {
    return (dqn * (M + D) + qn * D) * 1.0001f + (float)d * 1.2e-7f * qn * (M + D);
}

// m keys in `keys` (0 = empty) -> descending; returns where they are.  Up to `network_max` keys - and beyond 2048, or with a
// block of other than 512 threads - the all-LDS network sorts `keys` in place (cheap for a few hundred keys; 66 stages, most
// behind a block barrier, for 2048); between, the per-wave run sort writes `other` (>= 1024 keys for m <= 1024, else 2048;
// its keys must be unique: a fixed ~4 us whatever the count).  All threads call.
template <int NT, int SITE = 0>
__device__ inline const unsigned long long* sort_keys_desc(unsigned long long* keys, unsigned long long* other, int m,
                                                           int network_max) {
    const int tid = threadIdx.x;
    if constexpr (NT == 512) {
        if (m > network_max && m <= 2048) {
            for (int i = tid; i < (m <= 1024 ? 1024 : 2048); i += NT) other[i] = 0ull;   // the run sort places no zero key
            __syncthreads();
            if (m <= 1024) sort_desc_runs<2, SITE>(keys, other, m);
            else sort_desc_runs<4, SITE>(keys, other, m);
            return other;
        }
    }
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = m + tid; i < P; i += NT) keys[i] = 0ull;
    __syncthreads();
    bitonic_desc<SITE>(keys, P);
    return keys;
}

// The k-th largest 32-bit score image among the block's keys, by PASSES radix passes of 11 + 11 + 10 bits from the top
// (PASSES < 3: the low bits stay clear, a value <= the k-th).  for_each_key(f) calls f(key) for the calling thread's share
// of the 64-bit keys; key 0 is an empty slot and is not counted.  Fewer than k keys -> 0.  FIT > 0: stops as soon as the
// keys at or above the prefix found so far number <= FIT (the caller gathers those and sorts: the remaining passes - each a
// walk over the keys - are not needed).  hist[2048], scratch[NT + 2] in LDS; all threads call; the result is block-uniform.
template <int NT, int PASSES, int FIT = 0, class ForEachKey>
__device__ inline uint32_t select_prefix_desc(int* hist, int* scratch, int k, ForEachKey for_each_key) {
    constexpr int shifts[3] = {21, 10, 0}, nbits[3] = {11, 11, 10};
    uint32_t prefix = 0u, pmask = 0u;
    int rr = k;
#pragma unroll
    for (int pass = 0; pass < PASSES; ++pass) {
        for (int i = threadIdx.x; i < 2048; i += NT) hist[i] = 0;
        __syncthreads();
        const uint32_t bm = (1u << nbits[pass]) - 1u;
        for_each_key([&](unsigned long long key) {
            const uint32_t u = (uint32_t)(key >> 32);
            if (key != 0ull && (u & pmask) == prefix) atomicAdd(&hist[(u >> shifts[pass]) & bm], 1);
        });
        __syncthreads();
        const int bin = find_bin_desc<2048, NT>(hist, rr, scratch);
        if (bin < 0) return 0u;                              // (pass 0 only) block-uniform
        prefix |= (uint32_t)bin << shifts[pass];
        pmask |= bm << shifts[pass];
        if constexpr (FIT > 0) {
            // the k - rr keys above the bin (rr = the k-th key's rank inside it) + the bin's own
            const int at_or_above = (k - rr) + hist[bin];
            __syncthreads();                                 // hist is cleared by the next pass
            if (at_or_above <= FIT) break;                   // block-uniform
        }
    }
    return prefix;
}

// ---- cross-workgroup hand-off ---------------------------------------------------------
// n workgroups each store their part of a result, then call this with the same ticket (0 before the first): true in the one
// that arrives last, where every part is then visible (agent-scope release / acquire around the ticket, as in
// cdna_hip_programming.md "in-launch split-K reduction").  reset: the last one returns the ticket to 0 for the next launch.
// All threads call; the result is block-uniform; begins and ends with a block barrier.
__device__ inline bool last_workgroup(int* ticket, int n, bool reset) {
    __shared__ int last_sh;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's stores are out
    __syncthreads();                                           // ... every wave's
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the fence's own wait may be dropped: keep this one)
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_sh = t == n - 1;
        if (t == n - 1) {
            if (reset) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return last_sh;
}

// ---- fp32 re-score ----------------------------------------------------------------------
// a[u] = <row xr[u], qv> for RU rows by one wave (d4 = dim / 4 16-byte chunks; qv in LDS; every lane gets the sums).  One
// fixed evaluation order per row: lane l folds its chunks l, l + 64, ... into one fma chain in element order, then the 64
// partial sums go through the xor butterfly 32 .. 1.  Column chunk outermost: the RU row loads of one chunk are independent
// and go out back to back (with the row loop outside, each row's load had to return before the next row's was issued:
// measured 100 ns per row).
template <int RU>
__device__ __forceinline__ void dot_rows(const f32x4* (&xr)[RU], const float* qv, int d4, int lane, float (&a)[RU]) {
#pragma unroll
    for (int u = 0; u < RU; ++u) a[u] = 0.f;
    for (int c = lane; c < d4; c += 64) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(&qv[4 * c]);
        f32x4 x[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) x[u] = xr[u][c];
#pragma unroll
        for (int u = 0; u < RU; ++u)           // explicit fma chain: the same rounding sequence in every slot u
            a[u] = __builtin_fmaf(x[u][3], y[3], __builtin_fmaf(x[u][2], y[2], __builtin_fmaf(x[u][1], y[1],
                                  __builtin_fmaf(x[u][0], y[0], a[u]))));
    }
#pragma unroll
    for (int u = 0; u < RU; ++u)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[u] += __shfl_xor(a[u], o, 64);
}

// keys[0 .. n) in LDS (approximate score, corpus position) -> (exact fp32 score, position), by a block of NW waves: one
// wave per key, RU rows (random 1 KB reads: latency-bound) in flight per wave.  A NaN score (inf - inf in fp32 that the bf16
// pass did not produce) becomes key 0 and ranks last, as in the fix-up scan.  Ends with a block barrier.
// `term`: what is added to a row's inner product to form its score.  NoTerm: nothing - the plain searches.  RowBoost: the
// boosted flat search's t = w * boost[pos], as TWO rounded fp32 operations, t = w * b and s = ip + t, whatever the
// translation unit's contraction setting (a fused multiply-add would round once and differ from the scan's key in the last bit).
__device__ __forceinline__ float boost_term(float w, float b) {
#pragma clang fp contract(off)
    return w * b;
}
__device__ __forceinline__ float boost_add(float ip, float t) {
#pragma clang fp contract(off)
    return ip + t;
}
struct NoTerm {
    static constexpr bool boosted = false;
};
struct RowBoost {
    static constexpr bool boosted = true;
    const float* boost;      // [nrows]
    float w;                 // the query's weight
    __device__ __forceinline__ float operator()(float ip, uint32_t pos) const { return boost_add(ip, boost_term(w, boost[pos])); }
};
template <int NW, int RU, class Term = NoTerm>
__device__ inline void rescore_keys(unsigned long long* keys, int n, const float* X, long long ldx, const float* qv, int d4,
                                    Term term = Term{}) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i0 = w; i0 < n; i0 += NW * RU) {
        float a[RU];
        uint32_t pos[RU];
        const f32x4* xr[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int i = i0 + NW * u;
            pos[u] = key_pos(keys[i < n ? i : i0]);
            xr[u] = reinterpret_cast<const f32x4*>(X + (long long)pos[u] * ldx);
        }
        dot_rows<RU>(xr, qv, d4, lane, a);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // keys[i] of this round were read (pos) before they are rewritten
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int i = i0 + NW * u;
            if constexpr (Term::boosted) {
                if (lane == 0 && i < n) keys[i] = (a[u] == a[u]) ? make_key(term(a[u], pos[u]), pos[u]) : 0ull;
            } else {
                if (lane == 0 && i < n) keys[i] = (a[u] == a[u]) ? make_key(a[u], pos[u]) : 0ull;
            }
        }
    }
    __syncthreads();
}

// ---- the bf16 pass's error bound and candidate lists (flat mixed search) ----------------------------------------
// fp32 bits -> bf16 bits, round to nearest even (NaN is the caller's business)
__device__ __forceinline__ uint32_t bf16_rne(uint32_t u) { return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }

// Copies the query Q[0 .. d) to qv (LDS) and returns eps_bound for it against the corpus norms max_norm[0 .. 2): ||q|| and
// ||q - bf16(q)||, the rounding that bf16_rows_kernel applies.  NT threads all call; red[16] in LDS; one block barrier
// inside, after which qv is complete.
template <int NT>
__device__ inline float query_eps(const float* Q, int d, float* qv, float* red, const float* max_norm) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float ss = 0.f, ds = 0.f;
    for (int i = tid; i < d; i += NT) {
        const float v = Q[i];
        qv[i] = v;
        ss += v * v;
        const float dv = v - __uint_as_float(bf16_rne(__float_as_uint(v)) << 16);
        ds += dv * dv;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o, 64);
        ds += __shfl_xor(ds, o, 64);
    }
    if (lane == 0) { red[w] = ss; red[8 + w] = ds; }
    __syncthreads();
    float qn = 0.f, dqn = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) { qn += red[i]; dqn += red[8 + i]; }
    return eps_bound(sqrtf(qn), sqrtf(dqn) * 1.0001f, max_norm[0], max_norm[1], d);
}

// A query's candidate block: nseg (<= 256) segments of seg_cap slots, slot-major, + oc keys in an overflow block;
// segcnt[0 .. nseg) = hits each segment saw (the excess over seg_cap went to the overflow block).  Fills seg_n[g] = valid
// slots of segment g (and raises *maxn, if given - the caller's thread 0 cleared it -, to the largest) and returns the
// candidate count c, or -1 when the list is not usable: a hit is in neither place, more than 2048 overflowed, or c outside
// [need, cap].  NT threads all call; the result is block-uniform; a block barrier first and last.
template <int NT>
__device__ inline int segment_counts(const int* segcnt, int nseg, int seg_cap, int oc, int need, int cap, int* seg_n,
                                     int* maxn = nullptr) {
    __shared__ int tot_sh, lost_sh;
    const int tid = threadIdx.x;
    if (tid == 0) { tot_sh = 0; lost_sh = 0; }
    __syncthreads();
    for (int g0 = 0; g0 < nseg; g0 += NT) {
        int sv = 0, lost = 0;
        if (g0 + tid < nseg) {
            const int v = segcnt[g0 + tid];
            sv = v < seg_cap ? v : seg_cap;
            lost = v - sv;
            seg_n[g0 + tid] = sv;
            if (maxn && sv) atomicMax(maxn, sv);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sv += __shfl_xor(sv, o, 64);
            lost += __shfl_xor(lost, o, 64);
        }
        if ((tid & 63) == 0) {
            if (sv) atomicAdd(&tot_sh, sv);
            if (lost) atomicAdd(&lost_sh, lost);
        }
    }
    __syncthreads();
    const int c = tot_sh + oc;
    return (lost_sh != oc || oc > 2048 || c < need || c > cap) ? -1 : c;
}

// does element s_ of the slot-major segment area (slot s_ / nseg of segment s_ % nseg) hold a key?  (An empty slot is key 0,
// which no hit can be: its score would have to be NaN.)
__device__ __forceinline__ bool slot_valid(int s_, int nseg, int seg_cap, const int* seg_n) {
    if (s_ >= nseg * seg_cap) return false;
    const int slot = (nseg & (nseg - 1)) == 0 ? s_ >> (31 - __builtin_clz((unsigned)nseg)) : s_ / nseg;
    return slot < seg_n[s_ - slot * nseg];
}

// query q goes to the exact fix-up scan; fail[nq] counts such queries.  One workgroup per query calls, all its threads.
__device__ inline void give_up(int* fail, int q, int nq) {
    if (threadIdx.x == 0) {
        fail[q] = 1;
        atomicAdd(&fail[nq], 1);
    }
}

// Certificate of the mixed search (block-uniform): rows outside the candidate list have exact score < bound = tau + eps, so
// the sorted exact keys hold the top `need` if the need-th reaches the bound (or the list held every row).  If not, gives up.
__device__ inline bool certify_or_fail(const unsigned long long* sorted, int need, bool all_rows, float bound, int* fail,
                                       int q, int nq) {
    const unsigned long long kth = sorted[need - 1];
    if (all_rows || (kth != 0ull && key_score(kth) >= bound)) return true;
    give_up(fail, q, nq);
    return false;
}

// ---- per-group caps (amdrec_select_topk_capped, amdrec_group_cap_compact) -----------------------------------------
// The group key of corpus position pos: group_of[pos], or -1 (ungrouped) for a position outside [0, n_rows), which is never read.
__device__ __forceinline__ long long group_at(const long long* group_of, long long n_rows, long long pos) {
    return (pos >= 0 && pos < n_rows) ? group_of[pos] : -1ll;
}

// grp[0 .. n) in LDS: the group keys of a query's entries in rank order (negative = ungrouped, or no entry at all).  Does
// entry i of group g >= 0 have fewer than `cap` earlier entries of its group, i.e. does the greedy pass accept it?  The scan
// stops once cap earlier ones are seen: a row that is all one group costs ~cap reads per entry, a row of distinct groups i reads
// (every lane of a wave reads the same words: LDS broadcasts).  Blocks of 8 entries between two looks at the count: their
// reads are independent and go out together (one entry per trip waited a whole LDS latency for each: 135 us against 40 for
// amdrec_group_cap_compact at 512 x 1000 -> 500).
__device__ __forceinline__ bool below_group_cap(const long long* grp, int i, long long g, int cap) {
    int seen = 0, j = 0;
    for (; j + 8 <= i && seen < cap; j += 8) {
        int hit = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) hit += grp[j + t] == g;
        seen += hit;
    }
    for (; j < i && seen < cap; ++j) seen += grp[j] == g;
    return seen < cap;
}

// Order-preserving compaction by a block of NT threads whose thread t owns entries t, t + NT, ... (ROUNDS of them): slot[r]
// = the number of kept entries before entry r * NT + t, returns the number kept in all.  Wave ballot + popcount of the lower
// lanes, the wave totals of every round through LDS behind ONE block barrier.  All threads call.
template <int NT, int ROUNDS>
__device__ inline int compact_slots(const bool (&keep)[ROUNDS], int (&slot)[ROUNDS], int (*wave_total)[NT / 64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned long long m = __ballot(keep[r]);
        slot[r] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[r][w] = __popcll(m);
    }
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        slot[r] += base;
#pragma unroll
        for (int x = 0; x < NT / 64; ++x) {
            const int t = wave_total[r][x];
            if (x < w) slot[r] += t;
            base += t;
        }
    }
    return base;
}

__device__ inline void write_result(const unsigned long long* buf, int have, int k, long long q, float* outD,
                                    long long* outI, long long pos_offset) {
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        unsigned long long key = (i < have) ? buf[i] : 0ull;
        bool valid = key != 0ull;
        outD[q * k + i] = valid ? key_score(key) : -INFINITY;
        outI[q * k + i] = valid ? (long long)key_pos(key) + pos_offset : -1ll;
    }
}


}  // namespace amdrec
