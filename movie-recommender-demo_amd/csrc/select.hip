// Stage-2 selection (inference.py:258-263, faiss_retrieval.py:355-358): per user, the top_k of its k_c ranked candidates, the
// winners' ad ids, candidate slots and sigmoid of every task's logit.  ONE frame serves amdrec_select_topk (order by the
// ranking task's LOGIT: sigmoid is monotone, and ranking on logits avoids the ties of saturated sigmoids),
// amdrec_select_topk_capped (the same under a per-group cap, amdrec/group_cap.py) and amdrec_select_topk_auction (order by
// expected revenue e = bid * pCTR with an optional per-user reserve, the cap, and generalised second prices,
// amdrec/auction.py): a key function, a winner write-out and two kernel shapes, templated on AUCTION and CAPPED.
// Order everywhere: (key desc, candidate slot asc), a NaN score last, a slot that is no candidate never.
// amdrec_select_topk_diverse (amdrec/diversity.py) builds on the same key function, cap helpers and winner write-out with a
// kernel of its own further down: the plain order gives it a pool, which it re-orders by similarity-discounted relevance.
// amdrec_select_topk_value / _value_auction (amdrec/value.py has the rule) are the frame's VALUE switch: the key is the
// weighted blend of every task's probability, the winner write-out reports it, and the auction solves its price from it.
// Their arguments ride behind SelectArgs in a struct of their own, so the instantiations without the switch keep their
// kernel arguments - and their instruction streams - as they were.
// amdrec_select_topk_sampled (amdrec/explore.py) is a kernel of its own as well: the plain order's prefix, then a
// Plackett-Luce draw by Gumbel-perturbed keys under the same cap, with each winner's conditional pick probability.
#include <optional>
#include <type_traits>
#include "../../include/amdrec.h"
#include "common.hpp"
#include "topk_utils.hpp"

namespace amdrec {

// everything the kernels read and write; the auction's and the cap's fields are looked at by their instantiations only
struct SelectArgs {
    const float* logits;
    long long ld;
    int n_tasks, rank_task;
    const long long* cand_ids;
    const long long* cand_pos;   // the candidates' stage-1 positions; nullable in the plain selection only
    int k_c, top_k;
    long long n_users;
    long long* out_ids;
    float* out_scores;
    int* out_slots;              // nullable
    // auction
    const float* bid_of;
    long long n_bid_rows;
    const float* reserve;        // [n_users] or nullptr
    float* out_ecpm;
    float* out_price;
    // cap
    const long long* group_of;
    long long n_group_rows;
    int cap;
};

// what the VALUE instantiations take on top: the users' blend weights and the winners' values
struct ValueArgs : SelectArgs {
    const float* weights;        // [n_users][n_tasks]
    float* out_values;           // [n_users][top_k]
};
template <bool VALUE>
using SelectArgsOf = std::conditional_t<VALUE, ValueArgs, SelectArgs>;

// one user's blend weights, wave-uniform (VALUE; the other instantiations carry an empty one)
struct BlendWeights {
    float w[AMDREC_MAX_TASKS];
};
struct NoWeights {};
template <bool VALUE>
using WeightsOf = std::conditional_t<VALUE, BlendWeights, NoWeights>;

// user u's weights through scalar registers: u is wave-uniform (n_users < 2^31 in the VALUE entries)
__device__ __forceinline__ BlendWeights load_weights(const ValueArgs& a, long long u) {
    const long long us = __builtin_amdgcn_readfirstlane((int)u);
    BlendWeights bw;
#pragma unroll
    for (int t = 0; t < AMDREC_MAX_TASKS; ++t) bw.w[t] = t < a.n_tasks ? a.weights[us * a.n_tasks + t] : 0.0f;
    return bw;
}
__device__ __forceinline__ NoWeights load_weights(const SelectArgs&, long long) { return NoWeights{}; }

// The blend of amdrec/value.py: the tasks in order, a term with weight 0 (either sign) skipped - its y is never looked at -,
// x_t = w_t * y_t, v = the first x_t, then v = v + x_t; every product and sum one rounded fp32 operation (boost_term /
// boost_add: this file is compiled with contraction on).  `skip`: a task left out whatever its weight (the price's q; -1:
// none).  Nothing left: +0.0.
__device__ __forceinline__ float value_sub(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ float blend(const BlendWeights& bw, const float (&y)[AMDREC_MAX_TASKS], int n_tasks, int skip) {
    float v = 0.0f;
    bool first = true;
#pragma unroll
    for (int t = 0; t < AMDREC_MAX_TASKS; ++t) {
        if (t < n_tasks && t != skip && bw.w[t] != 0.0f) {                     // (wave-uniform)
            const float x = boost_term(bw.w[t], y[t]);
            v = first ? x : boost_add(v, x);
            first = false;
        }
    }
    return v;
}

// the bid of corpus position pos >= 0: bid_of[pos], or 1.0 for a position beyond the array, which is never read
__device__ __forceinline__ float bid_at(const float* bid_of, long long n_rows, long long pos) {
    return pos < n_rows ? bid_of[pos] : 1.0f;
}

// a NaN score has no score image: its key carries 1 in the high word (below every real score image, above the empty key 0)
// and the slot in the low word
__device__ __forceinline__ bool key_is_nan(unsigned long long key) { return (key >> 32) == 1ull; }

// the eCPM a key contributes to the price of the rank before it: 0 for no candidate and for a NaN eCPM
__device__ __forceinline__ float key_floor_ecpm(unsigned long long key) {
    return (key != 0ull && !key_is_nan(key)) ? key_score(key) : 0.0f;
}

// the stage-1 position of candidate slot i of user u: -1 (no candidate) beyond k_c; 0 where the plain entry gave no cand_pos
__device__ __forceinline__ long long candidate_pos(const SelectArgs& a, long long u, int i) {
    if (i >= a.k_c) return -1ll;
    return a.cand_pos ? a.cand_pos[u * a.k_c + i] : 0ll;
}

// The key of candidate slot i of user u at position pos (candidate_pos).  0 = no candidate: a slot beyond k_c, or one the
// search never filled (negative position); it lies below every real key, NaN scores included, so it can only appear behind
// all real candidates, where it reads id -1 / probability 0 like the tail of a list shorter than top_k.  The score is the
// ranking task's logit, or (AUCTION) e = bid * sigmoid_prob(logit), dropped (key 0) iff a reserve is given and !(e >= rv),
// which drops a NaN e as well.  A NaN score ranks last.  VALUE: the score is the blend v of the tasks' probabilities under
// the user's weights bw (AUCTION: with e in the ranking task's place), the reserve compared with v; the logits of the tasks
// with a nonzero weight are independent loads and go out together with the bid's.
template <bool AUCTION, bool VALUE = false>
__device__ __forceinline__ unsigned long long candidate_key(const SelectArgsOf<VALUE>& a, long long u, int i, long long pos,
                                                            float rv, const WeightsOf<VALUE>& bw = {}) {
    if (pos < 0) return 0ull;
    float s;
    if constexpr (VALUE) {
        float y[AMDREC_MAX_TASKS];
#pragma unroll
        for (int t = 0; t < AMDREC_MAX_TASKS; ++t)
            y[t] = (t < a.n_tasks && bw.w[t] != 0.0f) ? a.logits[(long long)t * a.ld + u * a.k_c + i] : 0.0f;
        float b = 1.0f;
        if constexpr (AUCTION) b = bid_at(a.bid_of, a.n_bid_rows, pos);
#pragma unroll
        for (int t = 0; t < AMDREC_MAX_TASKS; ++t) {
            if (t < a.n_tasks && bw.w[t] != 0.0f) {                            // (wave-uniform)
                y[t] = sigmoid_prob(y[t]);
                if constexpr (AUCTION) y[t] = t == a.rank_task ? boost_term(b, y[t]) : y[t];
            }
        }
        s = blend(bw, y, a.n_tasks, -1);
        if constexpr (AUCTION)
            if (a.reserve && !(s >= rv)) return 0ull;
    } else {
        s = a.logits[(long long)a.rank_task * a.ld + u * a.k_c + i];
        if constexpr (AUCTION) {
            s = bid_at(a.bid_of, a.n_bid_rows, pos) * sigmoid_prob(s);
            if (a.reserve && !(s >= rv)) return 0ull;
        }
    }
    return (s == s) ? make_key(s, (uint32_t)i) : ((unsigned long long)(~(uint32_t)i) | (1ull << 32));
}

// Result slot r of user u: winner `key` (0: the unfilled tail, which reads id -1 / slot -1 / probability +0.0).  AUCTION:
// next_e = key_floor_ecpm of the candidate the selection would report at rank r + 1; price = min(bid, max(reserve, next_e) /
// p), 0 where that floor is 0, NaN for a NaN eCPM; NaN outputs are the canonical quiet NaN.  VALUE: next_e is the next
// rank's v in the same sense; the winner's v, and for the price its q (the blend without the ranking task) and d = w_r * p_r,
// are formed again from the probabilities written here, so that out_values is the blend of out_scores (and out_ecpm) bit for
// bit; price = min(bid, (floor - q) / d), 0 where !(floor - q > 0) or !(d > 0), NaN for a NaN v.
template <bool AUCTION, bool VALUE = false>
__device__ __forceinline__ void write_winner(const SelectArgsOf<VALUE>& a, unsigned long long key, long long u, int r,
                                             float next_e, const WeightsOf<VALUE>& bw = {}) {
    const bool valid = key != 0ull;
    const int slot = valid ? (int)key_pos(key) : -1;
    const long long o = u * a.top_k + r;
    a.out_ids[o] = valid ? a.cand_ids[u * a.k_c + slot] : -1;
    if (a.out_slots) a.out_slots[o] = slot;
    float p = 0.0f;
    if constexpr (VALUE) {
        float y[AMDREC_MAX_TASKS];
#pragma unroll
        for (int t = 0; t < AMDREC_MAX_TASKS; ++t) {
            y[t] = 0.0f;
            if (t < a.n_tasks) {
                const float x = valid ? a.logits[(long long)t * a.ld + u * a.k_c + slot] : -INFINITY;
                y[t] = sigmoid_prob(x);
                a.out_scores[((long long)t * a.n_users + u) * a.top_k + r] = y[t];
            }
        }
        float v = 0.0f, e = 0.0f, price = 0.0f;
        if (valid) {
            float b = 1.0f;
            if constexpr (AUCTION) {
                b = bid_at(a.bid_of, a.n_bid_rows, a.cand_pos[u * a.k_c + slot]);
#pragma unroll
                for (int t = 0; t < AMDREC_MAX_TASKS; ++t) {
                    p = t == a.rank_task ? y[t] : p;
                    y[t] = t == a.rank_task ? boost_term(b, y[t]) : y[t];
                    e = t == a.rank_task ? y[t] : e;
                }
            }
            v = blend(bw, y, a.n_tasks, -1);
            if constexpr (AUCTION) {
                if (v != v) {
                    price = __builtin_nanf("");
                } else {
                    float w_r = 0.0f;
#pragma unroll
                    for (int t = 0; t < AMDREC_MAX_TASKS; ++t) w_r = t == a.rank_task ? bw.w[t] : w_r;
                    const float q = blend(bw, y, a.n_tasks, a.rank_task);
                    const float d = boost_term(w_r, p);
                    float fl = next_e;
                    const float base = a.reserve ? a.reserve[u] : 0.0f;
                    fl = base > fl ? base : fl;
                    const float num = value_sub(fl, q);
                    if (num > 0.0f && d > 0.0f) {
                        const float g = num / d;
                        price = g < b ? g : b;
                    }
                }
                e = e != e ? __builtin_nanf("") : e;
            }
            v = v != v ? __builtin_nanf("") : v;
        }
        a.out_values[o] = v;
        if constexpr (AUCTION) {
            a.out_ecpm[o] = e;
            a.out_price[o] = price;
        }
        return;
    } else {
        for (int t = 0; t < a.n_tasks; ++t) {
            const float x = valid ? a.logits[(long long)t * a.ld + u * a.k_c + slot] : -INFINITY;
            const float s = sigmoid_prob(x);
            a.out_scores[((long long)t * a.n_users + u) * a.top_k + r] = s;
            if constexpr (AUCTION) p = t == a.rank_task ? s : p;
        }
    }
    if constexpr (AUCTION) {
        float e = 0.0f, price = 0.0f;
        if (valid) {
            if (key_is_nan(key)) {
                e = price = __builtin_nanf("");
            } else {
                e = key_score(key);
                const float b = bid_at(a.bid_of, a.n_bid_rows, a.cand_pos[u * a.k_c + slot]);
                float fl = next_e;
                if (a.reserve) {
                    const float rv = a.reserve[u];
                    fl = rv > fl ? rv : fl;
                }
                if (fl != 0.0f) {
                    const float q = fl / p;
                    price = q < b ? q : b;
                }
            }
        }
        a.out_ecpm[o] = e;
        a.out_price[o] = price;
    }
}

// Wave shape (top_k <= 32, k_c <= 64 * KPL: the serving path's top-10 of 500) without a sort: ONE WAVE per user holds the
// user's keys in registers (KPL per lane; the bid and group gathers through cand_pos go out with the logit loads) and extracts
// the maximum top_k times (wave max by lane exchange, the unique holder retires its key).  Keys are unique (the slot is part of
// the key), so the order is the sort's; a 512-key bitonic sort takes ~20 us of barriers whatever the batch, this takes ~3.
// CAPPED, the greedy rule in this form: a round's winner belongs to a group that is not saturated, so it is accepted; the wave
// then counts the accepted winners of that group (lanes 0 .. r hold them: a ballot and a popcount), and when the count reaches
// the cap every lane retires its remaining keys of the group - a saturated group never wins a later round.  AUCTION: one
// round more; lane top_k keeps the runner-up, found under the same cap bookkeeping as every winner, and a lane's price needs
// the next lane's eCPM, one __shfl.
// VALUE: the user's weights are loaded once, into scalar registers; the key build reads up to n_tasks logits per slot, the
// rounds are the same, and the price's next v takes next_e's route.
template <int KPL, bool AUCTION, bool CAPPED, bool VALUE = false>
__global__ __launch_bounds__(256) void select_wave_kernel(SelectArgsOf<VALUE> a) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.n_users) return;                                // wave-uniform
    float rv = 0.0f;
    if constexpr (AUCTION) rv = a.reserve ? a.reserve[u] : 0.0f;
    const WeightsOf<VALUE> bw = load_weights(a, u);
    unsigned long long key[KPL];
    long long grp[CAPPED ? KPL : 1];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i = lane + 64 * j;
        const long long pos = candidate_pos(a, u, i);
        key[j] = candidate_key<AUCTION, VALUE>(a, u, i, pos, rv, bw);
        if constexpr (CAPPED) grp[j] = group_at(a.group_of, a.n_group_rows, pos);
    }
    unsigned long long mine = 0ull;                            // lane r keeps the candidate of rank r (and its group): the
    long long mine_g = -1ll;                                   // dependent loads (candidate id, the tasks' logits) go out
    const int rounds = a.top_k + (AUCTION ? 1 : 0);            // together after the loop, one latency instead of one per
    for (int r = 0; r < rounds; ++r) {                         // rank (they were 10 of the kernel's 15 us)
        unsigned long long m = key[0];
#pragma unroll
        for (int j = 1; j < KPL; ++j) m = key[j] > m ? key[j] : m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, 64);
            m = other > m ? other : m;
        }
        // Wave-uniform: no candidate is left, the tail stays empty.  A round without a winner changes nothing in any variant, so
        // the exit is for speed alone, and the plain selection is faster without it: a lone wave pays 0.4 us for the ten tests
        // (1 x 500 -> 10: 8.5 us with it, 8.1 without), where the other two gain 0.6 us at 512 users (auction: 14.0 against 14.6).
        if constexpr (AUCTION || CAPPED)
            if (m == 0ull) break;
        long long g = -1ll;                                    // the winner's group, from its unique holder
        bool holder = false;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const bool hit = key[j] == m;
            if constexpr (CAPPED) {
                g = hit ? grp[j] : g;
                holder = holder || hit;
            }
            key[j] = hit ? 0ull : key[j];                      // retire the winner (0 = empty)
        }
        if (lane == r) mine = m;
        if constexpr (CAPPED) {
            g = __shfl(g, __ffsll((long long)__ballot(holder)) - 1, 64);
            if (lane == r) mine_g = g;
            if (g >= 0) {                                      // wave-uniform
                const int taken = __popcll(__ballot(lane <= r && mine != 0ull && mine_g == g));
                if (taken >= a.cap) {
#pragma unroll
                    for (int j = 0; j < KPL; ++j) key[j] = grp[j] == g ? 0ull : key[j];
                }
            }
        }
    }
    float next_e = 0.0f;
    if constexpr (AUCTION) next_e = __shfl(key_floor_ecpm(mine), (lane + 1) & 63, 64);     // (every lane takes part)
    if (lane < a.top_k) write_winner<AUCTION, VALUE>(a, mine, u, lane, next_e, bw);
}

// Sort shape (up to AMDREC_MAX_K candidates, any top_k): one workgroup of 512 per user, a bitonic sort of the keys in LDS.
// Without a cap the sorted index is the result slot, and the next entry's eCPM the price floor.  CAPPED: the sorted entries'
// groups next to them, keep = "fewer than cap earlier entries of my group" (below_group_cap), a block prefix sum over the
// keep flags (compact_slots), and the first top_k kept entries go out by compacted slot; AUCTION: compacted slot top_k is the
// runner-up, and the floor eCPMs pass through LDS by slot, so that slot r reads slot r + 1 behind one barrier.  Static LDS:
// 16 KB of keys (+ 16 KB of groups, CAPPED; + 8 KB of eCPMs, CAPPED auction).
constexpr int SORT_NT = 512;
constexpr int SORT_ROUNDS = AMDREC_MAX_K / SORT_NT;

template <bool AUCTION, bool CAPPED, bool VALUE = false>
__global__ __launch_bounds__(SORT_NT) void select_sort_kernel(SelectArgsOf<VALUE> a) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[AMDREC_MAX_K];
    __shared__ float floor_e[(AUCTION && CAPPED) ? AMDREC_MAX_K + 1 : 1];
    const long long u = blockIdx.x;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < a.k_c) P <<= 1;
    float rv = 0.0f;
    if constexpr (AUCTION) rv = a.reserve ? a.reserve[u] : 0.0f;
    const WeightsOf<VALUE> bw = load_weights(a, u);
    for (int i = tid; i < P; i += SORT_NT) keys[i] = candidate_key<AUCTION, VALUE>(a, u, i, candidate_pos(a, u, i), rv, bw);
    if constexpr (AUCTION && CAPPED)
        for (int i = tid; i <= a.top_k; i += SORT_NT) floor_e[i] = 0.0f;     // a rank nobody fills: no candidate, floor 0
    __syncthreads();
    bitonic_desc(keys, P);                                     // (ends behind a block barrier)
    if constexpr (!CAPPED) {
        for (int i = tid; i < a.top_k; i += SORT_NT)
            write_winner<AUCTION, VALUE>(a, i < P ? keys[i] : 0ull, u, i,
                                         (AUCTION && i + 1 < P) ? key_floor_ecpm(keys[i + 1]) : 0.0f, bw);
    } else {
        __shared__ __attribute__((aligned(16))) long long grp[AMDREC_MAX_K];
        __shared__ int wave_total[SORT_ROUNDS][SORT_NT / 64];
        unsigned long long key[SORT_ROUNDS];
        long long g[SORT_ROUNDS];
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r) {
            const int i = r * SORT_NT + tid;
            key[r] = i < P ? keys[i] : 0ull;
            g[r] = key[r] != 0ull ? group_at(a.group_of, a.n_group_rows, a.cand_pos[u * a.k_c + key_pos(key[r])]) : -1ll;
            if (i < P) grp[i] = g[r];
        }
        __syncthreads();
        bool keep[SORT_ROUNDS];
        int slot[SORT_ROUNDS];
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r)
            keep[r] = key[r] != 0ull && (g[r] < 0 || below_group_cap(grp, r * SORT_NT + tid, g[r], a.cap));
        const int kept = compact_slots<SORT_NT, SORT_ROUNDS>(keep, slot, wave_total);
        if constexpr (AUCTION) {
#pragma unroll
            for (int r = 0; r < SORT_ROUNDS; ++r)
                if (keep[r] && slot[r] <= a.top_k) floor_e[slot[r]] = key_floor_ecpm(key[r]);
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r)
            if (keep[r] && slot[r] < a.top_k)
                write_winner<AUCTION, VALUE>(a, key[r], u, slot[r], AUCTION ? floor_e[slot[r] + 1] : 0.0f, bw);
        for (int i = kept + tid; i < a.top_k; i += SORT_NT) write_winner<AUCTION, VALUE>(a, 0ull, u, i, 0.0f, bw);
    }
}

// ---- diversified selection (amdrec_select_topk_diverse, amdrec/diversity.py has the rule) ---------------------------------
// One workgroup of 512 per user, one dynamic LDS area used twice.  Phase A: the plain selection's keys, sorted (the cap's
// below_group_cap filter and compaction on the sorted entries, as in the sort shape above), the first `pool` accepted ones
// are the pool, in relevance order.  Phase B: the pool's rows are gathered over the sort's LDS (a position beyond the row
// array, and an empty pool slot, is a row of zeros: similarity 0 or NaN, neither of which discounts).  Phase C: top_k
// rounds.  Every wave finds the round's winner for itself from the members' (rel, m) in LDS - 64-bit keys (value image,
// ~pool index; a NaN value in the plane below, as candidate_key's) and a wave maximum, so the choice is workgroup-uniform
// without a barrier - then takes its share of the remaining members (DIV_RU at a time: their LDS reads are independent),
// dots them with the winner's row and writes the new m into the OTHER of two m arrays: a wave that is still reading this
// round's m is never overtaken, and one barrier per round suffices.  Every loop bound is top_k, pool or dim.
constexpr int DIV_NT = SORT_NT, DIV_NW = DIV_NT / 64, DIV_RU = 4, DIV_GU = 8;
constexpr int DIV_MAX_POOL = 128, DIV_MAX_FLOATS = 32768;
constexpr size_t DIV_SORT_BYTES = 3ull * AMDREC_MAX_K * 8;     // keys, the run sort's second array, the groups
constexpr size_t DIV_MAX_LDS = DIV_MAX_FLOATS * sizeof(float);
static_assert(DIV_SORT_BYTES <= DIV_MAX_LDS, "the sort phase fits the largest row area");

struct DiverseArgs {
    const float* rows;
    long long n_rows, ld_rows;
    int dim;
    float lam;
    int pool;
    float* out_values;
};

__device__ __forceinline__ float dot_acc(float x, float y, float acc) { return __builtin_fmaf(x, y, acc); }
__device__ __forceinline__ float dot_acc(const f32x4& x, const f32x4& y, float acc) {
    return __builtin_fmaf(x[3], y[3], __builtin_fmaf(x[2], y[2], __builtin_fmaf(x[1], y[1], __builtin_fmaf(x[0], y[0], acc))));
}

// One round's similarity update by one wave: members i = wv, wv + DIV_NW, ... of the pool that are still alive (bit i of
// alive_lo / alive_hi; the winner w is not) get m_next[i] = min(1, maxNum(m_cur[i], <row i, row w>)).  T = f32x4 (dim % 4 ==
// 0, n = dim / 4) or float (n = dim): rows of n elements of T in LDS.
template <class T>
__device__ __forceinline__ void diverse_update(const T* rowbuf, int n, int pool, int w, unsigned long long alive_lo,
                                               unsigned long long alive_hi, const float* m_cur, float* m_next) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T* rw = rowbuf + (long long)w * n;
    for (int i0 = wv; i0 < pool; i0 += DIV_NW * DIV_RU) {
        bool act[DIV_RU];
        const T* ri[DIV_RU];
        float acc[DIV_RU];
        bool any = false;
#pragma unroll
        for (int u = 0; u < DIV_RU; ++u) {
            const int i = i0 + DIV_NW * u;
            act[u] = i < pool && (((i < 64 ? alive_lo >> i : alive_hi >> (i - 64)) & 1ull) != 0ull);
            ri[u] = act[u] ? rowbuf + (long long)i * n : rw;
            acc[u] = 0.0f;
            any = any || act[u];
        }
        if (!any) continue;                                    // wave-uniform
        for (int c = lane; c < n; c += 64) {
            const T y = rw[c];
            T x[DIV_RU];
#pragma unroll
            for (int u = 0; u < DIV_RU; ++u) x[u] = ri[u][c];
#pragma unroll
            for (int u = 0; u < DIV_RU; ++u) acc[u] = dot_acc(x[u], y, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < DIV_RU; ++u)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o, 64);
#pragma unroll
        for (int u = 0; u < DIV_RU; ++u) {
            const int i = i0 + DIV_NW * u;
            // fmaxf is maxNum: a NaN similarity leaves m as it was; m itself is never NaN
            if (lane == 0 && act[u]) m_next[i] = fminf(1.0f, fmaxf(m_cur[i], acc[u]));
        }
    }
}

template <bool CAPPED>
__global__ __launch_bounds__(DIV_NT) void select_diverse_kernel(SelectArgs a, DiverseArgs d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char div_lds[];
    __shared__ unsigned long long pool_key[DIV_MAX_POOL];      // the pool in relevance order; 0: no member
    __shared__ long long pool_pos[DIV_MAX_POOL];               // the members' row positions; -1: a row of zeros
    __shared__ float pool_rel[DIV_MAX_POOL];
    __shared__ float pool_m[2][DIV_MAX_POOL];
    __shared__ int win_idx[DIV_MAX_POOL];                      // per rank: the winner's pool index, -1: none
    __shared__ float win_val[DIV_MAX_POOL];
    const long long u = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;

    // ---- phase A: the relevance order, the cap, the pool
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(div_lds);
    unsigned long long* other = keys + AMDREC_MAX_K;
    for (int i = tid; i < a.k_c; i += DIV_NT) keys[i] = candidate_key<false>(a, u, i, candidate_pos(a, u, i), 0.0f);
    if (tid < DIV_MAX_POOL) {
        pool_key[tid] = 0ull;
        win_idx[tid] = -1;
    }
    __syncthreads();
    // the all-LDS network up to 128 keys, the per-wave run sort beyond: 512 x 500 -> 10 at pool 64 takes 64.3 us with the
    // 500 keys through the network (a block barrier per stage) and an update in the last round, 59.7 through the runs
    // without that update (the two were changed together)
    const unsigned long long* sorted = sort_keys_desc<DIV_NT>(keys, other, a.k_c, 128);    // (ends behind a block barrier)
    if constexpr (!CAPPED) {
        if (tid < d.pool && tid < a.k_c) pool_key[tid] = sorted[tid];
    } else {
        long long* grp = reinterpret_cast<long long*>(other + AMDREC_MAX_K);
        __shared__ int wave_total[SORT_ROUNDS][DIV_NW];
        unsigned long long key[SORT_ROUNDS];
        long long g[SORT_ROUNDS];
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r) {
            const int i = r * DIV_NT + tid;
            key[r] = i < a.k_c ? sorted[i] : 0ull;
            g[r] = key[r] != 0ull ? group_at(a.group_of, a.n_group_rows, a.cand_pos[u * a.k_c + key_pos(key[r])]) : -1ll;
            if (i < a.k_c) grp[i] = g[r];
        }
        __syncthreads();
        bool keep[SORT_ROUNDS];
        int slot[SORT_ROUNDS];
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r)
            keep[r] = key[r] != 0ull && (g[r] < 0 || below_group_cap(grp, r * DIV_NT + tid, g[r], a.cap));
        compact_slots<DIV_NT, SORT_ROUNDS>(keep, slot, wave_total);
#pragma unroll
        for (int r = 0; r < SORT_ROUNDS; ++r)
            if (keep[r] && slot[r] < d.pool) pool_key[slot[r]] = key[r];
    }
    __syncthreads();                                           // the pool is complete, and the sort's LDS is free

    // ---- phase B: relevance, and the pool's rows into LDS
    float* rowbuf = reinterpret_cast<float*>(div_lds);
    if (tid < DIV_MAX_POOL) {
        // a member's row position, -1 for "a row of zeros": no member, or a position beyond the rows.  Through LDS, so that
        // the gather's loads depend on nothing but LDS and go out back to back (with the cand_pos load inside the gather loop
        // every row load waited for one: 512 x 500 -> 10 took 59.7 us against 58.4 at pool 64, 136.7 against 125.1 at 128)
        const unsigned long long pk = pool_key[tid];
        long long pos = -1ll;
        float rel = 0.0f;
        if (pk != 0ull) {
            pos = a.cand_pos[u * a.k_c + key_pos(pk)];
            rel = sigmoid_prob(a.logits[(long long)a.rank_task * a.ld + u * a.k_c + key_pos(pk)]);
        }
        pool_pos[tid] = pos < d.n_rows ? pos : -1ll;
        pool_rel[tid] = rel;
        pool_m[0][tid] = 0.0f;
        pool_m[1][tid] = 0.0f;
    }
    __syncthreads();
    const bool vec_lds = (d.dim & 3) == 0;
    const bool vec_glb = vec_lds && (d.ld_rows & 3) == 0 && (reinterpret_cast<uintptr_t>(d.rows) & 15) == 0;
    if (vec_glb) {
        const int d4 = d.dim >> 2, total = d.pool * d4;
        f32x4* rb4 = reinterpret_cast<f32x4*>(rowbuf);
        for (int e0 = tid; e0 < total; e0 += DIV_GU * DIV_NT) {
            f32x4 v[DIV_GU];
#pragma unroll
            for (int k = 0; k < DIV_GU; ++k) {
                const int e = e0 + k * DIV_NT;
                v[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (e < total) {
                    const int i = e / d4, c = e - i * d4;
                    const long long pos = pool_pos[i];
                    if (pos >= 0) v[k] = reinterpret_cast<const f32x4*>(d.rows + pos * d.ld_rows)[c];
                }
            }
#pragma unroll
            for (int k = 0; k < DIV_GU; ++k)
                if (e0 + k * DIV_NT < total) rb4[e0 + k * DIV_NT] = v[k];
        }
    } else {
        const int total = d.pool * d.dim;
        for (int e0 = tid; e0 < total; e0 += DIV_GU * DIV_NT) {
            float v[DIV_GU];
#pragma unroll
            for (int k = 0; k < DIV_GU; ++k) {
                const int e = e0 + k * DIV_NT;
                v[k] = 0.0f;
                if (e < total) {
                    const int i = e / d.dim, c = e - i * d.dim;
                    const long long pos = pool_pos[i];
                    if (pos >= 0) v[k] = d.rows[pos * d.ld_rows + c];
                }
            }
#pragma unroll
            for (int k = 0; k < DIV_GU; ++k)
                if (e0 + k * DIV_NT < total) rowbuf[e0 + k * DIV_NT] = v[k];
        }
    }
    __syncthreads();

    // ---- phase C: the greedy rounds.  Lane l of every wave looks after members l and l + 64
    const float rel0 = pool_rel[lane], rel1 = pool_rel[lane + 64];
    bool alive0 = lane < d.pool && pool_key[lane] != 0ull, alive1 = lane + 64 < d.pool && pool_key[lane + 64] != 0ull;
    for (int r = 0; r < a.top_k; ++r) {
        const float* m_cur = pool_m[r & 1];
        float* m_next = pool_m[(r + 1) & 1];
        const float m0 = m_cur[lane], m1 = m_cur[lane + 64];
        const float v0 = rel0 * __builtin_fmaf(-d.lam, m0, 1.0f), v1 = rel1 * __builtin_fmaf(-d.lam, m1, 1.0f);
        const unsigned long long k0 =
            !alive0 ? 0ull : (v0 == v0) ? make_key(v0, (uint32_t)lane) : ((unsigned long long)(~(uint32_t)lane) | (1ull << 32));
        const unsigned long long k1 =
            !alive1 ? 0ull : (v1 == v1) ? make_key(v1, (uint32_t)(lane + 64))
                                        : ((unsigned long long)(~(uint32_t)(lane + 64)) | (1ull << 32));
        unsigned long long best = k0 > k1 ? k0 : k1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long x = __shfl_xor(best, o, 64);
            best = x > best ? x : best;
        }
        if (best == 0ull) break;                               // workgroup-uniform: the pool is used up, the tail stays empty
        const int w = (int)key_pos(best);
        if (tid == (w & 63)) {                                 // (wave 0's lane that looks after w)
            win_idx[r] = w;
            win_val[r] = w < 64 ? v0 : v1;
        }
        if (r + 1 == a.top_k) break;                           // the last winner discounts nobody
        if (lane == (w & 63)) {
            if (w < 64) alive0 = false;
            else alive1 = false;
        }
        const unsigned long long alive_lo = __ballot(alive0), alive_hi = __ballot(alive1);
        // members that sit this round out keep their m: a taken one is never read again, and the winner's is in win_val
        // (lane l copies this wave's l-th member, one LDS instruction for all of them; lane 0 writes a member's updated m in a
        // later instruction, and a wave's LDS operations execute in order)
        {
            const int i = (tid >> 6) + DIV_NW * lane;
            if (i < d.pool) m_next[i] = m_cur[i];
        }
        if (vec_lds)
            diverse_update<f32x4>(reinterpret_cast<const f32x4*>(rowbuf), d.dim >> 2, d.pool, w, alive_lo, alive_hi, m_cur, m_next);
        else
            diverse_update<float>(rowbuf, d.dim, d.pool, w, alive_lo, alive_hi, m_cur, m_next);
        __syncthreads();
    }
    __syncthreads();                                           // (wave 0's win_idx / win_val)
    for (int r = tid; r < a.top_k; r += DIV_NT) {
        const int w = win_idx[r];
        write_winner<false>(a, w >= 0 ? pool_key[w] : 0ull, u, r, 0.0f);
        d.out_values[u * a.top_k + r] = w >= 0 ? win_val[r] : 0.0f;
    }
}

// ---- sampled selection (amdrec_select_topk_sampled, amdrec/explore.py has the rule) -----------------------------------------
// One workgroup of 512 per user, one dynamic LDS area: two key arrays for the sorts, the candidates' x = z / T and group keys
// by slot, and the group keys of the walk in walk order.  Phase A: the plain order P (candidate_key, sort_keys_desc), the cap's
// below_group_cap filter and compaction as in the sort shape above; the first g accepted entries (top_k for a user that is
// served greedily) are the prefix winners.  Phase B: the perturbed keys of the candidates not yet chosen, sorted, and the same
// filter over [the prefix winners, the sampled order]: an entry is accepted iff fewer than cap earlier entries of that walk
// share its group, which is the greedy rule with the prefix's counts carried over.  Phase C: the ranks behind the prefix in
// order; xs[i] holds x_i while candidate i is in R (finite logit, not chosen, its group not full) and a NaN otherwise; a rank
// costs two fixed-order block reductions in fp64 (the maximum, then the sum of exp(x - m)), after which the winner leaves R
// and, where its group is now full, so does its group.  Every loop bound is k_c, top_k or the block size.
constexpr int SMP_NT = SORT_NT, SMP_NW = SMP_NT / 64, SMP_MAX_TOP = 128;
constexpr size_t smp_lds_bytes(int n_al) { return (size_t)(5 * n_al + SMP_MAX_TOP) * 8; }
constexpr size_t SMP_MAX_LDS = smp_lds_bytes(AMDREC_MAX_K);

struct SampleArgs {
    const float* temperature;                // [n_users]
    const unsigned long long* seeds;         // [n_users]
    int greedy;
    float* out_propensity;                   // [n_users][top_k]
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the Gumbel noise of ad `id` under the user's mixed seed: U has 23 random bits and lies strictly inside (0, 1)
__device__ __forceinline__ double gumbel_of(unsigned long long mixed_seed, long long id) {
    const unsigned long long h = mix64(mixed_seed ^ (unsigned long long)id);
    const float U = ((float)(h >> 41) + 0.5f) * 1.1920928955078125e-07f;         // (exact: 24 significant bits)
    return -log(-log((double)U));
}

// The sampled order's key of a candidate with logit z at slot i: +inf logits first (high word above every score image), then
// the finite ones by k = (float)(x + G), then -inf logits (high word 2: below every score image, above the NaN plane), then
// NaN logits (candidate_key's NaN plane); the slot in the low word, so that each class is in slot order.
__device__ __forceinline__ unsigned long long sampled_key(float z, int i, double x, double G) {
    const unsigned long long low = (unsigned long long)(~(uint32_t)i);
    if (z != z) return low | (1ull << 32);
    if (z == INFINITY) return low | (0xffffffffull << 32);
    if (z == -INFINITY) return low | (2ull << 32);
    return make_key((float)(x + G), (uint32_t)i);
}

// fixed-order block reductions of one double per thread (SMP_NT threads, red[2][SMP_NW] in LDS: the two calls of a rank
// alternate between the halves, so that one barrier per call suffices)
template <bool MAX>
__device__ __forceinline__ double block_reduce_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(v, o, 64);
        v = MAX ? (other > v ? other : v) : v + other;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int w = 1; w < SMP_NW; ++w) r = MAX ? (red[w] > r ? red[w] : r) : r + red[w];
    return r;
}

// The cap's filter and compaction over the sorted keys `sorted`[0 .. k_c) that continue a walk of n_before accepted entries
// (their groups in grp_seq[0 .. n_before)): the accepted entries of walk rank < top_k go to win_key.  Returns the
// number accepted.  All threads call; begins and ends behind a block barrier.
__device__ __forceinline__ int sampled_walk(const unsigned long long* sorted, int k_c, int n_before, int limit, bool capped,
                                            int cap, const long long* grp_slot, long long* grp_seq,
                                            unsigned long long* win_key, int (*wave_total)[SMP_NW]) {
    const int tid = threadIdx.x;
    unsigned long long key[SORT_ROUNDS];
    long long g[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int i = r * SMP_NT + tid;
        key[r] = i < k_c ? sorted[i] : 0ull;
        g[r] = key[r] != 0ull ? grp_slot[key_pos(key[r])] : -1ll;
        if (i < k_c) grp_seq[n_before + i] = g[r];
    }
    __syncthreads();
    bool keep[SORT_ROUNDS];
    int slot[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r)
        keep[r] = key[r] != 0ull && (!capped || g[r] < 0 || below_group_cap(grp_seq, n_before + r * SMP_NT + tid, g[r], cap));
    const int kept = compact_slots<SMP_NT, SORT_ROUNDS>(keep, slot, wave_total);
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r)
        if (keep[r] && n_before + slot[r] < limit) win_key[n_before + slot[r]] = key[r];
    __syncthreads();
    return kept;
}

__global__ __launch_bounds__(SMP_NT) void select_sampled_kernel(SelectArgs a, SampleArgs s, int n_al) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smp_lds[];
    __shared__ unsigned long long win_key[SMP_MAX_TOP];        // per rank: the winner's key (its slot in the low word); 0: none
    __shared__ float win_prop[SMP_MAX_TOP];
    __shared__ int wave_total[SORT_ROUNDS][SMP_NW];
    __shared__ double red[2][SMP_NW];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smp_lds);
    unsigned long long* other = keys + n_al;
    double* xs = reinterpret_cast<double*>(other + n_al);
    long long* grp_slot = reinterpret_cast<long long*>(xs + n_al);
    long long* grp_seq = grp_slot + n_al;                      // [n_al + SMP_MAX_TOP]
    const long long u = blockIdx.x;
    const int tid = threadIdx.x;
    const bool capped = a.cap > 0;
    const float T = s.temperature[u];
    const bool explore = T > 0.0f;                             // (zero, negative, NaN: served greedily)
    const int g_u = explore ? s.greedy : a.top_k;
    const double nan64 = __builtin_nan("");

    if (tid < SMP_MAX_TOP) {
        win_key[tid] = 0ull;
        win_prop[tid] = 0.0f;
    }
    for (int i = tid; i < a.k_c; i += SMP_NT) {
        const long long pos = a.cand_pos[u * a.k_c + i];
        keys[i] = candidate_key<false>(a, u, i, pos, 0.0f);
        grp_slot[i] = capped ? group_at(a.group_of, a.n_group_rows, pos) : -1ll;
    }
    __syncthreads();

    // ---- phase A: the greedy prefix
    int n_pre = 0;
    if (g_u > 0) {                                             // workgroup-uniform
        const unsigned long long* sorted = sort_keys_desc<SMP_NT, 1>(keys, other, a.k_c, 128);    // (an instantiation of its own)
        const int kept = sampled_walk(sorted, a.k_c, 0, g_u, capped, a.cap, grp_slot, grp_seq, win_key, wave_total);
        n_pre = kept < g_u ? kept : g_u;
    }
    int n_win = n_pre;
    // (a prefix shorter than g: the plain walk has used every candidate the cap lets through, nothing is left to draw)
    if (n_pre == g_u && g_u < a.top_k) {                       // workgroup-uniform
        // ---- phase B: the perturbed keys of the candidates that are left, their order, the walk behind the prefix
        if (tid < n_pre) {
            const int w = (int)key_pos(win_key[tid]);
            grp_seq[tid] = grp_slot[w];
            win_prop[tid] = 1.0f;
        }
        const unsigned long long ms = mix64(s.seeds[u]);
        for (int i = tid; i < a.k_c; i += SMP_NT) {
            const long long pos = a.cand_pos[u * a.k_c + i];
            unsigned long long key = 0ull;
            double x = nan64;
            if (pos >= 0) {
                const float z = a.logits[(long long)a.rank_task * a.ld + u * a.k_c + i];
                const bool finite = z == z && z != INFINITY && z != -INFINITY;
                if (finite) x = (double)z / (double)T;
                key = sampled_key(z, i, x, finite ? gumbel_of(ms, a.cand_ids[u * a.k_c + i]) : 0.0);
            }
            keys[i] = key;
            xs[i] = x;
        }
        __syncthreads();
        if (tid < n_pre) {                                     // the prefix winners are chosen: out of the order and out of R
            const int w = (int)key_pos(win_key[tid]);
            keys[w] = 0ull;
            xs[w] = nan64;
        }
        __syncthreads();
        if (capped) {                                          // a group the prefix has filled is out of R
            for (int i = tid; i < a.k_c; i += SMP_NT) {
                const long long gi = grp_slot[i];
                if (gi < 0) continue;
                int seen = 0;
                for (int j = 0; j < n_pre; ++j) seen += grp_seq[j] == gi;
                if (seen >= a.cap) xs[i] = nan64;
            }
        }
        const unsigned long long* sorted = sort_keys_desc<SMP_NT, 1>(keys, other, a.k_c, 128);    // (an instantiation of its own)
        const int kept = sampled_walk(sorted, a.k_c, n_pre, a.top_k, capped, a.cap, grp_slot, grp_seq, win_key, wave_total);
        n_win = n_pre + kept < a.top_k ? n_pre + kept : a.top_k;

        // ---- phase C: the propensities of the ranks behind the prefix
        for (int j = n_pre; j < n_win; ++j) {
            const int w = (int)key_pos(win_key[j]);
            const double xw = xs[w];
            float p = 1.0f;                                    // a winner outside F was forced
            if (xw == xw) {                                    // workgroup-uniform
                double m = -INFINITY;
                for (int i = tid; i < a.k_c; i += SMP_NT) {
                    const double x = xs[i];
                    m = x > m ? x : m;                         // (a NaN never replaces m)
                }
                m = block_reduce_f64<true>(m, red[0]);
                double sum = 0.0;
                for (int i = tid; i < a.k_c; i += SMP_NT) {
                    const double x = xs[i];
                    if (x == x) sum += exp(x - m);
                }
                sum = block_reduce_f64<false>(sum, red[1]);
                p = (float)(exp(xw - m) / sum);
            }
            __syncthreads();                                   // every read of xs is done
            if (tid == 0) win_prop[j] = p;
            const long long gw = grp_slot[w];
            bool full = false;
            if (capped && gw >= 0) {                           // workgroup-uniform
                int seen = 0;
                for (int r = 0; r <= j; ++r) seen += grp_slot[key_pos(win_key[r])] == gw;
                full = seen >= a.cap;
            }
            for (int i = tid; i < a.k_c; i += SMP_NT)
                if (i == w || (full && grp_slot[i] == gw)) xs[i] = nan64;
            __syncthreads();
        }
    } else if (tid < n_pre) {
        win_prop[tid] = 1.0f;
    }
    __syncthreads();
    for (int r = tid; r < a.top_k; r += SMP_NT) {
        write_winner<false>(a, win_key[r], u, r, 0.0f);
        s.out_propensity[u * a.top_k + r] = win_prop[r];
    }
}

template <bool AUCTION, bool CAPPED, bool VALUE = false>
static void launch_select(const SelectArgsOf<VALUE>& a, hipStream_t st) {
    if (a.top_k <= 32 && a.k_c <= 512) {                       // one wave per user, no sort
        const dim3 grid((unsigned)((a.n_users + 3) / 4));
        if (a.k_c <= 128) hipLaunchKernelGGL((select_wave_kernel<2, AUCTION, CAPPED, VALUE>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((select_wave_kernel<8, AUCTION, CAPPED, VALUE>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((select_sort_kernel<AUCTION, CAPPED, VALUE>), dim3((unsigned)a.n_users), dim3(SORT_NT), 0, st, a);
    }
}

// What the entries share: the checks of the common arguments, the pick of shape and KPL, the launch.  auction: the
// order is by eCPM and out_ecpm / out_price are written; a.cap > 0: the cap applies.  prof_tag (nullptr: not timed) and
// prof_bytes are the launch's ProfScope.  A = ValueArgs: the VALUE instantiations (the entry has checked its own fields).
template <class A>
static int select_any(const A& a, bool auction, const char* prof_tag, double prof_bytes, void* stream) {
    constexpr bool VALUE = std::is_same_v<A, ValueArgs>;
    REQUIRE(a.n_tasks >= 1 && a.rank_task >= 0 && a.rank_task < a.n_tasks, "bad task index");
    REQUIRE(a.k_c >= 1 && a.k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(a.top_k >= 1 && a.top_k <= AMDREC_MAX_K, "top_k out of range");
    if (a.n_users <= 0) return AMDREC_OK;
    REQUIRE(a.logits && a.cand_ids && a.out_ids && a.out_scores && (!auction || (a.out_ecpm && a.out_price)), "null pointer");
    REQUIRE(a.ld >= a.n_users * a.k_c, "ld_logits too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::optional<ProfScope> prof;
    if (prof_tag) prof.emplace(prof_tag, 0.0, prof_bytes, st);
    const bool capped = a.cap > 0;
    if (auction && capped) launch_select<true, true, VALUE>(a, st);
    else if (auction) launch_select<true, false, VALUE>(a, st);
    else if (capped) launch_select<false, true, VALUE>(a, st);
    else launch_select<false, false, VALUE>(a, st);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

// The two value entries' own checks, before the first HIP call (select_any has the common ones): 0 = fine.
static int check_value_args(int n_tasks, int64_t n_users, const void* cand_pos, const void* weights, const void* group_of,
                            int64_t n_group_rows, int max_per_group, const void* out_values) {
    REQUIRE(n_tasks >= 1 && n_tasks <= AMDREC_MAX_TASKS, "n_tasks=%d out of range [1, %d]", n_tasks, AMDREC_MAX_TASKS);
    REQUIRE(max_per_group >= 0 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [0, %d] (0: no cap)",
            max_per_group, AMDREC_MAX_K);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (n_users > 0) {                                         // (no user: nothing to do, and no pointer is looked at)
        REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
        REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the value selection's candidates are decided by position)");
        REQUIRE(weights != nullptr, "null pointer: weights");
        REQUIRE(out_values != nullptr, "null pointer: out_values");
        REQUIRE(max_per_group == 0 || group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    }
    return AMDREC_OK;
}

}  // namespace amdrec

using namespace amdrec;

extern "C" int amdrec_select_topk(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                  const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                  int64_t* out_ids, float* out_scores, int32_t* out_slots, void* stream) {
    const SelectArgs a{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return select_any(a, false, nullptr, 0.0, stream);
}

extern "C" int amdrec_select_topk_capped(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                         const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                         int64_t* out_ids, float* out_scores, int32_t* out_slots, const int64_t* group_of,
                                         int64_t n_group_rows, int max_per_group, void* stream) {
    REQUIRE(max_per_group >= 1 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [1, %d]", max_per_group,
            AMDREC_MAX_K);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (n_users > 0) {                                         // (no user: nothing to do, and no pointer is looked at)
        REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
        REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the capped selection reads every candidate's group through it)");
        REQUIRE(group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    }
    const SelectArgs a{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       nullptr, 0, nullptr, nullptr, nullptr, (const long long*)group_of, (long long)n_group_rows, max_per_group};
    return select_any(a, false, "select_topk_capped", (double)n_users * k_c * 20.0, stream);
}

extern "C" int amdrec_select_topk_auction(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                          const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                          const float* bid_of, int64_t n_bid_rows, const float* reserve,
                                          const int64_t* group_of, int64_t n_group_rows, int max_per_group, int64_t* out_ids,
                                          float* out_scores, int32_t* out_slots, float* out_ecpm, float* out_price,
                                          void* stream) {
    REQUIRE(max_per_group >= 0 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [0, %d] (0: no cap)",
            max_per_group, AMDREC_MAX_K);
    REQUIRE(n_bid_rows >= 0, "n_bid_rows=%lld is negative", (long long)n_bid_rows);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    const bool capped = max_per_group > 0;
    if (n_users > 0) {                                         // (no user: nothing to do, and no pointer is looked at)
        REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
        REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the auction reads every candidate's bid through it)");
        REQUIRE(bid_of != nullptr || n_bid_rows == 0, "null pointer: bid_of");
        REQUIRE(!capped || group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    }
    const SelectArgs a{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       bid_of, (long long)n_bid_rows, reserve, out_ecpm, out_price,
                       capped ? (const long long*)group_of : nullptr, capped ? (long long)n_group_rows : 0, max_per_group};
    return select_any(a, true, "select_topk_auction", (double)n_users * k_c * (capped ? 24.0 : 16.0), stream);
}

extern "C" int amdrec_select_topk_value(const float* logits, int64_t ld_logits, int n_tasks, const int64_t* cand_ids,
                                        const int64_t* cand_pos, int64_t n_users, int k_c, int top_k, const float* weights,
                                        const int64_t* group_of, int64_t n_group_rows, int max_per_group, int64_t* out_ids,
                                        float* out_scores, int32_t* out_slots, float* out_values, void* stream) {
    if (const int rc = check_value_args(n_tasks, n_users, cand_pos, weights, group_of, n_group_rows, max_per_group, out_values))
        return rc;
    const bool capped = max_per_group > 0;
    const ValueArgs a{{logits, (long long)ld_logits, n_tasks, 0, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       nullptr, 0, nullptr, nullptr, nullptr,
                       capped ? (const long long*)group_of : nullptr, capped ? (long long)n_group_rows : 0, max_per_group},
                      weights, out_values};
    return select_any(a, false, "select_topk_value", (double)n_users * k_c * (16.0 + 4.0 * n_tasks + (capped ? 8.0 : 0.0)), stream);
}

extern "C" int amdrec_select_topk_value_auction(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                                const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c,
                                                int top_k, const float* weights, const float* bid_of, int64_t n_bid_rows,
                                                const float* reserve, const int64_t* group_of, int64_t n_group_rows,
                                                int max_per_group, int64_t* out_ids, float* out_scores, int32_t* out_slots,
                                                float* out_values, float* out_ecpm, float* out_price, void* stream) {
    if (const int rc = check_value_args(n_tasks, n_users, cand_pos, weights, group_of, n_group_rows, max_per_group, out_values))
        return rc;
    REQUIRE(n_bid_rows >= 0, "n_bid_rows=%lld is negative", (long long)n_bid_rows);
    if (n_users > 0) REQUIRE(bid_of != nullptr || n_bid_rows == 0, "null pointer: bid_of");
    const bool capped = max_per_group > 0;
    const ValueArgs a{{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       bid_of, (long long)n_bid_rows, reserve, out_ecpm, out_price,
                       capped ? (const long long*)group_of : nullptr, capped ? (long long)n_group_rows : 0, max_per_group},
                      weights, out_values};
    return select_any(a, true, "select_topk_value_auction",
                      (double)n_users * k_c * (16.0 + 4.0 * n_tasks + (capped ? 8.0 : 0.0)), stream);
}

extern "C" int amdrec_select_topk_sampled(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                          const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                          int64_t* out_ids, float* out_scores, int32_t* out_slots, const int64_t* group_of,
                                          int64_t n_group_rows, int max_per_group, const float* temperature,
                                          const uint64_t* seeds, int greedy, float* out_propensity, void* stream) {
    REQUIRE(n_tasks >= 1 && rank_task >= 0 && rank_task < n_tasks, "bad task index");
    REQUIRE(k_c >= 1 && k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(top_k >= 1 && top_k <= SMP_MAX_TOP, "top_k=%d out of range [1, %d] (one block reduction per sampled rank)", top_k,
            SMP_MAX_TOP);
    REQUIRE(greedy >= 0 && greedy <= top_k, "greedy=%d out of range [0, top_k=%d]", greedy, top_k);
    REQUIRE(max_per_group >= 0 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [0, %d] (0: no cap)",
            max_per_group, AMDREC_MAX_K);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (n_users <= 0) return AMDREC_OK;                        // (no user: nothing to do, and no pointer is looked at)
    const bool capped = max_per_group > 0;
    REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
    REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the sampled selection's candidates are decided by position)");
    REQUIRE(!capped || group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    REQUIRE(temperature != nullptr && seeds != nullptr && out_propensity != nullptr,
            "null pointer: temperature, seeds or out_propensity");
    REQUIRE(logits && cand_ids && out_ids && out_scores, "null pointer");
    REQUIRE((reinterpret_cast<uintptr_t>(seeds) & 7) == 0 && (reinterpret_cast<uintptr_t>(cand_ids) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(cand_pos) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_ids) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(group_of) & 7) == 0,
            "seeds, cand_ids, cand_pos, out_ids and group_of must be 8-byte aligned");
    REQUIRE(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(temperature) |
              reinterpret_cast<uintptr_t>(out_scores) | reinterpret_cast<uintptr_t>(out_propensity) |
              reinterpret_cast<uintptr_t>(out_slots)) & 3) == 0,
            "logits, temperature, out_scores, out_propensity and out_slots must be 4-byte aligned");
    REQUIRE(ld_logits >= n_users * k_c, "ld_logits too small");
    const SelectArgs a{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       nullptr, 0, nullptr, nullptr, nullptr,
                       capped ? (const long long*)group_of : nullptr, capped ? (long long)n_group_rows : 0, max_per_group};
    const SampleArgs s{temperature, (const unsigned long long*)seeds, greedy, out_propensity};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int n_al = k_c <= 1024 ? 1024 : AMDREC_MAX_K;        // (the run sort's second array holds 1024 or 2048 keys)
    static PerDeviceOnce attr;
    HIP_TRY(attr.set_dynamic_lds(reinterpret_cast<const void*>(select_sampled_kernel), SMP_MAX_LDS));
    ProfScope prof("select_topk_sampled", 0.0, (double)n_users * k_c * (capped ? 28.0 : 20.0), st);
    hipLaunchKernelGGL(select_sampled_kernel, dim3((unsigned)n_users), dim3(SMP_NT), smp_lds_bytes(n_al), st, a, s, n_al);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_select_topk_diverse(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                          const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                          const float* rows, int64_t n_rows, int64_t ld_rows, int dim, float lam, int pool,
                                          const int64_t* group_of, int64_t n_group_rows, int max_per_group, int64_t* out_ids,
                                          float* out_scores, int32_t* out_slots, float* out_values, void* stream) {
    REQUIRE(n_tasks >= 1 && rank_task >= 0 && rank_task < n_tasks, "bad task index");
    REQUIRE(k_c >= 1 && k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(pool >= 1 && pool <= DIV_MAX_POOL, "pool=%d out of range [1, %d]", pool, DIV_MAX_POOL);
    REQUIRE(top_k >= 1 && top_k <= pool, "top_k=%d out of range [1, pool=%d]", top_k, pool);
    REQUIRE(dim >= 1, "dim=%d must be >= 1", dim);
    REQUIRE(ld_rows >= dim, "ld_rows=%lld is smaller than dim=%d", (long long)ld_rows, dim);
    REQUIRE((long long)pool * dim <= DIV_MAX_FLOATS, "pool * dim = %lld exceeds %d (the pool's rows must fit one workgroup's LDS)",
            (long long)pool * dim, DIV_MAX_FLOATS);
    REQUIRE(lam >= 0.0f && lam <= 1.0f, "lam=%g must be finite and in [0, 1]", (double)lam);      // (refuses a NaN as well)
    REQUIRE(n_rows >= 0, "n_rows=%lld is negative", (long long)n_rows);
    REQUIRE(max_per_group >= 0 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [0, %d] (0: no cap)",
            max_per_group, AMDREC_MAX_K);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (n_users <= 0) return AMDREC_OK;                        // (no user: nothing to do, and no pointer is looked at)
    const bool capped = max_per_group > 0;
    REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
    REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the diversified selection reads every pool member's row through it)");
    REQUIRE(rows != nullptr || n_rows == 0, "null pointer: rows");
    REQUIRE(!capped || group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    REQUIRE(logits && cand_ids && out_ids && out_scores && out_values, "null pointer");
    REQUIRE(ld_logits >= n_users * k_c, "ld_logits too small");
    const SelectArgs a{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, (long long)n_users, (long long*)out_ids, out_scores, out_slots,
                       nullptr, 0, nullptr, nullptr, nullptr,
                       capped ? (const long long*)group_of : nullptr, capped ? (long long)n_group_rows : 0, max_per_group};
    const DiverseArgs d{rows, (long long)n_rows, (long long)ld_rows, dim, lam, pool, out_values};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t row_bytes = (size_t)pool * dim * sizeof(float);
    const size_t lds = row_bytes > DIV_SORT_BYTES ? row_bytes : DIV_SORT_BYTES;
    static PerDeviceOnce attr_plain, attr_capped;
    HIP_TRY((capped ? attr_capped : attr_plain)
                .set_dynamic_lds(capped ? reinterpret_cast<const void*>(select_diverse_kernel<true>)
                                        : reinterpret_cast<const void*>(select_diverse_kernel<false>), DIV_MAX_LDS));
    ProfScope prof("select_topk_diverse", 2.0 * n_users * top_k * pool * dim,
                   (double)n_users * (k_c * 20.0 + (double)row_bytes), st);
    if (capped) hipLaunchKernelGGL(select_diverse_kernel<true>, dim3((unsigned)n_users), dim3(DIV_NT), lds, st, a, d);
    else hipLaunchKernelGGL(select_diverse_kernel<false>, dim3((unsigned)n_users), dim3(DIV_NT), lds, st, a, d);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
