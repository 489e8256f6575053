// Stage-2 selection (inference.py:258-263, faiss_retrieval.py:355-358): per user, the top_k of its k_c ranked candidates, the
// winners' ad ids, candidate slots and sigmoid of every task's logit.  ONE frame serves amdrec_select_topk (order by the
// ranking task's LOGIT: sigmoid is monotone, and ranking on logits avoids the ties of saturated sigmoids),
// amdrec_select_topk_capped (the same under a per-group cap, amdrec/group_cap.py) and amdrec_select_topk_auction (order by
// expected revenue e = bid * pCTR with an optional per-user reserve, the cap, and generalised second prices,
// amdrec/auction.py): a key function, a winner write-out and two kernel shapes, templated on AUCTION and CAPPED.
// Order everywhere: (key desc, candidate slot asc), a NaN score last, a slot that is no candidate never.
#include <optional>
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
// which drops a NaN e as well.  A NaN score ranks last.
template <bool AUCTION>
__device__ __forceinline__ unsigned long long candidate_key(const SelectArgs& a, long long u, int i, long long pos, float rv) {
    if (pos < 0) return 0ull;
    float s = a.logits[(long long)a.rank_task * a.ld + u * a.k_c + i];
    if constexpr (AUCTION) {
        s = bid_at(a.bid_of, a.n_bid_rows, pos) * sigmoid_prob(s);
        if (a.reserve && !(s >= rv)) return 0ull;
    }
    return (s == s) ? make_key(s, (uint32_t)i) : ((unsigned long long)(~(uint32_t)i) | (1ull << 32));
}

// Result slot r of user u: winner `key` (0: the unfilled tail, which reads id -1 / slot -1 / probability +0.0).  AUCTION:
// next_e = key_floor_ecpm of the candidate the selection would report at rank r + 1; price = min(bid, max(reserve, next_e) /
// p), 0 where that floor is 0, NaN for a NaN eCPM; NaN outputs are the canonical quiet NaN.
template <bool AUCTION>
__device__ __forceinline__ void write_winner(const SelectArgs& a, unsigned long long key, long long u, int r, float next_e) {
    const bool valid = key != 0ull;
    const int slot = valid ? (int)key_pos(key) : -1;
    const long long o = u * a.top_k + r;
    a.out_ids[o] = valid ? a.cand_ids[u * a.k_c + slot] : -1;
    if (a.out_slots) a.out_slots[o] = slot;
    float p = 0.0f;
    for (int t = 0; t < a.n_tasks; ++t) {
        const float x = valid ? a.logits[(long long)t * a.ld + u * a.k_c + slot] : -INFINITY;
        const float s = sigmoid_prob(x);
        a.out_scores[((long long)t * a.n_users + u) * a.top_k + r] = s;
        if constexpr (AUCTION) p = t == a.rank_task ? s : p;
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
template <int KPL, bool AUCTION, bool CAPPED>
__global__ __launch_bounds__(256) void select_wave_kernel(SelectArgs a) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.n_users) return;                                // wave-uniform
    float rv = 0.0f;
    if constexpr (AUCTION) rv = a.reserve ? a.reserve[u] : 0.0f;
    unsigned long long key[KPL];
    long long grp[CAPPED ? KPL : 1];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i = lane + 64 * j;
        const long long pos = candidate_pos(a, u, i);
        key[j] = candidate_key<AUCTION>(a, u, i, pos, rv);
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
    if (lane < a.top_k) write_winner<AUCTION>(a, mine, u, lane, next_e);
}

// Sort shape (up to AMDREC_MAX_K candidates, any top_k): one workgroup of 512 per user, a bitonic sort of the keys in LDS.
// Without a cap the sorted index is the result slot, and the next entry's eCPM the price floor.  CAPPED: the sorted entries'
// groups next to them, keep = "fewer than cap earlier entries of my group" (below_group_cap), a block prefix sum over the
// keep flags (compact_slots), and the first top_k kept entries go out by compacted slot; AUCTION: compacted slot top_k is the
// runner-up, and the floor eCPMs pass through LDS by slot, so that slot r reads slot r + 1 behind one barrier.  Static LDS:
// 16 KB of keys (+ 16 KB of groups, CAPPED; + 8 KB of eCPMs, CAPPED auction).
constexpr int SORT_NT = 512;
constexpr int SORT_ROUNDS = AMDREC_MAX_K / SORT_NT;

template <bool AUCTION, bool CAPPED>
__global__ __launch_bounds__(SORT_NT) void select_sort_kernel(SelectArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[AMDREC_MAX_K];
    __shared__ float floor_e[(AUCTION && CAPPED) ? AMDREC_MAX_K + 1 : 1];
    const long long u = blockIdx.x;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < a.k_c) P <<= 1;
    float rv = 0.0f;
    if constexpr (AUCTION) rv = a.reserve ? a.reserve[u] : 0.0f;
    for (int i = tid; i < P; i += SORT_NT) keys[i] = candidate_key<AUCTION>(a, u, i, candidate_pos(a, u, i), rv);
    if constexpr (AUCTION && CAPPED)
        for (int i = tid; i <= a.top_k; i += SORT_NT) floor_e[i] = 0.0f;     // a rank nobody fills: no candidate, floor 0
    __syncthreads();
    bitonic_desc(keys, P);                                     // (ends behind a block barrier)
    if constexpr (!CAPPED) {
        for (int i = tid; i < a.top_k; i += SORT_NT)
            write_winner<AUCTION>(a, i < P ? keys[i] : 0ull, u, i, (AUCTION && i + 1 < P) ? key_floor_ecpm(keys[i + 1]) : 0.0f);
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
            if (keep[r] && slot[r] < a.top_k) write_winner<AUCTION>(a, key[r], u, slot[r], AUCTION ? floor_e[slot[r] + 1] : 0.0f);
        for (int i = kept + tid; i < a.top_k; i += SORT_NT) write_winner<AUCTION>(a, 0ull, u, i, 0.0f);
    }
}

template <bool AUCTION, bool CAPPED>
static void launch_select(const SelectArgs& a, hipStream_t st) {
    if (a.top_k <= 32 && a.k_c <= 512) {                       // one wave per user, no sort
        const dim3 grid((unsigned)((a.n_users + 3) / 4));
        if (a.k_c <= 128) hipLaunchKernelGGL((select_wave_kernel<2, AUCTION, CAPPED>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((select_wave_kernel<8, AUCTION, CAPPED>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((select_sort_kernel<AUCTION, CAPPED>), dim3((unsigned)a.n_users), dim3(SORT_NT), 0, st, a);
    }
}

// What the three entries share: the checks of the common arguments, the pick of shape and KPL, the launch.  auction: the
// order is by eCPM and out_ecpm / out_price are written; a.cap > 0: the cap applies.  prof_tag (nullptr: not timed) and
// prof_bytes are the launch's ProfScope.
static int select_any(const SelectArgs& a, bool auction, const char* prof_tag, double prof_bytes, void* stream) {
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
    if (auction && capped) launch_select<true, true>(a, st);
    else if (auction) launch_select<true, false>(a, st);
    else if (capped) launch_select<false, true>(a, st);
    else launch_select<false, false>(a, st);
    HIP_TRY(hipGetLastError());
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
