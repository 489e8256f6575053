// Auction ranking (amdrec_select_topk_auction): the stage-2 selection by expected revenue e = bid * pCTR, with an optional
// per-user reserve, the per-group cap and generalised second prices.  amdrec/auction.py has the rule; the two kernels mirror
// the capped selection of rows.hip (one wave per user for the serving shape, an LDS sort for the general one) and run one
// rank further: the candidate behind the last winner sets the last winner's price.
#include "../../include/amdrec.h"
#include "common.hpp"
#include "topk_utils.hpp"

namespace amdrec {

// what both kernels need beyond the keys: everything a winner's outputs are read from and written to
struct AuctionIO {
    const float* logits;
    long long ld;
    int n_tasks, rank_task;
    const long long* cand_ids;
    const long long* cand_pos;
    int k_c, top_k;
    const float* bid_of;
    long long n_bid_rows;
    const float* reserve;        // [n_users] or nullptr
    long long* out_ids;
    float* out_scores;
    int* out_slots;              // nullable
    float* out_ecpm;
    float* out_price;
    long long n_users;
};

// the bid of corpus position pos >= 0: bid_of[pos], or 1.0 for a position beyond the array, which is never read
__device__ __forceinline__ float bid_at(const float* bid_of, long long n_rows, long long pos) {
    return pos < n_rows ? bid_of[pos] : 1.0f;
}

// a NaN eCPM has no score image: its key carries 1 in the high word (below every real eCPM, which is >= +0.0, above the
// empty key 0) and the slot in the low word, as the CTR selection builds it for a NaN logit
__device__ __forceinline__ bool key_is_nan(unsigned long long key) { return (key >> 32) == 1ull; }

// The key of a candidate with logit v and bid b (the caller has checked position >= 0): e = b * sigmoid_prob(v); dropped
// (key 0) iff a reserve is given and !(e >= reserve), which drops a NaN e as well.
__device__ __forceinline__ unsigned long long auction_key(float v, float b, int slot, bool has_reserve, float rv) {
    const float e = b * sigmoid_prob(v);
    if (has_reserve && !(e >= rv)) return 0ull;
    return (e == e) ? make_key(e, (uint32_t)slot) : ((unsigned long long)(~(uint32_t)slot) | (1ull << 32));
}

// the eCPM a key contributes to the price of the rank before it: 0 for no candidate and for a NaN eCPM
__device__ __forceinline__ float key_floor_ecpm(unsigned long long key) {
    return (key != 0ull && !key_is_nan(key)) ? key_score(key) : 0.0f;
}

// Result slot r of user u: winner `key` (0: the unfilled tail), next_e = key_floor_ecpm of the candidate the selection would
// report at rank r + 1.  price = min(bid, max(reserve, next_e) / p), 0 where that floor is 0, NaN for a NaN eCPM; NaN outputs
// are the canonical quiet NaN.
__device__ __forceinline__ void write_auction_winner(const AuctionIO& io, unsigned long long key, long long u, int r,
                                                     float next_e) {
    const bool valid = key != 0ull;
    const int slot = valid ? (int)key_pos(key) : -1;
    const long long o = u * io.top_k + r;
    io.out_ids[o] = valid ? io.cand_ids[u * io.k_c + slot] : -1;
    if (io.out_slots) io.out_slots[o] = slot;
    float p = 0.0f;
    for (int t = 0; t < io.n_tasks; ++t) {
        const float x = valid ? io.logits[(long long)t * io.ld + u * io.k_c + slot] : -INFINITY;
        const float s = sigmoid_prob(x);
        io.out_scores[((long long)t * io.n_users + u) * io.top_k + r] = s;
        p = t == io.rank_task ? s : p;
    }
    float e = 0.0f, price = 0.0f;
    if (valid) {
        if (key_is_nan(key)) {
            e = price = __builtin_nanf("");
        } else {
            e = key_score(key);
            const float b = bid_at(io.bid_of, io.n_bid_rows, io.cand_pos[u * io.k_c + slot]);
            float fl = next_e;
            if (io.reserve) {
                const float rv = io.reserve[u];
                fl = rv > fl ? rv : fl;
            }
            if (fl != 0.0f) {
                const float q = fl / p;
                price = q < b ? q : b;
            }
        }
    }
    io.out_ecpm[o] = e;
    io.out_price[o] = price;
}

// Serving shape (top_k <= 32, k_c <= 64 * KPL): one wave per user, the keys in registers.  The bid gather through cand_pos goes
// out with the logit loads (and the group gather, CAPPED only).  top_k + 1 extraction rounds: lane r keeps winner r, lane top_k
// the runner-up, which is found under the same cap bookkeeping as every winner; a lane's price needs the next lane's eCPM, one
// __shfl.
template <int KPL, bool CAPPED>
__global__ __launch_bounds__(256) void auction_small_kernel(AuctionIO io, const long long* group_of, long long n_group_rows,
                                                            int cap) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= io.n_users) return;                               // wave-uniform
    const float* lr = io.logits + (long long)io.rank_task * io.ld + u * io.k_c;
    const long long* pu = io.cand_pos + u * io.k_c;
    const bool has_reserve = io.reserve != nullptr;
    const float rv = has_reserve ? io.reserve[u] : 0.0f;
    unsigned long long key[KPL];
    long long grp[CAPPED ? KPL : 1];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i = lane + 64 * j;
        const long long pos = i < io.k_c ? pu[i] : -1ll;
        unsigned long long kk = 0ull;
        if (pos >= 0) kk = auction_key(lr[i], bid_at(io.bid_of, io.n_bid_rows, pos), i, has_reserve, rv);
        key[j] = kk;
        if constexpr (CAPPED) grp[j] = group_at(group_of, n_group_rows, pos);
    }
    unsigned long long mine = 0ull;                            // lane r keeps the candidate of rank r and its group
    long long mine_g = -1ll;
    for (int r = 0; r <= io.top_k; ++r) {
        unsigned long long m = key[0];
#pragma unroll
        for (int j = 1; j < KPL; ++j) m = key[j] > m ? key[j] : m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, 64);
            m = other > m ? other : m;
        }
        if (m == 0ull) break;                                  // wave-uniform: no candidate is left, the tail stays empty
        long long g = -1ll;                                    // the winner's group, from its unique holder
        bool holder = false;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const bool hit = key[j] == m;
            if constexpr (CAPPED) g = hit ? grp[j] : g;
            holder = holder || hit;
            key[j] = hit ? 0ull : key[j];                      // retire the winner (0 = empty)
        }
        if constexpr (CAPPED) {
            const int src = __ffsll((long long)__ballot(holder)) - 1;
            g = __shfl(g, src, 64);
        }
        if (lane == r) { mine = m; mine_g = g; }
        if constexpr (CAPPED) {
            if (g >= 0) {                                      // wave-uniform
                const int taken = __popcll(__ballot(lane <= r && mine != 0ull && mine_g == g));
                if (taken >= cap) {
#pragma unroll
                    for (int j = 0; j < KPL; ++j) key[j] = grp[j] == g ? 0ull : key[j];
                }
            }
        }
    }
    const float next_e = __shfl(key_floor_ecpm(mine), (lane + 1) & 63, 64);     // (every lane takes part)
    if (lane < io.top_k) write_auction_winner(io, mine, u, lane, next_e);
}

// General shape (up to AMDREC_MAX_K candidates, any top_k): one workgroup of 512 per user.  LDS bitonic sort of the keys, the
// sorted entries' groups next to them (CAPPED), keep = below_group_cap, compact_slots.  The entries of compacted slot <= top_k
// matter: slot top_k is the runner-up.  Their floor eCPMs pass through LDS by slot, so that slot r reads slot r + 1 behind one
// barrier.  Static LDS: 16 KB of keys + 16 KB of groups (CAPPED) + 8 KB of eCPMs.
constexpr int AUC_NT = 512;
constexpr int AUC_ROUNDS = AMDREC_MAX_K / AUC_NT;

template <bool CAPPED>
__global__ __launch_bounds__(AUC_NT) void auction_kernel(AuctionIO io, const long long* group_of, long long n_group_rows,
                                                         int cap) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[AMDREC_MAX_K];
    __shared__ __attribute__((aligned(16))) long long grp[CAPPED ? AMDREC_MAX_K : 1];
    __shared__ float floor_e[AMDREC_MAX_K + 1];
    __shared__ int wave_total[AUC_ROUNDS][AUC_NT / 64];
    const long long u = blockIdx.x;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < io.k_c) P <<= 1;
    const float* lr = io.logits + (long long)io.rank_task * io.ld + u * io.k_c;
    const long long* pu = io.cand_pos + u * io.k_c;
    const bool has_reserve = io.reserve != nullptr;
    const float rv = has_reserve ? io.reserve[u] : 0.0f;
    for (int i = tid; i < P; i += AUC_NT) {
        const long long pos = i < io.k_c ? pu[i] : -1ll;
        keys[i] = pos >= 0 ? auction_key(lr[i], bid_at(io.bid_of, io.n_bid_rows, pos), i, has_reserve, rv) : 0ull;
    }
    for (int i = tid; i <= io.top_k; i += AUC_NT) floor_e[i] = 0.0f;     // a rank nobody fills: no candidate, floor 0
    __syncthreads();
    bitonic_desc(keys, P);                                     // (ends behind a block barrier)
    unsigned long long key[AUC_ROUNDS];
    long long g[AUC_ROUNDS];
#pragma unroll
    for (int r = 0; r < AUC_ROUNDS; ++r) {
        const int i = r * AUC_NT + tid;
        key[r] = i < P ? keys[i] : 0ull;
        g[r] = -1ll;
        if constexpr (CAPPED) {
            if (key[r] != 0ull) g[r] = group_at(group_of, n_group_rows, pu[key_pos(key[r])]);
            if (i < P) grp[i] = g[r];
        }
    }
    if constexpr (CAPPED) __syncthreads();
    bool keep[AUC_ROUNDS];
    int slot[AUC_ROUNDS];
#pragma unroll
    for (int r = 0; r < AUC_ROUNDS; ++r) {
        keep[r] = key[r] != 0ull;
        if constexpr (CAPPED) keep[r] = keep[r] && (g[r] < 0 || below_group_cap(grp, r * AUC_NT + tid, g[r], cap));
    }
    const int kept = compact_slots<AUC_NT, AUC_ROUNDS>(keep, slot, wave_total);
#pragma unroll
    for (int r = 0; r < AUC_ROUNDS; ++r)
        if (keep[r] && slot[r] <= io.top_k) floor_e[slot[r]] = key_floor_ecpm(key[r]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < AUC_ROUNDS; ++r)
        if (keep[r] && slot[r] < io.top_k) write_auction_winner(io, key[r], u, slot[r], floor_e[slot[r] + 1]);
    for (int i = kept + tid; i < io.top_k; i += AUC_NT) write_auction_winner(io, 0ull, u, i, 0.0f);
}

template <bool CAPPED>
static void launch_auction(const AuctionIO& io, const long long* group_of, long long n_group_rows, int cap, hipStream_t st) {
    if (io.top_k <= 32 && io.k_c <= 512) {                     // one wave per user, no sort
        const dim3 grid((unsigned)((io.n_users + 3) / 4));
        if (io.k_c <= 128)
            hipLaunchKernelGGL((auction_small_kernel<2, CAPPED>), grid, dim3(256), 0, st, io, group_of, n_group_rows, cap);
        else
            hipLaunchKernelGGL((auction_small_kernel<8, CAPPED>), grid, dim3(256), 0, st, io, group_of, n_group_rows, cap);
    } else {
        hipLaunchKernelGGL((auction_kernel<CAPPED>), dim3((unsigned)io.n_users), dim3(AUC_NT), 0, st, io, group_of,
                           n_group_rows, cap);
    }
}

}  // namespace amdrec

using namespace amdrec;

extern "C" int amdrec_select_topk_auction(const float* logits, int64_t ld_logits, int n_tasks, int rank_task,
                                          const int64_t* cand_ids, const int64_t* cand_pos, int64_t n_users, int k_c, int top_k,
                                          const float* bid_of, int64_t n_bid_rows, const float* reserve,
                                          const int64_t* group_of, int64_t n_group_rows, int max_per_group, int64_t* out_ids,
                                          float* out_scores, int32_t* out_slots, float* out_ecpm, float* out_price,
                                          void* stream) {
    REQUIRE(n_tasks >= 1 && rank_task >= 0 && rank_task < n_tasks, "bad task index");
    REQUIRE(k_c >= 1 && k_c <= AMDREC_MAX_K, "candidates per user must be in [1,%d]", AMDREC_MAX_K);
    REQUIRE(top_k >= 1 && top_k <= AMDREC_MAX_K, "top_k out of range");
    REQUIRE(max_per_group >= 0 && max_per_group <= AMDREC_MAX_K, "max_per_group=%d out of range [0, %d] (0: no cap)",
            max_per_group, AMDREC_MAX_K);
    REQUIRE(n_bid_rows >= 0, "n_bid_rows=%lld is negative", (long long)n_bid_rows);
    REQUIRE(n_group_rows >= 0, "n_group_rows=%lld is negative", (long long)n_group_rows);
    if (n_users <= 0) return AMDREC_OK;
    REQUIRE(n_users <= 2147483647ll, "n_users=%lld: at most 2^31 - 1 users per call", (long long)n_users);
    REQUIRE(logits && cand_ids && out_ids && out_scores && out_ecpm && out_price, "null pointer");
    REQUIRE(cand_pos != nullptr, "null pointer: cand_pos (the auction reads every candidate's bid through it)");
    REQUIRE(bid_of != nullptr || n_bid_rows == 0, "null pointer: bid_of");
    const bool capped = max_per_group > 0;
    REQUIRE(!capped || group_of != nullptr || n_group_rows == 0, "null pointer: group_of");
    REQUIRE(ld_logits >= n_users * k_c, "ld_logits too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("select_topk_auction", 0.0, (double)n_users * k_c * (capped ? 24.0 : 16.0), st);
    const AuctionIO io{logits, (long long)ld_logits, n_tasks, rank_task, (const long long*)cand_ids, (const long long*)cand_pos,
                       k_c, top_k, bid_of, (long long)n_bid_rows, reserve, (long long*)out_ids, out_scores, out_slots, out_ecpm,
                       out_price, (long long)n_users};
    if (capped) launch_auction<true>(io, (const long long*)group_of, (long long)n_group_rows, max_per_group, st);
    else launch_auction<false>(io, nullptr, 0, 0, st);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}
