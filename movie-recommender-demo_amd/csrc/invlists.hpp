// What the inverted-list scans share (ivf.hip, ivfpq.hip): the search that takes a workgroup of a grouped scan to its list,
// and the two scoring rules every path that files a key must agree on.
#pragma once
#include "common.hpp"
#include "topk_utils.hpp"

namespace amdrec {

// NaN scores rank last: filed as -inf, behind every finite row (make_key's order has no place for a NaN)
__device__ __forceinline__ float rank_last(float sc) {
    if (!(sc == sc)) sc = -INFINITY;
    return sc;
}

// acc + x . y over four elements as ONE explicit fma chain, element 0 innermost.  The order is part of the contract: every
// path that scores a row in fp32 (the pair scan, the prefilter's quarter-wave re-score and its overflow re-score) must round
// identically, and a sum of products left to the compiler is contracted differently from one context to the next.
__device__ __forceinline__ float fma4(f32x4 x, f32x4 y, float acc) {
    return __builtin_fmaf(x[3], y[3], __builtin_fmaf(x[2], y[2], __builtin_fmaf(x[1], y[1], __builtin_fmaf(x[0], y[0], acc))));
}

// ---- per-request eligibility in the list scans (the *_eligible scan entries; amdrec.h has the contract) ----------------------
// The flat search's predicate (search.hip) over LIST-ORDER tags: list_tags[r] is the tag word of list-order row r (the
// index keeps list_tags = tags[row_pos] next to its lists), so a scan reads a row's tag where it reads the row's position,
// coalesced.  Every scan kernel and epilogue takes the predicate as a type: ListNoElig, an empty one, in the scans without
// masks - their kernels are the ones they were -, ListElig in the filtered instantiations.  A scan reads a tag once per row
// (tag) and a query's two words once per accumulator register (mask), then tests them per (query, row) element (ok).
struct ListNoElig {
    static constexpr bool on = false;
    struct Tag {};
    struct Mask {};
    __device__ __forceinline__ ListNoElig at(long long) const { return {}; }
    __device__ __forceinline__ Tag tag(long long) const { return {}; }
    __device__ __forceinline__ Mask mask(long long) const { return {}; }
    static __device__ __forceinline__ bool ok(Tag, Mask) { return true; }
};
struct ListElig {
    static constexpr bool on = true;
    const uint64_t* tags;    // [N], list order
    const uint64_t* all;     // [nq]
    const uint64_t* any;     // [nq]
    using Tag = uint64_t;
    struct Mask { uint64_t all, any; };
    __device__ __forceinline__ ListElig at(long long r0) const { return {tags + r0, all, any}; }   // rows counted from r0
    __device__ __forceinline__ Tag tag(long long row) const { return tags[row]; }
    // q < 0: no query in this accumulator register (nothing is loaded; the caller drops the register's elements)
    __device__ __forceinline__ Mask mask(long long q) const { return q >= 0 ? Mask{all[q], any[q]} : Mask{0ull, 0ull}; }
    static __device__ __forceinline__ bool ok(Tag t, Mask m) { return (t & m.all) == m.all && (m.any == 0ull || (t & m.any) != 0ull); }
};

// ---- stage-1 score boosts in the list scans (the *_boosted scan entries; amdrec.h has the contract) --------------------------
// The flat search's key s = ip + w_q * boost[r] (topk_utils.hpp: boost_term, boost_add - two rounded fp32 operations, never a
// fused multiply-add) over LIST-ORDER boosts: list_boosts[r] is the boost of list-order row r (the index keeps list_boosts =
// boosts[row_pos] next to its lists), read where the row's position and tag are read: one coalesced 4-byte load per row.  A
// query's weight is read where its threshold / pool offset is read.  The type sits next to the eligibility type: ListNoBoost,
// an empty one, in the scans without a boost - their kernels are the ones they were -, ListBoost in the *_boosted ones.
struct ListNoBoost {
    static constexpr bool on = false;
    struct Row {};
    struct Weight {};
    __device__ __forceinline__ ListNoBoost at(long long) const { return {}; }
    __device__ __forceinline__ Row row(long long) const { return {}; }
    __device__ __forceinline__ Weight w(long long) const { return {}; }
    struct Term {};
    static __device__ __forceinline__ Term term(Weight, Row) { return {}; }
    static __device__ __forceinline__ float add(float ip, Term) { return ip; }
    static __device__ __forceinline__ float apply(float ip, Weight, Row) { return ip; }
};
struct ListBoost {
    static constexpr bool on = true;
    const float* boosts;     // [N], list order
    const float* weight;     // [nq]
    using Row = float;
    using Weight = float;
    __device__ __forceinline__ ListBoost at(long long r0) const { return {boosts + r0, weight}; }   // rows counted from r0
    __device__ __forceinline__ Row row(long long r) const { return boosts[r]; }
    // q < 0: no query in this accumulator register (nothing is loaded; the caller drops the register's elements)
    __device__ __forceinline__ Weight w(long long q) const { return q >= 0 ? weight[q] : 0.f; }
    using Term = float;      // t = w_q * boost[r], one rounded multiply
    static __device__ __forceinline__ Term term(Weight w, Row b) { return boost_term(w, b); }
    static __device__ __forceinline__ float add(float ip, Term t) { return boost_add(ip, t); }   // one rounded add
    static __device__ __forceinline__ float apply(float ip, Weight w, Row b) { return add(ip, term(w, b)); }
};

// A scan kernel's trailing arguments -> its two types: the eligibility pointers first (ListNoElig: none), then the boost's
// (ListNoBoost: none).  One overload per combination, picked by the argument types.
template <class EL, class BO>
struct ListPreds {
    [[no_unique_address]] EL el;
    [[no_unique_address]] BO bo;
};
__device__ __forceinline__ ListPreds<ListNoElig, ListNoBoost> list_preds() { return {}; }
__device__ __forceinline__ ListPreds<ListElig, ListNoBoost> list_preds(const uint64_t* tags, const uint64_t* all, const uint64_t* any) {
    return {{tags, all, any}, {}};
}
__device__ __forceinline__ ListPreds<ListNoElig, ListBoost> list_preds(const float* boosts, const float* weight) {
    return {{}, {boosts, weight}};
}
__device__ __forceinline__ ListPreds<ListElig, ListBoost> list_preds(const uint64_t* tags, const uint64_t* all, const uint64_t* any,
                                                                     const float* boosts, const float* weight) {
    return {{tags, all, any}, {boosts, weight}};
}

// The list of query tile y of amdrec_ivf_group (blockIdx.y of a grouped scan): l with qt_prefix[l] <= y < qt_prefix[l+1];
// the caller has returned for y >= qt_prefix[nlist].  The kernels keep the rest of the frame (list_off / group_off / p0 and
// the second early return) themselves: moved in here as well, in any form tried, it compiled to another instruction stream.
// A binary search is log2(nlist) DEPENDENT global loads - 12 round trips at nlist 4096, ~10 us in front of a workgroup
// whose MFMAs take 14 (the per-rank shape of an 8-way sharded 10M index: 305-row lists, tools/shard_step_probe.py --index
// ivf) - so every wave searches 64-ary: the lanes probe 64 evenly spaced entries of the bracket at once, a ballot counts
// those at or below y (the prefix is non-decreasing): two or three round trips for any nlist up to 2^18.
__device__ __forceinline__ int tile_list(long long y, const long long* qt_prefix, int nlist) {
    int lo = 0, hi = nlist;
    const int lane = threadIdx.x & 63;
    while (hi - lo > 1) {                                                  // wave-uniform
        const int step = (hi - lo + 63) >> 6;
        const int idx = lo + lane * step;
        const bool le = idx < hi && qt_prefix[idx] <= y;                   // lane 0 probes lo itself: always true
        const int c = __builtin_popcountll(__ballot(le));                  // >= 1
        const int nlo = lo + (c - 1) * step;
        hi = nlo + step < hi ? nlo + step : hi;
        lo = nlo;
    }
    return lo;
}

}  // namespace amdrec
