// Live corpus (behind FAISSIndex.remove_ids and AdRecommenderInference.remove_ads / add_ads): removing rows is an
// order-preserving compaction of every per-row array, done in two steps that never recompute a row.
//   remove_plan : which rows stay.  Three plain launches, none of which waits for another workgroup:
//            flag   one thread per row, 1024 rows per workgroup: a binary search of the row's key (its id, or its position)
//                   in the ascending removal list decides whether it stays; the flag goes to the workspace and the block's
//                   survivors are counted (wave ballot + popcount, wave totals through LDS);
//            scan   ONE workgroup turns the block counts into exclusive offsets, 1024 counts per turn of its loop with the
//                   running total carried along, and writes n_kept;
//            write  the flag kernel's frame again: a survivor's slot is its block's offset + the survivors before it in
//                   the block; kept[slot] = the row's old position.
//   rows_gather : dst[j] = src[pos[j]] byte for byte, any row size.  A group of L lanes (a power of two, at most 256) owns a
//            row and walks it in units of the widest access (16 / 8 / 4 / 1 bytes) that the pointers, pitches and row size
//            allow; one row per group and turn of its loop.  A position outside [0, n_src) gives a row of zeros, never a read.
#include "common.hpp"
#include "../../include/amdrec.h"

namespace amdrec {

constexpr int RP_NT = 1024;                       // rows (= threads) per workgroup of the plan kernels
constexpr int RP_WAVES = RP_NT / 64;
constexpr int RG_NT = 256;                        // threads per workgroup of the gather
constexpr int RG_MAX_BLOCKS = 1 << 20;            // grid cap: beyond it the groups stride over the rows.  (A cap of 16384
                                                  // with four rows in flight per group measured 15-30 % slower on 1 KB / 4 KB rows:
                                                  // the gather wants every row's loads in the air at once, not a loop per lane)

struct RemovePlanWs : Carver {                    // ONE layout for the workspace query and the entry
    unsigned char* flags;                         // [n] 1 = the row stays
    unsigned* counts;                             // [blocks] survivors per block, then their exclusive prefix sums
    RemovePlanWs(void* ws, long long n) : Carver(ws) {
        flags = take<unsigned char>((size_t)n);
        counts = take<unsigned>((size_t)((n + RP_NT - 1) / RP_NT));
    }
};

__global__ __launch_bounds__(RP_NT) void remove_flag_kernel(const long long* ids, long long n, const long long* remove,
                                                            long long n_remove, unsigned char* flags, unsigned* counts) {
    __shared__ int wave_total[RP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long row = (long long)blockIdx.x * RP_NT + tid;
    bool keep = false;
    if (row < n) {
        const long long key = ids ? ids[row] : row;
        long long lo = 0, hi = n_remove;          // first index whose entry is >= key (ascending list)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (remove[mid] < key) lo = mid + 1; else hi = mid;
        }
        keep = !(lo < n_remove && remove[lo] == key);
        flags[row] = keep ? 1 : 0;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_total[w] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int x = 0; x < RP_WAVES; ++x) s += wave_total[x];
        counts[blockIdx.x] = (unsigned)s;
    }
}

__global__ __launch_bounds__(RP_NT) void remove_scan_kernel(unsigned* counts, int blocks, long long* n_kept) {
    __shared__ unsigned wave_sum[RP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned carry = 0;                           // survivors of the turns before this one (at most 2^31 - 1 in all)
    for (int base = 0; base < blocks; base += RP_NT) {
        const int i = base + tid;
        const unsigned c = i < blocks ? counts[i] : 0u;
        unsigned x = c;                           // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[w] = x;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < RP_WAVES; ++k) {
            const unsigned t = wave_sum[k];
            if (k < w) before += t;
            total += t;
        }
        if (i < blocks) counts[i] = carry + before + x - c;
        carry += total;
        __syncthreads();                          // wave_sum is written again in the next turn
    }
    if (tid == 0) *n_kept = (long long)carry;
}

__global__ __launch_bounds__(RP_NT) void remove_write_kernel(const unsigned char* flags, long long n, const unsigned* offsets,
                                                             long long* kept) {
    __shared__ int wave_total[RP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long row = (long long)blockIdx.x * RP_NT + tid;
    const bool keep = row < n && flags[row] != 0;
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[w] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    long long slot = (long long)offsets[blockIdx.x] + before;
#pragma unroll
    for (int x = 0; x < RP_WAVES; ++x)
        if (x < w) slot += wave_total[x];
    kept[slot] = row;                             // slot < survivors of all blocks <= n
}

// T: the access unit (16 / 8 / 4 / 1 bytes); pitches and the row length arrive in units of it
template <class T> __device__ __forceinline__ T zero_unit();
template <> __device__ __forceinline__ uint4 zero_unit<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint2 zero_unit<uint2>() { return make_uint2(0u, 0u); }
template <> __device__ __forceinline__ unsigned zero_unit<unsigned>() { return 0u; }
template <> __device__ __forceinline__ unsigned char zero_unit<unsigned char>() { return 0; }

template <class T>
__global__ __launch_bounds__(RG_NT) void rows_gather_kernel(const T* src, long long ld_src, long long n_src,
                                                            const long long* pos, long long n_out, long long units,
                                                            T* dst, long long ld_dst, int lanes_log2) {
    const int L = 1 << lanes_log2;
    const int sub = threadIdx.x & (L - 1);
    const long long group = (long long)blockIdx.x * (RG_NT >> lanes_log2) + (threadIdx.x >> lanes_log2);
    const long long groups = (long long)gridDim.x * (RG_NT >> lanes_log2);
    for (long long j = group; j < n_out; j += groups) {
        const long long p = pos[j];
        const T* from = p >= 0 && p < n_src ? src + p * ld_src : nullptr;      // nullptr: zeros
        T* to = dst + j * ld_dst;
        for (long long u = sub; u < units; u += L) to[u] = from ? from[u] : zero_unit<T>();
    }
}

template <class T>
static int launch_gather(const void* src, long long ld_src_bytes, long long n_src, const long long* pos, long long n_out,
                         long long row_bytes, void* dst, long long ld_dst_bytes, hipStream_t st) {
    const long long units = row_bytes / (long long)sizeof(T);
    int lanes_log2 = 0;
    while (lanes_log2 < 8 && (1ll << lanes_log2) < units) ++lanes_log2;
    const long long rows_per_block = RG_NT >> lanes_log2;
    const long long want = (n_out + rows_per_block - 1) / rows_per_block;
    const unsigned blocks = (unsigned)(want < RG_MAX_BLOCKS ? want : RG_MAX_BLOCKS);
    hipLaunchKernelGGL(rows_gather_kernel<T>, dim3(blocks), dim3(RG_NT), 0, st, (const T*)src,
                       ld_src_bytes / (long long)sizeof(T), n_src, pos, n_out, units, (T*)dst,
                       ld_dst_bytes / (long long)sizeof(T), lanes_log2);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

}  // namespace amdrec

using namespace amdrec;

static int check_plan_n(int64_t n) {
    REQUIRE(n >= 0, "n=%lld is negative", (long long)n);
    REQUIRE(n <= 2147483647ll, "n=%lld: at most 2^31 - 1 rows per call", (long long)n);
    return AMDREC_OK;
}

extern "C" int amdrec_remove_plan_workspace(int64_t n, size_t* bytes) {
    REQUIRE(bytes != nullptr, "null pointer: bytes");
    if (int rc = check_plan_n(n)) return rc;
    *bytes = RemovePlanWs(nullptr, n).bytes() + 256;
    return AMDREC_OK;
}

extern "C" int amdrec_remove_plan(const int64_t* ids, int64_t n, const int64_t* remove, int64_t n_remove, int64_t* kept,
                                  int64_t* n_kept, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_plan_n(n)) return rc;
    REQUIRE(n_remove >= 0, "n_remove=%lld is negative", (long long)n_remove);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) {
        if (n_kept == nullptr) return AMDREC_OK;              // nothing to plan and nowhere to say so
        hipLaunchKernelGGL(remove_scan_kernel, dim3(1), dim3(RP_NT), 0, st, (unsigned*)nullptr, 0, (long long*)n_kept);
        HIP_TRY(hipGetLastError());
        return AMDREC_OK;
    }
    REQUIRE(n_remove == 0 || remove != nullptr, "null pointer: remove");
    REQUIRE(kept != nullptr && n_kept != nullptr, "null pointer: kept / n_kept");
    RemovePlanWs w(ws, n);
    if (int rc = require_workspace(ws, ws_bytes, w.bytes(), 256)) return rc;
    const unsigned blocks = (unsigned)((n + RP_NT - 1) / RP_NT);
    ProfScope prof("remove_plan", 0.0, (double)n * ((ids ? 8 : 0) + 2 + 8) + (double)n_remove * 8, st);
    hipLaunchKernelGGL(remove_flag_kernel, dim3(blocks), dim3(RP_NT), 0, st, (const long long*)ids, (long long)n,
                       (const long long*)remove, (long long)n_remove, w.flags, w.counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(remove_scan_kernel, dim3(1), dim3(RP_NT), 0, st, w.counts, (int)blocks, (long long*)n_kept);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(remove_write_kernel, dim3(blocks), dim3(RP_NT), 0, st, (const unsigned char*)w.flags, (long long)n,
                       (const unsigned*)w.counts, (long long*)kept);
    HIP_TRY(hipGetLastError());
    return AMDREC_OK;
}

extern "C" int amdrec_rows_gather(const void* src, int64_t ld_src_bytes, int64_t n_src, const int64_t* pos, int64_t n_out,
                                  int64_t row_bytes, void* dst, int64_t ld_dst_bytes, void* stream) {
    REQUIRE(row_bytes >= 1, "row_bytes=%lld: a row has at least one byte", (long long)row_bytes);
    REQUIRE(n_src >= 0 && n_out >= 0, "n_src=%lld / n_out=%lld is negative", (long long)n_src, (long long)n_out);
    REQUIRE(ld_src_bytes >= row_bytes, "ld_src_bytes=%lld is smaller than row_bytes=%lld", (long long)ld_src_bytes,
            (long long)row_bytes);
    REQUIRE(ld_dst_bytes >= row_bytes, "ld_dst_bytes=%lld is smaller than row_bytes=%lld", (long long)ld_dst_bytes,
            (long long)row_bytes);
    if (n_out == 0) return AMDREC_OK;
    REQUIRE(pos != nullptr && dst != nullptr, "null pointer: pos / dst");
    REQUIRE(src != nullptr || n_src == 0, "null pointer: src");
    if (n_src > 0) {                                           // the byte ranges the two arrays span must be disjoint
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(n_src - 1) * (uintptr_t)ld_src_bytes + (uintptr_t)row_bytes;
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(n_out - 1) * (uintptr_t)ld_dst_bytes + (uintptr_t)row_bytes;
        REQUIRE(s1 <= d0 || d1 <= s0, "dst overlaps src: the gather is out of place");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof("rows_gather", 0.0, (double)n_out * (2.0 * (double)row_bytes + 8.0), st);
    const uintptr_t all = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)ld_src_bytes | (uintptr_t)ld_dst_bytes |
                          (uintptr_t)row_bytes;                // widest unit that divides pointers, pitches and row size
    const long long* p = (const long long*)pos;
    if (all % 16 == 0) return launch_gather<uint4>(src, ld_src_bytes, n_src, p, n_out, row_bytes, dst, ld_dst_bytes, st);
    if (all % 8 == 0) return launch_gather<uint2>(src, ld_src_bytes, n_src, p, n_out, row_bytes, dst, ld_dst_bytes, st);
    if (all % 4 == 0) return launch_gather<unsigned>(src, ld_src_bytes, n_src, p, n_out, row_bytes, dst, ld_dst_bytes, st);
    return launch_gather<unsigned char>(src, ld_src_bytes, n_src, p, n_out, row_bytes, dst, ld_dst_bytes, st);
}
