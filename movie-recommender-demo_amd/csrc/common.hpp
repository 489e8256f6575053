// Common device/host helpers for libamdrec (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace amdrec {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- error plumbing (amdrec_last_error) -------------------------------------------
extern thread_local char g_err[512];
int set_error(int code, const char* fmt, ...);

#define AMDREC_OK 0
#define AMDREC_EINVAL (-1)
#define AMDREC_EHIP (-2)
#define AMDREC_EWORKSPACE (-3)
#define AMDREC_EINDEX (-4)

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess)                                                          \
            return amdrec::set_error(AMDREC_EHIP, "%s failed: %s (%s:%d)", #expr,       \
                                     hipGetErrorString(e__), __FILE__, __LINE__);       \
    } while (0)

#define REQUIRE(cond, ...)                                                              \
    do {                                                                                \
        if (!(cond)) return amdrec::set_error(AMDREC_EINVAL, __VA_ARGS__);              \
    } while (0)

// ---- order-preserving 64-bit candidate keys ---------------------------------------
// key = (orderable(score) << 32) | ~position : larger key == better candidate
// (higher score; equal score -> LOWER position wins).  Positions are unique, so keys of
// one query are a strict total order and every selection below is deterministic.
__host__ __device__ inline uint32_t f32_orderable(float f) {
    f += 0.0f;  // -0.0 -> +0.0 so equal floats give equal keys
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float f32_from_orderable(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
// v0^2 + v1^2 + v2^2 + v3^2 as ONE explicit fma chain: the row-norm kernels (amdrec_l2_normalize, the towers' fused second
// normalisation) must round identically, and a sum of products left to the compiler is contracted differently from one
// context to the next
__device__ __forceinline__ float sumsq4(const f32x4& v) {
    return __builtin_fmaf(v[3], v[3], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[1], v[1], v[0] * v[0])));
}

// ReLU that keeps a NaN, as torch.relu does (fmaxf alone returns its other operand, 0): a row with a NaN feature then leaves a
// tower as a NaN embedding, which the search answers with an empty candidate list, and a ranker as NaN logits, instead of as
// the output of an all-zero hidden layer.  Every other value, -0.0 included, gives what fmaxf(v, 0) gives.  Used by every
// Linear+ReLU epilogue (tower_small.hip, layers.hip EpiLinearT); the row-owner ranker kernels keep their one-instruction
// ReLUs and restore the NaN per row at the logit store (x3_common.hpp keep_nan).
__device__ __forceinline__ float relu_keep_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// the probability the stage-2 entries report for a logit (amdrec_select_topk, amdrec_ranker_winner_heads): ONE expression, so
// that a task's score does not depend on which of them wrote it
__device__ __forceinline__ float sigmoid_prob(float x) { return 1.0f / (1.0f + expf(-x)); }

__host__ __device__ inline unsigned long long make_key(float score, uint32_t pos) {
    return ((unsigned long long)f32_orderable(score) << 32) | (unsigned long long)(~pos);
}
__host__ __device__ inline float key_score(unsigned long long k) {
    return f32_from_orderable((uint32_t)(k >> 32));
}
__host__ __device__ inline uint32_t key_pos(unsigned long long k) { return ~(uint32_t)k; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- caller-provided workspaces -------------------------------------------------------
// Cuts a workspace into 256-byte-aligned sub-buffers, in the order of the take() calls.  ONE layout (a struct that derives
// from it and cuts in its constructor, or a function) serves a workspace's *_workspace query (null base: it only measures,
// its pointers are never dereferenced) and the entry that consumes the workspace: size and carve cannot drift apart.
struct Carver {
    char* base;
    size_t next = 0, used = 0;   // offset of the next sub-buffer; end of the last one, without its padding
    explicit Carver(void* ws) : base(static_cast<char*>(ws)) {}
    template <class T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + next) : nullptr;
        used = next + count * sizeof(T);
        next = align_up(used, 256);
        return p;
    }
    size_t bytes() const { return next; }
    // a run of adjacent sub-buffers that one memset clears: m = bytes() before its first take(), bytes_since(m) after its last
    size_t bytes_since(size_t m) const { return used - m; }
};

// the check of every workspace-taking entry: present, large enough and (align > 0) aligned
inline int require_workspace(const void* ws, size_t have, size_t need, size_t align = 0) {
    if (!ws || have < need) return set_error(AMDREC_EWORKSPACE, "workspace too small: need %zu bytes, got %zu", need, have);
    if (align && (uintptr_t)ws % align) return set_error(AMDREC_EINVAL, "workspace must be %zu-byte aligned", align);
    return AMDREC_OK;
}

// hipFuncSetAttribute applies to the CURRENT device only, so "done once" must be tracked per device (a process may
// drive several GPUs; a benign race between threads sets an attribute twice).
struct PerDeviceOnce {
    bool done[64] = {};
    bool pending() const {
        int d = 0;
        return hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64 || !done[d];
    }
    void mark() {
        int d = 0;
        if (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64) done[d] = true;
    }
    // the dynamic-LDS ceiling of one kernel (`this` is that kernel's static record), set on the first launch per device
    hipError_t set_dynamic_lds(const void* kern, size_t bytes) {
        if (!pending()) return hipSuccess;
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) mark();
        return e;
    }
};

// ---- optional per-launch timing (amdrec_profile_*): HIP events recorded on the launch stream
// around each GEMM launch, accumulated per kernel tag.  Off by default (zero cost).
struct ProfScope {
    hipEvent_t end;          // nullptr: not timed.  The scope keeps the EVENT, not an index into the record table: another
    hipStream_t st;          // thread may reset the table (amdrec_profile_enable) between this scope's two ends
    unsigned long long gen;  // generation of the record table the scope was opened in: a reset in between recycles its events,
                             // which may by then belong to another scope - the end record is skipped in that case
    ProfScope(const char* tag, double flops, double bytes, hipStream_t st);
    ~ProfScope();
};
extern std::atomic<bool> g_prof_on;

}  // namespace amdrec
