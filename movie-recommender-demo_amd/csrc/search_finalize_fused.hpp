// finalize_fused_kernel's definition (search.hip has its description).  No include guard: search.hip includes this file
// TWICE, inside namespace amdrec, with five macros that name the kernel and say what a boost adds to it -
//   AMDREC_FUSED_KERNEL   the kernel's name
//   AMDREC_FUSED_PARAMS   parameters behind fticket           (plain: none; boosted: , boost, weight, boost_max)
//   AMDREC_FUSED_BOOST    a statement at the top of the body  (plain: none; boosted: const Boosted bo{...};)
//   AMDREC_FUSED_EPS(e)   the error bound from query_eps's e  (plain: e;    boosted: fin_eps(e, d, q, bo))
//   AMDREC_FUSED_TERM     rescore_keys' last argument         (plain: none; boosted: , fin_term(bo, q))
// - because the two kernels must be two functions of different NAMES with one text.  A shared __device__ body called from two
// kernels changes the plain kernel's register allocation and instruction order, and a boosted instantiation of one kernel
// template sorts, by name, in front of finalize_mixed_kernel in the module's LDS lowering (it numbers the kernels that reach
// LDS variables through a call in name order, and each loads its number as a constant) and changes that constant there.
// With the plain macros the token stream is the one the kernel always had.
__global__ __launch_bounds__(512) void AMDREC_FUSED_KERNEL(const unsigned long long* cand, long long cstride, const int* segcnt,
                                                             int nseg, int seg_cap, const int* ocnt, int cap, int k,
                                                             long long nrows, const float* tau, const float* max_norm,
                                                             const float* X, long long ldx, int d, const float* Q, long long ldq,
                                                             int* fail, float* outD, long long* outI, long long pos_offset,
                                                             unsigned long long* exact, int* fcount, int* fticket AMDREC_FUSED_PARAMS) {
    AMDREC_FUSED_BOOST
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];      // [cap] then qv[d]
    float* qv = reinterpret_cast<float*>(keys + cap);
    __shared__ int hist[2048];
    __shared__ int scratch[514];
    __shared__ float red[16];
    __shared__ int m_sh, own_sh, base_sh;
    __shared__ int seg_n[256];
    constexpr int PER = CAND_CAP / 512;
    constexpr int OVP = 4;
    const int q = blockIdx.y, nq = gridDim.y, s = blockIdx.x, S = gridDim.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int need = (int)(nrows < k ? nrows : k);
    // the candidate slots are requested before the segment counts that say which of them are valid have arrived (one
    // global round trip instead of two); validity is applied below
    const unsigned long long* blk = cand + (long long)q * cstride;
    unsigned long long mine[PER + OVP];
#pragma unroll
    for (int j = 0; j < PER; ++j) mine[j] = tid + 512 * j < nseg * seg_cap ? blk[tid + 512 * j] : 0ull;
#pragma unroll
    for (int j = 0; j < OVP; ++j) mine[PER + j] = blk[CAND_CAP + tid + 512 * j];
    if (tid == 0) { m_sh = 0; own_sh = 0; }
    const int oc = ocnt[q];
    const int c = segment_counts<512>(segcnt + (long long)q * nseg, nseg, seg_cap, oc, need, cap, seg_n);
    // every workgroup of the query reaches the same verdict: one reports
    if (c < 0) { if (s == 0) give_up(fail, q, nq); return; }
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (!slot_valid(tid + 512 * j, nseg, seg_cap, seg_n)) mine[j] = 0ull;
#pragma unroll
    for (int j = 0; j < OVP; ++j)
        if (tid + 512 * j >= oc) mine[PER + j] = 0ull;
    const float eps = AMDREC_FUSED_EPS(query_eps<512>(Q + (long long)q * ldq, d, qv, red, max_norm));
    if (!(eps < INFINITY)) { if (s == 0) give_up(fail, q, nq); return; }
    if (need == 0) {
        if (s == 0) write_result(keys, 0, k, q, outD, outI, pos_offset);
        return;
    }
    // a_k to its top 22 bits (two radix passes): the remaining 10 bits cleared give a value <= a_k in the orderable image,
    // i.e. a slightly lower cut - a superset of the survivors of the exact a_k (a relative 2^-13 of the score: no
    // measurable number of extra survivors), never a missing one
    const uint32_t a_k = select_prefix_desc<512, 2>(hist, scratch, need, [&](auto count_key) {
#pragma unroll
        for (int j = 0; j < PER + OVP; ++j) count_key(mine[j]);
    });
    // prune (finalize_mixed_kernel's rule); this workgroup keeps the survivors at positions pos % S == s
    const float cut = f32_from_orderable(a_k) - 2.f * eps;
    int n_surv = 0;
#pragma unroll
    for (int j = 0; j < PER + OVP; ++j)
        if (mine[j] != 0ull && key_score(mine[j]) >= cut) {
            ++n_surv;
            if ((int)(key_pos(mine[j]) % (uint32_t)S) == s) keys[atomicAdd(&own_sh, 1)] = mine[j];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_surv += __shfl_xor(n_surv, o, 64);
    if (lane == 0 && n_surv) atomicAdd(&m_sh, n_surv);
    __syncthreads();
    const int m = m_sh, own = own_sh;                         // need <= m <= c
    rescore_keys<8, 8>(keys, own, X, ldx, qv, d >> 2 AMDREC_FUSED_TERM);
    if (tid == 0) base_sh = __hip_atomic_fetch_add(&fcount[q], own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    unsigned long long* list = exact + (long long)q * cap;
    for (int i = tid; i < own; i += 512) list[base_sh + i] = keys[i];
    if (!last_workgroup(&fticket[q], S, false)) return;
    // the query's last workgroup: all m exact keys are in the list (NaN re-scores as key 0: they sort last)
    for (int i = tid; i < m; i += 512) keys[i] = list[i];
    __syncthreads();
    const unsigned long long* sorted = sort_keys_desc<512>(keys, keys + (m <= 1024 ? 1024 : 2048), m, 0);
    if (!certify_or_fail(sorted, need, (long long)c >= nrows, tau[q] + eps, fail, q, nq)) return;
    write_result(sorted, m, k, q, outD, outI, pos_offset);
}
