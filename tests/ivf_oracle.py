"""Helpers of the IVF-Flat shape-surface tests (tests/test_ivf_surface_cpu.py, tests/test_ivf_surface_gpu.py): bounds that
scale with the shape, float64 / integer numpy statements of what the kernels of csrc/ivf.hip compute, and the seeded inputs
both files share.  No GPU, no torch.

Bounds (derived, not measured):

* ``score_tol(dim, qnorm, xnorm)`` = (dim + 2) * 2^-24 * qnorm * xnorm bounds |fl32(<q, x>) - <q, x>| for an fp32 inner
  product of ``dim`` terms summed in ANY order, with or without fused multiply-adds.  Every partial sum of a summation
  tree is rounded once (relative error <= u = 2^-24) and every product at most once; an input term passes through at most
  ``dim`` roundings on its way to the root (dim - 1 additions, 1 product), so the computed value is sum_i q_i x_i (1 +
  t_i) with |t_i| <= (1 + u)^dim - 1 ~ dim * u, and |error| <= dim * u * sum_i |q_i x_i| <= dim * u * |q| |x| (Cauchy-
  Schwarz).  The per-pair scan (64 lanes x fma chains + a shuffle tree), the fp32-MFMA GEMM of the grouped scan and the
  16-lane re-score of the prefiltered scan are three such orders.  The ``+ 2`` covers the other side of the comparison:
  the float64 reference value is itself rounded to fp32 when it is compared or stored (1 u) and the second-order term of
  (1 + u)^dim (2048^2 u^2 / 2 < 0.01 u).
* ``topk_tau(...)`` = 2 * score_tol: two rows whose exact scores differ by less than that can be ranked either way by a
  correct fp32 scan (each may be off by one bound), so this is the near-tie band of oracle.search.check_topk.
* ``eps64``: the prefilter's error bound as include/amdrec.h states it for amdrec_flat_search_mixed, in float64:
  eps = |dq| (M + D) + |q| D + 2 dim 2^-24 |q| (M + D), dq = bf16(q) - q, M / D = largest row norm / largest row
  rounding-error norm of the bf16 shadow.  amdrec_ivf_filter_bounds must return tau_lo <= tau - eps64 (soundness: every row
  whose fp32 score reaches tau has a bf16 score of at least tau_lo).
"""
import numpy as np

U = 2.0 ** -24                  # fp32 unit roundoff

# dimensions of the end-to-end surface: under one float4 wave stride of the per-pair scan (dim / 4 < 64), not multiples of
# 8 / 16 / 64, the loop case (dim / 4 > 64) and the limit
SURFACE_DIMS = (4, 12, 36, 64, 100, 136, 512, 1000, 2048)
# amdrec_ivf_assign / amdrec_ivf_kmeans_step: fewer centroids than one GEMM tile ... more centroids than rows
ASSIGN_DIMS = (4, 36, 100, 2048)
ASSIGN_NLISTS = (1, 3, 200, 4096)
ASSIGN_ROWS = 1500
FILTER_BOUND_DIMS = (8, 72, 256, 2048)


def score_tol(dim, qnorm=1.0, xnorm=1.0):
    return (dim + 2) * U * float(qnorm) * float(xnorm)


def topk_tau(dim, qnorm=1.0, xnorm=1.0):
    return 2.0 * score_tol(dim, qnorm, xnorm)


def max_norm(x):
    """Largest float64 row norm over the finite rows of x (1.0 if there is none)."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x).all(axis=1)
    return float(np.sqrt((x[fin] ** 2).sum(axis=1)).max()) if fin.any() else 1.0


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def clustered(n, d, n_clusters, seed, spread=0.35, sizes=None, return_centres=False):
    """n unit rows around n_clusters random centres (sizes: rows per cluster, in cluster order, instead of a uniform draw)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_clusters, d)).astype(np.float32)
    if sizes is None:
        which = rng.integers(0, n_clusters, n)
    else:
        assert sum(sizes) == n and len(sizes) == n_clusters
        which = rng.permutation(np.repeat(np.arange(n_clusters), sizes))
    x = c[which] + spread * rng.standard_normal((n, d)).astype(np.float32)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    if return_centres:
        return x, c / np.linalg.norm(c, axis=1, keepdims=True)
    return x


def surface_rows(dim):
    """Rows of the k-means-trained index of the surface test: fewer as the rows get longer."""
    return 6000 if dim <= 136 else 4000 if dim <= 512 else 3000 if dim <= 1000 else 2500


LONG_LIST_ROWS = 2400           # past the grouped scan's short-list limit (1536 rows: 128-row tiles up to it, 256-row beyond)


def surface_corpus(dim, layout, nlist):
    """-> (unit rows, the nlist unit cluster centres).  'short': surface_rows(dim) rows drawn evenly from the clusters (the
    index trains on them); 'long': one cluster of LONG_LIST_ROWS rows and 20 in each of the others, for an index whose
    quantizer is the centres themselves, so that list 0 is longer than 1536 rows."""
    if layout == "short":
        return clustered(surface_rows(dim), dim, nlist, 100 + dim, return_centres=True)
    return clustered(LONG_LIST_ROWS + 20 * (nlist - 1), dim, nlist, 200 + dim, spread=0.2,
                     sizes=[LONG_LIST_ROWS] + [20] * (nlist - 1), return_centres=True)


def assign_case(dim, nlist):
    """(x [ASSIGN_ROWS, dim], centroids [nlist, dim]) of the direct amdrec_ivf_assign / kmeans_step test: unit rows.
    The fp32 near-tie band grows with dim (4.9e-4 at 2048) while the scores of isotropic rows against many centroids crowd
    together like 1 / sqrt(dim), so the rows live in a 24-dimensional latent space mapped densely into dim coordinates:
    every coordinate carries signal, and the two best centroids of a row stay further apart than the band (asserted in
    tests/test_ivf_surface_cpu.py)."""
    m = min(dim, 24)
    rng = np.random.default_rng(3000 + dim)
    B = rng.standard_normal((m, dim)).astype(np.float32)

    def lift(y):
        x = y @ B
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x = lift(clustered(ASSIGN_ROWS, m, 25, 1000 + dim))
    cent = lift(clustered(nlist, m, 25, 2000 + dim + nlist, spread=0.6))
    return x, cent


# add()-time training on a corpus with non-finite rows (no sub-sampling at this size: the trainer's first draw is over the
# rows as given)
NAN_TRAIN_ROWS, NAN_TRAIN_NLIST, NAN_TRAIN_DIM, TRAIN_SEED = 3000, 16, 64, 1234


def initial_centroid_rows(torch, n, nlist):
    """The rows amdrec.ivf.InvertedLists.train copies into the initial centroid table when it does not sub-sample: the
    first nlist entries of torch.randperm(n) from a CPU generator seeded with ivf.SEED."""
    g = torch.Generator(device="cpu")
    g.manual_seed(TRAIN_SEED)
    return torch.randperm(n, generator=g)[:nlist].tolist()


def nan_train_bad_rows(torch):
    """Rows made non-finite in the training case: two that the initial draw picks and one that it does not."""
    drawn = initial_centroid_rows(torch, NAN_TRAIN_ROWS, NAN_TRAIN_NLIST)
    other = next(i for i in range(NAN_TRAIN_ROWS) if i not in drawn)
    return [drawn[0], drawn[3], other]


# ---- fp32 inner products in two summation orders (self-check of score_tol) -------------------------------------------------
def dot32_forward(q, x):
    """Row-wise fp32 inner products of q[i] and x[i], one forward chain per pair (products rounded, then added)."""
    q, x = np.asarray(q, dtype=np.float32), np.asarray(x, dtype=np.float32)
    acc = np.zeros(q.shape[0], dtype=np.float32)
    for i in range(q.shape[1]):
        acc = acc + q[:, i] * x[:, i]
    return acc


def dot32_pairwise(q, x):
    """The same products summed by a balanced binary tree in fp32."""
    p = np.asarray(q, dtype=np.float32) * np.asarray(x, dtype=np.float32)
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), dtype=np.float32)], axis=1)
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


# ---- 64-bit pool keys (csrc/common.hpp make_key) ---------------------------------------------------------------------------
def make_keys(scores, pos):
    """(order-preserving image of the fp32 score << 32) | ~position: larger key = better, equal scores -> lower position."""
    u = np.asarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(u >= 0x80000000, (~u) & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (o << np.uint64(32)) | ((~np.asarray(pos).astype(np.uint64)) & np.uint64(0xFFFFFFFF))


def decode_keys(keys):
    """-> (fp32 scores, int64 positions) of non-zero keys (a zero key is an empty slot: decode it as (-inf, -1))."""
    k = np.asarray(keys).view(np.uint64) if np.asarray(keys).dtype != np.uint64 else np.asarray(keys)
    o = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o >= 0x80000000, o ^ np.uint32(0x80000000), ~o).astype(np.uint32)
    sc = bits.view(np.float32).copy()
    pos = ((~k) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    empty = k == 0
    sc[empty] = -np.inf
    pos[empty] = -1
    return sc, pos


# ---- amdrec_ivf_group -------------------------------------------------------------------------------------------------------
def group_reference(probes, nlist, list_len, qtile):
    """What amdrec_ivf_group returns for probes [nq, ncol] (the probe columns the call is given; a probe < 0 or >= nlist is
    no list: length 0, member of no group) -> dict(pool_base [nq, ncol], pool_count [nq], group_off [nlist + 1],
    qtile_prefix [nlist + 1], members = the flat pair numbers q * ncol + p sorted by (list, pair number): list l's group is
    members[group_off[l]:group_off[l + 1]], in unspecified order on the device)."""
    probes = np.asarray(probes, dtype=np.int64)
    list_len = np.asarray(list_len, dtype=np.int64)
    nq, ncol = probes.shape
    valid = (probes >= 0) & (probes < nlist)
    lens = np.where(valid, list_len[np.where(valid, probes, 0)], 0)
    run = np.cumsum(lens, axis=1)
    cnt = np.bincount(probes[valid], minlength=nlist).astype(np.int64)
    flat = np.nonzero(valid.reshape(-1))[0]
    order = np.lexsort((flat, probes.reshape(-1)[flat]))
    return {"pool_base": run - lens, "pool_count": run[:, -1] if ncol else np.zeros(nq, np.int64),
            "group_off": np.concatenate([[0], np.cumsum(cnt)]),
            "qtile_prefix": np.concatenate([[0], np.cumsum((cnt + qtile - 1) // qtile)]),
            "members": flat[order]}


def group_members(pair_query, pair_probe, group_off, ncol):
    """The device's pair arrays in the canonical form of group_reference()['members'] (sorted inside every group)."""
    group_off = np.asarray(group_off, dtype=np.int64)
    total = int(group_off[-1])
    flat = np.asarray(pair_query, dtype=np.int64)[:total] * ncol + np.asarray(pair_probe, dtype=np.int64)[:total]
    which = np.repeat(np.arange(len(group_off) - 1), np.diff(group_off))
    return flat[np.lexsort((flat, which))]


# ---- the bf16 prefilter's bound ---------------------------------------------------------------------------------------------
def bf16_round(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, finite inputs."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def eps64(q, q16, M, D):
    """eps of every query row: q fp32 [nq, dim], q16 = its bf16 copy as fp32 values; M, D = max_norm[0], max_norm[1]."""
    q, q16 = np.asarray(q, dtype=np.float64), np.asarray(q16, dtype=np.float64)
    dim = q.shape[1]
    qn, dqn = np.sqrt((q * q).sum(axis=1)), np.sqrt(((q16 - q) ** 2).sum(axis=1))
    return dqn * (M + D) + qn * D + 2.0 * dim * U * qn * (M + D)


# ---- assignment, one Lloyd step, search with non-finite rows ---------------------------------------------------------------
def scores64(x, cent):
    """float64 <x, c> with the kernels' rule for non-finite scores: a NaN score never wins (-inf)."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(x, dtype=np.float64) @ np.asarray(cent, dtype=np.float64).T
    return np.where(np.isnan(s), -np.inf, s)


def assign_reference(x, cent):
    """-> (arg max_c <x, c> per row, ties -> lower c; a row without a finite score -> list 0,
           best float64 score, gap to the second best score (inf with one centroid))."""
    s = scores64(x, cent)
    best = np.argmax(s, axis=1)
    top = s[np.arange(len(s)), best]
    if s.shape[1] > 1:
        t = s.copy()
        t[np.arange(len(s)), best] = -np.inf
        with np.errstate(invalid="ignore"):
            gap = top - t.max(axis=1)
        gap = np.where(np.isnan(gap), 0.0, gap)
    else:
        gap = np.full(len(s), np.inf)
    return best, top, gap


def kmeans_step_reference(x, assign, cent):
    """One spherical Lloyd update given the assignment: float64 sum of the members, normalised; empty clusters keep their
    centroid.  -> (centroids float64, members per cluster, norm of each member sum)."""
    x64 = np.asarray(x, dtype=np.float64)
    out = np.asarray(cent, dtype=np.float64).copy()
    nlist = out.shape[0]
    count = np.bincount(assign, minlength=nlist)
    sums = np.zeros_like(out)
    np.add.at(sums, assign, x64)
    norm = np.sqrt((sums * sums).sum(axis=1))
    live = (count > 0) & (norm > 0)
    out[live] = sums[live] / norm[live, None]
    return out, count, norm


def ivf_search_nonfinite(xb, assign, nlist, xq, k, probes):
    """oracle.search.ivf_search for a corpus with non-finite rows, given the probes: a row whose float64 score is NaN
    scores -inf and ranks after every finite row (lower position first); unfilled slots (-inf, -1)."""
    xb64, xq64 = np.asarray(xb, dtype=np.float64), np.asarray(xq, dtype=np.float64)
    assign = np.asarray(assign)
    order = np.argsort(assign, kind="stable")
    bounds = np.searchsorted(assign[order], np.arange(nlist + 1))
    nq = xq64.shape[0]
    D = np.full((nq, k), -np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        rows = [order[bounds[c]:bounds[c + 1]] for c in probes[q] if 0 <= c < nlist]
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        if len(rows) == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            s = xb64[rows] @ xq64[q]
        s = np.where(np.isnan(s), -np.inf, s).astype(np.float32)
        o = np.lexsort((rows, -s.astype(np.float64)))[:k]
        D[q, :len(o)] = s[o]
        I[q, :len(o)] = rows[o]
    return D, I


def check_probes(probes, s64, tau):
    """The coarse probes of every query against the float64 centroid scores s64 [nq, nlist]: distinct, sorted descending up
    to ``tau``, and no centroid left out that beats a probed one by more than ``tau``."""
    probes = np.asarray(probes)
    nq, nprobe = probes.shape
    for q in range(nq):
        p = probes[q]
        assert (p >= 0).all() and (p < s64.shape[1]).all() and len(set(p.tolist())) == nprobe, (q, p)
        sp = s64[q, p]
        assert (np.diff(sp) <= tau).all(), (q, float(np.diff(sp).max()))
        rest = np.delete(s64[q], p)
        if rest.size:
            assert rest.max() <= sp.min() + tau, (q, float(rest.max() - sp.min()))
