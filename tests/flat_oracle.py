"""Helpers of the flat-search shape-surface tests (tests/test_flat_surface_cpu.py, tests/test_flat_surface_gpu.py): the tables
both files share, the seeded inputs, the float64 statement of the search's contract for non-finite rows, and a Python
restatement of the host plan of csrc/search.hip.  numpy only: no GPU, no torch.

Tolerances.  Scores: cases.SCORE_ATOL against float64 rounded to fp32; near-tie band at the k-th score: cases.TOPK_TAU; both
times |q|_max * |x|_max where a case feeds un-normalised rows to the C entry points (``score_tol`` / ``topk_tau``).
amdrec_flat_search_mixed holds SCORE_ATOL at every dimension (its scores are the re-score's: 64 lane chains of dim / 256
float4 steps and a six-level tree).  amdrec_flat_search returns the scores of its fp32-MFMA pass, ONE chain of dim / 2
accumulations per (row, query) (gemm_core.hpp: v_mfma_f32_32x32x2_f32 into the same accumulator), and misses 1e-6 from
d = 512 on by that summation's rounding alone.  FP32_DEVIATION is that rounding measured on the CPU, against float64, on the
scores that are compared (every query of the surface case against its 100 best rows): a forward chain
(ivf_oracle.dot32_forward) leaves 1.06e-6 / 1.53e-6 / 2.75e-6 at d = 512 / 1000 / 2048, a balanced tree (dot32_pairwise)
1.0e-7 at each.  SCORE_TOL_BY_DIM, for the fp32 engine at those dimensions, is 4 x the larger figure - 4.24e-6, 6.12e-6,
1.10e-5 - and stays under the derived ivf_oracle.score_tol(dim) (3.1e-5, 6.0e-5, 1.2e-4); tests/test_flat_surface_cpu.py
measures the figures again and holds both tables to that rule.
"""
import numpy as np

from amdrec import synth
from tests import cases, ivf_oracle

# ---- tables -----------------------------------------------------------------------------------------------------------------
FLAT_DIMS_STREAM = (32, 64, 128, 256)                     # scan_filter_kernel / sample_max_kernel are instantiated for these
FLAT_DIMS_GENERIC = (8, 24, 72, 136, 512, 1000, 2048)     # generic bf16 tiles (dim % 8 == 0): under one K-step ... the limit
FLAT_DIMS_FP32_ONLY = (4, 12, 36, 100)                    # dim % 8 == 4: FAISSIndex runs amdrec_flat_search under either prefilter
FLAT_DIMS = FLAT_DIMS_STREAM + FLAT_DIMS_GENERIC + FLAT_DIMS_FP32_ONLY
# query counts at which the host dispatch or a kernel switches: tau inside the streaming pass (<= 8); GEMM query tile (32,
# 64); work split of scan_filter_kernel (64, 128, 256); fused finalize (<= 128); make_plan's target (>= 256); a second
# 512-query group
NQ_EDGES = (1, 8, 9, 32, 33, 64, 65, 128, 129, 255, 256, 257, 512, 513)
NQ_EDGES_FP32 = (32, 33, 64, 65, 129)

# csrc/search.hip
CAND_CAP, SAMPLE_RANK, KMAX, FIX_BUF, SAMPLE_G = 8192, 64, 2048, 4096, 256
SCAN_ROWS, SCAN_QGROUP, FUSED_MAX_NQ, OVERFLOW_MAX = 128, 512, 128, 2048

FP32_DEVIATION = {512: (1.06e-6, 1.02e-7), 1000: (1.53e-6, 1.04e-7), 2048: (2.75e-6, 1.01e-7)}    # dim -> measured (forward, tree)
SCORE_TOL_BY_DIM = {d: 4 * max(v) for d, v in FP32_DEVIATION.items()}    # amdrec_flat_search only: 4.24e-6, 6.12e-6, 1.10e-5


def score_tol(dim, scale=1.0, engine="mixed"):
    """Score tolerance at ``dim`` for |q| * |x| <= scale and the engine ("mixed" / "fp32") whose scores are compared; never
    above the derived fp32 bound ivf_oracle.score_tol(dim)."""
    t = max(cases.SCORE_ATOL, SCORE_TOL_BY_DIM.get(dim, 0.0) if engine == "fp32" else 0.0)
    assert t <= max(cases.SCORE_ATOL, ivf_oracle.score_tol(dim))
    return t * float(scale)


def topk_tau(scale=1.0):
    return cases.TOPK_TAU * float(scale)


def fp32_sum_deviation(q, x):
    """Largest deviation from float64 of the fp32 inner products of q[i] and x[i] in two summation orders -> (forward, tree)."""
    ref = (np.asarray(q, np.float64) * np.asarray(x, np.float64)).sum(axis=1)
    return (float(np.abs(ivf_oracle.dot32_forward(q, x) - ref).max()), float(np.abs(ivf_oracle.dot32_pairwise(q, x) - ref).max()))


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
LATENT = 8


def _lift(y, dim):
    """Unit rows of a LATENT-dimensional space mapped into ``dim`` coordinates by a dense isometry (one per dim: inner products
    and angles are those of the latent rows) and re-normalised in fp32."""
    if dim <= y.shape[1]:
        return y
    B = np.linalg.qr(np.random.default_rng(10_000 + dim).standard_normal((dim, y.shape[1])))[0].T.astype(np.float32)
    x = y @ B
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _cone(n, seed, lo, hi):
    """n unit rows of the latent space at an angle uniform in [lo, hi] from the first axis."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(lo, hi, n)
    v = rng.standard_normal((n, LATENT - 1))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([np.cos(t)[:, None], np.sin(t)[:, None] * v], axis=1).astype(np.float32)


def rows(n, dim, seed, kind, near=700, hi=1.4):
    """Unit rows [n, dim].  'iso': synth.unit_corpus (isotropic: at a large dim every score is small and the scores around
    the k-th lie 1e-5 apart, so only k = 1 cases use it).  'lifted': isotropic in LATENT dimensions, lifted - every
    coordinate carries signal while the scores stay spread like those of an 8-dimensional corpus (the trick of
    ivf_oracle.assign_case).  'cone': two populations for k >= 300 - ``near`` rows spread
    over angles 0.15 .. ``hi`` from one axis, the rest beyond hi + 0.5 - so that the k best rows of a 'cone_q' query (within
    0.25 of the axis) span most of the score range instead of crowding."""
    if kind == "iso" or (kind == "lifted" and dim <= LATENT):
        return synth.unit_corpus(n, dim, seed=seed)
    if kind == "lifted":
        return _lift(synth.unit_corpus(n, LATENT, seed=seed), dim)
    if kind == "cone":
        near = min(n, near)
        y = np.concatenate([_cone(near, seed, 0.15, hi), _cone(n - near, seed + 1, hi + 0.5, np.pi)])
        return _lift(y[np.random.default_rng(seed + 2).permutation(n)], dim)
    if kind == "cone_q":
        return _lift(_cone(n, seed, 0.0, 0.25), dim)
    raise ValueError(kind)


def case_inputs(c):
    """(corpus rows, queries) of a seeded case: dict(n, dim, nq, kind, seed[, near, hi])."""
    xb = rows(c["n"], c["dim"], c["seed"], c["kind"], c.get("near", 700), c.get("hi", 1.4))
    return xb, rows(c["nq"], c["dim"], c["seed"] + 500, "cone_q" if c["kind"] == "cone" else c["kind"])


def unnormalised(x, seed, lo, hi):
    """Rows scaled to norms drawn from [lo, hi] (the C entry points take rows as they are)."""
    return (x * np.random.default_rng(seed).uniform(lo, hi, (len(x), 1))).astype(np.float32)


# (a) dimension surface: per dim a small corpus (every row a candidate) and a sampled one, searched with the first 5 / 70 /
# 200 of 200 queries.  k = 1 on isotropic rows, k = 100 on lifted ones.  Seeds: the first from 1 under which at most 2 % of
# the queries of every prefix have their (k + 1)-th score inside the near-tie band (tests/test_flat_surface_cpu.py).
SURFACE_NQ, SURFACE_KS = (5, 70, 200), (1, 100)
SURFACE_SMALL_ROWS = 3000


def surface_rows(dim):
    return 9000 if dim >= 1000 else 12_000


# (dim, rows, k) -> seed where 1 does not do
SURFACE_SEEDS = {**{(d, n, 100): 2 for d in FLAT_DIMS if d != 4 for n in (SURFACE_SMALL_ROWS, surface_rows(d)) if n != 9000},
                 (4, surface_rows(4), 100): 4}


def surface_case(dim, n, k):
    kind = "iso" if k == 1 else "lifted"
    return dict(group="a", n=n, dim=dim, nq=SURFACE_NQ[-1], k=k, kind=kind, seed=SURFACE_SEEDS.get((dim, n, k), 1),
                prefixes=SURFACE_NQ)


# (b) batch-size edges: one corpus and 513 queries per dim, searched by prefixes
EDGE_ROWS, EDGE_K, EDGE_DIMS, EDGE_DIMS_FP32 = 20_000, 50, FLAT_DIMS_STREAM + (72,), (64, 72, 100)
EDGE_SEEDS = {}


def edge_case(dim):
    return dict(group="b", n=EDGE_ROWS, dim=dim, nq=NQ_EDGES[-1], k=EDGE_K, kind="lifted", seed=EDGE_SEEDS.get(dim, 1),
                prefixes=NQ_EDGES)


# (c) finalize shapes behind both pass kinds: (nq, k) -> the shape plan() must name
FINALIZE_ROWS, FINALIZE_DIMS = 20_000, (128, 72, 136)
FINALIZE_SHAPES = {(129, 50): "mixed<256,2048>", (256, 64): "mixed<128,1024>", (256, 300): "mixed<256,2048>",
                   (129, 500): "mixed<512,8192>"}
FINALIZE_SEEDS = {(d, 256, 300): 2 for d in FINALIZE_DIMS}


def finalize_case(dim, nq, k):
    return dict(group="c", n=FINALIZE_ROWS, dim=dim, nq=nq, k=k, kind="cone" if k >= 300 else "lifted",
                seed=FINALIZE_SEEDS.get((dim, nq, k), 1), prefixes=(nq,))


# (d) small corpus, many query groups (d = 32)
SMALL_DIM, SMALL_ROWS, SMALL_NQ, SMALL_KS = 32, (8192, 8000, 777), (1100, 2600), (10, 500)
SMALL_SEEDS = {}


def small_case(n, nq, k):
    return dict(group="d", n=n, dim=SMALL_DIM, nq=nq, k=k, kind="cone" if k >= 300 else "lifted", seed=SMALL_SEEDS.get((n, nq, k), 1),
                prefixes=(nq,))


# (a) at the limits: d = 2048, k = 2048 (nslices = 4; the general finalize with the largest dim * 4 LDS tail), 3 and 130 queries.
# 2300 near rows over angles up to 1.8: the 2048 best rows span the whole score range.
KMAX_SEED = 1


def kmax_case():
    return dict(group="a", n=9000, dim=2048, nq=130, k=KMAX, kind="cone", near=2300, hi=1.8, seed=KMAX_SEED, prefixes=(3, 130))


# (d) past the overflow block's limit.  With every row a candidate (at most CAND_CAP rows) no query count makes a workgroup
# spill more than 1342 keys per query (tests/test_flat_surface_cpu.py walks them all), so this case is a sampled corpus
# whose hits are concentrated by construction: 30 whole 128-row tiles, none of them a sample tile, hold every row that any
# query scores above 0 (angles up to 1.3 from the axis, the queries within 0.25 of it; the other rows lie beyond 2.0 and score
# under -0.17), so the threshold - taken from sample rows that all score low - admits every one of them.  Each of those
# tiles is one workgroup's only hot tile and fills its segment of seg_cap = 52 slots: 30 * (128 - 52) = 2280 keys per query
# overflow, more than OVERFLOW_MAX, while the candidate count (3840 + about 900 cold rows) stays far inside CAND_CAP.  100
# of the hot rows are spread over angles 0.3 .. 1.0 so that the k = 10 best do not crowd.
def overflow_case():
    """-> (rows, queries, k, hot tiles, overflow keys per query the streaming pass must produce)"""
    n, nq, k, dim = 20_000, 70, 10, SMALL_DIM
    p = plan(nq, n, k, dim)
    free = [t for t in range(n // SCAN_ROWS) if t not in p.sample_tiles]
    hot_tiles = free[::4][:30]
    assert p.ny == 1 and p.nseg == 157 and p.seg_cap == 52 and len(hot_tiles) == 30 and len(p.sample_tiles) == 12
    y = _cone(n, 41, 2.0, np.pi)
    hot = np.concatenate([np.arange(t * SCAN_ROWS, (t + 1) * SCAN_ROWS) for t in hot_tiles])
    yh = _cone(len(hot), 43, 1.0, 1.3)
    yh[np.random.default_rng(42).permutation(len(hot))[:100]] = _cone(100, 44, 0.3, 1.0)
    y[hot] = yh
    return _lift(y, dim), rows(nq, dim, 45, "cone_q"), k, hot_tiles, len(hot_tiles) * (SCAN_ROWS - p.seg_cap)


# (e) non-finite rows: 20,000 rows, 40 queries, k = 100 at a streaming, a generic and an fp32-only dim
NONFINITE_DIMS, NONFINITE_ROWS, NONFINITE_NQ, NONFINITE_K = (64, 72, 100), 20_000, 40, 100
NONFINITE_SEEDS = {d: 4 for d in NONFINITE_DIMS}


def nonfinite_case(dim):
    return dict(group="e", n=NONFINITE_ROWS, dim=dim, nq=NONFINITE_NQ, k=NONFINITE_K, kind="lifted",
                seed=NONFINITE_SEEDS.get(dim, 1), prefixes=(NONFINITE_NQ,))


NONFINITE_KINDS = ("all_nan", "one_nan", "pos_inf_first", "neg_inf_last")


def nonfinite_positions(n, rotation=0):
    """Where the four kinds of bad row go: row 0, the middle, the last (partial) 128-row tile - the clamped-row loads of the
    streaming pass -, the very last row.  ``rotation`` r puts kind i at place (i + r) % 4: over r = 0 .. 3 every kind
    visits every place."""
    assert n % SCAN_ROWS > 2
    places = (0, n // 2, n - n % SCAN_ROWS + 1, n - 1)
    return {kind: places[(i + rotation) % 4] for i, kind in enumerate(NONFINITE_KINDS)}


def with_nonfinite_rows(xb, rotation=0):
    """A copy of xb with an all-NaN row, a row with one NaN, a row with +inf in coordinate 0 and one with -inf in the last."""
    x = xb.copy()
    at = nonfinite_positions(len(x), rotation)
    x[at["all_nan"]] = np.nan
    x[at["one_nan"], x.shape[1] // 3] = np.nan
    x[at["pos_inf_first"], 0] = np.inf
    x[at["neg_inf_last"], -1] = -np.inf
    return x, at


# (f) C entry points with real strides
STRIDE_DIMS, STRIDE_NQ, STRIDE_ROWS, STRIDE_K, STRIDE_POS_OFFSET = (8, 72, 256, 2048), (3, 130), 9000, 50, 1_000_000
STRIDE_SEEDS = {}


def stride_case(dim):
    return dict(group="f", n=STRIDE_ROWS, dim=dim, nq=STRIDE_NQ[-1], k=STRIDE_K, kind="lifted", seed=STRIDE_SEEDS.get(dim, 1),
                prefixes=STRIDE_NQ)


def stride_inputs(dim):
    """Un-normalised rows (norms 0.5 .. 2) and queries (norms 0.5 .. 1.5) -> (xb, xq, |q|_max * |x|_max)."""
    c = stride_case(dim)
    xb, xq = case_inputs(c)
    xb, xq = unnormalised(xb, c["seed"] + 7, 0.5, 2.0), unnormalised(xq, c["seed"] + 8, 0.5, 1.5)
    return xb, xq, ivf_oracle.max_norm(xb) * ivf_oracle.max_norm(xq)


def seeded_cases():
    """Every seeded case of the GPU file whose result is compared through check_topk's near-tie band."""
    out = []
    for dim in FLAT_DIMS:
        for n in (SURFACE_SMALL_ROWS, surface_rows(dim)):
            out += [surface_case(dim, n, k) for k in SURFACE_KS]
    out += [edge_case(dim) for dim in sorted(set(EDGE_DIMS + EDGE_DIMS_FP32))]
    out += [finalize_case(dim, nq, k) for dim in FINALIZE_DIMS for nq, k in FINALIZE_SHAPES]
    out += [small_case(n, nq, k) for n in SMALL_ROWS for nq in SMALL_NQ for k in SMALL_KS]
    out += [stride_case(dim) for dim in STRIDE_DIMS]
    out += [kmax_case()] + [nonfinite_case(dim) for dim in NONFINITE_DIMS]
    return out


def reference(xb, xq, k):
    """float64 scores rounded to fp32 -> exact top-k (D, I) by (score descending, position ascending)."""
    import oracle
    return oracle.search.flat_ip_search(xb, xq, k, dtype=np.float64)


def loose_queries(xb, xq, k, tau):
    """Per query: does a row outside the float64 top-k score within ``tau`` of the k-th score without equalling it?  (That
    is what oracle.search.check_topk lets slip: such a row may replace the k-th.)"""
    if k >= len(xb):
        return np.zeros(len(xq), bool)
    D, _ = reference(xb, xq, k + 1)
    gap = D[:, k - 1].astype(np.float64) - D[:, k].astype(np.float64)
    return (gap <= tau) & (gap > 0)


# ---- the contract with non-finite rows --------------------------------------------------------------------------------------
def flat_search_nonfinite(xb, xq, k):
    """What amdrec_flat_search / amdrec_flat_search_mixed return, in float64: a row whose score against the query is NaN is
    never returned; the result is the exact top-k of the other rows by (score descending, position ascending), scores
    computed in float64 and rounded to fp32; unfilled tail slots are (-inf, -1).  -> (D [nq, k] fp32, I [nq, k] int64).
    Mirrors ivf_oracle.ivf_search_nonfinite; not through oracle.search.topk_desc, whose np.partition sorts NaN as the
    largest value."""
    xb64, xq64 = np.asarray(xb, dtype=np.float64), np.asarray(xq, dtype=np.float64)
    nq = xq64.shape[0]
    D = np.full((nq, k), -np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        with np.errstate(invalid="ignore", over="ignore"):
            s = (xb64 * xq64[q]).sum(axis=1) if xb64.shape[0] else np.zeros(0)
            s32 = s.astype(np.float32)
        keep = np.nonzero(~np.isnan(s32))[0]
        o = keep[np.lexsort((keep, -s32[keep].astype(np.float64)))[:k]]
        D[q, :len(o)] = s32[o]
        I[q, :len(o)] = o
    return D, I


def normalized_like_the_index(x):
    """amdrec_l2_normalize on a copy, as float32 numpy: x * (1 / sqrt(sum x^2)) for rows with sum x^2 > 0.  A row with an
    inf coordinate has sum = inf, factor 0: the inf becomes NaN (inf * 0) and every finite coordinate 0; a row with a NaN
    has sum = NaN, which is not > 0: it stays as it is."""
    x = np.array(x, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        ss = (x.astype(np.float64) ** 2).sum(axis=1)
        inv = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 1.0).astype(np.float32)
        return x * inv[:, None]


# ---- the sampled threshold of the generic and the fp32 corpus pass -------------------------------------------------------------
def sample_rows(p):
    """Corpus rows whose scores run_passes samples (not the streaming pass): n_sample / SAMPLE_G blocks of SAMPLE_G rows,
    gstride apart (DenseRows with gshift 8), rows past the corpus left out."""
    i = np.arange(p.n_sample)
    r = (i // SAMPLE_G) * p.gstride + i % SAMPLE_G
    return r[r < p.nrows]


def sampled_tau(sample_scores):
    """sample_threshold_kernel: float4 chunk c of a query's sample scores belongs to group c % 256; tau = the SAMPLE_RANK-th
    largest of the 256 group maxima (an empty group counts -inf)."""
    s = np.asarray(sample_scores, dtype=np.float64)
    gm = np.full(256, -np.inf)
    np.maximum.at(gm, (np.arange(len(s)) // 4) % 256, s)
    return np.sort(gm)[::-1][SAMPLE_RANK - 1]


def admitted(xb, xq, p, margin):
    """Per query the candidates a sampled generic / fp32 pass admits, from float64 scores: (at least, at most) with every
    score and tau itself moved by up to ``margin`` (the bf16 pass's error; 0 for the fp32 pass)."""
    s = xq.astype(np.float64) @ xb.astype(np.float64).T
    tau = np.array([sampled_tau(row[sample_rows(p)]) for row in s])
    return (s >= tau[:, None] + margin).sum(axis=1), (s >= tau[:, None] - margin).sum(axis=1)


# ---- the host plan ----------------------------------------------------------------------------------------------------------
class Plan(dict):
    __getattr__ = dict.__getitem__


def _align(n, a=256):
    return (n + a - 1) // a * a


def plan(nq, nrows, k, dim=0, mixed=None):
    """Python restatement of csrc/search.hip: make_plan (target, n_sample, nslices, the Carver layout -> bytes), scan_segments
    (nseg, seg_cap), sample_plan (sample_tiles), the pass choice of amdrec_flat_search_mixed (streaming), its finalize choice
    (FUSED_MAX_NQ, AMDREC_FINALIZE) and where ``search_threshold`` is launched.  ``dim`` = 0 or ``mixed`` = False: the plan of
    amdrec_flat_search.  Test documentation, not a second source of truth: the n_fixup and profile-tag assertions of
    tests/test_flat_surface_gpu.py and the byte counts of tests/test_flat_surface_cpu.py show where it and the library differ.
    overflow = keys per query the streaming pass must put into the overflow block when EVERY row is a hit (tau = -inf: a
    corpus of at most CAND_CAP rows): workgroup w owns the 128-row tiles w, w + nseg, ... and seg_cap slots."""
    mixed = bool(dim) if mixed is None else mixed
    dim16 = dim if mixed else 0
    p = Plan(nq=nq, nrows=nrows, k=k, dim=dim, mixed=mixed)
    t5 = k + 900
    if nq >= 256:
        lo = max((28 * k + 9) // 10, k + 256)
        t5 = min(t5, max(int(0.6 * np.sqrt(float(max(nrows, 1)))), lo))
    target = max(2 * k, t5)
    p.target = 0 if nrows <= CAND_CAP else target
    nt = (nrows + SAMPLE_G - 1) // SAMPLE_G
    if nrows <= CAND_CAP:
        p.n_sample, p.gstride = 0, SAMPLE_G
    else:
        st = min(max(((SAMPLE_RANK * nrows + target - 1) // target + SAMPLE_G - 1) // SAMPLE_G, 1), nt)
        p.n_sample, p.gstride = st * SAMPLE_G, nt // st * SAMPLE_G
    p.nslices = min(max(CAND_CAP // k, 1), 16)
    p.streaming = mixed and nrows > 0 and dim in FLAT_DIMS_STREAM
    ny = (nq + SCAN_QGROUP - 1) // SCAN_QGROUP
    ntiles = (nrows + SCAN_ROWS - 1) // SCAN_ROWS
    p.ny = ny
    p.nseg = max(1, min(max(256 // ny, 1), ntiles)) if p.streaming else 1
    p.seg_cap = CAND_CAP // p.nseg
    p.overflow = 0
    if p.streaming:
        last = nrows - (ntiles - 1) * SCAN_ROWS
        for w in range(p.nseg):
            mine = range(w, ntiles, p.nseg)
            own = sum(last if t == ntiles - 1 else SCAN_ROWS for t in mine)
            p.overflow += max(0, own - p.seg_cap)
    p.sample_tiles = ()
    if p.streaming and p.n_sample:
        full = nrows // SCAN_ROWS
        n_t = max(1, min((p.n_sample + SCAN_ROWS - 1) // SCAN_ROWS, full))
        p.sample_tiles = tuple(i * (full // n_t) for i in range(n_t))
    # launches: sampled streaming pass -> tau inside the corpus pass up to 8 queries; sampled generic / fp32 pass -> always
    p.threshold_launch = bool(p.n_sample) and (not p.streaming or nq > 8)
    if not mixed:
        p.finalize = "fp32"
    elif nq <= FUSED_MAX_NQ:
        p.finalize = "fused"
    elif p.target > 0 and 2 * p.target <= 1024:
        p.finalize = "mixed<128,1024>"
    elif p.target > 0 and 2 * p.target <= 2048:
        p.finalize = "mixed<256,2048>"
    else:
        p.finalize = "mixed<512,8192>"
    takes = [4 * nq] + [4 * nq] * 5 + [4 * (nq + 1)]                               # tau | cnt ocnt ticket fcount fticket | fail
    takes += [4 * 256 * nq if dim16 else 0, 8 * nq * CAND_CAP * (2 if dim16 else 1)]       # segcnt, cand (+ overflow block)
    takes += [4 * nq * p.n_sample, 8 * nq * p.nslices * k, 2 * nq * dim16]          # sample, fix-up slices, bf16 queries
    takes += [8 * CAND_CAP * (nq if dim16 and nq <= FUSED_MAX_NQ else 0)]           # fused finalize: re-scored keys
    p.bytes = sum(_align(b) for b in takes)
    return p
