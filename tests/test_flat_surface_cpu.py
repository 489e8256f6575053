"""CPU: the helpers of the flat-search surface tests (tests/flat_oracle.py) are what they claim to be - the non-finite
contract equals the oracle on finite inputs and the hand-made lists on others; plan() answers the byte counts of the
library's own workspace queries (host-only calls); the seeded inputs of tests/test_flat_surface_gpu.py leave check_topk's
near-tie band almost nothing to excuse; and the tolerances are where fp32 summation puts them."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle
from tests import cases
from tests import flat_oracle as fo
from tests import ivf_oracle as io


# ---- flat_search_nonfinite ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,k,dim", [(500, 7, 20, 12), (300, 3, 300, 8), (40, 5, 100, 36), (1, 2, 3, 4), (2000, 4, 1, 64)])
def test_nonfinite_contract_equals_the_oracle_on_finite_inputs(n, nq, k, dim):
    """Bit for bit, k > n and duplicated rows (equal scores: lower position first) included."""
    xb, xq = fo.rows(n, dim, 3, "lifted"), fo.rows(nq, dim, 4, "lifted")
    if n >= 40:
        xb[n // 2:n // 2 + 10] = xb[:10]                               # duplicates
        xb[n - 3:] = xb[5]
    D, I = fo.flat_search_nonfinite(xb, xq, k)
    rD, rI = oracle.search.flat_ip_search(xb, xq, k, dtype=np.float64)
    assert np.array_equal(I, rI) and np.array_equal(D.view(np.uint32), rD.view(np.uint32))
    assert D.dtype == np.float32 and I.dtype == np.int64 and (I[:, min(k, n):] == -1).all()


def test_nonfinite_contract_on_hand_made_rows():
    nan, inf = np.nan, np.inf
    xb = np.array([[1, 0, 0, 0],            # 0
                   [nan, nan, nan, nan],    # 1: never returned
                   [0.5, 0, nan, 0],        # 2: NaN against every query (NaN * 0 = NaN)
                   [inf, 0, 0, 0],          # 3: +inf, -inf or NaN (inf * 0) by the query's first coordinate
                   [0, 1, 0, 0],            # 4
                   [1, 0, 0, 0]],           # 5: duplicate of row 0
                  dtype=np.float32)
    xq = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-1, 0.5, 0, 0], [nan, 0, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    D, I = fo.flat_search_nonfinite(xb, xq, 4)
    assert I.tolist() == [[3, 0, 5, 4], [4, 0, 5, -1], [4, 0, 5, 3], [-1, -1, -1, -1], [0, 4, 5, -1]]
    assert D[0].tolist() == [inf, 1, 1, 0] and D[1].tolist() == [1, 0, 0, -inf] and D[2].tolist() == [0.5, -1, -1, -inf]
    assert np.isneginf(D[3]).all() and D[4].tolist() == [0, 0, 0, -inf]
    D, I = fo.flat_search_nonfinite(xb[:0], xq, 2)
    assert (I == -1).all() and np.isneginf(D).all()


def test_normalisation_statement_turns_an_inf_row_into_one_nan_and_zeros():
    x = np.array([[3, 4, 0, 0], [np.inf, 1, 2, 3], [1, 2, 3, -np.inf], [1, np.nan, 1, 1], [0, 0, 0, 0]], dtype=np.float32)
    y = fo.normalized_like_the_index(x)
    assert y[0].tolist() == pytest.approx([0.6, 0.8, 0, 0]) and y[4].tolist() == [0, 0, 0, 0]
    assert np.isnan(y[1, 0]) and y[1, 1:].tolist() == [0, 0, 0] and np.isnan(y[2, 3]) and y[2, :3].tolist() == [0, 0, 0]
    assert np.array_equal(np.isnan(y[3]), [False, True, False, False]) and y[3, 0] == 1


# ---- plan() against the library's own layout ------------------------------------------------------------------------------------
def _ask(fn, *args):
    from amdrec import _lib
    n = C.c_size_t(0)
    assert fn(*args, C.byref(n)) == 0, _lib.load().amdrec_last_error()
    return n.value


def test_plan_answers_the_workspace_bytes_of_both_entry_points():
    """make_plan's layout restated: n_sample (sample buffer), nslices (fix-up slices), the fused finalize's re-scored key
    block, the mixed-only buffers - over the nq edges x corpus sizes on both sides of CAND_CAP x k x dim of every case."""
    from amdrec import _lib
    lib = _lib.load()
    nqs = fo.NQ_EDGES + (3, 5, 70, 130, 200, 1100, 2600)
    nrows = (0, 777, 3000, 8000, 8192, 8193, 9000, 12_000, 20_000, 1_000_000)
    ks = (1, 10, 50, 64, 100, 300, 500, 2048)
    for nq, n, k in itertools.product(nqs, nrows, ks):
        assert fo.plan(nq, n, k).bytes == _ask(lib.amdrec_flat_search_workspace, nq, n, k), (nq, n, k)
        for dim in (8, 32, 72, 256, 2048):
            assert fo.plan(nq, n, k, dim).bytes == _ask(lib.amdrec_flat_search_mixed_workspace, nq, n, k, dim), (nq, n, k, dim)


def test_plan_names_the_paths_the_gpu_cases_are_written_for():
    # (c): the finalize shapes, behind the streaming and the generic pass alike
    for dim in fo.FINALIZE_DIMS:
        for (nq, k), shape in fo.FINALIZE_SHAPES.items():
            p = fo.plan(nq, fo.FINALIZE_ROWS, k, dim)
            assert p.finalize == shape and p.n_sample > 0 and p.streaming == (dim == 128), (dim, nq, k)
            assert (p.nseg, p.seg_cap) == ((157, 52) if dim == 128 else (1, fo.CAND_CAP))
    assert fo.plan(128, 20_000, 50, 64).finalize == "fused" and fo.plan(64, 20_000, 50).finalize == "fp32"
    # (b): the threshold launch appears at 9 queries behind the streaming pass, and is always there behind the others
    assert not fo.plan(8, 20_000, 50, 64).threshold_launch and fo.plan(9, 20_000, 50, 64).threshold_launch
    assert fo.plan(1, 20_000, 50, 72).threshold_launch and fo.plan(1, 20_000, 50).threshold_launch
    assert not fo.plan(9, 8192, 50, 64).threshold_launch
    assert fo.plan(255, 20_000, 50, 64).target == 950 and fo.plan(256, 20_000, 50, 64).target == 306
    assert fo.plan(512, 20_000, 50, 64).nseg == 157 and fo.plan(513, 20_000, 50, 64).nseg == 128
    # (d): segments, slots and the keys per query that must travel through the overflow block
    want = {(8192, 1100): (64, 128, 0), (8192, 2600): (42, 195, 22 * 61), (8000, 1100): (63, 130, 0),
            (8000, 2600): (42, 195, 20 * 61), (777, 1100): (7, 1170, 0), (777, 2600): (7, 1170, 0)}
    for (n, nq), (nseg, seg_cap, overflow) in want.items():
        p = fo.plan(nq, n, 10, fo.SMALL_DIM)
        assert (p.nseg, p.seg_cap, p.overflow) == (nseg, seg_cap, overflow) and p.n_sample == 0 and p.target == 0, (n, nq)
        assert p.finalize == "mixed<512,8192>" and p.overflow <= fo.OVERFLOW_MAX
    # the k = 2048 case
    p = fo.plan(130, 9000, 2048, 2048)
    assert p.nslices == 4 and p.finalize == "mixed<512,8192>" and fo.plan(3, 9000, 2048, 2048).finalize == "fused"


def test_k_2048_case_is_served_by_the_main_path():
    """d = 2048, k = 2048 on 9000 rows: the plan samples ONE 256-row block (rows 0 .. 255) and takes the 64th largest of 64
    group maxima of four consecutive scores - a low threshold.  From the float64 scores, with every score and the threshold
    moved by 0.02 (more than the bf16 pass's 2^-7 |q| |x| twice over; 1e-5 for the fp32 pass), every query admits at least k
    rows and at most CAND_CAP under either engine: no query may take the fix-up, which the GPU case asserts."""
    c = fo.kmax_case()
    xb, xq = fo.case_inputs(c)
    for nq in c["prefixes"]:
        for mixed in (True, False):
            p = fo.plan(nq, c["n"], c["k"], c["dim"], mixed)
            assert p.n_sample == 256 and not p.streaming and np.array_equal(fo.sample_rows(p), np.arange(256))
            lo, hi = fo.admitted(xb, xq[:nq], p, 0.02 if mixed else 1e-5)
            assert lo.min() >= 2 * c["k"] and hi.max() <= fo.CAND_CAP - 900, (nq, mixed, int(lo.min()), int(hi.max()))
    s = np.arange(1024, dtype=np.float64)
    assert fo.sampled_tau(s) == 4 * (255 - 63) + 3 and fo.sampled_tau(s[:256]) == 3 and fo.sampled_tau(s[:252]) == -np.inf


def test_nonfinite_placements_visit_every_place_with_every_kind():
    n = fo.NONFINITE_ROWS
    seen = {(kind, place) for r in range(4) for kind, place in fo.nonfinite_positions(n, r).items()}
    assert len(seen) == 16 and {p for _, p in seen} == {0, n // 2, n - n % fo.SCAN_ROWS + 1, n - 1}
    assert n - n % fo.SCAN_ROWS + 1 > (n // fo.SCAN_ROWS) * fo.SCAN_ROWS       # inside the partial last tile


def test_no_small_corpus_overflows_past_the_limit():
    """Why the over-limit case of (d) is a sampled corpus: with every row a candidate, the most a query's workgroups spill
    is 1342 keys (8192 rows, six query groups), whatever the query count."""
    worst = max((fo.plan(fo.SCAN_QGROUP * ny, n, 10, fo.SMALL_DIM).overflow, n, ny)
                for ny in range(1, 258) for n in range(64, fo.CAND_CAP + 1, 64))
    assert worst == (1342, 8192, 6)
    xb, xq, k, hot_tiles, overflow = fo.overflow_case()
    assert overflow == 2280 > fo.OVERFLOW_MAX
    hot = np.zeros(len(xb), bool)
    for t in hot_tiles:
        hot[t * fo.SCAN_ROWS:(t + 1) * fo.SCAN_ROWS] = True
    s = xq.astype(np.float64) @ xb.astype(np.float64).T
    # every hot row beats every cold row by far more than bf16 resolves (2^-7 of a unit score) for every query ...
    assert s[:, hot].min() > 0.0 and s[:, ~hot].max() < -0.17
    # ... so a threshold that admits the expected ~900 of 16,160 cold rows admits all 3840 hot ones, and the count fits
    assert hot.sum() + 4 * fo.plan(len(xq), len(xb), k, fo.SMALL_DIM).target < fo.CAND_CAP
    assert not fo.loose_queries(xb, xq, k, cases.TOPK_TAU).any()


# ---- the inputs are fit for purpose ---------------------------------------------------------------------------------------------
def _id(c):
    return f"{c['group']}-d{c['dim']}-n{c['n']}-q{c['nq']}-k{c['k']}"


@pytest.mark.parametrize("c", fo.seeded_cases(), ids=_id)
def test_seeded_cases_leave_the_near_tie_band_nearly_empty(c):
    """For every query count the case is searched with: at most 2 % of the queries have a row outside the float64 top-k
    within TOPK_TAU (scaled for un-normalised rows) of the k-th score - the rows check_topk would accept in its place."""
    if c["group"] == "f":
        xb, xq, scale = fo.stride_inputs(c["dim"])
    else:
        (xb, xq), scale = fo.case_inputs(c), 1.0
    assert xb.shape == (c["n"], c["dim"]) and xq.shape == (c["nq"], c["dim"]) and xb.dtype == np.float32
    if c["group"] != "f":
        assert np.abs(np.linalg.norm(xb.astype(np.float64), axis=1) - 1).max() < 1e-6
    loose = fo.loose_queries(xb, xq, c["k"], fo.topk_tau(scale))
    for nq in c["prefixes"]:
        assert loose[:nq].sum() <= 0.02 * nq, (nq, int(loose[:nq].sum()))


def test_lifted_rows_use_every_coordinate():
    """The lift is dense: a K loop that stopped early would lose signal in every row (no coordinate block is idle)."""
    x = fo.rows(2000, 2048, 1, "lifted")
    energy = (x.astype(np.float64) ** 2).reshape(2000, 8, 256).sum(axis=2)
    assert energy.min() > 0.02 and np.abs(energy.mean(axis=0) - 0.125).max() < 0.01


# ---- tolerances -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sorted(fo.FP32_DEVIATION))
def test_fp32_summation_figures_and_the_rule_for_a_wider_tolerance(dim):
    """Every query of the surface case against its 100 best rows, fp32 in one forward chain and in a balanced tree, against
    float64: the figures recorded in flat_oracle.FP32_DEVIATION are the measured ones; a forward chain - the order of
    amdrec_flat_search's MFMA pass - leaves SCORE_ATOL at these dimensions and a balanced tree stays four times inside it;
    the fp32 engine's tolerance is 4 x the larger figure, under the derived bound; the mixed engine's is SCORE_ATOL."""
    c = fo.surface_case(dim, fo.surface_rows(dim), 100)
    xb, xq = fo.case_inputs(c)
    _, I = fo.reference(xb, xq, 100)
    q, x = np.repeat(xq, 100, axis=0), xb[I.reshape(-1)]
    fwd, tree = fo.fp32_sum_deviation(q, x)
    rec = fo.FP32_DEVIATION[dim]
    assert 0.9 * rec[0] <= fwd <= rec[0] and 0.9 * rec[1] <= tree <= rec[1], (fwd, tree)
    assert tree <= cases.SCORE_ATOL / 4 and fwd > cases.SCORE_ATOL
    assert fo.score_tol(dim, engine="fp32") == pytest.approx(4 * max(rec)) and fo.score_tol(dim, engine="fp32") <= io.score_tol(dim)
    assert fo.score_tol(dim) == cases.SCORE_ATOL and fo.score_tol(dim, 3.0) == 3 * cases.SCORE_ATOL


def test_no_other_dimension_has_a_wider_tolerance():
    assert sorted(fo.SCORE_TOL_BY_DIM) == [512, 1000, 2048] == sorted(fo.FP32_DEVIATION)
    for dim in fo.FLAT_DIMS:
        if dim not in fo.SCORE_TOL_BY_DIM:
            assert fo.score_tol(dim, engine="fp32") == cases.SCORE_ATOL
