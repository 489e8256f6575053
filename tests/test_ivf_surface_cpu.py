"""Self-checks of tests/ivf_oracle.py and of the input conditions the IVF-Flat surface tests (tests/test_ivf_surface_gpu.py)
rely on.  No GPU: numpy, and torch only for the seeded draw of amdrec.ivf's trainer."""
import numpy as np
import pytest

from tests import cases, ivf_oracle as io


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def test_score_tol_formula_and_its_relation_to_the_dim_256_constant():
    assert io.score_tol(256) == 258 * 2.0 ** -24
    assert io.score_tol(2048, 2.0, 3.0) == 2050 * 2.0 ** -24 * 6.0
    assert io.topk_tau(100) == 2 * io.score_tol(100)
    # the existing tests keep cases.SCORE_ATOL (set for unit vectors at dim 256, an observed level); the derived forward
    # bound at that dim is not below it, so no surface test asks for more than the existing ones do at 256
    assert io.score_tol(256) >= cases.SCORE_ATOL
    assert io.topk_tau(256) >= cases.TOPK_TAU
    assert 1.1e-4 < io.score_tol(2048) < 1.3e-4


@pytest.mark.parametrize("dim", sorted(set(io.SURFACE_DIMS) | set(io.ASSIGN_DIMS) | set(io.FILTER_BOUND_DIMS) | {256}))
def test_fp32_dot_products_in_two_orders_stay_inside_score_tol(dim):
    """numpy fp32 inner products of the seeded unit rows, one forward chain and one balanced tree, against float64."""
    x = io.clustered(400, dim, 20, 1)
    q = io.clustered(400, dim, 20, 2)
    ref = (x.astype(np.float64) * q.astype(np.float64)).sum(axis=1)
    tol = io.score_tol(dim, io.max_norm(q), io.max_norm(x))
    for f in (io.dot32_forward, io.dot32_pairwise):
        got = f(q, x)
        assert got.dtype == np.float32
        assert np.abs(got.astype(np.float64) - ref).max() <= tol
        assert np.abs(got - ref.astype(np.float32)).max() <= tol          # (the oracle's fp32 rounding is inside the + 2)
    # and with long rows and queries: the bound scales with both norms
    tol = io.score_tol(dim, 1e3 * io.max_norm(q), 1e-3 * io.max_norm(x))
    got = io.dot32_forward(1e3 * q, 1e-3 * x)
    ref = ((1e3 * q).astype(np.float32).astype(np.float64) * (1e-3 * x).astype(np.float32).astype(np.float64)).sum(axis=1)
    assert np.abs(got - ref).max() <= tol


def test_keys_round_trip_and_order():
    sc = np.array([1.5, -0.25, 0.0, -0.0, -np.inf, 3e-39, 7.0, 7.0], dtype=np.float32)
    pos = np.array([5, 0, 77, 3, 12, 1 << 31, 9, 8], dtype=np.int64)
    keys = io.make_keys(sc, pos)
    s2, p2 = io.decode_keys(keys)
    assert np.array_equal(s2.view(np.uint32), sc.view(np.uint32)) and np.array_equal(p2, pos)
    assert (keys != 0).all()
    order = np.argsort(keys)[::-1]
    # (score desc, position asc); -0.0 sorts just below +0.0
    assert order.tolist() == [7, 6, 0, 5, 2, 3, 1, 4]
    s0, p0 = io.decode_keys(np.zeros(2, dtype=np.uint64))
    assert np.isneginf(s0).all() and (p0 == -1).all()


# ---- amdrec_ivf_group ------------------------------------------------------------------------------------------------------
def test_group_reference_on_a_hand_example():
    probes = np.array([[2, 0, -1], [2, 5, 1], [0, 2, 2]])      # 5 >= nlist and -1: no list; list 1 is empty; list 3 unprobed
    g = io.group_reference(probes, nlist=4, list_len=[10, 0, 3, 8], qtile=2)
    assert g["pool_base"].tolist() == [[0, 3, 13], [0, 3, 3], [0, 10, 13]]
    assert g["pool_count"].tolist() == [13, 3, 16]
    assert g["group_off"].tolist() == [0, 2, 3, 7, 7]
    assert g["qtile_prefix"].tolist() == [0, 1, 2, 4, 4]
    assert g["members"].tolist() == [1, 6, 5, 0, 3, 7, 8]
    # a device result with another order inside the groups canonicalises to the same members
    pq, pp = np.array([2, 0, 1, 2, 0, 2, 1]), np.array([0, 1, 2, 2, 0, 1, 0])
    assert io.group_members(pq, pp, g["group_off"], 3).tolist() == g["members"].tolist()
    # one list, qtile 64: every valid probe in one group
    g1 = io.group_reference(np.array([[0, 0], [3, 0]]), 1, [7], 64)
    assert g1["group_off"].tolist() == [0, 3] and g1["qtile_prefix"].tolist() == [0, 1]
    assert g1["pool_base"].tolist() == [[0, 7], [0, 0]] and g1["pool_count"].tolist() == [14, 7]


# ---- the prefilter bound ---------------------------------------------------------------------------------------------------
def test_bf16_round_and_eps64():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.14159, 1e-20], dtype=np.float32)
    r = io.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == np.float32(1.015625)     # ties to even, both ways
    assert (r.view(np.uint32) & 0xFFFF == 0).all()
    assert (np.abs(r.astype(np.float64) - x) <= np.abs(x) * 2.0 ** -8).all()
    # header formula by hand: q = (3, 4), bf16(q) - q = (0.5, 0) -> |q| = 5, |dq| = 0.5
    q = np.array([[3.0, 4.0]])
    e = io.eps64(q, q + np.array([[0.5, 0.0]]), M=2.0, D=0.25)
    assert e[0] == 0.5 * 2.25 + 5 * 0.25 + 2 * 2 * 2.0 ** -24 * 5 * 2.25
    # and its stated worst case for real roundings: (2^-7 + 2^-16) |q| M + the accumulation term
    for dim in io.FILTER_BOUND_DIMS:
        qq = io.clustered(50, dim, 5, 3) * np.float32(7.0)
        M = 1.0
        e = io.eps64(qq, io.bf16_round(qq), M, M * 2.0 ** -8)
        qn = np.sqrt((qq.astype(np.float64) ** 2).sum(1))
        assert (e <= (2.0 ** -7 + 2.0 ** -16) * qn * M + 2 * dim * io.U * qn * M * (1 + 2.0 ** -8)).all()
        assert (e > 0).all()


# ---- assignment: the near-tie exemption cannot swallow a wrong kernel --------------------------------------------------------
@pytest.mark.parametrize("dim", io.ASSIGN_DIMS)
def test_assign_cases_have_few_float64_near_ties(dim):
    """The GPU test exempts a row from `assignment == float64 arg-max` when its two best float64 scores are closer than
    2 * score_tol: on these seeds the reference alone puts under 1 % of the rows there (and nlist 1 none at all)."""
    for nlist in io.ASSIGN_NLISTS:
        x, cent = io.assign_case(dim, nlist)
        assert x.shape == (io.ASSIGN_ROWS, dim) and cent.shape == (nlist, dim)
        best, top, gap = io.assign_reference(x, cent)
        tie = gap < 2 * io.score_tol(dim, io.max_norm(x), io.max_norm(cent))
        assert tie.mean() < 0.01, (dim, nlist, float(tie.mean()))
        if nlist == 1:
            assert not tie.any() and (best == 0).all()
        if nlist == 4096:
            assert nlist > len(x) and len(np.unique(best)) < nlist       # more centroids than rows: empty clusters exist


def test_assign_reference_rules():
    cent = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    x = np.array([[2.0, 1.0], [0.0, 3.0], [np.nan, 1.0], [1.0, 1.0]])
    best, top, gap = io.assign_reference(x, cent)
    assert best.tolist() == [0, 2, 0, 0]                       # tie -> lower centroid; no finite score -> list 0
    assert top[0] == 2.0 and gap[0] == 0.0 and gap[1] == 3.0 and np.isneginf(top[2])
    new, count, norm = io.kmeans_step_reference(x[[0, 1, 3]], best[[0, 1, 3]], cent)
    assert count.tolist() == [2, 0, 1]
    assert np.allclose(new[0], np.array([3.0, 2.0]) / np.sqrt(13.0)) and np.array_equal(new[1], cent[1])


def test_search_reference_with_non_finite_rows_ranks_them_last():
    xb = np.array([[1.0, 0.0], [np.nan, 0.0], [0.0, 1.0], [0.5, 0.5], [np.nan, np.nan]], dtype=np.float32)
    assign = np.array([0, 0, 1, 0, 0])
    D, I = io.ivf_search_nonfinite(xb, assign, 2, np.array([[1.0, 0.0]], dtype=np.float32), 5, np.array([[0, -1]]))
    assert I.tolist() == [[0, 3, 1, 4, -1]]
    assert D[0, :2].tolist() == [1.0, 0.5] and np.isneginf(D[0, 2:]).all()


# ---- training with non-finite rows: the trainer's seeded draw hits one of them -----------------------------------------------
def test_the_nan_rows_of_the_training_case_are_drawn_as_initial_centroids():
    """amdrec.ivf.InvertedLists.train seeds the centroids with the first nlist entries of a torch.randperm (CPU generator,
    seed 1234).  The GPU test puts a non-finite row exactly where that draw looks, so a trainer that copies it into the
    centroid table is caught."""
    torch = pytest.importorskip("torch")
    n, nlist = io.NAN_TRAIN_ROWS, io.NAN_TRAIN_NLIST
    assert n <= 256 * nlist                                    # no sub-sampling: the draw is over the rows as given
    drawn = io.initial_centroid_rows(torch, n, nlist)
    bad = io.nan_train_bad_rows(torch)
    assert len(drawn) == nlist and len(set(bad) & set(drawn)) >= 2 and len(set(bad) - set(drawn)) >= 1


@pytest.mark.parametrize("dim", io.SURFACE_DIMS)
def test_the_long_layout_of_the_surface_corpus_has_a_list_past_the_short_row_tile_limit(dim):
    """With the generating centres as the quantizer, float64 arg-max files more than 1536 rows in one list (the grouped
    scan's 256-row tiles) - far enough past it that fp32 near-ties cannot bring it back under."""
    xb, centres = io.surface_corpus(dim, "long", 32)
    best, _, gap = io.assign_reference(xb, centres)
    lens = np.bincount(best, minlength=32)
    near = int((gap < 2 * io.score_tol(dim, io.max_norm(xb), io.max_norm(centres))).sum())
    assert lens.max() - near > 1536, (lens.max(), near)
    xs, _ = io.surface_corpus(dim, "short", 32)
    assert len(xs) == io.surface_rows(dim) and len(xs) // 32 < 1536 // 4
