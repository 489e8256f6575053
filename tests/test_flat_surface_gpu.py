"""The flat inner-product search (csrc/search.hip) across what its entry points accept, against float64 rounded to fp32
(tests/flat_oracle.py has the tables, the seeded inputs, the tolerances and plan(), the restated host dispatch):
(a) every dimension kind - streaming, generic bf16 tiles, fp32-only - under both prefilters, on a corpus where every row is a
candidate and on a sampled one; (b) the query counts at which the dispatch switches; (c) the finalize shapes behind both
kinds of corpus pass; (d) small corpora under many query groups, where candidates must travel through the overflow block;
(e) non-finite rows and queries; (f) the C entry points with padded leading dimensions on a poisoned private workspace.
Every case asserts n_fixup: a main path that always gave up would otherwise pass unseen through the exact fix-up scan."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib
from tests import flat_oracle as fo

pytestmark = pytest.mark.gpu


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(t, ld, fill=float("nan")):
    """A [rows][ld] buffer whose first t.shape[1] columns are t and the rest ``fill``."""
    p = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    p[:, :t.shape[1]] = t
    return p


def _index(xb, prefilter, ad_ids=None):
    from amdrec.index import FAISSIndex
    dim = xb.shape[1]
    idx = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    assert idx._mixed == (prefilter == "bf16" and dim % 8 == 0)
    idx.add(xb, ad_ids)
    return idx


def _normalized(idx, x):
    """x as the index normalises it (amdrec_l2_normalize) -> device fp32."""
    return idx._normalize_(idx._to_device_f32(x))


def _search(idx, qn, k, profile=False, positions=False):
    """FAISSIndex.search_device on normalised queries -> (ids or positions, scores, n_fixup of the C call - through the
    index's n_fixup_out hook -, the engine that ran, profile tags)."""
    idx.n_fixup_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    tags = None
    try:
        if profile:
            _lib.profile_enable(True)
        ids, D = idx.search_device(qn, k, normalize=False, return_positions=positions)
        torch.cuda.synchronize()
        if profile:
            tags = {t: int(e["launches"]) for t, e in _lib.profile_report().items()}
    finally:
        nfix, idx.n_fixup_out = int(idx.n_fixup_out.item()), None
        if profile:
            _lib.profile_enable(False)
    assert nfix >= 0, "the search did not report n_fixup"
    return ids.cpu().numpy(), D.cpu().numpy(), nfix, "mixed" if idx._mixed else "fp32", tags


def _check(xb, xq, rD, rI, D, I, dim, engine, scale=1.0, offset=0, record=None):
    """A result of ``engine`` against the float64 reference (rD, rI) of rows xb and queries xq: check_topk with the near-tie
    band and the score tolerance of flat_oracle, every returned position's score that row's own."""
    tol = fo.score_tol(dim, scale, engine)
    q64 = xq.astype(np.float64)
    oracle.search.check_topk(rD, np.where(rI >= 0, rI + offset, -1), D, I, tau=fo.topk_tau(scale), score_tol=tol,
                             scores_of=lambda qi, ids: (xb[np.asarray(ids) - offset].astype(np.float64) @ q64[qi]).astype(np.float32))
    assert np.array_equal(I >= 0, np.isfinite(D))
    if record is not None:
        fin = np.isfinite(rD)
        record[0](record[1], record[2], float(np.abs(D[fin] - rD[fin]).max(initial=0.0)) / tol, bound=tol)


class _Case:
    """A seeded case on the device: the index, its stored rows and normalised queries on the host, the float64 reference
    for all queries - computed once, sliced by the query prefixes."""

    def __init__(self, c, prefilter):
        xb, xq = fo.case_inputs(c)
        self.c, self.idx = c, _index(xb, prefilter)
        self.qn = _normalized(self.idx, xq)
        self.xb, self.xq = self.idx._xb[:c["n"]].cpu().numpy(), self.qn.cpu().numpy()
        self.rD, self.rI = fo.reference(self.xb, self.xq, c["k"])

    def run(self, nq, profile=False, record=None):
        """Search with the first nq queries; exact, and every query through the main path -> (engine, profile tags)."""
        c = self.c
        ids, D, nfix, engine, tags = _search(self.idx, self.qn[:nq].contiguous(), c["k"], profile)
        _check(self.xb, self.xq[:nq], self.rD[:nq], self.rI[:nq], D, ids, c["dim"], engine, record=record)
        return nfix, engine, tags


# ---- (a) the dimension surface ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
@pytest.mark.parametrize("dim", fo.FLAT_DIMS)
def test_every_dimension_under_both_prefilters(dim, prefilter, accuracy):
    """dim / 4 float4 chunks of the fp32 kernels, dim / 8 of the bf16 shadow viewed as floats: under one K-step of the GEMM
    core (4 .. 24), a partial last K-step (36, 72, 100, 136, 1000), past 256 (fixup_kernel's qv, query_eps, rescore_keys
    and the finalize kernels' dim * 4 LDS tail as run-time loop bounds) up to the limit; a corpus of 3000 rows (every row a
    candidate, no sampling) and a sampled one; 5 / 70 / 200 queries (the three GEMM query tiles; fused and one-workgroup
    finalize); k = 1 on isotropic rows and k = 100 on lifted ones.  The fp32-only dims run amdrec_flat_search under either
    prefilter."""
    mixed = prefilter == "bf16" and dim not in fo.FLAT_DIMS_FP32_ONLY
    for n in (fo.SURFACE_SMALL_ROWS, fo.surface_rows(dim)):
        for k in fo.SURFACE_KS:
            case = _Case(fo.surface_case(dim, n, k), prefilter)
            assert case.idx._mixed == mixed
            for nq in fo.SURFACE_NQ:
                p = fo.plan(nq, n, k, dim, mixed)
                assert (p.n_sample > 0) == (n > fo.CAND_CAP) and p.streaming == (mixed and dim in fo.FLAT_DIMS_STREAM)
                nfix, engine, _ = case.run(nq, record=(accuracy, f"flat/surface/d{dim}", f"{prefilter}_n{n}_k{k}_q{nq}"))
                assert engine == ("mixed" if mixed else "fp32") and nfix == 0, (n, k, nq, nfix)


@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
def test_dim_2048_with_k_2048(prefilter):
    """k = AMDREC_MAX_K at the largest dimension, 3 and 130 queries: four fix-up slices, the fused and the general finalize
    with the largest dim * 4 LDS tail.  The plan takes its threshold from one 256-row sample block; that it admits between
    4391 and 7238 rows for every query under either engine is shown from the float64 scores in
    tests/test_flat_surface_cpu.py (test_k_2048_case_is_served_by_the_main_path), so no query may take the fix-up: the
    finalize kernels themselves produce these 2048-long lists."""
    c = fo.kmax_case()
    case = _Case(c, prefilter)
    for nq in c["prefixes"]:
        p = fo.plan(nq, c["n"], c["k"], c["dim"], case.idx._mixed)
        assert p.nslices == 4 and p.finalize == {("bf16", 3): "fused", ("bf16", 130): "mixed<512,8192>"}.get((prefilter, nq), "fp32")
        nfix, _, _ = case.run(nq)
        assert nfix == 0, (nq, nfix)


# ---- (b) batch-size edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", fo.EDGE_DIMS)
def test_query_count_edges_mixed_engine(dim):
    """1 .. 513 queries at every streaming dim and a generic one: tau inside the corpus pass or from its own launch (8 / 9;
    read from the profile tags), the GEMM query tiles (32 / 33, 64 / 65), the work split of scan_filter_kernel (qsh 0 .. 3),
    the fused or the one-workgroup finalize (128 / 129), make_plan's target (255 / 256) and a second query group, which
    halves the segments (512 / 513)."""
    case = _Case(fo.edge_case(dim), "bf16")
    for nq in fo.NQ_EDGES:
        p = fo.plan(nq, fo.EDGE_ROWS, fo.EDGE_K, dim)
        nfix, engine, tags = case.run(nq, profile=True)
        assert engine == "mixed" and nfix == 0, (nq, nfix)
        assert ("search_threshold" in tags) == p.threshold_launch, (nq, tags)
        assert ("search_filter_stream128x512_bf16" in tags) == ("search_sample_max128x512_bf16" in tags) == p.streaming, (nq, tags)
        assert tags["search_finalize_mixed"] == 1 and tags["search_fixup"] == 1, (nq, tags)
    assert _lib.profile_report() == {}


@pytest.mark.parametrize("dim", fo.EDGE_DIMS_FP32)
def test_query_count_edges_fp32_engine(dim):
    """amdrec_flat_search at its query-tile edges (32 / 33, 64 / 65) and past 128, at a streaming, a generic and an fp32-only
    dimension."""
    case = _Case(fo.edge_case(dim), "fp32")
    for nq in fo.NQ_EDGES_FP32:
        nfix, engine, tags = case.run(nq, profile=True)
        assert engine == "fp32" and nfix == 0, (nq, nfix)
        assert "search_threshold" in tags and "search_finalize_mixed" not in tags, (nq, tags)


# ---- (c) finalize shapes behind both pass kinds -------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,k", list(fo.FINALIZE_SHAPES))
@pytest.mark.parametrize("dim", fo.FINALIZE_DIMS)
def test_finalize_shapes_behind_the_streaming_and_the_generic_pass(dim, nq, k):
    """finalize_mixed_kernel<128, 1024>, <256, 2048> and <512, 8192> reading the streaming pass's 157 segments of 52 slots
    (d = 128) and the generic pass's single segment (nseg = 1, seg_cap = CAND_CAP, segcnt = the filter's counters; d = 72 and
    136).  Which shape a case takes is flat_oracle.plan's word (tests/test_flat_surface_cpu.py); that the shape itself
    produced the result is n_fixup == 0."""
    p = fo.plan(nq, fo.FINALIZE_ROWS, k, dim)
    assert p.finalize == fo.FINALIZE_SHAPES[(nq, k)] and (p.nseg == 1) == (dim != 128)
    nfix, engine, _ = _Case(fo.finalize_case(dim, nq, k), "bf16").run(nq)
    assert engine == "mixed" and nfix == 0, nfix


# ---- (d) small corpus, many query groups ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", fo.SMALL_KS)
@pytest.mark.parametrize("nq", fo.SMALL_NQ)
@pytest.mark.parametrize("n", fo.SMALL_ROWS)
def test_small_corpus_under_many_query_groups(n, nq, k):
    """Every row is a candidate (tau = -inf) and three or six 512-query groups share the 256 workgroups of the streaming
    pass.  Segments x slots and the keys per query that must go through the overflow block, from flat_oracle.plan:
    8192 rows: 3 groups 64 x 128, none; 6 groups 42 x 195, 22 workgroups own two tiles: 22 * 61 = 1342 keys.
    8000 rows: 3 groups 63 x 130, none; 6 groups 42 x 195, 20 workgroups own two full tiles: 1220 keys.
    777 rows: 7 x 1170, none.  All under the 2048-key limit: exact without a single fix-up."""
    p = fo.plan(nq, n, k, fo.SMALL_DIM)
    assert p.streaming and p.n_sample == 0 and p.overflow == {(8192, 2600): 1342, (8000, 2600): 1220}.get((n, nq), 0)
    nfix, engine, _ = _Case(fo.small_case(n, nq, k), "bf16").run(nq)
    assert engine == "mixed" and nfix == 0, nfix


def test_overflow_past_its_limit_sends_every_query_to_the_fixup():
    """flat_oracle.overflow_case: 30 tiles hold every row any query scores above 0, each fills its workgroup's 52 slots and
    spills 76 keys - 2280 per query, past the 2048 the finalize accepts - while the candidate count stays inside CAND_CAP:
    every query must report the fix-up, and the result is still exact."""
    xb, xq, k, hot_tiles, overflow = fo.overflow_case()
    assert overflow > fo.OVERFLOW_MAX
    idx = _index(xb, "bf16")
    qn = _normalized(idx, xq)
    ids, D, nfix, engine, _ = _search(idx, qn, k)
    xbn, q = idx._xb[:len(xb)].cpu().numpy(), qn.cpu().numpy()
    rD, rI = fo.reference(xbn, q, k)
    _check(xbn, q, rD, rI, D, ids, fo.SMALL_DIM, engine)
    assert engine == "mixed" and nfix == len(xq), nfix
    assert np.isin(ids // fo.SCAN_ROWS, hot_tiles).all()


# ---- (e) non-finite rows and queries --------------------------------------------------------------------------------------------
def _check_nonfinite(xb, xq, k, D, I, dim, engine, scale=1.0):
    rD, rI = fo.flat_search_nonfinite(xb, xq, k)
    assert not np.isnan(D).any()
    _check(np.nan_to_num(xb), xq, rD, rI, D, I, dim, engine, scale)
    return rD, rI


@pytest.mark.parametrize("rotation", range(4))
@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
@pytest.mark.parametrize("dim", fo.NONFINITE_DIMS)
def test_non_finite_rows_are_never_returned(dim, prefilter, rotation):
    """An all-NaN row, a row with one NaN, a row with +inf in coordinate 0 and one with -inf in its last coordinate at row
    0, in the middle, in the last, partial 128-row tile and as the very last row - rotated so that every kind visits every
    place (an all-NaN row among the clamped loads of the last tile, ...) - through FAISSIndex.add: amdrec_l2_normalize
    leaves the NaN rows as they are and turns an inf coordinate into NaN and the rest of its row into 0 (sum of squares
    inf, factor 1 / inf = 0) - asserted on the stored rows.  All four score NaN against every query and are never
    returned; the result is flat_search_nonfinite of the stored rows.  The mixed engine's max_norm is NaN, so every query
    takes the exact scan (n_fixup == nq); the fp32 engine needs none."""
    c = fo.nonfinite_case(dim)
    xb, xq = fo.case_inputs(c)
    xb, at = fo.with_nonfinite_rows(xb, rotation)
    idx = _index(xb, prefilter)
    stored = idx._xb[:c["n"]].cpu().numpy()
    want = fo.normalized_like_the_index(xb)
    assert np.array_equal(np.isnan(stored), np.isnan(want)) and np.isnan(stored).sum() == dim + 3 and not np.isinf(stored).any()
    for name in ("pos_inf_first", "neg_inf_last"):
        row = stored[at[name]]
        assert np.isnan(row).sum() == 1 and (row[~np.isnan(row)] == 0).all(), name
    assert np.isnan(stored[at["pos_inf_first"], 0]) and np.isnan(stored[at["neg_inf_last"], -1])
    fin = np.isfinite(stored).all(axis=1)
    assert np.abs(stored[fin] - want[fin]).max() <= 1e-6
    if idx._mixed:
        assert torch.isnan(idx._maxnorm[0]).item()
    qn = _normalized(idx, xq)
    ids, D, nfix, engine, _ = _search(idx, qn, c["k"])
    _check_nonfinite(stored, qn.cpu().numpy(), c["k"], D, ids, dim, engine)
    assert not np.isin(ids, list(at.values())).any() and (ids >= 0).all()
    assert nfix == (c["nq"] if engine == "mixed" else 0), (engine, nfix)


@pytest.mark.parametrize("custom_ids", [False, True])
@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
def test_unfilled_slots_read_the_last_id_with_default_and_custom_ids(prefilter, custom_ids, tmp_path):
    """300 rows of which 250 are NaN, k = 100 <= n: 50 slots are filled and 50 are not.  The unfilled ones carry -inf and the
    id ``id_map[-1]`` - what the reference wrapper's ``id_map[I]`` and the oracle's FlatIndex give for I = -1 - whether the
    ids are the default arange (no remap launch) or custom (amdrec_remap_ids); positions stay -1."""
    n, k, dim = 300, 100, 64
    xb, xq = fo.rows(n, dim, 11, "lifted"), fo.rows(7, dim, 12, "lifted")
    bad = np.random.default_rng(13).permutation(n)[:250]
    xb[bad] = np.nan
    id_map = (np.arange(n) * 7 + 1000) if custom_ids else np.arange(n)
    idx = _index(xb, prefilter, id_map.tolist() if custom_ids else None)
    assert idx._identity == (not custom_ids)
    rD, rI = fo.flat_search_nonfinite(idx._xb[:n].cpu().numpy(), _normalized(idx, xq).cpu().numpy(), k)
    assert (rI[:, :50] >= 0).all() and (rI[:, 50:] == -1).all()
    want = id_map[rI]                                              # numpy's -1 is Python's: the last id
    assert (want[:, 50:] == id_map[-1]).all()
    ids, D = idx.search(xq, k)
    assert np.array_equal(ids, want) and np.abs(D[:, :50] - rD[:, :50]).max() <= fo.score_tol(dim) and np.isneginf(D[:, 50:]).all()
    ids_d, _ = idx.search_device(_dev(xq), k)
    pos_d, _ = idx.search_device(_dev(xq), k, return_positions=True, pos_offset=5000)
    assert np.array_equal(ids_d.cpu().numpy(), want)
    assert np.array_equal(pos_d.cpu().numpy(), np.where(rI >= 0, rI + 5000, -1))
    # a loaded index knows its NaN rows as the one that add() built
    from amdrec.index import FAISSIndex
    path = str(tmp_path / "nan_rows.bin")
    idx.save(path)
    idx2 = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    idx2.load(path)
    assert idx._nonfinite and idx2._nonfinite and idx2._identity == idx._identity
    ids2, D2 = idx2.search(xq, k)
    assert np.array_equal(ids2, want) and np.array_equal(D2.view(np.uint32), D.view(np.uint32))


@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
@pytest.mark.parametrize("dim", [64, 72])
def test_a_nan_query_and_a_zero_query_among_ordinary_ones(dim, prefilter):
    """A query with a NaN scores NaN against every row: nothing is returned (-1 / -inf in all k slots).  An all-zero query
    (left as it is by the normalisation) scores 0 against every row: an ordinary result, the k lowest positions at score
    0.  The queries around them are unaffected."""
    c = fo.nonfinite_case(dim)
    xb, xq = fo.case_inputs(c)
    xq = xq[:12].copy()
    xq[3, dim // 2] = np.nan
    xq[8] = 0
    idx = _index(xb, prefilter)
    qn = _normalized(idx, xq)
    q = qn.cpu().numpy()
    assert np.isnan(q[3]).any() and (q[8] == 0).all()
    pos, D, nfix, engine, _ = _search(idx, qn, c["k"], positions=True)
    stored = idx._xb[:c["n"]].cpu().numpy()
    _check_nonfinite(stored, q, c["k"], D, pos, dim, engine)
    assert (pos[3] == -1).all() and np.isneginf(D[3]).all()
    assert np.array_equal(pos[8], np.arange(c["k"])) and (D[8] == 0).all()
    assert 1 <= nfix <= 2, nfix                                       # the NaN query; the zero query's 20,000-way tie may
    # As ids: no stored row is non-finite, so the default-id path does not look for unfilled slots (that would cost every
    # search a launch) and the NaN query's slots read -1; custom ids go through amdrec_remap_ids and read ids[n - 1].
    # Documented in search_device; pinned here so that it cannot move unseen.  Every other query agrees on both paths.
    assert not idx._nonfinite
    ids, _ = idx.search_device(qn, c["k"], normalize=False)
    assert np.array_equal(ids.cpu().numpy(), pos)
    id_map = np.arange(c["n"]) * 3 + 50
    idc = _index(xb, prefilter, id_map.tolist())
    ids_c, D_c = idc.search_device(qn, c["k"], normalize=False)
    ids_c = ids_c.cpu().numpy()
    assert (ids_c[3] == id_map[-1]).all() and np.array_equal(np.delete(ids_c, 3, 0), id_map[np.delete(pos, 3, 0)])
    assert np.array_equal(D_c.cpu().numpy().view(np.uint32), D.view(np.uint32))


@pytest.mark.parametrize("engine", ["mixed", "fp32"])
def test_c_entries_with_nan_coordinates_in_unnormalised_rows(engine):
    """The C entry points on rows as they are (norms 0.5 .. 2, no normalisation), NaN coordinates only: an all-NaN row, rows
    with one NaN at row 0, in the middle, in the last partial tile and at the end."""
    from amdrec.index import flat_search, flat_search_mixed
    dim, k = 72, 50
    xb, xq, scale = fo.stride_inputs(dim)
    n, nq = len(xb), 40
    xq = xq[:nq]
    xb[0, 5] = np.nan
    xb[n // 2] = np.nan
    xb[n - n % fo.SCAN_ROWS + 3, dim - 1] = np.nan
    xb[n - 1, 0] = np.nan
    X, Q = _dev(xb), _dev(xq)
    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    nfix = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    if engine == "mixed":
        X16 = torch.empty((n, dim), dtype=torch.bfloat16, device="cuda")
        mx = torch.zeros(2, dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().amdrec_bf16_rows(_lib.ptr(X), n, dim, dim, _lib.ptr(X16), dim, _lib.ptr(mx), _lib.stream_ptr(X.device)))
        flat_search_mixed(X, X16, mx, n, Q, k, D, I, n_fixup=nfix)
    else:
        flat_search(X, n, Q, k, D, I, n_fixup=nfix)
    torch.cuda.synchronize()
    I = I.cpu().numpy()
    _check_nonfinite(xb, xq, k, D.cpu().numpy(), I, dim, engine, scale)
    assert not np.isin(I, [0, n // 2, n - n % fo.SCAN_ROWS + 3, n - 1]).any()
    assert int(nfix.item()) == (nq if engine == "mixed" else 0)


# ---- (f) the C entry points with real strides, on a poisoned workspace ------------------------------------------------------------
def _bf16_shadow(Xp, dim, ld_out):
    """amdrec_bf16_rows of the first dim columns of padded Xp -> (int16 [rows][ld_out], NaN patterns in the padding; max_norm)."""
    out = torch.full((Xp.shape[0], ld_out), 0x7FC0, dtype=torch.int16, device=Xp.device)
    mx = torch.zeros(2, dtype=torch.float32, device=Xp.device)
    _lib.check(_lib.load().amdrec_bf16_rows(_lib.ptr(Xp), Xp.shape[0], Xp.stride(0), dim, _lib.ptr(out), ld_out, _lib.ptr(mx),
                                            _lib.stream_ptr(Xp.device)))
    return out, mx


@pytest.mark.parametrize("dim", fo.STRIDE_DIMS)
def test_bf16_rows_with_padded_leading_dimensions(dim):
    """amdrec_bf16_rows with ld = dim + 4 and ld_out = dim + 8: round-to-nearest-even bf16 of the first dim columns, NaN
    source padding never read into the norms, output padding untouched; max_norm[0] the largest row norm and max_norm[1]
    the largest rounding-error norm of a row."""
    xb, _, _ = fo.stride_inputs(dim)
    X = _dev(xb)
    out, mx = _bf16_shadow(_padded(X, dim + 4), dim, dim + 8)
    assert torch.equal(out[:, :dim], X.to(torch.bfloat16).view(torch.int16)) and (out[:, dim:] == 0x7FC0).all()
    assert abs(mx[0].item() - X.double().norm(dim=1).max().item()) <= 1e-6 * 2
    dmax = (X - X.to(torch.bfloat16).float()).double().norm(dim=1).max().item()
    assert dmax * (1 - 1e-6) <= mx[1].item() <= dmax * 1.001


@pytest.mark.parametrize("engine", ["mixed", "fp32"])
@pytest.mark.parametrize("dim", fo.STRIDE_DIMS)
def test_c_entries_with_padded_strides_on_a_poisoned_workspace(dim, engine):
    """amdrec_flat_search_mixed / amdrec_flat_search called directly: ld_corpus = dim + 4, ld_bf16 = dim + 8, ld_queries =
    dim + 4 with NaN in all padding, pos_offset = 1,000,000 (the fused finalize at 3 queries, the one-workgroup one at
    130), un-normalised rows.  The workspace is the test's own: exactly the bytes the *_workspace query reports plus a
    4 KiB tail, every byte 0xFF before the first call (counters -1, keys and scores NaN patterns).  The result is exact
    with no fix-up, the tail is untouched, and a second call on the same, now used, workspace returns the same bits."""
    lib = _lib.load()
    xb, xq_all, scale = fo.stride_inputs(dim)
    n, k, off = len(xb), fo.STRIDE_K, fo.STRIDE_POS_OFFSET
    Xp = _padded(_dev(xb), dim + 4)
    if engine == "mixed":
        X16, mx = _bf16_shadow(Xp, dim, dim + 8)
    rD_all, rI_all = fo.reference(xb, xq_all, k)
    st = lambda: _lib.stream_ptr(Xp.device)      # noqa: E731
    for nq in fo.STRIDE_NQ:
        xq = xq_all[:nq]
        Qp = _padded(_dev(xq), dim + 4)
        nb = C.c_size_t(0)
        if engine == "mixed":
            _lib.check(lib.amdrec_flat_search_mixed_workspace(nq, n, k, dim, C.byref(nb)))
        else:
            _lib.check(lib.amdrec_flat_search_workspace(nq, n, k, C.byref(nb)))
        assert nb.value == fo.plan(nq, n, k, dim, engine == "mixed").bytes
        ws = torch.full((nb.value + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 256 == 0
        results = []
        for _ in range(2):
            D = torch.full((nq, k), float("nan"), device="cuda")
            I = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            nfix = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            if engine == "mixed":
                _lib.check(lib.amdrec_flat_search_mixed(_lib.ptr(Xp), n, dim + 4, dim, _lib.ptr(X16), dim + 8, _lib.ptr(mx), _lib.ptr(Qp),
                                                        nq, dim + 4, k, off, _lib.ptr(D), _lib.ptr(I), _lib.ptr(ws), nb.value,
                                                        _lib.ptr(nfix), st()))
            else:
                _lib.check(lib.amdrec_flat_search(_lib.ptr(Xp), n, dim + 4, dim, _lib.ptr(Qp), nq, dim + 4, k, off, _lib.ptr(D),
                                                  _lib.ptr(I), _lib.ptr(ws), nb.value, _lib.ptr(nfix), st()))
            torch.cuda.synchronize()
            assert (ws[nb.value:] == 0xFF).all(), "the call wrote past the bytes it asked for"
            results.append((D.cpu().numpy(), I.cpu().numpy(), int(nfix.item())))
        (D1, I1, f1), (D2, I2, f2) = results
        _check(xb, xq, rD_all[:nq], rI_all[:nq], D1, I1, dim, engine, scale, offset=off)
        assert f1 == 0 and f2 == 0, (nq, f1, f2)
        assert np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32)), nq
        assert I1.min() >= off
