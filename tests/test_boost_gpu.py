"""Per-ad score boosts inside the flat search's corpus pass (amdrec.boost has the rule; tests/boost_oracle.py its loops, the
seeded boost patterns and the float64 oracle).  N = 20000 rows: above CAND_CAP, so the sampled path runs, and the last
128-row tile is partial (32 rows).

The defining property is checked bit for bit under the bf16 engine: ip[q][r] is taken from the index itself - unboosted
searches with k = slice size over sub-indexes of <= 2048 stored rows return every row's fp32 re-score -, s = ip + w * b is
formed in numpy float32, sorted by (s descending, position ascending), and the boosted search must equal it exactly in
positions and scores.  The fp32 engine returns its MFMA pass's values and is held to the float64 oracle."""
import functools
import json
import math
import struct

import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib
from tests import boost_oracle as bx, cases, exclude_oracle, flat_oracle as fo, group_cap_oracle
from tests.guarded import GuardedArena, SENTINEL, guarded

pytestmark = pytest.mark.gpu

N, NQ = bx.N, bx.NQ
PREFIXES = (1, 9, 33, 129, 513)       # tau inside the pass | threshold launch, small batch | per-query finalize | 2nd group
SLICE = 2000


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _index(rows, prefilter, boosts=None, stored=None):
    """A Flat index over ``rows``; ``stored``: device rows that replace what add() normalised, bit for bit (a row that was
    normalised once is not a fixed point of the normalisation), with the bf16 shadow rebuilt from them."""
    from amdrec.index import FAISSIndex
    idx = FAISSIndex(rows.shape[1], index_type="Flat", prefilter=prefilter)
    idx.add(rows, boosts=boosts)
    if stored is not None:
        idx._xb[:len(rows)].copy_(stored)
        idx._maxnorm.zero_()
        idx._shadow_rows(0, len(rows))
    return idx


def _search(idx, q, k, w=None, profile=False, **kw):
    """-> (positions, scores, n_fixup, profile tags)"""
    idx.n_fixup_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    tags = None
    try:
        if profile:
            _lib.profile_enable(True)
        I, D = idx.search_device(q, k, normalize=False, return_positions=True, boost_weight=w, **kw)
        torch.cuda.synchronize()
        if profile:
            tags = {t: int(e["launches"]) for t, e in _lib.profile_report().items()}
    finally:
        nfix, idx.n_fixup_out = int(idx.n_fixup_out.item()), None
        if profile:
            _lib.profile_enable(False)
    return I, D, nfix, tags


class _Case:
    """One (dim, prefilter): the index, its stored rows, the normalised queries, the weights, and (bf16 engine) ip."""

    def __init__(self, dim, prefilter):
        xb, xq = fo.case_inputs(dict(n=N, dim=dim, nq=NQ, kind="lifted", seed=1))
        self.dim, self.prefilter = dim, prefilter
        self.idx = _index(xb, prefilter)
        self.engine = "mixed" if self.idx._mixed else "fp32"
        self.qn = self.idx._normalize_(self.idx._to_device_f32(xq))
        self.xb, self.xq = self.idx._xb[:N].cpu().numpy(), self.qn.cpu().numpy()
        self.w = bx.weights_for(NQ)
        self.wd = _dev(self.w)

    @functools.cached_property
    def ip(self):
        """ip[q][r] float32 [NQ, N] from the index itself: the unboosted search of each slice of stored rows with k = its size
        returns every row of the slice with its score."""
        out = np.empty((NQ, N), dtype=np.float32)
        for lo in range(0, N, SLICE):
            hi = min(lo + SLICE, N)
            sub = _index(self.xb[lo:hi], self.prefilter, stored=self.idx._xb[lo:hi])
            pos, sc = sub.search_device(self.qn, hi - lo, normalize=False, return_positions=True)
            pos, sc = pos.cpu().numpy(), sc.cpu().numpy()
            assert (np.sort(pos, axis=1) == np.arange(hi - lo)).all()
            np.put_along_axis(out[:, lo:hi], pos, sc, axis=1)
        return out

    def with_boosts(self, boost):
        idx = _index(self.xb, self.prefilter, stored=self.idx._xb[:N])
        idx.set_boosts(boost)
        return idx

    @functools.cached_property
    def plain(self):
        """the unboosted search of all NQ queries for k = 100: (positions, scores) on the host"""
        I, D, _, _ = _search(self.idx, self.qn, 100)
        return I.cpu().numpy(), D.cpu().numpy()

    def check64(self, D, I, boost, nq, k):
        rD, rI = bx.expected64(self.xb, self.xq[:nq], boost, self.w[:nq], k)
        q64, b64 = self.xq[:nq].astype(np.float64), boost.astype(np.float64)
        oracle.search.check_topk(rD, rI, D, I, tau=cases.TOPK_TAU, score_tol=fo.score_tol(self.dim, engine=self.engine),
                                 scores_of=lambda qi, ids: (self.xb[np.asarray(ids)].astype(np.float64) @ q64[qi] +
                                                            float(self.w[qi]) * b64[np.asarray(ids)]).astype(np.float32))
        assert np.array_equal(I >= 0, np.isfinite(D))


@functools.lru_cache(maxsize=None)
def _case(dim, prefilter):
    return _Case(dim, prefilter)


def _boost_tags(tags):
    return sorted(t for t in (tags or {}) if "_boost" in t)


def _unseen(nq, k, dim):
    p = fo.plan(nq, N, k, dim)
    seen = np.zeros(N, dtype=bool)
    if p.streaming:
        for t in p.sample_tiles:
            seen[t * fo.SCAN_ROWS:(t + 1) * fo.SCAN_ROWS] = True
    else:
        seen[fo.sample_rows(p)] = True
    assert 0 < seen.sum() < N // 4
    return seen


def _pattern(c, name):
    if name == "noise":
        return bx.noise()
    if name == "sparse_half":
        return bx.sparse_half()
    if name == "demote":
        return bx.demote(np.unique(c.plain[0][::50, :100]))           # the unboosted top-100 of every fiftieth query
    if name == "quantised":
        return bx.quantised()
    raise KeyError(name)


# ---- 1. the defining property, bf16 engine, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["noise", "sparse_half", "demote", "quantised"])
@pytest.mark.parametrize("dim", [256, 32, 72])
def test_boosted_search_is_the_sort_of_ip_plus_term(dim, pattern):
    c = _case(dim, "bf16")
    assert c.engine == "mixed"
    boost = _pattern(c, pattern)
    idx = c.with_boosts(boost)
    assert idx._boost_max == float(np.abs(boost).max())
    stream = dim in fo.FLAT_DIMS_STREAM
    for k in (10, 100):
        wD, wI = bx.topk(c.ip, boost, c.w, k)
        for nq in PREFIXES:
            q = c.qn[:nq].contiguous()
            I, D, nfix, tags = _search(idx, q, k, c.wd[:nq].contiguous(), profile=True)
            assert torch.equal(I, _dev(wI[:nq])) and torch.equal(D, _dev(wD[:nq])), (dim, pattern, k, nq)
            print(f"dim {dim} {pattern} k {k} nq {nq}: n_fixup {nfix}")
            if pattern in ("noise", "sparse_half"):
                # a boost on benign data must not push queries into the exact scan
                assert nfix == _search(c.idx, q, k)[2], (dim, pattern, k, nq, nfix)
            # a boosted call runs the boosted kernels, and no unboosted search kernel where a boosted one exists
            assert ("search_filter_stream128x512_bf16_boost" in tags) == stream and "search_filter_stream128x512_bf16" not in tags
            assert ("search_sample_max128x512_bf16_boost" in tags) == stream
            assert not [t for t in tags if t.startswith(("search_sample", "search_filter", "search_fixup", "search_finalize"))
                        and "_boost" not in t], tags
            assert "search_fixup_boost" in tags and "search_finalize_mixed_boost" in tags


@pytest.mark.parametrize("dim", [256, 32, 72])
def test_blind_sample(dim):
    """Large boosts only on rows the strided sample of THIS (nq, k) does not read, so tau is the plain search's: with t >= 2
    every boosted row of a query with w != 0 lies above it (a cosine is <= 1).  (a) 300 such rows are all admitted beside the
    usual candidates and the main path answers (n_fixup == 0); (b) 9000 are more than CAND_CAP: every query with w != 0
    overflows its candidate list and the boosted fix-up scan answers it.  Both exact, bit for bit."""
    c = _case(dim, "bf16")
    idx = c.with_boosts(np.zeros(N, dtype=np.float32))
    for nq, k in ((9, 10), (40, 10), (129, 100), (513, 100)):
        seen = _unseen(nq, k, dim)
        for count in (300, 9000):
            assert count > fo.CAND_CAP or count + 2048 < fo.CAND_CAP
            boost = bx.unseen_only(seen, count, value=4.0, seed=count + nq)
            idx.set_boosts(boost)
            wD, wI = bx.topk(c.ip[:nq], boost, c.w[:nq], k)
            I, D, nfix, _ = _search(idx, c.qn[:nq].contiguous(), k, c.wd[:nq].contiguous())
            assert torch.equal(I, _dev(wI)) and torch.equal(D, _dev(wD)), (dim, nq, k, count)
            boosted = c.w[:nq] != 0
            assert np.isin(wI[boosted], np.flatnonzero(boost)).all()          # the winners are the unseen rows
            assert nfix == (int(boosted.sum()) if count > fo.CAND_CAP else 0), (dim, nq, k, count, nfix)


# ---- 2. w = 0 and None ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(256, "bf16"), (72, "bf16"), (100, "fp32")])
def test_zero_weight_is_the_plain_search_and_none_runs_no_boosted_kernel(dim, prefilter):
    c = _case(dim, prefilter)
    idx = c.with_boosts(bx.sparse_half())
    pI, pD = c.plain
    for nq in (9, 33, 129):
        q = c.qn[:nq].contiguous()
        nI, nD, _, ntags = _search(idx, q, 100, None, profile=True)
        _, _, _, ptags = _search(c.idx, q, 100, None, profile=True)
        assert not _boost_tags(ntags) and ntags == ptags, (ntags, ptags)
        assert np.array_equal(nI.cpu().numpy(), pI[:nq]) and np.array_equal(nD.cpu().numpy(), pD[:nq])
        for w in (0.0, torch.zeros(nq, device="cuda")):
            zI, zD, _, ztags = _search(idx, q, 100, w, profile=True)
            assert _boost_tags(ztags)
            assert np.array_equal(zI.cpu().numpy(), pI[:nq]) and (zD.cpu().numpy() == pD[:nq]).all()
    # mixed weights: the queries with weight 0 (every fourth) equal the plain search
    I, D, _, _ = _search(idx, c.qn, 100, c.wd)
    zero = np.flatnonzero(c.w == 0)
    assert np.array_equal(I.cpu().numpy()[zero], pI[zero]) and (D.cpu().numpy()[zero] == pD[zero]).all()


# ---- 3. the fp32 engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["noise", "sparse_half"])
@pytest.mark.parametrize("k", [10, 100])
def test_fp32_engine_against_the_oracle(k, pattern):
    c = _case(100, "fp32")
    assert c.engine == "fp32"
    boost = _pattern(c, pattern)
    idx = c.with_boosts(boost)
    for nq in (1, 33, 129, 513):
        I, D, _, tags = _search(idx, c.qn[:nq].contiguous(), k, c.wd[:nq].contiguous(), profile=True)
        c.check64(D.cpu().numpy(), I.cpu().numpy(), boost, nq, k)
        assert any(t.startswith("search_filter_boost") for t in tags) and any(t.startswith("search_sample_boost") for t in tags), tags
        assert not [t for t in tags if t.startswith(("search_filter_2", "search_filter_1", "search_sample_2", "search_sample_1"))], tags


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_k_above_ntotal_and_the_no_sample_path(dim, prefilter):
    c, nq = _case(dim, prefilter), 70
    q, w = c.qn[:nq].contiguous(), c.wd[:nq].contiguous()
    for n, k in ((60, 100), (3000, 10)):                                 # k > ntotal | a small corpus: no sample
        assert n <= fo.CAND_CAP
        boost = bx.noise(n, seed=n) + np.where(np.arange(n) % 50 == 0, np.float32(0.5), np.float32(0)).astype(np.float32)
        idx = _index(c.xb[:n], prefilter, boost, stored=c.idx._xb[:n])
        I, D, _, tags = _search(idx, q, k, w, profile=True)
        I, D = I.cpu().numpy(), D.cpu().numpy()
        assert not [t for t in tags if t.startswith("search_sample")]
        kk = min(k, n)
        assert (I[:, kk:] == -1).all() and np.isneginf(D[:, kk:]).all() and (I[:, :kk] >= 0).all()
        if c.engine == "mixed":
            ip = c.ip[:nq, :n]
            wD, wI = bx.topk(ip, boost, c.w[:nq], k)
            assert np.array_equal(I, wI) and np.array_equal(D, wD)
        else:
            rD, rI = bx.expected64(c.xb[:n], c.xq[:nq], boost, c.w[:nq], k)
            b64 = boost.astype(np.float64)
            oracle.search.check_topk(rD[:, :kk], rI[:, :kk], D[:, :kk], I[:, :kk], tau=cases.TOPK_TAU, score_tol=fo.score_tol(dim, engine="fp32"),
                                     scores_of=lambda qi, ids: (c.xb[np.asarray(ids)].astype(np.float64) @ c.xq[qi].astype(np.float64)
                                                                + float(c.w[qi]) * b64[np.asarray(ids)]).astype(np.float32))


@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_a_nan_row_is_never_returned_however_large_its_boost(dim, prefilter):
    c, nq, k = _case(dim, prefilter), 40, 10
    xb, at = fo.with_nonfinite_rows(c.xb)
    boost = bx.noise()
    boost[at["all_nan"]], boost[at["one_nan"]] = 1000.0, 1000.0
    idx = _index(xb, prefilter, boost)
    I, D, _, _ = _search(idx, c.qn[:nq].contiguous(), k, 1.0)
    I, D = I.cpu().numpy(), D.cpu().numpy()
    assert not np.isnan(D).any() and not (set(I.ravel().tolist()) & {at["all_nan"], at["one_nan"]})
    assert (I >= 0).all()


@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_boosts_at_the_first_and_the_last_row(dim, prefilter):
    c, nq, k = _case(dim, prefilter), 40, 10
    boost = np.zeros(N, dtype=np.float32)
    boost[0], boost[N - 1] = 5.0, 2.5                                    # (|ip| <= 1) the last row sits in the partial tile
    idx = c.with_boosts(boost)
    I, D, _, _ = _search(idx, c.qn[:nq].contiguous(), k, 1.0)
    I = I.cpu().numpy()
    assert (I[:, 0] == 0).all() and (I[:, 1] == N - 1).all()
    if c.engine == "mixed":
        wD, wI = bx.topk(c.ip[:nq], boost, np.ones(nq, dtype=np.float32), k)
        assert np.array_equal(I, wI) and np.array_equal(D.cpu().numpy(), wD)


@pytest.mark.parametrize("nq", [33, 513])
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (72, "fp32")])
def test_exact_size_buffers(dim, prefilter, nq):
    """Both C entries with boosts of exactly nrows values, weights of exactly nq, outputs of exactly nq * k and a workspace of
    exactly the queried size, each between guard bands: bands intact, every output slot written, the usual result."""
    from amdrec.index import flat_search, flat_search_mixed
    c, k = _case(dim, prefilter), 10
    hb = bx.sparse_half()
    boost = guarded((N,), torch.float32, "cuda")
    boost.copy_(_dev(hb))
    w = guarded((nq,), torch.float32, "cuda")
    w.copy_(c.wd[:nq])
    D, I = guarded((nq, k), torch.float32, "cuda", "output"), guarded((nq, k), torch.int64, "cuda", "output")
    q = c.qn[:nq].contiguous()
    arena = GuardedArena()
    with _lib.WORKSPACE.private(arena):
        if c.engine == "mixed":
            flat_search_mixed(c.idx._xb, c.idx._xb16, c.idx._maxnorm, N, q, k, D, I, boost=(boost, w, 0.5))
        else:
            flat_search(c.idx._xb, N, q, k, D, I, boost=(boost, w, 0.5))
        arena.check()
    for t in (boost, w, D, I):
        t.check()
    assert not torch.isnan(D).any() and not (I == SENTINEL).any()
    if c.engine == "mixed":
        wD, wI = bx.topk(c.ip[:nq], hb, c.w[:nq], k)
        assert np.array_equal(I.cpu().numpy(), wI) and np.array_equal(D.cpu().numpy(), wD)
    else:
        c.check64(D.cpu().numpy(), I.cpu().numpy(), hb, nq, k)


# ---- 5. composition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_exclusion_lists_and_group_caps_wrap_the_boosted_search(dim, prefilter):
    c, nq, k, E = _case(dim, prefilter), 40, 20, 6
    boost = bx.sparse_half()
    idx = c.with_boosts(boost)
    q, w = c.qn[:nq].contiguous(), c.wd[:nq].contiguous()
    posc, scc, _, _ = _search(idx, q, k + E, w)
    posc, scc = posc.cpu().numpy(), scc.cpu().numpy()
    rng = np.random.default_rng(8)
    excl = np.full((nq, E), -1, dtype=np.int64)
    for i in range(nq):
        pick = rng.choice(posc[i], size=int(rng.integers(0, E + 1)), replace=False)
        excl[i, :len(pick)] = pick
    want_pos, want_sc = exclude_oracle.compact(posc, posc, scc, excl, k, exclude_oracle.fill_score("Flat"))
    pos, sc, _, _ = _search(idx, q, k, w, exclude=_dev(excl))
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(sc.cpu().numpy(), want_sc)
    # the cap rule on the boosted top-K1
    groups = (np.arange(N) % 7).astype(np.int64)
    groups[::11] = -1
    idx.set_groups(groups)
    k1 = 2 * k
    pos1, sc1, _, _ = _search(idx, q, k1, w)
    want_pos, want_sc = group_cap_oracle.compact(pos1.cpu().numpy(), sc1.cpu().numpy(), groups, 2, k, group_cap_oracle.fill_score("Flat"))
    pos, sc, _, _ = _search(idx, q, k, w, max_per_group=2)
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(sc.cpu().numpy(), want_sc)
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx.search_device(q, k, boost_weight=w, require_all=torch.zeros(nq, dtype=torch.int64, device="cuda"))


# ---- 6. life cycle --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
def test_boosts_follow_add_set_save_load_and_remove(prefilter, tmp_path):
    from amdrec.index import FAISSIndex
    dim, nq, k = 32, 40, 10
    c = _case(dim, prefilter)
    n1, n2 = 9000, 3000
    n = n1 + n2
    boost = bx.noise(n, seed=5) + bx.sparse_half(n, seed=6)
    boost[7] = -0.0
    ids = np.arange(n) * 5 + 3
    q, w = c.qn[:nq].contiguous(), c.wd[:nq].contiguous()

    def header(path):
        with open(path, "rb") as f:
            f.read(9)
            (hl,) = struct.unpack("<Q", f.read(8))
            return json.loads(f.read(hl).decode())

    idx = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    idx.add(c.xb[:n1], ids[:n1].tolist())                         # no boosts yet: no tensor, the file as ever
    assert idx._boosts is None and len(idx.resident_tensors()) == 4 and not idx.get_boosts().any()
    with pytest.raises(ValueError, match="without boosts"):
        idx.search_device(q, k, boost_weight=1.0)
    idx.save(str(tmp_path / "plain.bin"))
    assert "boosts" not in [a["name"] for a in header(tmp_path / "plain.bin")["arrays"]]
    idx.add(c.xb[n1:n], ids[n1:].tolist(), boosts=boost[n1:])       # the first boosts: earlier rows read 0
    assert any(t is idx._boosts for t in idx.resident_tensors())
    got = idx.get_boosts().cpu().numpy()
    assert not got[:n1].any() and np.array_equal(got[n1:], boost[n1:])
    assert idx._boost_max == float(np.abs(boost[n1:]).max())
    for bad in ([1.0, 2.0, 3.0], [1.0, float("nan")], [float("inf"), 0.0]):
        with pytest.raises(ValueError):
            idx.add(c.xb[:2], [1, 2], boosts=bad)
    with pytest.raises(ValueError):
        idx.set_boosts(boost[:-1])
    assert idx.index.ntotal == n
    before = idx._boosts
    idx.set_boosts(boost)                                          # out of place: the old tensor is not written
    assert idx._boosts is not before and not before[:n1].any()
    got = idx.get_boosts().cpu().numpy()
    assert np.array_equal(got, boost) and not np.signbit(got[7])
    assert idx._boost_max == float(np.abs(boost).max())

    stored = idx._xb[:n].clone()

    def result(index, **kw):
        I, D = index.search_device(q, k, normalize=False, boost_weight=w, **kw)
        return I.cpu().numpy(), D.cpu().numpy()

    wantI, wantD = result(idx)
    posI, posD = result(idx, return_positions=True)
    assert np.array_equal(wantI, ids[posI]) and np.array_equal(wantD, posD)
    fresh = _index(c.xb[:n], prefilter, boost, stored=stored)
    fI, fD = result(fresh, return_positions=True)
    assert np.array_equal(fI, posI) and np.array_equal(fD, posD)
    # a graph captured before set_boosts replays the old boosts
    g = torch.cuda.CUDAGraph()
    arena = _lib.FixedArena(1 << 28, "cuda")
    with _lib.WORKSPACE.private(arena):
        idx.search_device(q, k, normalize=False, return_positions=True, boost_weight=w)
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            gI, gD = idx.search_device(q, k, normalize=False, return_positions=True, boost_weight=w)
    old = idx._boosts
    idx.set_boosts(-boost)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(gI.cpu().numpy(), posI) and np.array_equal(gD.cpu().numpy(), posD)
    assert not np.array_equal(result(idx, return_positions=True)[0], posI)
    idx.set_boosts(boost)
    del g, old
    # save / load
    idx.save(str(tmp_path / "boosted.bin"))
    assert "boosts" in [a["name"] for a in header(tmp_path / "boosted.bin")["arrays"]]
    back = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    back.load(str(tmp_path / "boosted.bin"))
    assert np.array_equal(back.get_boosts().cpu().numpy(), boost) and back._boost_max == idx._boost_max
    bI, bD = result(back)
    assert np.array_equal(bI, wantI) and np.array_equal(bD, wantD)
    plain = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    plain.load(str(tmp_path / "plain.bin"))
    assert plain._boosts is None
    # remove_ids: the boosted search of what is left equals a fresh index over the surviving rows and boosts
    gone = np.random.default_rng(3).choice(n, size=n // 3, replace=False)
    keep = np.setdiff1d(np.arange(n), gone)
    assert idx.remove_ids(ids[gone].tolist()) == len(gone)
    assert np.array_equal(idx.get_boosts().cpu().numpy(), boost[keep])
    fresh = _index(c.xb[keep], prefilter, boost[keep], stored=stored[_dev(keep)])
    aI, aD = result(idx, return_positions=True)
    bI, bD = result(fresh, return_positions=True)
    assert np.array_equal(aI, bI)
    assert np.array_equal(aD, bD) if c.engine == "mixed" else np.abs(aD - bD).max() <= fo.score_tol(dim, engine="fp32")
    # the numpy-level calls slice the weights with the query chunks
    hI, hD = idx.batch_search(c.xq[:nq], k, batch_size=16, boost_weight=c.w[:nq])
    sI, sD = idx.search(c.xq[:nq], k, boost_weight=[float(v) for v in c.w[:nq]])
    assert np.array_equal(hI, sI) and np.array_equal(hD, sD)
    assert np.array_equal(sI, ids[keep][aI])


# ---- 7. the serving pipeline ----------------------------------------------------------------------------------------------------------
def _clone(out):
    return {k_: (v.clone() if isinstance(v, torch.Tensor) else v) for k_, v in out.items()}


@pytest.mark.parametrize("B", [6, 36])
def test_pipeline_boosts_stage_one(B):
    from tests.test_exclude_gpu import _rec, _users
    n_ads, top_k, k1 = 8192, 10, 200
    rec, user, nnum = _rec(n_ads)
    idx = rec.faiss_index
    boost = bx.sparse_half(n_ads, seed=44) + bx.noise(n_ads, seed=45)
    bids = np.exp(np.random.default_rng(46).standard_normal(n_ads)).astype(np.float32)
    idx.set_boosts(boost)
    idx.set_bids(bids)
    users = _users(user, B, 5)
    uc, un = rec.preprocess_batch(users)
    wh = bx.weights_for(B)
    w = _dev(wh)
    out = _clone(rec.recommend_device(uc, un, top_k, k1, stage1_boost=w))
    # stage 2 fed with the boosted search's positions
    emb = rec.two_tower_model.user_tower.encode(uc, un, check_indices=False, renormalize=True)
    pos, sc = idx.search_device(emb, k1, normalize=False, return_positions=True, boost_weight=w)
    want = rec._stage2(uc, un, pos, top_k, False)
    for key in ("ad_ids", "scores", "candidate_ids", "logits"):
        assert torch.equal(out[key], want[key]), key
    assert torch.equal(out["candidate_scores"], sc)
    plain = _clone(rec.recommend_device(uc, un, top_k, k1))
    assert not torch.equal(plain["candidate_ids"], out["candidate_ids"])
    zero = np.flatnonzero(wh == 0)
    assert torch.equal(plain["candidate_ids"][zero], out["candidate_ids"][zero])
    # heads="ctr_first" and rank_by="ecpm" agree with heads="all" bit for bit
    first = rec.recommend_device(uc, un, top_k, k1, stage1_boost=w, heads="ctr_first")
    assert torch.equal(first["ad_ids"], out["ad_ids"]) and torch.equal(first["scores"], out["scores"])
    ea = _clone(rec.recommend_device(uc, un, top_k, k1, stage1_boost=w, rank_by="ecpm", heads="all"))
    ef = rec.recommend_device(uc, un, top_k, k1, stage1_boost=w, rank_by="ecpm", heads="ctr_first")
    for key in ("ad_ids", "scores", "ecpm", "prices", "candidate_ids"):
        assert torch.equal(ea[key], ef[key]), key
    assert torch.equal(ea["candidate_ids"], out["candidate_ids"])
    # the reference API ships the weights in the staging block
    res = rec.batch_recommend(users, top_k, k1, stage1_boost=wh.tolist())
    assert [r["ad_ids"] for r in res] == out["ad_ids"].cpu().tolist()
    assert [r["scores"]["ctr"] for r in res] == out["scores"][0].cpu().tolist()
    assert rec.recommend_ads(users[1], top_k, k1, stage1_boost=float(wh[1]))["ad_ids"] == out["ad_ids"][1].cpu().tolist()
    assert rec.recommend_tensors(uc, un, top_k, k1, stage1_boost=wh)[2]["ad_ids"] == out["ad_ids"][2].cpu().tolist()
    assert rec.recommend_ads(users[1], top_k, k1)["ad_ids"] == plain["ad_ids"][1].cpu().tolist()
    # a graph captured with stage1_boost replays the eager result; one captured without raises on a weight
    g = rec.capture(B, top_k, k1, stage1_boost=True)
    r = g(uc, un, stage1_boost=w)
    assert torch.equal(r["ad_ids"], out["ad_ids"]) and torch.equal(r["scores"], out["scores"])
    assert torch.equal(r["candidate_ids"], out["candidate_ids"])
    r = g(uc, un)                                                   # None: zeros, the plain search's positions
    assert torch.equal(r["ad_ids"], plain["ad_ids"]) and torch.equal(r["scores"], plain["scores"])
    g0 = rec.capture(B, top_k, k1)
    assert torch.equal(g0(uc, un)["ad_ids"], plain["ad_ids"])
    with pytest.raises(ValueError, match="stage1_boost"):
        g0(uc, un, stage1_boost=1.0)
    # add_ads / remove_ads keep the array in step
    emb_new = torch.nn.functional.normalize(torch.randn(3, idx.dimension, generator=torch.Generator().manual_seed(1)), dim=1)
    rec.add_ads(emb_new.numpy(), rec.ad_features[:3].cpu().numpy(), boosts=[1.0, 2.0, 3.0])
    assert idx.get_boosts()[-3:].cpu().tolist() == [1.0, 2.0, 3.0] and idx._boost_max == 3.0
    rec.remove_ads([0, 1])
    assert np.array_equal(idx.get_boosts().cpu().numpy(), np.concatenate([boost[2:], [1.0, 2.0, 3.0]]).astype(np.float32))


def test_a_bid_aware_boost_brings_the_ecpm_winner_into_the_auction():
    """Why the feature exists: one ad at similarity rank stage1_k + 50 with a bid that makes it the eCPM winner is absent
    without the boost - eCPM ranking can only order what retrieval returned - and first with boost = beta * log(bid)."""
    from tests.test_exclude_gpu import _rec, _users
    n_ads, top_k, k1, B = 8192, 10, 200, 1
    rec, user, nnum = _rec(n_ads)
    idx = rec.faiss_index
    users = _users(user, B, 9)
    uc, un = rec.preprocess_batch(users)
    emb = rec.two_tower_model.user_tower.encode(uc, un, check_indices=False, renormalize=True)
    pos, sc = idx.search_device(emb, k1 + 51, normalize=False, return_positions=True)
    target = int(pos[0, k1 + 50])
    gap = float(sc[0, 0] - sc[0, k1 + 50])                              # what the boost has to bridge to reach rank 1
    bids = np.ones(n_ads, dtype=np.float32)
    bids[target] = 1.0e6                                                # pCTR in (0, 1): no other ad's eCPM comes close
    idx.set_bids(bids)
    without = rec.recommend_device(uc, un, top_k, k1, rank_by="ecpm")
    assert target not in without["candidate_ids"][0].cpu().tolist() and target not in without["ad_ids"][0].cpu().tolist()
    beta = 2.0 * gap / math.log(1.0e6)
    idx.set_boosts(beta * torch.log(idx.get_bids()))
    boosted = rec.recommend_device(uc, un, top_k, k1, rank_by="ecpm", stage1_boost=1.0)
    assert int(boosted["candidate_ids"][0, 0]) == target
    assert int(boosted["ad_ids"][0, 0]) == target
    # every other ad has boost 0: the rest of the candidate list is the plain list, shifted by one
    assert boosted["candidate_ids"][0, 1:].cpu().tolist() == without["candidate_ids"][0, :k1 - 1].cpu().tolist()


def test_ivf_index_refuses_a_boost():
    from amdrec.index import FAISSIndex
    xb, xq = fo.case_inputs(dict(n=2000, dim=32, nq=4, kind="lifted", seed=1))
    idx = FAISSIndex(32, index_type="IVF", nlist=8, nprobe=2)
    idx.add(xb)
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx.search_device(_dev(xq), 5, boost_weight=1.0)
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx.set_boosts(np.zeros(2000, dtype=np.float32))
