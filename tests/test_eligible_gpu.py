"""Per-request eligibility masks inside the flat search's corpus pass (amdrec.eligible has the contract; tests/eligible_oracle.py
the seeded tags, the seven query classes and the float64 oracle).  N = 20000 rows: above CAND_CAP, so the sampled path runs,
and the last 128-row tile is partial (32 rows).

The defining property is checked bit for bit: the filtered result of a query equals the UNFILTERED search of an index that
holds only the query's eligible rows (the same stored fp32 rows, the same bf16 shadow rows), positions mapped through those
rows - both are the exact top-k under the same fp32 re-score chain, so no tolerance applies under the bf16 engine.  The fp32
engine returns its MFMA pass's scores and is held to the float64 oracle with flat_oracle.score_tol."""
import functools
import json
import struct

import numpy as np
import pytest
import torch

import oracle
from amdrec import _lib, eligible as el
from tests import cases, eligible_oracle as eo, exclude_oracle, flat_oracle as fo
from tests.guarded import GuardedArena, SENTINEL, guarded

pytestmark = pytest.mark.gpu

N, NQ, TAG_SEED = 20_000, 513, 901
PREFIXES = (1, 9, 33, 129, 513)       # tau inside the pass | threshold launch, fused finalize | per-query finalize | 2nd group


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(a):
    return _dev(el.as_words(a, len(a)))


def _index(rows, prefilter, tags=None, stored=None):
    """A Flat index over ``rows``; ``stored``: device rows that replace what add() normalised, bit for bit (a row that was
    normalised once is not a fixed point of the normalisation), with the bf16 shadow rebuilt from them."""
    from amdrec.index import FAISSIndex
    idx = FAISSIndex(rows.shape[1], index_type="Flat", prefilter=prefilter)
    idx.add(rows, tags=tags)
    if stored is not None:
        idx._xb[:len(rows)].copy_(stored)
        idx._maxnorm.zero_()
        idx._shadow_rows(0, len(rows))
    return idx


class _Case:
    """One (dim, prefilter): the tagged index, its stored rows and the normalised queries (device and host), the masks."""

    def __init__(self, dim, prefilter):
        xb, xq = fo.case_inputs(dict(n=N, dim=dim, nq=NQ, kind="lifted", seed=1))
        self.dim, self.prefilter = dim, prefilter
        self.tags = eo.tags_for(N, TAG_SEED)
        self.idx = _index(xb, prefilter, self.tags)
        self.engine = "mixed" if self.idx._mixed else "fp32"
        self.qn = self.idx._normalize_(self.idx._to_device_f32(xq))
        self.xb, self.xq = self.idx._xb[:N].cpu().numpy(), self.qn.cpu().numpy()
        self.a, self.y = eo.masks_for(NQ)
        self.ma, self.my = _words(self.a), _words(self.y)

    @functools.lru_cache(maxsize=None)
    def expected(self, k):
        return eo.expected(self.xb, self.xq, k, self.tags, self.a, self.y)

    @functools.lru_cache(maxsize=None)
    def subindex_result(self, k):
        """Per query the unfiltered search of a fresh index holding only the rows of the query's class, positions mapped
        back, padded with (-inf, -1) -> device (D, I) [NQ, k]."""
        D = torch.full((NQ, k), float("-inf"), device="cuda")
        I = torch.full((NQ, k), -1, dtype=torch.int64, device="cuda")
        for c in range(7):
            rows = eo.class_rows(self.tags, c)
            if not len(rows):
                continue
            r = _dev(rows)
            sub = _index(self.xb[rows], self.prefilter, stored=self.idx._xb[r])
            pos, sc = sub.search_device(self.qn[c::7].contiguous(), k, normalize=False, return_positions=True)
            D[c::7], I[c::7] = sc, torch.where(pos >= 0, r[pos.clamp(min=0)], pos)
        return D, I

    def search(self, nq, k, masks=True, profile=False, positions=True, idx=None):
        """-> (positions or ids, scores, n_fixup, profile tags)"""
        idx = self.idx if idx is None else idx
        idx.n_fixup_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        tags = None
        try:
            if profile:
                _lib.profile_enable(True)
            kw = dict(require_all=self.ma[:nq].contiguous(), require_any=self.my[:nq].contiguous()) if masks is True else (masks or {})
            I, D = idx.search_device(self.qn[:nq].contiguous(), k, normalize=False, return_positions=positions, **kw)
            torch.cuda.synchronize()
            if profile:
                tags = {t: int(e["launches"]) for t, e in _lib.profile_report().items()}
        finally:
            nfix, idx.n_fixup_out = int(idx.n_fixup_out.item()), None
            if profile:
                _lib.profile_enable(False)
        return I, D, nfix, tags

    def check(self, D, I, rD, rI, xq=None):
        """check_topk against the float64 oracle: near-tie band, the engine's score tolerance, each score its row's own."""
        xq = self.xq[:len(rD)] if xq is None else xq
        q64 = xq.astype(np.float64)
        oracle.search.check_topk(rD, rI, D, I, tau=cases.TOPK_TAU, score_tol=fo.score_tol(self.dim, engine=self.engine),
                                 scores_of=lambda qi, ids: (self.xb[np.asarray(ids)].astype(np.float64) @ q64[qi]).astype(np.float32))
        assert np.array_equal(I >= 0, np.isfinite(D))


@functools.lru_cache(maxsize=None)
def _case(dim, prefilter):
    return _Case(dim, prefilter)


def _elig_tags(tags):
    return sorted(t for t in (tags or {}) if "_elig" in t)


# ---- 1. the defining property, bf16 engine, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("dim", [256, 32, 72])
def test_filtered_search_is_the_search_of_the_eligible_rows(dim, k):
    c = _case(dim, "bf16")
    assert c.engine == "mixed"
    wD, wI = c.subindex_result(k)
    rD, rI = c.expected(k)
    counts = np.array([eo.CLASS_ROWS_20000[q % 7] for q in range(NQ)])
    for nq in PREFIXES:
        I, D, nfix, tags = c.search(nq, k, profile=True)
        assert torch.equal(D, wD[:nq]) and torch.equal(I, wI[:nq]), (dim, k, nq)
        c.check(D.cpu().numpy(), I.cpu().numpy(), rD[:nq], rI[:nq])
        # only a query with fewer than k eligible rows may need the exact scan
        assert nfix == int((counts[:nq] < k).sum()), (nq, nfix)
        assert _elig_tags(tags), tags
        stream = dim in fo.FLAT_DIMS_STREAM
        assert ("search_filter_stream128x512_bf16_elig" in tags) == stream and "search_filter_stream128x512_bf16" not in tags
        assert ("search_sample_max128x512_bf16_elig" in tags) == stream and not [t for t in tags if t.startswith("search_sample") and "_elig" not in t]
        assert "search_fixup_elig" in tags and "search_fixup" not in tags


# ---- 2. the fp32 engine -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("dim", [72, 100])
def test_fp32_engine_against_the_oracle(dim, k):
    c = _case(dim, "fp32")
    assert c.engine == "fp32"
    rD, rI = c.expected(k)
    for nq in (1, 33, 129, 513):
        I, D, _, tags = c.search(nq, k, profile=True)
        c.check(D.cpu().numpy(), I.cpu().numpy(), rD[:nq], rI[:nq])
        assert any(t.startswith("search_filter_elig") for t in tags) and any(t.startswith("search_sample_elig") for t in tags), tags
        assert not [t for t in tags if t.startswith(("search_filter_2", "search_filter_1", "search_sample_2", "search_sample_1"))], tags


# ---- 3. no constraint is no change ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(256, "bf16"), (72, "bf16"), (100, "fp32")])
def test_zero_masks_equal_the_plain_search_and_none_runs_no_filtered_kernel(dim, prefilter):
    c = _case(dim, prefilter)
    for nq in (9, 33, 129):
        zero = torch.zeros(nq, dtype=torch.int64, device="cuda")
        pI, pD, pfix, ptags = c.search(nq, 100, masks=False, profile=True)
        nI, nD, _, ntags = c.search(nq, 100, masks=dict(require_all=None, require_any=None), profile=True)
        zI, zD, zfix, ztags = c.search(nq, 100, masks=dict(require_all=zero, require_any=zero), profile=True)
        oI, oD, _, otags = c.search(nq, 100, masks=dict(require_any=zero), profile=True)      # the other defaults to 0
        assert not _elig_tags(ptags) and not _elig_tags(ntags) and ptags == ntags, (ptags, ntags)
        assert _elig_tags(ztags) and _elig_tags(otags) == _elig_tags(ztags), ztags
        assert len(ztags) == len(ptags)                                    # launch for launch the same pipeline
        for I, D in ((nI, nD), (zI, zD), (oI, oD)):
            assert torch.equal(I, pI) and torch.equal(D, pD)
        assert pfix == zfix == 0
        ids0, sc0 = c.idx.search_device(c.qn[:nq].contiguous(), 100, normalize=False)
        ids1, sc1 = c.idx.search_device(c.qn[:nq].contiguous(), 100, normalize=False, require_all=zero, require_any=zero)
        assert torch.equal(ids0, ids1) and torch.equal(sc0, sc1)


# ---- 4. fewer than k eligible rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_fewer_than_k_eligible_rows_leave_an_unfilled_tail(dim, prefilter):
    c, k, nq = _case(dim, prefilter), 300, 70
    rD, rI = c.expected(k)
    I, D, nfix, _ = c.search(nq, k)
    I, D = I.cpu().numpy(), D.cpu().numpy()
    c.check(D, I, rD[:nq], rI[:nq])
    assert nfix == len(range(4, nq, 7)) + len(range(5, nq, 7))            # classes 4 (241 rows) and 5 (none): the exact scan
    rows4 = set(eo.class_rows(c.tags, 4).tolist())
    for q in range(4, nq, 7):                                             # every eligible row once, in order, then the tail
        assert sorted(I[q, :241].tolist()) == sorted(rows4) and (I[q, 241:] == -1).all() and np.isneginf(D[q, 241:]).all()
        assert np.array_equal(I[q], rI[q]) or np.abs(D[q, :241] - rD[q, :241]).max() <= fo.score_tol(dim, engine=c.engine)
        assert (np.diff(D[q, :241]) <= 0).all()
    for q in range(5, nq, 7):
        assert (I[q] == -1).all() and np.isneginf(D[q]).all()
    # the identity-id path: an unfilled slot reads id_map[-1], as ever
    ids, sc, _, _ = c.search(nq, k, positions=False)
    assert np.array_equal(ids.cpu().numpy(), np.where(I < 0, N - 1, I)) and np.array_equal(sc.cpu().numpy(), D)


# ---- 5. a sample that sees no eligible row ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 72])
def test_blind_sample(dim):
    """Only rows the sample does not read are eligible, so tau is -inf for every query: (a) 300 such rows are all admitted
    and the main path answers (n_fixup == 0); (b) 9000 are more than CAND_CAP, every query overflows its candidate list
    and the filtered fix-up scan answers (n_fixup == nq).  Both exact."""
    c, nq, k = _case(dim, "bf16"), 40, 10
    p = fo.plan(nq, N, k, dim)
    seen = np.zeros(N, dtype=bool)
    if p.streaming:
        for t in p.sample_tiles:
            seen[t * fo.SCAN_ROWS:(t + 1) * fo.SCAN_ROWS] = True
    else:
        seen[fo.sample_rows(p)] = True
    assert 0 < seen.sum() < N // 4
    unseen = np.nonzero(~seen)[0]
    one = _words(np.full(nq, eo.B63, dtype=np.uint64))
    masks = dict(require_all=one, require_any=None)
    for count, want_fix in ((300, 0), (9000, nq)):
        assert count > fo.CAND_CAP or want_fix == 0
        rows = np.sort(np.random.default_rng(count).choice(unseen, size=count, replace=False))
        tags = np.zeros(N, dtype=np.uint64)
        tags[rows] = np.uint64(eo.B63)
        idx = _index(c.xb, "bf16", tags, stored=c.idx._xb[:N])
        I, D, nfix, _ = c.search(nq, k, masks=masks, idx=idx)
        rD, rI = eo.expected(c.xb, c.xq[:nq], k, tags, np.full(nq, eo.B63, dtype=np.uint64), np.zeros(nq, dtype=np.uint64))
        c.check(D.cpu().numpy(), I.cpu().numpy(), rD, rI)
        assert set(I.cpu().numpy().ravel().tolist()) <= set(rows.tolist())
        assert nfix == want_fix, (count, nfix)


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_eligible_rows_at_the_ends_of_the_corpus(dim, prefilter):
    c, nq, k = _case(dim, prefilter), 40, 10
    bit = np.uint64(eo.B32)
    a, y = np.zeros(nq, dtype=np.uint64), np.full(nq, bit, dtype=np.uint64)
    last_tile = np.arange(N - N % fo.SCAN_ROWS, N)
    assert len(last_tile) == 32
    for rows in (last_tile, np.array([0]), np.array([0, N - 1])):
        tags = np.zeros(N, dtype=np.uint64)
        tags[rows] = bit | np.uint64(eo.B0)
        idx = _index(c.xb, prefilter, tags, stored=c.idx._xb[:N])
        I, D, nfix, _ = c.search(nq, k, masks=dict(require_all=None, require_any=_words(y)), idx=idx)
        rD, rI = eo.expected(c.xb, c.xq[:nq], k, tags, a, y)
        c.check(D.cpu().numpy(), I.cpu().numpy(), rD, rI)
        assert nfix == (nq if len(rows) < k else 0)


@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_small_corpus_takes_the_no_sample_path(dim, prefilter):
    c, n, nq, k = _case(dim, prefilter), 3000, 70, 10
    assert n <= fo.CAND_CAP
    tags = eo.tags_for(n, 5)
    idx = _index(c.xb[:n], prefilter, tags, stored=c.idx._xb[:n])
    I, D, nfix, tags_run = c.search(nq, k, idx=idx, profile=True)
    rD, rI = eo.expected(c.xb[:n], c.xq[:nq], k, tags, c.a[:nq], c.y[:nq])
    c.check(D.cpu().numpy(), I.cpu().numpy(), rD, rI)
    assert nfix == len(range(5, nq, 7)) and not [t for t in tags_run if t.startswith("search_sample")]


@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_an_eligible_nan_row_is_still_never_returned(dim, prefilter):
    c, nq, k = _case(dim, prefilter), 40, 10
    xb, at = fo.with_nonfinite_rows(c.xb)
    tags = eo.tags_for(N, TAG_SEED)
    tags[at["all_nan"]] |= np.uint64(eo.B0)                     # eligible for class 1, never returned
    tags[at["one_nan"]] &= ~np.uint64(eo.B0)                    # not eligible for it
    tags[at["pos_inf_first"]] |= np.uint64(eo.B0)
    idx = _index(xb, prefilter, tags)
    stored = idx._xb[:N].cpu().numpy()
    a, y = np.full(nq, eo.B0, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
    I, D, _, _ = c.search(nq, k, masks=dict(require_all=_words(a), require_any=None), idx=idx)
    I, D = I.cpu().numpy(), D.cpu().numpy()
    rows = np.nonzero(el.eligible(tags, [eo.B0], [0])[0])[0]
    assert at["all_nan"] in rows and at["one_nan"] not in rows
    rD, ri = fo.flat_search_nonfinite(stored[rows], c.xq[:nq], k)
    rI = np.where(ri >= 0, rows[np.maximum(ri, 0)], -1)
    assert not np.isnan(D).any() and not (set(I.ravel().tolist()) & {at["all_nan"], at["one_nan"]})
    ok = np.isfinite(stored).all(axis=1)
    oracle.search.check_topk(rD, rI, D, I, tau=cases.TOPK_TAU, score_tol=fo.score_tol(dim, engine=c.engine),
                             scores_of=lambda qi, ids: (np.where(ok[np.asarray(ids), None], stored[np.asarray(ids)], 0).astype(np.float64)
                                                        @ c.xq[qi].astype(np.float64)).astype(np.float32))


# ---- 7. exact-size buffers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [33, 513])
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (72, "fp32")])
def test_exact_size_buffers(dim, prefilter, nq):
    """Both C entries with tags of exactly nrows words, masks of exactly nq words, outputs of exactly nq * k and a workspace
    of exactly the queried size, each between guard bands: bands intact, every output slot written, the usual result."""
    from amdrec.index import flat_search, flat_search_mixed
    c, k = _case(dim, prefilter), 10
    tags = guarded((N,), torch.int64, "cuda")
    tags.copy_(_words(c.tags))
    ma, my = guarded((nq,), torch.int64, "cuda"), guarded((nq,), torch.int64, "cuda")
    ma.copy_(c.ma[:nq])
    my.copy_(c.my[:nq])
    D, I = guarded((nq, k), torch.float32, "cuda", "output"), guarded((nq, k), torch.int64, "cuda", "output")
    q = c.qn[:nq].contiguous()
    arena = GuardedArena()
    with _lib.WORKSPACE.private(arena):
        if c.engine == "mixed":
            flat_search_mixed(c.idx._xb, c.idx._xb16, c.idx._maxnorm, N, q, k, D, I, elig=(tags, ma, my))
        else:
            flat_search(c.idx._xb, N, q, k, D, I, elig=(tags, ma, my))
        arena.check()
    for t in (tags, ma, my, D, I):
        t.check()
    assert not torch.isnan(D).any() and not (I == SENTINEL).any()
    rD, rI = c.expected(k)
    c.check(D.cpu().numpy(), I.cpu().numpy(), rD[:nq], rI[:nq])


# ---- 8. with an exclusion list --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, prefilter", [(32, "bf16"), (72, "bf16"), (100, "fp32")])
def test_exclusion_lists_compose_with_the_masks(dim, prefilter):
    c, nq, k, E = _case(dim, prefilter), 40, 20, 6
    posc, scc, _, _ = c.search(nq, k + E)
    posc, scc = posc.cpu().numpy(), scc.cpu().numpy()
    rng = np.random.default_rng(8)
    excl = np.full((nq, E), -1, dtype=np.int64)
    for q in range(nq):
        have = posc[q][posc[q] >= 0]
        pick = rng.choice(have, size=min(len(have), int(rng.integers(0, E + 1))), replace=False) if len(have) else []
        excl[q, :len(pick)] = pick
    want_pos, want_sc = exclude_oracle.compact(posc, posc, scc, excl, k, exclude_oracle.fill_score("Flat"))
    pos, sc = c.idx.search_device(c.qn[:nq].contiguous(), k, normalize=False, return_positions=True, exclude=_dev(excl),
                                  require_all=c.ma[:nq].contiguous(), require_any=c.my[:nq].contiguous())
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(sc.cpu().numpy(), want_sc)
    ids, sc2 = c.idx.search_device(c.qn[:nq].contiguous(), k, normalize=False, exclude=_dev(excl),
                                   require_all=c.ma[:nq].contiguous(), require_any=c.my[:nq].contiguous())
    assert np.array_equal(ids.cpu().numpy(), exclude_oracle.ids_of(want_pos, np.arange(N))) and torch.equal(sc, sc2)
    # the limit k + E <= AMDREC_MAX_K is the exclusion list's alone: 10 000 ineligible rows are no list
    with pytest.raises(ValueError, match="AMDREC_MAX_K"):
        c.idx.search_device(c.qn[:1].contiguous(), 2045, exclude=_dev(excl[:1]), require_all=c.ma[:1].contiguous())


# ---- 9. maintenance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefilter", ["bf16", "fp32"])
def test_tags_follow_add_set_save_load_and_remove(prefilter, tmp_path):
    from amdrec.index import FAISSIndex
    dim, nq, k = 32, 40, 10
    c = _case(dim, prefilter)
    n1, n2 = 9000, 3000
    n = n1 + n2
    tags = eo.tags_for(n, 12)
    ids = np.arange(n) * 5 + 3
    masks = dict(require_all=c.ma[:nq].contiguous(), require_any=c.my[:nq].contiguous())

    def header(path):
        with open(path, "rb") as f:
            f.read(9)
            (hl,) = struct.unpack("<Q", f.read(8))
            return json.loads(f.read(hl).decode())

    idx = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    idx.add(c.xb[:n1], ids[:n1].tolist())                         # no tags yet: no tensor, the file as ever
    assert idx._tags is None and len(idx.resident_tensors()) == 4 and not idx.get_tags().any()
    idx.save(str(tmp_path / "plain.bin"))
    assert "tags" not in [a["name"] for a in header(tmp_path / "plain.bin")["arrays"]]
    idx.add(c.xb[n1:n], ids[n1:].tolist(), tags=tags[n1:])         # the first tags: earlier rows read 0
    assert any(t is idx._tags for t in idx.resident_tensors())
    got = idx.get_tags().cpu().numpy().view(np.uint64)
    assert not got[:n1].any() and np.array_equal(got[n1:], tags[n1:])
    with pytest.raises(ValueError):
        idx.add(c.xb[:2], [1, 2], tags=[1, 2, 3])
    with pytest.raises(ValueError):
        idx.set_tags(tags[:-1])
    assert idx.index.ntotal == n
    before = idx._tags
    idx.set_tags(tags)                                             # out of place: the old tensor is not written
    assert idx._tags is not before and not before[:n1].any()
    assert np.array_equal(idx.get_tags().cpu().numpy().view(np.uint64), tags)

    stored = idx._xb[:n].clone()

    def result(index, **kw):
        I, D = index.search_device(c.qn[:nq].contiguous(), k, normalize=False, **masks, **kw)
        return I.cpu().numpy(), D.cpu().numpy()

    rD, rI = eo.expected(stored.cpu().numpy(), c.xq[:nq], k, tags, c.a[:nq], c.y[:nq])
    I, D = result(idx, return_positions=True)
    c.check(D, I, rD, rI)
    wantI, wantD = result(idx)
    # save / load
    idx.save(str(tmp_path / "tagged.bin"))
    assert "tags" in [a["name"] for a in header(tmp_path / "tagged.bin")["arrays"]]
    back = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    back.load(str(tmp_path / "tagged.bin"))
    assert np.array_equal(back.get_tags().cpu().numpy().view(np.uint64), tags)
    gI, gD = result(back)
    assert np.array_equal(gI, wantI) and np.array_equal(gD, wantD)
    plain = FAISSIndex(dim, index_type="Flat", prefilter=prefilter)
    plain.load(str(tmp_path / "plain.bin"))
    assert plain._tags is None
    # remove_ids: the filtered search of what is left equals a fresh index over the surviving rows and tags
    gone = np.random.default_rng(3).choice(n, size=n // 3, replace=False)
    keep = np.setdiff1d(np.arange(n), gone)
    assert idx.remove_ids(ids[gone].tolist()) == len(gone)
    assert np.array_equal(idx.get_tags().cpu().numpy().view(np.uint64), tags[keep])
    fresh = _index(c.xb[keep], prefilter, tags[keep], stored=stored[_dev(keep)])
    aI, aD = result(idx, return_positions=True)
    bI, bD = result(fresh, return_positions=True)
    fin = aI >= 0
    assert np.array_equal(aI, bI) and np.array_equal(np.isfinite(aD), fin) and np.array_equal(np.isfinite(bD), fin)
    assert np.array_equal(aD, bD) if c.engine == "mixed" else np.abs(aD[fin] - bD[fin]).max() <= fo.score_tol(dim, engine="fp32")
    assert np.array_equal(result(idx)[0], np.where(aI >= 0, ids[keep][np.maximum(aI, 0)], ids[keep][-1]))
    # the numpy-level calls slice the masks with the query chunks
    hI, hD = idx.batch_search(c.xq[:nq], k, batch_size=16, require_all=c.a[:nq], require_any=c.y[:nq])
    sI, sD = idx.search(c.xq[:nq], k, require_all=[int(v) for v in c.a[:nq]], require_any=[int(v) for v in c.y[:nq]])
    assert np.array_equal(hI, sI) and np.array_equal(hD, sD)
    assert np.array_equal(np.isfinite(hD), aI >= 0)


# ---- 10. the serving pipeline -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [6, 36])
def test_pipeline_filters_stage_one(B):
    from tests.test_exclude_gpu import _rec, _users
    n_ads, top_k, k1 = 12_288, 10, 200
    rec, user, nnum = _rec(n_ads)
    gone, _, _ = _rec(n_ads)
    tags = eo.tags_for(n_ads, 44)
    rec.faiss_index.set_tags(tags)
    users = _users(user, B, 5)
    uc, un = rec.preprocess_batch(users)
    sets = [(eo.B0 | eo.B63, 0), (eo.B63, eo.B0 | eo.B32)]
    outs = []
    for a, y in sets:
        ma, my = _words(np.full(B, a, dtype=np.uint64)), _words(np.full(B, y, dtype=np.uint64))
        out = {k_: (v.clone() if isinstance(v, torch.Tensor) else v)
               for k_, v in rec.recommend_device(uc, un, top_k, k1, require_all=ma, require_any=my).items()}
        outs.append((ma, my, out))
        ok = el.eligible(tags, [a], [y])[0]
        assert ok[out["ad_ids"].cpu().numpy()].all() and ok[out["candidate_ids"].cpu().numpy()].all()
    # the same request after every ineligible ad has left the corpus (unique ids, one mask for all users)
    a, y = sets[0]
    ok = el.eligible(tags, [a], [y])[0]
    assert gone.remove_ads(np.nonzero(~ok)[0].tolist()) == int((~ok).sum())
    want = gone.recommend_device(uc, un, top_k, k1)
    got = outs[0][2]
    assert torch.equal(got["ad_ids"], want["ad_ids"]) and torch.equal(got["scores"], want["scores"])
    assert torch.equal(got["candidate_ids"], want["candidate_ids"]) and torch.equal(got["candidate_scores"], want["candidate_scores"])
    # the reference API agrees
    res = rec.batch_recommend(users, top_k, k1, require_all=a, require_any=[y] * B)
    assert [r["ad_ids"] for r in res] == got["ad_ids"].cpu().tolist()
    assert [r["scores"]["ctr"] for r in res] == got["scores"][0].cpu().tolist()
    assert rec.recommend_ads(users[1], top_k, k1, require_all=a, require_any=y)["ad_ids"] == got["ad_ids"][1].cpu().tolist()
    assert rec.recommend_tensors(uc, un, top_k, k1, require_all=np.full(B, a, dtype=np.uint64))[2]["ad_ids"] == got["ad_ids"][2].cpu().tolist()
    plain = rec.recommend_device(uc, un, top_k, k1)
    assert rec.recommend_ads(users[1], top_k, k1)["ad_ids"] == plain["ad_ids"][1].cpu().tolist()
    # a graph captured with eligibility replays the eager result for both mask sets; one captured without raises on masks
    g = rec.capture(B, top_k, k1, eligibility=True)
    for ma, my, out in outs:
        r = g(uc, un, require_all=ma, require_any=my)
        assert torch.equal(r["ad_ids"], out["ad_ids"]) and torch.equal(r["scores"], out["scores"])
    r = g(uc, un)                                                   # None: zeros, no constraint
    assert torch.equal(r["ad_ids"], plain["ad_ids"]) and torch.equal(r["scores"], plain["scores"])
    g0 = rec.capture(B, top_k, k1)
    assert torch.equal(g0(uc, un)["ad_ids"], plain["ad_ids"])
    with pytest.raises(ValueError, match="eligibility"):
        g0(uc, un, require_all=outs[0][0])


def test_ivf_index_refuses_masks():
    from amdrec.index import FAISSIndex
    xb, xq = fo.case_inputs(dict(n=2000, dim=32, nq=4, kind="lifted", seed=1))
    idx = FAISSIndex(32, index_type="IVF", nlist=8, nprobe=2)
    idx.add(xb)
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx.search_device(_dev(xq), 5, require_all=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx.search(xq, 5, require_any=[1, 1, 1, 1])
