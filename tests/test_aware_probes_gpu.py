"""GPU: aware probes (amdrec.probes; FAISSIndex(index_type="IVF" / "IVFPQ", aware_probes=True)).

Every check is bit for bit and none of the references runs the new kernels: the summaries against numpy; the aware key table
against the PLAIN export's table re-keyed in numpy under the rule; the probes against the numpy oracle fed the plain table's
scores; the aware search against the existing search run with ``coarse_probes`` replaced by the oracle's probes.  Shapes: the
coarse kernel's three query-tile classes and the odd-nlist padding, (nlist, nprobe, nq) = (32, 16, 3), (257, 20, 48),
(100, 100, 130), at dims 8, 100 and 256, on a few thousand rows around hand-built centroids of which a third get no row."""
import functools

import numpy as np
import pytest
import torch

from amdrec import _lib, probes
from tests import ivf_oracle as io

pytestmark = pytest.mark.gpu

SHAPES = [(32, 16, 3), (257, 20, 48), (100, 100, 130)]
DIMS = (8, 100, 256)
N_ROWS = 3000
B63, RARE, ONES = np.uint64(1) << np.uint64(63), np.uint64(1) << np.uint64(9), np.uint64((1 << 64) - 1)
WEIGHTS = (0.0, 1.0, -1.0, 0.25, 4.0, -0.5)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(a):
    return _dev(np.asarray(a, dtype=np.uint64).view(np.int64))


@functools.lru_cache(maxsize=None)
def _corpus(dim, nlist, n=N_ROWS):
    """-> (unit rows, unit centroids, tags uint64, boosts float32, the list that holds the RARE rows' source).  Rows lie
    around two thirds of the centroids, so the other lists stay empty; the tags follow the source centroid (cluster-
    correlated), bit 63 included; RARE sits on a third of the rows of ONE source centroid."""
    cent = io.clustered(nlist, dim, 12, 700 + dim + nlist)
    rng = np.random.default_rng(1000 * dim + nlist)
    live = rng.permutation(nlist)[:max(2, 2 * nlist // 3)]
    src = live[rng.integers(0, len(live), n)]
    x = cent[src] + 0.05 * rng.standard_normal((n, dim)).astype(np.float32)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    tags = (np.uint64(1) << (src % 5).astype(np.uint64)) | np.where(src % 7 == 0, B63, np.uint64(0))
    rare_rows = np.flatnonzero(src == live[0])[::3]
    tags[rare_rows] |= RARE
    boosts = (0.02 * rng.standard_normal(n)).astype(np.float32)
    boosts[rng.choice(n, 30, replace=False)] = 0.5
    boosts[rng.choice(n, 30, replace=False)] = -1.0
    return x, cent, tags, boosts, int(live[0])


def _masks(nq):
    """Per-query mixtures: unmasked, one common bit, bit 63 in require_any, the rare bit (few feasible lists), every bit
    (no feasible list), all + any."""
    a, y = np.zeros(nq, np.uint64), np.zeros(nq, np.uint64)
    for q in range(nq):
        c = q % 6
        if c == 1:
            a[q] = np.uint64(1) << np.uint64(q % 5)
        elif c == 2:
            y[q] = B63
        elif c == 3:
            a[q] = RARE
        elif c == 4:
            a[q] = ONES
        elif c == 5:
            a[q], y[q] = np.uint64(1) << np.uint64(q % 3), B63 | np.uint64(2)
    return a, y


def _weights(nq):
    return np.array([WEIGHTS[(q // 2) % len(WEIGHTS)] for q in range(nq)], dtype=np.float32)


def _queries(dim, nq, seed):
    return io.clustered(nq, dim, 12, 800 + dim + seed)


def _ivf(dim, nlist, nprobe, aware=True, rows=None, list_boosts=True):
    from amdrec.index import FAISSIndex
    x, cent, tags, boosts, _ = _corpus(dim, nlist)
    idx = FAISSIndex(dim, index_type="IVF", nlist=nlist, nprobe=nprobe, list_tags=True, list_boosts=list_boosts,
                     aware_probes=aware)
    idx.set_trained_centroids(cent)
    sl = slice(None) if rows is None else rows
    idx.add(x[sl], tags=tags[sl], **({"boosts": boosts[sl]} if list_boosts else {}))
    return idx


def _normalized(idx, q):
    return idx._normalize_(idx._to_device_f32(q))


def _layout(idx):
    """Make sure the list layout stands (the first search after an add lays the lists out)."""
    st = idx._ivf
    if st.lists is None or st.lists.n != idx.index.ntotal:
        idx.search_device(torch.zeros((1, idx.dimension), device="cuda"), 1, normalize=False)
    return st


# ---- the numpy side ---------------------------------------------------------------------------------------------------------
def _plain_table(cent, qn):
    """amdrec_ivf_coarse_keys -> (raw keys uint64 [nq, ld], scores float32 [nq, nlist])."""
    nlist, dim = cent.shape
    nq, ld = qn.shape[0], (nlist + 1) // 2 * 2
    keys = torch.full((nq, ld), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().amdrec_ivf_coarse_keys(_lib.ptr(cent), nlist, cent.stride(0), dim, _lib.ptr(qn), nq, qn.stride(0),
                                                  _lib.ptr(keys), ld, _lib.stream_ptr(cent.device)))
    torch.cuda.synchronize()
    raw = keys.cpu().numpy().view(np.uint64)
    c, pos = io.decode_keys(raw[:, :nlist])
    assert (pos == np.arange(nlist)[None, :]).all()
    return raw, c


def _aware_table(cent, qn, lens, tag_or=None, ma=None, my=None, hi=None, lo=None, w=None):
    nlist, dim = cent.shape
    nq, ld = qn.shape[0], (nlist + 1) // 2 * 2
    keys = torch.full((nq, ld), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().amdrec_ivf_coarse_keys_aware(
        _lib.ptr(cent), nlist, cent.stride(0), dim, _lib.ptr(qn), nq, qn.stride(0), _lib.ptr(keys), ld, _lib.ptr(lens),
        _lib.ptr(tag_or), _lib.ptr(ma), _lib.ptr(my), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(w), _lib.stream_ptr(cent.device)))
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


def _host_summaries(idx):
    """The summaries of the index's current layout in numpy, from its tags and boosts in insertion order."""
    st = idx._ivf
    off, spos = st.lists.off.cpu().numpy(), st.lists.spos.cpu().numpy()
    tags = idx.get_tags().cpu().numpy()[spos]
    boosts = idx.get_boosts().cpu().numpy()[spos] if getattr(idx, "_boosts", None) is not None else None
    return (np.diff(off),) + probes.list_summaries(off, tags, boosts)


def _oracle_probes(idx, qn, ma=None, my=None, w=None):
    """The rule in numpy over the PLAIN table's scores and the host summaries -> int64 [nq, nprobe]."""
    from amdrec.ivf import search_nprobe
    st = _layout(idx)
    lens, tag_or, hi, lo = _host_summaries(idx)
    _, c = _plain_table(st.centroids, qn)
    kw = {}
    if ma is not None:
        kw.update(tag_or=tag_or, require_all=ma, require_any=my)
    if w is not None:
        kw.update(boost_hi=hi, boost_lo=lo, weight=w)
    return probes.aware_probes(c, search_nprobe(idx.nprobe, idx.nlist), lens, **kw)[0]


def _search(idx, qn, k, ma=None, my=None, w=None, policy=None):
    kw = {}
    if ma is not None:
        kw.update(require_all=_words(ma), require_any=_words(my))
    if w is not None:
        kw.update(boost_weight=_dev(w))
    pos, D = idx.search_device(qn, k, normalize=False, return_positions=True, probe_policy=policy, **kw)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), D.cpu().numpy()


def _bits_equal(a, b):
    (pa, da), (pb, db) = a, b
    assert np.array_equal(pa, pb)
    assert np.array_equal(da.view(np.uint32), db.view(np.uint32))


def _check_search_against_oracle_probes(idx, qn, k, monkeypatch, ma=None, my=None, w=None):
    """The aware search == the existing search run on the oracle's probes, bit for bit.  -> (the oracle's probes, result)."""
    want_probes = _oracle_probes(idx, qn, ma, my, w)
    got = _search(idx, qn, k, ma, my, w)
    fixed = _dev(want_probes)
    with monkeypatch.context() as m:
        m.setattr(idx._ivf, "coarse_probes", lambda q, nprobe, keys=None, **kw: fixed[:q.shape[0], :nprobe].contiguous())
        want = _search(idx, qn, k, ma, my, w, policy="similarity")
    _bits_equal(got, want)
    return want_probes, got


# ---- 1. summaries -----------------------------------------------------------------------------------------------------------
def test_summaries_equal_numpy_bit_for_bit():
    """amdrec_ivf_list_summaries called directly: more lists than the launch has waves (4096: the grid-stride loop), empty
    lists, one-row lists, lists shorter and longer than a wave's 64 lanes; tags only, boosts only, both."""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    nlist = 4096 + 37
    lens = rng.integers(0, 90, nlist)
    lens[rng.choice(nlist, 400, replace=False)] = 0
    lens[rng.choice(nlist, 200, replace=False)] = 1
    lens[[0, 4095, 4096, nlist - 1]] = [1, 0, 700, 65]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    tags = rng.integers(0, 1 << 62, n).astype(np.uint64) & rng.integers(0, 1 << 62, n).astype(np.uint64) & \
        rng.integers(0, 1 << 62, n).astype(np.uint64)
    tags[rng.choice(n, n // 50, replace=False)] |= B63
    boosts = rng.standard_normal(n).astype(np.float32)
    boosts[rng.choice(n, n // 10, replace=False)] = 0.0
    want = probes.list_summaries(off, tags, boosts)
    d_off, d_tags, d_boosts = _dev(off), _words(tags), _dev(boosts)
    for use_tags, use_boosts in ((True, True), (True, False), (False, True)):
        t = torch.full((nlist,), -1, dtype=torch.int64, device="cuda")
        hi = torch.full((nlist,), float("nan"), dtype=torch.float32, device="cuda")
        lo = torch.full((nlist,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.amdrec_ivf_list_summaries(_lib.ptr(d_off), nlist, _lib.ptr(d_tags) if use_tags else None,
                                                 _lib.ptr(d_boosts) if use_boosts else None, _lib.ptr(t), _lib.ptr(hi),
                                                 _lib.ptr(lo), _lib.stream_ptr(t.device)))
        torch.cuda.synchronize()
        if use_tags:
            assert np.array_equal(t.cpu().numpy().view(np.uint64), want[0])
        else:
            assert (t == -1).all()                                       # not written
        if use_boosts:
            assert np.array_equal(hi.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
            assert np.array_equal(lo.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
        else:
            assert torch.isnan(hi).all() and torch.isnan(lo).all()
    assert want[0][4095] == 0 and want[1][4095] == 0.0 and (lens == 0).sum() > 300


@pytest.mark.parametrize("dim", DIMS)
def test_an_index_keeps_the_summaries_of_its_layout(dim):
    idx = _ivf(dim, 100, 10)
    st = _layout(idx)
    lens, tag_or, hi, lo = _host_summaries(idx)
    assert (lens == 0).any() and (lens == st.lists.lens.cpu().numpy()).all()
    assert np.array_equal(st.list_tag_or.cpu().numpy().view(np.uint64), tag_or)
    assert np.array_equal(st.list_boost_hi.cpu().numpy().view(np.uint32), hi.view(np.uint32))
    assert np.array_equal(st.list_boost_lo.cpu().numpy().view(np.uint32), lo.view(np.uint32))
    kept = st.resident_tensors()
    assert all(any(t is k for k in kept) for t in (st.list_tag_or, st.list_boost_hi, st.list_boost_lo))
    plain = _ivf(dim, 100, 10, aware=False)                              # without the flag: no summaries, nothing launched
    _layout(plain)
    assert plain._ivf.list_tag_or is None and plain._ivf.list_boost_hi is None and plain._ivf.list_tags is not None


# ---- 2. the key table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nlist, nprobe, nq", SHAPES)
def test_key_table_equals_the_plain_table_rekeyed_in_numpy(dim, nlist, nprobe, nq):
    rng = np.random.default_rng(dim + nlist)
    cent_h = io.clustered(nlist, dim, 12, 700 + dim + nlist)
    cent_h[5, 0] = np.nan                                                # a NaN score files as the plain table files it
    cent, qn = _dev(cent_h), _dev(_queries(dim, nq, nq))
    raw_plain, c = _plain_table(cent, qn)
    lens = rng.integers(0, 3, nlist).astype(np.int64)
    tag_or = (rng.integers(0, 32, nlist).astype(np.uint64) | np.where(rng.integers(0, 2, nlist) == 1, B63, np.uint64(0)))
    rare = rng.choice(nlist, 2, replace=False)
    lens[rare] = 2
    tag_or[rare] |= RARE
    tag_or[lens == 0] = 0
    hi = rng.standard_normal(nlist).astype(np.float32)
    lo = (hi - np.abs(rng.standard_normal(nlist))).astype(np.float32)
    a, y = _masks(nq)
    w = _weights(nq)
    d = dict(lens=_dev(lens), tag_or=_words(tag_or), ma=_words(a), my=_words(y), hi=_dev(hi), lo=_dev(lo), w=_dev(w))
    pos = np.arange(nlist)[None, :]

    def want(masked, boosted):
        s = probes.rank_last(probes.aware_scores(c, hi, lo, w if boosted else None))
        ok = probes.feasible(lens, tag_or if masked else None, a, y, nq=nq)
        return np.where(ok, io.make_keys(s, np.broadcast_to(pos, s.shape)), np.uint64(0)), ok

    for masked, boosted in ((True, True), (True, False), (False, True), (False, False)):
        got = _aware_table(cent, qn, d["lens"], *((d["tag_or"], d["ma"], d["my"]) if masked else (None, None, None)),
                           *((d["hi"], d["lo"], d["w"]) if boosted else (None, None, None)))
        exp, ok = want(masked, boosted)
        assert np.array_equal(got[:, :nlist], exp), (masked, boosted)
        if nlist % 2:
            assert (got[:, nlist] == 0).all()                            # the odd-nlist padding key is written as 0
        if masked and nq >= 6:                                           # (the six-query cycle of _masks is complete)
            n_ok = ok.sum(axis=1)
            assert (n_ok == 0).any() and ((n_ok > 0) & (n_ok < nprobe)).any() and (n_ok >= min(nprobe, 3)).any()
    # all-zero masks and no weight on non-empty lists: exactly the plain table
    ones = _dev(np.ones(nlist, dtype=np.int64))
    zeros = _words(np.zeros(nq, dtype=np.uint64))
    got = _aware_table(cent, qn, ones, d["tag_or"], zeros, zeros)
    assert np.array_equal(got[:, :nlist], raw_plain[:, :nlist])
    # w == 0 for every query: the plain scores as numbers (c + 0 * b), the same order
    got = _aware_table(cent, qn, ones, None, None, None, d["hi"], d["lo"], _dev(np.zeros(nq, dtype=np.float32)))
    s0, _ = io.decode_keys(got[:, :nlist])
    assert np.array_equal(s0, probes.rank_last(c))


# ---- 3. probes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nlist, nprobe, nq", SHAPES)
def test_probes_equal_the_oracle_also_from_a_chunked_table(dim, nlist, nprobe, nq, monkeypatch):
    from amdrec import ivf
    idx = _ivf(dim, nlist, nprobe)
    st = _layout(idx)
    qn = _normalized(idx, _queries(dim, nq, 1))
    a, y = _masks(nq)
    w = _weights(nq)
    assert (st.lists.lens == 0).any()
    for ma, my, wt in ((a, y, None), (None, None, w), (a, y, w)):
        want = _oracle_probes(idx, qn, ma, my, wt)
        elig = None if ma is None else (_words(ma), _words(my))
        boost = None if wt is None else (_dev(wt), idx._boost_max)
        got = st.coarse_probes(qn, nprobe, elig=elig, boost=boost)
        assert np.array_equal(got.cpu().numpy(), want)
        if ma is not None and nq >= 6:
            tail = (want == -1).sum(axis=1)
            assert (tail == nprobe).any() and ((tail > 0) & (tail < nprobe)).any()      # no feasible list; fewer than nprobe
        if nq > 4:
            with monkeypatch.context() as m:                             # the table of all queries does not fit: chunks of 4
                m.setattr(ivf, "POOL_BYTES", 4 * st.coarse_ld * 8 + 8)
                assert st.coarse_table_bytes(nq, nprobe) == 0 and st.aware_table_rows(nq) == 4
                chunked = st.coarse_probes(qn, nprobe, elig=elig, boost=boost)
            assert torch.equal(chunked, got)
    # a search with neither takes the plain coarse path: the plain probes
    plain = st.coarse_probes(qn, nprobe)
    _, c = _plain_table(st.centroids, qn)
    order = np.stack([np.lexsort((np.arange(nlist), -c[q].astype(np.float64)))[:nprobe] for q in range(nq)])
    assert np.array_equal(plain.cpu().numpy(), order)


# ---- 4. the search result on every path -------------------------------------------------------------------------------------
def _modes(nq):
    a, y = _masks(nq)
    w = _weights(nq)
    return {"masks": (a, y, None), "boost": (None, None, w), "both": (a, y, w)}


@pytest.mark.parametrize("mode", ["masks", "boost", "both"])
@pytest.mark.parametrize("dim", DIMS)
def test_search_equals_the_existing_search_on_the_oracle_probes(dim, mode, monkeypatch):
    """Pair scan (3 queries), two-phase grouped scans (48 x 20 of 257 lists: 2 first-phase probes; 130 x 100 of 100: 12),
    the single-phase grouped scan and the bf16-prefiltered second phase (dims 8 and 256)."""
    from amdrec import ivf
    monkeypatch.setenv("AMDREC_IVF_MIXED", "0")
    k = 10
    for nlist, nprobe, nq in SHAPES:
        idx = _ivf(dim, nlist, nprobe)
        qn = _normalized(idx, _queries(dim, nq, 2))
        ma, my, w = _modes(nq)[mode]
        grouped = ivf.use_grouped_scan(nq, nprobe, nlist)
        assert grouped == (nq > 3) and (nprobe >= ivf.TWO_PHASE_MIN_PROBES)
        want_probes, _ = _check_search_against_oracle_probes(idx, qn, k, monkeypatch, ma, my, w)
        if grouped and ma is not None:                                   # a -1 tail inside the first phase's columns
            first = ivf.first_phase_probes(nprobe)
            short = (want_probes[:, :first] == -1).any(axis=1) & (want_probes[:, 0] >= 0)
            assert short.any() or nlist == 257
        if grouped:
            with monkeypatch.context() as m:                             # the grouped scan in one unfiltered phase
                m.setattr(ivf, "TWO_PHASE_MIN_PROBES", 1 << 20)
                _check_search_against_oracle_probes(idx, qn, k, monkeypatch, ma, my, w)
            if dim % 8 == 0:
                with monkeypatch.context() as m:                         # second phase on the bf16 shadow
                    m.setenv("AMDREC_IVF_MIXED", "1")
                    _check_search_against_oracle_probes(idx, qn, k, monkeypatch, ma, my, w)


PQ_N, PQ_DIM, PQ_NLIST, PQ_NPROBE = 4096, 64, 16, 4


@functools.lru_cache(maxsize=None)
def _pq_rows():
    x = io.clustered(PQ_N, PQ_DIM, 16, 31)
    rng = np.random.default_rng(32)
    tags = np.uint64(1) << rng.integers(0, 5, PQ_N).astype(np.uint64)
    tags[rng.choice(PQ_N, 40, replace=False)] |= B63
    tags[np.flatnonzero(x @ x[0] > 0.8)[:60:2]] |= RARE                 # the rare tag on rows of one cluster only
    return x, tags


@pytest.mark.parametrize("refine", [None, "fp32"])
def test_ivfpq_search_equals_the_existing_search_on_the_oracle_probes(refine, monkeypatch):
    from amdrec.index import FAISSIndex
    x, tags = _pq_rows()
    idx = FAISSIndex(PQ_DIM, index_type="IVFPQ", nlist=PQ_NLIST, nprobe=PQ_NPROBE, pq_m=8, refine=refine, list_tags=True,
                     aware_probes=True)
    idx.train(x)
    idx.add(x, tags=tags)
    nq, k = 40, 10
    qn = _normalized(idx, io.clustered(nq, PQ_DIM, 16, 33))
    a, y = _masks(nq)
    want_probes, got = _check_search_against_oracle_probes(idx, qn, k, monkeypatch, a, y)
    tail = (want_probes == -1).sum(axis=1)
    assert (tail == PQ_NPROBE).any() and ((tail > 0) & (tail < PQ_NPROBE)).any()
    rare = np.flatnonzero(a == RARE)
    assert (got[0][rare] >= 0).any()                                     # the rare rows are found
    with pytest.raises(NotImplementedError):                             # IVFPQ still takes no boost
        idx.search_device(qn, k, normalize=False, boost_weight=1.0)


# ---- 5. the superset property -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_masked_aware_result_is_never_worse_than_the_similarity_result(dim):
    """Masks only: the plain probes' feasible lists are a subset of the aware probes (both orders are by c; the aware one
    skips infeasible lists), so per query the filled count and the k-th score can only grow."""
    k = 10
    for nlist, nprobe, nq in SHAPES[:2]:
        idx = _ivf(dim, nlist, max(2, nprobe // 4))
        qn = _normalized(idx, _queries(dim, nq, 4))
        a, y = _masks(nq)
        pa, da = _search(idx, qn, k, a, y)
        ps, ds = _search(idx, qn, k, a, y, policy="similarity")
        assert ((pa >= 0).sum(axis=1) >= (ps >= 0).sum(axis=1)).all()
        assert (da[:, k - 1] >= ds[:, k - 1]).all()
        if nq >= 6:
            assert ((pa >= 0).sum(axis=1) > (ps >= 0).sum(axis=1)).any()    # and it does grow for some query


@pytest.mark.parametrize("dim", DIMS)
def test_a_rare_tag_far_from_the_query_is_found(dim):
    """The constructed case: the rare tag sits in lists far from the query; similarity returns fewer than k, aware fills k -
    checked against brute force over the lists the rule chooses."""
    nlist, nprobe, k = 32, 4, 5
    x, cent, tags, _, rare_list = _corpus(dim, nlist)
    idx = _ivf(dim, nlist, nprobe)
    far = int(np.argmin(cent @ cent[rare_list]))
    qn = _normalized(idx, cent[far][None, :].copy())
    a, y = np.array([RARE], np.uint64), np.zeros(1, np.uint64)
    ps, _ = _search(idx, qn, k, a, y, policy="similarity")
    pa, da = _search(idx, qn, k, a, y)
    assert (ps[0] >= 0).sum() < k and (pa[0] >= 0).all()
    chosen = _oracle_probes(idx, qn, a, y)[0]
    assign = idx._ivf.assign.cpu().numpy()
    rows = np.flatnonzero(np.isin(assign, chosen[chosen >= 0]) & ((tags & RARE) != 0))
    assert len(rows) >= k
    xn, q = _normalized(idx, x).cpu().numpy().astype(np.float64), qn.cpu().numpy().astype(np.float64)[0]
    s = xn[rows] @ q
    best = np.sort(s)[::-1]
    tol = io.score_tol(dim)
    assert np.isin(pa[0], rows).all() and len(set(pa[0].tolist())) == k
    assert np.abs(da[0].astype(np.float64) - xn[pa[0]] @ q).max() <= tol
    assert np.abs(np.sort(da[0].astype(np.float64))[::-1] - best[:k]).max() <= tol


# ---- 6. life cycle ----------------------------------------------------------------------------------------------------------
def test_summaries_follow_the_corpus(tmp_path, monkeypatch):
    from amdrec.index import FAISSIndex
    dim, nlist, nprobe, nq, k = 100, 100, 10, 33, 10
    x, cent, tags, boosts, _ = _corpus(dim, nlist)
    half = N_ROWS // 2
    idx = _ivf(dim, nlist, nprobe, rows=slice(0, half))
    qn = _normalized(idx, _queries(dim, nq, 5))
    a, y = _masks(nq)
    w = _weights(nq)

    def check(i=idx):
        st = _layout(i)
        lens, tag_or, hi, lo = _host_summaries(i)
        assert np.array_equal(st.list_tag_or.cpu().numpy().view(np.uint64), tag_or)
        assert np.array_equal(st.list_boost_hi.cpu().numpy().view(np.uint32), hi.view(np.uint32))
        assert np.array_equal(st.list_boost_lo.cpu().numpy().view(np.uint32), lo.view(np.uint32))
        return _check_search_against_oracle_probes(i, qn, k, monkeypatch, a, y, w)[1]
    check()
    st = idx._ivf
    old = (st.list_tag_or, st.list_tag_or.clone(), st.list_boost_hi, st.list_boost_hi.clone())
    rng = np.random.default_rng(9)
    idx.set_tags(np.roll(tags[:half], 7))                                # a swap: new summaries, out of place
    assert st.list_tag_or is not old[0] and torch.equal(old[0], old[1]) and st.list_boost_hi is old[2]
    check()
    idx.set_boosts(rng.standard_normal(half).astype(np.float32))
    assert st.list_boost_hi is not old[2] and torch.equal(old[2], old[3])
    check()
    idx.add(x[half:], tags=tags[half:], boosts=boosts[half:])            # the layout is dropped and rebuilt with its summaries
    check()
    assert idx.remove_ids(list(range(0, N_ROWS, 3))) == len(range(0, N_ROWS, 3))
    before = check()
    path = str(tmp_path / "ix")
    idx.save(path)
    loaded = FAISSIndex(dim, index_type="IVF", nlist=nlist, nprobe=nprobe)
    loaded.load(path)
    assert loaded.aware_probes is True and loaded._ivf.aware_probes is True
    _bits_equal(check(loaded), before)
    late = _ivf(dim, nlist, nprobe, aware=False)                         # opting in a built index
    _layout(late)
    assert late._ivf.list_tag_or is None
    with pytest.raises(ValueError, match=r"enable_aware_probes\(\)"):
        late.search_device(qn, k, normalize=False, probe_policy="aware")
    late.enable_aware_probes()
    assert late._ivf.list_tag_or is not None and late._ivf.list_boost_lo is not None
    _bits_equal(check(late), _search(_ivf(dim, nlist, nprobe), qn, k, a, y, w))


def test_a_captured_graph_keeps_its_summaries():
    from tests import eligible_oracle as eo
    from tests.test_exclude_gpu import _users
    from tests.test_ivf_eligible_gpu import _ivf_rec
    n_ads, B, top_k, k1 = 12_288, 6, 10, 200
    rec, user = _ivf_rec(n_ads, True)
    index = rec.faiss_index
    index.enable_aware_probes()
    rng = np.random.default_rng(5)
    tags = eo.tags_for(n_ads, 44)
    tags[rng.choice(n_ads, 60, replace=False)] |= RARE
    index.set_tags(tags)
    uc, un = rec.preprocess_batch(_users(user, B, 5))
    ma, my = _words(np.full(B, RARE, dtype=np.uint64)), _words(np.zeros(B, dtype=np.uint64))
    eager = {k_: v.clone() for k_, v in rec.recommend_device(uc, un, top_k, k1, require_all=ma, require_any=my).items()
             if isinstance(v, torch.Tensor)}
    sim = index.search_device(rec.two_tower_model.user_tower.encode(uc, un, check_indices=False, renormalize=True), k1,
                              normalize=False, return_positions=True, require_all=ma, require_any=my,
                              probe_policy="similarity")[0]
    assert (eager["candidate_ids"] >= 0).sum() >= (sim >= 0).sum()
    g = rec.capture(B, top_k, k1, eligibility=True)
    r = g(uc, un, require_all=ma, require_any=my)
    assert torch.equal(r["ad_ids"], eager["ad_ids"]) and torch.equal(r["scores"], eager["scores"])
    st = index._ivf
    held, copy = st.list_tag_or, st.list_tag_or.clone()
    index.set_tags(np.roll(tags, 1000))                                  # the swap: the rare tag sits on other ads now ...
    assert st.list_tag_or is not held and torch.equal(held, copy)
    now = rec.recommend_device(uc, un, top_k, k1, require_all=ma, require_any=my)
    assert not torch.equal(now["candidate_ids"], eager["candidate_ids"])
    r = g(uc, un, require_all=ma, require_any=my)                        # ... but the graph replays on the copies it was captured with
    assert torch.equal(r["ad_ids"], eager["ad_ids"]) and torch.equal(r["scores"], eager["scores"])


# ---- 7. policy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["masks", "boost", "both", "plain"])
def test_similarity_policy_on_a_flagged_index_is_the_unflagged_index(mode):
    dim, k = 100, 10
    for nlist, nprobe, nq in SHAPES:
        flagged, plain = _ivf(dim, nlist, nprobe), _ivf(dim, nlist, nprobe, aware=False)
        qn = _normalized(flagged, _queries(dim, nq, 6))
        ma, my, w = (None, None, None) if mode == "plain" else _modes(nq)[mode]
        ref = _search(plain, qn, k, ma, my, w)
        _bits_equal(_search(flagged, qn, k, ma, my, w, policy="similarity"), ref)
        _bits_equal(_search(plain, qn, k, ma, my, w, policy="similarity"), ref)
        if mode == "plain":                                              # neither masks nor weight: the flag changes nothing
            _bits_equal(_search(flagged, qn, k), ref)
            _bits_equal(_search(flagged, qn, k, policy="aware"), ref)
