"""GPU: per-request eligibility masks inside the inverted-list scans (FAISSIndex(index_type="IVF" / "IVFPQ", list_tags=True)).

Two references, both bit for bit and neither running the filtered kernels (tests/ivf_eligible_oracle.py): R1 restricts the
index's own plain result for 2048 slots to eligible rows on the host (asserting that the plain result held the whole probed
set); R2 is the plain search of a twin index from which the ineligible ads were removed.  Scan paths are forced through
AMDREC_IVF_MIXED in the filtered search and in its reference alike."""
import functools

import numpy as np
import pytest
import torch

from amdrec import _lib, eligible as el, ivf as ivf_mod
from tests import eligible_oracle as eo, exclude_oracle, ivf_eligible_oracle as io, ivf_oracle
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

NEG, POS = np.float32(-np.inf), np.float32(np.inf)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(a):
    return _dev(el.as_words(a, len(a)))


def _ivf(x, centres, nprobe, tags, list_tags=True):
    from amdrec.index import FAISSIndex
    idx = FAISSIndex(x.shape[1], index_type="IVF", nlist=len(centres), nprobe=nprobe, list_tags=list_tags)
    idx.set_trained_centroids(centres)
    idx.add(x, tags=tags)
    return idx


@functools.lru_cache(maxsize=None)
def _corpus(name):
    x, c, _ = io.corpus(name)
    return x, c, eo.tags_for(len(x), 77)


@functools.lru_cache(maxsize=None)
def _index(name, nprobe):
    x, c, tags = _corpus(name)
    return _ivf(x, c, nprobe, tags)


def _queries(idx, name, nq):
    return idx._normalize_(idx._to_device_f32(io.queries(name, nq)))


def _search(idx, q, k, a=None, y=None, **kw):
    """-> (positions, scores) numpy"""
    if a is not None:
        kw.update(require_all=_words(a), require_any=_words(y))
    I, D = idx.search_device(q, k, normalize=False, return_positions=True, **kw)
    return I.cpu().numpy(), D.cpu().numpy()


def _check_r1(idx, q, k, tags, a, y, fill=NEG, **kw):
    """The masked search for k against R1; -> (positions, scores) of the masked search."""
    pI, pD = _search(idx, q, io.PLAIN_K)
    wD, wI = io.restrict(pI, pD, tags, a, y, k, fill)
    gI, gD = _search(idx, q, k, a, y, **kw)
    assert np.array_equal(gI, wI), np.argwhere(gI != wI)[:5]
    assert np.array_equal(gD, wD), np.argwhere(gD != wD)[:5]
    assert (gD[gI < 0] == fill).all()                                   # (a filled slot may hold the fill value too: a NaN row)
    for row in gI:                                                      # no position repeated
        f = row[row >= 0]
        assert len(np.unique(f)) == len(f)
    return gI, gD


def _profiled(fn):
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {t: int(e["launches"]) for t, e in _lib.profile_report().items()}
    finally:
        _lib.profile_enable(False)


# ---- 1. the pair scan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name", ["even36", "even64"])
def test_pair_scan(name, k):
    idx, (_, _, tags) = _index(name, 8), _corpus(name)
    nq = 3
    assert not ivf_mod.use_grouped_scan(nq, 8, 64)
    a, y = io.masks_cycle(6)
    for lo in (0, 3):                                                   # the six masks, three queries at a time
        q = _queries(idx, name, 6)[lo:lo + 3].contiguous()
        (gI, _), prof = _profiled(lambda: _check_r1(idx, q, k, tags, a[lo:lo + 3], y[lo:lo + 3]))
        assert "ivf_scan_pairs_elig" in prof and "ivf_scan_pairs" in prof
    assert (gI[2] == -1).all()                                          # the mask no row satisfies


# ---- 2. grouped, one phase ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["even36", "even72"])
def test_grouped_one_phase(name):
    idx, (_, _, tags) = _index(name, 8), _corpus(name)
    nq = 33
    assert ivf_mod.use_grouped_scan(nq, 8, 64) and 8 < ivf_mod.TWO_PHASE_MIN_PROBES
    a, y = io.masks_cycle(nq)
    q = _queries(idx, name, nq)
    for k in (10, 100):
        _check_r1(idx, q, k, tags, a, y)


# ---- 2b. query chunks: the masks are offset with the queries ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pairs", "grouped", "two_phase", "pq"])
def test_query_chunks_offset_the_masks(kind, monkeypatch):
    """A pool budget of ~14 queries: the drivers scan q[s:] chunk by chunk and must pass masks[s:] with them."""
    from amdrec import ivfpq as pq_mod
    if kind == "pq":
        idx, (_, tags), fill, nq = _pq_index(8), _pq_rows(), POS, 33
        q = _pq_queries(idx, nq)
    else:
        name, nprobe, nq = {"pairs": ("even36", 8, 15), "grouped": ("even36", 8, 33), "two_phase": ("even64", 16, 33)}[kind]
        monkeypatch.setenv("AMDREC_IVF_MIXED", "1")
        idx, (_, _, tags), fill = _index(name, nprobe), _corpus(name), NEG
        q = _queries(idx, name, nq)
    idx.search_device(q, 5, normalize=False)                            # lays the lists out: the pool's row pitch is known
    budget = 14 * idx._ivf.pool_rows_bound(idx.nprobe) * 8 + 64
    monkeypatch.setattr(ivf_mod, "POOL_BYTES", budget)
    monkeypatch.setattr(pq_mod, "POOL_BYTES", budget)
    chunks = []
    group = ivf_mod.InvertedLists.group
    monkeypatch.setattr(ivf_mod.InvertedLists, "group", lambda self, w, probes, ld, m, *a: (chunks.append(m), group(self, w, probes, ld, m, *a))[1])
    a, y = io.masks_cycle(nq)
    _check_r1(idx, q, 10, tags, a, y, fill=fill)
    assert max(chunks) <= 14 and len(set(chunks)) > 1, chunks


# ---- 3 / 4. two phases: fp32 filter, bf16 prefilter ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("nq", [33, 129])
@pytest.mark.parametrize("name", ["even64", "even72"])
@pytest.mark.parametrize("mixed", ["0", "1"])
def test_two_phase(mixed, name, nq, k, monkeypatch):
    monkeypatch.setenv("AMDREC_IVF_MIXED", mixed)
    idx, (_, _, tags) = _index(name, 16), _corpus(name)
    assert ivf_mod.use_grouped_scan(nq, 16, 64) and 16 >= ivf_mod.TWO_PHASE_MIN_PROBES
    a, y = io.masks_cycle(nq)
    q = _queries(idx, name, nq)
    _, prof = _profiled(lambda: _check_r1(idx, q, k, tags, a, y))
    want = "ivf_scan_grouped_bf16_" if mixed == "1" else "ivf_scan_grouped_"
    assert any(t.startswith(want) and t.endswith("_elig") for t in prof), prof
    assert any(t.startswith("ivf_scan_grouped_bf16_") for t in prof) == (mixed == "1"), prof


# ---- 5. a long list: 256-row tiles with a partial last tile ----------------------------------------------------------------------
@pytest.mark.parametrize("mixed", ["0", "1"])
def test_long_list_tile_tails(mixed, monkeypatch):
    monkeypatch.setenv("AMDREC_IVF_MIXED", mixed)
    idx, (_, _, tags) = _index("long64", 16), _corpus("long64")
    nq = 33
    a, y = io.masks_cycle(nq)
    q = _queries(idx, "long64", nq)
    for k in (10, 100):
        _, prof = _profiled(lambda: _check_r1(idx, q, k, tags, a, y))
        assert any(t.endswith("x256_elig") for t in prof), prof
    assert idx._ivf.lists.max_len == 1600                               # past the short-list limit (1536 rows): 256-row tiles


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq, nprobe", [(3, 8), (33, 8), (33, 16)])
def test_edges(nq, nprobe):
    x, c, _ = _corpus("even64")
    idx = _ivf(x, c, nprobe, None)
    q = _queries(idx, "even64", nq)
    idx.search_device(q, 5, normalize=False)                            # lays the lists out
    lists = idx._ivf.lists
    spos, off = lists.spos.cpu().numpy(), lists.off.cpu().numpy()
    probes = idx._ivf.coarse_probes(q, nprobe).cpu().numpy()
    B = [np.uint64(1 << b) for b in range(4)]
    tags = np.zeros(len(x), dtype=np.uint64)
    live = off[1:] > off[:-1]
    tags[spos[off[:-1][live]]] |= B[0]                                  # bit 0: the first row of every list
    tags[spos[off[1:][live] - 1]] |= B[1]                               # bit 1: the last row of every list
    dead = int(probes[0, 0])                                            # bit 2: every row outside query 0's nearest list
    tags[spos[np.r_[0:off[dead], off[dead + 1]:len(x)]]] |= B[2]
    tags[spos[off[int(probes[0, 1])]]] |= B[3]                          # bit 3: one row of query 0's second list
    idx.set_tags(tags)
    k = 20
    for bit in B:
        a = np.full(nq, bit, dtype=np.uint64)
        gI, gD = _check_r1(idx, q, k, tags, a, np.zeros(nq, dtype=np.uint64))
        if bit in (B[0], B[1]):                                         # one row per probed list: fewer than k, exact tail
            for qi in range(nq):
                n_ok = int(live[probes[qi]].sum())
                assert (gI[qi, :n_ok] >= 0).all() and (gI[qi, n_ok:] == -1).all() and np.isneginf(gD[qi, n_ok:]).all()
        if bit == B[2]:
            assert not np.isin(gI[0], spos[off[dead]:off[dead + 1]]).any()
        if bit == B[3]:
            assert gI[0, 0] == spos[off[int(probes[0, 1])]] and (gI[0, 1:] == -1).all()
    none = np.full(nq, 1 << 9, dtype=np.uint64)                         # no eligible row at all
    gI, gD = _check_r1(idx, q, k, tags, none, np.zeros(nq, dtype=np.uint64))
    assert (gI == -1).all() and np.isneginf(gD).all()


# ---- 7. a large pool through the split select --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 3])
def test_large_pool_split_select(nq, monkeypatch):
    calls = []
    select = ivf_mod.InvertedLists.select
    x, c = ivf_oracle.clustered(40000, 32, 4, 9, return_centres=True)
    tags = eo.tags_for(len(x), 12)
    ok = el.eligible(tags, [0], [eo.B32])[0]                            # f ~ 0.05
    assert 0.03 < ok.mean() < 0.07
    idx, twin = _ivf(x, c, 2, tags), _ivf(x, c, 2, tags, list_tags=False)
    kept = np.nonzero(ok)[0]
    assert twin.remove_ids(np.nonzero(~ok)[0].tolist()) == int((~ok).sum())
    rng = np.random.default_rng(4)
    qh = c[rng.integers(0, 4, nq)] + 0.3 * rng.standard_normal((nq, 32)).astype(np.float32)
    q = idx._normalize_(idx._to_device_f32(qh))
    k = 100
    tI, tD = _search(twin, q, k)
    monkeypatch.setattr(ivf_mod.InvertedLists, "select",             # (pool, pool_ld, ...): note the pool's row pitch
                        lambda self, *a, **kw: (calls.append(a[1]), select(self, *a, **kw))[1])
    gI, gD = _search(idx, q, k, np.zeros(nq, dtype=np.uint64), np.full(nq, eo.B32, dtype=np.uint64))
    assert calls and min(ivf_mod.SELECT_MAX_SLICES, calls[0] // ivf_mod.SELECT_SLICE_KEYS) >= 4     # amdrec_ivf_select_split
    assert calls[0] >= 18000                                            # ~20 000 pool slots, mostly empty keys
    assert np.array_equal(gI, io.map_kept(tI, kept)) and np.array_equal(gD, tD)
    assert (gI >= 0).all()



# ---- 8. NaN rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [3, 33])
def test_nan_rows(nq):
    x, c, tags = _corpus("even64")
    x, tags = x.copy(), tags.copy()
    bad = [5, 1000, 3000]
    x[bad, 7] = np.nan                                                  # normalised: the whole row NaN, filed under list 0
    tags[[5, 1000]] |= np.uint64(eo.B0)
    tags[3000] &= ~np.uint64(eo.B0)
    idx = _ivf(x, c, 8, tags)
    rng = np.random.default_rng(8)
    qh = c[np.zeros(nq, dtype=np.int64)] + 0.2 * rng.standard_normal((nq, 64)).astype(np.float32)
    q = idx._normalize_(idx._to_device_f32(qh))
    assert (idx._ivf.coarse_probes(q, 8).cpu().numpy() == 0).any(axis=1).all()      # every query probes list 0
    a, y = np.full(nq, eo.B0, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
    gI, gD = _check_r1(idx, q, io.PLAIN_K, tags, a, y)
    for qi in range(nq):
        filled = gI[qi][gI[qi] >= 0]
        assert filled[-2:].tolist() == [5, 1000] and 3000 not in filled
        assert np.isneginf(gD[qi, len(filled) - 2:len(filled)]).all() and np.isfinite(gD[qi, :len(filled) - 2]).all()


# ---- 9. zero masks / no masks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, nprobe, mixed", [("even36", 8, "0"), ("even72", 8, "0"), ("even64", 16, "1"), ("even72", 16, "1")])
def test_zero_masks_are_the_plain_search_and_none_runs_no_filtered_kernel(name, nprobe, mixed, monkeypatch):
    monkeypatch.setenv("AMDREC_IVF_MIXED", mixed)
    idx = _index(name, nprobe)
    for nq in (33, 129):
        q = _queries(idx, name, nq)
        z = np.zeros(nq, dtype=np.uint64)
        for k in (10, 100):
            (pI, pD), ptags = _profiled(lambda: _search(idx, q, k))
            (nI, nD), ntags = _profiled(lambda: _search(idx, q, k, require_all=None, require_any=None))
            (zI, zD), ztags = _profiled(lambda: _search(idx, q, k, z, z))
            assert not [t for t in ptags if t.endswith("_elig")] and ptags == ntags, (ptags, ntags)
            scans = [t for t in ztags if t.startswith("ivf_scan_grouped")]
            assert scans and all(t.endswith("_elig") for t in scans), ztags
            assert sorted(t[:-len("_elig")] if t.endswith("_elig") else t for t in ztags) == sorted(ptags)
            assert sum(ztags.values()) == sum(ptags.values())               # launch for launch the same pipeline
            for I, D in ((nI, nD), (zI, zD)):
                assert np.array_equal(I, pI) and np.array_equal(D, pD)


# ---- 10. IVFPQ ----------------------------------------------------------------------------------------------------------------------------
PQ_N, PQ_DIM, PQ_NLIST, PQ_NPROBE = 4096, 64, 16, 4


@functools.lru_cache(maxsize=None)
def _pq_rows(nonfinite=False):
    x, tags = ivf_oracle.clustered(PQ_N, PQ_DIM, 16, 31), eo.tags_for(PQ_N, 32)
    if nonfinite:                                                       # row 11 eligible for (b63, b0 | b32), row 700 not
        x[[11, 700, 2222, 4000], 3] = np.array([np.nan, np.inf, np.nan, -np.inf], dtype=np.float32)
        tags[11] |= np.uint64(eo.B63 | eo.B0)
        tags[700] &= ~np.uint64(eo.B63)
    return x, tags


def _pq(m, refine=None, nonfinite=False, list_tags=True, rows=None, tags=None):
    from amdrec.index import FAISSIndex
    x, t = _pq_rows(nonfinite)
    idx = FAISSIndex(PQ_DIM, index_type="IVFPQ", nlist=PQ_NLIST, nprobe=PQ_NPROBE, pq_m=m, refine=refine, refine_factor=4,
                     list_tags=list_tags)
    idx.train(_pq_rows(False)[0])
    idx.add(x if rows is None else rows, tags=t if tags is None else tags)
    return idx


@functools.lru_cache(maxsize=None)
def _pq_index(m):
    return _pq(m)


def _pq_queries(idx, nq):
    rng = np.random.default_rng(50 + nq)
    x, _ = _pq_rows()
    qh = x[rng.integers(0, PQ_N, nq)] + 0.1 * rng.standard_normal((nq, PQ_DIM)).astype(np.float32)
    return idx._normalize_(idx._to_device_f32(qh))


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("nq", [3, 33])
@pytest.mark.parametrize("m", [8, 16])
def test_ivfpq_code_scan(m, nq, k):
    idx, (_, tags) = _pq_index(m), _pq_rows()
    a, y = io.masks_cycle(nq)
    q = _pq_queries(idx, nq)
    (gI, gD), prof = _profiled(lambda: _check_r1(idx, q, k, tags, a, y, fill=POS))
    assert "ivfpq_scan_elig" in prof
    for qi in range(nq):
        f = gD[qi][gI[qi] >= 0]
        assert (np.diff(f) >= 0).all()                                  # distances ascend
    assert (gI[5::6] == -1).all() and np.isposinf(gD[5::6]).all()


def _check_r2_pq(m, refine, nonfinite, nq, k):
    x, tags = _pq_rows(nonfinite)
    a, y = eo.B63, eo.B0 | eo.B32
    ok = el.eligible(tags, [a], [y])[0]
    if nonfinite:
        assert ok[11] and not ok[700]                                   # a non-finite row on either side of the mask
    idx, twin = _pq(m, refine, nonfinite), _pq(m, refine, nonfinite, list_tags=False)
    kept = np.nonzero(ok)[0]
    assert twin.remove_ids(np.nonzero(~ok)[0].tolist()) == int((~ok).sum())
    q = _pq_queries(idx, nq)
    tI, tD = _search(twin, q, k)
    gI, gD = _search(idx, q, k, np.full(nq, a, dtype=np.uint64), np.full(nq, y, dtype=np.uint64))
    assert np.array_equal(gI, io.map_kept(tI, kept)) and np.array_equal(gD, tD)
    assert ok[gI[gI >= 0]].all()
    return gI, gD


@pytest.mark.parametrize("nq", [3, 33])
@pytest.mark.parametrize("refine", ["fp32", "bf16"])
def test_ivfpq_refine_reranks_the_best_eligible_candidates(refine, nq):
    for k in (10, 100):
        _check_r2_pq(8, refine, False, nq, k)


@pytest.mark.parametrize("refine", [None, "fp32"])
def test_ivfpq_rows_with_a_non_finite_coordinate(refine):
    for nq in (3, 33):
        gI, gD = _check_r2_pq(16, refine, True, nq, io.PLAIN_K if refine is None else 500)
        assert 700 not in gI


# ---- 11. exclusion lists compose ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["IVF", "IVFPQ"])
def test_exclusion_lists_compose(kind):
    nq, k, E = 33, 10, 7
    if kind == "IVF":
        idx, (_, _, tags), fill = _index("even36", 8), _corpus("even36"), NEG
        q = _queries(idx, "even36", nq)
    else:
        idx, (_, tags), fill = _pq_index(8), _pq_rows(), POS
        q = _pq_queries(idx, nq)
    a, y = io.masks_cycle(nq)
    cI, cD = _check_r1(idx, q, k + E, tags, a, y, fill=fill)
    rng = np.random.default_rng(2)
    excl = np.full((nq, E), -1, dtype=np.int64)
    for qi in range(nq):                                                # hits among the leaders, a miss, padding
        f = cI[qi][cI[qi] >= 0]
        take = f[rng.permutation(len(f))[:5]] if len(f) else f
        excl[qi, :len(take)] = take
        excl[qi, 5] = len(tags) + 5
    wI, wD = exclude_oracle.compact(cI, cI, cD, excl, k, fill)
    gI, gD = _search(idx, q, k, a, y, exclude=_dev(excl))
    assert np.array_equal(gI, np.asarray(wI)) and np.array_equal(gD, np.asarray(wD))


# ---- 12. the tags follow the corpus ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["IVF", "IVFPQ"])
def test_tags_follow_the_corpus(kind, tmp_path):
    from amdrec.index import FAISSIndex
    nq, k = 33, 50
    a, y = io.masks_cycle(nq)
    if kind == "IVF":
        x, c, tags = _corpus("even36")
        half = len(x) // 2
        idx = FAISSIndex(36, index_type="IVF", nlist=64, nprobe=8, list_tags=True)
        idx.set_trained_centroids(c)
        late = FAISSIndex(36, index_type="IVF", nlist=64, nprobe=8)
        late.set_trained_centroids(c)
        q, fill = idx._normalize_(idx._to_device_f32(io.queries("even36", nq))), NEG
    else:
        x, tags = _pq_rows()
        half = len(x) // 2
        idx = FAISSIndex(PQ_DIM, index_type="IVFPQ", nlist=PQ_NLIST, nprobe=PQ_NPROBE, list_tags=True)
        late = FAISSIndex(PQ_DIM, index_type="IVFPQ", nlist=PQ_NLIST, nprobe=PQ_NPROBE)
        for i in (idx, late):
            i.train(x)
        q, fill = _pq_queries(idx, nq), POS
    ids = np.arange(len(x), dtype=np.int64)
    idx.add(x[:half], ids[:half].tolist(), tags=tags[:half])
    _check_r1(idx, q, k, tags[:half], a, y, fill=fill)
    idx.add(x[half:], ids[half:].tolist(), tags=tags[half:])            # add(tags=) after a search
    _check_r1(idx, q, k, tags, a, y, fill=fill)
    other = eo.tags_for(len(x), 99)
    before = idx._ivf.list_tags
    idx.set_tags(other)                                                 # swaps the tensor: a new list-order copy, the old one untouched
    assert idx._ivf.list_tags is not before
    _check_r1(idx, q, k, other, a, y, fill=fill)
    gone = np.random.default_rng(6).choice(len(x), size=len(x) // 3, replace=False)
    keep = np.setdiff1d(ids, gone)
    assert idx.remove_ids(gone.tolist()) == len(gone)
    _check_r1(idx, q, k, other[keep], a, y, fill=fill)
    path = str(tmp_path / "ix")
    idx.save(path)
    back = FAISSIndex(x.shape[1], index_type=kind, nlist=4, nprobe=1)
    back.load(path)
    assert back.list_tags is True
    bI, bD = _check_r1(back, q, k, other[keep], a, y, fill=fill)
    gI, gD = _search(idx, q, k, a, y)
    assert np.array_equal(bI, gI) and np.array_equal(bD, gD)
    # an index built without the flag: refuses, then enable_list_tags() opts it in (and the flag is saved)
    late.add(x, tags=tags)
    late.search_device(q, k, normalize=False)
    with pytest.raises(NotImplementedError, match="follow-up"):
        late.search_device(q, k, normalize=False, require_all=_words(a))
    late.enable_list_tags()
    _check_r1(late, q, k, tags, a, y, fill=fill)
    late.save(path + "2")
    old = FAISSIndex(x.shape[1], index_type=kind, nlist=4, nprobe=1, list_tags=True)
    old.load(path + "2")
    assert old.list_tags is True
    _check_r1(old, q, k, tags, a, y, fill=fill)


# ---- 13. exact-size buffers ------------------------------------------------------------------------------------------------------------
class _GuardedTags:
    """The list-order tags and the two mask vectors of a search in guarded exact-size buffers (N words, nq words each)."""

    def __init__(self, lists_owner, a, y):
        self.owner = lists_owner
        self.a, self.y = _words(a), _words(y)
        self.bufs = []

    def install(self, monkeypatch):
        owner, this = self.owner, self

        def tail(elig, nq):
            lt = owner.refresh_list_tags()
            g = [guarded((lt.numel(),), torch.int64, "cuda"), guarded((nq,), torch.int64, "cuda"), guarded((nq,), torch.int64, "cuda")]
            for t, src in zip(g, (lt, elig[0], elig[1])):
                t.copy_(src)
            this.bufs += g
            assert g[0].numel() == owner.lists.n
            # a chunk's masks start at query s: the views stay inside the guarded vector
            return lambda s: (_lib.ptr(g[0]), _lib.ptr(g[1][s:]), _lib.ptr(g[2][s:]))
        monkeypatch.setattr(owner, "elig_tail", tail)
        return self

    def check(self):
        assert self.bufs
        for t in self.bufs:
            t.check()


@pytest.mark.parametrize("case", ["pairs", "grouped", "two_phase_fp32", "two_phase_bf16", "pq"])
def test_exact_size_buffers(case, monkeypatch):
    from tests.guarded import SplitScanWorkspace
    if case == "pq":
        idx, (_, tags), fill, nq = _pq(8), _pq_rows(), POS, 33
        q = _pq_queries(idx, nq)
    else:
        nprobe = 16 if case.startswith("two_phase") else 8
        nq = 3 if case == "pairs" else 33
        monkeypatch.setenv("AMDREC_IVF_MIXED", "1" if case == "two_phase_bf16" else "0")
        x, c, tags = _corpus("even72" if case != "pairs" else "even36")
        idx, fill = _ivf(x, c, nprobe, tags), NEG
        q = _queries(idx, "even72" if case != "pairs" else "even36", nq)
        # list lengths of 45-84 rows: every 128-row tile is a partial last tile, every 32-row round of the pair scan too
        assert bool((idx._ivf.assign.bincount() % 32 != 0).any())
    a, y = io.masks_cycle(nq)
    k = 100
    wI, wD = _search(idx, q, k, a, y)
    ws = SplitScanWorkspace().install(monkeypatch)
    gt = _GuardedTags(idx._ivf, a, y).install(monkeypatch)
    out_d, out_i = guarded((nq, k), torch.float32, "cuda", "output"), guarded((nq, k), torch.int64, "cuda", "output")
    if case == "pq":
        idx._pq.search(q, k, idx.nprobe, out_d, out_i, elig=(gt.a, gt.y))
    else:
        idx._ivf.search(idx._xb, idx._n, q, k, idx.nprobe, out_d, out_i, elig=(gt.a, gt.y))
    torch.cuda.synchronize()
    ws.check()
    gt.check()
    out_d.check()
    out_i.check()
    assert np.array_equal(out_i.cpu().numpy(), wI) and np.array_equal(out_d.cpu().numpy(), wD)
    _check_r1(idx, q, k, tags, a, y, fill=fill)


# ---- 14. the serving pipeline ------------------------------------------------------------------------------------------------------
def _ivf_rec(n_ads, list_tags):
    from amdrec.pipeline import AdRecommenderInference, Preprocessor, build_faiss_index
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    from amdrec import synth
    from tests import cases
    from tests.test_pipeline_gpu import _t
    user, ad, nnum = cases.small_dims()
    tt = TwoTowerModel(dict(user), dict(ad), nnum)
    tt.load_state_dict(_t(synth.two_tower_state(user, ad, nnum, seed=21)))
    rk = TransformerRanker(dict(user), dict(ad), nnum)
    rk.load_state_dict(_t(synth.ranker_state(user, ad, nnum, seed=22, cross_scale=1.0 / 16)))
    ad_table = synth.ad_features(ad, n_ads, seed=23)
    index = build_faiss_index(tt, ad_table, index_type="IVF", nlist=8, nprobe=4)
    if list_tags:
        index.enable_list_tags()
    rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=index, ad_features=ad_table)
    classes = {c: [f"cat_{j}" for j in range(card)] for c, card in user.items()}
    rec.preprocessor = Preprocessor(classes, [f"I{i}" for i in range(1, 14)], np.zeros(13), np.ones(13))
    return rec, user


@pytest.mark.parametrize("B", [6, 36])
def test_pipeline_on_an_opted_in_ivf_index(B):
    from tests.test_exclude_gpu import _users
    n_ads, top_k, k1 = 12_288, 10, 200
    rec, user = _ivf_rec(n_ads, True)
    gone, _ = _ivf_rec(n_ads, False)
    assert torch.equal(rec.faiss_index.centroids, gone.faiss_index.centroids)
    tags = eo.tags_for(n_ads, 44)
    rec.faiss_index.set_tags(tags)
    users = _users(user, B, 5)
    uc, un = rec.preprocess_batch(users)
    with pytest.raises(NotImplementedError, match="follow-up"):        # _host_masks refuses in step with the index
        gone.batch_recommend(users, top_k, k1, require_all=1)
    sets = [(eo.B0 | eo.B63, 0), (eo.B63, eo.B0 | eo.B32)]
    outs = []
    for a, y in sets:
        ma, my = _words(np.full(B, a, dtype=np.uint64)), _words(np.full(B, y, dtype=np.uint64))
        out = {k_: (v.clone() if isinstance(v, torch.Tensor) else v)
               for k_, v in rec.recommend_device(uc, un, top_k, k1, require_all=ma, require_any=my).items()}
        outs.append((ma, my, out))
        ok = el.eligible(tags, [a], [y])[0]
        cand = out["candidate_ids"].cpu().numpy()
        assert ok[out["ad_ids"].cpu().numpy()].all() and ok[cand[cand >= 0]].all()
    a, y = sets[0]
    ok = el.eligible(tags, [a], [y])[0]
    assert gone.remove_ads(np.nonzero(~ok)[0].tolist()) == int((~ok).sum())
    want = gone.recommend_device(uc, un, top_k, k1)
    got = outs[0][2]
    assert torch.equal(got["ad_ids"], want["ad_ids"]) and torch.equal(got["scores"], want["scores"])
    assert torch.equal(got["candidate_ids"], want["candidate_ids"]) and torch.equal(got["candidate_scores"], want["candidate_scores"])
    res = rec.batch_recommend(users, top_k, k1, require_all=a, require_any=[y] * B)
    assert [r["ad_ids"] for r in res] == got["ad_ids"].cpu().tolist()
    assert rec.recommend_ads(users[1], top_k, k1, require_all=a, require_any=y)["ad_ids"] == got["ad_ids"][1].cpu().tolist()
    plain = {k_: (v.clone() if isinstance(v, torch.Tensor) else v) for k_, v in rec.recommend_device(uc, un, top_k, k1).items()}
    g = rec.capture(B, top_k, k1, eligibility=True)
    for ma, my, out in outs:
        r = g(uc, un, require_all=ma, require_any=my)
        assert torch.equal(r["ad_ids"], out["ad_ids"]) and torch.equal(r["scores"], out["scores"])
    r = g(uc, un)                                                       # None: zeros, no constraint
    assert torch.equal(r["ad_ids"], plain["ad_ids"]) and torch.equal(r["scores"], plain["scores"])
    # the list-order tags follow remove_ads / add_ads
    drop = np.nonzero(ok)[0][:200]
    assert rec.remove_ads(drop.tolist()) == len(drop)
    left = np.setdiff1d(np.arange(n_ads), drop)
    ma, my, _ = outs[0]
    out = rec.recommend_device(uc, un, top_k, k1, require_all=ma, require_any=my)
    ids = out["ad_ids"].cpu().numpy()
    assert ok[ids].all() and not np.isin(ids, drop).any()
    assert np.array_equal(rec.faiss_index.get_tags().cpu().numpy().view(np.uint64), tags[left])
    lt = rec.faiss_index._ivf.list_tags.cpu().numpy().view(np.uint64)
    assert np.array_equal(lt, tags[left][rec.faiss_index._ivf.lists.spos.cpu().numpy()])
