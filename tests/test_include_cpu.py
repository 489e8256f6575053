"""Include lists without a GPU: the numpy oracle of the rule against a slow loop restatement, the host helpers, every refusal
before the library is touched, the lazily built id table on CPU tensors, and amdrec_include_merge's argument validation
(nothing is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

from amdrec import _lib, include
from tests import include_oracle as io_


def _case(seed):
    """Seeded R, L and scores on a grid of few distinct score values, so that ties occur at equal and at different positions."""
    rng = np.random.default_rng(seed)
    n = 60
    k = int(rng.integers(1, 24))
    I = k if seed % 4 == 0 else int(rng.integers(1, k + 1))            # I = k every fourth seed
    f = k if seed % 3 == 0 else int(rng.integers(0, k + 1))            # f < k otherwise
    grid = np.arange(-4, 5, dtype=np.float32) * np.float32(0.25)
    r_pos = np.full(k, -1, dtype=np.int64)
    r_sc = np.full(k, -np.inf, dtype=np.float32)
    p = rng.permutation(n)[:f]
    s = rng.choice(grid, size=f)
    order = np.lexsort((p, -s))
    r_pos[:f], r_sc[:f] = p[order], s[order]
    L = rng.integers(-2, n + 4, size=I).astype(np.int64)
    if f and I >= 1:
        L[int(rng.integers(0, I))] = r_pos[f - 1]                       # R's last filled slot: it must survive the eviction
    if f and I >= 3:
        L[int(rng.integers(0, I))] = r_pos[0]
    if I >= 2:
        L[I - 1] = L[0]                                                 # a duplicate
    ls = rng.choice(grid, size=I).astype(np.float32)
    if f and I >= 4:
        ls[1] = r_sc[f // 2]                                            # a tie with a kept entry, at another position
    ls[rng.random(I) < 0.15] = np.nan
    ok = None if seed % 2 else rng.random(I) < 0.8
    return r_pos, r_sc, L, n, ls, ok


@pytest.mark.parametrize("seed", range(60))
def test_oracle_equals_the_loop_restatement(seed):
    r_pos, r_sc, L, n, ls, ok = _case(seed)
    got = include.merge_oracle(r_pos, r_sc, L, n, ls, ok)
    want = io_.merge_loop(r_pos, r_sc, L, n, ls, ok)
    for g, w, what in zip(got, want, ("positions", "scores", "injected")):
        assert np.array_equal(g, w), (what, g, w)
    pos, sc, inj = got
    k = len(r_pos)
    f = int((pos >= 0).sum())
    assert (pos[f:] == -1).all() and np.isneginf(sc[f:]).all() and not inj[f:].any()
    assert ((sc[:f][:-1] > sc[:f][1:]) | ((sc[:f][:-1] == sc[:f][1:]) & (pos[:f][:-1] < pos[:f][1:]))).all()
    # every valid entry is in the output; the listed entries of R keep score and relative order
    seen = set()
    for i, p in enumerate(L):
        valid = 0 <= p < n and int(p) not in seen and not np.isnan(ls[i]) and (ok is None or ok[i])
        seen.add(int(p))
        if valid:
            assert p in pos
            if p in r_pos:
                assert not inj[list(pos).index(p)] and sc[list(pos).index(p)] == r_sc[list(r_pos).index(p)]
    assert f == min(k, int((r_pos >= 0).sum()) + int(inj.sum()))


def test_oracle_named_cases():
    r_pos = np.array([7, 3, 9, -1], dtype=np.int64)
    r_sc = np.array([0.9, 0.5, 0.1, -np.inf], dtype=np.float32)
    # padding only: R bit for bit
    pos, sc, inj = include.merge_oracle(r_pos, r_sc, [-1, -1], 20, [np.nan, np.nan])
    assert np.array_equal(pos, r_pos) and np.array_equal(sc, r_sc) and not inj.any()
    # f < k: the injected row fills the unfilled slot, nothing is evicted
    pos, sc, inj = include.merge_oracle(r_pos, r_sc, [4], 20, [0.7])
    assert pos.tolist() == [7, 4, 3, 9] and inj.tolist() == [0, 1, 0, 0]
    # two injected into one free slot: the lowest-ranked unlisted entry leaves; the listed last entry (9) stays
    pos, sc, inj = include.merge_oracle(r_pos, r_sc, [4, 9, 5], 20, [0.7, 123.0, -3.0])
    assert pos.tolist() == [7, 4, 9, 5] and inj.tolist() == [0, 1, 0, 1] and sc[2] == np.float32(0.1)
    # ties: equal scores order by position, whichever list they come from
    pos, sc, inj = include.merge_oracle(r_pos, r_sc, [2, 8], 20, [0.5, 0.5])
    assert pos.tolist() == [7, 2, 3, 8] and inj.tolist() == [0, 1, 0, 1]
    # I = k, all new: the whole of R leaves
    full = np.array([7, 3], dtype=np.int64), np.array([0.9, 0.5], dtype=np.float32)
    pos, sc, inj = include.merge_oracle(*full, [11, 12], 20, [-1.0, -2.0])
    assert pos.tolist() == [11, 12] and inj.tolist() == [1, 1]
    # NaN, out of range, duplicate, not ok
    pos, sc, inj = include.merge_oracle(*full, [11, 20, 12, 12], 20, [np.nan, 5.0, 0.6, 0.7], [True, True, True, True])
    assert pos.tolist() == [7, 12] and sc.tolist() == [np.float32(0.9), np.float32(0.6)]
    pos, sc, inj = include.merge_oracle(*full, [12], 20, [0.6], [False])
    assert pos.tolist() == [7, 3] and not inj.any()


def test_host_helpers():
    assert include.check_include(500, 64) == 64 and include.check_include(3, 3) == 3 and include.check_include(5, 0) == 0
    with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
        include.check_include(500, 65)
    with pytest.raises(ValueError, match="exceeds k = 3"):
        include.check_include(3, 4)
    with pytest.raises(ValueError):
        include.check_include(3, -1)
    blk = include.pad_inclusions([[5, 3, 5], [], (7,), np.array([1, 2], dtype=np.int32), None])
    assert blk.dtype == np.int64 and blk.tolist() == [[5, 3, 5], [-1] * 3, [7, -1, -1], [1, 2, -1], [-1] * 3]
    assert include.pad_inclusions([[1]], width=3).tolist() == [[1, -1, -1]]
    with pytest.raises(ValueError, match="width"):
        include.pad_inclusions([[1, 2, 3]], width=2)
    with pytest.raises(ValueError, match=">= 0"):
        include.pad_inclusions([[1, -1]])
    for bad in (1.0, np.float32(2), "3", True, None):
        with pytest.raises(TypeError, match="included ad ids must be integers"):
            include.pad_inclusions([[1, bad]])
    assert include.as_block(None, 3) is None and include.as_block([[], [], []], 3) is None
    arr = np.array([[4, -1], [5, 6]], dtype=np.int32)
    assert include.as_block(arr, 2).dtype == np.int64 and include.as_block(arr, 2).tolist() == arr.tolist()
    with pytest.raises(ValueError, match="2 include lists for 3 queries"):
        include.as_block(arr, 3)
    with pytest.raises(TypeError):
        include.as_block(np.zeros((2, 2), dtype=np.float32), 2)


def _bare_index(index_type="Flat"):
    from amdrec.index import FAISSIndex
    idx = FAISSIndex.__new__(FAISSIndex)                                # no device, no library
    idx.index_type, idx._host_ids, idx._n, idx._identity = index_type, None, 100, True
    return idx


def _no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_index_refusals_fire_before_the_library_is_touched(monkeypatch):
    from amdrec.index import FAISSIndex
    _no_library(monkeypatch)
    q = torch.zeros(2, 8)

    def blk(I):
        return torch.zeros((2, I), dtype=torch.int64)
    idx = _bare_index()
    with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
        FAISSIndex.search_device(idx, q, 500, include=blk(65))
    with pytest.raises(ValueError, match="exceeds k = 10"):
        FAISSIndex.search_device(idx, q, 10, include=blk(11))
    with pytest.raises(ValueError, match="left undecided"):
        FAISSIndex.search_device(idx, q, 10, include=blk(4), max_per_group=2)
    with pytest.raises(NotImplementedError, match="codes, not rows"):
        FAISSIndex.search_device(_bare_index("IVFPQ"), q, 10, include=blk(4))
    # the numpy-level calls: the same refusals, and non-integer ids
    xq = np.zeros((2, 8), dtype=np.float32)
    for call in (idx.search, idx.batch_search):
        with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
            call(xq, 500, include=[list(range(65)), []])
        with pytest.raises(ValueError, match="exceeds k = 3"):
            call(xq, 3, include=np.zeros((2, 4), dtype=np.int64))
        with pytest.raises(ValueError, match="left undecided"):
            call(xq, 10, include=[[1], [2]], max_per_group=2)
        with pytest.raises(TypeError, match="must be integers"):
            call(xq, 10, include=[[1.5], []])
        with pytest.raises(TypeError, match="must be integers"):
            call(xq, 10, include=[["ad-1"], []])
        with pytest.raises(ValueError, match="1 include lists for 2 queries"):
            call(xq, 10, include=[[1]])
    with pytest.raises(NotImplementedError, match="codes, not rows"):
        _bare_index("IVFPQ").search(xq, 10, include=[[1], []])


def test_pipeline_refusals_fire_before_the_library_is_touched(monkeypatch):
    from amdrec.pipeline import AdRecommenderInference, GraphedRecommender, TwoStageRetriever
    _no_library(monkeypatch)
    rec = AdRecommenderInference.__new__(AdRecommenderInference)
    rec.faiss_index = _bare_index()
    rec.faiss_index._groups = torch.zeros(100, dtype=torch.int64)

    def blk(I):
        return torch.zeros((1, I), dtype=torch.int64)
    with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
        rec.recommend_device(None, None, 10, 500, include_ad_ids=blk(65))
    with pytest.raises(ValueError, match="exceeds k = 20"):
        rec.recommend_device(None, None, 10, 20, include_ad_ids=blk(21))
    with pytest.raises(ValueError, match="left undecided"):
        rec.recommend_device(None, None, 10, 500, include_ad_ids=blk(3), stage1_max_per_group=2)
    users = [{"categorical": {}, "numerical": {}}]
    for call in (lambda **kw: rec.batch_recommend(users, 10, 500, **kw),
                 lambda include_ad_ids, **kw: rec.recommend_ads(users[0], 10, 500, include_ad_ids=include_ad_ids[0], **kw),
                 lambda **kw: rec.recommend_tensors(torch.zeros((1, 6), dtype=torch.int64), torch.zeros((1, 13)), 10, 500, **kw)):
        with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
            call(include_ad_ids=[list(range(65))])
        with pytest.raises(ValueError, match="left undecided"):
            call(include_ad_ids=[[1, 2]], stage1_max_per_group=2)
        with pytest.raises(TypeError, match="must be integers"):
            call(include_ad_ids=[["ad-1"]])
    with pytest.raises(ValueError, match="exceeds k = 20"):
        rec.batch_recommend(users, 10, 20, include_ad_ids=[list(range(21))])
    rec.faiss_index.index_type = "IVFPQ"
    with pytest.raises(NotImplementedError, match="codes, not rows"):
        rec.recommend_device(None, None, 10, 500, include_ad_ids=blk(3))
    with pytest.raises(NotImplementedError, match="codes, not rows"):
        rec.batch_recommend(users, 10, 500, include_ad_ids=[[1]])
    rec.faiss_index.index_type = "Flat"
    # capture: the width of the static block is held to the same limits
    with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
        GraphedRecommender(rec, 4, 10, 500, max_include=65)
    with pytest.raises(ValueError, match="exceeds k = 20"):
        rec.capture(4, 10, 20, max_include=21)
    with pytest.raises(ValueError, match="left undecided"):
        rec.capture(4, 10, 500, stage1_max_per_group=2, max_include=8)
    # the tensor-level retriever
    r = TwoStageRetriever.__new__(TwoStageRetriever)
    r.faiss_index = rec.faiss_index
    with pytest.raises(ValueError, match="AMDREC_MAX_INCLUDE = 64"):
        r.retrieve_and_rank(None, None, 500, 10, include_ad_ids=list(range(65)))
    with pytest.raises(ValueError, match="left undecided"):
        r.retrieve_and_rank(None, None, 500, 10, include_ad_ids=[1], stage1_max_per_group=2)
    with pytest.raises(TypeError, match="must be integers"):
        r.retrieve_and_rank(None, None, 500, 10, include_ad_ids=[2.5])


def test_id_table_lookup_on_cpu_tensors():
    ids = torch.tensor([40, 7, 40, 3, 7, 99], dtype=torch.int64)
    table = include.build_id_table(ids)
    got = include.lookup_positions(table, torch.tensor([[7, 40, 3], [99, 5, -1], [100, 0, 41]], dtype=torch.int64))
    assert got.tolist() == [[1, 0, 3], [5, -1, -1], [-1, -1, -1]]       # the lowest position of a repeated id; absent: -1
    empty = include.build_id_table(torch.empty((0,), dtype=torch.int64))
    assert include.lookup_positions(empty, torch.tensor([[1, 2]])).tolist() == [[-1, -1]]


def _cpu_index(monkeypatch):
    """A Flat fp32 index whose tensors live on the CPU: the row kernels are replaced by torch (nothing here searches)."""
    from amdrec import rows_edit
    from amdrec.index import FAISSIndex
    monkeypatch.setattr(FAISSIndex, "_normalize_", lambda self, t: t)

    def plan_for(keys, n, remove_sorted, device):
        key = torch.arange(n) if keys is None else keys[:n]
        kept = torch.nonzero(~torch.isin(key, torch.from_numpy(remove_sorted))).reshape(-1)
        return kept, n - kept.shape[0]
    monkeypatch.setattr(rows_edit, "plan_for", plan_for)
    monkeypatch.setattr(rows_edit, "gather_rows", lambda t, kept, n=None, out=None: t[:n][kept].clone())
    return FAISSIndex(8, index_type="Flat", prefilter="fp32", device="cpu")


def test_index_id_table_is_lazy_and_dropped_by_every_edit(monkeypatch, tmp_path):
    idx = _cpu_index(monkeypatch)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((6, 8)).astype(np.float32)
    idx.add(x)                                                          # identity ids: the ids are the positions
    want = torch.tensor([[3, 77, -1]])
    assert idx._id_positions(want) is want and idx._id_table is None
    idx = _cpu_index(monkeypatch)
    idx.add(x, [40, 7, 40, 3, 7, 99])
    assert idx._id_table is None                                        # built on first use, not by add
    assert idx._id_positions(torch.tensor([[7, 40, 5, -1]])).tolist() == [[1, 0, -1, -1]]
    table = idx._id_table
    assert table is not None
    idx._id_positions(torch.tensor([[3]]))
    assert idx._id_table is table                                       # ... and kept
    idx.add(x[:2], [5, 3])
    assert idx._id_table is None                                        # dropped by add
    assert idx._id_positions(torch.tensor([[5, 3, 40]])).tolist() == [[6, 3, 0]]
    assert idx._id_table is not None
    assert idx.remove_ids([40, 1234]) == 2                              # rows 0 and 2 leave: the positions move
    assert idx._id_table is None                                        # dropped by remove_ids
    assert idx._id_positions(torch.tensor([[7, 40, 3, 99, 5]])).tolist() == [[0, -1, 1, 3, 4]]
    idx.add(x[:1], [40])                                                # the id is back, at a new position
    assert idx._id_table is None
    assert idx._id_positions(torch.tensor([[40, 7]])).tolist() == [[6, 0]]
    path = str(tmp_path / "ix")
    idx.save(path)
    assert idx._id_table is not None
    idx.load(path)
    assert idx._id_table is None                                        # dropped by load
    assert idx._id_positions(torch.tensor([[40, 7, 8]])).tolist() == [[6, 0, -1]]
    assert idx._id_table[0].data_ptr() in {t.data_ptr() for t in idx.resident_tensors()}    # a captured graph pins it


def test_merge_entry_validates_arguments_without_a_gpu():
    """amdrec_include_merge refuses bad arguments before anything is launched; nq = 0 returns 0."""
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(nq=1, k=500, I=8, ld_i=8, ldx=256, n=1000, d=256, ldq=256, pos=p, scores=p, incl=p, X=p, Q=p, tags=None, ra=None,
             ry=None, excl=None, E=0, ld_e=0, ids=None, boosts=None, w=None, op=p, os_=p, oi=None):
        return lib.amdrec_include_merge(pos, scores, nq, k, incl, I, ld_i, X, ldx, n, d, Q, ldq, tags, ra, ry, excl, E, ld_e,
                                        ids, boosts, w, op, os_, oi, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.amdrec_last_error(), (kw, lib.amdrec_last_error())
    refused(b"k=0", k=0)
    refused(b"k=2049", k=2049)
    refused(b"n_include=0", I=0, ld_i=0)
    refused(b"n_include=65", I=65, ld_i=65)
    refused(b"n_include=8", k=7)                                        # I > k
    refused(b"ld_include=7", ld_i=7)
    refused(b"d=254", d=254)
    refused(b"d=2052", d=2052, ldx=2052, ldq=2052)
    refused(b"d=0", d=0)
    refused(b"ldx=252", ldx=252)
    refused(b"ldx=258", ldx=258)
    refused(b"ldq=255", ldq=255)
    refused(b"n_rows=-1", n=-1)
    refused(b"n_rows=4294967296", n=1 << 32)
    refused(b"go together", tags=p)
    refused(b"go together", ra=p, ry=p)
    refused(b"without an exclusion block", E=4, ld_e=4)
    refused(b"n_exclude=0", excl=p)
    refused(b"n_exclude=2048", excl=p, E=2048, ld_e=2048)
    refused(b"ld_exclude=3", excl=p, E=4, ld_e=3)
    refused(b"ids without an exclusion block", ids=p)
    refused(b"boosts and boost_w", boosts=p)
    refused(b"boosts and boost_w", w=p)
    assert call(nq=0, pos=None, scores=None, incl=None, X=None, Q=None, op=None, os_=None) == 0      # nothing to do, nulls and all
    assert call(nq=0, k=2048, I=64, ld_i=64, d=2048, ldx=2048, ldq=2048, excl=p, E=2047, ld_e=2047) == 0   # the largest shapes
    refused(b"at most 2^31 - 1", nq=1 << 31)
    for name in ("pos", "scores", "incl", "X", "Q", "op", "os_"):
        refused(b"null pointer", **{name: None})
    odd = C.c_void_p(C.addressof(buf) + 8)
    if (C.addressof(buf) + 8) % 16:
        refused(b"16-byte aligned", X=odd)
    assert "amdrec_include_merge" in _lib.exported_symbols() and _lib.MAX_INCLUDE == 64
    assert _lib.load().amdrec_abi_version() == 14 == _lib.ABI_VERSION
