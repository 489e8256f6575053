"""CPU: the host side of the stage-1 score boosts (amdrec.boost) - the numpy statement of the rule against plain loops,
host validation, the refusals (before the library is touched), the two C entries' argument checks (every call returns
before its first HIP call), the near-tie cap of the fp32-engine GPU inputs, and the storage life cycle that needs no launch."""
import ctypes

import numpy as np
import pytest
import torch

from amdrec import _lib, boost as bo
from tests import boost_oracle as bx, cases, flat_oracle

FP32_DIM, GPU_KS = 100, (10, 100)


def test_rule_matches_the_loops():
    rng = np.random.default_rng(3)
    nq, n, k = 9, 60, 7
    ip = rng.standard_normal((nq, n)).astype(np.float32)
    ip[2, 5] = ip[2, 6]                                    # a tie in ip
    ip[3, 10] = np.nan                                     # never returned, whatever its boost
    boost = (rng.standard_normal(n) * 0.3).astype(np.float32)
    boost[10], boost[0], boost[n - 1] = 100.0, 3.0, -3.0
    w = bx.weights_for(nq)
    D, I = bx.topk(ip, boost, w, k)
    Dl, Il = bx.topk_loops(ip, boost, w, k)
    assert I.tolist() == Il and D.tolist() == [[float(v) for v in row] for row in Dl]
    pos, sc = bo.boost_oracle(ip, boost, w, k)
    assert np.array_equal(pos, I) and np.array_equal(sc, D)
    s = bo.boosted_scores(ip, boost, w)
    assert s.dtype == np.float32
    for q in range(nq):
        for r in range(n):
            v = bx.score(ip[q, r], w[q], boost[r])
            assert (np.isnan(v) and np.isnan(s[q, r])) or v == s[q, r]
    assert 10 not in I[3].tolist()
    # w == 0: the plain order
    plain = [sorted((r for r in range(n) if ip[0][r] == ip[0][r]), key=lambda r: (-float(ip[0][r]), r))[:k]]
    assert I[0].tolist() == plain[0] and w[0] == 0.0
    # k > n: the tail is unfilled
    D2, I2 = bx.topk(ip, boost, w, n + 3)
    assert (I2[:, n:] == -1).all() and np.isneginf(D2[:, n:]).all() and I2[3, n - 1] == -1
    # two roundings, not one: a case where the fused form differs
    a, b, c = np.float32(-(1.0 + 2.0 ** -11)), np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)
    fused = np.float32(np.float64(a) + np.float64(b) * np.float64(c))        # b * c = 1 + 2^-11 + 2^-24, exactly
    assert bx.score(a, b, c) == 0.0 and fused == np.float32(2.0 ** -24)


def test_as_boosts_and_weights_validate():
    b = bo.as_boosts([0.5, -0.0, 2], 3)
    assert b.dtype == np.float32 and b.tolist() == [0.5, 0.0, 2.0] and not np.signbit(b[1])
    assert bo.as_boosts(1.5, 4).tolist() == [1.5] * 4
    assert bo.as_boosts(torch.tensor([1.0, -2.0]), 2).tolist() == [1.0, -2.0]
    assert bo.as_boosts(np.arange(3), 3).tolist() == [0.0, 1.0, 2.0]
    for bad, exc in (([1.0, np.nan], ValueError), ([np.inf, 0.0], ValueError), ([1e39, 0.0], ValueError),
                     ([1.0, 2.0, 3.0], ValueError), (np.zeros((2, 1)), ValueError), (["a", "b"], TypeError),
                     (True, TypeError), (np.array([True, False]), TypeError)):
        with pytest.raises(exc):
            bo.as_boosts(bad, 2)
    assert bo.check_weight(2) == 2.0 and bo.check_weight(np.float32(0.5)) == 0.5
    for bad, exc in ((float("nan"), ValueError), (float("inf"), ValueError), (1e39, ValueError), (True, TypeError),
                     ("1", TypeError), (None, TypeError)):
        with pytest.raises(exc):
            bo.check_weight(bad)
    assert bo.as_weights(0.5, 3).tolist() == [0.5] * 3 and bo.as_weights([1, 2], 2).dtype == np.float32
    assert bo.as_weights(np.array([1.0, 4.0]), 2).tolist() == [1.0, 4.0]
    with pytest.raises(ValueError):
        bo.as_weights([1.0, 2.0, 3.0], 2)
    with pytest.raises(ValueError):
        bo.as_weights([1.0, float("nan")], 2)
    with pytest.raises(TypeError):
        bo.device_weights(torch.zeros(2), 2, "cpu")                  # a tensor must be a device float32 tensor
    with pytest.raises(ValueError):
        bo.device_weights(float("inf"), 2, "cpu")


def _bare(index_type="Flat", boosts=None):
    """An index object that was never constructed: the refusals depend on neither a device nor the library."""
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type = index_type
    if boosts is not None:
        idx._boosts, idx._boost_max = boosts, 1.0
    return idx


@pytest.mark.parametrize("index_type", ["IVF", "IVFPQ"])
def test_ivf_indexes_refuse_a_boost_before_the_library_is_touched(index_type, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    idx = _bare(index_type)
    q = np.zeros((2, 8), dtype=np.float32)
    for call in (lambda: idx.search_device(q, 3, boost_weight=1.0), lambda: idx.search(q, 3, boost_weight=[1.0, 2.0]),
                 lambda: idx.batch_search(q, 3, boost_weight=0.5), lambda: idx.add(q, boosts=[1.0, 2.0]),
                 lambda: idx.search_device(q, 3, boost_weight=torch.zeros(2))):
        with pytest.raises(NotImplementedError, match="follow-up"):
            call()


def test_flat_refusals_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    q = np.zeros((2, 8), dtype=np.float32)
    bare = _bare()
    for call in (lambda: bare.search_device(q, 3, boost_weight=1.0), lambda: bare.search(q, 3, boost_weight=1.0),
                 lambda: bare.batch_search(q, 3, boost_weight=[1.0, 1.0])):
        with pytest.raises(ValueError, match="without boosts"):
            call()
    idx = _bare(boosts=torch.zeros(4))
    zero = torch.zeros(2, dtype=torch.int64)
    for call in (lambda: idx.search_device(q, 3, boost_weight=1.0, require_all=zero),
                 lambda: idx.search(q, 3, boost_weight=1.0, require_any=[0, 0]),
                 lambda: idx.batch_search(q, 3, boost_weight=1.0, require_all=0)):
        with pytest.raises(NotImplementedError, match="follow-up"):
            call()
    for w in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            idx.search_device(q, 3, boost_weight=w)
        with pytest.raises(ValueError, match="finite"):
            idx.search(q, 3, boost_weight=[1.0, w])
    with pytest.raises(ValueError, match="boost weights for 2 queries"):
        idx.search(q, 3, boost_weight=[1.0, 2.0, 3.0])
    with pytest.raises(TypeError):
        idx.search_device(q, 3, boost_weight=True)
    assert idx._check_boost(None) is False


def test_pipeline_refusals_before_the_library_is_touched(monkeypatch):
    from amdrec.pipeline import AdRecommenderInference, TwoStageRetriever
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    rec = object.__new__(AdRecommenderInference)
    rec.heads_mode = "all"
    for index, exc, match in ((_bare("IVF"), NotImplementedError, "follow-up"), (_bare(), ValueError, "without boosts")):
        rec.faiss_index = index
        z = torch.zeros((2, 3))
        for call in (lambda: rec.recommend_device(z, z, stage1_boost=1.0), lambda: rec.batch_recommend([{}], stage1_boost=1.0),
                     lambda: rec.recommend_ads({}, stage1_boost=1.0), lambda: rec.recommend_tensors(z, z, stage1_boost=1.0)):
            with pytest.raises(exc, match=match):
                call()
        two = object.__new__(TwoStageRetriever)
        two.faiss_index = index
        with pytest.raises(exc, match=match):
            two.retrieve_and_rank(z, z, stage1_boost=1.0)
    rec.faiss_index = _bare(boosts=torch.zeros(4))
    with pytest.raises(NotImplementedError, match="follow-up"):
        rec.recommend_device(z, z, stage1_boost=1.0, require_all=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="finite"):
        rec.recommend_device(z, z, stage1_boost=float("nan"))


def _fake_pointer():
    raw = ctypes.create_string_buffer(4096 + 256)
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256            # non-null, aligned, never dereferenced


def test_boosted_entries_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    raw, p = _fake_pointer()

    def fp32(k=5, nq=1, boost=p, weight=p, bmax=1.0, dim=256):
        return lib.amdrec_flat_search_boosted(p, 10, 256, dim, p, nq, 256, k, 0, p, p, None, 0, None, None, boost, weight, bmax)

    def mixed(k=5, nq=1, boost=p, weight=p, bmax=1.0, dim=256):
        return lib.amdrec_flat_search_mixed_boosted(p, 10, 256, dim, p, 256, p, p, nq, 256, k, 0, p, p, None, 0, None, None,
                                                    boost, weight, bmax)
    for call in (fp32, mixed):
        assert call(boost=None) == -1 and b"boost is null" in lib.amdrec_last_error()
        assert call(weight=None) == -1 and b"weight is null" in lib.amdrec_last_error()
        assert call(boost=p + 4) == -1 and b"64-byte aligned" in lib.amdrec_last_error()
        assert call(weight=p + 2) == -1 and b"4-byte aligned" in lib.amdrec_last_error()
        for bad in (-1.0, float("inf"), float("nan")):
            assert call(bmax=bad) == -1 and b"boost_max" in lib.amdrec_last_error()
        assert call(k=0) == -1 and b"k=0" in lib.amdrec_last_error()
        assert call(k=_lib.MAX_K + 1) == -1 and b"k=" in lib.amdrec_last_error()
        assert call(dim=250) == -1 and b"multiple of" in lib.amdrec_last_error()
        assert call(nq=0, boost=None, weight=None) == 0                  # nq = 0: nothing to do
        # every argument good: the next refusal is the (missing) workspace, still before the first HIP call
        assert call() != 0 and b"workspace" in lib.amdrec_last_error()
    del raw


@pytest.mark.parametrize("pattern", ["noise", "sparse_half"])
def test_near_tie_cap_of_the_fp32_gpu_inputs(pattern):
    """The fp32-engine GPU test holds the search to the float64 oracle with oracle.search.check_topk; at most 2 % of its 513
    queries (tests/test_eligible_cpu.py's cap) may have their (k + 1)-th boosted score inside cases.TOPK_TAU of the k-th
    without equalling it."""
    xb, xq = flat_oracle.case_inputs(dict(n=bx.N, dim=FP32_DIM, nq=bx.NQ, kind="lifted", seed=1))
    xb = xb / np.linalg.norm(xb, axis=1, keepdims=True)
    xq = xq / np.linalg.norm(xq, axis=1, keepdims=True)
    boost, w = getattr(bx, pattern)(), bx.weights_for(bx.NQ)
    for k in GPU_KS:
        D, _ = bx.expected64(xb.astype(np.float32), xq.astype(np.float32), boost, w, k + 1)
        gap = D[:, k - 1].astype(np.float64) - D[:, k].astype(np.float64)
        loose = int(((gap <= cases.TOPK_TAU) & (gap > 0)).sum())
        print(f"{pattern} k {k}: {loose} of {bx.NQ} queries inside the near-tie band")
        assert loose <= 0.02 * bx.NQ


# ---- storage life cycle that needs no launch ------------------------------------------------------------------------------------
def _cpu_index(n):
    """A Flat fp32 index on "cpu" allocates and saves without a kernel: rows are put in place by hand."""
    from amdrec.index import FAISSIndex
    idx = FAISSIndex(8, index_type="Flat", device="cpu", prefilter="fp32")
    idx._reserve(n)
    idx._xb[:n] = torch.eye(8)[:n]
    idx._ids[:n] = torch.arange(n)
    idx._n = n
    return idx


def _header(path):
    import json
    import struct
    with open(path, "rb") as f:
        f.read(9)
        (hl,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(hl).decode())


def test_boosts_in_the_index_file_through_growth_and_a_plain_file_loads_as_ever(tmp_path):
    from amdrec.index import FAISSIndex
    boosts = [0.0, -0.5, 3.0, 1.0, -2.25]
    idx = _cpu_index(5)
    assert idx._boosts is None and idx._boost_max == 0.0 and idx.get_boosts().tolist() == [0.0] * 5
    assert len(idx.resident_tensors()) == 4
    idx.set_boosts(boosts)
    assert idx.get_boosts().tolist() == boosts and idx._boosts.dtype == torch.float32 and idx._boost_max == 3.0
    assert any(t is idx._boosts for t in idx.resident_tensors()) and len(idx.resident_tensors()) == 5
    old, snapshot = idx._boosts, idx._boosts.clone()
    idx.set_boosts([-0.0] * 5)                                              # out of place; -0.0 is stored as +0.0
    assert idx._boosts is not old and torch.equal(old, snapshot) and not torch.signbit(idx._boosts[:5]).any()
    assert idx._boost_max == 0.0
    idx.set_boosts(np.array(boosts[:4] + [-0.0]))
    assert not torch.signbit(idx._boosts[4]) and idx._boost_max == 3.0
    idx.set_boosts(boosts)
    path = str(tmp_path / "with_boosts.bin")
    idx.save(path)
    assert [a["name"] for a in _header(path)["arrays"]] == ["xb", "ids", "boosts"]
    back = FAISSIndex(8, index_type="Flat", device="cpu", prefilter="fp32")
    back.load(path)
    assert back.get_boosts().tolist() == boosts and back._boosts.dtype == torch.float32 and back.index.ntotal == 5
    assert back._boost_max == 3.0                                           # restored from the array itself
    idx.set_bids([1.0, 2.0, 3.0, 4.0, 5.0])
    idx.set_groups([3, -1, 3, 7, 9])
    idx.save(path)
    assert [a["name"] for a in _header(path)["arrays"]] == ["xb", "ids", "groups", "bids", "boosts"]   # behind what was written before
    back.load(path)
    assert back.get_boosts().tolist() == boosts and back.get_bids().tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    idx._reserve(5000)                                                      # growth keeps the boosts
    assert idx.get_boosts().tolist() == boosts and idx._boosts.shape[0] >= 5000      # (add() zeroes the rows it appends)
    plain = str(tmp_path / "plain.bin")
    _cpu_index(5).save(plain)
    assert [a["name"] for a in _header(plain)["arrays"]] == ["xb", "ids"]   # the file every earlier build wrote
    back = FAISSIndex(8, index_type="Flat", device="cpu", prefilter="fp32")
    back.load(plain)
    assert back._boosts is None and back._boost_max == 0.0 and back.get_boosts().tolist() == [0.0] * 5


@pytest.mark.parametrize("bad, exc", [([1.0, 2.0], ValueError), ([1.0] * 6, ValueError), ([1.0, 2.0, float("nan"), 0.0, 0.0], ValueError),
                                      ([float("inf")] + [0.0] * 4, ValueError), ([1e39] + [0.0] * 4, ValueError),
                                      (["a"] * 5, TypeError), (np.zeros((5, 1)), ValueError)])
def test_bad_boosts_are_refused_and_leave_the_index_as_it_was(bad, exc):
    idx = _cpu_index(5)
    with pytest.raises(exc):
        idx.set_boosts(bad)
    assert idx._boosts is None and idx._boost_max == 0.0 and len(idx.resident_tensors()) == 4
    idx.set_boosts([1.0, -2.0, 3.0, 4.0, 5.0])
    kept = idx._boosts
    with pytest.raises(exc):
        idx.set_boosts(bad)
    assert idx._boosts is kept and idx.get_boosts().tolist() == [1.0, -2.0, 3.0, 4.0, 5.0] and idx._boost_max == 5.0
    # a weight on an index that holds boosts is still validated before anything else happens
    with pytest.raises(ValueError, match="finite"):
        idx._check_boost(float("nan"))
    with pytest.raises(NotImplementedError, match="follow-up"):
        idx._check_boost(1.0, masked=True)
    assert idx._check_boost(1.0) is True and idx._check_boost(torch.zeros(2)) is True
