"""IVFPQ on the GPU (FAISSIndex(index_type='IVFPQ'), faiss_retrieval.py:56-63): (i) the scan is exact given the index's
own state (probes, codes, centroids, codebooks) against the float64 oracle (tests/ivfpq_oracle.py), (ii) the encoder's
codes are the arg-min codewords up to near-ties, (iii) training is bit-reproducible and its coarse level is the IVF
index's, (iv) recall against Flat matches the oracle's, (v) the drop-in API and the pipeline."""
import numpy as np
import pytest
import torch

import oracle
from amdrec import synth
from tests import ivfpq_oracle

pytestmark = pytest.mark.gpu

# fp32 tables (|(q - c)_s - C_s[j]|^2, an fma chain over dsub <= 64 terms) summed over m <= 32 sub-spaces against the
# float64 oracle: values are O(1), the error a few ulp per term
DIST_ATOL = 2e-5
DIST_TAU = 4e-5           # near-tie class at the k-th distance (ids there may differ)
CODE_TIE_ATOL = 1e-5      # an encoder mismatch is allowed only between codewords this close


def _clustered(n, d, n_clusters, seed, spread=0.35):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_clusters, d)).astype(np.float32)
    x = c[rng.integers(0, n_clusters, n)] + spread * rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _normalized_on_device(idx, x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return idx._normalize_(t)


def _state(idx):
    pq = idx._pq
    return (pq.codes.cpu().numpy(), pq.assign.cpu().numpy(), pq.centroids.cpu().numpy(),
            pq.codebooks.cpu().numpy())


def _check_against_oracle(idx, xq, k, nprobe):
    """-> (positions, distances) of the index's search and the oracle's (distances, positions) given its state."""
    qn = _normalized_on_device(idx, xq)
    pos, D = idx.search_device(qn, k, normalize=False, return_positions=True)
    ids, D = pos.cpu().numpy(), D.cpu().numpy()
    probes = idx._pq.coarse_probes(qn, nprobe).cpu().numpy()
    codes, assign, cent, cb = _state(idx)
    rD, rI = ivfpq_oracle.adc_search(codes, assign, cent, cb, qn.cpu().numpy(), k, nprobe, probes=probes)
    fin = np.isfinite(rD)
    assert np.array_equal(fin, np.isfinite(D))
    assert np.abs(D[fin] - rD[fin]).max() <= DIST_ATOL
    oracle.search.check_topk(-rD, rI, -D, ids, tau=DIST_TAU, score_tol=DIST_ATOL)
    assert (np.diff(D, axis=1)[fin[:, 1:]] >= 0).all()          # ascending
    return ids, D, rD, rI


@pytest.mark.parametrize("n,d,m,nlist,nprobe,k,nq", [
    (20_000, 256, 8, 100, 10, 100, 1),       # one request at the reference defaults
    (20_000, 256, 8, 100, 10, 500, 5),
    (20_000, 256, 16, 100, 10, 300, 64),
    (30_000, 256, 32, 37, 5, 200, 300),
    (20_000, 64, 8, 50, 8, 500, 64),
    (20_000, 64, 16, 50, 8, 100, 5),
    (12_000, 128, 4, 20, 4, 50, 33),
    (20_000, 256, 4, 100, 10, 200, 64),      # dsub 64: the encoder stages a sub-space in two steps
    # long lists split over several workgroups: ~10 000 and ~6 000 rows per list
    (40_000, 256, 8, 4, 2, 500, 64),
    (12_000, 128, 32, 2, 1, 500, 5),
])
def test_ivfpq_scan_is_exact_given_the_index_state(n, d, m, nlist, nprobe, k, nq):
    from amdrec.index import FAISSIndex
    xb = _clustered(n, d, 40, 1)
    xq = _clustered(nq, d, 40, 2)
    idx = FAISSIndex(d, index_type="IVFPQ", nlist=nlist, nprobe=nprobe, pq_m=m)
    idx.add(xb)
    assert idx.index.is_trained and idx.index.ntotal == n and idx._xb.numel() == 0
    if nlist <= 4:
        lens = np.bincount(idx._pq.assign.cpu().numpy(), minlength=nlist)
        assert lens.max() >= 5_000
    _check_against_oracle(idx, xq, k, nprobe)


def test_ivfpq_underfilled_slots_are_inf_and_id_map_last():
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(600, 256, 20, 3), _clustered(4, 256, 20, 4)
    idx = FAISSIndex(256, index_type="IVFPQ", nlist=30, nprobe=2)
    idx.add(xb, ad_ids=list(range(1000, 1600)))
    pos, D, rD, rI = _check_against_oracle(idx, xq, 500, 2)
    assert np.isinf(D[:, -1]).all() and (pos[:, -1] == -1).all()   # two lists of ~20 rows cannot fill 500 slots
    ids, D2 = idx.search(xq, 500)
    assert np.array_equal(D2.view(np.uint32), D.view(np.uint32))
    fin = np.isfinite(D)
    assert (ids[~fin] == 1599).all()                             # id_map[-1], as the reference's list indexing
    assert ((ids[fin] >= 1000) & (ids[fin] < 1600)).all()


@pytest.mark.parametrize("d,m", [(256, 8), (128, 32), (256, 16), (256, 4)])
def test_ivfpq_encoder_matches_argmin_codes(d, m):
    from amdrec.index import FAISSIndex
    xb = _clustered(20_000, d, 40, 5)
    idx = FAISSIndex(d, index_type="IVFPQ", nlist=64, pq_m=m)
    idx.add(xb)
    xn = _normalized_on_device(idx, xb).cpu().numpy()
    codes, assign, cent, cb = _state(idx)
    ref = ivfpq_oracle.encode(xn, assign, cent, cb)
    same = codes == ref
    assert same.mean() >= 0.999, same.mean()
    rows, subs = np.nonzero(~same)
    for s in np.unique(subs):
        r = rows[subs == s]
        dg = ivfpq_oracle.code_distances(xn, assign, cent, cb, r, s, codes[r, s].astype(np.int64))
        dr = ivfpq_oracle.code_distances(xn, assign, cent, cb, r, s, ref[r, s].astype(np.int64))
        assert (np.abs(dg - dr) <= CODE_TIE_ATOL).all(), (s, float(np.abs(dg - dr).max()))


def test_ivfpq_training_is_bit_reproducible_and_shares_the_ivf_quantizer():
    from amdrec.index import FAISSIndex
    xb = _clustered(20_000, 256, 40, 6)
    a = FAISSIndex(256, index_type="IVFPQ", nlist=100)
    a.add(xb)
    b = FAISSIndex(256, index_type="IVFPQ", nlist=100)
    b.add(xb)
    assert torch.equal(a._pq.codebooks, b._pq.codebooks)
    assert torch.equal(a._pq.codes, b._pq.codes)
    ivf = FAISSIndex(256, index_type="IVF", nlist=100)
    ivf.add(xb)
    assert torch.equal(a._pq.centroids, ivf._ivf.centroids)
    assert torch.equal(a._pq.assign, ivf._ivf.assign)
    assert a._pq.codebooks.shape == (8, 256, 32) and torch.isfinite(a._pq.codebooks).all()


@pytest.mark.parametrize("d,m", [(64, 8), (256, 4)])
def test_ivfpq_train_step_computes_the_lloyd_means(d, m):
    """One amdrec_ivfpq_train_step from codewords that are sample residuals (not a fixed point): every used codeword becomes
    the float64 mean of the residuals the step's own assignment (amdrec_ivfpq_encode with the same codewords) gives it, an
    unused one keeps its value."""
    import ctypes as C
    from amdrec import _lib
    from amdrec.index import FAISSIndex
    n, nlist = 6_000, 16
    xb = _clustered(n, d, 10, 12)
    idx = FAISSIndex(d, index_type="IVFPQ", nlist=nlist, pq_m=m)
    idx.add(xb)
    pq = idx._pq
    x = _normalized_on_device(idx, xb)
    a, cent = pq.assign, pq.centroids
    res = x - cent[a]
    cb0 = res[torch.arange(0, 256 * 7, 7, device=x.device)].view(256, m, d // m).permute(1, 0, 2).contiguous()
    lib, st = _lib.load(), _lib.stream_ptr(x.device)
    codes = torch.empty((n, m), dtype=torch.uint8, device=x.device)
    _lib.check(lib.amdrec_ivfpq_encode(_lib.ptr(x), n, x.stride(0), d, _lib.ptr(a), _lib.ptr(cent), cent.stride(0), nlist,
                                       _lib.ptr(cb0), m, _lib.ptr(codes), _lib.stream_ptr(x.device)))
    cb = cb0.clone()
    nb = C.c_size_t(0)
    _lib.check(lib.amdrec_ivfpq_train_workspace(n, d, m, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=x.device)
    _lib.check(lib.amdrec_ivfpq_train_step(_lib.ptr(x), n, x.stride(0), d, _lib.ptr(a), _lib.ptr(cent), cent.stride(0), nlist,
                                           _lib.ptr(cb), m, _lib.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    r = x.cpu().numpy().astype(np.float64) - cent.cpu().numpy().astype(np.float64)[a.cpu().numpy()]
    cn, ref = codes.cpu().numpy(), cb0.cpu().numpy().astype(np.float64)
    dsub = d // m
    for s in range(m):
        for j in np.unique(cn[:, s]):
            ref[s, j] = r[cn[:, s] == j, s * dsub:(s + 1) * dsub].mean(0)
    got = cb.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-6, float(np.abs(got - ref).max())
    unused = [(s, j) for s in range(m) for j in range(256) if not (cn[:, s] == j).any()]
    for s, j in unused:
        assert np.array_equal(got[s, j], cb0.cpu().numpy()[s, j])
    assert not np.array_equal(got, cb0.cpu().numpy())


def test_ivfpq_recall_against_flat_matches_the_oracle():
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(20_000, 256, 40, 7), _clustered(32, 256, 40, 8)
    k = 100
    flat = FAISSIndex(256, index_type="Flat")
    flat.add(xb)
    fids, _ = flat.search(xq, k)
    idx = FAISSIndex(256, index_type="IVFPQ", nlist=100, nprobe=10)
    idx.add(xb)
    codes, assign, cent, cb = _state(idx)
    qn = _normalized_on_device(idx, xq)
    for nprobe in (10, 100):
        idx.index.nprobe = nprobe
        ids, _ = idx.search(xq, k)
        probes = idx._pq.coarse_probes(qn, nprobe).cpu().numpy()
        _, rI = ivfpq_oracle.adc_search(codes, assign, cent, cb, qn.cpu().numpy(), k, nprobe, probes=probes)
        rec = np.mean([len(set(a) & set(b)) / k for a, b in zip(ids, fids)])
        rrec = np.mean([len(set(a) & set(b)) / k for a, b in zip(rI, fids)])
        assert abs(rec - rrec) <= 0.02 and rec >= 0.2, (nprobe, rec, rrec)
        print(f"IVFPQ recall@{k} vs Flat at nprobe {nprobe}: GPU {rec:.3f}, oracle {rrec:.3f}")
    # nprobe = nlist: the oracle's exhaustive ADC search (its own coarse order does not matter: every list is probed)
    ids, D = idx.search(xq, k)
    rD, rI = ivfpq_oracle.adc_search(codes, assign, cent, cb, qn.cpu().numpy(), k, 100)
    oracle.search.check_topk(-rD, rI, -D, ids, tau=DIST_TAU, score_tol=DIST_ATOL)


def test_ivfpq_reference_api(tmp_path):
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(3_000, 256, 20, 9), _clustered(6, 256, 20, 10)
    idx = FAISSIndex(256, index_type="IVFPQ")                     # the reference's call: nlist 100, nprobe 10, m 8
    assert idx.pq_m == 8 and not idx.index.is_trained
    idx.add(xb[:2000])                                            # trains on the first add
    assert idx.index.is_trained and idx.index.ntotal == 2000
    idx.add(xb[2000:], ad_ids=list(range(10_000, 11_000)))        # second add: custom int ids, no re-training
    assert idx.index.ntotal == 3000 and idx._xb.numel() == 0
    assert idx.index.nprobe == 10
    idx.index.nprobe = 20
    assert idx.nprobe == 20 and idx.index.nprobe == 20
    ids, D = idx.search(xq, 50)
    assert ids.shape == (6, 50) and D.shape == (6, 50) and (np.diff(D, axis=1) >= 0).all()
    bids, bD = idx.batch_search(xq, k=50, batch_size=4)
    assert np.array_equal(bids, ids) and np.array_equal(bD, D)
    st = idx.get_stats()
    assert st == {"index_type": "IVFPQ", "dimension": 256, "num_vectors": 3000, "is_trained": True, "nlist": 100,
                  "nprobe": 20}
    # save / load: identical ids and distance bits; the file holds codes, not an fp32 corpus
    p = tmp_path / "pq.bin"
    idx.save(str(p))
    n, m = 3000, 8
    assert p.stat().st_size < n * (m + 24) + 2 * 1024 * 1024
    idx2 = FAISSIndex(256, index_type="IVF")
    idx2.load(str(p))
    assert idx2.index_type == "IVFPQ" and idx2.pq_m == 8 and idx2.index.ntotal == 3000 and idx2.nprobe == 20
    ids2, D2 = idx2.search(xq, 50)
    assert np.array_equal(ids2, ids) and np.array_equal(D2.view(np.uint32), D.view(np.uint32))
    # str ids
    s = FAISSIndex(256, index_type="IVFPQ", nlist=16, nprobe=4)
    s.add(xb[:1000], ad_ids=[f"ad_{i}" for i in range(1000)])
    sids, _ = s.search(xq, 10)
    assert all(isinstance(v, str) and v.startswith("ad_") for v in sids.ravel())


def test_ivfpq_rejected_add_leaves_the_index_unchanged():
    """An add whose ad_ids do not match the rows raises and commits nothing: the codes, the assignment, ntotal and every
    later search are those of the index before it; a retry with the right ids then works."""
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(3_000, 256, 20, 13), _clustered(5, 256, 20, 14)
    idx = FAISSIndex(256, index_type="IVFPQ", nlist=32, nprobe=8)
    idx.add(xb[:2000], ad_ids=list(range(5000, 7000)))
    ids0, D0 = idx.search(xq, 100)
    with pytest.raises(ValueError):
        idx.add(xb[2000:], ad_ids=list(range(10)))
    assert idx.index.ntotal == 2000 and idx._pq.ntotal == 2000 and idx._pq.assign.numel() == 2000
    ids1, D1 = idx.search(xq, 100)
    assert np.array_equal(ids1, ids0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32))
    idx.add(xb[2000:], ad_ids=list(range(7000, 8000)))
    assert idx.index.ntotal == 3000 and idx._pq.ntotal == 3000
    ids2, _ = idx.search(xq, 100)
    assert ((ids2 >= 5000) & (ids2 < 8000)).all()


def test_ivfpq_refusals():
    from amdrec.index import FAISSIndex
    with pytest.raises(ValueError):
        FAISSIndex(256, index_type="IVFPQ", pq_m=12)
    with pytest.raises(ValueError):
        FAISSIndex(96, index_type="IVFPQ", pq_m=16)              # dsub = 6
    with pytest.raises(NotImplementedError):
        FAISSIndex(256, index_type="HNSW")
    with pytest.raises(ValueError):
        FAISSIndex(256, index_type="IVFPQ", nlist=65535)          # beyond the grouped scan's grid: refused up front
    idx = FAISSIndex(256, index_type="IVFPQ", nlist=16)
    with pytest.raises(ValueError):
        idx.add(_clustered(200, 256, 5, 11))                      # < 256 training rows
    with pytest.raises(ValueError):
        idx.set_trained_centroids(np.zeros((16, 256), np.float32))   # IVF only


def _setup_pq(n_ads=20_000):
    from tests.test_pipeline_gpu import _setup
    return _setup(n_ads, 1.0 / 16, index_type="IVFPQ")


def test_ivfpq_pipeline_captures_in_a_hip_graph_and_refuses_sharding():
    from amdrec.sharded import ShardedRecommender
    from tests.test_ivf_gpu import assert_replay_survives_a_larger_eager_search
    rec, _, (user, ad, nnum) = _setup_pq()
    assert rec.faiss_index.index_type == "IVFPQ"
    for B in (4, 32):
        uc, un = synth.user_batch(user, nnum, B, seed=70 + B)
        uc, un = torch.from_numpy(uc).cuda(), torch.from_numpy(un).cuda()
        eager = rec.recommend_device(uc, un, 10, 200)
        ids, sc = eager["ad_ids"].clone(), eager["scores"].clone()
        cids, cd = eager["candidate_ids"].clone(), eager["candidate_scores"].clone()
        assert (cd[:, 1:] >= cd[:, :-1]).all()                   # candidate_scores are L2 distances, ascending
        g = rec.capture(B, 10, 200)
        out = g(uc, un)
        torch.cuda.synchronize()
        assert torch.equal(out["ad_ids"], ids) and torch.equal(out["scores"], sc)
        assert torch.equal(out["candidate_ids"], cids) and torch.equal(out["candidate_scores"], cd)
        assert_replay_survives_a_larger_eager_search(rec, g, uc, un, user, nnum)
    with pytest.raises(NotImplementedError):
        ShardedRecommender(rec, rank=0, world=1, shard_offset=0)


def test_ivfpq_model_dir_roundtrip(tmp_path):
    from amdrec import prep
    from amdrec.pipeline import AD_COLS, USER_COLS, AdRecommenderInference, build_faiss_index
    from amdrec.towers import TwoTowerModel
    numerical, categorical, _ = prep.synthetic_criteo(6000)
    pp, _, cat_enc = prep.fit_preprocessor(numerical, categorical)
    user_dims = {c: pp.feature_dims[c] for c in USER_COLS}
    ad_dims = {c: pp.feature_dims[c] for c in AD_COLS}
    ad_table = cat_enc[:4000, 6:]
    tt_sd = synth.two_tower_state(user_dims, ad_dims, 13, seed=61)
    rk_sd = synth.ranker_state(user_dims, ad_dims, 13, seed=62, cross_scale=1.0 / 16)
    t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}   # noqa: E731
    d = tmp_path / "models"
    d.mkdir()
    pp.save(d / "preprocessor.json")
    torch.save(t(tt_sd), d / "two_tower_final.pt")
    torch.save(t(rk_sd), d / "transformer_ranker_final.pt")
    np.save(d / "ad_features.npy", ad_table)
    tt = TwoTowerModel(user_dims, ad_dims, 13)
    tt.load_state_dict(t(tt_sd))
    built = build_faiss_index(tt, ad_table, save_path=str(d / "faiss_index.bin"), index_type="IVFPQ")
    rec = AdRecommenderInference(str(d))
    assert rec.faiss_index.index_type == "IVFPQ" and rec.faiss_index.index.ntotal == 4000
    assert torch.equal(rec.faiss_index._pq.codes, built._pq.codes)
    rng = np.random.default_rng(8)
    users = [{"categorical": {f"C{i}": f"cat_{rng.integers(0, 50)}" for i in range(1, 7)},
              "numerical": {f"I{i}": float(rng.random() * 100) for i in range(1, 14)}} for _ in range(5)]
    out = rec.batch_recommend(users, top_k=10, stage1_k=200)
    assert len(out) == 5 and all(len(r["ad_ids"]) == 10 for r in out)
    assert all(0 <= i < 4000 for r in out for i in r["ad_ids"])


def test_benchmark_faiss_index_ivfpq_arm():
    from amdrec.index import benchmark_faiss_index
    r = benchmark_faiss_index(num_vectors=20_000, num_queries=8, k=50, index_types=("IVFPQ",))
    assert list(r) == ["IVFPQ"] and set(r["IVFPQ"]) == {"add_time", "search_time_ms", "per_query_ms"}
