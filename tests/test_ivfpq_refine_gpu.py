"""IVFPQ refine on the GPU (FAISSIndex(index_type='IVFPQ', refine='fp32' | 'bf16')): the result is the float64 oracle's
re-rank (tests/ivfpq_refine_oracle.py) of the plain index's own k' candidates, distances within the derived fp32 bound;
recall against the exact neighbours follows the oracle's; bit-determinism across batches; the IVFPQ contracts carry over
(non-finite rows, unfilled slots, ids, incremental and rejected adds, save / load, the captured pipeline)."""
import numpy as np
import pytest
import torch

from amdrec import synth
from tests import ivfpq_oracle
from tests import ivfpq_refine_oracle as ro
from tests.test_ivfpq_gpu import _clustered, _normalized_on_device, _state

pytestmark = pytest.mark.gpu

EXCUSED_CAP = 0.01            # share of slots that may differ from the oracle as near-tie swaps


def _pair(xb, d=256, kind="fp32", factor=4, nlist=100, nprobe=10, m=8, **kw):
    """A refined index and a plain IVFPQ index on the same rows; training is bit-reproducible, so their states are equal."""
    from amdrec.index import FAISSIndex
    ref = FAISSIndex(d, index_type="IVFPQ", nlist=nlist, nprobe=nprobe, pq_m=m, refine=kind, refine_factor=factor)
    plain = FAISSIndex(d, index_type="IVFPQ", nlist=nlist, nprobe=nprobe, pq_m=m)
    ref.add(xb, **kw)
    plain.add(xb, **kw)
    for a, b in zip(_state(ref), _state(plain)):              # codes, assignment, centroids, codebooks
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return ref, plain


def _kept_rows(idx):
    """The rows the index re-ranks against, as fp32 numpy (bf16 widened), and its finite flags."""
    return idx._pq.rows.float().cpu().numpy(), idx._pq.finite.cpu().numpy()


def _check(ref, plain, xq, k, accuracy=None, engine=None):
    """The refined search of xq against the oracle's re-rank of the plain index's search(k') positions.
    -> (excused, slots, err / bound, positions, distances)."""
    from amdrec import ivfpq
    kc = ivfpq.refine_candidates(k, ref.refine_factor)
    qn = _normalized_on_device(ref, xq)
    cand, _ = plain.search_device(qn, kc, normalize=False, return_positions=True)
    pos, D = ref.search_device(qn, k, normalize=False, return_positions=True)
    rows, finite = _kept_rows(ref)
    ex, total, worst = ro.check_rerank(rows, finite, qn.cpu().numpy(), cand.cpu().numpy(), k, pos.cpu().numpy(),
                                       D.cpu().numpy(), ref.dimension)
    if accuracy is not None:
        accuracy("ivfpq_refine", engine, worst, excused_share=ex / total)
    return ex, total, worst, pos.cpu().numpy(), D.cpu().numpy()


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_refine_is_the_oracle_rerank_of_the_plain_candidates(kind, accuracy, monkeypatch):
    """|d_gpu - d_64| <= (dim + 3) 2^-24 d_64 + 2^-126 (ivfpq_refine_oracle.dist_bound), positions equal up to near-tie swaps
    of rank neighbours / at the k-th boundary, at most 1 % of the slots.  refine='bf16': the oracle is given the bf16-rounded
    rows (round to nearest even, computed in numpy from the fp32 rows): the rounding is in the data, not in the arithmetic.
    Corpus / query seeds 21 / 22 (their check with the bound-perturbed oracle: tests/test_ivfpq_refine_cpu.py).  Then the
    paths those cases do not take: k' = 800 (the two-keys-per-lane run sort) against the oracle; one workgroup per query
    (no scratch given to the library) at k' = 400, 800 and 2000, against the oracle and bit for bit against the split
    launch; and 600 queries in one call (never split) bit for bit against the same queries in two calls."""
    d = 256
    xb, xq = _clustered(20_000, d, 40, 21), _clustered(512, d, 40, 22)
    ref, plain = _pair(xb, kind=kind)
    rows, _ = _kept_rows(ref)
    xn = _normalized_on_device(ref, xb).cpu().numpy()
    exp = xn if kind == "fp32" else ro.bf16_round(xn)
    assert np.array_equal(rows.view(np.uint32), exp.view(np.uint32))           # the kept rows are what the contract says
    assert ref._pq.rows.dtype == (torch.float32 if kind == "fp32" else torch.bfloat16) and ref._xb.numel() == 0
    ex_all = tot_all = 0
    worst_all = 0.0
    cases = [(k, nq) for k in (1, 10, 100, 500) for nq in (1, 7, 64, 512)] + [(200, 64)]
    for k, nq in cases:
        ex, total, worst, _, _ = _check(ref, plain, xq[:nq], k, accuracy, f"rerank_kernel {kind}")
        ex_all, tot_all, worst_all = ex_all + ex, tot_all + total, max(worst_all, worst)
        assert ex <= EXCUSED_CAP * total or ex <= 2, (k, nq, ex, total)
    from amdrec import ivfpq
    split = {k: _check(ref, plain, xq[:64], k)[3:] for k in (100, 200, 500)}
    x600 = _normalized_on_device(ref, _clustered(600, d, 40, 29))
    two = [ref.search_device(x600[s:s + 300], 500, normalize=False, return_positions=True) for s in (0, 300)]
    one = ref.search_device(x600, 500, normalize=False, return_positions=True)
    assert torch.equal(one[0], torch.cat([p for p, _ in two]))
    assert torch.equal(one[1].view(torch.int32), torch.cat([x for _, x in two]).view(torch.int32))
    monkeypatch.setattr(ivfpq, "RERANK_SPLIT_MAX_QUERIES", 0)     # no scratch, no tickets: one workgroup per query
    for k, (pos, D) in split.items():
        ex, total, worst, pos1, D1 = _check(ref, plain, xq[:64], k, accuracy, f"rerank_kernel {kind}")
        ex_all, tot_all, worst_all = ex_all + ex, tot_all + total, max(worst_all, worst)
        assert np.array_equal(pos1, pos) and np.array_equal(D1.view(np.uint32), D.view(np.uint32)), k
    monkeypatch.undo()
    print(f"refine {kind}: {ex_all} of {tot_all} slots excused as near-tie swaps ({ex_all / tot_all:.5f}), "
          f"largest err / bound {worst_all:.4f}")
    assert ex_all <= EXCUSED_CAP * tot_all


def test_refine_clamps_the_candidates_to_max_k():
    xb, xq = _clustered(20_000, 256, 40, 23), _clustered(9, 256, 40, 24)
    ref, plain = _pair(xb, factor=8)
    _check(ref, plain, xq, 500)                                 # k' = min(4000, 2048)
    ref4, _ = _pair(xb, factor=4)
    _, _, _, pos, D = _check(ref4, plain, xq, 2048)             # k' = k = 2048: the candidates themselves, re-ordered
    cand = plain.search_device(_normalized_on_device(plain, xq), 2048, normalize=False, return_positions=True)[0].cpu().numpy()
    assert all(sorted(a[a >= 0].tolist()) == sorted(b[b >= 0].tolist()) for a, b in zip(pos, cand))


def test_refine_factor_one_reranks_the_k_candidates():
    xb, xq = _clustered(20_000, 256, 40, 25), _clustered(20, 256, 40, 26)
    ref, plain = _pair(xb, factor=1)
    _, _, _, pos, _ = _check(ref, plain, xq, 100)
    cand = plain.search_device(_normalized_on_device(plain, xq), 100, normalize=False, return_positions=True)[0].cpu().numpy()
    assert all(sorted(a.tolist()) == sorted(b.tolist()) for a, b in zip(pos, cand))


def test_refined_recall_follows_the_oracle_and_never_falls_below_plain():
    """The corpus of tests/test_ivfpq_refine_cpu.py's recall test.  GPU refined recall@100 at factors 1, 2, 4, 8 is >= the
    plain GPU index's and within 0.01 (one neighbour in a hundred per query) of the float64 oracle's for the same state."""
    from amdrec.index import FAISSIndex
    n, d, k = 20_000, 256, 100
    xb, xq = _clustered(n, d, 40, 7), _clustered(32, d, 40, 8)
    plain = FAISSIndex(d, index_type="IVFPQ", nlist=100, nprobe=10)
    plain.add(xb)
    codes, assign, cent, cb = _state(plain)
    qn = _normalized_on_device(plain, xq)
    xn = _normalized_on_device(plain, xb).cpu().numpy()
    q64, x64 = qn.cpu().numpy().astype(np.float64), xn.astype(np.float64)
    truth = np.argsort((q64 * q64).sum(1)[:, None] - 2 * q64 @ x64.T + (x64 * x64).sum(1)[None, :], axis=1,
                       kind="stable")[:, :k]
    probes = plain._pq.coarse_probes(qn, 10).cpu().numpy()
    base = ro.recall(plain.search(xq, k)[0], truth)
    prev = 0.0
    for factor in (1, 2, 4, 8):
        ref = FAISSIndex(d, index_type="IVFPQ", nlist=100, nprobe=10, refine="fp32", refine_factor=factor)
        ref.add(xb)
        assert torch.equal(ref._pq.codes, plain._pq.codes)
        got = ro.recall(ref.search(xq, k)[0], truth)
        _, cand = ivfpq_oracle.adc_search(codes, assign, cent, cb, qn.cpu().numpy(), k * factor, 10, probes=probes)
        _, oids = ro.refine(xn, None, qn.cpu().numpy(), cand, k)
        want = ro.recall(oids, truth)
        print(f"recall@{k} vs exact at factor {factor}: GPU refined {got:.4f}, oracle {want:.4f}, plain GPU {base:.4f}")
        assert got >= base and abs(got - want) <= 0.01, (factor, got, want, base)
        assert got >= prev - 0.01
        prev = got


def test_refine_70001_queries_cross_the_rerank_launch_cap():
    """nq > 65 535: two amdrec_ivfpq_rerank launches of one search; equal bit for bit to searches of 10 000-query slices,
    and a sample of both launches against the oracle."""
    from amdrec.index import FAISSIndex
    d, k, nq = 64, 10, 70_001
    xb = _clustered(3000, d, 20, 1)
    ref, plain = _pair(xb, d=d, nlist=16, nprobe=2)
    qn = _normalized_on_device(ref, _clustered(nq, d, 20, 4))
    pos, D = ref.search_device(qn, k, normalize=False, return_positions=True)
    parts = [ref.search_device(qn[s:s + 10_000], k, normalize=False, return_positions=True) for s in range(0, nq, 10_000)]
    assert torch.equal(pos, torch.cat([p for p, _ in parts]))
    assert torch.equal(D.view(torch.int32), torch.cat([x for _, x in parts]).view(torch.int32))
    sel = torch.from_numpy(np.unique(np.concatenate([np.arange(0, nq, 350), [65_534, 65_535, 65_536, nq - 1]]))).to(qn.device)
    cand, _ = plain.search_device(qn[sel], 4 * k, normalize=False, return_positions=True)
    rows, finite = _kept_rows(ref)
    ro.check_rerank(rows, finite, qn[sel].cpu().numpy(), cand.cpu().numpy(), k, pos[sel].cpu().numpy(), D[sel].cpu().numpy(), d)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_refine_is_bit_deterministic_across_batches(kind):
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(20_000, 256, 40, 27), _clustered(50, 256, 40, 28)
    idx = FAISSIndex(256, index_type="IVFPQ", refine=kind)
    idx.add(xb)
    ids, D = idx.search(xq, 500)
    ids2, D2 = idx.search(xq, 500)
    assert np.array_equal(ids, ids2) and np.array_equal(D.view(np.uint32), D2.view(np.uint32))
    for bs in (1, 3, 1000):
        bids, bD = idx.batch_search(xq, k=500, batch_size=bs)
        assert np.array_equal(bids, ids) and np.array_equal(bD.view(np.uint32), D.view(np.uint32)), bs


# ---- contract carry-over ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_refine_non_finite_rows_rank_last_at_inf(kind):
    from amdrec.index import FAISSIndex
    d, n, nlist = 64, 1500, 8
    xb = _clustered(n, d, 20, 15)
    clean = xb.copy()
    bad = [5, 77, 1400]
    xb[5] = np.nan
    xb[77, 3] = np.inf
    xb[1400, 60] = np.nan
    idx = FAISSIndex(d, index_type="IVFPQ", nlist=nlist, nprobe=nlist, refine=kind, refine_factor=2)
    plain = FAISSIndex(d, index_type="IVFPQ", nlist=nlist, nprobe=nlist)
    for i in (idx, plain):
        i.train(clean)
        i.add(xb)
    xq = _clustered(24, d, 20, 16)
    _, _, _, pos, D = _check(idx, plain, xq, 2048)              # every row appears: the non-finite ones last among the filled
    nf = n - len(bad)
    assert np.isfinite(D[:, :nf]).all() and np.isinf(D[:, nf:]).all() and (D[:, nf:] > 0).all()
    assert all(pos[q, nf:n].tolist() == bad for q in range(len(xq)))            # by position
    assert (pos[:, n:] == -1).all() and not np.isin(pos[:, :nf], bad).any()
    idx.index.nprobe = plain.index.nprobe = 2
    _, _, _, pos, D = _check(idx, plain, xq, 100)
    assert np.isfinite(D).all() and not np.isin(pos, bad).any()
    # a NaN query: +inf in every slot, the rest of its batch unchanged
    qn = _normalized_on_device(idx, xq)
    r_pos, r_D = idx.search_device(qn, 100, normalize=False, return_positions=True)
    qq = torch.cat([qn[:5], torch.full((1, d), float("nan"), device=qn.device), qn[5:]]).contiguous()
    p2, D2 = idx.search_device(qq, 100, normalize=False, return_positions=True)
    keep = torch.tensor([i for i in range(25) if i != 5], device=qn.device)
    assert torch.isinf(D2[5]).all() and (D2[5] > 0).all()
    assert torch.equal(p2[keep], r_pos) and torch.equal(D2[keep].view(torch.int32), r_D.view(torch.int32))


def test_refine_underfilled_slots_empty_index_and_ids():
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(600, 256, 20, 3), _clustered(4, 256, 20, 4)
    ref, plain = _pair(xb, nlist=30, nprobe=2, ad_ids=list(range(1000, 1600)))
    _, _, _, pos, D = _check(ref, plain, xq, 500)
    assert np.isinf(D[:, -1]).all() and (pos[:, -1] == -1).all()   # two lists of ~20 rows cannot fill 500 slots
    ids, D2 = ref.search(xq, 500)
    assert np.array_equal(D2.view(np.uint32), D.view(np.uint32))
    fin = np.isfinite(D)
    assert (ids[~fin] == 1599).all() and ((ids[fin] >= 1000) & (ids[fin] < 1600)).all()
    assert np.array_equal(ids[fin], pos[fin] + 1000)              # custom integer ids
    # positions with an offset
    p_off, _ = ref.search_device(_normalized_on_device(ref, xq), 500, normalize=False, return_positions=True, pos_offset=7000)
    assert np.array_equal(p_off.cpu().numpy()[fin], pos[fin] + 7000) and (p_off.cpu().numpy()[~fin] == -1).all()
    # host-side object ids
    s = FAISSIndex(256, index_type="IVFPQ", nlist=16, nprobe=4, refine="bf16")
    s.add(xb, ad_ids=[f"ad_{i}" for i in range(600)])
    sids, sD = s.search(xq, 10)
    spos, _ = s.search_device(_normalized_on_device(s, xq), 10, normalize=False, return_positions=True)
    assert [[f"ad_{p}" for p in row] for row in spos.cpu().numpy()] == sids.tolist() and np.isfinite(sD).all()
    # a trained index without rows
    e = FAISSIndex(256, index_type="IVFPQ", nlist=16, refine="fp32")
    e.train(xb)
    eids, eD = e.search(xq, 5)
    assert np.isinf(eD).all() and (eD > 0).all() and eids.shape == (4, 5)
    assert e.get_stats() == {"index_type": "IVFPQ", "dimension": 256, "num_vectors": 0, "is_trained": True, "nlist": 16,
                             "nprobe": 10}


def test_refine_incremental_and_rejected_adds():
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(3_000, 256, 20, 13), _clustered(5, 256, 20, 14)
    idx = FAISSIndex(256, index_type="IVFPQ", nlist=32, nprobe=8, refine="fp32")
    plain = FAISSIndex(256, index_type="IVFPQ", nlist=32, nprobe=8)
    idx.add(xb[:2000], ad_ids=list(range(5000, 7000)))
    plain.add(xb[:2000], ad_ids=list(range(5000, 7000)))
    ids0, D0 = idx.search(xq, 100)
    _check(idx, plain, xq, 100)
    rows0, codes0 = idx._pq.rows.clone(), idx._pq.codes.clone()
    with pytest.raises(ValueError):
        idx.add(xb[2000:], ad_ids=list(range(10)))
    pq = idx._pq
    assert idx.index.ntotal == 2000 and pq.ntotal == 2000 and pq.assign.numel() == 2000 and pq.rows.shape == (2000, 256)
    assert torch.equal(pq.rows, rows0) and torch.equal(pq.codes, codes0)
    ids1, D1 = idx.search(xq, 100)
    assert np.array_equal(ids1, ids0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32))
    idx.add(xb[2000:], ad_ids=list(range(7000, 8000)))          # an add after a search
    plain.add(xb[2000:], ad_ids=list(range(7000, 8000)))
    assert idx.index.ntotal == 3000 and idx._pq.rows.shape == (3000, 256)
    _check(idx, plain, xq, 100)
    ids2, _ = idx.search(xq, 100)
    assert ((ids2 >= 5000) & (ids2 < 8000)).all() and (ids2 >= 7000).any()


@pytest.mark.parametrize("d,m,kind", [(96, 8, "fp32"), (96, 4, "bf16"), (2048, 32, "fp32"), (2048, 4, "bf16")])
def test_refine_other_dimensions(d, m, kind):
    xb, xq = _clustered(3000, d, 20, 1), _clustered(9, d, 20, 2)
    ref, plain = _pair(xb, d=d, kind=kind, nlist=16, nprobe=4, m=m)
    for k in (50, 600):
        _check(ref, plain, xq, k)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_refine_save_load_round_trip(kind, tmp_path):
    from amdrec.index import FAISSIndex
    xb, xq = _clustered(3_000, 256, 20, 9), _clustered(6, 256, 20, 10)
    idx = FAISSIndex(256, index_type="IVFPQ", nlist=32, nprobe=8, refine=kind, refine_factor=3)
    idx.add(xb)
    ids, D = idx.search(xq, 50)
    p = tmp_path / "pqr.bin"
    idx.save(str(p))
    assert p.stat().st_size >= 3000 * 256 * (4 if kind == "fp32" else 2)
    idx2 = FAISSIndex(256, index_type="IVF")
    idx2.load(str(p))
    assert (idx2.index_type, idx2.refine, idx2.refine_factor, idx2.pq_m) == ("IVFPQ", kind, 3, 8)
    assert torch.equal(idx2._pq.rows.view(torch.uint8), idx._pq.rows.view(torch.uint8))
    ids2, D2 = idx2.search(xq, 50)
    assert np.array_equal(ids2, ids) and np.array_equal(D2.view(np.uint32), D.view(np.uint32))
    # a file saved from a plain IVFPQ index loads (also into a refined object) and searches as before
    plain = FAISSIndex(256, index_type="IVFPQ", nlist=32, nprobe=8)
    plain.add(xb)
    pids, pD = plain.search(xq, 50)
    pp = tmp_path / "pq.bin"
    plain.save(str(pp))
    import json
    import struct
    raw = pp.read_bytes()
    (hl,) = struct.unpack("<Q", raw[9:17])
    assert "refine" not in json.loads(raw[17:17 + hl].decode())            # the unrefined file format is unchanged
    idx3 = FAISSIndex(256, index_type="IVFPQ", refine=kind)
    idx3.load(str(pp))
    assert idx3.refine is None and idx3._pq.rows is None
    ids3, D3 = idx3.search(xq, 50)
    assert np.array_equal(ids3, pids) and np.array_equal(D3.view(np.uint32), pD.view(np.uint32))


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_refined_pipeline_captures_in_a_hip_graph_and_refuses_sharding(kind):
    from amdrec.index import FAISSIndex
    from amdrec.pipeline import AdRecommenderInference
    from amdrec.sharded import ShardedRecommender
    from tests.test_ivf_gpu import assert_replay_survives_a_larger_eager_search
    from tests.test_pipeline_gpu import _setup
    rec0, (_, _, _, ad_table), (user, ad, nnum) = _setup(20_000, 1.0 / 16, index_type="IVFPQ")
    tt = rec0.two_tower_model
    with torch.no_grad():
        emb = tt.get_ad_embeddings(torch.from_numpy(np.ascontiguousarray(ad_table)).cuda())
    index = FAISSIndex(tt.output_dim, index_type="IVFPQ", refine=kind)
    index.add(emb)
    assert torch.equal(index._pq.codes, rec0.faiss_index._pq.codes)
    rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rec0.transformer_ranker, faiss_index=index,
                                 ad_features=ad_table)
    assert all(isinstance(t, torch.Tensor) for t in index.resident_tensors())
    for B in (4, 32):
        uc, un = synth.user_batch(user, nnum, B, seed=70 + B)
        uc, un = torch.from_numpy(uc).cuda(), torch.from_numpy(un).cuda()
        eager = rec.recommend_device(uc, un, 10, 200)
        ids, sc = eager["ad_ids"].clone(), eager["scores"].clone()
        cids, cd = eager["candidate_ids"].clone(), eager["candidate_scores"].clone()
        assert (cd[:, 1:] >= cd[:, :-1]).all()                   # exact L2 distances, ascending
        plain_cd = rec0.recommend_device(uc, un, 10, 200)["candidate_scores"]
        assert not torch.equal(plain_cd, cd)
        g = rec.capture(B, 10, 200)
        assert index._pq.rows.data_ptr() in {t.data_ptr() for t in g._pinned if isinstance(t, torch.Tensor)}
        out = g(uc, un)
        torch.cuda.synchronize()
        assert torch.equal(out["ad_ids"], ids) and torch.equal(out["scores"], sc)
        assert torch.equal(out["candidate_ids"], cids) and torch.equal(out["candidate_scores"], cd)
        assert_replay_survives_a_larger_eager_search(rec, g, uc, un, user, nnum)
    with pytest.raises(NotImplementedError):
        ShardedRecommender(rec, rank=0, world=1, shard_offset=0)
