"""GPU: topk_merge_kernel (csrc/search.hip) behind amdrec_topk_merge and amdrec_topk_merge_partial, called through the ABI
itself on lists built by tests/merge_oracle.py, against merge_oracle.merge_reference - bit for bit: positions, scores (a zero
may carry either sign), the count of unproven queries, and every word next to the outputs and the counter.  Every case runs
twice.  (a) the shape grid: every sort size, list counts 1 .. 16384, k below, at and above the total; (b) strides, offsets,
query slices, a large grid; (c) what the lists hold: ties by the thousand, unfilled tails, NaN, -1, +-inf, +-0, denormals;
(d) every branch of the proof rule; (e) real search results at the 16384-entry limit."""
import numpy as np
import pytest
import torch

from tests import merge_oracle as mo

pytestmark = pytest.mark.gpu


def _check(res, ref, k, partial=True):
    D, I, bad = ref
    assert res.D.shape == (len(D), k)
    assert np.array_equal(res.I, I)
    assert mo.scores_equal(res.D, D)
    assert (res.guard_D == mo.GUARD).all() and (res.guard_I == mo.GUARD).all()
    assert res.counter[0] == mo.GUARD and res.counter[2] == mo.GUARD
    assert res.delta == (int(bad.sum()) if partial else 0)


def _same_run(a, b):
    assert np.array_equal(a.I, b.I) and np.array_equal(a.D.view(np.uint32), b.D.view(np.uint32)) and a.delta == b.delta


def _run(ptrs, G, L, q0, nq, k, ref, partial=True):
    """One launch, twice; -> the first result, checked against rows [q0, q0 + nq) of ``ref``."""
    sp, pp, stride = ptrs
    res = mo.run_merge(sp, pp, G, L, stride, q0, nq, k, partial=partial)
    _check(res, tuple(r[q0:q0 + nq] for r in ref), k, partial)
    _same_run(res, mo.run_merge(sp, pp, G, L, stride, q0, nq, k, partial=partial))
    return res


def _case(S, P, k, partial=True):
    """A whole batch in the packed layout."""
    G, nq, L = S.shape
    ref = mo.merge_reference(S, P, k)
    buf, sp, pp, stride = mo.pack(S, P, nq)
    res = _run((sp, pp, stride), G, L, 0, nq, k, ref, partial)
    del buf
    return res, ref


# ---- (a) the shape grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mo.GRID, ids=lambda s: "x".join(map(str, s)))
def test_shape_grid(shape):
    G, L, k = shape
    nq = mo.grid_nq(G, L)
    variant = "tails" if (G * L) % 2 else "full"                 # odd totals also carry unfilled tails
    S, P = mo.build_case(G, L, nq, seed=1000 + G * 7 + L * 3 + k, variant=variant, palette_queries=0.2)
    res, ref = _case(S, P, k)
    if L == k:
        full, _ = _case(S, P, k, partial=False)                  # amdrec_topk_merge: the same D and I, no counter
        assert np.array_equal(full.I, res.I) and np.array_equal(full.D.view(np.uint32), res.D.view(np.uint32))


# ---- (b) layout -----------------------------------------------------------------------------------------------------------
LAYOUT_SHAPE, LAYOUT_NQ = (8, 128, 500), 37
SLICES = [(0, 37), (5, 11), (36, 1), (0, 1)]


@pytest.fixture(scope="module")
def layout_case():
    G, L, k = LAYOUT_SHAPE
    S, P = mo.build_case(G, L, LAYOUT_NQ, seed=87, variant="neg_pos", palette_queries=0.2)
    ref = mo.merge_reference(S, P, k)
    assert 0 < ref[2][5:16].sum() < 11 and ref[2][36] and not ref[2][0]  # counted and proven queries in and next to the slices
    return S, P, ref


@pytest.mark.parametrize("gaps", [(0, 0, 0), (4, 0, 0), (0, 12, 8), (260, 4, 4), "split"], ids=str)
def test_layout_strides_offsets_and_slices(layout_case, gaps):
    G, L, k = LAYOUT_SHAPE
    S, P, ref = layout_case
    if gaps == "split":                                          # scores and positions in two allocations, one stride
        sb, pb, stride = mo.split_host(S, P, LAYOUT_NQ, 40)
        keep = (torch.from_numpy(sb).cuda(), torch.from_numpy(pb).cuda())
        ptrs = (keep[0].data_ptr(), keep[1].data_ptr(), stride)
    else:
        keep, sp, pp, stride = mo.pack(S, P, LAYOUT_NQ, score_gap=gaps[0], pos_gap=gaps[1], lead=gaps[2])
        assert keep.numel() == gaps[2] + G * stride
        ptrs = (sp, pp, stride)
    whole = None
    for q0, nq in SLICES:
        res = _run(ptrs, G, L, q0, nq, k, ref)
        whole = res if whole is None else whole
        assert np.array_equal(res.I, whole.I[q0:q0 + nq]) and np.array_equal(res.D.view(np.uint32), whole.D[q0:q0 + nq].view(np.uint32))
        assert res.delta == int(ref[2][q0:q0 + nq].sum())
    del keep


def test_layout_large_grid():
    G, L, k, nq = 3, 16, 40, 4099
    S, P = mo.build_case(G, L, nq, seed=78, variant="tails", palette_queries=0.1)
    res, ref = _case(S, P, k)
    assert 0 < ref[2].sum() < nq
    buf, sp, pp, stride = mo.pack(S, P, nq, score_gap=8, pos_gap=4, lead=12)
    _run((sp, pp, stride), G, L, 4000, 99, k, ref)               # the last rows of a large batch, not the packed stride
    del buf


# ---- (c) contents -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["full", "tails", "nan", "neg_pos", "nan_query", "neginf_query"])
@pytest.mark.parametrize("shape", [(8, 128, 500), (3, 11, 20), (2, 500, 500)], ids=lambda s: "x".join(map(str, s)))
def test_contents(shape, variant):
    G, L, k = shape
    nq = 24
    S, P = mo.build_case(G, L, nq, seed=300 + G + len(variant), variant=variant, palette_queries=0.3)
    res, ref = _case(S, P, k)
    assert not np.isnan(res.D).any()
    q = nq // 2
    if variant == "nan_query":
        assert (res.I[q] == -1).all() and np.isneginf(res.D[q]).all() and not ref[2][q]
    if variant == "neginf_query":                                # returned, ordered by position
        m = min(k, G * L)
        assert np.array_equal(res.I[q, :m], np.sort(P[:, q].reshape(-1).astype(np.int64))[:m]) and np.isneginf(res.D[q]).all()
    if L == k:
        _case(S, P, k, partial=False)


# ---- (d) the proof rule -----------------------------------------------------------------------------------------------------
def test_proof_rule_table_on_the_device():
    S, P, want = mo.proof_table_arrays()
    res, ref = _case(S, P, mo.PROOF_K)
    assert np.array_equal(ref[2], want) and res.delta == 5
    buf, sp, pp, stride = mo.pack(S, P, len(want))
    for q, row in enumerate(mo.PROOF_TABLE):                     # row by row: which query is counted, not only how many
        assert mo.run_merge(sp, pp, 3, 2, stride, q, 1, mo.PROOF_K).delta == int(row[3]), row[0]
    del buf


@pytest.mark.parametrize("shape", [(8, 128, 500), (2, 250, 500)], ids=lambda s: "x".join(map(str, s)))
def test_proof_rule_one_last_entry_across_the_kth_key(shape):
    G, L, k = shape
    S, P, want = mo.relation_family(G, L, k, seed=31)
    nq = len(want)
    ref = mo.merge_reference(S, P, k)
    assert np.array_equal(ref[2], want)
    buf, sp, pp, stride = mo.pack(S, P, nq)
    _run((sp, pp, stride), G, L, 0, nq, k, ref)
    for q in range(nq):
        assert mo.run_merge(sp, pp, G, L, stride, q, 1, k).delta == int(want[q]), mo.RELATIONS[q]
    del buf


def test_proof_rule_cut_list_beyond_the_first_512():
    G, L, k, nq = 1024, 16, 500, 3
    S1, P1, S0, P0 = mo.single_cut_list(G, L, nq, seed=41, g_cut=700)
    res, ref = _case(S1, P1, k)
    assert ref[2].all() and res.delta == nq
    res, ref = _case(S0, P0, k)
    assert not ref[2].any() and res.delta == 0


# ---- (e) real lists at the limit ----------------------------------------------------------------------------------------------
def test_real_shard_lists_at_the_limit():
    """8 emulated shards of a 24 000-row corpus, top-2048: 8 x 2048 = 16384 entries per query, the kernel's limit and its
    128 KB of LDS.  HipEngine.merge of the full lists == the unsharded search; the same lists cut to 512 entries == the
    reference, and == the unsharded search wherever the cut is proven harmless."""
    from amdrec import synth
    from amdrec.index import FAISSIndex
    from amdrec.sharded import HipEngine, packed_layout
    n, dim, nq, k, G, short = 24_000, 64, 5, 2048, 8, 512
    xb, xq = synth.unit_corpus(n, dim, seed=51), synth.unit_corpus(nq, dim, seed=52)
    full = FAISSIndex(dim, index_type="Flat")
    full.add(xb)
    q = torch.from_numpy(xq).cuda()
    ref_pos, ref_sc = full.search_device(q, k, return_positions=True)
    s_bytes, chunk = packed_layout(nq, k)
    gathered = torch.empty(chunk * G, dtype=torch.uint8, device="cuda")
    per = n // G
    Ds, Is = [], []
    for g in range(G):
        sh = FAISSIndex(dim, index_type="Flat")
        sh.add(xb[g * per:(g + 1) * per])
        pos, sc = sh.search_device(q, k, return_positions=True, pos_offset=g * per)
        c = gathered[g * chunk:(g + 1) * chunk]
        c[:s_bytes].view(torch.float32).copy_(sc.reshape(-1))
        c[s_bytes:].view(torch.int32).copy_(pos.reshape(-1))
        Ds.append(sc.cpu().numpy())
        Is.append(pos.cpu().numpy())
    sc, pos = HipEngine(None, 0).merge(gathered, G, nq, k, 0, nq)
    assert torch.equal(pos, ref_pos) and torch.equal(sc, ref_sc)
    S, P = np.stack(Ds), np.stack(Is)
    assert np.array_equal(np.frombuffer(gathered.cpu().numpy(), dtype=np.uint8), mo.pack_host(S, P, nq)[0])
    _case(S, P.astype(np.int32), k, partial=False)
    res, ref = _case(S[:, :, :short].copy(), P[:, :, :short].astype(np.int32), k)
    ok = ~ref[2]
    assert ok.any()
    assert np.array_equal(res.I[ok], ref_pos.cpu().numpy()[ok]) and np.array_equal(res.D[ok], ref_sc.cpu().numpy()[ok])
