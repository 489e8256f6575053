"""CPU: the three statements of the cross-shard merge rule agree before any of them is held against the kernel.
tests/merge_oracle.merge_reference (the reference of tests/test_merge_surface_gpu.py) against oracle.search.merge_partial
(the CPU engine of tests/test_sharded_cpu.py), both against the proof rule written out by hand, and the case builders and
the wire layout of the GPU file against their own premises."""
import numpy as np
import pytest

import oracle
from tests import merge_oracle as mo


def _oracle(S, P, k):
    G = len(S)
    return oracle.search.merge_partial([np.asarray(S[g]) for g in range(G)], [np.asarray(P[g]).astype(np.int64) for g in range(G)],
                                       [0] * G, k)


def _same(ref, got):
    return mo.scores_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])


def _small_random_case(rng):
    """Few lists of few entries with scores from a handful of values (ties everywhere, both zeros, both infinities), distinct
    positions from a small range (the position decides), unfilled tails, and k from 1 to above the total."""
    G, L, nq = int(rng.integers(1, 5)), int(rng.integers(1, 6)), int(rng.integers(1, 4))
    k = int(rng.integers(1, G * L + 3))
    values = np.array([2.0, 1.0, 1.0, 0.0, -0.0, -1.0, np.inf, -np.inf, 1e-45, 3e-39], dtype=np.float32)
    S = values[rng.integers(0, len(values), (G, nq, L))]
    P = np.stack([rng.permutation(2 * G * L)[:G * L].reshape(G, L) for _ in range(nq)], axis=1).astype(np.int64)
    S, P = mo.sort_lists(S, P)
    S, P = np.ascontiguousarray(S), np.ascontiguousarray(P)
    if rng.random() < 0.5:
        t = rng.integers(0, L + 1, (G, nq))
        cut = np.arange(L)[None, None, :] >= (L - t)[:, :, None]
        S[cut], P[cut] = -np.inf, -1
    return S, P, k


def test_reference_equals_the_oracle_on_nan_free_lists():
    rng = np.random.default_rng(20)
    seen = {"tie_at_k": 0, "tail": 0, "k_above_total": 0, "inexact": 0, "proven": 0}
    for _ in range(400):
        S, P, k = _small_random_case(rng)
        ref, got = mo.merge_reference(S, P, k), _oracle(S, P, k)
        assert _same(ref, got), (S, P, k, ref, got)
        seen["tail"] += bool((P < 0).any())
        seen["k_above_total"] += k > S.shape[0] * S.shape[2]
        seen["inexact"] += int(ref[2].sum())
        seen["proven"] += int((~ref[2]).sum())
        flat = np.sort(S.transpose(1, 0, 2).reshape(S.shape[1], -1), axis=1)[:, ::-1]
        seen["tie_at_k"] += bool(k < flat.shape[1] and (flat[:, k - 1] == flat[:, k]).any())
    assert min(seen.values()) >= 20, seen


def test_nan_scores_are_dropped_by_reference_and_oracle_alike():
    """The kernel drops an entry whose score is NaN, whatever its position.  oracle.search._merge used to keep it behind every
    finite score: list 0's (NaN, 3) came back as the third result, the merge had k entries, and the query counted as proven
    against (NaN, 3).  The contract is the kernel's: two entries merge, list 1 is full, the query is inexact."""
    S = S2 = np.array([[[5.0, np.nan]], [[4.0, 3.0]]], dtype=np.float32)          # [list][query][entry]
    P = np.array([[[0, 3]], [[1, -1]]], dtype=np.int32)                           # (3.0, -1): dropped as well, list 1 not full
    P2 = np.array([[[0, 3]], [[1, 2]]], dtype=np.int32)
    for s, p, k, want_i, want_bad in ((S, P, 3, [0, 1, -1], False), (S2, P2, 4, [0, 1, 2, -1], True), (S2, P2, 3, [0, 1, 2], False)):
        ref, got = mo.merge_reference(s, p, k), _oracle(s, p, k)
        assert _same(ref, got)
        assert ref[1][0].tolist() == want_i and not np.isnan(ref[0]).any() and bool(ref[2][0]) == want_bad
    rng = np.random.default_rng(21)
    hit = 0
    for _ in range(300):                                               # ... and wherever a NaN stands
        S, P, k = _small_random_case(rng)
        nan = rng.random(S.shape) < 0.2
        S[nan] = np.nan
        ref, got = mo.merge_reference(S, P, k), _oracle(S, P, k)
        assert _same(ref, got), (S, P, k, ref, got)
        assert not np.isnan(ref[0]).any()
        hit += bool(nan[:, :, -1].any())
    assert hit >= 100


def test_proof_rule_table_by_hand():
    S, P, want = mo.proof_table_arrays()
    assert S.shape == (3, 10, 2) and len({row[0] for row in mo.PROOF_TABLE}) == 10
    D, I, bad = mo.merge_reference(S, P, mo.PROOF_K)
    for q, row in enumerate(mo.PROOF_TABLE):
        assert bool(bad[q]) == row[3], row[0]
    assert int(bad.sum()) == 5
    assert _same((D, I, bad), _oracle(S, P, mo.PROOF_K))
    # the merged lists the table's comments spell out
    assert I[0].tolist() == [0, 1, 2, 4] and I[2].tolist() == [0, 2, 4, 1] and I[3].tolist() == [0, 2, 1, 3]
    assert I[4].tolist() == [0, 2, 4, 3] and I[5].tolist() == [0, 2, 4, 3] and I[6].tolist() == [1, 2, 4, 5]
    assert I[7].tolist() == [1, 3, 5, -1] and I[8].tolist() == [0, 2, 4, -1] and I[9].tolist() == [1, 2, -1, -1]
    assert D[7].tolist() == [8.0, 6.0, 4.0, -np.inf]


@pytest.mark.parametrize("shape", [(8, 128, 500), (2, 250, 500)])
def test_relation_family_moves_one_last_entry_across_the_kth_key(shape):
    G, L, k = shape
    S, P, want = mo.relation_family(G, L, k, seed=31)
    D, I, bad = mo.merge_reference(S, P, k)
    assert np.array_equal(bad, want)
    assert np.array_equal(mo.sort_lists(S, P)[1], P)                   # every list is still sorted
    x = P[G // 2, :, -1]
    if G * L > k:
        assert bad.tolist() == [True, False, False, True, False]
        assert I[1, k - 1] == x[1] and I[2, k - 1] + 1 == x[2] and I[3, k - 1] - 1 == x[3] and I[3, k - 2] == x[3]
        assert D[2, k - 1] == S[G // 2, 2, -1] and D[3, k - 1] == S[G // 2, 3, -1]
    assert _same((D, I, bad), _oracle(S, P, k))


def test_single_cut_list_is_the_only_reason():
    S1, P1, S0, P0 = mo.single_cut_list(1024, 16, 3, seed=41, g_cut=700)
    assert mo.merge_reference(S1, P1, 500)[2].all() and not mo.merge_reference(S0, P0, 500)[2].any()
    assert not mo.merge_reference(np.delete(S1, 700, axis=0), np.delete(P1, 700, axis=0), 500)[2].any()


@pytest.mark.parametrize("variant", ["full", "tails", "nan", "neg_pos", "nan_query", "neginf_query"])
def test_case_builders_keep_their_premises(variant):
    G, L, nq = 3, 11, 9
    S, P = mo.build_case(G, L, nq, seed=5, variant=variant, palette_queries=0.3)
    assert S.dtype == np.float32 and P.dtype == np.int32 and S.shape == P.shape == (G, nq, L)
    S2, P2 = mo.build_case(G, L, nq, seed=5, variant=variant, palette_queries=0.3)
    assert np.array_equal(S, S2, equal_nan=True) and np.array_equal(P, P2)            # seeded
    pal = set(mo.PALETTE.view(np.uint32).tolist())
    only = 0
    for q in range(nq):
        s, p = S[:, q].reshape(-1), P[:, q].reshape(-1).astype(np.int64)
        live = p >= 0
        assert len(set(p[live].tolist())) == int(live.sum())                           # shards are disjoint
        only += set(s.view(np.uint32).tolist()) <= pal
        for g in range(G):                                                             # the entries that exist are in order
            ok = (P[g, q] >= 0) & ~np.isnan(S[g, q])
            ss, pp = S[g, q][ok].astype(np.float64), P[g, q][ok].astype(np.int64)
            assert np.array_equal(np.lexsort((pp, -ss)), np.arange(len(ss)))
    assert (P == 0).any() and (P == mo.POS_MAX).any() and (P >= 2 ** 30).sum() > P.size // 16
    if variant in ("full", "tails", "neg_pos"):
        assert only >= 1                                                               # a query of palette values only
    if variant == "tails":
        t = (P < 0).sum(axis=2)
        assert (t == 0).any() and (t == L).any() and np.isneginf(S[P < 0]).all()
        assert all((P[g, q, L - t[g, q]:] < 0).all() and (P[g, q, :L - t[g, q]] >= 0).all() for g in range(G) for q in range(nq))
    elif variant == "nan":
        assert np.isnan(S[:, :, -1]).any() and np.isnan(S[:, :, :-1]).any() and (P >= 0).all()
    elif variant == "neg_pos":
        assert (P[:, :, :-1] < 0).any() and (P[:, :, -1] >= 0).all() and np.isfinite(S[P < 0]).any()
    elif variant == "nan_query":
        assert np.isnan(S[:, nq // 2]).all() and not np.isnan(np.delete(S, nq // 2, axis=1)).any()
    elif variant == "neginf_query":
        assert np.isneginf(S[:, nq // 2]).all() and (P[:, nq // 2] >= 0).all()
        D, I, _ = mo.merge_reference(S, P, G * L)
        assert np.array_equal(I[nq // 2], np.sort(P[:, nq // 2].reshape(-1)))          # returned, ordered by position


def test_palette_is_what_the_suite_says_it_is():
    p = mo.PALETTE
    assert len(p) == 12 and np.isposinf(p[0]) and np.isneginf(p[1]) and np.isfinite(p[2:]).all()
    assert p[5] > p[4] > p[6] and p[5].view(np.uint32) - 1 == p[4].view(np.uint32) == p[6].view(np.uint32) + 1   # adjacent floats
    assert p[7] == 0 and p[8] == 0 and np.signbit(p[8]) and not np.signbit(p[7])
    assert p[9].view(np.uint32) == 1 and p[10].view(np.uint32) == 0x80000001 and 0 < p[11] < np.finfo(np.float32).tiny


@pytest.mark.parametrize("gaps", [(0, 0, 0), (4, 0, 0), (0, 12, 8), (260, 4, 4)])
def test_pack_layout(gaps):
    from amdrec.sharded import packed_layout
    score_gap, pos_gap, lead = gaps
    G, L, nq = 3, 5, 4
    S, P = mo.build_case(G, L, nq, seed=9)
    buf, s_off, p_off, stride = mo.pack_host(S, P, nq, score_gap=score_gap, pos_gap=pos_gap, lead=lead)
    s_bytes = nq * L * 4
    assert len(buf) == lead + G * stride and stride == 2 * s_bytes + score_gap + pos_gap
    assert s_off == lead and p_off == lead + s_bytes + score_gap
    if gaps == (0, 0, 0):
        # exactly what ShardedRecommender._step packs per rank: chunk g = [scores | positions]
        assert (p_off, stride) == packed_layout(nq, L)
        want = np.concatenate([np.concatenate([S[g].reshape(-1).view(np.uint8), P[g].reshape(-1).view(np.uint8)]) for g in range(G)])
        assert np.array_equal(buf, want)
    seen = np.zeros(len(buf), dtype=bool)
    for g in range(G):
        a, b = s_off + g * stride, p_off + g * stride
        assert np.array_equal(buf[a:a + s_bytes].view(np.float32).reshape(nq, L), S[g], equal_nan=True)
        assert np.array_equal(buf[b:b + s_bytes].view(np.int32).reshape(nq, L), P[g])
        assert (buf[a + s_bytes:b].view(np.float32) == mo.GAP_SCORE).all() and b - a - s_bytes == score_gap
        assert (buf[b + s_bytes:a + stride].view(np.int32) == mo.GAP_POS).all()
        seen[a:a + stride] = True
    assert (buf[:lead].view(np.float32) == mo.GAP_SCORE).all() and seen[lead:].all() and not seen[:lead].any()
    sb, pb, st = mo.split_host(S, P, nq, 24)
    assert st == s_bytes + 24 and len(sb) == len(pb) == G * st
    for g in range(G):
        assert np.array_equal(sb[g * st:g * st + s_bytes].view(np.float32).reshape(nq, L), S[g], equal_nan=True)
        assert np.array_equal(pb[g * st:g * st + s_bytes].view(np.int32).reshape(nq, L), P[g])
        assert (sb[g * st + s_bytes:(g + 1) * st].view(np.float32) == mo.GAP_SCORE).all()
        assert (pb[g * st + s_bytes:(g + 1) * st].view(np.int32) == mo.GAP_POS).all()


def test_grid_is_the_issue_s_grid():
    assert len(mo.GRID) == len(set(mo.GRID)) == 27
    assert all(1 <= g * l <= 16384 and 1 <= k <= 16384 for g, l, k in mo.GRID)
    sizes = set()
    for g, l, _ in mo.GRID:
        P = 2
        while P < g * l:
            P <<= 1
        sizes.add(P)
    assert sizes == {2 ** e for e in range(1, 15)}                     # every sort size the kernel can run at
    assert mo.grid_nq(2, 2048) == 3 and mo.grid_nq(8, 500) == 9
