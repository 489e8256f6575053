"""Per-group caps on the GPU.  ``amdrec_select_topk_capped`` and ``amdrec_group_cap_compact`` are compared with the greedy loop
of tests/group_cap_oracle.py - never with each other - and every comparison is exact: the oracle is fed the device's own
logits, or the device's own top-K1, so no tolerance is involved.  Then the index (``search_device(max_per_group=)`` on Flat, IVF
and IVFPQ, default and custom ids, with exclusion lists and masks), persistence and the live corpus, and the serving pipeline
(both head modes, the captured graph, the reference API).  Without the new arguments nothing runs that did not run before."""
import numpy as np
import pytest
import torch

from amdrec import _lib, group_cap as gc
from tests import eligible_oracle as eo
from tests import group_cap_oracle as go
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

N_TASKS, N_ROWS = 3, 64
VALUES = np.array([-2.0, -0.0, 0.0, 0.5, 4.0], dtype=np.float32)        # 5 distinct floats (the zeros tie): heavy ties


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    """float32 tensor / array -> its bit patterns (NaN-safe equality)."""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _inputs(n_users, k_c, seed, n_rows=N_ROWS):
    """Logits [3, n_users * k_c] from 5 values with NaNs, positions with -1 holes, ids, and group keys from 3 values plus -1."""
    rng = np.random.default_rng(seed)
    logits = rng.choice(VALUES, size=(N_TASKS, n_users * k_c))
    logits[rng.random(logits.shape) < 0.08] = np.nan
    pos = rng.integers(0, n_rows, size=(n_users, k_c)).astype(np.int64)
    pos[rng.random(pos.shape) < 0.1] = -1
    ids = np.where(pos >= 0, pos * 3 + 1, 10 ** 6 + np.arange(k_c)[None])     # (an unfilled slot's id is the caller's to choose)
    group_of = rng.choice(np.array([-1, 3, 1 << 33, 7], dtype=np.int64), size=n_rows)
    return logits, ids, pos, group_of


def _select(entry, logits, ids, pos, top_k, tail=(), rank_task=0):
    """One selection entry on device tensors, every output in a guarded exact-size buffer -> (ids, scores, slots) numpy."""
    n_users, k_c = ids.shape
    out_ids = guarded((n_users, top_k), torch.int64, "cuda", "output")
    scores = guarded((N_TASKS, n_users, top_k), torch.float32, "cuda", "output")
    slots = guarded((n_users, top_k), torch.int32, "cuda", "output")
    _lib.check(entry(_lib.ptr(logits), logits.stride(0), N_TASKS, rank_task, _lib.ptr(ids), _lib.ptr(pos), n_users, k_c, top_k,
                     _lib.ptr(out_ids), _lib.ptr(scores), _lib.ptr(slots), *tail, _lib.stream_ptr("cuda")))
    for t in (out_ids, scores, slots):
        t.check()
    return out_ids.cpu().numpy(), scores.cpu().numpy(), slots.cpu().numpy()


def _capped(logits, ids, pos, top_k, group_of, cap, n_rows=None, rank_task=0):
    lib = _lib.load()
    n_rows = group_of.shape[0] if n_rows is None else n_rows
    return _select(lib.amdrec_select_topk_capped, logits, ids, pos, top_k, (_lib.ptr(group_of), n_rows, cap), rank_task)


def _prob_by_slot(logits, n_users, k_c):
    """Every candidate's probabilities as the device writes them: the uncapped selection of ALL k_c slots (no positions:
    every slot is a candidate), scattered back by slot -> [3, n_users, k_c]."""
    lib = _lib.load()
    ids = torch.zeros((n_users, k_c), dtype=torch.int64, device="cuda")
    _, sc, sl = _select(lib.amdrec_select_topk, logits, ids, None, k_c)
    assert (np.sort(sl, axis=1) == np.arange(k_c)[None]).all()
    table = np.empty_like(sc)
    for u in range(n_users):
        table[:, u, sl[u]] = sc[:, u]
    return table


def _check_against_oracle(got, logits_np, ids, pos, top_k, group_of, cap, table, rank_task=0, what=""):
    n_users, k_c = pos.shape
    e_ids, e_slots = go.select_topk_capped(logits_np[rank_task].reshape(n_users, k_c), ids, pos, top_k, group_of, cap)
    assert np.array_equal(got[0], e_ids), f"ids {what}"
    assert np.array_equal(got[2], e_slots), f"slots {what}"
    assert np.array_equal(_bits(got[1]), _bits(go.scores_at(table, e_slots))), f"scores {what}"
    return e_ids, e_slots


# k_c walks the keys-per-lane and path boundaries (128 / 512), top_k the wave kernel's limit (32), n_users a partial workgroup
@pytest.mark.parametrize("k_c", [1, 2, 63, 64, 65, 128, 129, 500, 512, 513, 2048])
def test_select_topk_capped_is_the_greedy_loop(k_c):
    lib = _lib.load()
    saturated = 0
    for n_users in (1, 5, 9):
        logits_np, ids_np, pos_np, groups_np = _inputs(n_users, k_c, 1000 * n_users + k_c)
        logits, ids, pos, group_of = _dev(logits_np), _dev(ids_np), _dev(pos_np), _dev(groups_np)
        table = _prob_by_slot(logits, n_users, k_c)
        for top_k in (1, 10, 32, 33):
            plain = _select(lib.amdrec_select_topk, logits, ids, pos, top_k)
            for cap in (1, 2, top_k, top_k + 1):
                got = _capped(logits, ids, pos, top_k, group_of, cap)
                e_ids, e_slots = _check_against_oracle(got, logits_np, ids_np, pos_np, top_k, groups_np, cap, table,
                                                       what=f"users {n_users} k_c {k_c} top_k {top_k} cap {cap}")
                saturated += int(not np.array_equal(e_slots, plain[2]))
            # a cap that no group can reach is the uncapped selection, in all three outputs
            free = _capped(logits, ids, pos, top_k, group_of, max(k_c, 1))
            assert np.array_equal(free[0], plain[0]) and np.array_equal(free[2], plain[2])
            assert np.array_equal(_bits(free[1]), _bits(plain[1]))
    assert saturated or k_c <= 2                                          # the caps did bite
    # the ranking task is an argument: rank by task 2
    got = _capped(logits, ids, pos, 10, group_of, 2, rank_task=2)
    _check_against_oracle(got, logits_np, ids_np, pos_np, 10, groups_np, 2, table, rank_task=2)


@pytest.mark.parametrize("k_c,top_k", [(65, 10), (500, 10), (500, 33), (2048, 32)])
def test_one_group_and_cap_one_returns_one_ad_and_the_unfilled_tail(k_c, top_k):
    n_users = 5
    logits_np, ids_np, pos_np, _ = _inputs(n_users, k_c, 77)
    pos_np = np.abs(pos_np)                                               # every slot filled
    ids_np = pos_np * 3 + 1
    groups_np = np.full(N_ROWS, 1 << 40, dtype=np.int64)
    logits, ids, pos = _dev(logits_np), _dev(ids_np), _dev(pos_np)
    got = _capped(logits, ids, pos, top_k, _dev(groups_np), 1)
    table = _prob_by_slot(logits, n_users, k_c)
    _check_against_oracle(got, logits_np, ids_np, pos_np, top_k, groups_np, 1, table)
    assert (got[0][:, 0] >= 0).all() and (got[0][:, 1:] == -1).all() and (got[2][:, 1:] == -1).all()
    assert (got[1][:, :, 1:] == 0.0).all()
    # ... and with every row ungrouped the cap is void
    plain = _select(_lib.load().amdrec_select_topk, logits, ids, pos, top_k)
    free = _capped(logits, ids, pos, top_k, _dev(np.full(N_ROWS, -5, dtype=np.int64)), 1)
    assert np.array_equal(free[0], plain[0]) and np.array_equal(free[2], plain[2]) and np.array_equal(_bits(free[1]), _bits(plain[1]))


@pytest.mark.parametrize("k_c,top_k", [(128, 10), (500, 10), (700, 40)])
def test_positions_beyond_the_group_array_are_ungrouped_and_never_read(k_c, top_k):
    """group_of lives in an exact-size guarded buffer of 50 keys; half of the candidates' positions lie beyond it.  A read
    past the end would see the guard band's bytes - one positive key for all of them - and cap what must not be capped."""
    n_users, n_rows = 5, 50
    logits_np, _, pos_np, _ = _inputs(n_users, k_c, 5, n_rows=2 * n_rows)
    ids_np = np.where(pos_np >= 0, pos_np * 3 + 1, -1)
    groups_np = np.random.default_rng(6).choice(np.array([-1, 0, 9], dtype=np.int64), size=n_rows)
    group_of = guarded((n_rows,), torch.int64, "cuda", "scratch")
    group_of.copy_(_dev(groups_np))
    logits, ids, pos = _dev(logits_np), _dev(ids_np), _dev(pos_np)
    table = _prob_by_slot(logits, n_users, k_c)
    for cap in (1, 2):
        got = _capped(logits, ids, pos, top_k, group_of, cap, n_rows=n_rows)
        e_ids, e_slots = _check_against_oracle(got, logits_np, ids_np, pos_np, top_k, groups_np, cap, table)
    assert (pos_np[np.arange(n_users)[:, None], np.maximum(e_slots, 0)] >= n_rows).any()      # such candidates did win
    group_of.check()
    # no group array at all: n_group_rows = 0 makes every candidate ungrouped
    plain = _select(_lib.load().amdrec_select_topk, logits, ids, pos, top_k)
    free = _select(_lib.load().amdrec_select_topk_capped, logits, ids, pos, top_k, (None, 0, 1))
    assert np.array_equal(free[0], plain[0]) and np.array_equal(free[2], plain[2])


# ---- amdrec_group_cap_compact --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [1, 2, 64, 65, 500, 1000, 2048])
def test_group_cap_compact_is_the_greedy_loop(kc):
    n_rows = 300
    for nq in (1, 7):
        rng = np.random.default_rng(kc * 10 + nq)
        groups_np = rng.choice(np.array([-1, 0, 1, 2, 5, 1 << 50], dtype=np.int64), size=n_rows)
        pos_np = rng.integers(0, n_rows + 40, size=(nq, kc)).astype(np.int64)    # (>= n_rows: outside the array)
        for q in range(1, nq):                                               # unfilled tails up to half the row, none in row 0
            tail = (q * kc) // (2 * (nq - 1))
            pos_np[q, kc - tail:] = -1
        group_of = guarded((n_rows,), torch.int64, "cuda", "scratch")
        group_of.copy_(_dev(groups_np))
        for fill in (np.float32(-np.inf), np.float32(np.inf)):
            sc_np = np.sort(rng.standard_normal((nq, kc)).astype(np.float32), axis=1)[:, ::-1].copy()
            sc_np[pos_np < 0] = fill
            pos, sc = _dev(pos_np), _dev(sc_np)
            for k in sorted({1, max(kc // 2, 1), kc}):
                for cap in (1, 3, kc):
                    out_pos = guarded((nq, k), torch.int64, "cuda", "output")
                    out_sc = guarded((nq, k), torch.float32, "cuda", "output")
                    _lib.check(_lib.load().amdrec_group_cap_compact(
                        _lib.ptr(pos), _lib.ptr(sc), nq, kc, _lib.ptr(group_of), n_rows, cap, k, float(fill),
                        _lib.ptr(out_pos), _lib.ptr(out_sc), _lib.stream_ptr("cuda")))
                    out_pos.check(), out_sc.check()
                    e_pos, e_sc = go.compact(pos_np, sc_np, groups_np, cap, k, fill)
                    assert np.array_equal(out_pos.cpu().numpy(), e_pos), (nq, k, cap)
                    assert np.array_equal(_bits(out_sc), _bits(e_sc)), (nq, k, cap)
        group_of.check()
    # the binding helper, and a cap nothing reaches: the first k entries as they were
    p, s = gc.compact(_dev(pos_np), _dev(sc_np), _dev(groups_np), n_rows, kc, kc, float("inf"))
    assert np.array_equal(p.cpu().numpy(), pos_np) and np.array_equal(_bits(s), _bits(sc_np))


# ---- the index -------------------------------------------------------------------------------------------------------------
N, D, NQ = 3000, 32, 33
KINDS = {
    "flat": dict(index_type="Flat"),
    "ivf": dict(index_type="IVF", nlist=16, nprobe=6, list_tags=True),
    "ivfpq": dict(index_type="IVFPQ", nlist=16, nprobe=6, list_tags=True),
    "ivfpq_refine": dict(index_type="IVFPQ", nlist=16, nprobe=6, list_tags=True, refine="fp32"),
}


def _corpus():
    rng = np.random.default_rng(11)
    centers = rng.standard_normal((12, D)).astype(np.float32)
    xb = centers[rng.integers(0, 12, N)] + 0.35 * rng.standard_normal((N, D)).astype(np.float32)
    xq = centers[rng.integers(0, 12, NQ)] + 0.35 * rng.standard_normal((NQ, D)).astype(np.float32)
    groups = np.where(rng.random(N) < 0.1, -1, rng.integers(0, 40, N)).astype(np.int64)   # near-duplicates share advertisers
    return xb, xq, groups


def _index(kind, ids_scheme):
    from amdrec.index import FAISSIndex
    xb, xq, groups = _corpus()
    id_map = np.arange(N) if ids_scheme == "default" else np.arange(N) * 3 + 11
    idx = FAISSIndex(D, **KINDS[kind])
    idx.add(xb, None if ids_scheme == "default" else id_map.tolist(), tags=eo.tags_for(N, 5), groups=groups)
    assert idx._identity == (ids_scheme == "default")
    return idx, idx._normalize_(_dev(xq)), groups, id_map


def _assert_capped_search(idx, q, k, cap, groups, id_map, overfetch=2, **kw):
    """The defining property: the cap rule over the same index's own search for K1, bit for bit; positions, ids, scores."""
    E = 0 if kw.get("exclude") is None else kw["exclude"].shape[1]
    k1 = min(k * overfetch, _lib.MAX_K - E)
    pos1, sc1 = idx.search_device(q, k1, normalize=False, return_positions=True, **kw)
    e_pos, e_sc = go.compact(pos1.cpu().numpy(), sc1.cpu().numpy(), groups, cap, k, go.fill_score(idx.index_type))
    pos, sc = idx.search_device(q, k, normalize=False, return_positions=True, max_per_group=cap, group_overfetch=overfetch, **kw)
    ids, sc2 = idx.search_device(q, k, normalize=False, max_per_group=cap, group_overfetch=overfetch, **kw)
    assert pos.shape == (q.shape[0], k) == sc.shape and pos.dtype == torch.int64 and sc.dtype == torch.float32
    assert np.array_equal(pos.cpu().numpy(), e_pos), "positions"
    assert np.array_equal(_bits(sc), _bits(e_sc)) and torch.equal(sc2, sc), "scores"
    assert np.array_equal(ids.cpu().numpy(), np.where(e_pos >= 0, id_map[np.maximum(e_pos, 0)], id_map[-1])), "ids"
    for row in e_pos:                                                        # what the rule is for
        g = groups[row[row >= 0]]
        assert (np.bincount(g[g >= 0], minlength=1) <= cap).all()
    return e_pos, pos1.cpu().numpy()


@pytest.mark.parametrize("ids_scheme", ["default", "custom"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_capped_search_is_the_rule_over_the_index_own_top_k1(kind, ids_scheme):
    idx, q, groups, id_map = _index(kind, ids_scheme)
    assert torch.equal(idx.get_groups().cpu(), torch.from_numpy(groups))
    rng = np.random.default_rng(8)
    k, E = 50, 20
    plain_ids, _ = idx.search_device(q, k + E, normalize=False)
    excl = np.full((NQ, E), -1, dtype=np.int64)
    for i in range(NQ):
        m = int(rng.integers(0, E + 1))
        excl[i, :m] = rng.choice(plain_ids[i].cpu().numpy(), size=m, replace=False)
    excl = _dev(excl)
    ma, my = (_dev(w.view(np.int64)) for w in eo.masks_for(NQ))
    short = full = 0
    for kw in (dict(), dict(exclude=excl), dict(require_all=ma, require_any=my), dict(exclude=excl, require_all=ma, require_any=my)):
        for cap in (1, 2):
            e_pos, pos1 = _assert_capped_search(idx, q, k, cap, groups, id_map, **kw)
            filled = (e_pos >= 0).sum(axis=1)
            short += int((filled < k).sum())
            full += int((filled == k).sum())
            assert not np.array_equal(e_pos, pos1[:, :k])                    # the cap dropped something
    assert short and full
    # another over-fetch factor, the clamp to AMDREC_MAX_K - E, and the shard offset of return_positions
    _assert_capped_search(idx, q, 10, 1, groups, id_map, overfetch=7)
    _assert_capped_search(idx, q, 700, 2, groups, id_map, overfetch=3, exclude=excl)
    pos, _ = idx.search_device(q, k, normalize=False, return_positions=True, max_per_group=2)
    off, _ = idx.search_device(q, k, normalize=False, return_positions=True, pos_offset=1000, max_per_group=2)
    assert torch.equal(off, torch.where(pos >= 0, pos + 1000, pos))
    # the numpy-level calls
    _, xq, _ = _corpus()
    want_ids, want_d = idx.search_device(_dev(xq), k, max_per_group=2, exclude=excl)
    got_ids, got_d = idx.search(xq, k, max_per_group=2, exclude=excl.cpu().numpy())
    b_ids, b_d = idx.batch_search(xq, k, batch_size=8, max_per_group=2, exclude=excl.cpu().numpy())
    assert np.array_equal(got_ids, want_ids.cpu().numpy()) and np.array_equal(_bits(got_d), _bits(want_d))
    # (an IVF scan's scores may differ in the last bits with the number of queries in the launch: chunk by chunk)
    chunks = [idx.search(xq[i:i + 8], k, max_per_group=2, exclude=excl.cpu().numpy()[i:i + 8]) for i in range(0, NQ, 8)]
    assert np.array_equal(b_ids, np.vstack([c[0] for c in chunks]))
    assert np.array_equal(_bits(b_d), _bits(np.vstack([c[1] for c in chunks])))


def test_no_cap_is_the_plain_search_without_the_new_launch():
    idx, q, groups, _ = _index("flat", "default")
    ids0, sc0 = idx.search_device(q, 100, normalize=False)
    _lib.profile_enable(True)
    try:
        ids1, sc1 = idx.search_device(q, 100, normalize=False, max_per_group=None)
        rep = _lib.profile_report()
        assert not [t for t in rep if "cap" in t], rep.keys()
        _lib.profile_enable(True)
        idx.search_device(q, 100, normalize=False, max_per_group=2)
        rep = _lib.profile_report()
        assert rep["group_cap_compact"]["launches"] == 1
    finally:
        _lib.profile_enable(False)
    assert torch.equal(ids1, ids0) and torch.equal(sc1, sc0)


def test_groups_follow_growth_set_groups_removal_and_save_load(tmp_path):
    from amdrec.index import FAISSIndex
    xb, _, groups = _corpus()
    idx = FAISSIndex(D, index_type="Flat")
    idx.add(xb[:700])
    assert idx._groups is None and (idx.get_groups() == -1).all() and len(idx.resident_tensors()) == 4
    with pytest.raises(ValueError, match="without group keys"):
        idx.search_device(_dev(xb[:2]), 5, max_per_group=1)
    idx.add(xb[700:900], groups=groups[700:900])                             # first keys: the earlier rows are ungrouped
    idx.add(xb[900:2000], groups=torch.from_numpy(groups[900:2000]).cuda())  # grows past the first capacity
    idx.add(xb[2000:])                                                       # no keys: ungrouped
    want = groups.copy()
    want[:700], want[2000:] = -1, -1
    assert np.array_equal(idx.get_groups().cpu().numpy(), want)
    assert any(t is idx._groups for t in idx.resident_tensors())
    n_before = idx.index.ntotal
    for bad, exc in ((groups[:5], ValueError), (groups.astype(np.float32), TypeError)):
        with pytest.raises(exc):
            idx.add(xb[:N], groups=bad)
        with pytest.raises(exc):
            idx.set_groups(bad)
    assert idx.index.ntotal == n_before and np.array_equal(idx.get_groups().cpu().numpy(), want)
    old = idx._groups
    snapshot = old.clone()
    idx.set_groups(groups)                                                   # out of place: the old tensor is never written
    assert idx._groups is not old and torch.equal(old, snapshot) and np.array_equal(idx.get_groups().cpu().numpy(), groups)
    gone = np.random.default_rng(2).choice(N, size=N // 4, replace=False)
    keep = np.setdiff1d(np.arange(N), gone)
    old = idx._groups
    assert idx.remove_ids(gone.tolist()) == len(gone)
    assert idx._groups is not old and np.array_equal(idx.get_groups().cpu().numpy(), groups[keep])
    path = str(tmp_path / "idx.bin")
    idx.save(path)
    back = FAISSIndex(D, index_type="Flat")
    back.load(path)
    assert np.array_equal(back.get_groups().cpu().numpy(), groups[keep])
    q = idx._normalize_(_dev(xb[5:9].copy()))
    a, b = idx.search_device(q, 20, normalize=False, max_per_group=1), back.search_device(q, 20, normalize=False, max_per_group=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    plain = FAISSIndex(D, index_type="Flat")                                 # a file without the array loads as ever
    plain.add(xb[:100])
    plain.save(path)
    back.load(path)
    assert back._groups is None


# ---- the serving pipeline --------------------------------------------------------------------------------------------------
def _clone(out):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _check_stage2(out, cand_pos, groups, top_k, cap):
    """ad_ids / scores of one recommend_device result against the oracle over that call's own logits and candidates."""
    B, k1 = cand_pos.shape
    logits = out["logits"]
    n_tasks = logits.shape[0]
    ids = torch.zeros((B, k1), dtype=torch.int64, device="cuda")
    lib = _lib.load()
    all_ids = torch.empty((B, k1), dtype=torch.int64, device="cuda")
    sc = torch.empty((n_tasks, B, k1), dtype=torch.float32, device="cuda")
    sl = torch.empty((B, k1), dtype=torch.int32, device="cuda")
    _lib.check(lib.amdrec_select_topk(_lib.ptr(logits), logits.stride(0), n_tasks, 0, _lib.ptr(ids), None, B, k1, k1,
                                      _lib.ptr(all_ids), _lib.ptr(sc), _lib.ptr(sl), _lib.stream_ptr("cuda")))
    sc, sl = sc.cpu().numpy(), sl.cpu().numpy()
    table = np.empty_like(sc)
    for u in range(B):
        table[:, u, sl[u]] = sc[:, u]
    e_ids, e_slots = go.select_topk_capped(logits[0].view(B, k1).cpu().numpy(), out["candidate_ids"].cpu().numpy(), cand_pos,
                                           top_k, groups, cap)
    assert np.array_equal(out["ad_ids"].cpu().numpy(), e_ids)
    assert np.array_equal(_bits(out["scores"][:n_tasks]), _bits(go.scores_at(table, e_slots)))
    return e_ids, e_slots


@pytest.mark.parametrize("B", [6, 36])                # 3000 rows: the column-split ranker; 18 000: the 128-row kernel
def test_pipeline_caps_the_answer_and_the_candidates(B):
    from tests.test_exclude_gpu import _rec, _users
    n_ads, top_k, k1 = 6000, 10, 500
    rec, user, nnum = _rec(n_ads)
    idx = rec.faiss_index
    rng = np.random.default_rng(9)
    groups = np.where(rng.random(n_ads) < 0.1, -1, rng.integers(0, 12, n_ads)).astype(np.int64)
    users = _users(user, B, 5)
    uc, un = rec.preprocess_batch(users)
    with pytest.raises(ValueError, match="without group keys"):
        rec.recommend_device(uc, un, top_k, k1, max_per_group=2)
    idx.set_groups(groups)
    plain = _clone(rec.recommend_device(uc, un, top_k, k1))
    cand_pos = plain["candidate_ids"].cpu().numpy()                          # default ids: an id is a position
    # stage 2: the cap inside the selection, both head modes bit for bit
    out = _clone(rec.recommend_device(uc, un, top_k, k1, max_per_group=2, heads="all"))
    assert torch.equal(out["candidate_ids"], plain["candidate_ids"]) and torch.equal(out["logits"], plain["logits"])
    e_ids, _ = _check_stage2(out, cand_pos, groups, top_k, 2)
    for row in e_ids:
        g = groups[row[row >= 0]]
        assert (np.bincount(g[g >= 0], minlength=1) <= 2).all()
    bites = any((np.bincount(g[g >= 0], minlength=1) > 2).any() for g in (groups[r] for r in plain["ad_ids"].cpu().numpy()))
    assert torch.equal(out["ad_ids"], plain["ad_ids"]) == (not bites)        # the cap changes an answer iff it has to
    first = _clone(rec.recommend_device(uc, un, top_k, k1, max_per_group=2, heads="ctr_first"))
    assert rec.heads_mode_effective("ctr_first") == ("ctr_first", None) and first["logits"].shape[0] == 1
    assert torch.equal(first["ad_ids"], out["ad_ids"]) and torch.equal(first["scores"], out["scores"])
    assert torch.equal(first["logits"][0], out["logits"][0])
    # stage 1: the cap on the candidate list = the rule over the index's own top 2 * k1
    emb = rec.two_tower_model.user_tower.encode(uc, un, check_indices=False, renormalize=True)
    pos1, sc1 = idx.search_device(emb, 2 * k1, normalize=False, return_positions=True)
    e_pos, e_sc = go.compact(pos1.cpu().numpy(), sc1.cpu().numpy(), groups, 3, k1, np.float32(-np.inf))
    assert ((e_pos >= 0).sum(axis=1) < k1).any()                             # 12 advertisers x 3: short candidate lists
    both = {}
    for heads in ("all", "ctr_first"):
        o = both[heads] = _clone(rec.recommend_device(uc, un, top_k, k1, max_per_group=2, stage1_max_per_group=3, heads=heads))
        assert np.array_equal(o["candidate_ids"].cpu().numpy(), np.where(e_pos >= 0, e_pos, n_ads - 1))
        assert np.array_equal(_bits(o["candidate_scores"]), _bits(e_sc))
        ids2, _ = _check_stage2(o, e_pos, groups, top_k, 2)
        assert all(set(r[r >= 0].tolist()) <= set(p[p >= 0].tolist()) for r, p in zip(ids2, e_pos))
    assert torch.equal(both["all"]["ad_ids"], both["ctr_first"]["ad_ids"])
    assert torch.equal(both["all"]["scores"], both["ctr_first"]["scores"])
    s1 = rec.recommend_device(uc, un, top_k, k1, stage1_max_per_group=3)      # the stage-1 cap alone
    assert np.array_equal(s1["candidate_ids"].cpu().numpy(), np.where(e_pos >= 0, e_pos, n_ads - 1))
    # a call without the new arguments launches what it launched before; with them, one launch each
    _lib.profile_enable(True)
    try:
        again = rec.recommend_device(uc, un, top_k, k1)
        rep = _lib.profile_report()
        assert not [t for t in rep if "cap" in t], rep.keys()
        _lib.profile_enable(True)
        rec.recommend_device(uc, un, top_k, k1, max_per_group=2, stage1_max_per_group=3)
        rep = _lib.profile_report()
        assert rep["select_topk_capped"]["launches"] == 1 and rep["group_cap_compact"]["launches"] == 1
    finally:
        _lib.profile_enable(False)
    assert torch.equal(again["ad_ids"], plain["ad_ids"]) and torch.equal(again["scores"], plain["scores"])
    # the reference API
    res = rec.batch_recommend(users, top_k, k1, max_per_group=2)
    assert [r["ad_ids"] for r in res] == out["ad_ids"].cpu().tolist()
    assert [r["scores"]["ctr"] for r in res] == out["scores"][0].cpu().tolist()
    assert rec.recommend_ads(users[1], top_k, k1, max_per_group=2)["ad_ids"] == out["ad_ids"][1].cpu().tolist()
    res = rec.batch_recommend(users, top_k, k1, max_per_group=2, stage1_max_per_group=3)
    assert [r["ad_ids"] for r in res] == both["all"]["ad_ids"].cpu().tolist()
    assert rec.recommend_tensors(uc, un, top_k, k1, max_per_group=2)[2]["ad_ids"] == out["ad_ids"][2].cpu().tolist()
    if B == 6:
        from amdrec.pipeline import TwoStageRetriever
        two = TwoStageRetriever(rec.two_tower_model, rec.transformer_ranker, idx)
        got = two.retrieve_and_rank(uc, un, k1, top_k, ad_features_lookup=rec.ad_features, max_per_group=2)
        assert got[0] == out["ad_ids"][0].cpu().tolist()
        cand, _ = two.retrieve_and_rank(uc, un, k1, top_k, stage1_max_per_group=3)      # no table: stage 1 alone
        with torch.no_grad():
            want, _ = idx.search_device(rec.two_tower_model.get_user_embeddings(uc, un), k1, max_per_group=3)
        assert cand == want[0].cpu().tolist() and cand != two.retrieve_and_rank(uc, un, k1, top_k)[0]
    # a captured graph: the caps are fixed at capture and replay to the eager result
    g = rec.capture(B, top_k, k1, max_per_group=2)
    r = g(uc, un)
    assert torch.equal(r["ad_ids"], out["ad_ids"]) and torch.equal(r["scores"], out["scores"])
    g = rec.capture(B, top_k, k1, max_per_group=2, stage1_max_per_group=3)
    r = g(uc, un)
    assert torch.equal(r["ad_ids"], both["all"]["ad_ids"]) and torch.equal(r["candidate_ids"], both["all"]["candidate_ids"])
    # live corpus: after remove_ads the caps follow the surviving rows' groups (ids are no longer positions)
    gone = np.unique(out["ad_ids"][:, :3].cpu().numpy().ravel())
    gone = gone[gone >= 0]
    keep = np.setdiff1d(np.arange(n_ads), gone)
    assert rec.remove_ads(gone.tolist()) == len(gone)
    assert np.array_equal(idx.get_groups().cpu().numpy(), groups[keep])
    after = _clone(rec.recommend_device(uc, un, top_k, k1, max_per_group=2))
    ids_c = after["candidate_ids"].cpu().numpy()
    pos_c = np.searchsorted(keep, ids_c)
    assert np.array_equal(keep[pos_c], ids_c) and not np.isin(ids_c, gone).any()
    a_ids, _ = _check_stage2(after, pos_c, groups[keep], top_k, 2)
    for row in a_ids:
        g_ = groups[row[row >= 0]]
        assert (np.bincount(g_[g_ >= 0], minlength=1) <= 2).all()
    rec.add_ads(np.random.default_rng(1).standard_normal((4, 256)).astype(np.float32), rec.ad_features[:4].cpu().numpy(),
                ad_ids=[n_ads, n_ads + 1, n_ads + 2, n_ads + 3], groups=[5, 5, -1, 11])
    assert idx.get_groups()[-4:].tolist() == [5, 5, -1, 11]
