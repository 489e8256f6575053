"""The diversified selection on the GPU.  ``amdrec_select_topk_diverse`` is walked along by the float64 oracle of
tests/diversity_oracle.py (every pick an untaken pool member and eps-optimal, every user whose rounds are all forced equal to
the pure oracle, at least 95 % of the rounds forced), is compared bit for bit with ``amdrec_select_topk`` /
``amdrec_select_topk_capped`` at ``lam == 0``, and is run over the edge data: duplicated rows, a NaN row, positions beyond the
row array in exact-size guarded buffers, a dominating group, a pool shorter than ``top_k``.  Then the serving pipeline: Flat and
IVF, both head modes, the cap, exclusion lists and masks, the captured graph, the reference API, the retriever and the live
corpus.  Without the new arguments nothing runs that did not run before."""
import numpy as np
import pytest
import torch

from amdrec import _lib
from tests import diversity_oracle as do
from tests import eligible_oracle as eo
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

N_TASKS = do.N_TASKS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rows_dev(rows_np, extra=0, n_rows=None):
    """The rows in an exact-size guarded buffer of [n_rows, dim + extra] floats; the padding columns hold NaN."""
    n_rows = rows_np.shape[0] if n_rows is None else n_rows
    dim = rows_np.shape[1]
    t = guarded((n_rows, dim + extra), torch.float32, "cuda", "output")         # (NaN everywhere)
    t[:, :dim] = _dev(rows_np[:n_rows])
    return t


def _select(entry, logits, ids, pos, top_k, mid=(), tail=(), n_tasks=N_TASKS, rank_task=0, slots=True):
    n_users, k_c = ids.shape
    out_ids = guarded((n_users, top_k), torch.int64, "cuda", "output")
    scores = guarded((n_tasks, n_users, top_k), torch.float32, "cuda", "output")
    out_slots = guarded((n_users, top_k), torch.int32, "cuda", "output") if slots else None
    extra = [guarded((n_users, top_k), torch.float32, "cuda", "output") for _ in range(1 if mid else 0)]
    _lib.check(entry(_lib.ptr(logits), logits.stride(0), n_tasks, rank_task, _lib.ptr(ids), _lib.ptr(pos), n_users, k_c, top_k,
                     *mid, _lib.ptr(out_ids), _lib.ptr(scores), _lib.ptr(out_slots), *[_lib.ptr(t) for t in extra], *tail,
                     _lib.stream_ptr("cuda")))
    outs = [out_ids, scores] + ([out_slots] if slots else []) + extra
    for t in outs:
        t.check()
    res = [out_ids.cpu().numpy(), scores.cpu().numpy(), out_slots.cpu().numpy() if slots else None]
    return res + [t.cpu().numpy() for t in extra]


def _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, group_of=None, cap=0, n_rows=None, **kw):
    """-> (ids, scores, slots, values); ``rows``: a 2-d device tensor whose row stride is its width."""
    n_rows = rows.shape[0] if n_rows is None else n_rows
    mid = (_lib.ptr(rows), n_rows, rows.shape[1], dim, lam, pool, _lib.ptr(group_of) if cap else None,
           group_of.shape[0] if cap else 0, cap)
    return _select(_lib.load().amdrec_select_topk_diverse, logits, ids, pos, top_k, mid, **kw)


def _prob_by_slot(logits, n_users, k_c, n_tasks=N_TASKS):
    """Every candidate's probabilities as the device writes them -> [n_tasks, n_users, k_c]."""
    ids = torch.zeros((n_users, k_c), dtype=torch.int64, device="cuda")
    _, sc, sl = _select(_lib.load().amdrec_select_topk, logits, ids, None, k_c, n_tasks=n_tasks)
    assert (np.sort(sl, axis=1) == np.arange(k_c)[None]).all()
    table = np.empty_like(sc)
    for u in range(n_users):
        table[:, u, sl[u]] = sc[:, u]
    return table


def _check_outputs(got, ids_np, table, n_tasks=N_TASKS):
    """ids and every task's probability follow from the winning slots as in amdrec_select_topk; tail -1 / 0.0."""
    g_ids, g_sc, g_sl, _ = got
    n_users, top_k = g_sl.shape
    for u in range(n_users):
        for r in range(top_k):
            s = g_sl[u, r]
            assert g_ids[u, r] == (ids_np[u, s] if s >= 0 else -1)
            want = table[:n_tasks, u, s] if s >= 0 else np.zeros(n_tasks, dtype=np.float32)
            assert np.array_equal(_bits(g_sc[:, u, r]), _bits(want))


@pytest.mark.parametrize("k_c", do.K_CS)
def test_direct_entry_against_the_walk_along_oracle(k_c):
    rounds = forced = 0
    for top_k, pool, dim, n_users, extra, lam, cap, seed in do.direct_cases(k_c):
        logits_np, ids_np, pos_np, groups_np = do.direct_inputs(n_users, k_c, seed)
        logits, ids, pos, group_of = _dev(logits_np), _dev(ids_np), _dev(pos_np), _dev(groups_np)
        rows_np = do.corpus(dim)
        rows = _rows_dev(rows_np, extra)
        table = _prob_by_slot(logits, n_users, k_c)
        what = f"k_c {k_c} top_k {top_k} pool {pool} dim {dim} users {n_users} lam {lam} cap {cap}"
        got = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, group_of, cap)
        rows.check()
        _check_outputs(got, ids_np, table)
        n, f = do.check(got[2], got[3], logits_np[0].reshape(n_users, k_c), table[0], pos_np, rows_np, lam, pool, top_k,
                        groups_np, cap, what)
        rounds, forced = rounds + n, forced + f
        # the rank-0 winner is the most relevant accepted candidate, and its value is its probability
        for u in range(n_users):
            members = do.pool_slots(logits_np[0].reshape(n_users, k_c)[u], pos_np[u], pool, groups_np, cap)
            assert got[2][u, 0] == (members[0] if members else -1)
            if members:
                assert np.array_equal(_bits(got[3][u, 0]), _bits(table[0, u, members[0]]))
        # without out_slots, and as the one-task call with slots (CTR-first's shape): the same winners and values
        bare = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, group_of, cap, slots=False)
        assert np.array_equal(bare[0], got[0]) and np.array_equal(_bits(bare[1]), _bits(got[1]))
        assert np.array_equal(_bits(bare[3]), _bits(got[3]))
        one = _diverse(logits[:1], ids, pos, top_k, rows, dim, lam, pool, group_of, cap, n_tasks=1)
        assert np.array_equal(one[0], got[0]) and np.array_equal(one[2], got[2])
        assert np.array_equal(_bits(one[1][0]), _bits(got[1][0])) and np.array_equal(_bits(one[3]), _bits(got[3]))
    # the ranking task is an argument
    got = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, group_of, cap, rank_task=2)
    n, f = do.check(got[2], got[3], logits_np[2].reshape(n_users, k_c), table[2], pos_np, rows_np, lam, pool, top_k, groups_np,
                    cap, "rank_task 2")
    rounds, forced = rounds + n, forced + f
    assert rounds and forced >= do.MIN_FORCED * rounds, (forced, rounds)


def _tied_inputs(n_users, k_c, seed):
    """Heavy ties, both zeros, NaN and +-inf logits, unfilled slots, and user 1 (if any) without a single candidate."""
    rng = np.random.default_rng(seed)
    values = np.array([-2.0, -0.0, 0.0, 0.5, 4.0, np.inf, -np.inf, 90.0, -90.0], dtype=np.float32)
    logits = rng.choice(values, size=(N_TASKS, n_users * k_c))
    logits[rng.random(logits.shape) < 0.08] = np.nan
    pos = rng.integers(0, do.N_ROWS, size=(n_users, k_c)).astype(np.int64)
    pos[rng.random(pos.shape) < 0.1] = -1
    if n_users > 1:
        pos[1] = -1
    ids = np.where(pos >= 0, pos * 3 + 1, 10 ** 6 + np.arange(k_c)[None])
    group_of = rng.choice(np.array([-1, 3, 1 << 33, 7], dtype=np.int64), size=do.N_ROWS)
    return logits, ids, pos, group_of


@pytest.mark.parametrize("k_c", do.K_CS)
def test_lam_zero_is_the_plain_and_the_capped_selection_bit_for_bit(k_c):
    lib = _lib.load()
    for n, (n_users, dim, extra) in enumerate(((1, 4, 0), (4, 60, 3), (5, 256, 0))):
        logits_np, ids_np, pos_np, groups_np = _tied_inputs(n_users, k_c, 50 * k_c + n)
        logits, ids, pos, group_of = _dev(logits_np), _dev(ids_np), _dev(pos_np), _dev(groups_np)
        rows = _rows_dev(do.corpus(dim), extra)
        for top_k in (1, 10, 32, 33):
            plain = _select(lib.amdrec_select_topk, logits, ids, pos, top_k)
            capped = _select(lib.amdrec_select_topk_capped, logits, ids, pos, top_k,
                             tail=(_lib.ptr(group_of), group_of.shape[0], 2))
            for pool in sorted({top_k, max(64, top_k), 128}):
                for want, cap in ((plain, 0), (capped, 2)):
                    got = _diverse(logits, ids, pos, top_k, rows, dim, 0.0, pool, group_of, cap)
                    what = f"k_c {k_c} users {n_users} top_k {top_k} pool {pool} cap {cap}"
                    assert np.array_equal(got[0], want[0]), f"ids {what}"
                    assert np.array_equal(got[2], want[2]), f"slots {what}"
                    assert np.array_equal(_bits(got[1]), _bits(want[1])), f"scores {what}"
                    assert np.array_equal(_bits(got[3]), _bits(want[1][0])), f"values {what}"      # v = rel * 1
        rows.check()


def test_duplicated_rows_at_lam_one_fall_behind_everything_dissimilar():
    """Every ad twice (the pool's rows are 16 distinct orthogonal unit rows, each held by two candidates): at lam = 1 the
    first 16 winners are one of each pair in relevance order, and only then the duplicates, whose value is exactly 0."""
    dim, k_c, top_k = 32, 32, 32
    rows_np = np.eye(dim, dtype=np.float32)[:16]
    rng = np.random.default_rng(4)
    logits_np = np.tile(np.sort(rng.standard_normal(k_c).astype(np.float32))[::-1], (N_TASKS, 1)).copy()
    pos_np = np.concatenate([rng.permutation(16), rng.permutation(16)])[None].astype(np.int64)
    ids_np = pos_np * 3 + 1
    logits, ids, pos = _dev(logits_np), _dev(ids_np), _dev(pos_np)
    table = _prob_by_slot(logits, 1, k_c)
    got = _diverse(logits, ids, pos, top_k, _rows_dev(rows_np), dim, 1.0, 32)
    first = {}
    for s in range(k_c):
        first.setdefault(int(pos_np[0, s]), s)
    firsts = sorted(first.values())
    assert got[2][0, :16].tolist() == firsts and got[2][0, 16:].tolist() == [s for s in range(k_c) if s not in firsts]
    assert np.array_equal(_bits(got[3][0, :16]), _bits(table[0, 0, firsts])) and (got[3][0, 16:] == 0.0).all()
    do.check(got[2], got[3], logits_np[0][None], table[0], pos_np, rows_np, 1.0, 32, top_k)
    # at lam = 0.5 a duplicate keeps half its probability
    half = _diverse(logits, ids, pos, top_k, _rows_dev(rows_np), dim, 0.5, 32)
    do.check(half[2], half[3], logits_np[0][None], table[0], pos_np, rows_np, 0.5, 32, top_k)
    dup = [r for r in range(top_k) if half[2][0, r] not in firsts]
    assert len(dup) == 16 and np.array_equal(_bits(half[3][0, dup]), _bits(table[0, 0, half[2][0, dup]] * np.float32(0.5)))


def test_a_nan_row_discounts_nothing_and_positions_beyond_the_rows_are_never_read():
    """50 rows in an exact-size guarded buffer, positions up to 100: a read past the end would see the guard band's bytes
    (one small positive float everywhere: a positive similarity between all such rows) and discount what must not be.  Row 7
    holds a NaN: similarity NaN, which leaves every m as it was."""
    n_rows, dim, k_c, top_k, n_users = 50, 60, 129, 33, 5
    rows_np = do.corpus(dim)[:n_rows].copy()
    rows_np[7, 3] = np.nan
    for extra in (0, 3):
        rows = _rows_dev(rows_np, extra)
        rng = np.random.default_rng(12 + extra)
        logits_np = (rng.standard_normal((N_TASKS, n_users * k_c)) - 3).astype(np.float32)
        pos_np = rng.integers(0, 2 * n_rows, size=(n_users, k_c)).astype(np.int64)
        pos_np[:, :3] = 7                                                    # the NaN row, three times per user
        logits_np[0].reshape(n_users, k_c)[:, 0] = 5.0                       # ... once as the clear rank-0 winner
        ids_np = pos_np * 3 + 1
        logits, ids, pos = _dev(logits_np), _dev(ids_np), _dev(pos_np)
        table = _prob_by_slot(logits, n_users, k_c)
        for lam, pool in ((1.0, 64), (0.7, 128)):
            got = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool)
            rows.check()
            n, f = do.check(got[2], got[3], logits_np[0].reshape(n_users, k_c), table[0], pos_np, rows_np, lam, pool, top_k)
            assert f >= do.MIN_FORCED * n
            assert (got[2][:, 0] == 0).all()
            far = pos_np[np.arange(n_users)[:, None], got[2]] >= n_rows
            assert far.any()                                                 # such candidates did win ...
            # ... at their undiscounted probability: similarity 0 to everything
            for u, r in zip(*np.nonzero(far)):
                assert np.array_equal(_bits(got[3][u, r]), _bits(table[0, u, got[2][u, r]]))
            for u in range(n_users):                                         # and so did the NaN row's other holders
                for r in range(top_k):
                    if got[2][u, r] in (1, 2):
                        assert np.array_equal(_bits(got[3][u, r]), _bits(table[0, u, got[2][u, r]]))
    # no rows at all: every similarity is 0, the result is the plain order
    none = _diverse(logits, ids, pos, top_k, rows, dim, 1.0, 64, n_rows=0)
    plain = _select(_lib.load().amdrec_select_topk, logits, ids, pos, top_k)
    assert np.array_equal(none[2], plain[2]) and np.array_equal(_bits(none[3]), _bits(plain[1][0]))


@pytest.mark.parametrize("k_c,top_k", [(65, 10), (500, 10), (500, 33), (2048, 32)])
def test_a_dominating_group_ungrouped_keys_and_the_short_tail(k_c, top_k):
    """One group holds the best 80 % of the relevance order: under cap c the pool holds c of its ads and whatever else there
    is.  With every ad in ONE group and cap 3 the pool is 3 ads: the tail past them reads -1 / 0.0.  Ungrouped keys: no cap."""
    n_users, dim, lam, pool = 5, 256, 0.7, 64
    rows_np = do.corpus(dim)
    rows = _rows_dev(rows_np)
    logits_np, ids_np, pos_np, _ = do.direct_inputs(n_users, k_c, 900 + k_c)
    groups_np = np.full(do.N_ROWS, 5, dtype=np.int64)
    rank = logits_np[0].reshape(n_users, k_c)
    for u in range(n_users):                                                 # the worst fifth of each user: other groups
        worst = np.argsort(np.nan_to_num(rank[u], nan=-np.inf))[:max(k_c // 5, 1)]
        groups_np[pos_np[u, worst][pos_np[u, worst] >= 0]] = np.arange(len(worst))[pos_np[u, worst] >= 0] % 4 + 10
    logits, ids, pos = _dev(logits_np), _dev(ids_np), _dev(pos_np)
    table = _prob_by_slot(logits, n_users, k_c)
    for cap in (1, 3):
        got = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, _dev(groups_np), cap)
        _check_outputs(got, ids_np, table)
        do.check(got[2], got[3], rank, table[0], pos_np, rows_np, lam, pool, top_k, groups_np, cap, f"cap {cap}")
        for u in range(n_users):
            g = groups_np[pos_np[u, got[2][u][got[2][u] >= 0]]]
            assert (np.bincount(g, minlength=1) <= cap).all()
    one = np.full(do.N_ROWS, 1 << 40, dtype=np.int64)
    got = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, _dev(one), 3)
    do.check(got[2], got[3], rank, table[0], pos_np, rows_np, lam, pool, top_k, one, 3, "one group")
    assert (got[0][:, :min(3, top_k)] >= 0).all() and (got[0][:, 3:] == -1).all() and (got[2][:, 3:] == -1).all()
    assert (got[1][:, :, 3:] == 0.0).all() and (got[3][:, 3:] == 0.0).all()
    free = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool, _dev(np.full(do.N_ROWS, -5, dtype=np.int64)), 1)
    none = _diverse(logits, ids, pos, top_k, rows, dim, lam, pool)
    assert np.array_equal(free[2], none[2]) and np.array_equal(_bits(free[3]), _bits(none[3]))


# ---- the serving pipeline --------------------------------------------------------------------------------------------------
def _clone(out):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _check_call(out, cand_pos, rows_np, top_k, lam, pool, groups=None, cap=0):
    """One recommend_device result against the walk-along oracle over that call's own logits and candidates."""
    B, k1 = cand_pos.shape
    logits = out["logits"]
    table = _prob_by_slot(logits, B, k1, n_tasks=logits.shape[0])
    rank = logits[0].view(B, k1).cpu().numpy()
    ids = out["ad_ids"].cpu().numpy()
    cand_ids = out["candidate_ids"].cpu().numpy()
    slots = np.full((B, top_k), -1, dtype=np.int32)
    for u in range(B):                                                       # the real ads of a row are distinct: id -> slot
        where = {int(cand_ids[u, s]): s for s in range(k1) if cand_pos[u, s] >= 0}
        for r in range(top_k):
            if ids[u, r] >= 0:
                slots[u, r] = where[int(ids[u, r])]
    values = out["diversity_values"].cpu().numpy()
    assert values.shape == (B, top_k) and values.dtype == np.float32
    n, f = do.check(slots, values, rank, table[0], cand_pos, rows_np, lam, pool, top_k, groups, cap)
    want = np.where(slots >= 0, np.take_along_axis(table[0], np.maximum(slots, 0), 1), 0)
    assert np.array_equal(_bits(out["scores"][0]), _bits(want))
    return slots, n, f


@pytest.mark.parametrize("B", [1, 12])
@pytest.mark.parametrize("index_type", ["Flat", "IVF"])
def test_pipeline_diversifies_the_answer(index_type, B):
    from tests.test_exclude_gpu import _rec, _users
    n_ads, top_k, k1, lam = 6000, 10, 500, 0.7
    rec, user, nnum = _rec(n_ads, index_type=index_type)
    idx = rec.faiss_index
    rng = np.random.default_rng(9)
    groups = np.where(rng.random(n_ads) < 0.1, -1, rng.integers(0, 12, n_ads)).astype(np.int64)
    idx.set_groups(groups)
    users = _users(user, B, 5)
    uc, un = rec.preprocess_batch(users)
    rows_np = idx._xb[:n_ads].cpu().numpy()
    plain = _clone(rec.recommend_device(uc, un, top_k, k1))
    assert "diversity_values" not in plain
    cand_pos = plain["candidate_ids"].cpu().numpy().copy()                   # default ids: an id is a position ...
    filled = np.isfinite(plain["candidate_scores"].cpu().numpy())
    cand_pos[~filled] = -1                                                   # ... and an unfilled slot is told by its score
    rounds = forced = 0
    for pool, cap in ((64, None), (128, None), (64, 2)):
        kw = dict(diversity=lam, diversity_pool=pool, max_per_group=cap)
        out = _clone(rec.recommend_device(uc, un, top_k, k1, heads="all", **kw))
        assert torch.equal(out["candidate_ids"], plain["candidate_ids"]) and torch.equal(out["logits"], plain["logits"])
        slots, n, f = _check_call(out, cand_pos, rows_np, top_k, lam, pool, groups, cap or 0)
        rounds, forced = rounds + n, forced + f
        first = _clone(rec.recommend_device(uc, un, top_k, k1, heads="ctr_first", **kw))
        assert rec.heads_mode_effective("ctr_first") == ("ctr_first", None) and first["logits"].shape[0] == 1
        for key in ("ad_ids", "scores", "diversity_values"):
            assert torch.equal(first[key], out[key]), key
        if cap:
            for row in out["ad_ids"].cpu().numpy():
                g = groups[row[row >= 0]]
                assert (np.bincount(g[g >= 0], minlength=1) <= cap).all()
    assert forced >= do.MIN_FORCED * rounds, (forced, rounds)
    out = _clone(rec.recommend_device(uc, un, top_k, k1, diversity=lam))     # (the default pool, 64: the first case above)
    # lam = 0 is the plain answer, and the values are the CTR probabilities
    zero = rec.recommend_device(uc, un, top_k, k1, diversity=0.0)
    assert torch.equal(zero["ad_ids"], plain["ad_ids"]) and torch.equal(zero["scores"], plain["scores"])
    assert torch.equal(zero["diversity_values"], plain["scores"][0])
    # with an exclusion list (and masks, Flat) in stage 1: the rule over the filtered candidates
    excl = plain["ad_ids"][:, :4].contiguous()
    kw = dict(exclude_ad_ids=excl)
    if index_type == "Flat":
        idx.set_tags(eo.tags_for(n_ads, 5))
        ma, my = (_dev(w.view(np.int64)) for w in eo.masks_for(B))
        kw.update(require_all=ma, require_any=my)
    base = _clone(rec.recommend_device(uc, un, top_k, k1, **kw))
    filt = _clone(rec.recommend_device(uc, un, top_k, k1, diversity=lam, **kw))
    assert torch.equal(filt["candidate_ids"], base["candidate_ids"])
    pos_f = base["candidate_ids"].cpu().numpy().copy()
    pos_f[~np.isfinite(base["candidate_scores"].cpu().numpy())] = -1
    _check_call(filt, pos_f, rows_np, top_k, lam, 64)
    for row, gone in zip(filt["ad_ids"].cpu().numpy(), excl.cpu().numpy()):
        assert not np.isin(row, gone[gone >= 0]).any()                       # (an exclusion list is per user)
    # a call without the new arguments launches what it launched before; with them, one launch of the new kernel
    _lib.profile_enable(True)
    try:
        again = rec.recommend_device(uc, un, top_k, k1)
        rep = _lib.profile_report()
        assert not [t for t in rep if "diverse" in t], rep.keys()
        _lib.profile_enable(True)
        rec.recommend_device(uc, un, top_k, k1, diversity=lam, max_per_group=2)
        rep = _lib.profile_report()
        assert rep["select_topk_diverse"]["launches"] == 1 and "select_topk_capped" not in rep
    finally:
        _lib.profile_enable(False)
    assert torch.equal(again["ad_ids"], plain["ad_ids"]) and torch.equal(again["scores"], plain["scores"])
    # the reference API and the retriever return the device result
    res = rec.batch_recommend(users, top_k, k1, diversity=lam)
    assert [r["ad_ids"] for r in res] == out["ad_ids"].cpu().tolist()
    assert [r["scores"]["ctr"] for r in res] == out["scores"][0].cpu().tolist()
    assert [r["diversity_values"] for r in res] == out["diversity_values"].cpu().tolist()
    assert "diversity_values" not in rec.batch_recommend(users, top_k, k1)[0]
    one = rec.recommend_ads(users[0], top_k, k1, diversity=lam)
    assert one["ad_ids"] == out["ad_ids"][0].cpu().tolist() and one["diversity_values"] == out["diversity_values"][0].cpu().tolist()
    assert rec.recommend_tensors(uc, un, top_k, k1, diversity=lam)[B - 1]["ad_ids"] == out["ad_ids"][B - 1].cpu().tolist()
    if B == 1:
        from amdrec.pipeline import TwoStageRetriever
        two = TwoStageRetriever(rec.two_tower_model, rec.transformer_ranker, idx)
        got = two.retrieve_and_rank(uc, un, k1, top_k, ad_features_lookup=rec.ad_features, diversity=lam)
        assert got[0] == out["ad_ids"][0].cpu().tolist() and got[1] == out["scores"][0, 0].cpu().tolist()
    # a captured graph: lam and the pool are fixed at capture and replay to the eager result
    capped = _clone(rec.recommend_device(uc, un, top_k, k1, diversity=lam, diversity_pool=128, max_per_group=2))
    g = rec.capture(B, top_k, k1, diversity=lam, diversity_pool=128, max_per_group=2)
    r = g(uc, un)
    for key in ("ad_ids", "scores", "diversity_values"):
        assert torch.equal(r[key], capped[key]), key
    # live corpus: after remove_ads the call reads the compacted rows (ids are no longer positions)
    gone = np.unique(out["ad_ids"][:, :3].cpu().numpy().ravel())
    gone = gone[gone >= 0]
    keep = np.setdiff1d(np.arange(n_ads), gone)
    assert rec.remove_ads(gone.tolist()) == len(gone)
    after = _clone(rec.recommend_device(uc, un, top_k, k1, diversity=lam))
    ids_c = after["candidate_ids"].cpu().numpy()
    pos_c = np.searchsorted(keep, ids_c)
    assert np.array_equal(keep[pos_c], ids_c) and not np.isin(ids_c, gone).any()
    pos_c[~np.isfinite(after["candidate_scores"].cpu().numpy())] = -1
    assert np.array_equal(idx._xb[:len(keep)].cpu().numpy(), rows_np[keep])
    _check_call(after, pos_c, rows_np[keep], top_k, lam, 64)
