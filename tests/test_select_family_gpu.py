"""The stage-2 selection family agrees WITH ITSELF at the dispatch boundaries.  ``amdrec_select_topk``,
``amdrec_select_topk_capped`` and ``amdrec_select_topk_auction`` are instantiations of one kernel frame (csrc/select.hip); the
neighbouring tests compare each with its oracle, this one compares the variants with each other where the rules say they must
coincide, bit for bit on ids, every score plane and slots (and on eCPMs and prices between the two auction calls):

* the plain selection == the capped one over ungrouped rows (group -1 is never capped) == the capped one over a single group
  with cap = k_c, which never binds;
* the auction without a cap == the auction with ``max_per_group = k_c`` over a single group;
* ``cand_pos = NULL`` == ``cand_pos = arange`` where every slot is filled.

Shapes: the keys-per-lane switch (128 / 129), the wave / sort switch on both conditions (512 / 513 candidates, top_k 32 / 33)
and the largest sort; 1, 4 and 5 users: a lone wave, a full workgroup, a partial one.  The CPU test shows with the plain loops of
tests/group_cap_oracle.py and tests/auction_oracle.py that the compared pairs are equal by the rules themselves, on the same
inputs."""
import functools

import numpy as np
import pytest
import torch

from amdrec import _lib
from tests import auction_oracle as ao
from tests import group_cap_oracle as go

F32 = np.float32
SHAPES = [(1, 1), (64, 32), (128, 32), (129, 32), (512, 32), (513, 32), (40, 33), (2048, 7)]
USERS = (1, 4, 5)
N_TASKS = 3
VALUES = np.array([-2.0, -0.0, 0.0, 0.5, 4.0], dtype=F32)               # five logits (the zeros tie): ties broken by slot
HUGE = F32(3e38)                                                        # under every unfilled slot: must never be seen
RESERVES = (None, 0.45)                                                 # 0.45 drops about half of BIDS x sigmoid(VALUES)


@functools.lru_cache(maxsize=None)
def _inputs(k_c, top_k):
    """Five users; the first n of them serve a case of n users.  Per user: logits of five repeated values in every plane, two
    NaN logits in the ranking plane, about a fifth of the slots unfilled (position -1) under a huge logit.  User 1 has fewer
    than top_k real candidates, user 3 none.  Filled positions are a permutation of the slots (k_c corpus rows).
    -> (logits [3, 5, k_c], ids [5, k_c], pos [5, k_c], bids [k_c]), numpy."""
    rng = np.random.default_rng(1000 * k_c + top_k)
    n = max(USERS)
    logits = rng.choice(VALUES, size=(N_TASKS, n, k_c))
    pos = np.stack([rng.permutation(k_c) for _ in range(n)]).astype(np.int64)
    for u in range(n):
        logits[0, u, rng.choice(k_c, size=min(2, k_c), replace=False)] = np.nan
    pos[rng.random(pos.shape) < 0.2] = -1
    pos[0, 0] = max(pos[0, 0], 0)                                       # user 0 has a candidate at every shape
    few = rng.choice(k_c, size=min(top_k, k_c) // 2, replace=False)     # user 1: fewer than top_k real candidates
    keep = pos[1, few]
    pos[1] = -1
    pos[1, few] = np.where(keep >= 0, keep, few)
    pos[3] = -1                                                         # user 3: none
    logits[:, pos < 0] = HUGE
    ids = np.where(pos >= 0, pos * 3 + 1, 10 ** 6 + np.arange(k_c)[None])
    bids = rng.choice(ao.BIDS, size=k_c)
    return logits, ids, pos, bids


def _case(k_c, top_k, n_users):
    logits, ids, pos, bids = _inputs(k_c, top_k)
    return np.ascontiguousarray(logits[:, :n_users]).reshape(N_TASKS, -1), ids[:n_users], pos[:n_users], bids


def _reserve(rv, n_users):
    return None if rv is None else np.full(n_users, rv, dtype=F32)


# ---- CPU: the compared pairs are equal by the rules ---------------------------------------------------------------------
@pytest.mark.parametrize("k_c,top_k", SHAPES)
def test_the_compared_variants_are_equal_by_the_rules_themselves(k_c, top_k):
    n = max(USERS)
    logits, ids, pos, bids = _case(k_c, top_k, n)
    rank = logits[0].reshape(n, k_c)
    assert np.isnan(rank[pos >= 0]).any() or k_c == 1                    # NaN candidates, ties, unfilled slots, short users
    assert (pos < 0).any() and (pos[3] < 0).all() and 0 < (pos[0] >= 0).sum()
    assert (pos[1] >= 0).sum() == min(top_k, k_c) // 2 < top_k
    ungrouped, one_group = np.full(k_c, -1, dtype=np.int64), np.zeros(k_c, dtype=np.int64)
    # the plain selection by its definition: the first top_k of the visiting order
    plain_slots = np.full((n, top_k), -1, dtype=np.int32)
    for u in range(n):
        won = go.select_order(rank[u], pos[u])[:top_k]
        plain_slots[u, :len(won)] = won
        assert all(rank[u, s] != HUGE for s in won)
    if k_c > 1:
        tied = [rank[u, plain_slots[u][plain_slots[u] >= 0]] for u in range(n)]
        assert any((np.diff(t[~np.isnan(t)]) == 0).any() for t in tied)  # winners do tie: the slot decides
    for group_of, cap in ((ungrouped, 1), (one_group, k_c)):
        e_ids, e_slots = go.select_topk_capped(rank, ids, pos, top_k, group_of, cap)
        assert np.array_equal(e_slots, plain_slots)
        assert np.array_equal(e_ids, np.where(plain_slots >= 0, np.take_along_axis(ids, np.maximum(plain_slots, 0).astype(np.int64), 1), -1))
    prob = ao.sigmoid(rank)
    for rv in RESERVES:
        free = ao.select_topk_auction(prob, ids, pos, top_k, bids, k_c, _reserve(rv, n), None, 0)
        bound = ao.select_topk_auction(prob, ids, pos, top_k, bids, k_c, _reserve(rv, n), one_group, k_c)
        assert all(np.array_equal(a.view(np.int32) if a.dtype == F32 else a, b.view(np.int32) if b.dtype == F32 else b)
                   for a, b in zip(free, bound))
    # no positions (every slot a candidate) against positions 0 .. k_c - 1
    dense = logits[0].reshape(n, k_c).copy()
    dense[dense == HUGE] = F32(0.5)
    for u in range(n):
        assert go.select_order(dense[u], np.zeros(k_c, dtype=np.int64)) == go.select_order(dense[u], np.arange(k_c))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    from tests.test_group_cap_gpu import _bits
    assert len(a) == len(b)
    for name, x, y in zip(("ids", "scores", "slots", "ecpm", "price"), a, b):
        if x.dtype == F32:
            x, y = _bits(x), _bits(y)
        assert np.array_equal(x, y), f"{name}: {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("n_users", USERS)
@pytest.mark.parametrize("k_c,top_k", SHAPES)
def test_plain_capped_and_auction_agree_where_the_cap_cannot_bind(k_c, top_k, n_users):
    from tests.test_auction_gpu import _auction
    from tests.test_group_cap_gpu import _capped, _dev, _select
    logits_np, ids_np, pos_np, bids_np = _case(k_c, top_k, n_users)
    logits, ids, pos, bids = _dev(logits_np), _dev(ids_np), _dev(pos_np), _dev(bids_np)
    ungrouped = torch.full((k_c,), -1, dtype=torch.int64, device="cuda")
    one_group = torch.zeros(k_c, dtype=torch.int64, device="cuda")
    what = f"k_c {k_c} top_k {top_k} users {n_users}"
    plain = _select(_lib.load().amdrec_select_topk, logits, ids, pos, top_k)
    # ... which is the definition's selection (the rest of this test compares kernels with each other)
    rank = logits_np[0].reshape(n_users, k_c)
    for u in range(n_users):
        won = go.select_order(rank[u], pos_np[u])[:top_k]
        assert plain[2][u].tolist() == won + [-1] * (top_k - len(won)), what
    _same(plain, _capped(logits, ids, pos, top_k, ungrouped, 1), f"ungrouped, cap 1, {what}")
    _same(plain, _capped(logits, ids, pos, top_k, one_group, k_c), f"one group, cap k_c, {what}")
    for rv in RESERVES:
        reserve = None if rv is None else _dev(_reserve(rv, n_users))
        free = _auction(logits, ids, pos, top_k, bids, reserve)
        _same(free, _auction(logits, ids, pos, top_k, bids, reserve, one_group, k_c), f"auction, reserve {rv}, {what}")
        assert np.array_equal(free[2] >= 0, free[0] >= 0) and (rv is not None or np.array_equal(free[2] >= 0, plain[2] >= 0))


@pytest.mark.gpu
@pytest.mark.parametrize("k_c,top_k", [(128, 32), (513, 32)])                  # one wave shape, one sort shape
def test_plain_selection_without_positions_is_the_one_with_every_slot_filled(k_c, top_k):
    from tests.test_group_cap_gpu import _dev, _select
    n_users = max(USERS)
    logits_np, ids_np, _, _ = _case(k_c, top_k, n_users)
    logits_np = np.where(logits_np == HUGE, F32(0.5), logits_np)
    logits, ids = _dev(logits_np), _dev(ids_np)
    arange = _dev(np.tile(np.arange(k_c, dtype=np.int64), (n_users, 1)))
    entry = _lib.load().amdrec_select_topk
    got = _select(entry, logits, ids, None, top_k)
    assert (got[2] >= 0).all()
    _same(got, _select(entry, logits, ids, arange, top_k), f"k_c {k_c} top_k {top_k}")
