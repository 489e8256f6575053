"""The diversified selection (amdrec.diversity) in float64, as a plain greedy loop, plus a WALK-ALONG checker for a device result.

fp32 similarities may differ from float64 ones by ``cases.SCORE_ATOL``, so two members whose values lie closer than that may
be picked in either order - and every later round depends on the pick.  The checker therefore follows the device's own picks:
at each round it rebuilds ``m`` from the device's earlier winners and asserts that the pick is an untaken pool member and
eps-optimal, ``v64[pick] >= max v64 - eps`` with ``eps = max(rel) * (lam * SCORE_ATOL + 4 * 2**-24)`` (the second term: the
two fp32 roundings of ``v``), and that the reported value is within eps of ``v64[pick]``.  A round is FORCED when the float64
runner-up is more than ``2 * eps`` behind; where every round of a user is forced the winners must equal the pure oracle's.
The tests assert that at least 95 % of their rounds are forced, so the tolerance cannot hide a wrong kernel.

The pool (relevance order, cap) comes from tests/group_cap_oracle.py's order and greedy loop."""
import math

import numpy as np

from tests import cases
from tests import group_cap_oracle as go

ROUNDING = 4 * 2.0 ** -24
MIN_FORCED = 0.95


def pool_slots(logits_row, pos_row, pool, group_of=None, cap=0):
    """One user's pool: the first ``pool`` accepted candidates in the selection's order."""
    order = go.select_order(logits_row, pos_row)
    if cap > 0:
        keep = go.greedy_keep([go.group_at(group_of, int(pos_row[s])) for s in order], cap)
        order = [s for s, ok in zip(order, keep) if ok]
    return order[:pool]


def gram64(rows, positions):
    """float64 inner products between the rows at ``positions``; a position beyond the array is a row of zeros (never read)."""
    n_rows, dim = rows.shape
    r = np.zeros((len(positions), dim), dtype=np.float64)
    for i, p in enumerate(positions):
        if p < n_rows:
            r[i] = rows[p]
    with np.errstate(invalid="ignore", over="ignore"):
        return r @ r.T


def epsilon(rel, lam):
    rel = np.asarray(rel, dtype=np.float64)
    top = float(np.nanmax(rel)) if rel.size and not np.isnan(rel).all() else 0.0
    return top * (lam * cases.SCORE_ATOL + ROUNDING)


def walk_user(logits_row, rel_row, pos_row, rows, lam, pool, top_k, group_of=None, cap=0, picks=None):
    """One user.  ``picks`` None: the pure oracle (arg-max, ties to the earlier member, NaN last).  ``picks`` = the device's
    winning slots [top_k]: follow them and assert each.  -> (slots [top_k], values [top_k], rounds, forced rounds, eps)."""
    lam = float(np.float32(lam))
    members = pool_slots(logits_row, pos_row, pool, group_of, cap)
    gram = gram64(rows, [int(pos_row[s]) for s in members])
    rel = np.asarray([rel_row[s] for s in members], dtype=np.float64)
    eps = epsilon(rel, lam)
    m = np.zeros(len(members))
    free = list(range(len(members)))
    slots, values = [-1] * top_k, [0.0] * top_k
    rounds = forced = 0
    for r in range(top_k):
        if not free:
            if picks is not None:
                assert all(int(s) == -1 for s in picks[r:]), f"rank {r}: the pool is used up, got slots {list(picks[r:])}"
            break
        v = rel * (1.0 - lam * m)
        finite = [i for i in free if not math.isnan(v[i])]
        if finite:
            best = max(finite, key=lambda i: (v[i], -i))
            rest = [v[i] for i in finite if i != best]
            is_forced = not rest or v[best] - max(rest) > 2 * eps
        else:
            best, is_forced = free[0], True                                 # only NaN values: the earliest member
        if picks is None:
            i = best
        else:
            assert int(picks[r]) in members, f"rank {r}: slot {int(picks[r])} is no pool member"
            i = members.index(int(picks[r]))
            assert i in free, f"rank {r}: slot {int(picks[r])} was taken before"
            if finite:
                assert not math.isnan(v[i]) and v[i] >= v[best] - eps, \
                    f"rank {r}: picked value {v[i]!r}, best {v[best]!r}, eps {eps!r}"
            else:
                assert i == best, f"rank {r}: among NaN values the earliest member wins"
        rounds += 1
        forced += int(is_forced)
        slots[r], values[r] = members[i], float(v[i])
        free.remove(i)
        for j in free:
            s = gram[j, i]
            if not math.isnan(s):
                m[j] = min(1.0, max(m[j], s))
    return slots, values, rounds, forced, eps


def select(rank_logits, rel, cand_pos, rows, lam, pool, top_k, group_of=None, cap=0):
    """The pure oracle for every user -> (slots int32 [n_users, top_k], values float64, rounds, forced rounds)."""
    n_users = cand_pos.shape[0]
    slots = np.full((n_users, top_k), -1, dtype=np.int32)
    values = np.zeros((n_users, top_k))
    rounds = forced = 0
    for u in range(n_users):
        s, v, n, f, _ = walk_user(rank_logits[u], rel[u], cand_pos[u], rows, lam, pool, top_k, group_of, cap)
        slots[u], values[u] = s, v
        rounds, forced = rounds + n, forced + f
    return slots, values, rounds, forced


def check(got_slots, got_values, rank_logits, rel, cand_pos, rows, lam, pool, top_k, group_of=None, cap=0, what=""):
    """Walk along a device result.  -> (rounds, forced rounds)."""
    n_users = cand_pos.shape[0]
    rounds = forced = 0
    for u in range(n_users):
        try:
            s, v, n, f, eps = walk_user(rank_logits[u], rel[u], cand_pos[u], rows, lam, pool, top_k, group_of, cap,
                                        picks=got_slots[u])
        except AssertionError as e:
            raise AssertionError(f"{what} user {u}: {e}") from None
        for r in range(top_k):
            g, w = float(got_values[u, r]), v[r]
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= eps, f"{what} user {u} rank {r}: value {g!r}, oracle {w!r}"
            if r >= n:
                assert g == 0.0 and int(got_slots[u, r]) == -1, f"{what} user {u} rank {r}: the tail reads slot -1, value 0.0"
        if n == f:                                                          # every round forced: the pure oracle's winners
            ps, _, _, _, _ = walk_user(rank_logits[u], rel[u], cand_pos[u], rows, lam, pool, top_k, group_of, cap)
            assert list(map(int, got_slots[u])) == ps, f"{what} user {u}: winners {list(got_slots[u])}, oracle {ps}"
        rounds, forced = rounds + n, forced + f
    return rounds, forced


# ---- the inputs of tests/test_diversity_gpu.py's direct-entry tests (built here so that tests/test_diversity_cpu.py can assert
# the forced share on them without a device) -----------------------------------------------------------------------------------
N_ROWS, N_TASKS = 4096, 3
K_CS = (1, 7, 64, 65, 128, 129, 500, 513, 2048)
# (top_k, pool or None for top_k, dim, n_users, extra row stride, lam): every top_k, pool, dim and user count of the issue
SHAPES = ((1, None, 4, 1, 0, 0.3), (10, 64, 256, 4, 0, 0.7), (32, 128, 60, 5, 3, 1.0), (33, None, 256, 5, 3, 0.3),
          (10, 128, 256, 1, 4, 1.0), (33, 64, 4, 4, 1, 0.7))

_corpora = {}


def corpus(dim, seed=5):
    """N_ROWS unit rows in 8 clusters (similarity ~0.8 inside a cluster, ~0 across), float32."""
    if (dim, seed) not in _corpora:
        rng = np.random.default_rng(seed + dim)
        centers = rng.standard_normal((8, dim)) / math.sqrt(dim)
        x = centers[rng.integers(0, 8, N_ROWS)] + 0.5 * rng.standard_normal((N_ROWS, dim)) / math.sqrt(dim)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        _corpora[(dim, seed)] = np.ascontiguousarray(x, dtype=np.float32)
    return _corpora[(dim, seed)]


def direct_inputs(n_users, k_c, seed):
    """Logits [3, n_users * k_c] = randn - 3 with a few NaNs, distinct positions per user with -1 holes, ids, group keys."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((N_TASKS, n_users * k_c)) - 3.0).astype(np.float32)
    logits[rng.random(logits.shape) < 0.01] = np.nan
    pos = np.stack([rng.permutation(N_ROWS)[:k_c] for _ in range(n_users)]).astype(np.int64)
    pos[rng.random(pos.shape) < 0.1] = -1
    ids = np.where(pos >= 0, pos * 3 + 1, 10 ** 6 + np.arange(k_c)[None])
    group_of = rng.choice(np.array([-1, 3, 1 << 33, 7, 11, 12], dtype=np.int64), size=N_ROWS)
    return logits, ids, pos, group_of


def direct_cases(k_c):
    """-> [(top_k, pool, dim, n_users, extra stride, lam, cap, seed)] for one k_c."""
    out = []
    for n, (top_k, pool, dim, n_users, extra, lam) in enumerate(SHAPES):
        out.append((top_k, top_k if pool is None else pool, dim, n_users, extra, lam, (0, 2, 3)[n % 3], 7000 + 10 * k_c + n))
    return out
