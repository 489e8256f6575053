"""The auction rule (amdrec.auction's docstring is the contract) restated as plain Python loops over one user at a time, in
``np.float32`` arithmetic.  It takes the per-slot probabilities as an INPUT - on the GPU tests those are the device's own,
produced by the CTR selection that predates the auction - so the only arithmetic here is one float32 multiply and one float32
division per value, and every comparison with the kernels is exact.  The kernels are compared with this, never with each other.
"""
import numpy as np

from tests import group_cap_oracle as go

F32 = np.float32
NAN = np.float32(np.nan)                                                # the canonical quiet NaN the entry reports
VALUES = np.array([-2.0, -0.0, 0.0, 0.5, 4.0], dtype=np.float32)        # five logits (the zeros tie): heavy ties
BIDS = np.array([0.0, 0.5, 1.0, 3.0], dtype=np.float32)
N_TASKS, N_ROWS = 3, 64
# reserves: none, 0 (drops the NaN eCPMs only), one that drops about half of the eCPMs of BIDS x sigmoid(VALUES), one that drops
# everything (the largest eCPM is 3 * sigmoid(4) < 3), and a per-user mix of them
RESERVE_KINDS = ("none", "zero", "half", "all", "mixed")
HALF, ALL = 0.45, 10.0


def sigmoid(x):
    """A numpy float32 sigmoid for the CPU-only checks (the GPU tests take the device's own probabilities instead)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (F32(1.0) / (F32(1.0) + np.exp(-np.asarray(x, dtype=F32)))).astype(F32)


def inputs(n_users, k_c, seed, n_rows=N_ROWS):
    """Logits [3, n_users * k_c] from five values with 8 % NaN, positions with 10 % holes, ids, bids from four values and group
    keys from three values plus -1 (as the cap tests draw them)."""
    rng = np.random.default_rng(seed)
    logits = rng.choice(VALUES, size=(N_TASKS, n_users * k_c))
    logits[rng.random(logits.shape) < 0.08] = np.nan
    pos = rng.integers(0, n_rows, size=(n_users, k_c)).astype(np.int64)
    pos[rng.random(pos.shape) < 0.1] = -1
    ids = np.where(pos >= 0, pos * 3 + 1, 10 ** 6 + np.arange(k_c)[None])     # (an unfilled slot's id is the caller's to choose)
    group_of = rng.choice(np.array([-1, 3, 1 << 33, 7], dtype=np.int64), size=n_rows)
    bid_of = rng.choice(BIDS, size=n_rows)
    return logits, ids, pos, group_of, bid_of


def reserve_for(kind, n_users):
    """The reserve argument of one case: None or float32 [n_users]."""
    if kind == "none":
        return None
    if kind == "mixed":
        return np.array([(0.0, HALF, ALL, 0.2)[u % 4] for u in range(n_users)], dtype=F32)
    return np.full(n_users, {"zero": 0.0, "half": HALF, "all": ALL}[kind], dtype=F32)


def bid_at(bid_of, n_bid_rows, pos):
    """The bid of corpus position ``pos`` >= 0: a position beyond the first ``n_bid_rows`` bids has 1.0 and is never read."""
    return F32(bid_of[pos]) if pos < n_bid_rows else F32(1.0)


def accepted(p_row, pos_row, bid_of, n_bid_rows, reserve_u, group_of, cap):
    """One user: -> (the accepted candidates' slots in the auction's order, e per slot, b per slot).  ``p_row``: float32
    probabilities of the ranking task per slot; ``reserve_u``: None or a float32; ``cap``: 0 / None = no cap."""
    k_c = len(p_row)
    e = np.zeros(k_c, dtype=F32)
    b = np.zeros(k_c, dtype=F32)
    cands = []
    for i in range(k_c):
        if pos_row[i] < 0:
            continue                                                     # no candidate
        b[i] = bid_at(bid_of, n_bid_rows, int(pos_row[i]))
        e[i] = F32(b[i]) * F32(p_row[i])                                 # one fp32 multiply
        if reserve_u is not None and not (e[i] >= F32(reserve_u)):
            continue                                                     # dropped: no candidate either
        cands.append(i)
    order = sorted(cands, key=lambda i: (1, 0.0, i) if np.isnan(e[i]) else (0, -float(e[i]), i))
    if cap:
        keep = go.greedy_keep([go.group_at(group_of, int(pos_row[s])) for s in order], cap)
        order = [s for s, ok in zip(order, keep) if ok]
    return order, e, b


def results(order, e, b, p_row, reserve_u, top_k):
    """One user's accepted order -> (slots int32 [top_k], ecpm float32 [top_k], price float32 [top_k], the runner-up's slot or
    -1): winners are the first top_k, rank r is priced by the candidate at rank r + 1."""
    slots = np.full(top_k, -1, dtype=np.int32)
    ecpm = np.zeros(top_k, dtype=F32)
    price = np.zeros(top_k, dtype=F32)
    for r, s in enumerate(order[:top_k]):
        slots[r] = s
        if np.isnan(e[s]):
            ecpm[r] = price[r] = NAN
            continue
        ecpm[r] = e[s]
        floor = F32(0.0)
        if r + 1 < len(order) and not np.isnan(e[order[r + 1]]):
            floor = e[order[r + 1]]
        if reserve_u is not None and F32(reserve_u) > floor:
            floor = F32(reserve_u)
        if floor == 0:
            continue                                                     # price 0.0
        with np.errstate(divide="ignore"):
            q = F32(floor) / F32(p_row[s])                               # the fp32 division
        price[r] = q if q < b[s] else b[s]
    return slots, ecpm, price, (order[top_k] if len(order) > top_k else -1)


def select_topk_auction(prob_rank, cand_ids, cand_pos, top_k, bid_of, n_bid_rows, reserve, group_of, cap):
    """amdrec_select_topk_auction for every user: ``prob_rank`` [n_users, k_c] -> (ids int64, slots int32, ecpm, price, each
    [n_users, top_k], runner-up slots [n_users])."""
    n_users, k_c = cand_pos.shape
    out_ids = np.full((n_users, top_k), -1, dtype=np.int64)
    out = [np.empty((n_users, top_k), dtype=t) for t in (np.int32, F32, F32)]
    runner = np.empty(n_users, dtype=np.int64)
    for u in range(n_users):
        rv = None if reserve is None else reserve[u]
        order, e, b = accepted(prob_rank[u], cand_pos[u], bid_of, n_bid_rows, rv, group_of, cap)
        out[0][u], out[1][u], out[2][u], runner[u] = results(order, e, b, prob_rank[u], rv, top_k)
        won = out[0][u][out[0][u] >= 0]
        out_ids[u, :len(won)] = cand_ids[u, won]
    return out_ids, out[0], out[1], out[2], runner
