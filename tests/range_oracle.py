"""The stage-2 selection family over the whole float32 logit range: a float64 sigmoid, an ulp measure, the rule the reported
probability must obey, a deterministic logit sweep and banded cap / auction inputs whose probabilities saturate, underflow and
pass through the denormals.  Helpers only - no GPU, no library.

The probability rule (``prob_rule``), for p = 1 / (1 + expf(-x)) in float32 with an expf of at most 1 ulp:
* NaN -> NaN; x = +-0 -> 0.5 exactly.
* x >= 17.5 (and +inf) -> the bits of 1.0f: e^-x < 2^-25, so 1 + e rounds to 1.
* ``exp(-x) >= FLT_MAX * (1 + 2^-22)`` (every x <= -89, and -inf) -> the bits of +0.0f: an expf within 1 ulp (2^-23 relative)
  of a value that far above FLT_MAX is +inf, and 1 / (1 + inf) = +0.
* ``exp(-x) <= FLT_MAX * (1 - 2^-22)`` (every other x >= -88.72) -> within 4 ulp of the float64 sigmoid: one expf at <= 2^-23
  relative, one add and one divide at 2^-24 each, < 2^-22 relative = 4 ulp of the result; below FLT_MIN the ulp is the denormal
  spacing 2^-149 and the division underflows gradually (the build passes no flush-to-zero flag).
* In the sliver between the two (|x + 88.7228| < 3e-7, a handful of bit patterns) expf may or may not overflow: either answer.
``FLUSHES_DENORMALS`` is the one switch for a device whose division flushed denormal results: it is False, because it does not.
"""
import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
ULP_BOUND = 4.0
ONE_AT, ZERO_AT = 17.5, -89.0            # x >= ONE_AT -> 1.0f, x <= ZERO_AT -> +0.0f (round figures past the two thresholds)
FLUSHES_DENORMALS = False                # True would mirror a device that returned +0.0 for every denormal result
_MARGIN = 2.0 ** -22                     # > the 1-ulp relative error of expf

WINDOW = 4096
WINDOW_CENTRES = (17.33, -17.33, -87.34, -88.72, -103.97)
SPECIALS = (np.inf, -np.inf, FLT_MAX, -FLT_MAX, 1e3, -1e3, FLT_MIN, -FLT_MIN, np.nan)


def sigmoid_f64(x):
    """float64 1 / (1 + exp(-x)), as exp(x) / (1 + exp(x)) for x < 0: no overflow, no cancellation.  NaN stays NaN."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        neg = x < 0
        e = np.exp(np.where(neg, x, -x))                                  # exp(-|x|) in (0, 1]
        return np.where(neg, e / (1.0 + e), 1.0 / (1.0 + e))


def sigmoid64(x):
    """The float64 sigmoid rounded ONCE to float32; gradual underflow is kept (float32 denormals come out)."""
    with np.errstate(under="ignore"):
        p = sigmoid_f64(x).astype(F32)
    if FLUSHES_DENORMALS:
        p = np.where(np.abs(p) < F32(FLT_MIN), F32(0.0), p)
    return p


def ulp_err(got_f32, want_f64):
    """|got - want| in units of np.spacing of the float32-rounded ``want`` (2^-149 below FLT_MIN)."""
    want = np.asarray(want_f64, dtype=np.float64)
    with np.errstate(under="ignore", invalid="ignore"):
        unit = np.spacing(np.abs(want.astype(F32))).astype(np.float64)
        return np.abs(np.asarray(got_f32, dtype=np.float64) - want) / unit


def regions(x):
    """-> dict of boolean masks over ``x`` (float32): how ``prob_rule`` treats each logit."""
    x = np.asarray(x, dtype=F32)
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.exp(-x64)                                                  # what expf(-x) approximates
    nan = np.isnan(x)
    zero = x == 0
    one = x64 >= ONE_AT
    flush = ~nan & (t >= FLT_MAX * (1.0 + _MARGIN))
    either = ~nan & ~flush & (t > FLT_MAX * (1.0 - _MARGIN))
    bounded = ~(nan | zero | one | flush | either)
    assert flush[x64 <= ZERO_AT].all() and not flush[x64 >= -88.72].any()
    with np.errstate(invalid="ignore"):
        denorm = bounded & (sigmoid_f64(x64) < FLT_MIN)
        near_one = bounded & (x64 > 15.0)
    return dict(nan=nan, zero=zero, one=one, flush=flush, either=either, bounded=bounded, denormal=denorm, near_one=near_one,
                normal=bounded & ~denorm & ~near_one)


def prob_rule(x, got):
    """The rule of this module's docstring for reported probabilities ``got`` (float32) of logits ``x`` (float32), elementwise.
    -> (ok bool array, ulp array: the error where the 4-ulp bound applies, 0 elsewhere, regions dict)."""
    x = np.asarray(x, dtype=F32)
    got = np.ascontiguousarray(got, dtype=F32)
    assert x.shape == got.shape
    bits = got.view(np.int32)
    r = regions(x)
    with np.errstate(invalid="ignore"):
        ulps = np.where(r["bounded"] | r["either"], ulp_err(got, sigmoid_f64(x)), 0.0)
    within = ulps <= ULP_BOUND
    ok = np.where(r["nan"], np.isnan(got),
         np.where(r["zero"], bits == F32(0.5).view(np.int32),
         np.where(r["one"], bits == F32(1.0).view(np.int32),
         np.where(r["flush"], bits == 0,
         np.where(r["either"], (bits == 0) | within, within)))))          # noqa: E128
    return ok, np.where(r["bounded"], ulps, 0.0), r


def assert_prob_rule(x, got, what=""):
    """Assert ``prob_rule`` everywhere; -> (ulps, regions) for the caller's records."""
    ok, ulps, r = prob_rule(x, got)
    if not ok.all():
        bad = np.flatnonzero(~ok.ravel())[:8]
        xs, gs = np.asarray(x, dtype=F32).ravel()[bad], np.asarray(got, dtype=F32).ravel()[bad]
        rows = [(float(a), float(b), float(sigmoid_f64(a)), float(u)) for a, b, u in zip(xs, gs, ulp_err(gs, sigmoid_f64(xs)))]
        raise AssertionError(f"{what}: {int((~ok).sum())} probabilities break the rule, e.g. (x, got, float64 sigmoid, ulps) {rows}")
    return ulps, r


def _window(centre):
    b = int(F32(centre).view(np.int32))
    return (np.arange(b - WINDOW // 2, b + WINDOW // 2, dtype=np.int64).astype(np.uint32)).view(F32)


def sweep():
    """The deterministic float32 logit set (about 69k values, duplicates kept): 4096 consecutive bit patterns around each of
    +-17.33 (1 - p reaches half an ulp of 1), -87.34 (p reaches FLT_MIN), -88.72 (expf overflows), -103.97 (the true sigmoid
    reaches half of 2^-149) and the 4096 patterns from +0 / -0 on (zero and the smallest denormal logits); 16 patterns either
    side of 0; denormal logits of either sign across their range; linspace(-110, 30, 40000); the specials."""
    parts = [_window(c) for c in WINDOW_CENTRES]
    parts.append(np.arange(0, WINDOW, dtype=np.uint32).view(F32))                          # +0 and up
    parts.append((np.arange(0, WINDOW, dtype=np.uint32) | np.uint32(1 << 31)).view(F32))   # -0 and down
    near = np.arange(0, 17, dtype=np.uint32)
    parts += [near.view(F32), (near | np.uint32(1 << 31)).view(F32)]
    den = (np.uint32(1) << np.arange(0, 23, dtype=np.uint32)) | np.uint32(1)               # 2^-149 ... just below FLT_MIN
    den = np.concatenate([den, np.array([0x007FFFFF, 0x00400000, 0x000ABCDE], dtype=np.uint32)])
    parts += [den.view(F32), (den | np.uint32(1 << 31)).view(F32)]
    parts.append(np.linspace(-110.0, 30.0, 40000).astype(F32))
    parts.append(np.array(SPECIALS, dtype=F32))
    return np.concatenate(parts).astype(F32)


# ---- banded cap / auction inputs -----------------------------------------------------------------------------------------
INF = np.inf
LOGIT_BANDS = {
    "sat_hi": [17, 17.5, 30, 1e3, 3e38, INF],
    "sat_lo": [-INF, -3e38, -1e3, -104, -89],
    "denorm": [-88.5, -88.25, -88, -87.75, -87.5, -87.4],
    "tail": [-87, -60, -30, -17, -16],
    "half": [0.0, -0.0, 1e-40, -1e-40, 1e-8, -1e-8],
    "edge1": [15, 16, 16.5, 16.75, 17, 17.25],
}
LOGIT_BANDS["mixed"] = [v for band in list(LOGIT_BANDS.values()) for v in band]
BID_BANDS = {
    "unit": [1],
    "small": [1e-45, 1e-40, 1e-30],
    "plain": [0, .5, 1, 3],
    "huge": [1e30, 3e38],
}
BID_BANDS["all"] = [v for band in list(BID_BANDS.values()) for v in band]
N_TASKS = 3
N_BAND_USERS = len(LOGIT_BANDS) * len(BID_BANDS)                         # 7 x 5 = 35
GROUP_KEYS = np.array([-1, 3, 1 << 33, 7], dtype=np.int64)
SHAPES = ((100, 10), (500, 32), (700, 33))                               # (k_c, top_k): both wave variants, the sort kernels
RESERVES = {"none": None, "zero": 0.0, "denormal": 1e-42, "tiny": 1e-20}
CAPS = (0, 2)


def band_of(u):
    """User u's (logit band name, bid band name)."""
    return list(LOGIT_BANDS)[u // len(BID_BANDS)], list(BID_BANDS)[u % len(BID_BANDS)]


def banded_inputs(k_c, seed):
    """One user per (logit band x bid band), 35 users.  User u owns corpus positions [u * k_c, (u + 1) * k_c), so its candidates'
    bids come from its bid band alone.  -> (logits float32 [3, 35 * k_c] with 3 % NaN, ids, pos int64 [35, k_c] with 10 % of
    the positions -1, group_of int64 [35 * k_c], bid_of float32 [35 * k_c])."""
    rng = np.random.default_rng(seed)
    n_users = N_BAND_USERS
    n_rows = n_users * k_c
    logits = np.empty((N_TASKS, n_users, k_c), dtype=F32)
    bid_of = np.empty(n_rows, dtype=F32)
    pos = np.empty((n_users, k_c), dtype=np.int64)
    for u in range(n_users):
        lb, bb = band_of(u)
        logits[:, u] = rng.choice(np.array(LOGIT_BANDS[lb], dtype=F32), size=(N_TASKS, k_c))
        bid_of[u * k_c:(u + 1) * k_c] = rng.choice(np.array(BID_BANDS[bb], dtype=F32), size=k_c)
        pos[u] = u * k_c + rng.integers(0, k_c, size=k_c)
    logits = logits.reshape(N_TASKS, n_users * k_c)
    logits[rng.random(logits.shape) < 0.03] = np.nan
    pos[rng.random(pos.shape) < 0.1] = -1
    ids = np.where(pos >= 0, pos * 3 + 1, 10 ** 6 + np.arange(k_c)[None])
    group_of = rng.choice(GROUP_KEYS, size=n_rows)
    return logits, ids, pos, group_of, bid_of


def seed_for(k_c):
    """One seed for all three shapes, picked on the CPU (tests/test_select_range_cpu.py) so that every class of ``CLASSES`` has
    winners at each of them: a denormal price needs a capped user whose accepted list runs out of its 1e-30 bids inside top_k."""
    return 6


def reserve_array(kind, n_users):
    """None or float32 [n_users]; "mixed" cycles through all four and +inf (which drops everything)."""
    if kind == "mixed":
        return np.array([(0.0, 1e-42, INF, 1e-20, 0.25)[u % 5] for u in range(n_users)], dtype=F32)
    v = RESERVES[kind]
    return None if v is None else np.full(n_users, v, dtype=F32)


CLASSES = ("ecpm_denormal", "ecpm_zero", "ecpm_huge", "p_zero", "p_denormal", "priced_at_bid_by_the_clamp", "price_denormal")


def class_counts(prob_rank, cand_pos, want, bid_of, reserve):
    """What one oracle result (``auction_oracle.select_topk_auction``'s tuple ``want``) exercised, counted over its winners with
    a non-NaN eCPM: a denormal eCPM, eCPM exactly 0, eCPM > 1e30, p = 0, p denormal, a denormal price - and winners of
    denormal p whose quotient floor / p reached their bid, so that the price is the bid by the ``min``.  (The quotient itself
    cannot overflow inside the bid domain: floor <= e = fl(b * p), so floor / p <= b * (1 + 2^-23) <= FLT_MAX.  The count of
    infinite quotients is returned too, as ``quotient_inf``, and must be 0.)"""
    slots, ecpm, price = want[1], want[2], want[3]
    n_users, top_k = slots.shape
    out = dict.fromkeys(CLASSES + ("quotient_inf",), 0)
    tiny = F32(FLT_MIN)
    for u in range(n_users):
        for r in range(top_k):
            s = slots[u, r]
            if s < 0 or np.isnan(ecpm[u, r]):
                continue
            p, e, q = F32(prob_rank[u, s]), ecpm[u, r], price[u, r]
            b = F32(bid_of[cand_pos[u, s]])
            out["ecpm_denormal"] += int(0 < e < tiny)
            out["ecpm_zero"] += int(e == 0)
            out["ecpm_huge"] += int(e > 1e30)
            out["p_zero"] += int(p == 0)
            out["p_denormal"] += int(0 < p < tiny)
            out["price_denormal"] += int(0 < q < tiny)
            if 0 < p < tiny and q == b and b > 0:
                floor = F32(0.0)
                if r + 1 < top_k and slots[u, r + 1] >= 0 and not np.isnan(ecpm[u, r + 1]):
                    floor = ecpm[u, r + 1]
                elif r + 1 == top_k and want[4][u] >= 0:                  # the runner-up prices the last winner
                    nxt = F32(bid_of[cand_pos[u, want[4][u]]]) * F32(prob_rank[u, want[4][u]])
                    floor = F32(0.0) if np.isnan(nxt) else nxt
                if reserve is not None and F32(reserve[u]) > floor:
                    floor = F32(reserve[u])
                if floor > 0:
                    with np.errstate(over="ignore"):
                        quotient = F32(floor) / p
                    out["priced_at_bid_by_the_clamp"] += int(quotient >= b)
                    out["quotient_inf"] += int(np.isinf(quotient))
    return out
