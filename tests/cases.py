"""Shared case definitions for the golden fixtures (mirrors tests/golden/make_golden.py)."""
from collections import OrderedDict

from amdrec import synth


def small_dims():
    cards = synth.CRITEO_SYNTH_CARDS
    user = OrderedDict((c, min(cards[i], 174 + 7 * i)) for i, c in enumerate(synth.USER_COLS))
    ad = OrderedDict((c, min(cards[6 + i], 97 + 13 * i)) for i, c in enumerate(synth.AD_COLS))
    return user, ad, 13


CASES = {
    "demo": (synth.demo_dims, (1, 7, 64), 11),
    "ragged": (small_dims, (3, 33), 12),
    # the reference's second usage example (tutorial.ipynb cells 10, 19): NOT the default architecture
    "tutorial": (small_dims, (1, 7, 64), 13),
    # two points of the constructor surface below (towers "single_linear" with ranker "narrow"; towers "eight_layers" with
    # ranker "x3_one_layer"), pinned to the reference's own outputs
    "narrow": (small_dims, (1, 7, 64), 14),
    "x3_one_layer": (small_dims, (1, 7, 64), 15),
}
# constructor arguments that differ from the reference's defaults (two_tower_model.py:193-201, transformer_ranker.py:213-224)
# and, for the ranker, the expected x3_fallback_reason() (None: the row-owner engine runs)
ARCH = {
    "tutorial": {"tt": dict(embedding_dim=16, hidden_dims=[256, 128], output_dim=128),
                 "rk": dict(embedding_dim=16, d_model=128, num_heads=4, num_layers=2, d_ff=512),
                 "x3_reason": "d_model 128 != 256"},
    "narrow": {"tt": dict(embedding_dim=16, hidden_dims=[], output_dim=64),
               "rk": dict(embedding_dim=4, d_model=100, num_heads=4, num_layers=2, d_ff=300),
               "x3_reason": "d_model 100 != 256"},
    "x3_one_layer": {"tt": dict(embedding_dim=4, hidden_dims=[36] * 7, output_dim=4),
                     "rk": dict(embedding_dim=8, d_model=256, num_heads=8, num_layers=1, d_ff=96),
                     "x3_reason": None},
}


def arch(name):
    return ARCH.get(name, {"tt": {}, "rk": {}, "x3_reason": None})


def x3_reason(name):
    """The x3_fallback_reason() a golden case's ranker must report (None: the row-owner engine runs)."""
    return arch(name)["x3_reason"]


CROSS = {"randn": 1.0, "scaled": 1.0 / 16}

# Parity tolerances, stated once and used by every parity test:
EMB_ATOL = 1e-5          # unit-norm tower embeddings, absolute
LOGIT_RTOL = 1e-4        # ranker logits: |d| <= LOGIT_RTOL * max(1, |logit|)
SCORE_ATOL = 1e-6        # inner-product scores of unit vectors, absolute
TOPK_TAU = 1e-5          # near-tie band at the k-th score


def two_tower_case(name):
    dims_fn, batches, seed = CASES[name]
    user, ad, nnum = dims_fn()
    sd = synth.two_tower_state(user, ad, nnum, seed=seed, **arch(name)["tt"])
    return user, ad, nnum, sd, batches


def ranker_case(name, cross):
    dims_fn, batches, seed = CASES[name]
    user, ad, nnum = dims_fn()
    sd = synth.ranker_state(user, ad, nnum, seed=seed + 1, cross_scale=CROSS[cross], **arch(name)["rk"])
    return user, ad, nnum, sd, batches


LOGIT_SCALE_RTOL = 1e-5  # randn fixtures only: ... or |d| <= LOGIT_SCALE_RTOL * max|logit| over the batch
LOGIT_STRICT_RTOL = 1e-5  # scaled fixtures (the benchmark's weights): |d| <= 1e-5 * max(1, |logit|), 10x inside SURVEY 8a


def logit_scale(ref_dict):
    """Largest |logit| over the batch and over all tasks (the heads share one trunk, whose
    magnitude sets the fp32 rounding noise of every head)."""
    import numpy as np
    return max(float(np.abs(np.asarray(v)).max()) if np.asarray(v).size else 0.0 for v in ref_dict.values())


def logit_close(got, ref, cross="randn", scale=None):
    """Ranker-logit tolerance, by conditioning of the network:

    * ``cross == "scaled"`` (cross weights randn/16: logits O(1), the weights bench.py uses): the STRICT rule alone,
      |d| <= LOGIT_STRICT_RTOL * max(1, |logit|) = 1e-5 - ten times tighter than SURVEY 8a's 1e-4; two fp32
      evaluations of this network sit ~1e-6 apart (measured: oracle vs reference golden 0.6-0.9e-6).
    * ``cross == "randn"`` (the reference's default unscaled randn(256,256) cross weights,
      transformer_ranker.py:177-184: logits ~1e3 out of three 16x-amplifying layers, heads cancel): the reference's
      OWN torch fp32 output is up to 4.4e-4 relative away from float64 truth per element while staying within 2.5e-6
      of the batch's logit scale, so an element passes if it is within SURVEY 8a's 1e-4 * max(1,|logit|) OR within
      LOGIT_SCALE_RTOL of the largest |logit| of the batch (``scale``, over all tasks).
    -> (ok, max err/bound)"""
    import numpy as np
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if cross == "scaled":
        bound = LOGIT_STRICT_RTOL * np.maximum(1.0, np.abs(ref))
    else:
        if scale is None:
            scale = float(np.abs(ref).max()) if ref.size else 0.0
        bound = np.maximum(LOGIT_RTOL * np.maximum(1.0, np.abs(ref)), LOGIT_SCALE_RTOL * scale)
    err = np.abs(got - ref)
    return bool((err <= bound).all()), float((err / bound).max()) if ref.size else 0.0


# ---- the constructor surface the HIP code accepts (csrc/layers.hip ranker_check / tower_check, amdrec/weights.py
# x3_ineligible_reason), one entry per edge.  Feature dims are small_dims() (6 user + 20 ad columns), so the ranker's
# projection K is 26 E + n_num, the user tower's K0 is 6 E + n_num and the ad tower's K0 is 20 E.
# ranker: name -> (TransformerRanker arguments, numerical_dim, expected x3_fallback_reason(), what it targets)
RANKER_SURFACE = {
    "x3_one_layer": (dict(embedding_dim=8, d_model=256, num_heads=8, num_layers=1, d_ff=96), 13, None,
                     "row-owner with a 2 + 3 + 1 phase list; d_ff % 128 != 0: no column-split kernel at <= 4096 rows"),
    "x3_no_encoder": (dict(embedding_dim=32, d_model=256, num_heads=8, num_layers=0, d_ff=1024), 13, None,
                      "phase list of the three crosses + heads only"),
    "x3_param_edge": (dict(embedding_dim=32, d_model=256, num_heads=8, num_layers=3, d_ff=1568), 13, None,
                      "n_par 11244 rounds to exactly X3_PARAM_FLOATS = 11264: the last eligible d_ff at 3 layers"),
    "past_param_edge": (dict(embedding_dim=32, d_model=256, num_heads=8, num_layers=3, d_ff=1600), 13,
                        "11340 bias / LayerNorm parameters exceed the kernel's LDS parameter area (11264)",
                        "first d_ff past the LDS parameter area; x6 fc1 with nout 1600 (partial 256 tile) above 8192 rows"),
    "x3_five_layers": (dict(embedding_dim=16, d_model=256, num_heads=8, num_layers=5, d_ff=32), 13, None,
                       "last eligible layer count at d_ff 32 (one hidden tile per FFN)"),
    "six_layers": (dict(embedding_dim=16, d_model=256, num_heads=8, num_layers=6, d_ff=32), 13,
                   "11340 bias / LayerNorm parameters exceed the kernel's LDS parameter area (11264)",
                   "first layer count past the LDS parameter area; fc2 on x6 with K = 32"),
    "narrow": (dict(embedding_dim=4, d_model=100, num_heads=4, num_layers=2, d_ff=300), 13, "d_model 100 != 256",
               "LayerNorm / cross epilogues at a width that is not a multiple of 32; x6 partial tile for fc1"),
    "minimal": (dict(embedding_dim=4, d_model=4, num_heads=1, num_layers=1, d_ff=4), 13, "d_model 4 != 256",
                "smallest legal widths through the wide (no-narrow) epilogues"),
    "wide_embed": (dict(embedding_dim=64, d_model=252, num_heads=4, num_layers=2, d_ff=1024), 13, "d_model 252 != 256",
                   "projection K = 1677; d_model 4 short of a full tile; user / ad split projection"),
    "no_numerical": (dict(embedding_dim=32, d_model=256, num_heads=8, num_layers=3, d_ff=1024), 0, None,
                     "default architecture with n_num = 0 (null numerical pointer)"),
}
# towers: name -> (TwoTowerModel arguments, numerical_dim, what it targets)
TOWER_SURFACE = {
    "single_linear": (dict(embedding_dim=16, hidden_dims=[], output_dim=64), 13,
                      "hidden_dims=[]: the gather loader straight into the L2-norm epilogue (ad tower always, user "
                      "tower past 4096 rows; below, the fused 16-row kernel with one layer)"),
    "ts_width_edge": (dict(embedding_dim=16, hidden_dims=[1024, 48], output_dim=32), 13,
                      "user tower: a width of exactly TS_MAX_WIDTH and narrow widths in the fused 16-row kernel"),
    "past_ts_width": (dict(embedding_dim=16, hidden_dims=[1040], output_dim=100), 13,
                      "a width past TS_MAX_WIDTH: tiled GEMMs at every row count; partial L2-norm tile"),
    "wide_embed": (dict(embedding_dim=64, hidden_dims=[512, 256], output_dim=256), 13,
                   "default widths at K0 = 397 / 1280: not the pipelined kernel"),
    "eight_layers": (dict(embedding_dim=4, hidden_dims=[36] * 7, output_dim=4), 13,
                     "MAX_LAYERS exactly; 4-wide output"),
    "no_numerical": (dict(embedding_dim=16, hidden_dims=[512, 256], output_dim=256), 0,
                     "user tower with a null numerical pointer"),
}


def surface_ranker_case(name, cross="scaled", seed=71):
    args, nnum, _, _ = RANKER_SURFACE[name]
    user, ad, _ = small_dims()
    sd = synth.ranker_state(user, ad, nnum, seed=seed, cross_scale=CROSS[cross], **args)
    return user, ad, nnum, sd


def surface_tower_case(name, seed=73):
    args, nnum, _ = TOWER_SURFACE[name]
    user, ad, _ = small_dims()
    sd = synth.two_tower_state(user, ad, nnum, seed=seed, **args)
    return user, ad, nnum, sd


# the golden cases "narrow" / "x3_one_layer" are points of these tables
assert ARCH["narrow"]["tt"] == TOWER_SURFACE["single_linear"][0] and ARCH["narrow"]["rk"] == RANKER_SURFACE["narrow"][0]
assert ARCH["x3_one_layer"]["tt"] == TOWER_SURFACE["eight_layers"][0]
assert ARCH["x3_one_layer"]["rk"] == RANKER_SURFACE["x3_one_layer"][0]
