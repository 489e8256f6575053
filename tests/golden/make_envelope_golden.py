#!/usr/bin/env python3
"""Generate the feature-envelope fixtures by running the REFERENCE modules on non-finite and out-of-range feature rows.

    python tests/golden/make_envelope_golden.py <reference directory> [case ...]

Calling convention and import rules of make_golden.py: ``two_tower_model.py`` and ``transformer_ranker.py`` are imported
from the given directory, the weights are drawn by this repo's seeded generator (amdrec.synth) exactly as make_golden.py
draws them for the same case, the eval-mode forward runs on CPU and only data is written:
``envelope_<case>.npz`` = one batch of 16 rows (tests/envelope.py families planted at PLANT_ROWS, ordinary rows between
them), the reference's user embeddings and its logits for both cross-weight scalings, and the sha256 of the weights.

What the fixtures pin: which rows the reference answers with NaN (a NaN or an infinity anywhere in a row's numerical
features: the whole row, in every embedding coordinate and every task) and that the scaled / tiny / zero rows stay finite.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-demo_amd"))
sys.path.insert(0, ROOT)
if len(sys.argv) < 2:
    sys.exit(f"usage: python {sys.argv[0]} <directory of the reference sources>")
sys.path.insert(0, os.path.abspath(sys.argv[1]))

from amdrec import synth  # noqa: E402
from tests import cases, envelope  # noqa: E402
import two_tower_model as ref_tt  # noqa: E402
import transformer_ranker as ref_rk  # noqa: E402

ENVELOPE_CASES = ("demo", "tutorial")
ROWS = 16
PLANT_ROWS = (0, 2, 3, 5, 6, 8, 9, 11, 12, 14)      # one row per family of envelope.FAMILIES, in that order


def to_torch(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def inputs(name):
    """The batch of a case (shared with tests/test_feature_envelope_cpu.py through the fixture, not through this code)."""
    dims_fn, _, seed = cases.CASES[name]
    user, ad, nnum = dims_fn()
    ucat, unum = synth.user_batch(user, nnum, ROWS, seed=seed + 400)
    acat = synth.ad_features(ad, ROWS, seed=seed + 500)
    unum, fam = envelope.bad_rows(unum, PLANT_ROWS)
    return ucat, unum, acat, fam


def main(only=None):
    torch.set_num_threads(1)
    torch.manual_seed(0)
    for name in ENVELOPE_CASES:
        if only and name not in only:
            continue
        user, ad, nnum, tt_sd, _ = cases.two_tower_case(name)
        arch = cases.arch(name)
        ucat, unum, acat, fam = inputs(name)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
        out = {"user_cat": ucat.astype(np.int16), "user_num": unum, "ad_cat": acat.astype(np.int16),
               "families": np.array(fam), "tt_weights_sha256": synth.state_sha256(tt_sd)}
        model = ref_tt.TwoTowerModel(dict(user), dict(ad), nnum, **arch["tt"])
        model.load_state_dict(to_torch(tt_sd))
        model.eval()
        with torch.no_grad():
            out["user_emb"] = model.get_user_embeddings(t(ucat), t(unum)).numpy()
        for cross in cases.CROSS:
            _, _, _, rk_sd, _ = cases.ranker_case(name, cross)
            model = ref_rk.TransformerRanker(dict(user), dict(ad), nnum, **arch["rk"])
            model.load_state_dict(to_torch(rk_sd))
            model.eval()
            with torch.no_grad():
                pred = model(t(ucat), t(acat), t(unum))
            assert list(pred.keys()) == ["ctr", "engagement", "revenue"]
            out[f"logits_{cross}"] = np.stack([pred[k].numpy().reshape(-1) for k in pred])
            out[f"rk_{cross}_weights_sha256"] = synth.state_sha256(rk_sd)
        np.savez_compressed(os.path.join(HERE, f"envelope_{name}.npz"), **out)
    print("envelope fixtures written to", HERE)


if __name__ == "__main__":
    main(sys.argv[2:])
