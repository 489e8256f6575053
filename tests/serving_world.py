"""The serving world shared by tests/test_threads_gpu.py and tests/test_side_stream_gpu.py: the demo models over a 3000-ad
Flat corpus that holds tags, groups, bids and boosts, a preprocessor for the dict API, seeded users, and fresh twins of the
recommender built the same way (the pattern of tests/coherence.py).  torch and amdrec are imported here: GPU tests only."""
import numpy as np
import torch

from amdrec import synth
from tests import coherence

N_ADS = 3000


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


class World:
    """The demo models over a 3000-ad Flat corpus that holds tags, groups, bids and boosts, and its dict-API users."""

    def __init__(self):
        from amdrec.pipeline import Preprocessor
        self.user, self.ad, self.nnum = synth.demo_dims()
        self.tt_sd = synth.two_tower_state(self.user, self.ad, self.nnum, seed=201)
        self.rk_sd = synth.ranker_state(self.user, self.ad, self.nnum, seed=202, cross_scale=1.0 / 16)
        self.table = synth.ad_features(self.ad, N_ADS, seed=203)
        self.tags, self.groups, self.bids = coherence.row_attrs(204, N_ADS)[:3]
        self.boosts = np.random.default_rng(205).uniform(-0.2, 0.2, N_ADS).astype(np.float32)
        classes = {c: [f"cat_{j}" for j in range(card)] for c, card in self.user.items()}
        self.pp = Preprocessor(classes, list(synth.NUM_COLS), np.full(self.nnum, 1.5), np.full(self.nnum, 0.7))
        self.rec, self.tower = self.build()

    def modules(self):
        from amdrec.ranker import TransformerRanker
        from amdrec.towers import TwoTowerModel
        tt = TwoTowerModel(dict(self.user), dict(self.ad), self.nnum)
        tt.load_state_dict(_t(self.tt_sd))
        rk = TransformerRanker(dict(self.user), dict(self.ad), self.nnum)
        rk.load_state_dict(_t(self.rk_sd))
        return tt, rk

    def index(self, tower):
        from amdrec.pipeline import build_faiss_index
        idx = build_faiss_index(tower, self.table, index_type="Flat")
        idx.set_tags(self.tags)
        idx.set_groups(self.groups)
        idx.set_bids(self.bids)
        idx.set_boosts(self.boosts)
        return idx

    def build(self, index_tower=None):
        """-> (a new recommender, the tower that made its corpus).  ``index_tower``: make the corpus with this (already
        used) tower and give the recommender modules that have never run."""
        from amdrec.pipeline import AdRecommenderInference
        tt, rk = self.modules()
        src = tt if index_tower is None else index_tower
        rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=self.index(src),
                                     ad_features=self.table, preprocessor=self.pp)
        return rec, src

    def dict_users(self, n, seed):
        uc, un = synth.user_batch(self.user, self.nnum, n, seed=seed)
        return [{"categorical": {c: f"cat_{int(uc[b, i])}" for i, c in enumerate(self.user)},
                 "numerical": {c: float(abs(un[b, i]) * 10) for i, c in enumerate(synth.NUM_COLS)}} for b in range(n)]

    def tensor_users(self, n, seed, device=None):
        uc, un = synth.user_batch(self.user, self.nnum, n, seed=seed)
        uc, un = torch.from_numpy(uc), torch.from_numpy(un)
        return (uc, un) if device is None else (uc.to(device), un.to(device))
