"""Reference-API latency: ms per recommend_ads call (one user) and per batch_recommend call (64 users) on the demo models over
100 000 ads, best-of-three loops, one JSON line.  TREE=<checkout> measures another tree's Python package (with AMDREC_LIB_PATH
for its library): how profiles/threads_streams_ab.log compares a commit with its parent."""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.environ.get("TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "movie-recommender-demo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from amdrec import synth  # noqa: E402
from amdrec.pipeline import AdRecommenderInference, Preprocessor, build_faiss_index  # noqa: E402
from amdrec.ranker import TransformerRanker  # noqa: E402
from amdrec.towers import TwoTowerModel  # noqa: E402

user, ad, nnum = synth.demo_dims()
t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}  # noqa: E731
tt = TwoTowerModel(dict(user), dict(ad), nnum)
tt.load_state_dict(t(synth.two_tower_state(user, ad, nnum, seed=3)))
rk = TransformerRanker(dict(user), dict(ad), nnum)
rk.load_state_dict(t(synth.ranker_state(user, ad, nnum, seed=4, cross_scale=1.0 / 16)))
table = synth.ad_features(ad, 100_000, seed=5)
rec = AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=build_faiss_index(tt, table, index_type="Flat"),
                             ad_features=table)
classes = {c: [f"cat_{j}" for j in range(card)] for c, card in user.items()}
rec.preprocessor = Preprocessor(classes, list(synth.NUM_COLS), np.full(nnum, 1.5), np.full(nnum, 0.7))
uc, un = synth.user_batch(user, nnum, 64, seed=6)
users = [{"categorical": {c: f"cat_{int(uc[b, i])}" for i, c in enumerate(user)},
          "numerical": {c: float(abs(un[b, i]) * 10) for i, c in enumerate(synth.NUM_COLS)}} for b in range(64)]
out = {"tree": os.path.basename(ROOT)}
for name, fn, n in (("recommend_ads_ms", lambda i: rec.recommend_ads(users[i % 64]), 3000),
                    ("batch_recommend_64_ms", lambda i: rec.batch_recommend(users), 500)):
    for i in range(200):
        fn(i)
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        best.append((time.perf_counter() - t0) * 1000 / n)
    out[name] = [round(x, 4) for x in best]
print(json.dumps(out), flush=True)
