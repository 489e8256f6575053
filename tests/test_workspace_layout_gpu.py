"""GPU: a workspace of exactly the queried size is enough, and nothing outside it is touched.

Each case runs once through the normal binding (the shared grow-only workspace) and once with ``GuardedArena`` installed
in its place: every workspace the binding asks for is then served at EXACTLY the requested size, from a 256-byte-aligned
offset inside a larger uint8 tensor with 4 KiB guard bands on both sides, its interior pre-filled with 0xA5 (an entry
that read a sub-buffer it had not initialised would compute from that pattern).  The bindings hand ``ws.numel()`` to the
C entry, so the entry sees exactly the queried byte count.  After a synchronise both guards are unchanged and the outputs
are ``torch.equal`` to the first run's.  The test looks only at bytes it owns."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cases
from tests.guarded import GuardedArena, both_ways

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def corpora(dev):
    """dim -> (fp32 rows, bf16 shadow, max norm) of 9000 unit rows: above CAND_CAP, so the sample buffers are live."""
    from amdrec import _lib, synth
    lib = _lib.load()
    out = {}
    for d in (64, 72):
        X = torch.from_numpy(synth.unit_corpus(9000, d, seed=5 + d)).to(dev)
        X16 = torch.empty((9000, d), dtype=torch.bfloat16, device=dev)
        mx = torch.zeros(2, dtype=torch.float32, device=dev)
        _lib.check(lib.amdrec_bf16_rows(_lib.ptr(X), 9000, d, d, _lib.ptr(X16), d, _lib.ptr(mx), _lib.stream_ptr(dev)))
        out[d] = (X, X16, mx)
    return out


# dim 64: the streaming scan, 72: the generic tiles; nq 1 / 9: tau inside the scan or not, 40: the 64-query tile,
# 129: past FUSED_MAX_NQ (the unfused finalize)
@pytest.mark.parametrize("nq", [1, 9, 40, 129])
@pytest.mark.parametrize("dim", [64, 72])
@pytest.mark.parametrize("engine", ["fp32", "mixed"])
def test_flat_search_in_an_exact_workspace(dev, corpora, engine, dim, nq):
    from amdrec import synth
    from amdrec.index import flat_search, flat_search_mixed
    X, X16, mx = corpora[dim]
    Q = torch.from_numpy(synth.unit_corpus(nq, dim, seed=100 + nq)).to(dev)

    def run():
        D = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        I = torch.empty((nq, 10), dtype=torch.int64, device=dev)    # noqa: E741
        nf = torch.zeros(1, dtype=torch.int32, device=dev)
        if engine == "fp32":
            flat_search(X, 9000, Q, 10, D, I, n_fixup=nf)
        else:
            flat_search_mixed(X, X16, mx, 9000, Q, 10, D, I, n_fixup=nf)
        return D, I, nf
    arena = both_ways(run)
    from amdrec import _lib
    n = C.c_size_t(0)
    if engine == "fp32":
        _lib.check(_lib.load().amdrec_flat_search_workspace(nq, 9000, 10, C.byref(n)))
    else:
        _lib.check(_lib.load().amdrec_flat_search_mixed_workspace(nq, 9000, 10, dim, C.byref(n)))
    assert [s[2] for s in arena.served] == [n.value]


def test_kmeans_steps_in_an_exact_workspace(dev):
    from amdrec import synth
    from amdrec.ivf import InvertedLists
    x = torch.from_numpy(synth.unit_corpus(3000, 64, seed=41)).to(dev)
    both_ways(lambda: (InvertedLists.train(x, 16).centroids,))


def test_ivf_group_in_an_exact_workspace(dev):
    """3000 rows in 16 lists, 40 queries x 4 probes: cnt | rank at exactly the bytes the entry states it needs."""
    from amdrec import _lib
    lib = _lib.load()
    nq, nprobe, nlist = 40, 4, 16
    rng = np.random.default_rng(3)
    probes = torch.from_numpy(np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)).to(dev)
    lens = torch.from_numpy(rng.multinomial(3000, np.full(nlist, 1 / nlist)).astype(np.int64)).to(dev)
    need = 256 * -(-4 * (nlist + 1) // 256) + 256 * -(-4 * nq * nprobe // 256)

    def run(ws):
        base = torch.zeros((nq, nprobe), dtype=torch.int64, device=dev)
        count = torch.zeros(nq, dtype=torch.int64, device=dev)
        pq, pp = (torch.zeros(nq * nprobe, dtype=torch.int64, device=dev) for _ in range(2))
        goff, qtp = (torch.zeros(nlist + 1, dtype=torch.int64, device=dev) for _ in range(2))
        _lib.check(lib.amdrec_ivf_group(_lib.ptr(probes), nprobe, nq, nprobe, nlist, _lib.ptr(lens), _lib.ptr(base),
                                        _lib.ptr(count), _lib.ptr(pq), _lib.ptr(pp), _lib.ptr(goff), _lib.ptr(qtp), 32,
                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        # the order of the pairs inside a list's group is unspecified (include/amdrec.h): compare them as sorted (q, p) per group
        torch.cuda.synchronize()
        g = goff.cpu().numpy()
        pairs = torch.stack([pq, pp], 1).cpu().numpy()
        groups = np.concatenate([np.array(sorted(map(tuple, pairs[g[i]:g[i + 1]])), dtype=np.int64).reshape(-1, 2)
                                 for i in range(nlist)])
        return base, count, goff, qtp, torch.from_numpy(groups)
    want = run(torch.empty(need + 4096, dtype=torch.uint8, device=dev))
    arena = GuardedArena()
    got = run(arena.get(need, dev))
    arena.check()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    short = arena.get(need - 1, dev)
    with pytest.raises(_lib.AmdrecError, match=f"need {need} bytes, got {need - 1}"):
        run(short)


def _models(dev):
    from amdrec.ranker import TransformerRanker
    from amdrec.towers import TwoTowerModel
    user, ad, nnum, sd, _ = cases.two_tower_case("demo")
    tt = TwoTowerModel(dict(user), dict(ad), nnum)
    tt.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    rk = TransformerRanker(dict(user), dict(ad), nnum)
    rk.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return tt.to(dev).eval(), rk.to(dev).eval(), user, ad, nnum


def test_tower_forward_in_an_exact_workspace(dev):
    """5000 rows: above the one-launch path, so both ping-pong buffers carry the hidden layers."""
    from amdrec import synth
    tt, _, _, ad, _ = _models(dev)
    ad_cat = torch.from_numpy(synth.ad_features(ad, 5000, seed=8)).to(dev)
    both_ways(lambda: (tt.get_ad_embeddings(ad_cat),))


def test_ranker_forward_in_an_exact_workspace(dev):
    """300 rows (3 users x 100 candidates) on the strict fp32 engine: X, T, X0, H and the hoisted user rows U all in use."""
    from amdrec import synth
    _, rk, user, ad, nnum = _models(dev)
    rk.gemm_engine = "fp32"
    table = torch.from_numpy(synth.ad_features(ad, 2000, seed=9)).to(dev)
    uc, un = synth.user_batch(user, nnum, 3, seed=10)
    uc, un = torch.from_numpy(uc).to(dev), torch.from_numpy(un).to(dev)
    cand = torch.from_numpy(np.random.default_rng(11).integers(0, 2000, (3, 100))).to(dev)
    both_ways(lambda: (rk.score_candidates(uc, un, cand, table, raw=True)[1],))
