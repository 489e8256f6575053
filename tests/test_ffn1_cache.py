"""CPU: the first-FFN hidden cache (weights.first_ffn_cache, TransformerRanker.cache_first_ffn).  With layer 1's attention
folded into the projection the chain starts with x1 = LN1(z), z = a_ad + u_user, and stage 1 of layer 1's FFN is
W_1 x1 + b_1 = rstd * (P[ad] + Q[user]) + c - checked here in float64, together with the packing: the third stream is the
16-row stream minus exactly layer 1's stage-1 fragment sets, the third blob carries c in the place of b_1."""
import numpy as np
import pytest

import oracle
from amdrec import synth, weights
from tests import cases


def _ptr_array(pk, ptr):
    return [t for t in pk._keep if t.data_ptr() == ptr][0].numpy()


def _halves(sd, user, ad, nnum, n=64):
    """float64 (ad embedding block, user | numerical block, a_ad, u_user) of n synthetic rows on the folded projection."""
    uc, un = synth.user_batch(user, nnum, n, seed=3)
    ac = synth.ad_features(ad, n, seed=4)
    feats = oracle.ranker.embed_features(sd, uc, ac, un).astype(np.float64)
    E = int(sd[f"user_embeddings.{list(user)[0]}.weight"].shape[1])
    nu, na = len(user) * E, len(ad) * E
    wf, bf = weights.folded_projection(sd)
    f_ad, f_user = feats[:, nu:nu + na], np.concatenate([feats[:, :nu], feats[:, nu + na:]], axis=1)
    a = f_ad @ wf[:, nu:nu + na].T
    u = f_user @ np.concatenate([wf[:, :nu], wf[:, nu + na:]], axis=1).T + bf
    return nu, na, f_ad, f_user, a, u


@pytest.mark.parametrize("name", ["demo", "tutorial"])
@pytest.mark.parametrize("cross", ["scaled", "randn"])
def test_cached_stage_1_equals_w1_ln1_in_float64(name, cross):
    user, ad, nnum, sd, _ = cases.ranker_case(name, cross)
    nu, na, f_ad, f_user, a, u = _halves(sd, user, ad, nnum)
    hc = weights.first_ffn_cache(sd, nu, na)
    pre = "transformer_layers.0"
    w1 = sd[f"{pre}.feed_forward.fc1.weight"].astype(np.float32).astype(np.float64)
    b1 = sd[f"{pre}.feed_forward.fc1.bias"].astype(np.float64)
    g1, be1 = sd[f"{pre}.norm1.weight"].astype(np.float64), sd[f"{pre}.norm1.bias"].astype(np.float64)
    d = a.shape[1]
    # rows the folded centering matrix is for: a large common offset (mean >> deviation) and a constant row (variance 0)
    a, u = a.copy(), u.copy()
    a[1] += 1e4
    u[2] += -3e3
    a[3], u[3] = 7.0, -2.0
    P = f_ad @ hc["w_ad"].T
    Q = f_user @ hc["w_user"].T + hc["b"]
    P[1] += hc["w1c"] @ np.full(d, 1e4)                      # the same offsets through W_1c: it annihilates constants
    Q[2] += hc["w1c"] @ np.full(d, -3e3)
    P[3], Q[3] = hc["w1c"] @ np.full(d, 7.0), hc["w1c"] @ np.full(d, -2.0)
    z = a + u
    mean = z.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mean) ** 2).mean(axis=1, keepdims=True) + 1e-5)
    x1 = (z - mean) * rstd * g1 + be1
    want = x1 @ w1.T + b1
    got = rstd * (P + Q) + hc["c"]
    assert got.dtype == np.float64
    # float64 rounding of z (|z| up to 1e4 in the offset rows) through W_1c and rstd <= 1 / sqrt(eps)
    tol = 1e-9 * max(1.0, np.abs(want).max())
    assert np.abs(got - want).max() <= tol, np.abs(got - want).max()
    assert np.abs(got[3] - (w1 @ be1 + b1)).max() <= tol      # the constant row: x1 = beta1
    assert np.abs(hc["w1c"].sum(axis=1)).max() <= 1e-12 * np.abs(hc["w1c"]).sum(axis=1).max()


def _pack(sd, user, ad, nnum, **kw):
    return weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=16, x3_min_rows=1,
                               fold_first_attention=True, **kw)


def test_third_stream_is_the_stream_minus_layer_1_stage_1_and_the_blob_keeps_its_size():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p0, pk0, _ = _pack(sd, user, ad, nnum)
    p1, pk1, _ = _pack(sd, user, ad, nnum, cache_first_ffn=True)
    assert not p0.x3.stream_hc and p0.x3.chunks_hc == 0 and not p0.x3.w_hidden_ad
    assert p1.x3.chunks == 524 and p1.x3.chunks_hc == 460
    s, s3 = _ptr_array(pk1, p1.x3.stream), _ptr_array(pk1, p1.x3.stream_hc)
    assert np.array_equal(s, _ptr_array(pk0, p0.x3.stream))                   # the 128-row stream itself is untouched
    # layer 1's FFN opens the folded stream: 33 steps of groups (4 fragment sets each) - step 0: 8 stage-1 groups, steps
    # 1..31: stage 1 and stage 2 alternating, step 32: 8 stage-2 groups (weights.x3b_stream_ffn)
    keep = np.ones(len(s) // 4, dtype=bool)
    keep[:8] = False
    keep[8:8 + 31 * 16:2] = False
    assert (~keep).sum() == 32 * 8
    assert np.array_equal(s.reshape(-1, 4, 64, 8)[keep].reshape(-1, 64, 8), s3.reshape(-1, 64, 8))
    # blob: same size, c in the place of layer 1's b_1 (folded layout: gamma1 | beta1 | b_1 ...), everything else equal
    b, b3 = _ptr_array(pk1, p1.x3.params), _ptr_array(pk1, p1.x3.params_hc)
    assert len(b3) == len(b) == p1.x3.n_params <= weights.X3_PARAM_FLOATS
    E = 32
    hc = weights.first_ffn_cache(sd, len(user) * E, len(ad) * E)
    assert np.array_equal(b3[512:512 + 1024], hc["c"].astype(np.float32))
    same = np.ones(len(b), dtype=bool)
    same[512:512 + 1024] = False
    assert np.array_equal(b[same], b3[same])
    # stacked user rows [W_user' ; W_1c W_user'] with [b_p' ; W_1c b_p'], and the ad matrix W_1c W_ad', rounded once
    wu = _ptr_array(pk1, p1.x3.w_user_uq)
    assert wu.shape[0] == 256 + 1024 and np.array_equal(wu[:256], _ptr_array(pk1, p1.w_proj_user))
    assert np.array_equal(wu[256:, :hc["w_user"].shape[1]], hc["w_user"].astype(np.float32))
    bu = _ptr_array(pk1, p1.x3.b_user_uq)
    assert np.array_equal(bu[:256], _ptr_array(pk1, p1.b_proj)) and np.array_equal(bu[256:], hc["b"].astype(np.float32))
    assert np.array_equal(_ptr_array(pk1, p1.x3.w_hidden_ad)[:, :hc["w_ad"].shape[1]], hc["w_ad"].astype(np.float32))


def test_hidden_cache_is_packed_only_for_the_folded_16_row_kernel():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    kw = dict(x6=False, x3=True, x3_min_rows=1, cache_first_ffn=True)
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3_variant=16, **kw)          # no fold
    assert not p.x3.stream_hc
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3_variant=32, fold_first_attention=True, **kw)
    assert p.x3.fold_attn1 == 1 and not p.x3.stream_hc                     # the 32-row kernel has no such phase
    user, ad, nnum, sd, _ = cases.ranker_case("tutorial", "scaled")         # not the engine's architecture
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3_variant=16, fold_first_attention=True, **kw)
    assert not p.x3.stream_hc


def test_model_flag_defaults_on_and_keys_the_packing():
    import torch
    from amdrec.ranker import TransformerRanker
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    m = TransformerRanker(dict(user), dict(ad), nnum)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.eval()
    assert m.cache_first_ffn and m.hidden_cache_max_bytes == 8 << 30
    p, _ = m._pack("cpu")
    assert p.x3.chunks_hc == 460
    key = m._packed[0]
    m.cache_first_ffn = False
    p, _ = m._pack("cpu")
    assert not p.x3.stream_hc and m._packed[0] != key
    m.cache_first_ffn = True
    m.gemm_engine = "fp32"
    assert not m._pack("cpu")[0].x3.stream_hc
