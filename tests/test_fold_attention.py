"""CPU: encoder layer 1's attention block folded into the feature projection (weights.folded_projection,
TransformerRanker.fold_first_attention).  At seq_len 1 everything of layer 1 before its first LayerNorm is linear in the
projection output, so the folded projection followed by LN1 alone is the unfolded chain up to LN1 - checked here in
float64 - and the packing of the row-owner engine drops exactly layer 1's W_ov fragments and b_ov."""
import numpy as np
import pytest

import oracle
from amdrec import synth, weights
from tests import cases


def _ptr_array(pk, ptr):
    return [t for t in pk._keep if t.data_ptr() == ptr][0].numpy()


@pytest.mark.parametrize("name", ["demo", "tutorial"])
@pytest.mark.parametrize("cross", ["scaled", "randn"])
def test_folded_projection_then_ln1_equals_the_unfolded_chain_in_float64(name, cross):
    user, ad, nnum, sd, _ = cases.ranker_case(name, cross)
    uc, un = synth.user_batch(user, nnum, 64, seed=3)
    ac = synth.ad_features(ad, 64, seed=4)
    feats = oracle.ranker.embed_features(sd, uc, ac, un).astype(np.float64)
    x0 = feats @ sd["feature_projection.weight"].astype(np.float64).T + sd["feature_projection.bias"] + \
        sd["positional_encoding"][0, 0].astype(np.float64)
    ln1 = oracle.ranker.chain_states(sd, x0, dtype=np.float64)[0]                # LN1(x0 + W_o (W_v x0 + b_v) + b_o)
    wf, bf = weights.folded_projection(sd)
    z = feats @ wf.T + bf
    got = oracle.ranker.layer_norm(z, sd["transformer_layers.0.norm1.weight"], sd["transformer_layers.0.norm1.bias"])
    assert got.dtype == np.float64
    assert np.abs(got - ln1).max() <= 1e-9 * np.abs(ln1).max(), np.abs(got - ln1).max()


def _pack(sd, user, ad, nnum, x3_variant=16, **kw):
    return weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=x3_variant, x3_min_rows=1,
                               **kw)


def test_folded_packing_drops_layer_1_attention_from_streams_and_blob():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p0, pk0, _ = _pack(sd, user, ad, nnum)
    p1, pk1, _ = _pack(sd, user, ad, nnum, fold_first_attention=True)
    assert p0.x3.fold_attn1 == 0 and p1.x3.fold_attn1 == 1
    # row-owner stream and column-split stream: the same fragment sets without layer 1's 16 W_ov chunks (its first phase)
    for ptr, n in (("stream", "chunks"), ("stream_cs", "chunks_cs")):
        assert getattr(p1.x3, n) == getattr(p0.x3, n) - 16
        s0, s1 = _ptr_array(pk0, getattr(p0.x3, ptr)), _ptr_array(pk1, getattr(p1.x3, ptr))
        assert np.array_equal(s0[16 * 16:], s1)                      # 16 fragment sets per chunk
    assert p1.x3.chunks == 3 * (16 + 128) - 16 + 3 * 16 + 60
    # parameter blob: layer 1's b_ov (the first 256 floats) left out, the rest shifted down; same padded size here
    b0, b1 = _ptr_array(pk0, p0.x3.params), _ptr_array(pk1, p1.x3.params)
    assert p1.x3.n_params == len(b1) and len(b1) % 1024 == 0
    used = 3 * (6 * 256 + 1024) + 3 * 256 + 3 * (256 + 132) - 256          # floats of the folded blob before its padding
    assert np.array_equal(b0[256:256 + used], b1[:used]) and not b1[used:].any()
    # projection: W_p' / b_p' rounded once to fp32, in the full matrix and in the user / ad split
    wf, bf = weights.folded_projection(sd)
    nu, na = len(user) * 32, len(ad) * 32
    assert np.array_equal(_ptr_array(pk1, p1.b_proj), bf.astype(np.float32))
    assert np.array_equal(_ptr_array(pk1, p1.w_proj)[:, :wf.shape[1]], wf.astype(np.float32))
    assert np.array_equal(_ptr_array(pk1, p1.w_proj_ad)[:, :na], wf[:, nu:nu + na].astype(np.float32))
    wu = _ptr_array(pk1, p1.w_proj_user)
    assert np.array_equal(wu[:, :nu], wf[:, :nu].astype(np.float32))
    assert np.array_equal(wu[:, nu:nu + nnum], wf[:, nu + na:].astype(np.float32))
    # the generic path's layer 1 is packed unchanged (amdrec_ranker_x3_prefix forms z from it)
    assert np.array_equal(_ptr_array(pk1, p1.layers[0].w_o), _ptr_array(pk0, p0.layers[0].w_o))
    assert np.array_equal(_ptr_array(pk1, p1.layers[0].b_o), _ptr_array(pk0, p0.layers[0].b_o))


def test_fold_only_where_every_pass_runs_the_row_owner_engine():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    assert _pack(sd, user, ad, nnum)[0].x3.fold_attn1 == 0                                  # packing default: off
    assert _pack(sd, user, ad, nnum, fold_first_attention=True, x3_variant=32)[0].x3.fold_attn1 == 1
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=16,
                                  x3_min_rows=8193, fold_first_attention=True)
    assert p.x3.fold_attn1 == 0                                          # small passes would run the generic chain
    p, pk, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=True, x3=False, fold_first_attention=True)
    assert p.x3.fold_attn1 == 0 and not p.x3.stream                      # fp32 / bf16x6 engines: unfolded
    b = _ptr_array(pk, p.b_proj)
    assert np.array_equal(b, (sd["feature_projection.bias"].astype(np.float64)
                              + sd["positional_encoding"][0, 0]).astype(np.float32))
    user, ad, nnum, sd, _ = cases.ranker_case("tutorial", "scaled")       # not the engine's architecture
    assert weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3=True, x3_min_rows=1,
                               fold_first_attention=True)[0].x3.fold_attn1 == 0
    user, ad, nnum, sd = cases.surface_ranker_case("x3_no_encoder")      # no encoder layer to fold
    assert _pack(sd, user, ad, nnum, fold_first_attention=True)[0].x3.fold_attn1 == 0


def test_model_flag_defaults_on_and_keys_the_packing():
    import torch
    from amdrec.ranker import TransformerRanker
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    m = TransformerRanker(dict(user), dict(ad), nnum)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.eval()
    assert m.fold_first_attention and m.fuse_attention
    p, _ = m._pack("cpu")
    assert p.x3.fold_attn1 == 1
    key = m._packed[0]
    m.fold_first_attention = False
    p, _ = m._pack("cpu")
    assert p.x3.fold_attn1 == 0 and m._packed[0] != key
    m.fold_first_attention = True
    m.gemm_engine = "fp32"
    assert m._pack("cpu")[0].x3.fold_attn1 == 0
    m.gemm_engine = "f16x3"
    m.fuse_attention = False                                             # the fold needs the fused attention (x3 does too)
    assert m._pack("cpu")[0].x3.fold_attn1 == 0
