"""A numpy model of the fp16x3 row-owner engine's two hidden-layer phases (FFN + LayerNorm, heads): the arithmetic of the
kernels with the scales of the packing, for asking on the CPU how the engine's error moves with the magnitudes inside a
weight matrix.  It is a model, not the kernel: products and sums run as float32 GEMMs of the fp16 planes (the MFMA adds
fp16 x fp16 products, which are exact in fp32, into an fp32 accumulator - in another order than BLAS).

What it mirrors, line by line:
* amdrec/weights.py ``x3_pow2_scale``: one power of two per weight matrix, maxima in [2^12, 2^13) (``x3_split``: sw_1,
  sw_2 per layer; sw_h1 for the stacked head layer 1, ONE sw_h2 over all tasks' layer 2);
* amdrec/weights.py ``x3_frags``: planes h = RN16(w s), l = RN16(w s - h);
* amdrec/weights.py ``x3_split`` / ``x3_hidden_bound``: hn = 16 max_j ||w_j||_2 (1 + 1e-6), hb = max_j |b_j| (hn_head /
  hb_head: over the stacked layer 1 of all tasks) and, with ``rebalance``, the lifts of ``x3_rebalance`` (the pack-time
  functions themselves are called, so the model follows the packing);
* csrc/rowowner16_common.hpp ``row_scale`` (rowowner.hpp has the same): per row the power of two s with max|x| s in
  [2^12, 2^13), exponent field clamped to [87, 250];
* csrc/x3_common.hpp ``hidden_scale``: the power of two sh with bound sh in [2^13, 2^14), bound = hn 2^13 / s + hb
  (rowowner16_impl.hpp ``phase_ffn_ln`` / ``phase_heads``: ``fmaf(P.hn * 8192.0f, inv, P.hb)``), exponent field clamped to
  [40, 250];
* csrc/rowowner16_common.hpp ``hidden_planes``: relu, the SILENT clamp of the scaled hidden value at 60000, planes;
* three products per MAC (h h, h l, l h; l l is dropped), bias and residual folded into the accumulator's start value,
  ``layer_norm_scaled``; the heads' layer 3 in plain fp32 (``phase_heads``: dot with w_3, + b_3).
"""
import numpy as np

from amdrec import weights

F32 = np.float32
LN_EPS = F32(1e-5)
CLAMP = F32(60000.0)


def _exp_field(v):
    return ((np.asarray(v, dtype=F32).view(np.uint32) >> np.uint32(23)) & np.uint32(0xff)).astype(np.int64)


def row_scale(x):
    """-> (s, inv) [R, 1] float32 (rowowner16_common.hpp row_scale)."""
    eb = np.clip(_exp_field(np.abs(x).max(axis=1, keepdims=True)), 87, 250)
    return np.ldexp(F32(1), (weights.X3_TARGET_EXP + 127 - eb).astype(np.int32)), \
        np.ldexp(F32(1), (eb - 127 - weights.X3_TARGET_EXP).astype(np.int32))


def hidden_scale(bound):
    """x3_common.hpp hidden_scale."""
    eb = np.clip(_exp_field(bound), 40, 250)
    return np.ldexp(F32(1), (13 + 127 - eb).astype(np.int32))


def planes(v32):
    """float32 -> (h, l) as float32 holding fp16 values (weights.py x3_frags, rowowner16_common.hpp split8)."""
    v32 = np.asarray(v32, dtype=F32)
    with np.errstate(over="ignore"):
        h = v32.astype(np.float16)
    assert np.isfinite(h).all(), "fp16 plane overflowed"
    l = (v32 - h.astype(F32)).astype(np.float16)
    return h.astype(F32), l.astype(F32)


def x3_gemm(a, b, acc):
    """acc + a b^T with both operands as two fp16 planes and three products, fp32 accumulation."""
    (ah, al), (bh, bl) = a, b
    return (acc + ah @ bh.T + ah @ bl.T + al @ bh.T).astype(F32)


def weight_planes(w64, scale):
    return planes((np.asarray(w64, dtype=np.float64) * scale).astype(F32))


def _hidden(x, xs, s, inv, w1, b1, sw1, hn, hb):
    """Stage 1 + ``hidden_planes`` -> (planes of relu(W_1 x + b_1) * sh, sh, number of clamped values)."""
    sh = hidden_scale((F32(hn) * F32(8192.0)) * inv + F32(hb))
    acc1 = x3_gemm(xs, weight_planes(w1, sw1), (b1.astype(F32)[None, :] * (s * F32(sw1))).astype(F32))
    c1 = (sh * inv / F32(sw1)).astype(F32)
    lim1 = CLAMP / c1
    clamped = int((acc1 > lim1).sum())
    return planes(np.clip(acc1, F32(0), lim1) * c1), sh, clamped


def layer_norm(y, g, b):
    mean = y.mean(axis=1, keepdims=True, dtype=F32)
    d = (y - mean).astype(F32)
    rstd = F32(1) / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=F32) + LN_EPS)
    return (d * rstd * g.astype(F32) + b.astype(F32)).astype(F32)


def _f32_64(a):
    return np.asarray(a, dtype=F32).astype(np.float64)


def ffn_ln(x, w1, b1, w2, b2, g, be, rebalance):
    """rowowner16_impl.hpp phase_ffn_ln on rows x (float32, LN1's output) -> (LN2(x + FFN(x)) float32, clamp count).
    ``rebalance``: pack with the per-unit lifts of weights.x3_rebalance (what x3_split does) or as before them."""
    w1, b1, w2 = _f32_64(w1), _f32_64(b1), _f32_64(w2)
    if rebalance:
        f = weights.x3_unit_lifts(w1, b1)
        w1, b1, w2 = w1 * f[:, None], b1 * f, w2 / f[None, :]
    sw1, sw2 = weights.x3_pow2_scale(np.abs(w1).max()), weights.x3_pow2_scale(np.abs(w2).max())
    hn, hb = weights.x3_hidden_bound(w1, b1)
    x = np.asarray(x, dtype=F32)
    s, inv = row_scale(x)
    hid, sh, clamped = _hidden(x, planes(x * s), s, inv, w1, b1, sw1, hn, hb)
    k2 = (F32(sw2) * sh).astype(F32)
    acc2 = x3_gemm(hid, weight_planes(w2, sw2), ((x + b2.astype(F32)) * k2).astype(F32))
    return layer_norm((acc2 * (F32(1) / k2)).astype(F32), g, be), clamped


def heads(x, h1, hb1, h2, b2, w3, b3, rebalance):
    """rowowner16_impl.hpp phase_heads: h1 [T * n1][256] stacked, hb1 [T * n1], per task h2 [64][n1], b2 [64], w3 [64],
    b3 -> (logits [T][R] float32, clamp count)."""
    h1, hb1 = _f32_64(h1), _f32_64(hb1)
    h2, b2, w3 = [_f32_64(w) for w in h2], [_f32_64(b) for b in b2], [_f32_64(w) for w in w3]
    if rebalance:
        h1, hb1, h2, _, f2 = weights.x3_rebalance_heads(h1, hb1, h2)
        b2, w3 = [b * f for b, f in zip(b2, f2)], [w / f for w, f in zip(w3, f2)]
    n1 = h1.shape[0] // len(h2)
    sw1, sw2 = weights.x3_pow2_scale(np.abs(h1).max()), weights.x3_pow2_scale(max(np.abs(w).max() for w in h2))
    hn, hb = weights.x3_hidden_bound(h1, hb1)
    x = np.asarray(x, dtype=F32)
    s, inv = row_scale(x)
    (hh, hl), sh, clamped = _hidden(x, planes(x * s), s, inv, h1, hb1, sw1, hn, hb)
    k2 = (F32(sw2) * sh).astype(F32)
    out = []
    for t, w in enumerate(h2):
        hid = (hh[:, t * n1:(t + 1) * n1], hl[:, t * n1:(t + 1) * n1])
        acc2 = x3_gemm(hid, weight_planes(w, sw2), (b2[t].astype(F32)[None, :] * k2).astype(F32))
        y = np.maximum(acc2 * (F32(1) / k2), F32(0)).astype(F32)
        out.append((y @ w3[t].astype(F32) + F32(np.asarray(b3[t]).reshape(-1)[0])).astype(F32))
    return np.stack(out), clamped


# ---- plain evaluations of the same two phases (the yardsticks) -------------------------------------------------------
def ffn_ln_plain(x, w1, b1, w2, b2, g, be, dtype):
    c = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    x = c(x)
    h = np.maximum(x @ c(w1).T + c(b1), dtype(0))
    y = x + (h @ c(w2).T + c(b2))
    mean = y.mean(axis=1, keepdims=True, dtype=dtype)
    d = y - mean
    return (d / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=dtype) + dtype(1e-5)) * c(g) + c(be)).astype(dtype)


def heads_plain(x, h1, hb1, h2, b2, w3, b3, dtype):
    c = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    n1 = np.asarray(h1).shape[0] // len(h2)
    h = np.maximum(c(x) @ c(h1).T + c(hb1), dtype(0))
    out = []
    for t in range(len(h2)):
        y = np.maximum(h[:, t * n1:(t + 1) * n1] @ c(h2[t]).T + c(b2[t]), dtype(0))
        out.append(y @ c(w3[t]).reshape(-1) + c(b3[t]).reshape(-1)[0])
    return np.stack(out).astype(dtype)


def ratios(got, f32, truth, per_row=True):
    """(max ratio, rms ratio) of got's error over the plain fp32 evaluation's, both against float64 ``truth``; relative to
    each row's largest |truth| (``per_row``, axis 1) or to the largest |truth| of all."""
    truth = np.asarray(truth, dtype=np.float64)
    scale = np.abs(truth).max(axis=1, keepdims=True) if per_row else np.abs(truth).max()
    d, d32 = (got - truth) / scale, (f32 - truth) / scale
    return float(np.abs(d).max() / np.abs(d32).max()), float(np.sqrt((d * d).mean()) / np.sqrt((d32 * d32).mean()))
