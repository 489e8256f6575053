"""A numpy model of the WHOLE row-owner chain in the single-product arithmetic of gemm_engine "f16" (csrc/rowowner16.hpp
"SINGLE PRODUCT"): every GEMM operand rounded to ONE fp16 plane under the kernel's power-of-two scaling, one float32 GEMM of
the planes per MAC block, bias and residual folded into the accumulator's start value as the kernel does.  It is the
yardstick of tests/test_f16_engine_gpu.py, not the kernel: it differs from the kernel in the order of the fp32 sums alone
(BLAS against the MFMA's k order), about 1e-7 relative - three orders below the engine's own error of 2^-12 per operand.

What it takes from tests/x3_model.py (which documents what each mirrors): ``row_scale``, ``hidden_scale``, ``planes`` (the
high plane is ``planes(v)[0]``), ``layer_norm``; from amdrec/weights.py the pack-time functions themselves
(``x3_rebalance``, ``x3_pow2_scale``, ``x3_hidden_bound``, ``ranker_chain``, ``first_ffn_cache``), so the model follows
the packing.  Phase types (csrc/x3_common.hpp PhaseType):
* PH_ATTN_LN        x = LN(x + W_ov x + b_ov): one GEMM, start value (x + b_ov) s sw_ov;
* PH_LN             x = LN(z), z = x0 + W_ov x0 + b_ov formed in fp32-level arithmetic outside the engine (the folded
                    projection; amdrec_ranker_x3_prefix's fold kernel) - no fp16 operand at all;
* PH_FFN_LN         two GEMMs around ``hidden_planes`` (relu, the silent clamp at 60000, one plane);
* PH_FFN_LN_CACHED  stage 1 replaced by relu((P + Q) rstd + c) in fp32 (P + Q = W_1c z, weights.first_ffn_cache), stage 2 as above;
* PH_CROSS          xl = x0 (xl W + b) + xl, start value b s sw_cross;
* PH_HEADS          stacked layer 1, per task layer 2 in planes, layer 3 in plain fp32.
"""
import numpy as np

from amdrec import weights
from tests.x3_model import CLAMP, F32, LN_EPS, hidden_scale, layer_norm, planes, row_scale


def high(v32):
    """float32 -> its fp16 high plane, as float32 (the only plane this engine forms)."""
    return planes(v32)[0]


def weight_high(w64, scale):
    return high((np.asarray(w64, dtype=np.float64) * scale).astype(F32))


def gemm(a_h, w_h, acc):
    """acc + a w^T: ONE product per MAC, fp16 x fp16 exact in fp32, fp32 accumulation."""
    return (acc + a_h @ w_h.T).astype(F32)


class Chain:
    """The packed view of a state dict: fp32-rounded matrices, rebalanced, with the scales and bounds of ``x3_split``."""

    def __init__(self, sd, fold=True):
        ch = weights.ranker_chain(sd)
        f32 = lambda a: np.asarray(a).astype(F32).astype(np.float64)     # noqa: E731
        mats = {"ov": [f32(L["wov"]) for L in ch.layers], "w1": [f32(L["w1"]) for L in ch.layers],
                "b1": [f32(L["b1"]) for L in ch.layers], "w2": [f32(L["w2"]) for L in ch.layers],
                "cross": [f32(w) for w in ch.cross_wt], "h1": f32(ch.head_w1), "hb1": f32(ch.head_b1),
                "h2": [f32(h["w2"]) for h in ch.heads]}
        self.ch, self.fold = ch, bool(fold and ch.layers)
        self.m, self.lift = weights.x3_rebalance(mats)
        m = self.m
        sc = weights.x3_pow2_scale
        self.sw_ov = [sc(np.abs(w).max()) for w in m["ov"]]
        self.sw_1 = [sc(np.abs(w).max()) for w in m["w1"]]
        self.sw_2 = [sc(np.abs(w).max()) for w in m["w2"]]
        self.sw_cross = [sc(np.abs(w).max()) for w in m["cross"]]
        self.sw_h1, self.sw_h2 = sc(np.abs(m["h1"]).max()), sc(max(np.abs(w).max() for w in m["h2"]))
        self.bound = [weights.x3_hidden_bound(w, b) for w, b in zip(m["w1"], m["b1"])]
        self.bound_head = weights.x3_hidden_bound(m["h1"], m["hb1"])
        # blob parameters that multiply with lifted units (weights._pack_x3)
        f2 = self.lift["h2"]
        self.head_b2 = [(h["b2"] * f).astype(F32) for h, f in zip(ch.heads, f2)]
        self.head_w3 = [(h["w3"] / f).astype(F32) for h, f in zip(ch.heads, f2)]
        self.head_b3 = [F32(h["b3"].reshape(-1)[0]) for h in ch.heads]

    # ---- phases -----------------------------------------------------------------------------------------------------
    def fold_rows(self, x0, fma_chain=False):
        """z = x0 + W_ov x0 + b_ov of layer 1: no fp16 operand - float64 rounded once here, fp32 on the device.
        ``fma_chain``: in the order of amdrec_ranker_x3_prefix's fold kernel instead (one fp32 fma per k, ascending, then x0 +
        (acc + b_ov)) - 256 numpy steps, for the few rows on which a test compares the LayerNorm-only phase, whose whole
        error is this chain's (an fma is emulated as float32(float64 sum of the exact product): double rounding is rare)."""
        L = self.ch.layers[0]
        if not fma_chain:
            x0 = np.asarray(x0, dtype=np.float64)
            return (x0 + x0 @ self.m["ov"][0].T + L["b_ov"]).astype(F32)
        x0, w = np.asarray(x0, dtype=F32), self.m["ov"][0]                    # (fp32 values held as float64)
        acc = np.zeros(x0.shape, dtype=F32)
        for k in range(w.shape[1]):
            acc = (acc.astype(np.float64) + x0[:, k:k + 1].astype(np.float64) * w[None, :, k]).astype(F32)
        return (x0 + (acc + L["b_ov"].astype(F32)[None, :]).astype(F32)).astype(F32)

    def ln(self, z, l):
        """PH_LN -> (x, rstd [R, 1])."""
        L = self.ch.layers[l]
        z = np.asarray(z, dtype=F32)
        d = (z - z.mean(axis=1, keepdims=True, dtype=F32)).astype(F32)
        rstd = (F32(1) / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=F32) + LN_EPS)).astype(F32)
        return layer_norm(z, L["g1"], L["be1"]), rstd

    def attn_ln(self, x, l):
        L, sw = self.ch.layers[l], F32(self.sw_ov[l])
        s, inv = row_scale(x)
        acc = gemm(high(x * s), weight_high(self.m["ov"][l], sw), ((x + L["b_ov"].astype(F32)) * (s * sw)).astype(F32))
        return layer_norm((acc * (inv / sw)).astype(F32), L["g1"], L["be1"])

    def _stage2_ln(self, x, hid_h, sh, l):
        L, sw2 = self.ch.layers[l], F32(self.sw_2[l])
        k2 = (sw2 * sh).astype(F32)
        acc2 = gemm(hid_h, weight_high(self.m["w2"][l], sw2), ((x + L["b2"].astype(F32)) * k2).astype(F32))
        return layer_norm((acc2 * (F32(1) / k2)).astype(F32), L["g2"], L["be2"])

    def ffn_ln(self, x, l):
        sw1 = F32(self.sw_1[l])
        hn, hb = self.bound[l]
        s, inv = row_scale(x)
        sh = hidden_scale((F32(hn) * F32(8192.0)) * inv + F32(hb))
        acc1 = gemm(high(x * s), weight_high(self.m["w1"][l], sw1), (self.m["b1"][l].astype(F32)[None, :] * (s * sw1)).astype(F32))
        c1 = (sh * inv / sw1).astype(F32)
        hid = high(np.clip(acc1, F32(0), CLAMP / c1) * c1)
        return self._stage2_ln(x, hid, sh, l)

    def ffn_ln_cached(self, x, z, rstd):
        """PH_FFN_LN_CACHED (layer 1 behind PH_LN): x = LN1(z), rstd = its 1 / sqrt(var + eps)."""
        hc = weights.first_ffn_cache(self.ch, 0, 0, folded=(np.zeros((256, 0)), np.zeros(256)), lift=self.lift["w1"][0])
        pq = (np.asarray(z, dtype=np.float64) @ hc["w1c"].T).astype(F32)            # P[ad] + Q[user] = W_1c z
        a = (pq * rstd + hc["c"].astype(F32)[None, :]).astype(F32)
        hn, hb = self.bound[0]
        _, inv = row_scale(x)
        sh = hidden_scale((F32(hn) * F32(8192.0)) * inv + F32(hb))
        hid = high(np.clip(a, F32(0), CLAMP / sh) * sh)
        return self._stage2_ln(x, hid, sh, 0)

    def cross(self, xl, x0, c):
        sw = F32(self.sw_cross[c])
        s, inv = row_scale(xl)
        acc = gemm(high(xl * s), weight_high(self.m["cross"][c], sw), (self.ch.cross_b[c].astype(F32)[None, :] * (s * sw)).astype(F32))
        return (x0 * (acc * (inv / sw)).astype(F32) + xl).astype(F32)

    def heads(self, x):
        """-> logits [T][R] float32."""
        m, sw1, sw2 = self.m, F32(self.sw_h1), F32(self.sw_h2)
        hn, hb = self.bound_head
        n1 = m["h1"].shape[0] // len(m["h2"])
        s, inv = row_scale(x)
        sh = hidden_scale((F32(hn) * F32(8192.0)) * inv + F32(hb))
        acc1 = gemm(high(x * s), weight_high(m["h1"], sw1), (m["hb1"].astype(F32)[None, :] * (s * sw1)).astype(F32))
        c1 = (sh * inv / sw1).astype(F32)
        hid = high(np.clip(acc1, F32(0), CLAMP / c1) * c1)
        k2 = (sw2 * sh).astype(F32)
        out = []
        for t, w in enumerate(m["h2"]):
            acc2 = gemm(hid[:, t * n1:(t + 1) * n1], weight_high(w, sw2), (self.head_b2[t][None, :] * k2).astype(F32))
            y = np.maximum(acc2 * (F32(1) / k2), F32(0)).astype(F32)
            out.append((y @ self.head_w3[t] + self.head_b3[t]).astype(F32))
        return np.stack(out)

    # ---- the chain --------------------------------------------------------------------------------------------------
    def states(self, x0, cached=False):
        """Rows x0 [R, 256] (the UNFOLDED projection's output incl. pos[0], float32 or float64) -> the row state after each
        phase, in oracle.ranker.chain_states' order, and last the logits [T][R].  ``cached``: layer 1's FFN as
        PH_FFN_LN_CACHED (needs the fold)."""
        assert not cached or self.fold
        out = []
        x = np.asarray(x0, dtype=F32)
        for l in range(len(self.ch.layers)):
            if l == 0 and self.fold:
                z = self.fold_rows(x0)
                x, rstd = self.ln(z, 0)
                out.append(x)
                x = self.ffn_ln_cached(x, z, rstd) if cached else self.ffn_ln(x, 0)
            else:
                x = self.attn_ln(x, l)
                out.append(x)
                x = self.ffn_ln(x, l)
            out.append(x)
        xl = x
        for c in range(len(self.ch.cross_wt)):
            xl = self.cross(xl, x, c)
            out.append(xl)
        out.append(self.heads(xl))
        return out


def phase_names(n_layers, n_cross=3):
    return [f"L{l}.{k}" for l in range(n_layers) for k in ("attn_ln1", "ffn_ln2")] + [f"cross{c}" for c in range(n_cross)] + ["heads"]


def rel_errors(got, truth):
    """(rms, max) of got - truth relative to each row's largest |truth|."""
    truth = np.asarray(truth, dtype=np.float64)
    d = (np.asarray(got, dtype=np.float64) - truth) / np.abs(truth).max(axis=1, keepdims=True)
    return float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
