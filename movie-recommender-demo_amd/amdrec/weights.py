"""Host-side weight preparation for libamdrec: fold eval-mode BatchNorm into the preceding
Linear, zero-pad K to a multiple of 32, stack embedding tables, transpose cross weights,
fold the positional row into the projection bias; build the ctypes parameter structs of
include/amdrec.h.  Runs once per weight load (float64 on the host, rounded to float32)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple

import numpy as np
import torch

MAX_LAYERS = 8
MAX_TASKS = 4
_FP = C.c_void_p
TASKS = ("ctr", "engagement", "revenue")


class TowerParams(C.Structure):
    _fields_ = [("n_feat", C.c_int32), ("emb_dim", C.c_int32), ("n_num", C.c_int32), ("n_layers", C.c_int32),
                ("dims", C.c_int32 * (MAX_LAYERS + 1)), ("ldw", C.c_int32 * MAX_LAYERS),
                ("tables", _FP), ("table_off", _FP), ("cards", _FP),
                ("w", _FP * MAX_LAYERS), ("b", _FP * MAX_LAYERS), ("renormalize", C.c_int32)]


class EncoderLayer(C.Structure):
    _fields_ = [(n, _FP) for n in ("w_v", "b_v", "w_o", "b_o", "ln1_g", "ln1_b", "w_1", "b_1", "w_2", "b_2",
                                   "ln2_g", "ln2_b")] + [("ldw_dm", C.c_int32), ("ldw_ff", C.c_int32)] + \
               [(n, _FP) for n in ("w_o_x6", "w_1_x6", "w_2_x6")]


class X3Weights(C.Structure):
    # (amdrec_x3_weights up to its CTR-first streams; what the header appended since is in X3WeightsP below)
    _fields_ = [("stream", _FP), ("chunks", C.c_int64), ("min_rows", C.c_int64), ("params", _FP), ("n_params", C.c_int64),
                ("variant", C.c_int64),
                ("sw_ov", C.c_float * MAX_LAYERS), ("sw_1", C.c_float * MAX_LAYERS), ("sw_2", C.c_float * MAX_LAYERS),
                ("hn", C.c_float * MAX_LAYERS), ("hb", C.c_float * MAX_LAYERS), ("sw_cross", C.c_float * MAX_LAYERS),
                ("sw_h1", C.c_float), ("sw_h2", C.c_float), ("hn_head", C.c_float), ("hb_head", C.c_float),
                ("stream_cs", _FP), ("chunks_cs", C.c_int64), ("cs_max_rows", C.c_int64), ("fold_attn1", C.c_int64),
                ("stream_hc", _FP), ("chunks_hc", C.c_int64), ("params_hc", _FP), ("w_user_uq", _FP), ("b_user_uq", _FP),
                ("w_hidden_ad", _FP),
                ("stream_ctr", _FP), ("chunks_ctr", C.c_int64), ("stream_ctr_cs", _FP), ("chunks_ctr_cs", C.c_int64),
                ("stream_ctr_hc", _FP), ("chunks_ctr_hc", C.c_int64), ("stream_win", _FP), ("chunks_win", C.c_int64),
                ("stream_win_cs", _FP), ("chunks_win_cs", C.c_int64)]


class X3WeightsP(X3Weights):
    """amdrec_x3_weights as the header has it now: ctypes lays a subclass's fields behind its base's, which is where the
    header appended ``products`` (0 / 3: the fp16x3 arithmetic, 1: the single-product engine)."""
    _fields_ = [("products", C.c_int64)]


class RankerParams(C.Structure):
    _fields_ = [("n_user_feat", C.c_int32), ("n_ad_feat", C.c_int32), ("emb_dim", C.c_int32), ("n_num", C.c_int32),
                ("d_model", C.c_int32), ("d_ff", C.c_int32), ("n_layers", C.c_int32), ("n_cross", C.c_int32),
                ("n_tasks", C.c_int32), ("head_h1", C.c_int32), ("head_h2", C.c_int32), ("ln_eps", C.c_float),
                ("ldw_proj", C.c_int32), ("ldw_cross", C.c_int32), ("ldw_head1", C.c_int32),
                ("ldw_head2", C.c_int32),
                ("tables", _FP), ("table_off", _FP), ("cards", _FP), ("w_proj", _FP), ("b_proj", _FP),
                ("w_proj_user", _FP), ("w_proj_ad", _FP), ("ldw_proj_user", C.c_int32), ("ldw_proj_ad", C.c_int32),
                ("layers", EncoderLayer * MAX_LAYERS),
                ("cross_wt", _FP * MAX_LAYERS), ("cross_b", _FP * MAX_LAYERS),
                ("head_w1", _FP), ("head_b1", _FP),
                ("head_w2", _FP * MAX_TASKS), ("head_b2", _FP * MAX_TASKS),
                ("head_w3", _FP * MAX_TASKS), ("head_b3", _FP * MAX_TASKS),
                ("ad_proj_cache", _FP), ("ld_ad_proj_cache", C.c_int64),
                ("ad_hidden_cache", _FP), ("ld_ad_hidden_cache", C.c_int64),
                ("cross_wt_x6", _FP * MAX_LAYERS), ("head_w1_x6", _FP), ("x3", X3WeightsP)]


def _np64(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def split_planes(w32: np.ndarray) -> np.ndarray:
    """fp32 [out][ld] (ld % 32 == 0) -> int16 view of [out][ld/16][3][16]: the bf16 planes h, m, l of the exact 3-way
    truncation split w = h + m + l consumed by the x6 GEMM (include/amdrec.h, amdrec_encoder_layer)."""
    w = np.ascontiguousarray(w32, dtype=np.float32)
    out_f, ld = w.shape
    assert ld % 32 == 0
    u = w.view(np.uint32)
    h = (u & np.uint32(0xffff0000)).view(np.float32)
    r1 = w - h                                              # exact
    m = (r1.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r2 = r1 - m                                             # exact, <= 8 significant bits
    planes = np.stack([(x.view(np.uint32) >> np.uint32(16)).astype(np.uint16) for x in (h, m, r2)], axis=0)
    assert np.array_equal(h + m + r2, w)                    # the split is exact
    return np.ascontiguousarray(planes.reshape(3, out_f, ld // 16, 16).transpose(1, 2, 0, 3)).view(np.int16)


# ---- fp16x3 row-owner engine: fragment packing (mirrors csrc/rowowner.hpp) --------------------------------------------
X3_TARGET_EXP = 12          # scaled maxima lie in [2^12, 2^13)
# position i = 8 h + j of a k-step holds feature offset 8 (j >> 2) + 4 h + (j & 3): bits 2 and 3 of the index swap
_X3_KSRC = np.array([(i & 3) | (((i >> 3) & 1) << 2) | (((i >> 2) & 1) << 3) for i in range(16)])


def x3_pow2_scale(maxabs: float, target_exp: int = X3_TARGET_EXP) -> float:
    """The power of two s with maxabs * s in [2^target_exp, 2^(target_exp+1)) (1.0 for an all-zero matrix)."""
    if not np.isfinite(maxabs) or maxabs <= 0:
        return 1.0
    return float(2.0 ** (target_exp - int(np.floor(np.log2(maxabs)))))


def x3_frags(w64: np.ndarray, scale: float) -> np.ndarray:
    """[N][K] (N % 32 == 0, K % 16 == 0) -> uint16 [N/32][K/16][2 planes][64 lanes][8]: the fp16 planes h = RN16(w s),
    l = RN16(w s - h) of every (32-feature tile, 16-wide k-step) as MFMA A fragments in lane order (lane = p + 32 half
    holds k positions 8 half .. 8 half + 7 of row p), with the accumulator-as-operand k permutation applied."""
    n, k = w64.shape
    assert n % 32 == 0 and k % 16 == 0
    ws = (np.asarray(w64, dtype=np.float64) * scale).astype(np.float32)        # exact: power-of-two scaling of fp32 values
    h = ws.astype(np.float16)
    assert np.isfinite(h).all(), "x3 weight plane overflowed fp16"
    l = (ws - h.astype(np.float32)).astype(np.float16)
    planes = np.stack([h, l]).view(np.uint16)                                  # [2][N][K]
    planes = planes.reshape(2, n, k // 16, 16)[:, :, :, _X3_KSRC]              # position i <- source k offset _X3_KSRC[i]
    planes = planes.reshape(2, n // 32, 32, k // 16, 2, 8)                     # plane, tile, p, ks, half, j
    return np.ascontiguousarray(planes.transpose(1, 3, 0, 4, 2, 5)).reshape(n // 32, k // 16, 2, 64, 8)


def x3_stream_gemm256(fr: np.ndarray) -> np.ndarray:
    """fragments of a [256][256] matrix -> stream order `for ks: for tile: (h, l)` (rowowner.hpp gemm256)."""
    return np.ascontiguousarray(fr.transpose(1, 0, 2, 3, 4)).reshape(-1, 64, 8)


def x3_stream_ffn(f1: np.ndarray, f2: np.ndarray) -> np.ndarray:
    """f1 = fragments of W_1 [d_ff][256], f2 = of W_2 [256][d_ff] -> rowowner.hpp ffn_step order: step t = 0 .. T:
    per micro-step u = 0..15: stage 1 (tile t, ks u) if t < T, then stage 2 (tile u & 7, ks 2 (t - 1) + (u >> 3)) if t >= 1."""
    T = f1.shape[0]
    out = []
    for t in range(T + 1):
        for u in range(16):
            if t < T:
                out += [f1[t, u, 0], f1[t, u, 1]]
            if t >= 1:
                i, ks = u & 7, 2 * (t - 1) + (u >> 3)
                out += [f2[i, ks, 0], f2[i, ks, 1]]
    return np.stack(out)


def x3_stream_heads(f1: np.ndarray, f2s: List[np.ndarray], tiles_per_task: int) -> np.ndarray:
    """f1 = fragments of the stacked head layer 1 [n_tasks * h1][256]; f2s[t] = of head t's layer 2 [64][h1] ->
    rowowner.hpp phase_heads order: per task, per hidden tile: 16 x (h, l) of stage 1, then for s in 0, 1: for i in 0, 1: (h, l)."""
    out = []
    for task, f2 in enumerate(f2s):
        for t in range(tiles_per_task):
            for u in range(16):
                out += [f1[task * tiles_per_task + t, u, 0], f1[task * tiles_per_task + t, u, 1]]
            for sp in range(2):
                for i in range(2):
                    out += [f2[i, 2 * t + sp, 0], f2[i, 2 * t + sp, 1]]
    return np.stack(out)


# ---- 16-rows-per-wave variant (csrc/rowowner16.hpp): 16-feature output tiles, 32-wide k-steps ------------------------
# k position i = 8 g + j of a 32-wide k-step holds feature offset 16 (j >> 2) + 4 g + (j & 3)
_X3B_KSRC = np.array([16 * ((i & 7) >> 2) + 4 * (i >> 3) + (i & 3) for i in range(32)])


def x3b_frags(w64: np.ndarray, scale: float) -> np.ndarray:
    """[N][K] (N % 16 == 0, K % 32 == 0) -> uint16 [N/16][K/32][2 planes][64 lanes][8]: A fragments of
    v_mfma_f32_16x16x32_f16 (lane = p + 16 g holds k positions 8 g .. 8 g + 7 of row p) with the 16-row kernel's k permutation."""
    n, k = w64.shape
    assert n % 16 == 0 and k % 32 == 0
    ws = (np.asarray(w64, dtype=np.float64) * scale).astype(np.float32)
    h = ws.astype(np.float16)
    assert np.isfinite(h).all(), "x3 weight plane overflowed fp16"
    l = (ws - h.astype(np.float32)).astype(np.float16)
    planes = np.stack([h, l]).view(np.uint16)                                  # [2][N][K]
    planes = planes.reshape(2, n, k // 32, 32)[:, :, :, _X3B_KSRC]             # position i <- source k offset
    planes = planes.reshape(2, n // 16, 16, k // 32, 4, 8)                     # plane, tile, p, ks, g, j
    return np.ascontiguousarray(planes.transpose(1, 3, 0, 4, 2, 5)).reshape(n // 16, k // 32, 2, 64, 8)


def _pair(f, t0, ks):
    return [f[t0, ks, 0], f[t0, ks, 1], f[t0 + 1, ks, 0], f[t0 + 1, ks, 1]]


def x3b_stream_gemm256(fr):
    out = []
    for ks in range(fr.shape[1]):
        for tp in range(fr.shape[0] // 2):
            out += _pair(fr, 2 * tp, ks)
    return np.stack(out)


def x3b_stream_cross(fr):
    """A cross layer's 256 x 256 GEMM in four QUARTERS of the output features (4 tiles of 16 = 2 tile pairs each, 16 groups =
    4 chunks): the 16-row kernel keeps x0 in registers across the cross layers and can only afford a 16-register
    accumulator beside it (csrc/rowowner16_impl.hpp phase_cross).  Within a quarter: k-step major, as in gemm256."""
    out = []
    for q4 in range(fr.shape[0] // 4):
        for ks in range(fr.shape[1]):
            for pr in range(2):
                out += _pair(fr, 2 * (2 * q4 + pr), ks)
    return np.stack(out)


def x3b_stream_ffn(f1, f2):
    T = f1.shape[0] // 2                     # hidden tiles of 32
    out = []
    for t in range(T + 1):
        for u in range(8):
            if t < T:
                out += _pair(f1, 2 * t, u)
            if t >= 1:
                out += _pair(f2, 2 * u, t - 1)
    return np.stack(out)


def x3b_stream_ffn_stage2(f2):
    """An FFN of the 16-row kernel whose stage 1 is served from the hidden cache (csrc/rowowner16_impl.hpp
    phase_ffn_ln_cached): the stage-2 groups of ``x3b_stream_ffn`` alone, in the same order (8 groups = 2 chunks per step)."""
    out = []
    for t in range(f2.shape[1]):
        for u in range(8):
            out += _pair(f2, 2 * u, t)
    return np.stack(out)


def _task_window(f2s, tiles_per_task, tasks):
    """``tasks`` = (first task, number of tasks) or None = all -> (the window's f2s, its first hidden tile in f1: f1 is
    stacked over ALL tasks and indexed by hidden tile through them, so a window that starts at task t0 starts at tile
    t0 * tiles_per_task)."""
    t0, n = (0, len(f2s)) if tasks is None else tasks
    assert 0 <= t0 and n >= 1 and t0 + n <= len(f2s)
    return f2s[t0:t0 + n], t0 * tiles_per_task


def x3b_stream_heads(f1, f2s, tiles_per_task, tasks=None):
    """Heads of the 16-row kernel, software-pipelined like the FFN (csrc/rowowner16_impl.hpp heads_step): step tt = the 8
    stage-1 groups of hidden tile tt (tiles counted through all tasks) with the 2 stage-2 groups of tile tt - 1 behind
    u = 3 and u = 7; step 0 has no stage 2, the last step no stage 1.  ``tasks``: the heads of that task window alone
    (``_task_window``) - a program of its own, so its first step has no stage 2 and its last no stage 1."""
    f2s, base = _task_window(f2s, tiles_per_task, tasks)
    nt = len(f2s) * tiles_per_task
    # the kernel's steps start at group 0 or 2 of a chunk and the last one at 2: an even number of hidden tiles, whole chunks
    assert nt % 2 == 0 and (nt * 10) % 4 == 0, "head stream is not a whole number of chunks"
    out = []
    for tt in range(nt + 1):
        prev = tt - 1
        for u in range(8):
            if tt < nt:
                out += _pair(f1, 2 * (base + tt), u)
            if tt >= 1 and u in (3, 7):
                out += _pair(f2s[prev // tiles_per_task], 2 * (u // 4), prev % tiles_per_task)
    return np.stack(out)


def _wave_chunk(groups):
    """One 16 KB chunk of the column-split kernel: group w (4 fragment sets) for wave w; None = a wave without work (zeros)."""
    out = []
    for g in groups:
        out += g if g is not None else [np.zeros((64, 8), np.uint16)] * 4
    assert len(out) == 16
    return out


def x3c_stream_gemm256(fr):
    """Column-split kernel (csrc/rowowner16c.hpp): wave w owns output tiles 4 w .. 4 w + 3 = tile pairs 2 w, 2 w + 1; per
    k-step two chunks (pair j of every wave)."""
    assert fr.shape[0] == 16
    out = []
    for ks in range(fr.shape[1]):
        for j in range(2):
            out += _wave_chunk([_pair(fr, 2 * (2 * w + j), ks) for w in range(4)])
    return np.stack(out)


def x3c_stream_ffn(f1, f2):
    """FFN in super-steps of four hidden steps (32 hidden units each), one per wave.  Super-step T: for i < 8 the stage-1
    chunk {wave w: W_1 tile pair of hidden step 4 T + w at k-step i} followed by the stage-2 chunk of super-step T - 1
    {wave w: W_2 output pair 2 w + (i & 1) at k-step 4 (T - 1) + (i >> 1)}."""
    T = f1.shape[0] // 2
    assert T % 4 == 0 and f2.shape[0] == 16
    S = T // 4
    out = []
    for s in range(S + 1):
        for i in range(8):
            if s < S:
                out += _wave_chunk([_pair(f1, 2 * (4 * s + w), i) for w in range(4)])
            if s >= 1:
                out += _wave_chunk([_pair(f2, 2 * (2 * w + (i & 1)), 4 * (s - 1) + (i >> 1)) for w in range(4)])
    return np.stack(out)


def x3c_stream_heads(f1, f2s, tiles_per_task, tasks=None):
    """Heads in super-steps of four hidden steps (counted through all tasks; tiles_per_task % 4 == 0 keeps a super-step inside
    one task).  Stage 1 as in the FFN; stage 2 of super-step s - 1 = four chunks (its k-steps, ascending) behind the stage-1
    chunks i = 3 (two) and i = 7 (two): {wave 0: output pair 0, wave 1: pair 1, waves 2 and 3: zeros}.  ``tasks``: as in
    ``x3b_stream_heads``; every super-step is 8 or 12 chunks, so any window is a multiple of 4 chunks long."""
    assert tiles_per_task % 4 == 0
    f2s, base = _task_window(f2s, tiles_per_task, tasks)
    nt = len(f2s) * tiles_per_task
    S = nt // 4
    out = []
    for s in range(S + 1):
        for i in range(8):
            if s < S:
                out += _wave_chunk([_pair(f1, 2 * (base + 4 * s + w), i) for w in range(4)])
            if s >= 1 and (i & 3) == 3:
                first = 4 * (s - 1)
                f2, k0 = f2s[first // tiles_per_task], first % tiles_per_task
                for kk in (2 * (i >> 2), 2 * (i >> 2) + 1):
                    out += _wave_chunk([_pair(f2, 0, k0 + kk), _pair(f2, 2, k0 + kk), None, None])
    return np.stack(out)


# stream kind -> the order in which its kernel reads the fragment sets of (a 256 x 256 GEMM, a cross layer, an FFN, the heads);
# the hidden-cache stream (amdrec_x3_weights.stream_hc) is kind 16 with layer 1's FFN as x3b_stream_ffn_stage2
_X3_ORDER = {32: (x3_stream_gemm256, x3_stream_gemm256, x3_stream_ffn, x3_stream_heads),
             16: (x3b_stream_gemm256, x3b_stream_cross, x3b_stream_ffn, x3b_stream_heads),
             "16cs": (x3c_stream_gemm256, x3c_stream_gemm256, x3c_stream_ffn, x3c_stream_heads)}


# ---- per-unit rebalancing of the hidden layers ------------------------------------------------------------------------
# The engine has ONE power-of-two scale per weight matrix and ONE per row for a whole hidden tile, taken from the worst-case
# bound of ``x3_hidden_bound``.  A hidden unit whose [w_j | b_j] lies many binades under the layer's largest therefore lands
# in fp16 subnormals twice: its W_1 row under sw_1 and its hidden value under the bound - while its W_2 column, which a
# trained net makes correspondingly large, sets sw_2 for everybody else.  relu(a t) / a == relu(t) exactly for a power of two
# a, so such a unit is lifted at pack time: row j of W_1 and b_1[j] times 2^k, column j of W_2 divided by it.  A unit within
# X3_REBALANCE_BINADES of the largest keeps the factor 1: i.i.d. weights pack to the bytes they always had.  The threshold
# comes from the sweep in tests/test_x3_model_cpu.py (None: no rebalancing, the packing before it existed).
X3_REBALANCE_BINADES = 4


def _binade(v):
    return np.floor(np.log2(v)).astype(np.int64)


def _lifts_to(size: np.ndarray) -> np.ndarray:
    """Per entry of ``size`` (>= 0) the power of two >= 1 that brings it to X3_REBALANCE_BINADES binades under the largest
    (1.0 for entries that are there already, for zeros and non-finite sizes, and for all when rebalancing is off)."""
    size = np.asarray(size, dtype=np.float64)
    f = np.ones(size.shape)
    ok = np.isfinite(size) & (size > 0)
    if X3_REBALANCE_BINADES is None or not ok.any():
        return f
    f[ok] = 2.0 ** np.maximum(0, _binade(size[ok].max()) - X3_REBALANCE_BINADES - _binade(size[ok]))
    return f


def x3_unit_lifts(w1: np.ndarray, b1: np.ndarray) -> np.ndarray:
    """Hidden layer W_1 [n][k], b_1 [n] -> the power of two per hidden unit by which its W_1 row and bias are multiplied
    (and its W_2 column divided): units measured by ||[w_j | b_j]||_2."""
    return _lifts_to(np.sqrt((np.asarray(w1, dtype=np.float64) ** 2).sum(axis=1) + np.asarray(b1, dtype=np.float64) ** 2))


def _scaled(a, f):
    return a if (f == 1.0).all() else a * f       # (the common case returns the very array)


def x3_rebalance_heads(h1, hb1, h2):
    """Stacked head layer 1 [T * n1][256], its bias, per task layer 2 [64][n1] -> (h1', hb1', h2', per-unit lifts of layer 1,
    per-task lifts of layer 2).  Layer 1 per unit as in an FFN (all tasks share sw_h1 and one hidden bound, so a task whose
    units are small as a whole is lifted as a whole); then a task whose layer 2 - after its columns took layer 1's lifts -
    lies more than X3_REBALANCE_BINADES under the largest task's in max |w| is lifted as a whole under the shared sw_h2: its
    b_2 goes with it and its w_3 (fp32, in the parameter blob) is divided."""
    f1 = x3_unit_lifts(h1, hb1)
    n1 = h1.shape[0] // len(h2)
    h2 = [_scaled(w, 1.0 / f1[None, t * n1:(t + 1) * n1]) for t, w in enumerate(h2)]
    f2 = _lifts_to(np.array([np.abs(w).max() for w in h2]))
    return _scaled(h1, f1[:, None]), _scaled(hb1, f1), [_scaled(w, f) for w, f in zip(h2, f2)], f1, f2


def x3_rebalance(mats: Dict):
    """``mats`` of ``pack_x3_stream`` -> (the same network with every FFN's and the heads' hidden units rebalanced,
    {"w1": per layer the unit lifts, "h1": the stacked head layer 1's, "h2": per task}).  Whatever else multiplies with
    these hidden units takes the same factors: b_1 / head b_1, b_2 and w_3 in ``pack_x3_params`` and the rows of
    ``first_ffn_cache``."""
    lift = {"w1": [x3_unit_lifts(w, b) for w, b in zip(mats["w1"], mats["b1"])]}
    out = dict(mats)
    out["w1"] = [_scaled(w, f[:, None]) for w, f in zip(mats["w1"], lift["w1"])]
    out["b1"] = [_scaled(b, f) for b, f in zip(mats["b1"], lift["w1"])]
    out["w2"] = [_scaled(w, 1.0 / f[None, :]) for w, f in zip(mats["w2"], lift["w1"])]
    out["h1"], out["hb1"], out["h2"], lift["h1"], lift["h2"] = x3_rebalance_heads(mats["h1"], mats["hb1"], mats["h2"])
    return out, lift


def x3_hidden_bound(w1: np.ndarray, b1: np.ndarray):
    """(hn, hb) of amdrec_x3_weights: |relu(w_j . x + b_j)| <= ||w_j||_2 ||x||_2 + |b_j| <= (16 max_j ||w_j||_2) max|x| +
    max_j |b_j| for 256-wide x."""
    return float(16.0 * np.linalg.norm(w1, axis=1).max() * (1 + 1e-6)), float(np.abs(b1).max())


def x3_split(mats: Dict, variant: int = 32, fold_first: bool = False):
    """Scale and plane-split every matrix of ``mats`` (see ``pack_x3_stream``) once -> (fragments {"ov", "w1", "w2", "cross":
    lists, "h1", "h2", "tiles"}, scales and hidden bounds of amdrec_x3_weights and "lift": the factors of ``x3_rebalance``,
    which is applied first).  Kinds 16 and "16cs" share the fragments of variant 16.  ``fold_first``: layer 1's W_ov is not
    split (its fragments are None, its scale reads 1.0)."""
    mats, lift = x3_rebalance(mats)
    frags = x3_frags if variant == 32 else x3b_frags
    fr, sc = {"tiles": mats["h1"].shape[0] // len(mats["h2"]) // 32}, {}
    for name, dst in (("ov", "sw_ov"), ("w1", "sw_1"), ("w2", "sw_2"), ("cross", "sw_cross")):
        ws = [None if name == "ov" and fold_first and l == 0 else w for l, w in enumerate(mats[name])]
        sc[dst] = [1.0 if w is None else x3_pow2_scale(np.abs(w).max()) for w in ws]
        fr[name] = [None if w is None else frags(w, s) for w, s in zip(ws, sc[dst])]
    sc["sw_h1"] = x3_pow2_scale(np.abs(mats["h1"]).max())
    sc["sw_h2"] = x3_pow2_scale(max(np.abs(w).max() for w in mats["h2"]))
    fr["h1"], fr["h2"] = frags(mats["h1"], sc["sw_h1"]), [frags(w, sc["sw_h2"]) for w in mats["h2"]]
    bounds = [x3_hidden_bound(w, b) for w, b in zip(mats["w1"], mats["b1"])]
    sc["hn"], sc["hb"] = [n for n, _ in bounds], [b for _, b in bounds]
    sc["hn_head"], sc["hb_head"] = x3_hidden_bound(mats["h1"], mats["hb1"])
    sc["lift"] = lift
    return fr, sc


def x3_order(fr: Dict, kind, cache_first_ffn: bool = False, tasks=None, trunk: bool = True) -> np.ndarray:
    """The fragments of ``x3_split`` in the order stream ``kind`` (32, 16, "16cs") is read -> uint16 [n_frag][64][8].
    ``tasks`` = (first task, number of tasks): the heads of that window alone (kinds 16 and "16cs"); ``trunk=False``: nothing
    in front of the heads (the heads-only program).  The streams of CTR-first ranking (``X3_CTR_FIRST_STREAMS``) are such cuts
    of the ONE split: nothing is scaled or split a second time."""
    s_gemm, s_cross, s_ffn, s_heads = _X3_ORDER[kind]
    assert trunk or not cache_first_ffn
    assert tasks is None or kind in (16, "16cs"), "task windows exist for the 16-row kernels only"
    parts = []
    for l, (ov, f1, f2) in enumerate(zip(fr["ov"], fr["w1"], fr["w2"]) if trunk else ()):
        parts += [] if ov is None else [s_gemm(ov)]
        parts.append(x3b_stream_ffn_stage2(f2) if cache_first_ffn and l == 0 else s_ffn(f1, f2))
    parts += [s_cross(f) for f in fr["cross"]] if trunk else []
    parts.append(s_heads(fr["h1"], fr["h2"], fr["tiles"], *(() if tasks is None else (tasks,))))
    stream = np.concatenate(parts)
    # every phase a whole number of chunks; the column-split kernel's ring position is a compile-time constant: multiples of 4
    assert stream.shape[0] % 16 == 0 and (kind != "16cs" or all(len(q) % 64 == 0 for q in parts))
    return stream


def x3_ctr_first_orders(n_tasks: int, column_split: bool, cache_first_ffn: bool) -> Dict:
    """amdrec_x3_weights field stem -> the ``x3_order`` arguments of that stream of CTR-first ranking: per ordering the trunk
    with the head of task 0 alone (stream_ctr*), and the heads of tasks 1 .. n_tasks - 1 alone (stream_win*)."""
    win = (1, n_tasks - 1)
    orders = {"ctr": dict(kind=16, tasks=(0, 1)), "win": dict(kind=16, tasks=win, trunk=False)}
    if column_split:
        orders["ctr_cs"] = dict(kind="16cs", tasks=(0, 1))
        orders["win_cs"] = dict(kind="16cs", tasks=win, trunk=False)
    if cache_first_ffn:
        orders["ctr_hc"] = dict(kind=16, tasks=(0, 1), cache_first_ffn=True)
    return orders


def pack_x3_stream(mats: Dict, variant: int = 32, fold_first: bool = False, cache_first_ffn: bool = False) -> Dict:
    """mats: float64 matrices of the chain {"ov": [L x [256][256]], "w1": [L x [d_ff][256]], "b1": [L x [d_ff]], "w2":
    [L x [256][d_ff]], "cross": [C x [256][256] (already [out][in])], "h1": [T*h1][256], "hb1": [T*h1], "h2": [T x
    [64][h1]]} -> {"stream": uint16 [n_frag][64][8], "chunks", scales and hidden bounds, "lift"} for amdrec_x3_weights: one
    ``x3_split`` in one ``x3_order`` (pack_ranker orders ONE split up to three ways).  "lift": the factors of
    ``x3_rebalance`` that the caller's parameter blob has to carry too.
    ``fold_first``: layer 1's attention block is folded into the projection (amdrec_x3_weights.fold_attn1): its W_ov is
    not packed (mats["ov"][0] is not read; its scale reads 1.0).  ``cache_first_ffn`` (variant 16 with ``fold_first``):
    layer 1's stage-1 fragment sets are left out too (amdrec_x3_weights.stream_hc); every scale and bound stays."""
    assert variant in (16, 32, "16cs")                       # "16cs": the 16-row fragments in the column-split kernel's order
    assert not cache_first_ffn or (variant == 16 and fold_first)
    fr, sc = x3_split(mats, variant, fold_first)
    stream = x3_order(fr, variant, cache_first_ffn)
    return {"stream": stream, "chunks": stream.shape[0] // 16, **sc}


X3_PARAM_FLOATS = 11264     # LDS parameter area of the kernel (csrc/x3_common.hpp PARAM_FLOATS)


def pack_x3_params(layers: List[Dict], cross_b: List, head_b1, heads: List[Dict], fold_first: bool = False) -> np.ndarray:
    """The parameter blob of the row-owner kernel (layout: csrc/ranker_x3.hip x3_param_floats): per encoder layer
    [b_ov | gamma1 | beta1 | b_1 | b_2 | gamma2 | beta2], per cross layer its bias, heads [stacked b_1] then per task
    [b_2 (64) | w_3 (64) | b_3 padded to 4]; float32, zero-padded to a multiple of 1024.  ``fold_first``: layer 1's b_ov
    is in the folded projection bias and left out."""
    parts = []
    for i, L in enumerate(layers):
        parts += ([] if fold_first and i == 0 else [L["b_ov"]]) + [L["g1"], L["be1"], L["b1"], L["b2"], L["g2"], L["be2"]]
    parts += list(cross_b)
    parts.append(head_b1)
    for h in heads:
        parts += [h["b2"], h["w3"], np.concatenate([np.asarray(h["b3"], dtype=np.float64).reshape(-1), np.zeros(3)])]
    blob = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in parts]).astype(np.float32)
    return np.pad(blob, (0, -len(blob) % 1024))


def _pad_k(w64, mult=32):
    w = np.pad(w64.astype(np.float32), ((0, 0), (0, -w64.shape[1] % mult)))
    return w, w.shape[1]


class Packed:
    """Keeps the device tensors alive and hands out pointers."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._keep: List[torch.Tensor] = []

    def ptr(self, arr):
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
        assert t.data_ptr() % 16 == 0
        self._keep.append(t)
        return C.c_void_p(t.data_ptr())

    def vec(self, v64):
        return self.ptr(v64.astype(np.float32))

    def mat(self, w64, x6: bool = False):
        """float64 [out][K] -> pointer to the fp32 matrix (K zero-padded to 32), its leading dimension, pointer to its x6 planes"""
        w, ld = _pad_k(w64)
        return self.ptr(w), ld, (self.ptr(split_planes(w)) if x6 else None)


def pack_tables(pk: Packed, tables: List):
    emb_dim = int(tables[0].shape[1])
    if emb_dim < 4 or emb_dim & (emb_dim - 1):
        raise ValueError("embedding_dim must be a power of two >= 4 for the fused gather")
    cards = [int(t.shape[0]) for t in tables]
    off = np.concatenate([[0], np.cumsum(cards)[:-1]]).astype(np.int32)
    cat = np.concatenate([_np64(t).astype(np.float32) for t in tables], axis=0)
    assert cat.shape[1] == emb_dim
    return pk.ptr(cat), pk.ptr(off), pk.ptr(np.asarray(cards, dtype=np.int32)), emb_dim


def pack_tower(sd: Dict, prefix: str, feature_names: List[str], n_num: int, device, bn_eps=1e-5):
    """sd: state_dict-like (torch tensors or numpy) with the reference's key names under
    ``prefix`` ('user_tower' / 'ad_tower').  -> (TowerParams, Packed)"""
    pk = Packed(device)
    tables = [sd[f"{prefix}.embedding_layer.embeddings.{n}.weight"] for n in feature_names]
    p = TowerParams()
    p.tables, p.table_off, p.cards, emb_dim = pack_tables(pk, tables)
    p.n_feat, p.emb_dim, p.n_num = len(tables), emb_dim, n_num
    p.dims[0] = len(tables) * emb_dim + n_num
    idx, l = 0, 0
    while f"{prefix}.mlp.{idx}.weight" in sd:
        w = _np64(sd[f"{prefix}.mlp.{idx}.weight"])
        b = _np64(sd[f"{prefix}.mlp.{idx}.bias"])
        if f"{prefix}.mlp.{idx + 1}.running_mean" in sd:      # Linear followed by BatchNorm1d (eval)
            g = _np64(sd[f"{prefix}.mlp.{idx + 1}.weight"])
            be = _np64(sd[f"{prefix}.mlp.{idx + 1}.bias"])
            mu = _np64(sd[f"{prefix}.mlp.{idx + 1}.running_mean"])
            var = _np64(sd[f"{prefix}.mlp.{idx + 1}.running_var"])
            s = g / np.sqrt(var + bn_eps)
            w = w * s[:, None]
            b = (b - mu) * s + be
            idx += 4
        else:
            idx += 1
        if l >= MAX_LAYERS:
            raise ValueError("too many layers")
        if w.shape[0] % 4:
            raise ValueError("layer widths must be multiples of 4")
        p.w[l], p.ldw[l], _ = pk.mat(w)
        p.b[l], p.dims[l + 1] = pk.vec(b), w.shape[0]
        l += 1
    p.n_layers = l
    return p, pk


def x3_ineligible_reason(sd: Dict, fuse_attention: bool):
    """None if the row-owner engine (f16x3) can run this state dict - the architecture it is written for is the
    reference's default: d_model 256, heads 256 -> 64 -> 1 (transformer_ranker.py:213-224, :277-305) - else a short
    reason.  Other architectures (e.g. tutorial.ipynb cell 19: d_model 128) run the generic tile GEMMs."""
    if not fuse_attention:
        return "fuse_attention is off (the engine needs the pre-multiplied W_ov)"
    if "feature_projection.weight" not in sd:
        return "no feature_projection in the state dict"
    dm = int(sd["feature_projection.weight"].shape[0])
    if dm != 256:
        return f"d_model {dm} != 256"
    dff, c = [], 0
    while f"transformer_layers.{len(dff)}.norm1.weight" in sd:
        dff.append(int(sd[f"transformer_layers.{len(dff)}.feed_forward.fc1.weight"].shape[0]))
        if dff[-1] % 32:
            return f"d_ff {dff[-1]} is not a multiple of 32"
    while f"feature_interaction.cross_weights.{c}" in sd:
        c += 1
    tasks = [t for t in TASKS if f"prediction_heads.{t}.0.weight" in sd]
    if not tasks or len(tasks) > MAX_TASKS:
        return f"{len(tasks)} prediction heads (1 .. {MAX_TASKS} supported)"
    if 2 * len(dff) + c + 1 > 20:
        return f"{2 * len(dff) + c + 1} phases (at most 20)"
    h1 = int(sd[f"prediction_heads.{tasks[0]}.0.weight"].shape[0])
    h2 = int(sd[f"prediction_heads.{tasks[0]}.3.weight"].shape[0])
    if h1 % 32 or h2 != 64:
        return f"head widths {h1} -> {h2} (multiple of 32 -> 64 supported)"
    n_par = sum(6 * 256 + d for d in dff) + 256 * c + len(tasks) * (h1 + 132)
    if (n_par + 1023) // 1024 * 1024 > X3_PARAM_FLOATS:
        return f"{n_par} bias / LayerNorm parameters exceed the kernel's LDS parameter area ({X3_PARAM_FLOATS})"
    return None


def x3_eligible(sd: Dict, fuse_attention: bool) -> bool:
    return x3_ineligible_reason(sd, fuse_attention) is None


def x3c_available(p) -> bool:             # stream_cs is packed for: the architecture part of csrc/ranker_x3.hip x3c_available
    return p.x3.variant == 16 and (p.n_layers == 0 or p.d_ff % 128 == 0) and p.head_h1 % 128 == 0


def x3_hidden_cache(p) -> bool:           # stream_hc ... are packed for: the per-pack part of csrc/ranker_x3.hip x3_hidden_cache
    return bool(p.x3.fold_attn1 and p.x3.variant == 16 and p.w_proj_user and p.d_ff % 64 == 0)


# the reference TransformerRanker's eval-mode chain at seq_len 1, in float64 (fields: ``ranker_chain``)
RankerChain = NamedTuple("RankerChain", [("w_proj", np.ndarray), ("b_proj", np.ndarray), ("layers", List[Dict]), ("cross_wt", List),
                                         ("cross_b", List), ("head_w1", np.ndarray), ("head_b1", np.ndarray), ("heads", List[Dict]),
                                         ("tasks", List[str])])
_LAYER_KEYS = (("wv", "self_attention.W_v.weight"), ("bv", "self_attention.W_v.bias"), ("wo", "self_attention.W_o.weight"),
               ("bo", "self_attention.W_o.bias"), ("w1", "feed_forward.fc1.weight"), ("b1", "feed_forward.fc1.bias"),
               ("w2", "feed_forward.fc2.weight"), ("b2", "feed_forward.fc2.bias"), ("g1", "norm1.weight"),
               ("be1", "norm1.bias"), ("g2", "norm2.weight"), ("be2", "norm2.bias"))


def ranker_chain(sd) -> RankerChain:
    """The one reader of the reference's state dict (torch tensors or numpy): what pack_ranker, the x3 packers,
    ``folded_projection`` and ``first_ffn_cache`` multiply with (a RankerChain passes through, so those two take either).
    w_proj [d_model][K], b_proj = bias + positional_encoding[0, 0] (only row 0 is ever read, :361); per encoder layer wv bv wo
    bo w1 b1 w2 b2 g1 be1 g2 be2 and wov = W_o W_v, b_ov = W_o b_v + b_o (the seq-len-1 attention is exactly W_o (W_v x +
    b_v) + b_o, transformer_ranker.py:59-88 with :358); per cross layer W^T ([out][in]: xl @ W == xl (W^T)^T) and bias; layer
    1 of all heads stacked [T * h1][d_model]; per task w2 [h2][h1], b2, w3 [h2], b3 [1]."""
    if isinstance(sd, RankerChain):
        return sd
    layers, n_cross = [], 0
    while f"transformer_layers.{len(layers)}.norm1.weight" in sd:
        L = {dst: _np64(sd[f"transformer_layers.{len(layers)}.{src}"]) for dst, src in _LAYER_KEYS}
        L["wov"], L["b_ov"] = L["wo"] @ L["wv"], L["wo"] @ L["bv"] + L["bo"]
        layers.append(L)
    while f"feature_interaction.cross_weights.{n_cross}" in sd:
        n_cross += 1
    tasks = [t for t in TASKS if f"prediction_heads.{t}.0.weight" in sd]
    head = lambda t, k: _np64(sd[f"prediction_heads.{t}.{k}"])     # noqa: E731
    return RankerChain(
        _np64(sd["feature_projection.weight"]), _np64(sd["feature_projection.bias"]) + _np64(sd["positional_encoding"])[0, 0],
        layers, [_np64(sd[f"feature_interaction.cross_weights.{c}"]).T for c in range(n_cross)],
        [_np64(sd[f"feature_interaction.cross_biases.{c}"]) for c in range(n_cross)],
        np.concatenate([head(t, "0.weight") for t in tasks], axis=0), np.concatenate([head(t, "0.bias") for t in tasks], axis=0),
        [{"w2": head(t, "3.weight"), "b2": head(t, "3.bias"), "w3": head(t, "6.weight").reshape(-1),
          "b3": head(t, "6.bias").reshape(-1)} for t in tasks], tasks)


def _user_ad_columns(w, nu: int, na: int):
    """Projection-like [out][user emb | ad emb | numerical] -> its ([user emb | numerical], [ad emb]) column blocks."""
    return np.concatenate([w[:, :nu], w[:, nu + na:]], axis=1), w[:, nu:nu + na]


def folded_projection(sd: Dict):
    """float64 (W_p', b_p') of the feature projection with encoder layer 1's attention block folded in.  At seq_len 1
    everything of layer 1 before its first LayerNorm is linear in the projection output x0 = W_p f + b_p (b_p incl.
    pos[0]): z = x0 + W_ov x0 + b_ov = (I + W_ov) W_p f + (I + W_ov) b_p + b_ov, W_ov = W_o W_v, b_ov = W_o b_v + b_o."""
    ch = ranker_chain(sd)
    L = ch.layers[0]
    return ch.w_proj + L["wov"] @ ch.w_proj, ch.b_proj + L["wov"] @ ch.b_proj + L["b_ov"]


def first_ffn_cache(sd: Dict, n_user_cols: int, n_ad_cols: int, ln_eps: float = 1e-5, folded=None, lift=None) -> Dict:
    """float64 algebra of the first-FFN hidden cache (amdrec_x3_weights.stream_hc).  With layer 1's attention folded the
    chain starts with x1 = LN1(z), z = a_ad + u_user (the two halves of ``folded_projection``), and stage 1 of layer 1's
    FFN is linear in z once the row's deviation is known:

        W_1 x1 + b_1 = rstd * W_1c z + c,   W_1c = W_1 diag(gamma1) (I - 11^T / d),   c = W_1 beta1 + b_1

    (x1 = gamma1 * (z - mean(z)) * rstd + beta1; the centering matrix is folded into W_1c, so no mean term is ever
    subtracted: W_1c annihilates the constant vector).  W_1 is the fp32-rounded matrix the engines multiply with.
    -> {"w1c", "c", "w_ad" = W_1c W_p'[:, ad columns], "w_user" = W_1c W_p'[:, user | numerical columns],
        "b" = W_1c b_p'}: the stacked matrices produce P[ad] = w_ad . emb(ad) and Q[user] = w_user . f_user + b straight
    from the embeddings, composed in float64 (no second fp32 rounding through the cached a_ad).
    ``folded``: the ``folded_projection`` where the caller already has it.  ``lift``: layer 1's unit lifts of
    ``x3_rebalance`` [d_ff] - every row of the result is a hidden unit's and is multiplied with its power of two (exact), so
    that rstd * (P + Q) + c is the lifted hidden value the stream's W_2 columns were divided for."""
    ch = ranker_chain(sd)
    L = ch.layers[0]
    w1 = L["w1"].astype(np.float32).astype(np.float64)
    w1g = w1 * L["g1"][None, :]
    w1c = w1g - w1g.mean(axis=1, keepdims=True)
    wp, bp = folded_projection(ch) if folded is None else folded
    w_user, w_ad = _user_ad_columns(wp, n_user_cols, n_ad_cols)
    hc = {"w1c": w1c, "c": w1 @ L["be1"] + L["b1"], "w_ad": w1c @ w_ad, "w_user": w1c @ w_user, "b": w1c @ bp}
    if lift is not None:
        hc = {k: _scaled(v, lift if v.ndim == 1 else lift[:, None]) for k, v in hc.items()}
    return {**hc, "ln_eps": ln_eps}


def _pack_encoder_layer(L, pk: Packed, c: Dict, fuse_attention: bool, x6: bool):
    if fuse_attention:
        L.w_v, L.b_v = None, None
        L.w_o, L.ldw_dm, L.w_o_x6 = pk.mat(c["wov"], x6)
    else:
        L.b_v = pk.vec(c["bv"])
        L.w_v, L.ldw_dm, _ = pk.mat(c["wv"])
        L.w_o, L.ldw_dm, L.w_o_x6 = pk.mat(c["wo"], x6)
    L.w_1, L.ldw_dm, L.w_1_x6 = pk.mat(c["w1"], x6)
    L.b_o = pk.vec(c["b_ov"] if fuse_attention else c["bo"])
    L.w_2, L.ldw_ff, L.w_2_x6 = pk.mat(c["w2"], x6)
    for dst, src in (("b_1", "b1"), ("b_2", "b2"), ("ln1_g", "g1"), ("ln1_b", "be1"), ("ln2_g", "g2"), ("ln2_b", "be2")):
        setattr(L, dst, pk.vec(c[src]))


def _pack_x3(p: RankerParams, pk: Packed, ch: RankerChain, wproj, bproj, nu: int, na: int, cache_first_ffn: bool):
    """p.x3 (its variant, fold_attn1, min_rows and cs_max_rows are set): the SAME fp32-rounded matrices the other engines
    multiply with, split into fp16 planes once and laid out in the order of every stream this packing serves."""
    f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    fold = bool(p.x3.fold_attn1)
    mats = {"ov": [f32(L["wov"]) for L in ch.layers], "w1": [f32(L["w1"]) for L in ch.layers],
            "b1": [f32(L["b1"]) for L in ch.layers], "w2": [f32(L["w2"]) for L in ch.layers],
            "cross": [f32(w) for w in ch.cross_wt], "h1": f32(ch.head_w1), "hb1": f32(ch.head_b1),
            "h2": [f32(h["w2"]) for h in ch.heads]}
    fr, sc = x3_split(mats, p.x3.variant, fold)
    pk.x3_fragments = fr                                        # for ``pack_ctr_first``, which orders this same split again

    def stream(kind, **kw):
        s = x3_order(fr, kind, **kw)
        return pk.ptr(s.view(np.int16)), s.shape[0] // 16
    # the parameters that multiply with rebalanced hidden units take the units' factors (``x3_rebalance``)
    lift = sc["lift"]
    layers = [dict(L, b1=_scaled(L["b1"], f)) for L, f in zip(ch.layers, lift["w1"])]
    heads = [dict(h, b2=_scaled(h["b2"], f), w3=_scaled(h["w3"], 1.0 / f)) for h, f in zip(ch.heads, lift["h2"])]
    blob = pack_x3_params(layers, ch.cross_b, _scaled(ch.head_b1, lift["h1"]), heads, fold_first=fold)
    assert len(blob) <= X3_PARAM_FLOATS
    p.x3.params, p.x3.n_params = pk.ptr(blob), len(blob)
    p.x3.stream, p.x3.chunks = stream(p.x3.variant)
    if p.x3.cs_max_rows >= 0 and x3c_available(p):
        p.x3.stream_cs, p.x3.chunks_cs = stream("16cs")         # the same fragments in the column-split kernel's chunk order
    if cache_first_ffn and x3_hidden_cache(p):
        hc = first_ffn_cache(ch, nu, na, folded=(wproj, bproj), lift=lift["w1"][0])
        p.x3.stream_hc, p.x3.chunks_hc = stream(16, cache_first_ffn=True)
        blob_hc = blob.copy()                                   # folded layout: [gamma1 | beta1 | b_1 ...] - c in b_1's place
        blob_hc[512:512 + len(hc["c"])] = hc["c"].astype(np.float32)
        p.x3.params_hc = pk.ptr(blob_hc)
        p.x3.w_user_uq, ldu, _ = pk.mat(np.concatenate([_user_ad_columns(wproj, nu, na)[0], hc["w_user"]]))
        p.x3.b_user_uq = pk.vec(np.concatenate([bproj, hc["b"]]))
        p.x3.w_hidden_ad, lda, _ = pk.mat(hc["w_ad"])
        assert ldu == p.ldw_proj_user and lda == p.ldw_proj_ad
    for dst in ("sw_ov", "sw_1", "sw_2", "hn", "hb", "sw_cross"):
        for i, v in enumerate(sc[dst]):
            getattr(p.x3, dst)[i] = v
    p.x3.sw_h1, p.x3.sw_h2, p.x3.hn_head, p.x3.hb_head = sc["sw_h1"], sc["sw_h2"], sc["hn_head"], sc["hb_head"]


def ctr_first_packable(p: RankerParams) -> bool:
    """The architecture part of csrc/ranker_x3.hip ranker_x3_ctr_first_supported: the 16-row engine is packed and there are
    tasks behind task 0."""
    return bool(p.x3.stream) and p.x3.variant == 16 and p.n_tasks >= 2


def pack_ctr_first(p: RankerParams, pk: Packed) -> bool:
    """Upload the streams of CTR-first ranking (amdrec_x3_weights.stream_ctr ... stream_win_cs) for a ranker packed by
    ``pack_ranker``, once, on the mode's first use: ~25 MB of device memory that a ranker which never uses the mode does not
    pay.  They are further orderings of the split ``pack_ranker`` made (``pk.x3_fragments``), one per stream the packing
    already serves; every other field of ``p`` - the existing streams, scales, bounds and parameter blobs - is untouched.
    -> whether the streams are there."""
    if p.x3.stream_ctr:
        return True
    fr = getattr(pk, "x3_fragments", None)
    if fr is None or not ctr_first_packable(p):
        return False
    for stem, kw in x3_ctr_first_orders(p.n_tasks, bool(p.x3.stream_cs), bool(p.x3.stream_hc)).items():
        s = x3_order(fr, **kw)
        setattr(p.x3, "stream_" + stem, pk.ptr(s.view(np.int16)))
        setattr(p.x3, "chunks_" + stem, s.shape[0] // 16)
    return True


def pack_ranker(sd: Dict, user_names: List[str], ad_names: List[str], n_num: int, device, ln_eps=1e-5,
                fuse_attention: bool = True, x6: bool = True, x3: bool = False, x3_min_rows: int = 0,
                x3_variant: int = 32, x3_cs_max_rows: int = 0, fold_first_attention: bool = False,
                cache_first_ffn: bool = False, x3_products: int = 3):
    """state_dict-like of the reference TransformerRanker -> (RankerParams, Packed, task names).
    ``fuse_attention``: pre-multiply W_ov = W_o W_v, b_ov = W_o b_v + b_o in float64 (``ranker_chain``), so each encoder layer's
    attention block is one GEMM instead of two.
    ``x6``: also upload the bf16 split planes of the big weight matrices (W_ov / W_o, fc1, fc2, cross, stacked head layer 1) so
    that passes of more than 8192 rows run on the error-compensated bf16-MFMA GEMM.
    ``x3``: also pack the row-owner engine's streams where ``x3_ineligible_reason`` is None (else it has no effect).
    ``fold_first_attention``: when every pass runs the row-owner engine (x3 packed, x3_min_rows == 1, at least one encoder
    layer), pack the projection as ``folded_projection`` (rounded once to fp32) and the engine's chain without layer 1's
    W_ov / b_ov (amdrec_x3_weights.fold_attn1); otherwise it has no effect.
    ``cache_first_ffn``: with the fold on the 16-row kernel, also pack what the first-FFN hidden cache needs (``first_ffn_cache``;
    amdrec_x3_weights.stream_hc ...); otherwise it has no effect.
    ``x3_products``: 3, or 1 for the single-product engine (amdrec_x3_weights.products): the same streams, scales and blobs,
    read by the kernels that multiply the high planes alone.  Needs ``x3_variant`` 16 and ``x3_min_rows`` 1 - a ranker that
    is half precision for some batch sizes and fp32 for others is a trap - and changes nothing where x3 is not packed."""
    if int(x3_products) not in (1, 3):
        raise ValueError("x3_products must be 3 or 1")
    if x3 and int(x3_products) == 1 and int(x3_variant) != 16:
        raise ValueError(f"the single-product engine runs on the 16-row kernels only (x3_variant {x3_variant})")
    if x3 and int(x3_products) == 1 and int(x3_min_rows) != 1:
        raise ValueError(f"the single-product engine runs every pass or none (x3_min_rows {x3_min_rows}, must be 1)")
    pk = Packed(device)
    tables = [sd[f"user_embeddings.{n}.weight"] for n in user_names] + \
             [sd[f"ad_embeddings.{n}.weight"] for n in ad_names]
    p = RankerParams()
    p.tables, p.table_off, p.cards, emb_dim = pack_tables(pk, tables)
    ch = ranker_chain(sd)
    if len(ch.layers) > MAX_LAYERS:
        raise ValueError(f"at most {MAX_LAYERS} encoder layers are supported (num_layers > {MAX_LAYERS})")
    x3 = bool(x3) and x3_eligible(sd, fuse_attention)
    fold = bool(fold_first_attention and x3 and int(x3_min_rows) == 1 and ch.layers)
    wproj, bproj = folded_projection(ch) if fold else (ch.w_proj, ch.b_proj)
    assert wproj.shape[1] == len(tables) * emb_dim + n_num
    p.n_user_feat, p.n_ad_feat, p.emb_dim, p.n_num = len(user_names), len(ad_names), emb_dim, n_num
    p.d_model, p.ln_eps = wproj.shape[0], ln_eps
    p.w_proj, p.ldw_proj, _ = pk.mat(wproj)
    nu, na = len(user_names) * emb_dim, len(ad_names) * emb_dim
    if nu + n_num > 0 and na > 0:                                   # split for the broadcast form
        w_user, w_ad = _user_ad_columns(wproj, nu, na)
        p.w_proj_user, p.ldw_proj_user, _ = pk.mat(w_user)
        p.w_proj_ad, p.ldw_proj_ad, _ = pk.mat(w_ad)
    p.b_proj = pk.vec(bproj)
    for l, c in enumerate(ch.layers):
        _pack_encoder_layer(p.layers[l], pk, c, fuse_attention, x6)
    p.n_layers, p.n_cross, p.n_tasks = len(ch.layers), len(ch.cross_wt), len(ch.tasks)
    p.d_ff = ch.layers[-1]["w1"].shape[0] if ch.layers else 4      # 4: placeholder (ranker_check wants d_ff >= 4), never read
    for c, (w, b) in enumerate(zip(ch.cross_wt, ch.cross_b)):
        p.cross_wt[c], p.ldw_cross, p.cross_wt_x6[c] = pk.mat(w, x6)
        p.cross_b[c] = pk.vec(b)
    p.head_h1, p.head_h2 = ch.head_w1.shape[0] // len(ch.tasks), ch.heads[0]["w2"].shape[0]
    p.head_w1, p.ldw_head1, p.head_w1_x6 = pk.mat(ch.head_w1, x6)
    p.head_b1 = pk.vec(ch.head_b1)
    for i, h in enumerate(ch.heads):
        p.head_w2[i], p.ldw_head2, _ = pk.mat(h["w2"])
        p.head_b2[i], p.head_w3[i], p.head_b3[i] = pk.vec(h["b2"]), pk.vec(h["w3"]), pk.vec(h["b3"])
    if x3:
        p.x3.variant, p.x3.fold_attn1 = x3_variant, int(fold)
        p.x3.min_rows, p.x3.cs_max_rows = int(x3_min_rows), int(x3_cs_max_rows)
        _pack_x3(p, pk, ch, wproj, bproj, nu, na, cache_first_ffn)
        p.x3.products = int(x3_products) if int(x3_products) == 1 else 0      # (0: what packs have always carried)
    return p, pk, ch.tasks
