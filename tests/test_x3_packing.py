"""CPU test of the fp16x3 weight-stream packer (amdrec/weights.py) against a numpy emulation of how the row-owner
kernel consumes it (csrc/rowowner.hpp): fragment sets are read strictly in stream order by loops that mirror
gemm256 / ffn_step / phase_heads, the B operand is built from the accumulator layout exactly as split8 does, and an
MFMA is emulated by its lane semantics  D[p][q] += sum_{half, j} A[lane p + 32 half][j] * B[lane q + 32 half][j].
If the k permutation or the stream order of the packer and the kernel disagree, the emulated chain is wrong."""
import numpy as np

import oracle
from amdrec import synth, weights
from tests import cases

F = np.float64


def _acc_layout_feature(i, r, h):
    return 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h


class Stream:
    def __init__(self, frags):
        self.f = frags.view(np.float16).astype(F)      # [n][64][8]
        self.pos = 0

    def read(self, n):
        out = self.f[self.pos:self.pos + n]
        self.pos += n
        return out


def _b_frags(x):
    """rows x [q][256] (real values, already 'scaled') -> B fragments [16 ks][64 lanes][8] from the accumulator layout:
    lane (q, h) element j of k-step 2 i + s = register 8 s + j of tile i."""
    q_n = x.shape[0]
    assert q_n == 32
    out = np.zeros((16, 64, 8), F)
    for i in range(8):
        for sp in range(2):
            for h in range(2):
                for j in range(8):
                    out[2 * i + sp, 32 * h:32 * h + 32, j] = x[:, _acc_layout_feature(i, 8 * sp + j, h)]
    return out


def _mfma(a, b):
    """a, b: [64][8] fragments -> D [32 p][32 q]"""
    d = np.zeros((32, 32), F)
    for h in range(2):
        d += a[32 * h:32 * h + 32] @ b[32 * h:32 * h + 32].T
    return d


def _tile_to_rows(acc_tiles):
    """list of D tiles [32 p][32 q] (tile i = features 32 i ..) -> rows [q][32 * n]"""
    return np.concatenate([t.T for t in acc_tiles], axis=1)


def _gemm256(st, xb):
    acc = [np.zeros((32, 32), F) for _ in range(8)]
    for ks in range(16):
        for ip in range(4):
            cur = st.read(4)
            for k, i in enumerate((2 * ip, 2 * ip + 1)):
                acc[i] += _mfma(cur[2 * k] + cur[2 * k + 1], xb[ks])      # planes recombined: (ah + al) . b
    return _tile_to_rows(acc)


def _ffn(st, xb, T, b1, relu_scale=1.0):
    acc2 = [np.zeros((32, 32), F) for _ in range(8)]
    hb = None
    for t in range(T + 1):
        acc1 = np.zeros((32, 32), F)
        for u in range(16):
            if t < T:
                a = st.read(2)
                acc1 += _mfma(a[0] + a[1], xb[u])
            if t >= 1:
                a = st.read(2)
                acc2[u & 7] += _mfma(a[0] + a[1], hb[u >> 3])
        if t < T:
            hrows = np.maximum(acc1.T + b1[32 * t:32 * t + 32][None, :], 0) * relu_scale     # [q][32 hidden], natural order
            # hidden tile in accumulator layout -> its two B fragments (registers 0..7, 8..15)
            hb = np.zeros((2, 64, 8), F)
            for sp in range(2):
                for h in range(2):
                    for j in range(8):
                        hb[sp, 32 * h:32 * h + 32, j] = hrows[:, _acc_layout_feature(0, 8 * sp + j, h)]
    return _tile_to_rows(acc2)


def test_stream_order_and_k_permutation_match_the_kernel_loops():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, tasks = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3=True)
    assert p.x3.stream and p.x3.chunks == 3 * (16 + 128) + 3 * 16 + 60
    stream = None
    for t in pk._keep:
        if t.data_ptr() == p.x3.stream:
            stream = t.numpy().view(np.uint16).reshape(-1, 64, 8)
    assert stream is not None and stream.shape[0] == p.x3.chunks * 16
    st = Stream(stream)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((32, 256))
    f64 = lambda k: np.asarray(sd[k], dtype=F)     # noqa: E731
    for l in range(3):
        pre = f"transformer_layers.{l}"
        wov = (f64(pre + ".self_attention.W_o.weight") @ f64(pre + ".self_attention.W_v.weight")).astype(np.float32).astype(F)
        got = _gemm256(st, _b_frags(x)) / p.x3.sw_ov[l]
        assert np.abs(got - x @ wov.T).max() <= 1e-5 * np.abs(x @ wov.T).max(), ("ov", l)
        w1, b1, w2 = f64(pre + ".feed_forward.fc1.weight"), f64(pre + ".feed_forward.fc1.bias"), f64(pre + ".feed_forward.fc2.weight")
        got = _ffn(st, _b_frags(x), 32, b1 * p.x3.sw_1[l]) / (p.x3.sw_1[l] * p.x3.sw_2[l])
        ref = np.maximum(x @ w1.T + b1, 0) @ w2.T
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), ("ffn", l)
        # the hidden bound really bounds the hidden activations of these rows
        hid = np.maximum(x @ w1.T + b1, 0)
        assert (hid.max(axis=1) <= p.x3.hn[l] * np.abs(x).max(axis=1) + p.x3.hb[l]).all()
    for c in range(3):
        wc = f64(f"feature_interaction.cross_weights.{c}")
        got = _gemm256(st, _b_frags(x)) / p.x3.sw_cross[c]
        assert np.abs(got - x @ wc).max() <= 1e-5 * np.abs(x @ wc).max(), ("cross", c)
    xb = _b_frags(x)
    for ti, t in enumerate(tasks):
        w1, b1 = f64(f"prediction_heads.{t}.0.weight"), f64(f"prediction_heads.{t}.0.bias")
        w2 = f64(f"prediction_heads.{t}.3.weight")
        acc2 = [np.zeros((32, 32), F) for _ in range(2)]
        for tt in range(8):
            acc1 = np.zeros((32, 32), F)
            for u in range(16):
                a = st.read(2)
                acc1 += _mfma(a[0] + a[1], xb[u])
            hrows = np.maximum(acc1.T / p.x3.sw_h1 + b1[32 * tt:32 * tt + 32][None, :], 0)
            hb = np.zeros((2, 64, 8), F)
            for sp in range(2):
                for h in range(2):
                    for j in range(8):
                        hb[sp, 32 * h:32 * h + 32, j] = hrows[:, _acc_layout_feature(0, 8 * sp + j, h)]
            for sp in range(2):
                a = st.read(4)
                acc2[0] += _mfma(a[0] + a[1], hb[sp])
                acc2[1] += _mfma(a[2] + a[3], hb[sp])
        got = _tile_to_rows(acc2) / p.x3.sw_h2
        ref = np.maximum(x @ w1.T + b1, 0) @ w2.T
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), ("head", t)
    assert st.pos == stream.shape[0]                 # the whole stream was consumed, nothing left over


def test_plane_split_is_22_bit_accurate_and_in_fp16_range():
    rng = np.random.default_rng(1)
    w = rng.standard_normal((64, 32)) * 10.0 ** rng.uniform(-6, 2, (64, 32))
    s = weights.x3_pow2_scale(np.abs(w).max())
    assert 2 ** 12 <= np.abs(w).max() * s < 2 ** 13 and np.log2(s) == int(np.log2(s))
    fr = weights.x3_frags(w.astype(np.float32).astype(np.float64), s).view(np.float16).astype(np.float64)
    assert np.isfinite(fr).all()
    # undo the fragment layout: tile, ks, plane, lane = p + 32 half, j  ->  W[32 tile + p][16 ks + src(8 half + j)]
    rec = np.zeros((64, 32))
    for tile in range(2):
        for ks in range(2):
            for lane in range(64):
                for j in range(8):
                    pos = 8 * (lane >> 5) + j
                    src = (pos & 3) | (((pos >> 3) & 1) << 2) | (((pos >> 2) & 1) << 3)
                    rec[32 * tile + (lane & 31), 16 * ks + src] = fr[tile, ks, 0, lane, j] + fr[tile, ks, 1, lane, j]
    w32 = w.astype(np.float32).astype(np.float64)
    err = np.abs(rec / s - w32)
    big = np.abs(w32) * s >= 2.0 ** -3                   # elements whose low plane is a normal fp16 number
    assert (err[big] <= 2.0 ** -22 * np.abs(w32[big])).all()
    assert (err[~big] <= 2.0 ** -25 / s).all()


# ---- the 16-rows-per-wave variant (csrc/rowowner16.hpp): v_mfma_f32_16x16x32_f16 lane semantics --------------------
def _b16(x):
    """rows x [16 q][256] -> B fragments [8 ks][64 lanes][8]: lane (q, g) element j = x[2 ks + (j >> 2)][j & 3] with
    tile T register r = feature 16 T + 4 g + r"""
    out = np.zeros((8, 64, 8), F)
    for ks in range(8):
        for g in range(4):
            for j in range(8):
                out[ks, 16 * g:16 * g + 16, j] = x[:, 16 * (2 * ks + (j >> 2)) + 4 * g + (j & 3)]
    return out


def _mfma16(a, b):
    d = np.zeros((16, 16), F)
    for g in range(4):
        d += a[16 * g:16 * g + 16] @ b[16 * g:16 * g + 16].T
    return d


def _hidden16(h32):
    """hidden rows [16 q][32] (natural feature order) -> the single B fragment [64][8] of their k-step"""
    out = np.zeros((64, 8), F)
    for g in range(4):
        for j in range(8):
            out[16 * g:16 * g + 16, j] = h32[:, 16 * (j >> 2) + 4 * g + (j & 3)]
    return out


def _group(st, b, acc, t0):
    a = st.read(4)
    acc[t0] += _mfma16(a[0] + a[1], b)
    acc[t0 + 1] += _mfma16(a[2] + a[3], b)


def test_16_row_variant_stream_order_and_k_permutation():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, tasks = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3=True, x3_variant=16)
    assert p.x3.variant == 16 and p.x3.chunks == 3 * (16 + 128) + 3 * 16 + 60
    stream = [t for t in pk._keep if t.data_ptr() == p.x3.stream][0].numpy().view(np.uint16).reshape(-1, 64, 8)
    st = Stream(stream)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((16, 256))
    f64 = lambda k: np.asarray(sd[k], dtype=F)     # noqa: E731
    rows = lambda acc: np.concatenate([t.T for t in acc], axis=1)     # noqa: E731

    def gemm256():
        acc = [np.zeros((16, 16), F) for _ in range(16)]
        xb = _b16(x)
        for ks in range(8):
            for tp in range(8):
                _group(st, xb[ks], acc, 2 * tp)
        return rows(acc)

    for l in range(3):
        pre = f"transformer_layers.{l}"
        wov = (f64(pre + ".self_attention.W_o.weight") @ f64(pre + ".self_attention.W_v.weight")).astype(np.float32).astype(F)
        got = gemm256() / p.x3.sw_ov[l]
        assert np.abs(got - x @ wov.T).max() <= 1e-5 * np.abs(x @ wov.T).max(), ("ov", l)
        w1, b1, w2 = f64(pre + ".feed_forward.fc1.weight"), f64(pre + ".feed_forward.fc1.bias"), f64(pre + ".feed_forward.fc2.weight")
        acc2 = [np.zeros((16, 16), F) for _ in range(16)]
        xb, hb = _b16(x), None
        for t in range(33):
            a1 = [np.zeros((16, 16), F), np.zeros((16, 16), F)]
            for u in range(8):
                if t < 32:
                    _group(st, xb[u], a1, 0)
                if t >= 1:
                    _group(st, hb, acc2, 2 * u)
            if t < 32:
                hb = _hidden16(np.maximum(rows(a1) / p.x3.sw_1[l] + b1[32 * t:32 * t + 32][None, :], 0))
        got = rows(acc2) / p.x3.sw_2[l]
        ref = np.maximum(x @ w1.T + b1, 0) @ w2.T
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), ("ffn", l)
    def gemm256_quarters():                 # the cross layers' order: four quarters of the output tiles, k-step major inside
        acc = [np.zeros((16, 16), F) for _ in range(16)]
        xb = _b16(x)
        for q4 in range(4):
            for ks in range(8):
                for pr in range(2):
                    _group(st, xb[ks], acc, 2 * (2 * q4 + pr))
        return rows(acc)

    for c in range(3):
        wc = f64(f"feature_interaction.cross_weights.{c}")
        got = gemm256_quarters() / p.x3.sw_cross[c]
        assert np.abs(got - x @ wc).max() <= 1e-5 * np.abs(x @ wc).max(), ("cross", c)
    # heads, pipelined: step tt = stage 1 of hidden tile tt (through all tasks) with stage 2 of tile tt - 1 behind u = 3, 7
    xb = _b16(x)
    T, nt = 8, 8 * len(tasks)
    acc2 = {t: [np.zeros((16, 16), F) for _ in range(4)] for t in tasks}
    hb = None
    for tt in range(nt + 1):
        a1 = [np.zeros((16, 16), F), np.zeros((16, 16), F)]
        for u in range(8):
            if tt < nt:
                _group(st, xb[u], a1, 0)
            if tt >= 1 and u in (3, 7):
                _group(st, hb, acc2[tasks[(tt - 1) // T]], 2 * (u // 4))
        if tt < nt:
            b1 = f64(f"prediction_heads.{tasks[tt // T]}.0.bias")
            hb = _hidden16(np.maximum(rows(a1) / p.x3.sw_h1 + b1[32 * (tt % T):32 * (tt % T) + 32][None, :], 0))
    for t in tasks:
        w1, b1, w2 = f64(f"prediction_heads.{t}.0.weight"), f64(f"prediction_heads.{t}.0.bias"), f64(f"prediction_heads.{t}.3.weight")
        got = rows(acc2[t]) / p.x3.sw_h2
        ref = np.maximum(x @ w1.T + b1, 0) @ w2.T
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), ("head", t)
    assert st.pos == stream.shape[0]


def test_parameter_blob_layout_matches_the_kernels_offsets():
    """pack_x3_params vs the offsets csrc/ranker_x3.hip x3_build derives from the architecture."""
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, tasks = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3=True)
    blob = [t for t in pk._keep if t.data_ptr() == p.x3.params][0].numpy()
    assert len(blob) == p.x3.n_params == 10240 and len(blob) % 1024 == 0
    o = 0
    for l in range(3):
        pre = f"transformer_layers.{l}"
        assert np.array_equal(blob[o + 256:o + 512], sd[pre + ".norm1.weight"])
        assert np.array_equal(blob[o + 768:o + 768 + 1024], sd[pre + ".feed_forward.fc1.bias"])
        assert np.array_equal(blob[o + 768 + 1024 + 512:o + 768 + 1024 + 768], sd[pre + ".norm2.bias"])
        o += 1536 + 1024
    for c in range(3):
        assert np.array_equal(blob[o:o + 256], sd[f"feature_interaction.cross_biases.{c}"])
        o += 256
    assert np.array_equal(blob[o:o + 256], sd["prediction_heads.ctr.0.bias"])
    o += 768
    for t in tasks:
        assert np.array_equal(blob[o:o + 64], sd[f"prediction_heads.{t}.3.bias"])
        assert np.array_equal(blob[o + 64:o + 128], sd[f"prediction_heads.{t}.6.weight"].reshape(-1))
        assert blob[o + 128] == sd[f"prediction_heads.{t}.6.bias"][0]
        o += 132
    assert not blob[o:].any()


# ---- the column-split kernel (csrc/rowowner16c.hpp): every chunk = one group per wave ------------------------------
def test_column_split_stream_gives_every_wave_its_group_in_every_chunk():
    """Host emulation of the kernel's loops, wave by wave: chunk c = 16 fragment sets, wave w multiplies sets 4 w .. 4 w + 3.
    gemm256: wave w accumulates output tiles 4 w .. 4 w + 3; FFN / heads: super-steps of four hidden steps, one per wave, stage
    2 of super-step T - 1 interleaved behind stage 1 of T; heads' stage 2 on waves 0, 1 (zeros for 2, 3)."""
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, tasks = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x3=True, x3_variant=16)
    assert p.x3.chunks_cs == 3 * (16 + 128) + 3 * 16 + 3 * 8 * 3 and p.x3.cs_max_rows == 0
    stream = [t for t in pk._keep if t.data_ptr() == p.x3.stream_cs][0].numpy().view(np.uint16).reshape(-1, 64, 8)
    assert stream.shape[0] == p.x3.chunks_cs * 16
    st = Stream(stream)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16, 256))
    f64 = lambda k: np.asarray(sd[k], dtype=F)     # noqa: E731
    rows = lambda acc: np.concatenate([t.T for t in acc], axis=1)     # noqa: E731

    def chunk(bs, accs, t0s):
        """one chunk: wave w's group against its B fragment bs[w] into accs[w][t0s[w]], [t0s[w] + 1] (None: no work)"""
        a = st.read(16)
        for w in range(4):
            if accs[w] is None:
                assert not a[4 * w:4 * w + 4].any()          # zero fragments for a wave without work
                continue
            accs[w][t0s[w]] += _mfma16(a[4 * w] + a[4 * w + 1], bs[w])
            accs[w][t0s[w] + 1] += _mfma16(a[4 * w + 2] + a[4 * w + 3], bs[w])

    def gemm256():
        acc = [np.zeros((16, 16), F) for _ in range(16)]
        xb = _b16(x)
        for ks in range(8):
            for j in range(2):
                chunk([xb[ks]] * 4, [acc] * 4, [4 * w + 2 * j for w in range(4)])
        return rows(acc)

    for l in range(3):
        pre = f"transformer_layers.{l}"
        wov = (f64(pre + ".self_attention.W_o.weight") @ f64(pre + ".self_attention.W_v.weight")).astype(np.float32).astype(F)
        got = gemm256() / p.x3.sw_ov[l]
        assert np.abs(got - x @ wov.T).max() <= 1e-5 * np.abs(x @ wov.T).max(), ("ov", l)
        w1, b1, w2 = f64(pre + ".feed_forward.fc1.weight"), f64(pre + ".feed_forward.fc1.bias"), f64(pre + ".feed_forward.fc2.weight")
        acc2 = [np.zeros((16, 16), F) for _ in range(16)]
        xb = _b16(x)
        hid = {}
        for T in range(9):
            a1 = [[np.zeros((16, 16), F), np.zeros((16, 16), F)] for _ in range(4)]
            for i in range(8):
                if T < 8:
                    chunk([xb[i]] * 4, a1, [0] * 4)
                if T >= 1:
                    chunk([hid[T - 1][i >> 1]] * 4, [acc2] * 4, [4 * w + 2 * (i & 1) for w in range(4)])
            if T < 8:
                hid[T] = [_hidden16(np.maximum(rows(a1[w]) / p.x3.sw_1[l] + b1[32 * (4 * T + w):32 * (4 * T + w) + 32][None, :], 0))
                          for w in range(4)]
        got = rows(acc2) / p.x3.sw_2[l]
        ref = np.maximum(x @ w1.T + b1, 0) @ w2.T
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), ("ffn", l)
    for c in range(3):
        wc = f64(f"feature_interaction.cross_weights.{c}")
        got = gemm256() / p.x3.sw_cross[c]
        assert np.abs(got - x @ wc).max() <= 1e-5 * np.abs(x @ wc).max(), ("cross", c)
    xb = _b16(x)
    Tt, S = 8, 8 * len(tasks) // 4
    acc2 = {t: [np.zeros((16, 16), F) for _ in range(4)] for t in tasks}
    hid = {}
    for ss in range(S + 1):
        a1 = [[np.zeros((16, 16), F), np.zeros((16, 16), F)] for _ in range(4)]
        for i in range(8):
            if ss < S:
                chunk([xb[i]] * 4, a1, [0] * 4)
            if ss >= 1 and (i & 3) == 3:
                task = tasks[4 * (ss - 1) // Tt]
                for kk in (2 * (i >> 2), 2 * (i >> 2) + 1):
                    chunk([hid[ss - 1][kk]] * 4, [acc2[task], acc2[task], None, None], [0, 2, 0, 0])
        if ss < S:
            hid[ss] = []
            for w in range(4):
                tt = 4 * ss + w
                b1 = f64(f"prediction_heads.{tasks[tt // Tt]}.0.bias")
                hid[ss].append(_hidden16(np.maximum(rows(a1[w]) / p.x3.sw_h1 + b1[32 * (tt % Tt):32 * (tt % Tt) + 32][None, :], 0)))
    for t in tasks:
        w1, b1, w2 = f64(f"prediction_heads.{t}.0.weight"), f64(f"prediction_heads.{t}.0.bias"), f64(f"prediction_heads.{t}.3.weight")
        got = rows(acc2[t]) / p.x3.sw_h2
        ref = np.maximum(x @ w1.T + b1, 0) @ w2.T
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), ("head", t)
    assert st.pos == stream.shape[0]
    # the 16-row kernel's stream holds the same fragment sets (the column-split one adds only zero sets)
    base = [t for t in pk._keep if t.data_ptr() == p.x3.stream][0].numpy().view(np.uint16).reshape(-1, 64 * 8)
    nz = stream.reshape(-1, 64 * 8)
    nz = nz[nz.any(axis=1)]
    key = lambda a: np.sort(np.ascontiguousarray(a).view([("", a.dtype)] * a.shape[1]).ravel())    # noqa: E731
    assert (key(base[base.any(axis=1)]) == key(nz)).all()


# ---- one split per matrix, one fold per pack ------------------------------------------------------------------------
def _count_calls(monkeypatch, name):
    calls, fn = [], getattr(weights, name)
    monkeypatch.setattr(weights, name, lambda *a, **k: (calls.append(name), fn(*a, **k))[1])
    return calls


def test_every_matrix_is_plane_split_once_however_many_streams_are_packed(monkeypatch):
    """The main, column-split and hidden-cache streams are three orderings of ONE set of fragments: a pack splits each of its
    (L - 1 folded | L) + 2 L + C + 1 + T matrices (W_ov, W_1 and W_2 per layer, cross, stacked head layer 1, head layer 2 per
    task; L = C = T = 3) exactly once."""
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    kw = dict(x6=False, x3=True, x3_variant=16, x3_min_rows=1)
    calls = _count_calls(monkeypatch, "x3b_frags")
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", fold_first_attention=True, cache_first_ffn=True, **kw)
    assert p.x3.stream and p.x3.stream_cs and p.x3.stream_hc                   # three streams
    assert len(calls) == (3 - 1) + 2 * 3 + 3 + 1 + 3 == 15
    del calls[:]
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", **kw)
    assert p.x3.stream and p.x3.stream_cs and not p.x3.stream_hc               # two streams
    assert len(calls) == 3 + 2 * 3 + 3 + 1 + 3 == 16


def test_the_projection_is_folded_once_per_pack(monkeypatch):
    """The folded projection feeds the packed projection AND the first-FFN hidden cache: computed once, handed on."""
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    calls = _count_calls(monkeypatch, "folded_projection")
    p, _, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=16, x3_min_rows=1,
                                  fold_first_attention=True, cache_first_ffn=True)
    assert p.x3.fold_attn1 == 1 and p.x3.stream_hc and len(calls) == 1
