"""CPU: the host side of CTR-first ranking (AdRecommenderInference ``heads="ctr_first"``): the task-windowed weight
streams are cuts of the existing ones, the lazy packer adds them without touching what is packed, the ABI carries the new
entries under the unchanged version, and the constructor refuses an unknown mode."""
import ctypes as C
import inspect

import numpy as np
import pytest

from amdrec import _lib, weights
from tests import cases

N_LAYERS, D_FF, N_CROSS, N_TASKS, TILES = 3, 1024, 3, 3, 8           # the reference architecture: heads 256 -> 64 -> 1
ORDERINGS = [(16, False), ("16cs", False), (16, True)]               # main, column-split, hidden-cache


def _labelled(n_tiles, n_ks, counter):
    """Fragments [tile][k-step][plane][64][8] whose every fragment set carries one label of its own (> 0: the column-split
    streams pad with all-zero sets)."""
    a = np.zeros((n_tiles, n_ks, 2, 64, 8), np.uint16)
    for t in range(n_tiles):
        for k in range(n_ks):
            for p in range(2):
                counter[0] += 1
                a[t, k, p] = counter[0]
    return a


@pytest.fixture(scope="module")
def fr():
    """What ``x3_split`` returns for the reference architecture with layer 1's attention folded, labels for bits."""
    n = [0]
    d = {"tiles": TILES,
         "ov": [None] + [_labelled(16, 8, n) for _ in range(N_LAYERS - 1)],
         "w1": [_labelled(D_FF // 16, 8, n) for _ in range(N_LAYERS)],
         "w2": [_labelled(16, D_FF // 32, n) for _ in range(N_LAYERS)],
         "cross": [_labelled(16, 8, n) for _ in range(N_CROSS)]}
    d["h1"] = _labelled(N_TASKS * TILES * 2, 8, n)                    # stacked over tasks: 16-feature tiles, 2 per hidden tile
    d["h2"] = [_labelled(4, TILES, n) for _ in range(N_TASKS)]
    assert n[0] < 65536
    return d


def _labels(stream):
    assert all((s == s[0, 0]).all() for s in stream[::97])            # a fragment set is one label throughout
    return stream[:, 0, 0].astype(np.int64)


def _task_labels(fr, task):
    stage1 = fr["h1"][task * TILES * 2:(task + 1) * TILES * 2]
    return set(np.unique(stage1)) | set(np.unique(fr["h2"][task]))


@pytest.mark.parametrize("kind,hc", ORDERINGS)
def test_ctr_first_and_winner_streams_are_cuts_of_the_existing_stream(fr, kind, hc):
    full = _labels(weights.x3_order(fr, kind, cache_first_ffn=hc))
    ctr = _labels(weights.x3_order(fr, kind, cache_first_ffn=hc, tasks=(0, 1)))
    win = _labels(weights.x3_order(fr, kind, tasks=(1, N_TASKS - 1), trunk=False))
    head_labels = set().union(*[_task_labels(fr, t) for t in range(N_TASKS)])
    first_head = next(i for i, v in enumerate(full) if v in head_labels)
    # the trunk part, fragment for fragment
    assert np.array_equal(ctr[:first_head], full[:first_head])
    assert not head_labels & set(ctr[:first_head]) and ctr[first_head] in head_labels
    assert set(win) - {0} <= head_labels
    # every task's fragment sets, in the order the existing heads stream has them, in the stream that carries the task
    for task in range(N_TASKS):
        mine = _task_labels(fr, task)
        want = [v for v in full[first_head:] if v in mine]
        carrier = ctr[first_head:] if task == 0 else win
        assert len(want) == TILES * 2 * 8 * 2 + 4 * TILES * 2 and [v for v in carrier if v in mine] == want
        other = win if task == 0 else ctr
        assert not mine & set(other)
    # whole chunks, a multiple of 4 for the column-split kernel; the reference architecture's counts
    n_ctr, n_win = len(ctr) - first_head, len(win)
    assert first_head % 16 == 0 and n_ctr % 16 == 0 and n_win % 16 == 0
    assert (n_ctr // 16, n_win // 16) == ((24, 48) if kind == "16cs" else (20, 40))
    if kind == "16cs":
        assert first_head // 16 % 4 == 0


def test_a_task_window_starts_at_its_first_hidden_tile(fr):
    """f1 is stacked over the tasks: the window (t0, n) reads hidden tiles t0 * tiles_per_task .. of it, and f2s[t0 ..]."""
    for fn in (weights.x3b_stream_heads, weights.x3c_stream_heads):
        for t0 in range(N_TASKS):
            got = set(_labels(fn(fr["h1"], fr["h2"], TILES, (t0, 1)))) - {0}
            assert got == _task_labels(fr, t0)
        assert np.array_equal(fn(fr["h1"], fr["h2"], TILES, (0, N_TASKS)), fn(fr["h1"], fr["h2"], TILES))
    with pytest.raises(AssertionError):
        weights.x3_order(fr, 32, tasks=(0, 1))                          # the 32-row kernel has no task window


def _stream_bytes(pk, ptr, chunks):
    t = next(t for t in pk._keep if t.data_ptr() == ptr)
    assert t.numel() * t.element_size() == chunks * 16384
    return t.numpy().tobytes()


def test_lazy_packing_adds_five_streams_and_touches_nothing_else(monkeypatch):
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, tasks = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=16, x3_min_rows=1,
                                       fold_first_attention=True, cache_first_ffn=True)
    x3 = p.x3
    assert not x3.stream_ctr and not x3.stream_win and x3.chunks_ctr == 0           # a pack pays nothing for the mode
    before = {n: _stream_bytes(pk, getattr(x3, "stream" + n), getattr(x3, "chunks" + n)) for n in ("", "_cs", "_hc")}
    scales = (x3.sw_h1, x3.sw_h2, x3.hn_head, x3.hb_head, x3.n_params, x3.params, x3.params_hc)
    n_kept = len(pk._keep)
    splits = []
    monkeypatch.setattr(weights, "x3b_frags", lambda *a, **k: splits.append(1))
    assert weights.ctr_first_packable(p) and weights.pack_ctr_first(p, pk)
    assert not splits and len(pk._keep) == n_kept + 5                                # five more orderings of the one split
    assert weights.pack_ctr_first(p, pk) and len(pk._keep) == n_kept + 5             # once
    assert (x3.chunks, x3.chunks_cs, x3.chunks_hc) == (524, 536, 460)
    assert (x3.chunks_ctr, x3.chunks_ctr_cs, x3.chunks_ctr_hc) == (524 - 40, 536 - 48, 460 - 40)
    assert (x3.chunks_win, x3.chunks_win_cs) == (40, 48)
    for n in ("", "_cs", "_hc"):                                                     # the existing streams: the same bytes
        assert _stream_bytes(pk, getattr(x3, "stream" + n), getattr(x3, "chunks" + n)) == before[n]
        ctr = _stream_bytes(pk, getattr(x3, "stream_ctr" + n), getattr(x3, "chunks_ctr" + n))
        heads = (60 if n != "_cs" else 72) * 16384
        assert ctr[:len(ctr) - heads // 3] == before[n][:len(before[n]) - heads]     # the trunk part, byte for byte
    # stacked scales, bounds and blobs as packed
    assert scales == (x3.sw_h1, x3.sw_h2, x3.hn_head, x3.hb_head, x3.n_params, x3.params, x3.params_hc)


def test_lazy_packing_refuses_what_the_mode_cannot_run():
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=32)
    assert not weights.ctr_first_packable(p) and not weights.pack_ctr_first(p, pk) and not p.x3.stream_ctr
    p, pk, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=True, x3=False)
    assert not weights.pack_ctr_first(p, pk) and not p.x3.stream_win


def test_abi_carries_the_new_entries_under_version_14():
    lib = _lib.load()
    new = ("amdrec_ranker_forward_ctr_first", "amdrec_ranker_ctr_first_supported", "amdrec_ranker_winner_heads",
           "amdrec_ranker_ctr_first_workspace")
    for n in new:
        assert n in _lib.exported_symbols() and hasattr(lib, n) and getattr(lib, n).argtypes is not None
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION
    assert len(_lib._SIGNATURES["amdrec_ranker_forward_ctr_first"]) == len(_lib._SIGNATURES["amdrec_ranker_forward"]) + 2
    # the new stream fields sit behind everything the struct had
    names = [f[0] for f in weights.X3Weights._fields_]
    assert names[names.index("w_hidden_ad") + 1:] == ["stream_ctr", "chunks_ctr", "stream_ctr_cs", "chunks_ctr_cs",
                                                       "stream_ctr_hc", "chunks_ctr_hc", "stream_win", "chunks_win",
                                                       "stream_win_cs", "chunks_win_cs"]


def test_host_side_refusals_of_the_new_entries():
    """No GPU: the argument checks that return before anything is launched."""
    lib = _lib.load()
    user, ad, nnum, sd, _ = cases.ranker_case("demo", "scaled")
    p, pk, _ = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", x6=False, x3=True, x3_variant=16, x3_min_rows=1,
                                   fold_first_attention=True, cache_first_ffn=True)
    assert lib.amdrec_ranker_ctr_first_supported(C.byref(p), 500) == 0               # streams not packed yet
    assert weights.pack_ctr_first(p, pk)
    for rows in (1, 53, 4096, 4097, 16384, 16385, 262144, 262500):
        assert lib.amdrec_ranker_ctr_first_supported(C.byref(p), rows) == 1
    assert lib.amdrec_ranker_ctr_first_supported(C.byref(p), 0) == 0
    assert lib.amdrec_ranker_ctr_first_supported(None, 500) == 0
    n = C.c_size_t(0)
    both, fwd = C.c_size_t(0), C.c_size_t(0)
    _lib.check(lib.amdrec_ranker_ctr_first_workspace(C.byref(p), 0, 6000, C.byref(n)))
    assert n.value == (2 * 6000 * 4 + 255) // 256 * 256                              # the winners' two logit rows
    _lib.check(lib.amdrec_ranker_workspace(C.byref(p), 5000, C.byref(fwd)))
    _lib.check(lib.amdrec_ranker_ctr_first_workspace(C.byref(p), 5000, 100, C.byref(both)))
    assert both.value == fwd.value
    one = (C.c_float * 4)()
    bad = lib.amdrec_ranker_winner_heads(C.byref(p), one, 128, 10, one, 1, 10, 10, one, one, 1 << 20, None)
    assert bad != 0 and b"trunk" in lib.amdrec_last_error()                          # ld_trunk < 256
    bad = lib.amdrec_ranker_winner_heads(C.byref(p), one, 256, 9, one, 1, 10, 10, one, one, 1 << 20, None)
    assert bad != 0 and b"fewer rows" in lib.amdrec_last_error()
    bad = lib.amdrec_ranker_winner_heads(C.byref(p), C.byref(one, 4), 256, 10, one, 1, 10, 10, one, one, 1 << 20, None)
    assert bad != 0 and b"trunk" in lib.amdrec_last_error()                          # not 16-byte aligned
    bad = lib.amdrec_ranker_winner_heads(C.byref(p), one, 256, 10, one, 1, 10, 10, one, one, 16, None)
    assert bad != 0 and b"workspace" in lib.amdrec_last_error()
    assert lib.amdrec_ranker_winner_heads(C.byref(p), None, 0, 0, None, 0, 10, 10, None, None, 0, None) == 0     # no users


def test_constructor_refuses_an_unknown_mode_and_defaults_to_all():
    from amdrec.pipeline import AdRecommenderInference
    with pytest.raises(ValueError):
        AdRecommenderInference(device="cuda", two_tower_model=None, transformer_ranker=None, faiss_index=None,
                               ad_features=None, heads="nonsense")
    sig = inspect.signature(AdRecommenderInference.__init__)
    assert sig.parameters["heads"].default == "all"
    assert inspect.signature(AdRecommenderInference.recommend_device).parameters["heads"].default is None
    assert AdRecommenderInference.HEADS_MODES == ("all", "ctr_first")


def test_unsupported_reasons_name_the_cause():
    from collections import OrderedDict
    from amdrec.ranker import TransformerRanker
    user, ad, nnum = cases.small_dims()
    m = TransformerRanker(OrderedDict(user), OrderedDict(ad), nnum, embedding_dim=8, d_ff=128, num_layers=1)
    assert m.ctr_first_unsupported_reason() is None
    for attr, val, word in (("gemm_engine", "fp32", "fp32"), ("gemm_engine", "bf16x6", "bf16x6"), ("x3_variant", 32, "32"),
                            ("x3_min_rows", 8193, "x3_min_rows")):
        old = getattr(m, attr)
        setattr(m, attr, val)
        assert word in m.ctr_first_unsupported_reason()
        setattr(m, attr, old)
    assert m.ctr_first_unsupported_reason() is None
    t = TransformerRanker(OrderedDict(user), OrderedDict(ad), nnum, **cases.arch("tutorial")["rk"])
    assert "d_model 128" in t.ctr_first_unsupported_reason()
