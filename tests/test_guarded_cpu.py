"""CPU: the guarded-buffer helpers themselves (tests/guarded.py).  ``SplitScanWorkspace`` must not drift from the carve it
replaces: for a grid of arguments every field equals ``InvertedLists.workspace``'s in ``numel()``, ``dtype`` and None-ness,
the real method running against a CPU-backed stand-in for ``amdrec._lib.WORKSPACE``.  And ``guarded`` / its ``check`` see a
byte written on either side."""
import itertools

import pytest
import torch

from tests.guarded import GUARD, GUARD_FILL, SENTINEL, SplitScanWorkspace, guarded


class _CpuArena:
    """Serves ``_lib.WORKSPACE`` requests from host memory, at exactly the requested size."""

    def __init__(self):
        self.sizes = []

    def get(self, nbytes, device):
        self.sizes.append(int(nbytes))
        return torch.empty(int(nbytes), dtype=torch.uint8)


# pairs = chunk * nprobe: 1, 7 * 9 = 63, 64, 65, 3 * 37 = 111, 640, 1000 * 16; nlist + 1: 2, 17, 64, 65, 101, 4097
GRID = list(itertools.product((1, 7, 64, 65, 3, 1000), (1, 9, 37, 16), (1, 333, 20_000), (0, 8, 300_000), (0, 7 * 9 * 8 * 1024),
                              (1, 16, 63, 64, 100, 4096)))


def test_the_split_workspace_has_the_real_carve_s_fields():
    from amdrec import _lib, ivf
    assert any((c * p) % 64 and (n + 1) % 64 for c, p, _, _, _, n in GRID)
    assert any((c * p) % 64 == 0 for c, p, *_ in GRID) and any((n + 1) % 64 == 0 for *_, n in GRID)
    for chunk, nprobe, pool_ld, coarse_bytes, extra_bytes, nlist in GRID:
        if chunk * pool_ld * 8 > 1 << 21:
            continue                                                  # (host memory: the carve is linear in these)
        lists = ivf.InvertedLists(torch.zeros((nlist, 4)))
        arena = _CpuArena()
        with _lib.WORKSPACE.private(arena):
            real = lists.workspace(chunk, nprobe, pool_ld, coarse_bytes, extra_bytes)
        split = SplitScanWorkspace()
        got = split.workspace(lists, chunk, nprobe, pool_ld, coarse_bytes, extra_bytes)
        assert type(got) is type(real) and got._fields == real._fields
        for name, r, g in zip(real._fields, real, got):
            assert (r is None) == (g is None), name
            if r is not None:
                assert (g.numel(), g.dtype) == (r.numel(), r.dtype), (name, chunk, nprobe, pool_ld, coarse_bytes, extra_bytes, nlist)
                assert g.data_ptr() % 256 == 0 and g.is_contiguous()
        assert (got.keys is None) == (coarse_bytes == 0)
        # and the real fields lie inside the one allocation, in the documented order, without overlap past the pool
        assert len(arena.sizes) == 1
        spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in real[1:] if t.numel()]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert spans[-1][1] - spans[0][0] <= arena.sizes[0]
        split.check()
        assert split.calls == [(chunk, nprobe, pool_ld, coarse_bytes, extra_bytes)]


def test_install_replaces_the_method(monkeypatch):
    from amdrec import ivf
    lists = ivf.InvertedLists(torch.zeros((5, 4)))
    split = SplitScanWorkspace().install(monkeypatch)
    w = lists.workspace(3, 2, 10, 0, extra_bytes=12)
    assert w.keys is None and w.pair_q.numel() == 6 and w.goff.numel() == 6 and w.extra.numel() == 12
    assert split.calls == [(3, 2, 10, 0, 12)]
    split.check()


@pytest.mark.parametrize("shape,dtype", [((3, 7), torch.float32), ((5,), torch.int64), ((0,), torch.int64), (11, torch.int32),
                                         ((2, 3), torch.bfloat16)])
def test_guarded_is_exact_aligned_filled_and_notices_either_band(shape, dtype):
    t = guarded(shape, dtype, "cpu", "output")
    want = (shape,) if isinstance(shape, int) else shape
    assert tuple(t.shape) == want and t.dtype == dtype and t.data_ptr() % 256 == 0
    assert bool(torch.isnan(t).all()) if dtype.is_floating_point else bool((t == SENTINEL).all())
    nbytes = t.numel() * t.element_size()
    off = t.offset
    assert nbytes == 0 or off == t.data_ptr() - t.block.data_ptr()
    assert off >= GUARD and t.block.numel() - off - nbytes >= GUARD
    assert bool((t.block[:off] == GUARD_FILL).all()) and bool((t.block[off + nbytes:] == GUARD_FILL).all())
    t.check()
    for at in (off - 1, off + nbytes, 0, t.block.numel() - 1):          # the bytes next to the tensor and the far ends
        keep = int(t.block[at])
        t.block[at] = keep ^ 1
        with pytest.raises(AssertionError, match="were written"):
            t.check()
        t.block[at] = keep
    t.check()
    assert bool((guarded(4, torch.uint8, "cpu") == 0xA5).all()) and bool((guarded(4, torch.int32, "cpu", 0) == 0).all())
