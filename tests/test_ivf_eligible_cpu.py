"""CPU: the host side of eligibility masks in the inverted-list scans - the four *_eligible scan exports and their refusals
(every C call returns before its first HIP call), the opt-in flag of FAISSIndex and its place in the saved header, R1's
condition on the shapes of the GPU cases, and the host oracle against a slot-by-slot loop.  No GPU."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from amdrec import _lib
from tests import eligible_oracle as eo, ivf_eligible_oracle as io

EXPORTS = ("amdrec_ivf_scan_eligible", "amdrec_ivf_scan_grouped_eligible", "amdrec_ivf_scan_grouped_mixed_eligible",
           "amdrec_ivfpq_scan_finite_eligible")


def _fake_pointer():
    raw = ctypes.create_string_buffer(4096 + 256)
    return raw, (ctypes.addressof(raw) + 255) // 256 * 256            # non-null, aligned, never dereferenced


def test_the_four_exports_exist_and_are_bound():
    lib = _lib.load()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        twin = name[:-len("_eligible")]
        assert len(getattr(lib, name).argtypes) == len(getattr(lib, twin).argtypes) + 3
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION


def test_scan_entries_refuse_bad_eligibility_pointers_before_any_hip_call():
    lib = _lib.load()
    raw, p = _fake_pointer()

    def pairs(nq=2, lt=p, ma=p, my=p):
        return lib.amdrec_ivf_scan_eligible(p, 64, 64, p, p, p, nq, 64, p, p, 4, p, 100, 0, None, lt, ma, my)

    def grouped(nq=2, lt=p, ma=p, my=p):          # nq = 0 <-> nothing to scan: no query tiles
        return lib.amdrec_ivf_scan_grouped_eligible(p, 64, 64, p, p, 8, 100, p, 64, p, p, 10 if nq else 0, 32, p, p, p, 4, p, 100,
                                                    0, None, 0, None, None, lt, ma, my)

    def mixed(nq=2, lt=p, ma=p, my=p):
        return lib.amdrec_ivf_scan_grouped_mixed_eligible(p, 64, p, 64, 64, p, p, 8, 100, p, 64, p, 64, p, p, 10 if nq else 0,
                                                          32, p, p, 100, 0, p, 1, p, p, None, lt, ma, my)

    def pq(nq=2, lt=p, ma=p, my=p):
        return lib.amdrec_ivfpq_scan_finite_eligible(p, 8, p, p, p, 8, 100, p, 4, p, p, 10, 32, p, p, p, nq * 4, p, 100, 0, None,
                                                     lt, ma, my)
    for call in (pairs, grouped, mixed, pq):
        for kw, word in ((dict(lt=None), b"list_tags is null"), (dict(ma=None), b"require_all is null"),
                         (dict(my=None), b"require_any is null"), (dict(lt=p + 4), b"list_tags must be 8-byte aligned"),
                         (dict(ma=p + 4), b"require_all must be 8-byte aligned"),
                         (dict(my=p + 2), b"require_any must be 8-byte aligned")):
            assert call(**kw) == -1 and word in lib.amdrec_last_error(), (call.__name__, kw, lib.amdrec_last_error())
        assert call(nq=0, lt=None, ma=None, my=None) == 0                  # nothing to scan: AMDREC_OK, as the plain twins
    # the plain twins' own refusals still come first
    assert lib.amdrec_ivf_scan_eligible(p, 64, 62, p, p, p, 2, 64, p, p, 4, p, 100, 0, None, None, None, None) == -1
    assert b"multiple of 4" in lib.amdrec_last_error()
    del raw


def _bare(index_type, **attrs):
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type = index_type
    for k, v in attrs.items():
        setattr(idx, k, v)
    return idx


@pytest.mark.parametrize("index_type", ["IVF", "IVFPQ"])
def test_check_masks_follows_the_flag_without_the_library(index_type, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    z = torch.zeros(2, dtype=torch.int64)
    assert _bare(index_type, list_tags=True)._check_masks(z, None) is True
    assert _bare(index_type, list_tags=True)._check_masks(None, z) is True
    assert _bare(index_type, list_tags=True)._check_masks(None, None) is False
    for idx in (_bare(index_type), _bare(index_type, list_tags=False)):
        with pytest.raises(NotImplementedError, match="follow-up") as e:
            idx._check_masks(z, None)
        assert "list_tags=True" in str(e.value)
        assert idx._check_masks(None, None) is False
    assert _bare("Flat")._check_masks(z, z) is True


class _NoDevice:
    """Stands in for the device side of save(): FAISSIndex.save only calls .cpu().numpy() on slices."""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, s):
        return _NoDevice(self.a[s])

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _header(path):
    with open(path, "rb") as f:
        f.read(9)
        (hl,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(hl).decode())


@pytest.mark.parametrize("flag", [True, False])
def test_saved_header_carries_the_flag(flag, tmp_path):
    idx = _bare("IVF", list_tags=flag, dimension=8, nlist=4, nprobe=2, pq_m=8, refine=None, refine_factor=4, verbose=False,
                _n=0, _ids=_NoDevice(np.zeros(0, np.int64)), _xb=_NoDevice(np.zeros((0, 8), np.float32)), _keeps_rows=True,
                _tags=None, _state=None, _identity=True, _host_ids=None)
    path = str(tmp_path / "ix")
    idx.save(path)
    h = _header(path)
    assert h.get("list_tags", False) is flag and ("list_tags" in h) == flag     # absent when off: an earlier file


def test_load_reads_the_flag_with_a_default(tmp_path, monkeypatch):
    """load() sets the flag from the header before it creates the index; a header without the field gives False."""
    from amdrec.index import FAISSIndex, _MAGIC
    seen = []

    class Reached(Exception):
        pass

    def create(self):
        seen.append(self.list_tags)
        raise Reached
    monkeypatch.setattr(FAISSIndex, "_create_index", create)
    for field, want in (({}, False), ({"list_tags": True}, True), ({"list_tags": False}, False)):
        header = dict(dimension=8, index_type="IVF", nlist=4, nprobe=2, ntotal=0, identity_ids=True, arrays=[], **field)
        hj = json.dumps(header).encode()
        path = str(tmp_path / f"ix{len(seen)}")
        with open(path, "wb") as f:
            f.write(_MAGIC + struct.pack("<Q", len(hj)) + hj)
        idx = _bare("IVF", pq_m=8, list_tags=not want)
        with pytest.raises(Reached):
            idx.load(path)
        assert seen[-1] is want


@pytest.mark.parametrize("name, nprobe", io.R1_SHAPES)
def test_r1_condition_holds_for_the_gpu_shapes(name, nprobe):
    """No query's probed lists can fill the 2048 slots of the plain search: the nprobe longest lists (float64 assignment to
    the given centres) hold fewer rows."""
    x, c, nlist = io.corpus(name)
    assert len(c) == nlist
    rows = io.longest_lists_rows(x, c, nprobe)
    print(f"{name} nprobe {nprobe}: the {nprobe} longest lists hold {rows} rows")
    assert rows < io.PLAIN_K
    if name == "long64":
        assert rows == 1840


def test_restrict_matches_a_slot_by_slot_loop():
    rng = np.random.default_rng(11)
    n, nq, filled = 500, 13, 300
    tags = eo.tags_for(n, 3)
    a, y = io.masks_cycle(nq)
    pos = np.full((nq, io.PLAIN_K), -1, dtype=np.int64)
    sc = np.full((nq, io.PLAIN_K), -np.inf, dtype=np.float32)
    for q in range(nq):
        pos[q, :filled] = rng.permutation(n)[:filled]
        sc[q, :filled] = np.sort(rng.standard_normal(filled).astype(np.float32))[::-1]
    for k in (10, 100, 400):
        D, I = io.restrict(pos, sc, tags, a, y, k, -np.inf)
        rD, rI = io.restrict_loop(pos, sc, tags, a, y, k, -np.inf)
        assert np.array_equal(I, rI) and np.array_equal(D, rD)
        assert (I[5::6] == -1).all() and np.array_equal(I[0], pos[0, :k] if k <= filled else np.r_[pos[0, :filled], [-1] * (k - filled)])
    full = pos.copy()
    full[:, -1] = 7
    with pytest.raises(AssertionError, match="whole probed set"):
        io.restrict(full, sc, tags, a, y, 10, -np.inf)
    assert np.array_equal(io.map_kept(np.array([[0, 2, -1]]), np.array([5, 6, 9])), [[5, 9, -1]])
