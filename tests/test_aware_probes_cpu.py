"""CPU: the host side of aware probes (amdrec.probes) - the numpy rule against a slot-by-slot loop, the opt-in flag and the
``probe_policy`` argument with their refusals (before the library is touched), the flag's place in the saved header, the
per-list summaries in numpy on a layout with empty lists, Flat ignoring the flag, and the two C exports' refusals (every call
returns before its first HIP call).  No GPU."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

from amdrec import _lib, probes


def _bare(index_type, **attrs):
    """A FAISSIndex without its device side (no constructor: no library, no GPU)."""
    from amdrec.index import FAISSIndex
    idx = object.__new__(FAISSIndex)
    idx.index_type = index_type
    for k, v in attrs.items():
        setattr(idx, k, v)
    return idx


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def _rule_case(seed, nq=7, nlist=37, with_masks=True, with_weight=True):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((nq, nlist)).astype(np.float32)
    c[0, 3] = np.nan                                                    # a NaN score files as -inf, it is not dropped
    c[1, :5] = c[1, 0]                                                  # ties -> the lower list
    lens = rng.integers(0, 4, nlist).astype(np.int64)                   # some lists are empty
    kw = {}
    if with_masks:
        tag_or = rng.integers(0, 1 << 6, nlist).astype(np.uint64) | (rng.integers(0, 2, nlist).astype(np.uint64) << np.uint64(63))
        tag_or[lens == 0] = 0
        ra = rng.integers(0, 1 << 3, nq).astype(np.uint64)
        ry = rng.integers(0, 1 << 6, nq).astype(np.uint64)
        ra[0] = ry[0] = 0                                               # an unmasked query in the batch
        ry[2] = np.uint64(1) << np.uint64(63)                           # bit 63 in require_any
        ra[3] = np.uint64((1 << 64) - 1)                                # nothing is feasible
        kw.update(tag_or=tag_or.view(np.int64), require_all=ra.view(np.int64), require_any=ry.view(np.int64))
    if with_weight:
        hi = rng.standard_normal(nlist).astype(np.float32) + 1
        lo = hi - np.abs(rng.standard_normal(nlist)).astype(np.float32)
        w = rng.standard_normal(nq).astype(np.float32)
        w[0], w[1], w[2] = 0.0, 2.5, -2.5
        kw.update(boost_hi=hi, boost_lo=lo, weight=w)
    return c, lens, kw


@pytest.mark.parametrize("with_masks, with_weight", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("nprobe", [1, 5, 37])
def test_the_numpy_rule_against_a_slot_by_slot_loop(with_masks, with_weight, nprobe):
    c, lens, kw = _rule_case(11 + nprobe, with_masks=with_masks, with_weight=with_weight)
    got, s, ok = probes.aware_probes(c, nprobe, lens, **kw)
    want = probes.aware_probes_slotwise(c, nprobe, lens, **kw)
    assert np.array_equal(got, want)
    assert not ok[:, lens == 0].any()                                   # an empty list is never feasible
    if with_masks:
        assert not ok[3].any() and (got[3] == -1).all()                 # no feasible list: all -1
    # every probed list is feasible, every row's valid probes are distinct and in front of the -1 tail
    for q in range(len(c)):
        valid = got[q][got[q] >= 0]
        assert ok[q, valid].all() and len(set(valid.tolist())) == len(valid)
        assert (got[q][len(valid):] == -1).all() and len(valid) == min(nprobe, int(ok[q].sum()))


def test_the_rule_without_masks_and_weight_is_similarity_over_non_empty_lists():
    c, lens, _ = _rule_case(5, with_masks=False, with_weight=False)
    got, s, _ = probes.aware_probes(c, 6, lens)
    assert np.array_equal(s.view(np.uint32), probes.rank_last(c).view(np.uint32))
    for q in range(len(c)):
        cand = np.flatnonzero(lens > 0)
        sq = probes.rank_last(c[q])
        want = cand[np.lexsort((cand, -sq[cand].astype(np.float64)))][:6]
        assert np.array_equal(got[q], want)


def test_the_key_is_two_rounded_operations_not_an_fma():
    """c + w * b with the product rounded to fp32 first (a product that is inexact in fp32), and the sign rule."""
    c = np.array([[1.0]], dtype=np.float32)
    w = np.array([1.0 + 2.0 ** -12], dtype=np.float32)
    b = np.array([1.0 + 2.0 ** -12], dtype=np.float32)
    s = probes.aware_scores(c, b, b, w)
    two = np.float32(np.float32(w[0] * b[0]) + c[0, 0])
    assert s[0, 0] == two
    assert np.float32(w[0] * b[0]) != np.float64(w[0]) * np.float64(b[0])      # the product is inexact in fp32
    # sign of the weight picks the bound
    s2 = probes.aware_scores(np.zeros((2, 1), np.float32), np.array([3.0], np.float32), np.array([-1.0], np.float32),
                             np.array([2.0, -2.0], np.float32))
    assert s2[0, 0] == 6.0 and s2[1, 0] == 2.0


# ---- the summaries --------------------------------------------------------------------------------------------------------------
def test_summaries_in_numpy_on_a_layout_with_empty_lists():
    off = np.array([0, 0, 3, 3, 4, 9, 9], dtype=np.int64)                # lists 0, 2, 5 empty; list 3 holds one row
    tags = np.array([1, 2, 4, -(1 << 63), 8, 8, 16, 0, 1], dtype=np.int64)
    boosts = np.array([0.5, -1.0, 2.0, -3.0, 0.0, 1.5, -0.25, 7.0, 0.125], dtype=np.float32)
    tag_or, hi, lo = probes.list_summaries(off, tags, boosts)
    assert tag_or.dtype == np.uint64 and hi.dtype == lo.dtype == np.float32
    assert tag_or.tolist() == [0, 7, 0, 1 << 63, 25, 0]
    assert hi.tolist() == [0.0, 2.0, 0.0, -3.0, 7.0, 0.0] and lo.tolist() == [0.0, -1.0, 0.0, -3.0, -0.25, 0.0]
    only_tags = probes.list_summaries(off, tags, None)
    assert only_tags[1] is None and only_tags[2] is None and np.array_equal(only_tags[0], tag_or)
    only_boosts = probes.list_summaries(off, None, boosts)
    assert only_boosts[0] is None and np.array_equal(only_boosts[1], hi)
    # feasibility reads them: an empty list never, bit 63 as any other bit
    lens = np.diff(off)
    ok = probes.feasible(lens, tag_or, np.array([0, 1 << 63], dtype=np.uint64), np.array([0, 0], dtype=np.uint64))
    assert ok.tolist() == [[False, True, False, True, True, False], [False, False, False, True, False, False]]


def test_feasibility_is_necessary_not_sufficient():
    """Two bits of require_all on different rows of one list: the list is feasible, no row is eligible."""
    off = np.array([0, 2], dtype=np.int64)
    tag_or, _, _ = probes.list_summaries(off, np.array([1, 2], dtype=np.int64))
    assert probes.feasible(np.diff(off), tag_or, np.array([3], np.uint64), np.array([0], np.uint64)).tolist() == [[True]]


# ---- flag and policy ------------------------------------------------------------------------------------------------------------
def test_policy_and_flag_refusals_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    assert probes.check_policy(None, True) is True and probes.check_policy(None, False) is False
    assert probes.check_policy("similarity", True) is False and probes.check_policy("similarity", False) is False
    assert probes.check_policy("aware", True) is True
    with pytest.raises(ValueError, match=r"enable_aware_probes\(\)"):
        probes.check_policy("aware", False)
    with pytest.raises(ValueError, match="probe_policy"):
        probes.check_policy("nearest", True)
    q = torch.zeros((2, 8))
    qn = np.zeros((2, 8), dtype=np.float32)
    for index_type in ("IVF", "IVFPQ"):
        idx = _bare(index_type, aware_probes=False)
        for call in (lambda: idx.search_device(q, 3, probe_policy="aware"), lambda: idx.search(qn, 3, probe_policy="aware"),
                     lambda: idx.batch_search(qn, 3, probe_policy="aware")):
            with pytest.raises(ValueError, match=r"enable_aware_probes\(\)"):
                call()
        with pytest.raises(ValueError, match="probe_policy"):
            _bare(index_type, aware_probes=True).search_device(q, 3, probe_policy="similar")
    assert _bare("IVF")._aware() is False                               # an object from before the flag
    assert _bare("IVF", aware_probes=True)._aware() is True and _bare("IVFPQ", aware_probes=True)._aware() is True


def test_flat_ignores_the_flag(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    idx = _bare("Flat", aware_probes=True, _ivf=None)
    assert idx._aware() is False
    idx.enable_aware_probes()                                           # nothing to do, nothing touched
    assert idx.aware_probes is True and idx._aware() is False
    with pytest.raises(ValueError, match=r"enable_aware_probes\(\)"):   # Flat has no probes to choose: "aware" is refused
        idx.search_device(torch.zeros((2, 8)), 3, probe_policy="aware")


def test_enable_reaches_the_coarse_level(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    from amdrec.ivf import InvertedLists
    st = object.__new__(InvertedLists)
    st.aware_probes, st.tag_source, st.boost_source, st.lists = False, None, None, None
    idx = _bare("IVFPQ", aware_probes=False, _ivf=st)
    idx.enable_aware_probes()
    assert st.aware_probes is True and idx._aware() is True
    with pytest.raises(ValueError, match=r"enable_aware_probes\(\)"):   # the coarse step itself refuses masks without the flag
        st.aware_probes = False
        st.coarse_probes(torch.zeros((1, 8)), 2, elig=(torch.zeros(1), torch.zeros(1)))


# ---- the saved header -----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("index_type, flag, want", [("IVF", True, True), ("IVF", False, False), ("Flat", True, False)])
def test_saved_header_carries_the_flag_only_when_on(index_type, flag, want, tmp_path):
    idx = _bare(index_type, aware_probes=flag, list_boosts=False, list_tags=False, dimension=8, nlist=4, nprobe=2, pq_m=8,
                refine=None, refine_factor=4, verbose=False, _n=0, _ids=_NoDevice(np.zeros(0, np.int64)),
                _xb=_NoDevice(np.zeros((0, 8), np.float32)), _keeps_rows=True, _tags=None, _state=None, _identity=True,
                _host_ids=None)
    path = str(tmp_path / "ix")
    idx.save(path)
    h = _header(path)
    assert h.get("aware_probes", False) is want and ("aware_probes" in h) == want


def test_load_reads_the_flag_and_defaults_to_off(tmp_path, monkeypatch):
    from amdrec.index import FAISSIndex, _MAGIC
    seen = []

    class Reached(Exception):
        pass

    def create(self):
        seen.append(self.aware_probes)
        raise Reached
    monkeypatch.setattr(FAISSIndex, "_create_index", create)
    for field, want in (({}, False), ({"aware_probes": True}, True), ({"aware_probes": False}, False), ({"list_tags": True}, False)):
        header = dict(dimension=8, index_type="IVF", nlist=4, nprobe=2, ntotal=0, identity_ids=True, arrays=[], **field)
        hj = json.dumps(header).encode()
        path = str(tmp_path / f"ix{len(seen)}")
        with open(path, "wb") as f:
            f.write(_MAGIC + struct.pack("<Q", len(hj)) + hj)
        idx = _bare("IVF", pq_m=8, aware_probes=not want)
        with pytest.raises(Reached):
            idx.load(path)
        assert seen[-1] is want


# ---- the C entries --------------------------------------------------------------------------------------------------------------
def test_the_two_exports_exist_and_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    assert len(lib.amdrec_ivf_coarse_keys_aware.argtypes) == len(lib.amdrec_ivf_coarse_keys.argtypes) + 7
    assert lib.amdrec_abi_version() == 14 == _lib.ABI_VERSION
    raw = (ctypes.c_char * 4096)()
    base = ctypes.addressof(raw)
    p = ctypes.c_void_p((base + 255) // 256 * 256)                      # never dereferenced: every call below returns first
    odd = ctypes.c_void_p(p.value + 8)

    def keys(nlist=8, dim=8, nq=2, ld=8, lens=p, masks=(p, p, p), boost=(p, p, p)):
        return lib.amdrec_ivf_coarse_keys_aware(p, nlist, dim, dim, p, nq, dim, p, ld, lens, *masks, *boost, None)
    assert keys(nq=0) == 0                                              # nothing to do
    assert keys(dim=6) != 0 and keys(nlist=0) != 0 and keys(ld=6) != 0 and keys(nlist=9, ld=9) != 0
    assert keys(lens=None) != 0
    assert keys(masks=(p, None, p)) != 0 and keys(masks=(None, p, p)) != 0          # all three or none
    assert keys(boost=(p, p, None)) != 0 and keys(boost=(None, None, p)) != 0
    assert keys(masks=(odd, p, p)) != 0 and keys(boost=(odd, p, p)) != 0 and keys(lens=odd) != 0   # 16-byte alignment
    assert b"aligned" in lib.amdrec_last_error()

    def summ(nlist=8, off=p, tags=p, boosts=p, tag_or=p, hi=p, lo=p):
        return lib.amdrec_ivf_list_summaries(off, nlist, tags, boosts, tag_or, hi, lo, None)
    assert summ(tags=None, boosts=None) == 0                            # nothing to summarise
    assert summ(nlist=0) != 0 and summ(off=None) != 0 and summ(tag_or=None) != 0 and summ(lo=None) != 0
    del raw
