"""Coherence of derived state, the part that needs no GPU: the drop-ins copy and pickle after their first pack; the ranker's
per-ad cache is keyed by the table itself, not by numbers a second table can repeat; the ``.data`` rule (``invalidate()`` is
the remedy); and the seeded walks of tests/test_coherence_walk_gpu.py contain every rule and every stale-state transition
they are there for (tests/coherence.py)."""
import copy
import hashlib
import io
import json
import os
import pickle
import weakref

import numpy as np
import pytest
import torch

from amdrec import _lib, ranker as ranker_mod, synth
from tests import cases
from tests import coherence as co

CPU = torch.device("cpu")
RANKER_ARCH = dict(embedding_dim=8, d_model=256, num_heads=8, num_layers=1, d_ff=128)


def _t(sd):
    return {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}


def _towers():
    from amdrec.towers import TwoTowerModel
    user, ad, nnum, sd, _ = cases.two_tower_case("ragged")
    m = TwoTowerModel(dict(user), dict(ad), nnum, **cases.arch("ragged")["tt"])
    m.load_state_dict(_t(sd))
    return m.eval()


def _ranker():
    from amdrec.ranker import TransformerRanker
    user, ad, nnum = cases.small_dims()
    sd = synth.ranker_state(user, ad, nnum, seed=91, cross_scale=1.0 / 16, **RANKER_ARCH)
    m = TransformerRanker(dict(user), dict(ad), nnum, **RANKER_ARCH)
    m.load_state_dict(_t(sd))
    return m.eval()


def _drop_ins(m):
    """The modules of ``m`` that keep derived state."""
    return [m] if isinstance(m, ranker_mod.TransformerRanker) else [m.user_tower, m.ad_tower]


def _pack_all(m):
    for d in _drop_ins(m):
        d._pack(CPU)
        assert d._packed is not None and "_amdrec_tensor_list" in d.__dict__


def _packed_tensors(d):
    """Host copies of everything a pack uploaded (weights.Packed keeps the tensors its pointers point at)."""
    keep = d._packed.keep if isinstance(d, ranker_mod.TransformerRanker) else d._packed[2]
    return [t.clone() for t in keep._keep]


def _install_entry(m, table, proj):
    """An _AdCache entry for ``table`` under the current pack key, as cache_ad_projection files it (that call needs a GPU)."""
    vals = dict(zip(("data_ptr", "shape", "version"), ranker_mod._table_key(table)), key=m._packed.key, proj=proj, hidden=None,
                table=weakref.ref(table))
    m._ad_cache = ranker_mod._AdCache(*[vals[f] for f in ranker_mod._AdCache._fields])


COPIES = {
    "deepcopy": copy.deepcopy,
    "pickle": lambda m: pickle.loads(pickle.dumps(m)),
    "torch_save": lambda m: (lambda b: (torch.save(m, b), b.seek(0), torch.load(b, weights_only=False))[2])(io.BytesIO()),
}


@pytest.mark.parametrize("how", list(COPIES))
@pytest.mark.parametrize("make", [_towers, _ranker], ids=["towers", "ranker"])
def test_a_packed_drop_in_copies_and_pickles(make, how):
    """After the first pack a module holds a ctypes structure of raw pointers; a copy must succeed, carry none of the
    derived state and none of the original's cached tensor list, and version its own tensors."""
    m = make()
    _pack_all(m)
    if isinstance(m, ranker_mod.TransformerRanker):
        _install_entry(m, torch.zeros((4, len(m._ad_names)), dtype=torch.int64), torch.zeros((4, 256)))
        m.ctr_first_unsupported_reason()
        assert "_ctr_first_why" in m.__dict__
    c = COPIES[how](m)
    assert type(c) is type(m)
    for a, b in zip(m.state_dict().values(), c.state_dict().values()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    originals = {id(t) for d in _drop_ins(m) for t in d.__dict__["_amdrec_tensor_list"]}
    for d in _drop_ins(c):
        assert d._packed is None and getattr(d, "_ad_cache", None) is None
        assert not [k for k in d.__dict__ if k.startswith("_amdrec_tensor_") or k == "_ctr_first_why"], d.__dict__.keys()
    for d in _drop_ins(m):                                   # the original keeps what it had
        assert d._packed is not None and "_amdrec_tensor_list" in d.__dict__
    before_m = [_lib.tensor_versions(d) for d in _drop_ins(m)]
    before_c = [_lib.tensor_versions(d) for d in _drop_ins(c)]
    for d in _drop_ins(c):
        assert not originals & {id(t) for t in d.__dict__["_amdrec_tensor_list"]}
        with torch.no_grad():
            next(d.parameters()).add_(1.0)
    assert [_lib.tensor_versions(d) for d in _drop_ins(m)] == before_m
    for d, b in zip(_drop_ins(c), before_c):
        assert _lib.tensor_versions(d) != b
    _pack_all(c)                                             # a copy packs for itself
    for dm, dc in zip(_drop_ins(m), _drop_ins(c)):
        assert dm._packed is not dc._packed


def test_equal_address_shape_and_version_do_not_share_a_cache_entry():
    """B is another tensor object over A's storage - the same data_ptr and shape, as the caching allocator gives a table
    loaded into a freed table's block - written to until its version equals A's: the entry filed for A is not B's."""
    m = _ranker()
    m._pack(CPU)
    A = torch.zeros((5, len(m._ad_names)), dtype=torch.int64)
    B = torch.empty(0, dtype=torch.int64).set_(A.untyped_storage(), 0, A.shape)
    B.fill_(3)                                               # other contents, written through B
    while A._version < B._version:                           # harmless in-place writes raise A's version to B's
        A.add_(0)
    assert B is not A and ranker_mod._table_key(A) == ranker_mod._table_key(B) and int(A[0, 0]) == 3
    proj = torch.zeros((5, 256))
    _install_entry(m, A, proj)
    assert m._entry_for(A) is m._ad_cache and m._cache_for(A) is proj
    assert m._entry_for(B) is None and m._cache_for(B) is None and m._hidden_cache_for(B) is None
    # the numbers still count: the same object after an in-place write is another table
    A.add_(1)
    assert m._entry_for(A) is None
    # and an entry whose table has been freed serves no-one
    _install_entry(m, B, proj)
    assert m._entry_for(B) is not None
    del B
    C = torch.empty(0, dtype=torch.int64).set_(A.untyped_storage(), 0, A.shape)
    assert m._ad_cache.table() is None and m._entry_for(C) is None


@pytest.mark.parametrize("make", [_towers, _ranker], ids=["towers", "ranker"])
def test_invalidate_is_the_remedy_after_a_data_write(make):
    """Writes through ``.data`` bump no version and change no identity: they are outside the cache keys, and ``invalidate()``
    makes the next pack read the weights again."""
    m = make()
    _pack_all(m)
    for d in _drop_ins(m):
        first = _packed_tensors(d)
        packed, versions = d._packed, _lib.tensor_versions(d)
        p = d.feature_projection.weight if isinstance(d, ranker_mod.TransformerRanker) else d.mlp[0].weight
        p.data.mul_(1.5)
        p.data = p.data.clone()
        assert _lib.tensor_versions(d) == versions           # the framework shows nothing ...
        d._pack(CPU)
        assert d._packed is packed                           # ... so the key stands (the documented gap)
        d.invalidate()
        assert d._packed is None
        d._pack(CPU)
        second = _packed_tensors(d)
        assert d._packed is not packed and len(first) == len(second)
        assert any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(first, second))
        twin = make()
        twin.load_state_dict(m.state_dict())
        dt = _drop_ins(twin)[_drop_ins(m).index(d)]
        dt._pack(CPU)
        for a, b in zip(second, _packed_tensors(dt)):
            assert torch.equal(a, b)
    if hasattr(m, "user_tower"):                             # the model-level call reaches both towers
        _pack_all(m)
        m.invalidate()
        assert m.user_tower._packed is None and m.ad_tower._packed is None


def test_the_data_rule_is_documented():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    for word in (".data", "invalidate()", "DLPack", "rec.ad_features"):
        assert word in text, word
    from amdrec import towers
    for doc in (ranker_mod.__doc__, towers.__doc__):
        assert ".data" in doc and "invalidate()" in doc
    for doc in (ranker_mod.TransformerRanker.invalidate.__doc__, towers._Tower.invalidate.__doc__):
        assert ".data" in doc and "DLPack" in doc


# ---- the walk generator -----------------------------------------------------------------------------------------------------
def test_corpus_model_follows_the_index_rules():
    c = co.CorpusModel(4, n_feat=2)
    c.add(np.ones((3, 4)), [5, 7, 5], tags=[1, 2, 3], feats=[[0, 1]] * 3)
    c.add(np.zeros((2, 4)), [9, 11], groups=[4, -1], bids=[2.0, 0.5], feats=[[1, 1]] * 2)
    assert c.tags.tolist() == [1, 2, 3, 0, 0] and c.groups.tolist() == [-1, -1, -1, 4, -1]
    assert c.bids.tolist() == [1.0, 1.0, 1.0, 2.0, 0.5]
    assert c.remove([5, 5, 404]) == 2 and c.ids == [7, 9, 11] and c.tags.tolist() == [2, 0, 0]
    assert c.rows.shape == (3, 4) and c.feats.tolist() == [[0, 1], [1, 1], [1, 1]] and c.rows[0, 0] == 1.0
    c.set_tags([8, 8, 8])
    c.set_groups([1, 2, 3])
    c.set_bids([3, 3, 3])
    assert c.tags.tolist() == [8, 8, 8] and c.groups.tolist() == [1, 2, 3] and c.bids.dtype == np.float32
    assert c.remove([7, 9, 11]) == 3 and c.n == 0 and c.rows.shape == (0, 4)


def test_corpus_model_carries_boosts():
    """float32; a row never given one has 0.0; -0.0 is stored as +0.0 (amdrec.boost); carried through add, remove, set_boosts."""
    from amdrec import boost
    c = co.CorpusModel(4)
    c.add(np.ones((3, 4)), [5, 7, 5], boosts=[0.25, -0.0, -1.5])
    c.add(np.zeros((2, 4)), [9, 11])
    assert c.boosts.dtype == np.float32 and c.boosts.tolist() == [0.25, 0.0, -1.5, 0.0, 0.0]
    assert not np.signbit(c.boosts).tolist()[1] and np.array_equal(c.boosts[:3], boost.as_boosts([0.25, -0.0, -1.5], 3))
    assert c.remove([5]) == 2 and c.boosts.tolist() == [0.0, 0.0, 0.0] and c.tags.tolist() == [0, 0, 0]
    c.set_boosts(np.array([-0.0, 2.0, -3.0]))
    assert c.boosts.dtype == np.float32 and c.boosts.tolist() == [0.0, 2.0, -3.0] and not np.signbit(c.boosts[0])
    assert c.remove([7, 9, 11]) == 3 and c.boosts.shape == (0,)
    # the values the steps write: mixed sign, up to BOOST_SCALE, exact zeros of both signs among them
    b = co.row_attrs(7, 4000)[3]
    assert b.dtype == np.float32 and np.abs(b).max() <= co.BOOST_SCALE and (b > 0.4).any() and (b < -0.4).any()
    assert 500 < (b == 0).sum() < 1500 and np.signbit(b[b == 0]).any() and not np.signbit(b[b == 0]).all()
    big = co.big_boosts(7, 37, 16.0)
    assert np.abs(big).max() == big[0] == 8.0 and np.array_equal(big[1:], (co.row_attrs(7, 37)[3] * np.float32(16))[1:])


# ---- the walks of before the option walks: walk() and row_attrs' first three values give what they gave ----------------------
def _digest(steps):
    return hashlib.sha256(repr(steps).encode()).hexdigest()


def test_the_existing_walks_have_not_moved():
    """tests/golden/coherence_walks.json was written from the walk generator as it was before it knew option walks: a sha256
    of repr(steps) per entry of INDEX_WALKS and PIPELINE_WALKS, called as tests/test_coherence_walk_gpu.py calls it."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coherence_walks.json")) as f:
        golden = json.load(f)
    assert (co.INDEX_WALKS, co.PIPELINE_WALKS) == (((33, "ints", 30), (60, "ints", 30), (70, "strings", 30)),
                                                   {"Flat": (2, 20), "IVF": (8, 20)})
    assert co.PROBES == ((1, 10), (33, 500), (512, 100), (3, 2000)) and co.VARIANTS == ("plain", "exclude", "masks", "cap", "all")
    assert len(co.INDEX_RULES) == 9 and len(co.PIPELINE_RULES) == 9
    assert set(golden["index"]) == {f"{seed}/{scheme}/{n}" for seed, scheme, n in co.INDEX_WALKS}
    for seed, scheme, n in co.INDEX_WALKS:
        assert _digest(co.walk(seed, co.INDEX_RULES, n, scheme)) == golden["index"][f"{seed}/{scheme}/{n}"], (seed, scheme)
    assert set(golden["pipeline"]) == set(co.PIPELINE_WALKS)
    for index_type, (seed, n) in co.PIPELINE_WALKS.items():
        steps = co.walk(seed, co.PIPELINE_RULES, n, "unique", n0=co.PIPELINE_ADS, add_sizes=co.PIPELINE_ADD_SIZES, bulk=0)
        assert _digest(steps) == golden["pipeline"][index_type], index_type
    for scheme in co.ID_SCHEMES:
        assert _digest(co.initial_step(scheme)) == golden["initial_step"][scheme], scheme
    for key, want in golden["row_attrs"].items():
        vseed, m = map(int, key.split("/"))
        got = co.row_attrs(vseed, m)
        assert len(got) == 4 and hashlib.sha256(b"".join(a.tobytes() for a in got[:3])).hexdigest() == want, key


def test_select_path_is_the_host_rule():
    """tests.coherence.select_path against amdrec.ivf's own dispatch arithmetic."""
    from amdrec import ivf
    assert (co.SELECT_SLICE_KEYS, co.SPLIT_MAX_QUERIES) == (ivf.SELECT_SLICE_KEYS, 1024 // co.SPLIT_MIN_SLICES)
    for n in (100, 6000, 16383, 16384, 18000):
        for nq, _ in co.PROBES:
            slices = min(ivf.SELECT_MAX_SLICES, n // ivf.SELECT_SLICE_KEYS, 1024 // nq)      # every list probed: pool_ld = n
            assert (co.select_path(n, co.NLIST, co.NLIST, nq) == "split") == (slices >= 4), (n, nq)
            assert co.select_path(n, 1, co.NLIST, nq) in ("single", "data")
    assert co.reserve_capacity(0, 6000) == 6000 and co.reserve_capacity(6000, 6001) == 9000
    assert co.reserve_capacity(0, 1) == 1024 and co.reserve_capacity(9000, 6038) == 9000


@pytest.mark.parametrize("seed,scheme,n_steps", co.INDEX_WALKS)
def test_index_walk_seeds_cover_every_rule_and_transition(seed, scheme, n_steps):
    steps = co.walk(seed, co.INDEX_RULES, n_steps, scheme)
    assert steps == co.walk(seed, co.INDEX_RULES, n_steps, scheme) and len(steps) == n_steps          # pure
    assert {r for r, _ in steps} == set(co.INDEX_RULES)
    missing = set(co.REQUIRED_TRANSITIONS) - co.transitions(steps)
    assert not missing, missing
    sizes = {a["m"] for r, a in steps if r == "add"}
    assert co.BULK_ADD in sizes and sizes & set(co.ADD_SIZES)
    assert {a["value"] for r, a in steps if r == "nprobe"} >= {co.NLIST}
    # the removal lists hold absent ids and duplicates, one of them names every row, and no step sets attributes of an empty corpus
    for r, a in steps:
        if r in ("remove", "remove_all", "remove_set_tags"):
            assert len(a["ids"]) > len(set(a["ids"])) and a["removed"] > 0
            assert a["n_after"] == (0 if r == "remove_all" else a["n_before"] - a["removed"])
        if "set_" in r:
            assert a["n_before"] > 0
    ids = {type(x) for r, a in steps if r == "add" for x in a["ids"]}
    assert ids == ({str} if scheme == "strings" else {int})
    if scheme == "strings":
        # the host id -> positions map is keyed by the number of ids: only a refill to the SAME count with no map built in
        # between (the probes on an empty index build none) can revive a stale one
        assert "remove_all_then_add_same_count" in co.transitions(steps)
    assert any(a["tags"] for r, a in steps if r == "add") and any(not a["tags"] for r, a in steps if r == "add")
    if scheme == "ints":                                     # ids that repeat, and ids that do not
        drawn = [x for r, a in steps if r == "add" and a["ids"][0] >= 10**6 for x in a["ids"]]      # the repeating scheme's
        assert len(set(drawn)) < len(drawn), "no id names two rows"
        assert any(a["ids"][0] < 10**6 and len(set(a["ids"])) == a["m"] for r, a in steps if r == "add")


@pytest.mark.parametrize("index_type", list(co.PIPELINE_WALKS))
def test_pipeline_walk_seeds_cover_every_rule(index_type):
    seed, n_steps = co.PIPELINE_WALKS[index_type]
    steps = co.walk(seed, co.PIPELINE_RULES, n_steps, "unique", n0=co.PIPELINE_ADS, add_sizes=co.PIPELINE_ADD_SIZES, bulk=0)
    assert {r for r, _ in steps} == set(co.PIPELINE_RULES) and len(steps) == n_steps
    found = co.transitions(steps)
    assert "remove_then_add_same_count" in found
    cap = [i for i, (r, _) in enumerate(steps) if r == "capture"]
    assert cap and cap[0] < n_steps - 3, "a graph must live through later steps"
    later = {r for r, _ in steps[cap[0] + 1:]}
    assert later & {"remove_ads", "add_ads"} and later & {"tower_update", "ranker_update", "load_state_dict"}
    assert {a["mode"] for r, a in steps if r == "heads"} >= {"ctr_first"}


# ---- the option walks (tests/test_coherence_options_gpu.py) ---------------------------------------------------------------------
def test_reserve_and_boost_bound_rules_are_the_index_rules():
    """The walk's picture of the long-lived index's boost bound, rule by rule, on a seed that has every rule."""
    seed, scheme, n = co.INDEX_WALKS_OPTIONS[0]
    for rule, a in co.walk(seed, co.INDEX_RULES_OPTIONS, n, scheme):
        vals = co.step_boosts(rule, a)
        if rule in ("set_boosts", "remove_set_boosts", "reload"):
            assert a["bound_after"] == a["true_after"], rule                      # replaced / recomputed
        elif rule in ("add", "add_big_boosts") and vals is not None:
            assert a["bound_after"] == max(a["bound_before"], float(np.abs(vals).max())), rule
        else:
            assert a["bound_after"] == a["bound_before"], rule                    # removals included: the bound stays
        assert a["bound_after"] >= a["true_after"]
        if rule == "add_big_boosts":
            assert float(np.abs(vals).max()) == co.BOOST_SCALE * a["scale"] >= 4 * a["bound_before"] > 0


@pytest.mark.parametrize("seed,scheme,n_steps", co.INDEX_WALKS_OPTIONS)
def test_index_option_walk_seeds_cover_every_rule_and_transition(seed, scheme, n_steps):
    steps = co.walk(seed, co.INDEX_RULES_OPTIONS, n_steps, scheme)
    assert steps == co.walk(seed, co.INDEX_RULES_OPTIONS, n_steps, scheme) and len(steps) == n_steps          # pure
    assert {r for r, _ in steps} == set(co.INDEX_RULES_OPTIONS) > set(co.INDEX_RULES)
    found = co.transitions_options(steps)
    missing = (set(co.REQUIRED_TRANSITIONS) | set(co.REQUIRED_TRANSITIONS_OPTIONS) | {"mixed_second_phase"}) - found
    assert not missing, missing
    sizes = {a["m"] for r, a in steps if r == "add"}
    assert co.BULK_ADD in sizes and sizes & set(co.ADD_SIZES)
    assert {a["value"] for r, a in steps if r == "nprobe"} >= {co.NLIST}
    assert co.initial_step(scheme, options=True)["boosts"] is True
    adds = [a for r, a in steps if r == "add"]
    assert any(a["boosts"] for a in adds) and any(not a["boosts"] for a in adds)
    for i, (r, a) in enumerate(steps):
        if "removed" in a:
            assert len(a["ids"]) > len(set(a["ids"])) and a["removed"] > 0
        if "set_" in r and r not in ("remove_set_tags", "remove_set_boosts"):
            assert a["n_before"] > 0
        if r == "remove_big_boosts":
            # exactly the rows of the last add_big_boosts that are still there - here: all of them -, and the bound outlives them
            last = [b for q, b in steps[:i] if q == "add_big_boosts"][-1]
            assert set(a["ids"]) - {10**12, 10**12 + 1, "no-such-ad-0", "no-such-ad-1"} == set(last["ids"])
            assert a["removed"] == last["m"] and a["bound_after"] == a["bound_before"] > a["true_after"]
    assert steps[-1][1]["n_after"] > 500
    ids = {type(x) for r, a in steps if "m" in a for x in a["ids"]}
    assert ids == ({str} if scheme == "strings" else {int})


@pytest.mark.parametrize("index_type", list(co.PIPELINE_WALKS_OPTIONS))
def test_pipeline_option_walk_seeds_cover_every_rule(index_type):
    seed, n_steps = co.PIPELINE_WALKS_OPTIONS[index_type]
    steps = co.walk(seed, co.PIPELINE_RULES_OPTIONS, n_steps, "unique", n0=co.PIPELINE_ADS, add_sizes=co.PIPELINE_ADD_SIZES,
                    bulk=0)
    rules = [r for r, _ in steps]
    assert set(rules) == set(co.PIPELINE_RULES_OPTIONS) > set(co.PIPELINE_RULES) and len(steps) == n_steps
    assert "remove_then_add_same_count" in co.transitions_options(steps)
    cap = rules.index("capture")
    assert cap < n_steps - 4, "a graph must live through later steps"
    later = set(rules[cap + 1:])
    assert later & {"remove_ads", "add_ads"} and later & {"tower_update", "ranker_update", "load_state_dict"}
    assert "set_boosts" in later, "a graph captured with stage1_boost must outlive a swap of the boosts"
    assert {a["mode"] for r, a in steps if r == "heads"} >= {"ctr_first"} and rules.index("heads") < n_steps - 2
    adds = [a["boosts"] for r, a in steps if r == "add_ads"]
    assert any(adds) and not all(adds)
    assert steps[-1][1]["n_after"] > 0


@pytest.mark.parametrize("kind", list(co.LATE_WALKS))
def test_late_opt_in_walks_enable_every_flag_once(kind):
    steps = co.late_walk(kind)
    assert steps == co.late_walk(kind)
    rules = [r for r, _ in steps]
    assert [r for r in rules if r in co.LATE_ENABLES[kind]] == list(co.LATE_ENABLES[kind])      # once each, in this order
    assert set(co.LATE_RULES) <= set(rules) and not rules[0].startswith("enable_")
    assert steps[0][1]["flags"] == () and steps[-1][1]["n_after"] > 500
    want = tuple(e[len("enable_"):] for e in co.LATE_ENABLES[kind] if e.startswith("enable_"))
    assert steps[-1][1]["flags"] == want
    for (r0, a0), (r1, a1) in zip(steps, steps[1:]):
        assert a1["n_before"] == a0["n_after"] and a1["flags"][:len(a0["flags"])] == a0["flags"]
        assert not (r0 in co.LATE_ENABLES[kind] and r1 in co.LATE_ENABLES[kind])
    # the two kinds meet "a list-order copy" and "the flag of its summaries" in both orders
    f = co.LATE_ENABLES
    assert f["ivf"].index("enable_list_tags") < f["ivf"].index("enable_aware_probes") < f["ivf"].index("enable_list_boosts")
    assert f["ivfpq"].index("enable_aware_probes") < f["ivfpq"].index("enable_list_tags") and "enable_list_boosts" not in f["ivfpq"]
    last = max(i for i, r in enumerate(rules) if r in co.LATE_ENABLES[kind])
    assert {"add", "remove", "reload"} & set(rules[last + 1:]), "the last opt-in must live through a later step"
