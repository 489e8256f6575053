"""Shared infrastructure of the coherence tests (tests/test_coherence_cpu.py, tests/test_coherence_models_gpu.py,
tests/test_coherence_walk_gpu.py): is a long-lived serving object, after an arbitrary history of calls, still the object a
fresh one built from the same final state would be?

* ``CorpusModel``: the plain truth of a corpus - rows as given, ids, tags, groups, bids and ad-feature rows in insertion
  order, with the index's own rules for the values a row was never given (tag 0, group -1, bid 1.0).  numpy only.
* ``walk(seed, rules, n_steps, ...)``: a pure function from a seed to a list of ``(rule, arguments)``; seeded numpy, replayed
  exactly, no GPU - so a CPU test can assert what a seed's sequence contains (``transitions``).
* ``fresh_index`` / ``fresh_pipeline``: the twin a step's state is compared with.  They import torch and amdrec lazily; a
  twin loads the trained state the test saved once (``FAISSIndex.save`` of the trained, still empty index) instead of
  training again.
"""
import numpy as np

# ---- the walks' fixed settings -------------------------------------------------------------------------------------------------
D, N0, NLIST = 64, 6000, 32
ADD_SIZES = (1, 37, 1500)
# one add per index walk lifts the corpus past SPLIT_MIN_POOL rows: 6000 + 7 x 1500 would need a third of the walk.  Only
# then can a query's candidate pool reach the size from which amdrec_ivf_select_split takes over (``select_path``)
BULK_ADD = 12_000
NPROBES = (1, 10, NLIST)
PROBES = ((1, 10), (33, 500), (512, 100), (3, 2000))            # (nq, k), in the order they run after every step
VARIANTS = ("plain", "exclude", "masks", "cap", "all")
EXCLUDE_WIDTH = 16                                              # k + E <= 2048 at k = 2000, and K1 = 2048 - E >= k under a cap
# remove_set_tags: a removal and set_tags in ONE step, no search in between - the only order in which the index reads its
# list layout (to regather the list-order tags) before a search has had the chance to notice the new row count
INDEX_RULES = ("add", "remove", "remove_all", "remove_set_tags", "set_tags", "set_groups", "set_bids", "nprobe", "reload")
PIPELINE_RULES = ("remove_ads", "add_ads", "tower_update", "ranker_update", "load_state_dict", "heads", "set_bids", "set_groups",
                  "capture")
PIPELINE_ADD_SIZES = (1, 37, 300)
ID_SCHEMES = ("ints", "strings", "unique")
# the seeds of the GPU walks, chosen on the CPU so that every rule and every transition of REQUIRED_TRANSITIONS occurs
# (tests/test_coherence_cpu.py asserts it): (seed, id scheme, steps)
INDEX_WALKS = ((33, "ints", 30), (60, "ints", 30), (70, "strings", 30))
PIPELINE_WALKS = {"Flat": (2, 20), "IVF": (8, 20)}
PIPELINE_ADS = 3000

# csrc / amdrec.ivf: InvertedLists.select splits a query over workgroups when min(64, pool_ld // 4096, 1024 // nq) >= 4
SELECT_SLICE_KEYS, SPLIT_MIN_SLICES, SPLIT_MAX_QUERIES = 4096, 4, 256
SPLIT_MIN_POOL = SELECT_SLICE_KEYS * SPLIT_MIN_SLICES


def select_path(n, nprobe, nlist, nq):
    """Which select a search of ``nq`` queries takes on an IVF / IVFPQ index of ``n`` rows: "split"
    (amdrec_ivf_select_split), "single" (amdrec_ivf_select), or "data" where the list lengths decide.  The pool pitch is the
    rows of the ``nprobe`` longest lists: all ``n`` rows when every list is probed, never more than ``n``."""
    if nq > SPLIT_MAX_QUERIES or n < SPLIT_MIN_POOL:
        return "single"
    return "split" if nprobe >= nlist else "data"


def reserve_capacity(cap, n):
    """FAISSIndex._reserve: the capacity after room for ``n`` rows was asked for (1.5x growth, minimum 1024)."""
    return cap if n <= cap else max(n, int(cap * 1.5), 1024)


# ---- the truth of a corpus -----------------------------------------------------------------------------------------------------
class CorpusModel:
    def __init__(self, dim, n_feat=0, nprobe=10):
        self.dim, self.nprobe = int(dim), int(nprobe)
        self.rows = np.empty((0, self.dim), dtype=np.float32)
        self.ids = []
        self.tags = np.empty(0, dtype=np.int64)
        self.groups = np.empty(0, dtype=np.int64)
        self.bids = np.empty(0, dtype=np.float32)
        self.feats = np.empty((0, int(n_feat)), dtype=np.int64)

    @property
    def n(self):
        return len(self.ids)

    def add(self, rows, ids, tags=None, groups=None, bids=None, feats=None):
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, self.dim)
        m = len(rows)
        assert len(ids) == m
        self.rows = np.concatenate([self.rows, rows])
        self.ids = self.ids + list(ids)
        self.tags = np.concatenate([self.tags, np.zeros(m, np.int64) if tags is None else np.asarray(tags, np.int64)])
        self.groups = np.concatenate([self.groups, np.full(m, -1, np.int64) if groups is None else np.asarray(groups, np.int64)])
        self.bids = np.concatenate([self.bids, np.ones(m, np.float32) if bids is None else np.asarray(bids, np.float32)])
        if self.feats.shape[1]:
            self.feats = np.concatenate([self.feats, np.asarray(feats, np.int64).reshape(m, self.feats.shape[1])])
        assert len(self.tags) == len(self.groups) == len(self.bids) == len(self.rows) == self.n

    def remove(self, ids):
        """Every row carrying a listed id goes, order kept -> rows removed."""
        gone = set(ids)
        keep = np.array([x not in gone for x in self.ids], dtype=bool)
        removed = int((~keep).sum())
        self.rows, self.tags, self.groups, self.bids = self.rows[keep], self.tags[keep], self.groups[keep], self.bids[keep]
        if self.feats.shape[1]:
            self.feats = self.feats[keep]
        self.ids = [x for x, k in zip(self.ids, keep) if k]
        return removed

    def set_tags(self, tags):
        self.tags = np.asarray(tags, dtype=np.int64).reshape(self.n).copy()

    def set_groups(self, groups):
        self.groups = np.asarray(groups, dtype=np.int64).reshape(self.n).copy()

    def set_bids(self, bids):
        self.bids = np.asarray(bids, dtype=np.float32).reshape(self.n).copy()

    def int_ids(self):
        return np.asarray(self.ids, dtype=np.int64)


def row_attrs(vseed, m):
    """The attribute values a step writes: (tags: 4 low bits, groups: -1 (ungrouped) .. 39, bids: 0.1 .. 5 in fp32)."""
    rng = np.random.default_rng(vseed)
    return (rng.integers(0, 16, m).astype(np.int64), rng.integers(-1, 40, m).astype(np.int64),
            np.round(rng.uniform(0.1, 5.0, m), 3).astype(np.float32))


def query_masks(nq):
    """The probe set's eligibility masks: (require_all, require_any) int64 [nq], a third of the queries unconstrained."""
    i = np.arange(nq)
    return (np.where(i % 3 == 0, 0, 1 << (i % 2))).astype(np.int64), np.where(i % 3 == 1, 0, 6).astype(np.int64)


# ---- the walk generator --------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, scheme, n0):
        self.scheme, self.ids, self.cap, self.next_id, self.pool_off, self.nprobe = scheme, [], 0, 0, 0, 10
        self.heads = "all"

    def new_ids(self, rng, m, repeating=False):
        if self.scheme == "strings":
            # strings, some of them naming two rows
            out = [f"ad-{self.next_id + j - (j % 11 == 10)}" for j in range(m)]
        elif repeating and self.scheme == "ints":
            out = (rng.integers(0, 9000, m) + 10**6).tolist()                   # repeat inside the add and across adds
        else:
            out = ((np.arange(m) + self.next_id) * 3 + 11).tolist()             # non-contiguous, unique
        self.next_id += m
        return out

    def absent(self, j):
        return f"no-such-ad-{j}" if self.scheme == "strings" else 10**12 + j


def initial_step(scheme="ints", n0=N0):
    """The first add of every walk: ``n0`` rows with tags, groups and bids (caps and the auction need the index to hold keys)."""
    st = _State(scheme, n0)
    return _add(st, np.random.default_rng(0), n0, True, True, True, False)[1]


def _add(st, rng, m, tags, groups, bids, repeating):
    n = len(st.ids)
    cap = reserve_capacity(st.cap, n + m)
    args = dict(m=int(m), start=st.pool_off, ids=st.new_ids(rng, m, repeating), tags=bool(tags), groups=bool(groups),
                bids=bool(bids), vseed=int(rng.integers(1 << 30)), n_before=n, grew=cap != st.cap)
    st.pool_off += m
    st.ids = st.ids + args["ids"]
    st.cap = cap
    args["n_after"] = len(st.ids)
    return "add", args


def walk(seed, rules, n_steps, scheme="ints", n0=N0, nlist=NLIST, add_sizes=ADD_SIZES, bulk=BULK_ADD):
    """-> [(rule, args)] of ``n_steps`` steps after ``initial_step``: every rule of ``rules`` at least once (a shuffled agenda,
    then uniform draws), with the follow-ups that make the stale-state traps certain instead of likely:
    the first removal is followed by an add of exactly as many rows, remove_all by an add, and the first add of an index walk is the bulk add, followed by nprobe = nlist.
    Every args dict also records ``n_before`` / ``n_after`` (rows) for ``transitions``; pure: the same seed gives the same list."""
    assert scheme in ID_SCHEMES
    rng = np.random.default_rng(seed)
    st = _State(scheme, n0)
    _add(st, np.random.default_rng(0), n0, True, True, True, False)
    alias = {"remove_ads": "remove", "add_ads": "add"}
    agenda = [rules[i] for i in rng.permutation(len(rules))]
    forced, steps, n_removals, bulk_done = [], [], 0, False

    def emit(rule, args):
        args.setdefault("n_before", len(st.ids))
        args.setdefault("n_after", len(st.ids))
        args["nprobe"] = st.nprobe
        steps.append((rule, args))

    while len(steps) < n_steps:
        if forced:
            rule, hint = forced.pop(0)
        elif agenda:
            rule, hint = agenda.pop(0), None
        else:
            rule, hint = rules[int(rng.integers(len(rules)))], None
        kind = alias.get(rule, rule)
        n = len(st.ids)
        if n == 0 and kind not in ("add", "reload", "nprobe"):
            rule = "add_ads" if "add_ads" in rules else "add"                   # nothing to remove or to set on an empty corpus
            kind, hint = "add", None
        if kind == "add":
            if hint is not None:
                m = hint
            elif not bulk_done and bulk and "nprobe" in rules:
                m, bulk_done = bulk, True
                forced.append(("nprobe", nlist))
            else:
                m = add_sizes[int(rng.integers(len(add_sizes)))]
            flags = rng.integers(0, 2, 4)
            _, args = _add(st, rng, m, flags[0], flags[1], flags[2], bool(flags[3]))
            emit(rule, args)
        elif kind in ("remove", "remove_all", "remove_set_tags"):
            distinct = list(dict.fromkeys(st.ids))
            if kind == "remove_all":
                chosen = distinct
                forced.insert(0, ("add_ads" if "add_ads" in rules else "add", add_sizes[-1]))
            else:
                cnt = int(rng.integers(1, max(2, len(distinct) // 4)))
                chosen = [distinct[i] for i in rng.choice(len(distinct), size=cnt, replace=False)]
            gone = set(chosen)
            removed = sum(1 for x in st.ids if x in gone)
            listed = chosen + [st.absent(0), st.absent(1)] + chosen[:3]         # absent ids, duplicates
            st.ids = [x for x in st.ids if x not in gone]
            st.cap = len(st.ids)                                                # the gathers are exact-size
            if kind == "remove":
                n_removals += 1
                if n_removals == 1:
                    forced.insert(0, ("add_ads" if "add_ads" in rules else "add", removed))
            emit(rule, dict(ids=listed, removed=removed, n_before=n, n_after=len(st.ids), vseed=int(rng.integers(1 << 30))))
        elif kind in ("set_tags", "set_groups", "set_bids", "tower_update", "ranker_update", "load_state_dict"):
            emit(rule, dict(vseed=int(rng.integers(1 << 30))))
        elif kind == "nprobe":
            st.nprobe = int(hint if hint is not None else NPROBES[int(rng.integers(len(NPROBES)))])
            emit(rule, dict(value=st.nprobe))
        elif kind == "reload":
            st.cap = reserve_capacity(0, n)                                     # a loaded index reserves for its rows
            emit(rule, {})
        elif kind == "heads":
            st.heads = "ctr_first" if st.heads == "all" else "all"
            emit(rule, dict(mode=st.heads))
        elif kind == "capture":
            emit(rule, {})
        else:
            raise ValueError(f"unknown rule {rule!r}")
    return steps


def pool_rows(steps, n0=N0):
    """Rows of the seeded row pool a walk draws from (``args['start']`` .. + m of every add; the first n0 are the initial add's)."""
    return n0 + sum(a["m"] for r, a in steps if "m" in a)


REQUIRED_TRANSITIONS = ("remove_then_add_same_count", "add_grows_capacity", "add_within_capacity", "remove_all_then_add",
                        "set_tags_before_masked_search", "remove_then_set_tags", "split_after_single", "single_after_split",
                        "reload_mid_life")


def transitions(steps, nlist=NLIST, probes=PROBES):
    """The named transitions a walk contains (every step is followed by the whole probe set, masked searches included)."""
    found = set()
    for i, (rule, a) in enumerate(steps):
        prev = steps[i - 1] if i else (None, {})
        if rule in ("add", "add_ads"):
            found.add("add_grows_capacity" if a["grew"] else "add_within_capacity")
            if prev[0] in ("remove", "remove_ads") and prev[1]["removed"] == a["m"] and prev[1]["removed"] > 0:
                found.add("remove_then_add_same_count")
            if prev[0] == "remove_all":
                found.add("remove_all_then_add")
                if prev[1]["removed"] == a["m"]:                                # no probe between them builds a host id map
                    found.add("remove_all_then_add_same_count")
        if rule in ("set_tags", "remove_set_tags"):
            found.add("set_tags_before_masked_search")
        if rule == "remove_set_tags" and a["removed"] > 0 and a["n_after"] > 0:
            found.add("remove_then_set_tags")
        if rule == "reload" and 0 < i < len(steps) - 1:
            found.add("reload_mid_life")
        paths = [select_path(a["n_after"], a["nprobe"], nlist, nq) for nq, _ in probes]
        for p, q in zip(paths, paths[1:]):
            if (p, q) == ("single", "split"):
                found.add("split_after_single")
            if (p, q) == ("split", "single"):
                found.add("single_after_split")
    return found


# ---- the twins -----------------------------------------------------------------------------------------------------------------
def index_kinds(nlist=NLIST):
    """tests.test_exclude_gpu.KINDS at the walks' nlist, the IVF kinds with list-order tags (they take masks)."""
    from tests.test_exclude_gpu import KINDS
    return {k: dict(v, nlist=nlist, list_tags=True) if v["index_type"] != "Flat" else dict(v) for k, v in KINDS.items()}


def fresh_index(kind, model, trained_file, dim=None, kinds=None):
    """A new FAISSIndex in the trained state saved in ``trained_file`` (saved empty, before the first add), given the
    model's rows in ONE add with explicit ids, tags, groups and bids, at the model's nprobe."""
    from amdrec.index import FAISSIndex
    kinds = index_kinds() if kinds is None else kinds
    idx = FAISSIndex(model.dim if dim is None else dim, **kinds[kind])
    idx.load(trained_file)
    assert idx.index_type == kinds[kind]["index_type"] and idx.index.ntotal == 0 and idx.index.is_trained
    if model.n:
        idx.add(model.rows, list(model.ids), tags=model.tags, groups=model.groups, bids=model.bids)
    else:
        # an add of zero rows cannot hand over attributes; the long-lived index still HOLDS (zero) keys and bids after its
        # last row left, and an index that holds none refuses caps and the auction: give the twin its empty ones
        idx.set_tags(model.tags)
        idx.set_groups(model.groups)
        idx.set_bids(model.bids)
    if idx.index_type != "Flat":
        idx.nprobe = model.nprobe
    return idx


def fresh_pipeline(model, tower_sd, ranker_sd, knobs):
    """A new AdRecommenderInference: new modules from the state dicts (read off the long-lived ones with ``state_dict()``), a
    new ad table from the model, ``fresh_index``.  ``knobs``: dict(make_tower, make_ranker: constructors of empty modules;
    kind, trained_file, kinds: as fresh_index; heads: the heads mode; ranker: attribute switches to set)."""
    import torch
    from amdrec.pipeline import AdRecommenderInference
    tt = knobs["make_tower"]()
    tt.load_state_dict({k: v.detach().clone().cpu() for k, v in tower_sd.items()})
    rk = knobs["make_ranker"]()
    rk.load_state_dict({k: v.detach().clone().cpu() for k, v in ranker_sd.items()})
    for name, value in knobs.get("ranker", {}).items():
        setattr(rk, name, value)
    idx = fresh_index(knobs["kind"], model, knobs["trained_file"], kinds=knobs.get("kinds"))
    table = torch.from_numpy(np.ascontiguousarray(model.feats, dtype=np.int64))
    return AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=idx, ad_features=table,
                                  heads=knobs.get("heads", "all"))
