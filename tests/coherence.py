"""Shared infrastructure of the coherence tests (tests/test_coherence_cpu.py, tests/test_coherence_models_gpu.py,
tests/test_coherence_walk_gpu.py, tests/test_coherence_options_gpu.py): is a long-lived serving object, after an arbitrary history of calls, still the object a
fresh one built from the same final state would be?

* ``CorpusModel``: the plain truth of a corpus - rows as given, ids, tags, groups, bids, boosts and ad-feature rows in insertion
  order, with the index's own rules for the values a row was never given (tag 0, group -1, bid 1.0, boost 0.0).  numpy only.
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
# the option walks (tests/test_coherence_options_gpu.py): boosts, list boosts, aware probes and value ranking.  New tuples - the
# rule sets, probes and seeds above stay as they are, and ``walk`` draws for them what it always drew (tests/golden/
# coherence_walks.json holds their digests).
#   remove_set_boosts: a removal and set_boosts in ONE step (remove_set_tags' trap for the list-order boosts and their summaries)
#   add_big_boosts:    an add whose boosts exceed in magnitude every boost stored so far - the long-lived _boost_max must grow
#   remove_big_boosts: removes exactly those rows - the long-lived _boost_max stays, a fresh index's is smaller
INDEX_RULES_OPTIONS = INDEX_RULES + ("set_boosts", "remove_set_boosts", "add_big_boosts", "remove_big_boosts")
PIPELINE_RULES_OPTIONS = PIPELINE_RULES + ("set_boosts", "set_tags")
PROBES_OPTIONS = ((1, 10), (33, 500), (512, 100))
BOOST_SCALE = 0.5                                               # row_attrs' boosts lie in [-BOOST_SCALE, BOOST_SCALE]
INDEX_WALKS_OPTIONS = ((4, "ints", 20), (1, "strings", 20))     # (seed, id scheme, steps), chosen like INDEX_WALKS
PIPELINE_WALKS_OPTIONS = {"Flat": (9, 14), "IVF": (26, 14)}
# the late opt-ins: the long-lived index is built with no flag and each enable_* call occurs once, at a seeded step.  IVF: tags,
# then the summaries' flag (made for the standing tag copy), then the boosts (their summary is made WITH the copy); IVFPQ (no
# list boosts): the summaries' flag first, the tags after it - so both orders of "a copy" and "the flag of its summary" occur
LATE_RULES = ("add", "remove", "set_tags", "nprobe", "reload")
LATE_ENABLES = {"ivf": ("enable_list_tags", "enable_aware_probes", "enable_list_boosts", "set_boosts"),
                "ivfpq": ("enable_aware_probes", "enable_list_tags")}
LATE_WALKS = {"ivf": (0, 8), "ivfpq": (0, 7)}                   # (seed, steps of LATE_RULES; the enables come on top)

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
        self.boosts = np.empty(0, dtype=np.float32)
        self.feats = np.empty((0, int(n_feat)), dtype=np.int64)

    @property
    def n(self):
        return len(self.ids)

    def add(self, rows, ids, tags=None, groups=None, bids=None, feats=None, boosts=None):
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, self.dim)
        m = len(rows)
        assert len(ids) == m
        self.rows = np.concatenate([self.rows, rows])
        self.ids = self.ids + list(ids)
        self.tags = np.concatenate([self.tags, np.zeros(m, np.int64) if tags is None else np.asarray(tags, np.int64)])
        self.groups = np.concatenate([self.groups, np.full(m, -1, np.int64) if groups is None else np.asarray(groups, np.int64)])
        self.bids = np.concatenate([self.bids, np.ones(m, np.float32) if bids is None else np.asarray(bids, np.float32)])
        self.boosts = np.concatenate([self.boosts, np.zeros(m, np.float32) if boosts is None else _plus_zero(boosts)])
        if self.feats.shape[1]:
            self.feats = np.concatenate([self.feats, np.asarray(feats, np.int64).reshape(m, self.feats.shape[1])])
        assert len(self.tags) == len(self.groups) == len(self.bids) == len(self.boosts) == len(self.rows) == self.n

    def remove(self, ids):
        """Every row carrying a listed id goes, order kept -> rows removed."""
        gone = set(ids)
        keep = np.array([x not in gone for x in self.ids], dtype=bool)
        removed = int((~keep).sum())
        self.rows, self.tags, self.groups, self.bids = self.rows[keep], self.tags[keep], self.groups[keep], self.bids[keep]
        self.boosts = self.boosts[keep]
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

    def set_boosts(self, boosts):
        self.boosts = _plus_zero(boosts).reshape(self.n).copy()

    def int_ids(self):
        return np.asarray(self.ids, dtype=np.int64)


def _plus_zero(boosts):
    """float32, -0.0 stored as +0.0 (amdrec.boost)."""
    return np.asarray(boosts, dtype=np.float32) + np.float32(0.0)


def row_attrs(vseed, m):
    """The attribute values a step writes: (tags: 4 low bits, groups: -1 (ungrouped) .. 39, bids: 0.1 .. 5 in fp32, boosts:
    -0.5 .. 0.5 in fp32, a quarter of them exactly 0.0 and some of those -0.0).  The boosts are drawn last: the first three
    are what they were before there was a fourth."""
    rng = np.random.default_rng(vseed)
    first = (rng.integers(0, 16, m).astype(np.int64), rng.integers(-1, 40, m).astype(np.int64),
             np.round(rng.uniform(0.1, 5.0, m), 3).astype(np.float32))
    boosts = np.round(rng.uniform(-BOOST_SCALE, BOOST_SCALE, m), 3).astype(np.float32)
    zero = rng.integers(0, 8, m)
    boosts[zero == 0] = 0.0
    boosts[zero == 1] = -0.0
    return first + (boosts,)


def big_boosts(vseed, m, scale):
    """add_big_boosts' values: row_attrs' boosts times ``scale`` (a power of two: exact), the first of them at the largest
    magnitude, BOOST_SCALE * scale."""
    b = row_attrs(vseed, m)[3] * np.float32(scale)
    b[0] = np.float32(BOOST_SCALE * scale)
    return b


def step_boosts(rule, args):
    """The boosts a step of an option walk writes (float32; None: the step gives none): the added rows' for an add, every
    row's for set_boosts / remove_set_boosts."""
    if rule == "add_big_boosts":
        return big_boosts(args["vseed"], args["m"], args["scale"])
    if rule in ("add", "add_ads"):
        return row_attrs(args["vseed"], args["m"])[3] if args.get("boosts") else None
    if rule in ("set_boosts", "remove_set_boosts"):
        return row_attrs(args["vseed"], args["n_after"])[3]
    return None


def query_masks(nq):
    """The probe set's eligibility masks: (require_all, require_any) int64 [nq], a third of the queries unconstrained."""
    i = np.arange(nq)
    return (np.where(i % 3 == 0, 0, 1 << (i % 2))).astype(np.int64), np.where(i % 3 == 1, 0, 6).astype(np.int64)


# ---- the walk generator --------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, scheme, n0, options=False):
        self.scheme, self.ids, self.cap, self.next_id, self.pool_off, self.nprobe = scheme, [], 0, 0, 0, 10
        self.heads = "all"
        # option walks only: |boost| of every row, the long-lived index's _boost_max (max(old, new) on add, replaced by
        # set_boosts, recomputed on load, left alone by remove_ids) and the ids of the last add_big_boosts
        self.babs = np.empty(0, dtype=np.float32) if options else None
        self.bound, self.big_ids = 0.0, []

    @property
    def true_bound(self):
        """max |boost| of the rows that are there: a fresh index's _boost_max."""
        return float(self.babs.max()) if self.babs is not None and len(self.babs) else 0.0

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


def initial_step(scheme="ints", n0=N0, options=False):
    """The first add of every walk: ``n0`` rows with tags, groups and bids (caps and the auction need the index to hold keys);
    ``options``: and boosts (an option walk's index holds a boost tensor from the start)."""
    st = _State(scheme, n0, options)
    return _add(st, np.random.default_rng(0), n0, True, True, True, False, boosts=True if options else None)[1]


def _add(st, rng, m, tags, groups, bids, repeating, boosts=None, scale=None):
    """``boosts`` (option walks; None: the args hold no such key, as ever): do the rows come with boosts?  ``scale``:
    add_big_boosts' factor."""
    n = len(st.ids)
    cap = reserve_capacity(st.cap, n + m)
    args = dict(m=int(m), start=st.pool_off, ids=st.new_ids(rng, m, repeating), tags=bool(tags), groups=bool(groups),
                bids=bool(bids), vseed=int(rng.integers(1 << 30)), n_before=n, grew=cap != st.cap)
    st.pool_off += m
    st.ids = st.ids + args["ids"]
    st.cap = cap
    args["n_after"] = len(st.ids)
    rule = "add"
    if boosts is not None:
        args["boosts"] = bool(boosts)
        if scale is not None:
            rule, args["scale"] = "add_big_boosts", float(scale)
        vals = step_boosts(rule, args)
        st.babs = np.concatenate([st.babs, np.zeros(m, np.float32) if vals is None else np.abs(vals)])
        if vals is not None:
            st.bound = max(st.bound, float(np.abs(vals).max()))
    return rule, args


def walk(seed, rules, n_steps, scheme="ints", n0=N0, nlist=NLIST, add_sizes=ADD_SIZES, bulk=BULK_ADD):
    """-> [(rule, args)] of ``n_steps`` steps after ``initial_step``: every rule of ``rules`` at least once (a shuffled agenda,
    then uniform draws), with the follow-ups that make the stale-state traps certain instead of likely:
    the first removal is followed by an add of exactly as many rows, remove_all by an add, and the first add of an index walk is the bulk add, followed by nprobe = nlist.
    Every args dict also records ``n_before`` / ``n_after`` (rows) for ``transitions``; pure: the same seed gives the same list.
    Option walks also follow the first add that leaves room in the capacity by an add of one row without boosts, and the
    first remove_big_boosts that leaves the bound stale by a reload.
    A rule set with ``set_boosts`` is an OPTION walk: its first add and (by a fifth flag) its adds carry boosts, and every
    args dict also records the long-lived index's boost bound and a fresh index's, before and after the step
    (``bound_before`` / ``bound_after`` / ``true_before`` / ``true_after``).  For every other rule set not one random number
    more is drawn than before there were option walks."""
    assert scheme in ID_SCHEMES
    options = "set_boosts" in rules
    rng = np.random.default_rng(seed)
    st = _State(scheme, n0, options)
    _add(st, np.random.default_rng(0), n0, True, True, True, False, boosts=True if options else None)
    alias = {"remove_ads": "remove", "add_ads": "add"}
    add_rule = "add_ads" if "add_ads" in rules else "add"
    agenda = [rules[i] for i in rng.permutation(len(rules))]
    forced, steps, n_removals, bulk_done, room_done, stale_done = [], [], 0, False, False, False
    before = {}

    def emit(rule, args):
        args.setdefault("n_before", len(st.ids))
        args.setdefault("n_after", len(st.ids))
        args["nprobe"] = st.nprobe
        if options:
            args.update(before, bound_after=st.bound, true_after=st.true_bound)
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
        if options:
            before = dict(bound_before=st.bound, true_before=st.true_bound)
        if n == 0 and kind not in ("add", "add_big_boosts", "reload", "nprobe"):
            rule = add_rule                                                     # nothing to remove or to set on an empty corpus
            kind, hint = "add", None
        if kind == "remove_big_boosts" and not set(st.big_ids) & set(st.ids):
            forced.insert(0, ("remove_big_boosts", None))                       # no such row (left): first the add, then this
            kind = rule = "add_big_boosts"
        if kind == "add":
            if hint is not None:
                m = hint
            elif not bulk_done and bulk and "nprobe" in rules:
                m, bulk_done = bulk, True
                forced.append(("nprobe", nlist))
            else:
                m = add_sizes[int(rng.integers(len(add_sizes)))]
            plain = isinstance(m, tuple)                                        # (option walks) a forced add WITHOUT boosts
            m = m[1] if plain else m
            flags = rng.integers(0, 2, 5 if options else 4)
            _, args = _add(st, rng, m, flags[0], flags[1], flags[2], bool(flags[3]),
                           boosts=(flags[4] and not plain) if options else None)
            if options and not room_done and args["grew"] and st.cap > len(st.ids):
                # the first add that leaves room is followed by one row without boosts: the in-place zero_() of its boost
                room_done = True
                forced.insert(0, (add_rule, ("plain", 1)))
            emit(rule, args)
        elif kind == "add_big_boosts":
            m = add_sizes[int(rng.integers(len(add_sizes)))]
            flags = rng.integers(0, 2, 3)
            # 4 x the long-lived bound (2.0 at the least): larger than every boost ever stored, a power of two times BOOST_SCALE
            scale = 4.0 * max(1.0, st.bound / BOOST_SCALE)
            _, args = _add(st, rng, m, flags[0], flags[1], flags[2], False, boosts=True, scale=scale)
            st.big_ids = list(dict.fromkeys(args["ids"]))
            emit(rule, args)
        elif kind in ("remove", "remove_all", "remove_set_tags", "remove_set_boosts", "remove_big_boosts"):
            distinct = list(dict.fromkeys(st.ids))
            if kind == "remove_all":
                chosen = distinct
                forced.insert(0, (add_rule, add_sizes[-1]))
            elif kind == "remove_big_boosts":
                there = set(st.ids)
                chosen = [x for x in st.big_ids if x in there]
                st.big_ids = []
            else:
                cnt = int(rng.integers(1, max(2, len(distinct) // 4)))
                chosen = [distinct[i] for i in rng.choice(len(distinct), size=cnt, replace=False)]
            gone = set(chosen)
            removed = sum(1 for x in st.ids if x in gone)
            listed = chosen + [st.absent(0), st.absent(1)] + chosen[:3]         # absent ids, duplicates
            if options:
                st.babs = st.babs[np.array([x not in gone for x in st.ids], dtype=bool)]
            st.ids = [x for x in st.ids if x not in gone]
            st.cap = len(st.ids)                                                # the gathers are exact-size
            if kind == "remove":
                n_removals += 1
                if n_removals == 1:
                    forced.insert(0, (add_rule, removed))
            args = dict(ids=listed, removed=removed, n_before=n, n_after=len(st.ids), vseed=int(rng.integers(1 << 30)))
            if kind == "remove_big_boosts" and not stale_done and "reload" in rules and st.bound > st.true_bound:
                stale_done = True                                               # probed with the stale bound, then reloaded with it
                forced.insert(0, ("reload", None))
            if kind == "remove_set_boosts" and len(st.ids):
                st.babs = np.abs(step_boosts(kind, args))
                st.bound = st.true_bound
            emit(rule, args)
        elif kind in ("set_tags", "set_groups", "set_bids", "set_boosts", "tower_update", "ranker_update", "load_state_dict"):
            args = dict(vseed=int(rng.integers(1 << 30)))
            if kind == "set_boosts":
                st.babs = np.abs(step_boosts(kind, dict(args, n_after=n)))
                st.bound = st.true_bound
            emit(rule, args)
        elif kind == "nprobe":
            st.nprobe = int(hint if hint is not None else NPROBES[int(rng.integers(len(NPROBES)))])
            emit(rule, dict(value=st.nprobe))
        elif kind == "reload":
            st.cap = reserve_capacity(0, n)                                     # a loaded index reserves for its rows
            st.bound = st.true_bound if options else st.bound                   # ... and takes its bound from them
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


REQUIRED_TRANSITIONS_OPTIONS = ("set_boosts_before_boosted_search", "remove_then_set_boosts", "boost_bound_grows_with_add",
                                "boost_bound_outlives_its_rows", "add_without_boosts_within_capacity",
                                "add_without_boosts_grows_capacity", "reload_with_stale_boost_bound")
MIXED_PROBE = (33, 10)           # PROBES_OPTIONS' k = 10 probe has one query, which never takes the grouped scan: the batch that
#                                  reaches the two-phase scan's bf16-prefiltered second phase (run where mixed_second_phase says so)


def mixed_second_phase(n, nprobe, nlist=NLIST, probe=MIXED_PROBE):
    """Does ``probe`` on an IVF index of ``n`` rows take the two-phase scan with the prefiltered second phase? (amdrec.ivf's
    own dispatch arithmetic)"""
    from amdrec import ivf
    p = min(max(1, nprobe), nlist)
    return bool(n and ivf.use_grouped_scan(probe[0], p, nlist) and p >= ivf.TWO_PHASE_MIN_PROBES and
                ivf.use_mixed_scan(n, nlist, p, probe[1]))


def transitions_options(steps, nlist=NLIST, probes=PROBES_OPTIONS):
    """``transitions`` of an option walk plus the named transitions of its boost state (every step is followed by the whole
    probe set, boosted searches included).  The select-path switches are looked for along the whole sequence of probes, the
    last probe of a step and the first of the next included: PROBES_OPTIONS ends on its 512 queries."""
    found = transitions(steps, nlist, probes)
    paths = [select_path(a["n_after"], a["nprobe"], nlist, nq) for _, a in steps for nq, _ in probes]
    for p, q in zip(paths, paths[1:]):
        if (p, q) == ("single", "split"):
            found.add("split_after_single")
        if (p, q) == ("split", "single"):
            found.add("single_after_split")
    for i, (rule, a) in enumerate(steps):
        if rule in ("set_boosts", "remove_set_boosts"):
            found.add("set_boosts_before_boosted_search")
        if rule == "remove_set_boosts" and a["removed"] > 0 and a["n_after"] > 0:
            found.add("remove_then_set_boosts")
        if rule in ("add", "add_ads", "add_big_boosts"):
            if a["boosts"] and a["n_before"] > 0 and a["bound_after"] > a["bound_before"] > 0:
                found.add("boost_bound_grows_with_add")
            if not a["boosts"]:                                  # (an option walk's index holds a boost tensor from its first add)
                found.add("add_without_boosts_grows_capacity" if a["grew"] else "add_without_boosts_within_capacity")
        if "removed" in a and a["n_after"] > 0 and a["bound_after"] > a["true_after"]:
            found.add("boost_bound_outlives_its_rows")
        if rule == "reload" and a["bound_before"] > a["true_before"] and a["n_after"] > 0:
            found.add("reload_with_stale_boost_bound")
        if mixed_second_phase(a["n_after"], a["nprobe"], nlist):
            found.add("mixed_second_phase")
    return found


def late_walk(kind):
    """The late opt-ins' walk of ``kind`` ("ivf" / "ivfpq"): ``walk`` over LATE_RULES with LATE_ENABLES[kind] inserted, in
    that order, before seeded steps (never before the first, so that the unflagged index is probed at least once; never two
    before the same step).  An enable step's args hold ``flags``: the flags that are on AFTER it; every other step's too."""
    seed, n = LATE_WALKS[kind]
    base = walk(seed, LATE_RULES, n, "ints", bulk=0)
    enables = LATE_ENABLES[kind]
    at = sorted(np.random.default_rng(seed + 1000).choice(np.arange(1, n), size=len(enables), replace=False).tolist())
    steps, flags = [], ()
    for i, (rule, a) in enumerate(base):
        if i in at:
            e = enables[at.index(i)]
            flags = flags + ((e[len("enable_"):],) if e.startswith("enable_") else ())
            steps.append((e, dict(vseed=seed * 1000 + i, n_before=a["n_before"], n_after=a["n_before"],
                                  nprobe=steps[-1][1]["nprobe"], flags=flags)))
        steps.append((rule, dict(a, flags=flags)))
    return steps


# ---- the twins-----------------------------------------------------------------------------------------------------------------
def index_kinds(nlist=NLIST):
    """tests.test_exclude_gpu.KINDS at the walks' nlist, the IVF kinds with list-order tags (they take masks)."""
    from tests.test_exclude_gpu import KINDS
    return {k: dict(v, nlist=nlist, list_tags=True) if v["index_type"] != "Flat" else dict(v) for k, v in KINDS.items()}


def index_kinds_options(nlist=NLIST):
    """The option walks' kinds: both Flat engines; IVF with every flag; the IVFPQ kinds with the flags they take (an IVFPQ
    index has no list boosts)."""
    from tests.test_exclude_gpu import KINDS
    flags = {"ivf": dict(list_tags=True, list_boosts=True, aware_probes=True),
             "ivfpq": dict(list_tags=True, aware_probes=True), "ivfpq_refine_fp32": dict(list_tags=True, aware_probes=True)}
    return {k: dict(KINDS[k], **(dict(flags[k], nlist=nlist) if k in flags else {}))
            for k in ("flat_bf16", "flat_fp32", "ivf", "ivfpq", "ivfpq_refine_fp32")}


FLAGS = ("list_tags", "list_boosts", "aware_probes")


def takes_boosts(kw):
    """Does an index constructed with ``kw`` take boosts?  (amdrec.boost: Flat; IVF with ``list_boosts``)"""
    return kw["index_type"] == "Flat" or (kw["index_type"] == "IVF" and bool(kw.get("list_boosts")))


def flagged_trained_file(trained_file, kw, path):
    """``trained_file`` (a trained, empty index saved WITHOUT flags) saved again with the flags of ``kw`` in its header ->
    ``path``: what an index constructed with ``kw`` and trained the same way would have saved (load() takes the flags from
    the file, so a twin with other flags than the file's needs a file of its own)."""
    from amdrec.index import FAISSIndex
    idx = FAISSIndex(**kw)
    idx.load(trained_file)
    assert idx.index.ntotal == 0
    for f in FLAGS:
        setattr(idx, f, bool(kw.get(f, False)))
    idx.save(path)
    return path


def fresh_index(kind, model, trained_file, dim=None, kinds=None, boosts=False):
    """A new FAISSIndex in the trained state saved in ``trained_file`` (saved empty, before the first add), given the
    model's rows in ONE add with explicit ids, tags, groups and bids, at the model's nprobe.  ``boosts``: the long-lived
    index holds a boost tensor - the twin gets the model's boosts where its kind takes them."""
    from amdrec.index import FAISSIndex
    kinds = index_kinds() if kinds is None else kinds
    idx = FAISSIndex(model.dim if dim is None else dim, **kinds[kind])
    idx.load(trained_file)
    assert idx.index_type == kinds[kind]["index_type"] and idx.index.ntotal == 0 and idx.index.is_trained
    if idx.index_type != "Flat":
        assert [getattr(idx, f) for f in FLAGS] == [bool(kinds[kind].get(f, False)) for f in FLAGS], "the file's flags"
    boosts = boosts and takes_boosts(kinds[kind])
    if model.n:
        idx.add(model.rows, list(model.ids), tags=model.tags, groups=model.groups, bids=model.bids,
                **({"boosts": model.boosts} if boosts else {}))
    else:
        # an add of zero rows cannot hand over attributes; the long-lived index still HOLDS (zero) keys and bids after its
        # last row left, and an index that holds none refuses caps and the auction: give the twin its empty ones
        idx.set_tags(model.tags)
        idx.set_groups(model.groups)
        idx.set_bids(model.bids)
        if boosts:                                               # ... and one that holds no boosts refuses boost_weight
            idx.set_boosts(model.boosts)
    if idx.index_type != "Flat":
        idx.nprobe = model.nprobe
    return idx


def fresh_pipeline(model, tower_sd, ranker_sd, knobs):
    """A new AdRecommenderInference: new modules from the state dicts (read off the long-lived ones with ``state_dict()``), a
    new ad table from the model, ``fresh_index``.  ``knobs``: dict(make_tower, make_ranker: constructors of empty modules;
    kind, trained_file, kinds, boosts: as fresh_index; heads: the heads mode; ranker: attribute switches to set)."""
    import torch
    from amdrec.pipeline import AdRecommenderInference
    tt = knobs["make_tower"]()
    tt.load_state_dict({k: v.detach().clone().cpu() for k, v in tower_sd.items()})
    rk = knobs["make_ranker"]()
    rk.load_state_dict({k: v.detach().clone().cpu() for k, v in ranker_sd.items()})
    for name, value in knobs.get("ranker", {}).items():
        setattr(rk, name, value)
    idx = fresh_index(knobs["kind"], model, knobs["trained_file"], kinds=knobs.get("kinds"), boosts=knobs.get("boosts", False))
    table = torch.from_numpy(np.ascontiguousarray(model.feats, dtype=np.int64))
    return AdRecommenderInference(two_tower_model=tt, transformer_ranker=rk, faiss_index=idx, ad_features=table,
                                  heads=knobs.get("heads", "all"))
