"""CPU: every ``*_workspace`` query answers the byte counts recorded in tests/golden/workspace_sizes.json, over tables that
cross each conditional term of its layout.  The numbers were taken from the library as it was BEFORE the layouts moved
onto one carving helper (csrc/common.hpp, Carver), through AMDREC_LIB_PATH: a layout function that drifts from them changes
what callers must allocate.  ``python -m tests.test_workspace_layout FILE`` writes the table of the loaded library."""
import ctypes as C
import itertools
import json
import os

import pytest

from tests.conftest import GOLDEN  # first: puts the package on sys.path when this file runs as a script
from tests import cases

RECORDED = os.path.join(GOLDEN, "workspace_sizes.json")
# nq 128 / 129 crosses FUSED_MAX_NQ, nrows 8192 / 8193 crosses CAND_CAP, dim 72 is not a streaming-kernel dim
FLAT_NQ, FLAT_NROWS, FLAT_K, FLAT_DIM = (1, 8, 9, 32, 33, 64, 65, 128, 129, 512), (0, 8192, 8193, 1_000_000), (1, 500, 2048), (8, 64, 72, 256)
MODEL_ROWS = (0, 1, 127, 129, 262144, 262145)           # 262144 / 262145 crosses ROW_CHUNK
MODEL_CASES = ("demo", "tutorial")


def sizes():
    """{query: {"arg,arg,...": bytes}} of the loaded library."""
    from amdrec import _lib, weights
    lib = _lib.load()
    n = C.c_size_t(0)

    def ask(fn, *args):
        assert fn(*args, C.byref(n)) == 0, lib.amdrec_last_error()
        return n.value

    key = lambda *a: ",".join(str(x) for x in a)   # noqa: E731
    out = {"flat": {}, "flat_mixed": {}, "kmeans": {}, "ivfpq_train": {}, "tower": {}, "ranker": {}}
    for nq, nrows, k in itertools.product(FLAT_NQ, FLAT_NROWS, FLAT_K):
        out["flat"][key(nq, nrows, k)] = ask(lib.amdrec_flat_search_workspace, nq, nrows, k)
        for dim in FLAT_DIM:
            out["flat_mixed"][key(nq, nrows, k, dim)] = ask(lib.amdrec_flat_search_mixed_workspace, nq, nrows, k, dim)
    for rows, nlist, dim in itertools.product((1, 31, 100_000), (1, 100, 4096), (4, 256)):
        out["kmeans"][key(rows, nlist, dim)] = ask(lib.amdrec_ivf_kmeans_workspace, rows, dim, nlist)
    for rows, m in itertools.product((1, 31, 100_000), (4, 8, 16, 32)):
        out["ivfpq_train"][key(rows, m)] = ask(lib.amdrec_ivfpq_train_workspace, rows, 128, m)
    for name in MODEL_CASES:
        user, ad, nnum, sd, _ = cases.two_tower_case(name)
        towers = {"ad_tower": weights.pack_tower(sd, "ad_tower", list(ad), 0, "cpu"),
                  "user_tower": weights.pack_tower(sd, "user_tower", list(user), nnum, "cpu")}
        user, ad, nnum, sd, _ = cases.ranker_case(name, "scaled")
        rp = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu")
        for rows in MODEL_ROWS:
            for tower, packed in towers.items():
                out["tower"][key(name, tower, rows)] = ask(lib.amdrec_tower_workspace, C.byref(packed[0]), rows)
            out["ranker"][key(name, rows)] = ask(lib.amdrec_ranker_workspace, C.byref(rp[0]), rows)
    return out


@pytest.fixture(scope="module")
def got():
    return sizes()


@pytest.mark.parametrize("query,count", [("flat", 120), ("flat_mixed", 480), ("kmeans", 18), ("ivfpq_train", 12),
                                         ("tower", 24), ("ranker", 12)])
def test_workspace_query_answers_the_recorded_bytes(got, query, count):
    with open(RECORDED) as f:
        want = json.load(f)[query]
    assert len(want) == count and sorted(got[query]) == sorted(want)
    wrong = {k: (got[query][k], v) for k, v in want.items() if got[query][k] != v}
    assert not wrong, f"{query}: (got, recorded) {wrong}"


def test_the_table_crosses_every_conditional_term_of_the_flat_layout(got):
    """The thresholds the table is built around do change the recorded sizes (else it would pin nothing there)."""
    mixed = got["flat_mixed"]
    per_query = lambda nq, nrows: mixed[f"{nq},{nrows},500,64"] / nq   # noqa: E731
    assert per_query(129, 8193) < per_query(128, 8193)         # FUSED_MAX_NQ: no re-scored key list past it
    assert mixed["9,8193,500,64"] > mixed["9,8192,500,64"]     # CAND_CAP: the sample buffer appears
    assert mixed["9,8193,500,72"] > mixed["9,8193,500,64"] > got["flat"]["9,8193,500"]     # bf16 queries; mixed-only buffers


if __name__ == "__main__":
    import sys
    with open(sys.argv[1], "w") as f:
        json.dump(sizes(), f, indent=0, sort_keys=True)
        f.write("\n")
