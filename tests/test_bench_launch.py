"""bench.py's N > 1 launch path on CPU: `python bench.py --gpus N` without WORLD_SIZE must start N
ranks itself - before anything touches a GPU - and a world that differs from --gpus must exit non-zero instead of printing
a line with the wrong n_gpus.  --dry-run forms the world (launcher, rendezvous over gloo, world-size agreement) and
prints a stub line; the measured N = 2 run on a GPU is tests/test_sharded_gpu.py::test_bench_rehearsal_*."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "LOCAL_WORLD_SIZE")}
    env.update(extra)
    return env


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1, 2, 4])
def test_self_launch_forms_a_world_of_n_ranks(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--dry-run"], env=_env(), capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                           # ONE line, from rank 0
    doc = json.loads(lines[0])
    assert doc["n_gpus"] == n and doc["config"]["world"] == n and doc["dry_run"] is True


@pytest.mark.timeout(300)
def test_world_size_mismatch_exits_non_zero_and_prints_no_line():
    # torchrun started 1 rank but the command line says 2 (the r2 bug: it printed "n_gpus": 1)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=_env(WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode != 0 and "refusing to run" in r.stderr and "{" not in r.stdout
    # ... and the other way round
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run"],
                       env=_env(WORLD_SIZE="2", RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999"),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode != 0 and "{" not in r.stdout


@pytest.mark.timeout(300)
def test_a_failing_rank_fails_the_launch():
    # rank 1 of 2 cannot start (bad flag only it sees is not expressible; use an env switch read by --dry-run instead)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=_env(AMDREC_BENCH_FAIL_RANK="1"),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode != 0 and "{" not in r.stdout


def test_launcher_runs_before_torch_is_imported():
    """The parent of a self-launched run must never initialise the GPU: the launcher sits above `import torch`."""
    src = open(BENCH).read()
    assert src.index("sys.exit(launch_ranks(") < src.index("import torch")


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    """--dump-outputs: every tensor of the result dict becomes <name>.npy, floats as float32, ids as float64 (exact);
    past the byte limit each array is cut to the same seeded sample on every call."""
    import numpy as np
    import torch
    import bench
    ids = torch.arange(4 * 500, dtype=torch.int64).reshape(4, 500) * 977
    out = {"ad_ids": ids[:, :10], "candidate_ids": ids, "logits": torch.randn(3, 2000), "tasks": ["ctr", "a", "b"],
           "scores": torch.rand(3, 4, 10, dtype=torch.float16)}
    written = bench.dump_outputs(out, str(tmp_path / "full"))
    assert sorted(written) == ["ad_ids.npy", "candidate_ids.npy", "logits.npy", "scores.npy"]
    a = np.load(tmp_path / "full" / "candidate_ids.npy")
    assert a.dtype == np.float64 and np.array_equal(a, ids.numpy())
    lg = np.load(tmp_path / "full" / "logits.npy")
    assert lg.dtype == np.float32 and np.array_equal(lg, out["logits"].numpy())
    assert np.load(tmp_path / "full" / "scores.npy").dtype == np.float32
    assert bench.dump_outputs(out, str(tmp_path / "r1"), rank=1) == {k.replace(".npy", ".rank1.npy"): v
                                                                     for k, v in written.items()}
    limit = 20_000
    s1 = bench.dump_outputs(out, str(tmp_path / "s1"), limit=limit)
    s2 = bench.dump_outputs(out, str(tmp_path / "s2"), limit=limit)
    assert s1 == s2
    assert sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in s1) <= limit
    for f in s1:
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_runs_the_steps_asked_for_and_dumps_the_last_one(tmp_path):
    """One small single-GPU bench run: the line reports the timed steps it was given and ms_per_step, and the dumped
    last step is a consistent recommend_device result (every top-10 id is one of that user's stage-1 candidates)."""
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--ads", "200000",
                        "--no-cpu-baseline", "--no-strict-fp32", "--no-latency-sweep", "--no-search-sweep",
                        "--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=880)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    doc = json.loads(lines[0])
    assert doc["steps"] == 3 and doc["ms_per_step"] > 0 and doc["value"] > 0
    assert doc["dumped_outputs"]["dir"] == str(d)
    ad_ids, cand = np.load(d / "ad_ids.npy"), np.load(d / "candidate_ids.npy")
    assert ad_ids.dtype == cand.dtype == np.float64 and ad_ids.shape == (512, 10) and cand.shape == (512, 500)
    assert all(set(ad_ids[b]) <= set(cand[b]) for b in range(512))
    for name, shape in (("logits", (3, 512 * 500)), ("scores", (3, 512, 10)), ("candidate_scores", (512, 500))):
        a = np.load(d / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), name
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20


def test_full_is_off_by_default():
    """A plain run is the headline run: every other figure and check waits for --full."""
    import bench
    assert bench.parse_args(["--gpus", "1"]).full is False
    assert bench.parse_args(["--gpus", "1", "--full"]).full is True


def _bench_line(args, **extra_env):
    r = subprocess.run([sys.executable, BENCH, *args], env=_env(**extra_env), capture_output=True, text=True, timeout=880)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_run_carries_the_headline_and_nothing_that_took_runs_of_its_own(gpus):
    """No --full: the headline and what the warm-up and timed steps measured; the one-batch replay, the strict fp32
    figure, the sweeps, the CPU legs and (N > 1) the unverified region and stage times are left out.  N = 2 runs both
    ranks on one GPU (the rehearsal switch)."""
    env = {"AMDREC_BENCH_REHEARSE": "1"} if gpus > 1 else {}
    doc = _bench_line(["--gpus", str(gpus), "--steps", "2", "--warmup", "1", "--ads", "200000"], **env)
    assert doc["full"] is False and doc["n_gpus"] == gpus and doc["steps"] == 2 and doc["warmup_steps_run"] >= 20
    assert doc["metric"].startswith("end-to-end recs/sec") and doc["unit"] == "recs/s" and doc["higher_is_better"] is True
    assert doc["value"] > 0 and doc["ms_per_step"] > 0 and doc["dtype"].startswith("f32")
    assert doc["kernels"] and doc["roofline"]["avg_launch_ms"] > 0
    assert doc["same_batch"] is None and doc["strict_fp32"] is None
    assert doc["cpu_baseline"] is None and doc["parity_check"] is None and "e2e_latency_by_batch" not in doc
    if gpus == 1:
        assert doc["search"]["filter_pass_ms"] > 0 and "sweep" not in doc["search"]
    else:
        assert doc["config"]["no_verify"] is None and doc["multi_gpu"]["stages_ms_rank0"] is None
        assert doc["multi_gpu"]["verified"]["value"] > 0 and doc["config"]["shard_lists"]["inexact_in_timed_steps"] == 0


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_full_run_adds_every_figure_and_check():
    """--full at N = 1: the one-batch replay, the strict fp32-MFMA figure, the search sweep, the latency by batch and the
    CPU baseline with the full-size parity check of the timed step against the oracle."""
    doc = _bench_line(["--gpus", "1", "--steps", "2", "--warmup", "1", "--ads", "200000", "--full", "--cpu-users", "8"])
    assert doc["full"] is True and doc["value"] > 0
    assert doc["same_batch"]["value"] > 0
    assert doc["strict_fp32"]["value"] > 0 and doc["strict_fp32"]["engine"] == "fp32"
    assert [r["B"] for r in doc["search"]["sweep"]["rows"]] == [1, 8, 32, 128, 512]
    assert [r["B"] for r in doc["e2e_latency_by_batch"]] == [1, 8, 64, 512]
    assert doc["cpu_baseline"]["value"] > 0
    par = doc["parity_check"]
    assert par["users"] == 8 and par["topk_set_ok"] and par["top10_selection_exact"]
    assert par["max_logit_err_over_bound"] <= 1.0
