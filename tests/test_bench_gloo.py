"""``bench.py --gpus N`` without a GPU: ``main()`` runs under gloo with world 2 over the fake engine of
tests/fake_engine.py, started exactly the way the driver starts it (one process per rank, RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* in the environment).  Checked: ONE JSON line, from rank 0 only; ``n_gpus``, ``steps``, ``warmup`` echo the
command line; ``value`` = world x B x K / (the max-over-ranks time the line reports as ms_per_step); ranks != 0 build
their models EMPTY and end up with rank 0's weights through the broadcast hook alone.  A plain run carries the headline alone;
the legs beside it (``engine_only``, ``replica_runners``, ...) come with ``--full``."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_main_world2_gloo_fake_engine(tmp_path):
    world, B, K, Wm = 2, 4, 2, 1
    port = str(_free_port())
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", str(world), "--steps", str(K), "--warmup", str(Wm), "--fake-engine",
           "--full", "--batch", str(B), "--height", "72", "--width", "128", "--scales", "players=n,ball=n,pose=n"]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{se[-3000:]}"
    assert outs[1][0].strip() == "", "only rank 0 prints"
    lines = [l for l in outs[0][0].splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["fake_engine"] is True and d["n_gpus"] == world and d["steps"] == K and d["warmup"] == Wm
    assert d["metric"].startswith("frames/sec") and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["config"]["frames_per_gpu_per_step"] == B
    # value = whole-job frames / (max over ranks of the timed region)
    assert abs(d["value"] - world * B * K / (d["ms_per_step"] * K / 1e3)) <= 0.02 * d["value"]
    # N > 1: `value` is the SHARDED runner (one clip of world x K x B frames, TrackingRunner(distributed=True): packed gather to
    # rank 0, ByteTrack there); the independent-replica number stays beside it
    rep = d["replica_runners"]
    assert abs(rep["value"] - world * B * K / (rep["ms_per_step"] * K / 1e3)) <= 0.02 * rep["value"]
    assert "distributed=True" in d["config"]["timed_path_n_gpus"]
    assert "strings_over_120_chars" not in d, d.get("strings_over_120_chars")          # the driver cuts longer strings in the fields it keeps
    assert d["config"]["tracked_players_rank0"] > 0                     # rank 0 holds the merged results of ALL shards
    assert d["config"]["frames_with_results_rank0"] == {"players": world * K * B, "ball": world * K * B, "pose": world * K * B}
    assert set(d["config"]["runner_seconds_per_tracker_rank0"]) == {"players_tracker", "ball_tracker", "players_keypoints_tracker"}
    e = d["engine_only"]
    assert abs(e["value"] - world * B * K / (e["ms_per_step"] * K / 1e3)) <= 0.02 * e["value"]
    # three trackers x (1 warm-up + K) fake steps of 10 ms each, at least: the timed region is real
    assert e["ms_per_step"] >= 3 * 10.0 * 0.9
    r0, r1 = d["ranks"]
    assert (r0["rank"], r1["rank"]) == (0, 1)
    assert sum("model created empty=False" in x for x in r0["log"]) == 3 and not any("empty=True" in x for x in r0["log"])
    assert sum("model created empty=True" in x for x in r1["log"]) == 3, r1["log"]
    assert sum("bcast root=0 had_weights=False" in x for x in r1["log"]) == 3 and sum("bcast root=0 had_weights=True" in x for x in r0["log"]) == 3
    assert any("comm_init nranks=2 rank=1" in x for x in r1["log"])
    # round 6: the sharded runner's gathers travel over the ENGINE's communicator (pa_engine_gather on the GPU box), not torch's
    assert any("gather_bytes via the engine's communicator" in x for x in r0["log"]) and any("gather_bytes via the engine's communicator" in x for x in r1["log"])
    assert r1["weight_checksums"] == r0["weight_checksums"] and all(v != 0 for v in r0["weight_checksums"].values())
    # the sharded runner's device stage goes through the two-call form (submit_sample / collect_sample -> yolo_submit / yolo_wait)
    assert "submit" in r0["log"] and "submit" in r1["log"]


def _fake_bench_world1(tmp_path, *args):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--warmup", "1", "--fake-engine", "--batch", "4", "--height", "72",
           "--width", "128", "--scales", "players=n,ball=n,pose=n", *args]
    p = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout)


FULL_LEGS = ("engine_only", "objects_materialised", "value_lazy_objects", "value_eager_objects", "host_frames", "reference_default",
             "roofline", "cpu_baseline", "parity", "replica_runners")


def test_plain_run_times_the_headline_alone(tmp_path):
    """Without ``--full`` the line carries the contract fields and none of the other legs; ``--full`` brings them back (under the
    fake engine, which implies ``--quick``: the engine-only, object-count and lazy-object legs)."""
    B, K = 4, 2
    d = _fake_bench_world1(tmp_path, "--steps", str(K))
    assert not [k for k in FULL_LEGS if k in d], [k for k in FULL_LEGS if k in d]
    assert d["metric"].startswith("frames/sec") and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["steps"] == K and d["warmup"] == 1 and d["n_gpus"] == 1
    assert abs(d["value"] - B * K / (d["ms_per_step"] * K / 1e3)) <= 0.02 * d["value"]
    assert d["config"]["frames_with_results_rank0"] == {"players": K * B, "ball": K * B, "pose": K * B}
    assert d["config"]["engine_only_frames_per_s"] is None
    f = _fake_bench_world1(tmp_path, "--steps", str(K), "--full")
    assert {"engine_only", "objects_materialised", "value_lazy_objects"} <= set(f)
    assert f["config"]["engine_only_frames_per_s"] == f["engine_only"]["value"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert f[k] == d[k], k


def test_plain_run_without_warmup(tmp_path):
    """``--warmup 0``: one untimed pass through every model (one ``yolo_infer`` each) stands in for the engine-only leg that used
    to precede the runner; the line and the results are those of K timed steps."""
    B, K = 4, 2
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "0", "--fake-engine", "--batch", str(B),
           "--height", "72", "--width", "128", "--scales", "players=n,ball=n,pose=n"]
    p = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout)
    assert d["steps"] == K and d["warmup"] == 0 and not [k for k in FULL_LEGS if k in d]
    assert abs(d["value"] - B * K / (d["ms_per_step"] * K / 1e3)) <= 0.02 * d["value"]
    assert d["config"]["frames_with_results_rank0"] == {"players": K * B, "ball": K * B, "pose": K * B}
    log = d["ranks"][0]["log"]
    # the priming pass comes before the runner's first submit
    assert "submit" in log and any("infer" in x for x in log[:log.index("submit")]), log


def test_plain_run_world2_is_the_sharded_runner_alone(tmp_path):
    """N > 1 without ``--full``: no replica runners in front, ``value`` is the sharded runner, rank 0 holds all shards."""
    world, B, K = 2, 4, 2
    port = str(_free_port())
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", str(world), "--steps", str(K), "--warmup", "1", "--fake-engine",
           "--batch", str(B), "--height", "72", "--width", "128", "--scales", "players=n,ball=n,pose=n"]
    procs = [subprocess.Popen(cmd, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                                       MASTER_PORT=port, OMP_NUM_THREADS="2")) for r in range(world)]
    outs = [p.communicate(timeout=900) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{se[-3000:]}"
    assert outs[1][0].strip() == ""
    d = json.loads(outs[0][0])
    assert not [k for k in FULL_LEGS if k in d], [k for k in FULL_LEGS if k in d]
    assert d["n_gpus"] == world and "distributed=True" in d["config"]["timed_path_n_gpus"]
    assert abs(d["value"] - world * B * K / (d["ms_per_step"] * K / 1e3)) <= 0.02 * d["value"]
    assert d["config"]["frames_with_results_rank0"] == {"players": world * K * B, "ball": world * K * B, "pose": world * K * B}


def test_dump_ops_needs_full(tmp_path):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--fake-engine", "--dump-ops", str(tmp_path / "ops.csv")], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--full" in p.stderr and p.stdout == ""


def test_bench_dump_outputs_is_the_last_timed_step(tmp_path):
    """``--dump-outputs DIR``: float64 tables of what the timed runner returned for its last step — frames (K - 1) B .. K B - 1
    in column 0 — identical from run to run; ``--steps`` sets the number of timed steps.  ``--engine-only``: the arrays of the
    last engine-only step (frames 0 .. B - 1 of the batch)."""
    B, K = 4, 3
    for run in ("a", "b"):
        d = _fake_bench_world1(tmp_path, "--steps", str(K), "--dump-outputs", str(tmp_path / run))
        assert d["steps"] == K and d["config"]["frames_with_results_rank0"] == {"players": K * B, "ball": K * B, "pose": K * B}
    for name, width in (("players", 8), ("ball", 4), ("pose", 1 + 13 * 2)):
        x = np.load(tmp_path / "a" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape[1:] == (width,) and len(x) > 0, (name, x.dtype, x.shape)
        assert set(x[:, 0].tolist()) <= set(range((K - 1) * B, K * B)), name
        np.testing.assert_array_equal(x, np.load(tmp_path / "b" / f"{name}.npy"))
    assert np.load(tmp_path / "a" / "ball.npy")[:, 0].tolist() == list(range((K - 1) * B, K * B))      # one row per frame
    _fake_bench_world1(tmp_path, "--steps", str(K), "--engine-only", "--dump-outputs", str(tmp_path / "e"))
    for name, width in (("players", 7), ("ball", 7), ("pose", 7 + 13 * 3)):
        x = np.load(tmp_path / "e" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape[1:] == (width,) and len(x) > 0, (name, x.dtype, x.shape)
        assert set(x[:, 0].tolist()) <= set(range(B)), name


def test_dump_outputs_seeded_sample_under_the_limit(tmp_path, monkeypatch):
    """Tables larger than the limit in all keep the same fraction of their rows, the same rows every time, in order."""
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 6400)
    tables = {"a": np.arange(800.0).reshape(100, 8), "b": np.arange(400.0).reshape(100, 4)}
    bench.write_outputs(tmp_path / "x", tables)
    bench.write_outputs(tmp_path / "y", tables)
    a, b = np.load(tmp_path / "x" / "a.npy"), np.load(tmp_path / "x" / "b.npy")
    assert a.nbytes + b.nbytes <= 6400 and len(a) == len(b) == 66
    assert (np.diff(a[:, 0]) > 0).all() and np.isin(a, tables["a"]).all() and (a[:, 0] % 8 == 0).all()
    np.testing.assert_array_equal(a, np.load(tmp_path / "y" / "a.npy"))
    np.testing.assert_array_equal(b, np.load(tmp_path / "y" / "b.npy"))
