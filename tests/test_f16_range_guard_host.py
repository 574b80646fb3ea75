"""Host side of the fp16 range guard (no GPU, no engine):

* ``Graph.f16_weight_overflow``: an f16 graph says whether a conv weight, BatchNorm folded, leaves +-65504 (its packed half would
  be an infinity) and which layer it was; never for h2 / f32 graphs; the packed blob of an ordinary graph is what it was;
* ``YOLO(half=True)``, ``YOLO.set_half(True)`` and ``BallTracker(half=True)`` on such a checkpoint come up with ``half False`` and
  one printed line that names the layer;
* ``Tracker.arithmetic`` and one step of ``use_full_range()`` from each starting point of the ladder f16 -> default -> bx3;
* the sharded runner's decision (tests/range_guard_worker.py, gloo, world 2): rank 1 leaves f16 in the first attempt, rank 0
  leaves h2 in the second, both ranks end on bx3 with the predictions of a single-process bx3 run."""
import hashlib
import json
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import tracknet_ref as tr
from padel_analytics_amd import checkpoint, detections as D, engine as E, graph as G, yolo, yolo_arch
from padel_analytics_amd.trackers import BallTracker, PlayerTracker
from padel_analytics_amd.trackers.tracker import Tracker
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)

WORKER = str(Path(__file__).with_name("range_guard_worker.py"))


# ---- the graph ----------------------------------------------------------------------------------------------------------------------
def one_conv(dtype, value):
    g = G.Graph(task=G.TASK_TRACKNET, dtype=dtype)
    b0, b1 = g.buf(0, 32), g.buf(0, 32)
    w = np.full((32, 32, 3, 3), 0.01, np.float32)
    w[7, 3, 1, 2] = value
    g.conv((b0, 0, 32), (b1, 0), w, np.zeros(32, np.float32), 3, 1, G.ACT_RELU, name="the.layer")
    return g


@pytest.mark.parametrize("value,want", [(7.0e4, True), (-7.0e4, True), (65520.0, True), (np.nan, True), (np.inf, True),
                                        (65504.0, False), (-65504.0, False), (1.0, False)])
def test_f16_weight_overflow_of_one_conv(value, want):
    g = one_conv(G.DTYPE_F16, value)
    assert g.f16_weight_overflow is want and g.f16_overflow_layer == ("the.layer" if want else None)
    packed = g.blob()[:g.ops[0]["b_off"]].view(np.float16)
    assert bool(np.isfinite(packed).all()) is (not want)      # (65520 is the first fp32 value whose half is inf: ties go to even)
    for dtype in (G.DTYPE_H2, G.DTYPE_F32):
        if np.isfinite(value):
            g = one_conv(dtype, value)
            assert g.f16_weight_overflow is False and g.f16_overflow_layer is None


def hot_tracknet_sd(value=7.0e4):
    """One weight of down_block_2.conv_1 is ``value`` after the BatchNorm fold."""
    sd = dict(tr.synth_tracknet_state_dict(5))
    p = "down_block_2.conv_1"
    w, scale, _ = G.fold_bn_split(sd, p, G.TRACKNET_BN_EPS)
    w = np.array(w, np.float32)
    w[3, 5, 1, 1] = np.float32(value) / scale[3]
    sd[f"{p}.conv.weight"] = w
    assert abs(float(G.fold_bn(sd, p, G.TRACKNET_BN_EPS)[0][3, 5, 1, 1]) - value) < 1e-3 * abs(value)
    return sd


def hot_yolo_sd():
    sd = dict(yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5))
    p = "model.2.cv1"
    w, scale, _ = G.fold_bn_split(sd, p, yolo_arch.BN_EPS)
    w = np.array(w, np.float32)
    w[2, 4, 0, 0] = np.float32(7.0e4) / scale[2]
    sd[f"{p}.conv.weight"] = w
    return sd


def test_f16_weight_overflow_of_the_builders():
    sd = hot_tracknet_sd()
    g = G.build_tracknet(sd, "f16")
    assert g.f16_weight_overflow is True and g.f16_overflow_layer == "down_block_2.conv_1"
    assert not G.build_tracknet(sd, "h2").f16_weight_overflow and not G.build_tracknet(sd, "f32").f16_weight_overflow
    assert G.build_tracknet(hot_tracknet_sd(6.0e4), "f16").f16_weight_overflow is False
    ysd = hot_yolo_sd()
    g = G.build_yolov8(ysd, 80, None, dtype="f16")
    assert g.f16_weight_overflow is True and g.f16_overflow_layer == "model.2.cv1"
    assert not G.build_yolov8(ysd, 80, None, dtype="h2").f16_weight_overflow and not G.build_yolov8(ysd, 80, None, dtype="f32").f16_weight_overflow


def test_ordinary_f16_blobs_are_unchanged():
    """sha256 of the packed blobs as the commit before the guard packed them."""
    g = G.build_tracknet(tr.synth_tracknet_state_dict(5), "f16")
    assert g.f16_weight_overflow is False and g.f16_overflow_layer is None
    assert hashlib.sha256(g.blob().tobytes()).hexdigest() == "645a65489d0fd4433747cecf0c6a576effd50137d62f7111561303b0246db7f1"
    g = G.build_yolov8(yolo_arch.synth_state_dict("n", 1, (13, 3), seed=2, cls_bias=1.0), 1, (13, 3), dtype="f16")
    assert g.f16_weight_overflow is False and g.n_floats == 1704400
    assert hashlib.sha256(g.blob().tobytes()).hexdigest() == "6ff1dde2861e4b7158324cd5e717bfeeaa6af6d8db141148143c085b60695a1c"


# ---- construction on a checkpoint whose fp16 weights overflow ---------------------------------------------------------------------------
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("no engine is involved")
    monkeypatch.setattr(E, "default_engine", boom)
    monkeypatch.setattr(E, "Model", boom)


def test_yolo_half_on_a_hot_checkpoint(tmp_path, capsys, monkeypatch):
    no_engine(monkeypatch)
    ck = tmp_path / "hot.pt"
    checkpoint.save_checkpoint(ck, hot_yolo_sd(), "detect", 80, None, "n", {0: "person"})
    y = yolo.YOLO(str(ck), half=True)
    out = capsys.readouterr().out
    assert y.half is False and y.fell_back and y._model is None
    assert y.fp32_mode == E.fp32_mode() and y.graph.dtype == G.build_yolov8(hot_yolo_sd(), 80, None, dtype=E.graph_dtype()).dtype
    assert not y.graph.f16_weight_overflow and np.isfinite(y.graph.blob()).all()
    assert out.count("\n") == 1 and "model.2.cv1" in out and "fp16 range" in out, out
    # the same through set_half, and nothing of the kind without half
    y2 = yolo.YOLO(str(ck))
    assert capsys.readouterr().out == "" and not y2.fell_back and y2.arithmetic == ("h2" if E.fp32_mode() == "h2" else "bx3")
    y2.set_half(True)
    out = capsys.readouterr().out
    assert y2.half is False and y2.fell_back and y2.graph.dtype != G.DTYPE_F16 and "model.2.cv1" in out and out.count("\n") == 1
    # ... once: callers that pass half= with every predict() neither rebuild nor hear it again
    for obj in (y, y2):
        g = obj.graph
        obj.set_half(True)
        assert obj.graph is g and obj.half is False and capsys.readouterr().out == ""


def test_ball_tracker_half_on_a_hot_checkpoint(tmp_path, capsys, monkeypatch):
    no_engine(monkeypatch)
    sd = hot_tracknet_sd()
    ck = tmp_path / "hot_tracknet.pt"
    checkpoint.save_checkpoint(ck, sd, "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    t = BallTracker(str(ck), None, 8, half=True)
    out = capsys.readouterr().out
    default = G.build_tracknet(sd, E.graph_dtype())
    assert t.half is False and t._model is None and t.fp32_mode == E.fp32_mode() and t.graph.dtype == default.dtype
    assert t.graph.blob().tobytes() == default.blob().tobytes()
    said = [line for line in out.splitlines() if "fp16 range" in line]
    assert len(said) == 1 and "down_block_2.conv_1" in said[0], out
    assert BallTracker(str(ck), None, 8).half is False and "fp16 range" not in capsys.readouterr().out


# ---- Tracker.arithmetic, one step of use_full_range ---------------------------------------------------------------------------------
def _player(tmp_path, **kw):
    ck = tmp_path / "players.pt"
    if not ck.exists():
        checkpoint.save_checkpoint(ck, yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None, "n", {0: "person"})
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    return PlayerTracker(str(ck), zone, batch_size=4, **kw)


def test_arithmetic_and_the_steps_of_a_yolo_tracker(tmp_path, monkeypatch):
    no_engine(monkeypatch)
    monkeypatch.setattr(E, "fp32_mode", lambda: "h2")
    t = _player(tmp_path, half=True)
    assert t.arithmetic == "f16" and t.full_range and t.model.graph.dtype == G.DTYPE_F16
    t.use_full_range()                                      # f16 -> the default path
    assert t.arithmetic == "h2" and not t.full_range and not t.model.half and t.model.graph.dtype == G.DTYPE_H2
    t.use_full_range()                                      # h2 -> bx3
    assert t.arithmetic == "bx3" and t.full_range and t.model.graph.dtype == G.DTYPE_F32
    blob = t.model.graph.blob().tobytes()
    t.use_full_range()                                      # nothing beyond
    assert t.arithmetic == "bx3" and t.model.graph.blob().tobytes() == blob
    assert not t.model.fell_back, "a step somebody asks for is no overflow"
    t0 = _player(tmp_path)
    assert t0.arithmetic == "h2"
    t0.model.fp32_mode = "tap"
    assert t0.arithmetic == "f32"
    # a half model whose fp32_mode is bx3 goes there in one step
    t1 = _player(tmp_path, half=True)
    t1.model.set_fp32_mode("bx3")
    assert t1.arithmetic == "f16"
    t1.use_full_range()
    assert t1.arithmetic == "bx3" and t1.model.graph.dtype == G.DTYPE_F32


def test_arithmetic_and_the_steps_of_the_ball_tracker(tmp_path, monkeypatch):
    no_engine(monkeypatch)
    monkeypatch.setattr(E, "fp32_mode", lambda: "h2")
    ck = tmp_path / "tracknet.pt"
    checkpoint.save_checkpoint(ck, tr.synth_tracknet_state_dict(5), "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    t = BallTracker(str(ck), None, 8, half=True)
    seen = [t.arithmetic]
    for _ in range(3):
        t.use_full_range()
        seen.append(t.arithmetic)
    assert seen == ["f16", "h2", "bx3", "bx3"] and t.graph.dtype == G.DTYPE_F32 and not t.half
    assert BallTracker(str(ck), None, 8).arithmetic == "h2"


def test_a_tracker_without_a_model_has_no_arithmetic():
    class Bare:
        arithmetic = Tracker.arithmetic
        full_range = Tracker.full_range
        use_full_range = Tracker.use_full_range
    b = Bare()
    assert b.arithmetic is None and b.full_range
    b.use_full_range()
    assert b.arithmetic is None


# ---- the sharded decision -------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(mode, world, out):
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, WORKER, mode, str(r), str(world), port, str(out)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, log) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, f"rank {r} failed:\n{log[-3000:]}"
    return json.loads(Path(out).read_text()), logs


def test_sharded_runner_takes_both_steps_together(tmp_path):
    """Rank 1's attempt switches f16 -> default, both ranks repeat; that attempt overflows on rank 0, both end on bx3 (the worker
    asserts the three attempts f16, h2, bx3 on every rank and tracker): the merged predictions are those of a bx3 run."""
    want, _ = _launch("bx3", 1, tmp_path / "bx3.json")
    got, logs = _launch("ladder", 2, tmp_path / "ladder.json")
    for name in ("players_tracker", "ball_tracker"):
        assert len(got[name]) == len(want[name]) == 45
        assert got[name] == want[name], name
    assert any(p for fr in want["players_tracker"] for p in fr) and sum(b["visibility"] for b in want["ball_tracker"]) > 5
    for log in logs:
        assert log.count("every rank repeats its shard on the default fp32-equivalent path") == 2, log[-2000:]
        assert log.count("every rank repeats its shard on the bf16x3 path") == 2, log[-2000:]
