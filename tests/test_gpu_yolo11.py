"""YOLO11 detect / pose checkpoints end to end on the HIP engine, through ``YOLO(model_path)`` — the call that fails without the
YOLO11 builder — against the torch restatement tests/yolo11_ref.py, held to the criteria of tests/test_gpu_yolo_parity.py:
``_check`` (identical class ids and detection sets; engine vs fp64 <= max(1e-3 px, 4 x fp32 oracle vs fp64); that file's RMS and
score bounds) and ``_check_heads`` (raw head maps against fp64) are that file's own functions, called unchanged: their oracle cache
is primed with the YOLO11 oracle's evaluations of the same checkpoint and clip, so they compare against those."""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import yolov8_ref as ref
from padel_analytics_amd import checkpoint, detections as D, engine as E, graph as G, video
from padel_analytics_amd.trackers import PlayerKeypointsTracker, PlayerTracker, Players, PlayersKeypoints, TrackingRunner
from padel_analytics_amd.yolo import YOLO
from tests import synth, test_gpu_yolo_parity as P, yolo11_synth
from tests.yolo11_ref import Yolo11Ref
from tests.yolo11_report import record

pytestmark = pytest.mark.gpu


def _prime(sd, nc, kpt, srcs, conf, iou, S):
    """Both arithmetics of the YOLO11 oracle on (checkpoint, clip), stored where ``P._oracle_heads`` / ``P._oracle_predict`` look."""
    for dt in (torch.float32, torch.float64):
        hk = P._content_key(sd, srcs, nc, kpt, S, str(dt), "heads")
        if hk not in P._ORACLE_CACHE:
            o = Yolo11Ref(sd, nc, kpt, dtype=dt)
            x = ref.preprocess(list(srcs), S)
            with torch.no_grad():
                P._ORACLE_CACHE[hk] = o.head_raw(o.features(x.to(dt)))
        pk = P._content_key(sd, srcs, nc, kpt, conf, iou, S, str(dt), "predict")
        if pk not in P._ORACLE_CACHE:
            P._ORACLE_CACHE[pk] = ref.predict(Yolo11Ref(sd, nc, kpt, dtype=dt), srcs, conf, iou, S, classes=[0], heads=P._ORACLE_CACHE[hk])


def _stretch(frames, S):
    from PIL import Image
    pil = [np.asarray(Image.fromarray(f[..., ::-1].copy()).resize((S, S))) for f in frames]
    return [p[..., ::-1] for p in pil]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scale, nc, kpt, frames, oracle sources, imgsz, conf, calibrated state_dict) of one end-to-end case."""
    if name == "n-detect":
        scale, nc, kpt, S, conf, seed = "n", 80, None, 640, 0.5, 5
    elif name == "n-pose":
        scale, nc, kpt, S, conf, seed = "n", 1, (13, 3), 640, 0.25, 11
    else:                       # 720p letterboxed to 192 x 320: 60 tokens; m: c3k True everywhere, 4 heads; l: two PSABlocks
        scale, nc, kpt, S, conf, seed = name[0], 80, None, 320, 0.5, 7
    frames = synth.synthetic_frames(2, 720, 1280, seed=3 if kpt is None else 7)
    srcs = _stretch(frames, S) if kpt else [f[..., ::-1] for f in frames]
    sd = yolo11_synth.calibrated_state_dict(scale, nc, kpt, ref.preprocess(srcs, S), conf, seed)
    return scale, nc, kpt, frames, srcs, S, conf, sd


def _yolo(tmp_path, name, eng, **kw):
    scale, nc, kpt, frames, srcs, S, conf, sd = _case(name)
    path = tmp_path / f"yolo11{scale}.pt"
    checkpoint.save_checkpoint(path, sd, "pose" if kpt else "detect", nc, kpt, scale, {0: "person"})
    y = YOLO(path, engine=eng, **kw)
    assert y.family == "yolo11"
    y.set_max_batch(len(frames))
    return y


def _infer(y, name, frames=None):
    scale, nc, kpt, all_frames, srcs, S, conf, sd = _case(name)
    frames = all_frames if frames is None else frames
    boxes, kpts, counts, *_ = y.infer_frames(frames, conf, 0.7, S, classes=[0], channel_reverse=kpt is not None, pil_stretch=kpt is not None)
    assert not y.fell_back
    return boxes, kpts, counts


def _parity(tag, y, name, got):
    scale, nc, kpt, frames, srcs, S, conf, sd = _case(name)
    _prime(sd, nc, kpt, srcs, conf, 0.7, S)
    heads = P._check_heads(tag, y._model, sd, nc, kpt, srcs, S, len(frames))
    P._check(tag, sd, nc, kpt, srcs, got, conf, 0.7, S)
    record(tag, dict(P.REPORT[tag], head_maps=heads))


@pytest.mark.parametrize("name", ["n-detect", "n-pose", "m-detect-320", "l-detect-320"])
def test_yolo11_parity(gpu_engine, tmp_path, name):
    y = _yolo(tmp_path, name, gpu_engine)
    try:
        assert sum(o["kind"] == G.OP_PSA_ATTN for o in y.graph.ops) == (2 if name[0] == "l" else 1)
        got = _infer(y, name)
        _parity(f"yolo11 {name} [{y.fp32_mode}]", y, name, got)
    finally:
        y.close()


def test_yolo11_bx3_mode(gpu_engine, tmp_path):
    y = _yolo(tmp_path, "n-detect", gpu_engine, fp32_mode="bx3")
    try:
        assert y.graph.dtype == G.DTYPE_F32
        _parity("yolo11 n-detect [bx3]", y, "n-detect", _infer(y, "n-detect"))
    finally:
        y.close()


@pytest.mark.parametrize("name", ["n-detect", "n-pose"])
def test_yolo11_batch_invariance(gpu_engine, tmp_path, name):
    """The second frame alone and as the second of a batch of two: the same head maps and results, bit for bit."""
    frames = _case(name)[3]
    y = _yolo(tmp_path, name, gpu_engine)
    try:
        b2, k2, c2 = (None if a is None else a.copy() for a in _infer(y, name))
        h2 = [y._model.read_head(l, 2)[1].copy() for l in range(3)]
        b1, k1, c1 = _infer(y, name, frames[1:2])
        h1 = [y._model.read_head(l, 1)[0] for l in range(3)]
    finally:
        y.close()
    for l in range(3):
        assert np.array_equal(h1[l].view(np.uint32), h2[l].view(np.uint32)), f"head level {l}"
    assert c1[0] == c2[1] and c1[0] > 0
    assert np.array_equal(b1[0].view(np.uint32), b2[1].view(np.uint32))
    assert k1 is None or np.array_equal(k1[0].view(np.uint32), k2[1].view(np.uint32))


def test_trackers_run_yolo11_checkpoints(gpu_engine, tmp_path):
    """PlayerTracker and PlayerKeypointsTracker on YOLO11 checkpoints through TrackingRunner, JSON caches written and read back."""
    src = "synthetic://?n=12&h=360&w=640&fps=30&seed=5"
    frames = list(video.get_video_frames_generator(src))
    srcs = [f[..., ::-1] for f in frames[:4]]
    sd_p = yolo11_synth.calibrated_state_dict("n", 80, None, ref.preprocess(srcs, 640), 0.5, seed=3)
    checkpoint.save_checkpoint(tmp_path / "players.pt", sd_p, "detect", 80, None, "n", {0: "person"})
    sd_k = yolo11_synth.calibrated_state_dict("n", 1, (13, 3), ref.preprocess(_stretch(frames[:4], 640), 640), 0.25, seed=4)
    checkpoint.save_checkpoint(tmp_path / "pose.pt", sd_k, "pose", 1, (13, 3), "n", {0: "person"})
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    players = PlayerTracker(str(tmp_path / "players.pt"), zone, batch_size=8, save_path=tmp_path / "players.json")
    pose = PlayerKeypointsTracker(str(tmp_path / "pose.pt"), 640, batch_size=8, load_path=None, save_path=tmp_path / "pose.json")
    assert players.model.family == pose.model.family == "yolo11"
    TrackingRunner([players, pose], src, tmp_path / "out.mp4").run()
    assert len(players) == len(pose) == 12
    assert sum(len(p) for p in players.results.predictions) > 0 and sum(len(p) for p in pose.results.predictions) > 0
    for fname, cls in (("players.json", Players), ("pose.json", PlayersKeypoints)):
        data = json.loads((tmp_path / fname).read_text())
        assert len(data) == 12 and len(cls.from_json(data[0])) == len(data[0])
    players2 = PlayerTracker(str(tmp_path / "players.pt"), zone, batch_size=8, load_path=tmp_path / "players.json")
    assert len(players2) == 12
    # the detections of the first batch agree with the oracle
    res = players.model.predict_frames(np.stack(frames[:8]), 0.5, 0.7, 640, classes=[0], channel_reverse=False)
    r32 = ref.predict(Yolo11Ref(sd_p, 80, None), [f[..., ::-1] for f in frames[:8]], 0.5, 0.7, 640, classes=[0])
    boxes = np.zeros((8, 300, 6), np.float32)
    counts = np.zeros(8, np.int32)
    for i, r in enumerate(res):
        counts[i] = len(r.boxes)
        boxes[i, :counts[i]] = r.boxes.data
    from tests import parity
    rep = parity.compare_batch(r32, boxes, None, counts, 0.5, 0.7)
    assert rep["worst_px"] < 0.1 and rep["n"] > 0
