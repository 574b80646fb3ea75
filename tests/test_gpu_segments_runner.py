"""``TrackingRunner(segments=...)`` on the GPU, 360 x 640, synthetic calibrated checkpoints as in tests/test_gpu_runner.py.

Clip A is 24 frames.  Clip B is A with a 5-frame cutaway after its first 5 frames and a 3-frame one appended (32 frames); the
matching segments keep exactly A's frames.  The player tracker over B then serialises to what it gives over A (the batches differ:
5 | 8, 8, 3 against 8, 8, 8 — batch invariance and the carried ByteTrack state make them equal), the ball tracker to the
concatenation of its runs over each segment as a clip of its own, the rendered clip holds the kept frames under their own marks with
the source frame number in the label, and ``segments="court"`` finds constructed runs."""
import json

import numpy as np
import pytest

import torch

from oracle import ball_ref as br, synth_weights, tracknet_ref as tr, yolov8_ref as ref
from padel_analytics_amd import checkpoint, detections as D, engine as E, render as R, video
from padel_analytics_amd.trackers import BallTracker, PlayerTracker, TrackingRunner
from tests import synth

pytestmark = pytest.mark.gpu

H, W = 360, 640
SEGMENTS = [(0, 5), (10, 29)]
KEPT = [i for lo, hi in SEGMENTS for i in range(lo, hi)]


@pytest.fixture(scope="module")
def clips():
    a = synth.synthetic_frames(24, H, W, seed=5)
    cut = synth.synthetic_frames(8, H, W, seed=77)
    b = np.concatenate([a[:5], cut[:5], a[5:], cut[5:]])
    assert len(b) == 32 and np.array_equal(b[KEPT], a)
    return a, b


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory, clips):
    d = tmp_path_factory.mktemp("segments_runner")
    srcs = [f[..., ::-1] for f in clips[0][:4]]
    sd = synth_weights.calibrated_state_dict("n", 80, None, ref.preprocess(srcs, 640), 0.5, seed=3)
    checkpoint.save_checkpoint(d / "players.pt", sd, "detect", 80, None, "n", {0: "person"})
    # TrackNet weights whose ENSEMBLED heat map crosses 0.5 on about 0.5 % of the pixels of the second segment's first 12 frames (the
    # oracle with a zero bias, then one shift of the predictor's bias): the ball results below are not all "nothing found"
    a = clips[0]
    sd_t = tr.synth_tracknet_state_dict(9)
    sd_t["predictor.bias"] = np.zeros(8, np.float32)
    heat = torch.from_numpy(np.asarray(br.track(list(a[5:17]), tr.TrackNetRef(sd_t).forward, median_chw=br.median_background(a[:12]), batch=4)[3]))
    shift = -torch.quantile(torch.log(heat / (1 - heat)).flatten()[::7], 0.995)
    sd_t["predictor.bias"] = shift.repeat(8).numpy().astype(np.float32)
    checkpoint.save_checkpoint(d / "tracknet.pt", sd_t, "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    return d


def players_tracker(d):
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(W, H))
    return PlayerTracker(str(d / "players.pt"), zone, batch_size=8)


@pytest.fixture(scope="module")
def segmented_run(gpu_engine, clips, checkpoints, tmp_path_factory):
    """Players and ball over B with the segments, rendered to a .y4m file (render batches of 8: none may span the cut either)."""
    out = tmp_path_factory.mktemp("segments_out")
    players = players_tracker(checkpoints)
    ball = BallTracker(str(checkpoints / "tracknet.pt"), None, batch_size=8, median_max_sample_num=12)
    saved = TrackingRunner.RENDER_BATCH
    TrackingRunner.RENDER_BATCH = 8
    try:
        runner = TrackingRunner([players, ball], video.ArrayClip(clips[1]), out / "out.mp4", segments=SEGMENTS, render=out / "out.y4m")
        runner.run()
    finally:
        TrackingRunner.RENDER_BATCH = saved
    yield runner, players, ball, out / "out.y4m"
    players.model.close()


def test_players_over_b_with_segments_equal_players_over_a(gpu_engine, clips, checkpoints, segmented_run, tmp_path):
    runner, players, _, _ = segmented_run
    assert runner.source_index.tolist() == KEPT and runner.n_available == runner.total_frames == 24
    plain = players_tracker(checkpoints)
    TrackingRunner([plain], video.ArrayClip(clips[0]), tmp_path / "out.mp4").run()
    want = [o.serialize() for o in plain.results]
    got = [o.serialize() for o in players.results]
    plain.model.close()
    assert len(got) == len(want) == 24
    assert json.dumps(got) == json.dumps(want)
    assert sum(len(f) for f in want) > 0
    ids = {p.id for pl in players.results.predictions[8:] for p in pl}
    assert ids and None not in ids                     # tracks confirmed before the cut keep their ids behind it
    assert runner.timings["players_tracker"]["frames"] == 24


def test_ball_background_is_the_median_of_the_first_kept_frames(segmented_run, clips):
    _, _, ball, _ = segmented_run
    assert len(ball.results) == 24 and [b.frame for b in ball.results] == list(range(24))
    # median_max_sample_num = 12 kept frames: 5 of the first segment and 7 of the second
    assert np.array_equal(ball.median, np.median(clips[0][:12, ..., ::-1], 0).astype(np.uint8))


def test_ball_over_b_equals_its_runs_over_each_segment(gpu_engine, clips, checkpoints, tmp_path):
    a, b = clips
    median = np.median(a[:12, ..., ::-1], 0).astype(np.uint8)
    make = lambda: BallTracker(str(checkpoints / "tracknet.pt"), None, batch_size=8, median=median)
    whole = make()
    dclip = video.DeviceClip(gpu_engine, b)
    try:
        TrackingRunner([whole], dclip, tmp_path / "out.mp4", segments=SEGMENTS).run()
    finally:
        dclip.free()
    want, kept = [], 0
    for lo, hi in SEGMENTS:
        part = make()
        TrackingRunner([part], video.ArrayClip(b[lo:hi]), tmp_path / "out.mp4").run()
        assert len(part.results) == hi - lo
        for o in part.results:
            s = o.serialize()
            s["frame"] += kept
            want.append(s)
        kept += hi - lo
    got = [o.serialize() for o in whole.results]
    assert json.dumps(got) == json.dumps(want)
    assert [s["frame"] for s in got] == list(range(24))
    assert any(s["visibility"] for s in got[5:])       # the 19-frame segment has windows (the 5-frame one is too short for any)


def test_rendered_clip_holds_the_kept_frames_under_their_marks(segmented_run, clips):
    runner, players, ball, path = segmented_run
    assert runner.timings["__render__"]["frames"] == 24
    clip = video.YuvClip.from_y4m(path, on_device=False)
    assert (clip.n, clip.w, clip.h) == (24, W, H)
    geom, enc = video.yuv_desc(W, H, "i420"), video.YUV_ENC_COEFFS["bt601_limited"]
    for i in range(24):
        src = int(runner.source_index[i])
        marks = runner.frame_marks(i)
        label = R.text(f"FRAME: {src + 1}", 20, 30, 3, (0, 255, 255))          # the source frame number, counted from 1
        want_marks = label + players.results[i].marks(**players.draw_kwargs()) + ball.results[i].marks(**ball.draw_kwargs())
        assert marks == want_marks, i
        want = R.render_host(clips[1][src:src + 1], *R.pack([marks]), out=E.RENDER_YUV420, geom=geom, enc=enc)
        assert np.array_equal(clip._host_bytes(i, 1), want), i
    assert KEPT[5] + 1 == 11 and runner.frame_marks(5)[:len(R.text("FRAME: 11", 20, 30, 3, (0, 255, 255)))] == R.text("FRAME: 11", 20, 30, 3, (0, 255, 255))


def court_clip():
    """40 frames: a static texture with every channel in [0, 100] and two 40 x 80 rectangles that move from frame to frame (6400 of
    230400 pixels: 2.78 %); in [10, 16) and [30, 33) cutaways, 255 - the frame without its rectangles: every pixel's luma differs by
    at least 55 there."""
    rng = np.random.default_rng(31)
    texture = rng.integers(0, 101, (H, W, 3), dtype=np.uint8)
    frames = np.repeat(texture[None], 40, 0)
    for i in range(40):
        for k, (x, y) in enumerate(((20 + 14 * i, 30 + 5 * i), (540 - 13 * i, 300 - 6 * i))):
            frames[i, y:y + 40, x:x + 80] = (200, 180, 220) if k else (230, 210, 190)
    for lo, hi in ((10, 16), (30, 33)):
        frames[lo:hi] = 255 - texture
    return frames


def test_court_finds_the_constructed_runs(gpu_engine, checkpoints, tmp_path):
    frames = court_clip()
    players = players_tracker(checkpoints)
    runner = TrackingRunner([players], video.ArrayClip(frames), tmp_path / "out.mp4", segments="court",
                            segment_options=dict(min_keep=4, max_gap=1))
    assert runner.segments is None and runner.n_available == 40          # decided by run(), before the first tracker
    runner.run()
    players.model.close()
    assert runner.segments == [(0, 10), (16, 30), (33, 40)]
    assert runner.n_available == runner.total_frames == len(players.results) == 31
    assert runner.timings["__segments__"]["frames"] == 40 and runner.timings["__segments__"]["kept"] == 31
    # what decided it: at most 2.8 % of the pixels changed on a court frame, all of them on a cutaway
    from padel_analytics_amd import activity as A
    act = A.scan(video.ArrayClip(frames), engine=gpu_engine)
    court = np.ones(40, bool)
    court[10:16] = court[30:33] = False
    assert act.npix == H * W and (act.changed[court] <= 0.028 * act.npix).all() and (act.changed[~court] == act.npix).all()
