"""``TrackingRunner(render=...)`` on the GPU: the clip comes back as a ``.y4m`` file with every tracker's results drawn on it, each
frame equal to ``render.render_host`` of that frame under the marks of the runner's own stored results; without ``render`` nothing
is written and ``timings`` is what it was.

The synthetic checkpoints detect 170-200 players and 300 persons' skeletons per frame (their confidences sit near 1 whatever the
threshold), so a frame carries 5 600-6 000 marks — 24 passes of the kernel's LDS list — and ``render_host`` of the 13 frames is what
the first test spends its time on: about 10 s of its 12 s on the host (measured; the render step itself takes 0.5 s)."""
import numpy as np
import pytest

from padel_analytics_amd import checkpoint, detections as D, engine as E, render as R, video, yolo_arch
from padel_analytics_amd.trackers import BallDetectTracker, PlayerKeypointsTracker, PlayerTracker, TrackingRunner
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)

pytestmark = pytest.mark.gpu

SRC = "synthetic://?n=13&h=360&w=640&fps=30&seed=15"


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_runner")
    checkpoint.save_checkpoint(d / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None, "n", {0: "person"})
    checkpoint.save_checkpoint(d / "pose.pt", yolo_arch.synth_state_dict("n", 1, (13, 3), seed=4, cls_bias=0.5), "pose", 1, (13, 3), "n", {0: "person"})
    checkpoint.save_checkpoint(d / "ball.pt", yolo_arch.synth_state_dict("n", 1, None, seed=5, cls_bias=0.5), "detect", 1, None, "n", {0: "ball"})
    return d


def make_runner(d, out, **kw):
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    trackers = [PlayerTracker(str(d / "players.pt"), zone, batch_size=5), PlayerKeypointsTracker(str(d / "pose.pt"), 640, batch_size=5),
                BallDetectTracker(str(d / "ball.pt"), batch_size=5)]
    return TrackingRunner(trackers, SRC, out / "out.mp4", **kw), trackers


def test_runner_writes_the_annotated_clip(gpu_engine, checkpoints, tmp_path, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 5)                    # 13 frames: two whole batches and a short last one
    runner, trackers = make_runner(checkpoints, tmp_path, render=tmp_path / "out.y4m")
    runner.run()
    assert set(runner.timings) == {"players_tracker", "players_keypoints_tracker", "ball_tracker", "__render__"}
    assert runner.timings["__render__"]["frames"] == 13
    clip = video.YuvClip.from_y4m(tmp_path / "out.y4m", on_device=False)
    assert (clip.n, clip.w, clip.h, clip.fps) == (13, 640, 360, 30)
    frames = np.stack(list(video.get_video_frames_generator(SRC)))
    geom = video.yuv_desc(640, 360, "i420")
    enc = video.YUV_ENC_COEFFS["bt601_limited"]
    kinds = set()
    for i in range(13):
        per_frame = [runner.frame_marks(i)]
        # the marks are the stored results': the frame text, then each tracker's results[i].marks(**draw_kwargs()) in tracker order
        want_marks = R.text(f"FRAME: {i + 1}", 20, 30, 3, (0, 255, 255))
        for t in trackers:
            want_marks += t.results[i].marks(**t.draw_kwargs())
        assert per_frame[0] == want_marks
        kinds |= {m[0] for m in want_marks}
        want = R.render_host(frames[i:i + 1], *R.pack(per_frame), out=E.RENDER_YUV420, geom=geom, enc=enc)
        assert np.array_equal(clip._host_bytes(i, 1), want), i
    assert kinds == {E.MARK_DISC, E.MARK_SEGMENT, E.MARK_FILL, E.MARK_BOX, E.MARK_GLYPH}      # players, skeletons and the ball were all drawn
    assert not np.array_equal(clip._host_bytes(0, 1), video.bgr_to_yuv420_host(frames[:1], geom, enc))
    for t in trackers:
        t.model.close()


def test_a_sink_object_and_device_frames(gpu_engine, checkpoints, tmp_path):
    """The same through a caller's ``FrameSink`` (NV12 with a padded pitch) over a clip resident in HBM."""
    frames = np.stack(list(video.get_video_frames_generator(SRC)))[:6]
    dclip = video.DeviceClip(gpu_engine, frames)
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    players = PlayerTracker(str(checkpoints / "players.pt"), zone, batch_size=6)
    with video.Y4mSink(tmp_path / "nv12.y4m", 640, 360, fps=30, layout="nv12", pitch=704) as sink:
        runner = TrackingRunner([players], dclip, tmp_path / "out.mp4", render=sink)
        runner.run()
        assert sink.frames_written == 6
    clip = video.YuvClip.from_y4m(tmp_path / "nv12.y4m", on_device=False)
    geom = video.yuv_desc(640, 360, "i420")
    for i in range(6):
        want = R.render_host(frames[i:i + 1], *R.pack([runner.frame_marks(i)]), out=E.RENDER_YUV420, geom=geom, enc=sink.enc)
        assert np.array_equal(clip._host_bytes(i, 1), want), i
    players.model.close()
    dclip.free()


def test_without_render_nothing_is_written(gpu_engine, checkpoints, tmp_path, capsys):
    runner, trackers = make_runner(checkpoints, tmp_path)
    runner.run()
    assert set(runner.timings) == {"players_tracker", "players_keypoints_tracker", "ball_tracker"}
    assert "drawing / data collection is outside the hot path of this build (skipped)" in capsys.readouterr().out
    assert list(tmp_path.iterdir()) == []
    for t in trackers:
        t.model.close()
