"""``TrackingRunner(topdown=...)`` on the GPU, end to end over a 160 x 96 synthetic clip with fixed court keypoints.  No detector runs:
the ``Players`` and the ``Ball`` come from prediction caches the test writes (tests/identity_script.py's boxes, a ball that crosses the
court).  The top-down ``.y4m`` equals ``render_host(warp_host(frame, ...), canvas marks)`` of every frame, the ``.avi`` is
``mjpeg.encode_host`` of the same, ``render=`` beside it writes the file it writes alone, and a run without ``topdown=`` writes nothing
new."""
import json

import numpy as np
import pytest

from padel_analytics_amd import engine as E, mjpeg, render as R, topdown as T, video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.ball_tracker import Ball
from padel_analytics_amd.trackers.tracker import NoPredictFrames, Tracker
from tests import identity_script as S, synth  # noqa: F401  (synth registers the synthetic:// frame source)
from tests.test_mjpeg_host import read_avi

pytestmark = pytest.mark.gpu

N, H, W = 11, S.H, S.W
SRC = f"synthetic://?n={N}&h={H}&w={W}&fps=30&seed=8"
OPTIONS = dict(px_per_m=8, margin_m=1, fill=(30, 60, 90))      # a 96 x 176 canvas: 16-byte stores
CW, CH = 96, 176


class BallStub(Tracker):
    """A tracker of ``Ball`` that only loads its prediction cache; asked to predict, it fails the test."""
    DEVICE = "cpu"
    streams = False
    batch_size = 8

    def video_info_post_init(self, video_info): return self
    def object(self): return Ball
    def draw_kwargs(self): return {}
    def restart(self): self.results.restart()
    def __str__(self): return "ball_tracker"
    def predict_sample(self, sample, **kwargs): raise AssertionError("the ball's cache was not used")
    def predict_frames(self, frame_generator, **kwargs): raise NoPredictFrames()


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    d = tmp_path_factory.mktemp("topdown")
    S.write_cache(d / "players.json", range(N))
    with open(d / "ball.json", "w") as f:
        json.dump([Ball(i, (30.0 + 9.5 * i, 40.0 + 4.25 * i), 1).serialize() for i in range(N)], f)
    return dict(dir=d, frames=np.stack(list(video.get_video_frames_generator(SRC))))


def run(script, out, **kw):
    players = S.PlayersStub(load_path=script["dir"] / "players.json")
    trackers = [players, BallStub(load_path=script["dir"] / "ball.json"), S.keypoints_tracker(N)]
    runner = TrackingRunner(trackers, SRC, out / "out.mp4", **kw)
    runner.run()
    assert players.fed == 0                                  # the caches were used: nothing was predicted
    return runner


def canvases(runner, script, enc):
    """``render_host(warp_host(frame), canvas marks)`` of every frame as tightly packed I420, from the runner's own projections."""
    view = runner.topdown_view
    assert view.size == (CW, CH)
    geom = video.yuv_desc(CW, CH, "i420")
    out = []
    for i in range(N):
        m, valid = view.matrices(runner._projected[i:i + 1])
        assert valid[0] == 1
        canvas = T.warp_host(script["frames"][i:i + 1], m, valid, CH, CW, view.fill)
        marks = runner.topdown_marks(i)
        assert len(marks) == 8 + len(runner.trackers["players_tracker"].results[i]) * 2 + 1      # lines, disc + one digit per player, the ball
        out.append(R.render_host(canvas, *R.pack([marks]), out=E.RENDER_YUV420, geom=geom, enc=enc))
    return out, geom


def test_the_topdown_y4m_is_the_twins(gpu_engine, script, tmp_path, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 4)                    # 11 frames: two whole batches and a short one
    runner = run(script, tmp_path, topdown=tmp_path / "top.y4m", topdown_options=OPTIONS)
    assert gpu_engine.warp_last_path() == E.WARP_PATH_VECTOR
    assert set(runner.timings) == {"__topdown__"} and set(runner.timings["__topdown__"]) == {"seconds", "frames", "bytes"}
    assert runner.timings["__topdown__"]["frames"] == N and runner.timings["__topdown__"]["bytes"] == (tmp_path / "top.y4m").stat().st_size
    assert sorted(p.name for p in tmp_path.iterdir()) == ["top.y4m"]
    clip = video.YuvClip.from_y4m(tmp_path / "top.y4m", on_device=False)
    assert (clip.n, clip.w, clip.h, clip.fps) == (N, CW, CH, 30)
    want, _ = canvases(runner, script, video.YUV_ENC_COEFFS["bt601_limited"])
    for i in range(N):
        assert np.array_equal(clip._host_bytes(i, 1), want[i]), i
    # the footage is in the picture: the canvas of frame 0 is not its marks on a blank canvas
    blank = np.empty((1, CH, CW, 3), np.uint8)
    blank[:] = OPTIONS["fill"]
    bare = R.render_host(blank, *R.pack([runner.topdown_marks(0)]), out=E.RENDER_YUV420, geom=video.yuv_desc(CW, CH, "i420"),
                         enc=video.YUV_ENC_COEFFS["bt601_limited"])
    assert (want[0] != bare).mean() > 0.2


def test_the_topdown_avi_and_render_beside_it(gpu_engine, script, tmp_path):
    (tmp_path / "both").mkdir()
    (tmp_path / "plain").mkdir()
    runner = run(script, tmp_path / "both", topdown=tmp_path / "both" / "top.avi", topdown_options=OPTIONS, render=tmp_path / "both" / "r.avi",
                 render_quality=85, collect_data=True)
    assert {"__topdown__", "__render__", "__collect__"} <= set(runner.timings)
    assert runner.timings["__topdown__"]["bytes"] == (tmp_path / "both" / "top.avi").stat().st_size
    got = read_avi(tmp_path / "both" / "top.avi", CW, CH, 30)
    assert len(got) == N
    want, geom = canvases(runner, script, video.YUV_ENC_COEFFS["bt601_full"])
    for i in range(N):
        data, _ = mjpeg.encode_host(want[i], 1, CH, CW, geom, 85)
        assert got[i] == data.tobytes(), i
    # render= beside it writes, byte for byte, the file it writes alone — and a run without topdown= writes nothing new
    plain = run(script, tmp_path / "plain", render=tmp_path / "plain" / "r.avi", render_quality=85, collect_data=True)
    assert (tmp_path / "both" / "r.avi").read_bytes() == (tmp_path / "plain" / "r.avi").read_bytes()
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["r.avi"] and "__topdown__" not in plain.timings
    assert sorted(p.name for p in (tmp_path / "both").iterdir()) == ["r.avi", "top.avi"]
