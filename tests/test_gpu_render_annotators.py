"""The players' four annotators and ``ball_trail`` through ``TrackingRunner(render=...)`` on the GPU: the first 24 frames of the
scripted 160 x 96 clip of tests/identity_script.py, ``Players`` and ``Ball`` from prediction caches the test writes (no detector
runs).  Each run writes a ``.y4m``; every frame of every file must equal ``render.render_host`` of the source frame under the runner's
own ``frame_marks``, and the default run's file the one written without the new arguments."""
import json

import numpy as np
import pytest

from padel_analytics_amd import engine as E, render as R, video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.ball_tracker import Ball
from tests import identity_script as S

pytestmark = pytest.mark.gpu

N, H, W = 24, S.H, S.W
ANNOTATORS = ("rectangle_bounding_box", "round_bounding_box", "corner_bounding_box", "ellipse")


class AnnotatedPlayers(S.PlayersStub):
    def __init__(self, annotator=None, **kw):
        self.annotator = annotator
        super().__init__(**kw)

    def draw_kwargs(self):
        kw = {"video_info": None, "show_confidence": True}
        return kw if self.annotator is None else dict(kw, annotator=self.annotator)


class BallStub(S.PlayersStub):
    def object(self): return Ball
    def draw_kwargs(self): return {}
    def __str__(self): return "ball_tracker"


def balls_script() -> list:
    """The ball crosses the frame and is not seen in frames 2, 9 and 10."""
    return [Ball(i, (8.0 + 6 * i, 80.0 - 2.5 * i), 0 if i in (2, 9, 10) else 1) for i in range(N)]


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    d = tmp_path_factory.mktemp("annotators")
    with video.Y4mSink(d / "clip.y4m", W, H, fps=30) as sink:
        sink.write_host(video.bgr_to_yuv420_host(S.clip(N), sink.desc, sink.enc), N)
    frames = np.stack([np.asarray(f) for f in video.get_video_frames_generator(str(d / "clip.y4m"))])
    assert frames.shape == (N, H, W, 3)
    S.write_cache(d / "players.json", range(N))
    with open(d / "balls.json", "w") as f:
        json.dump([b.serialize() for b in balls_script()], f)
    return dict(dir=d, path=str(d / "clip.y4m"), frames=frames)


def run(script, out, annotator=None, **kw):
    players = AnnotatedPlayers(annotator, load_path=script["dir"] / "players.json")
    balls = BallStub(load_path=script["dir"] / "balls.json")
    runner = TrackingRunner([players, balls], script["path"], script["dir"] / "out.mp4", render=out, **kw)
    runner.run()
    assert players.fed == 0 and balls.fed == 0               # the caches were used: nothing was predicted
    assert runner.timings["__render__"]["frames"] == N
    return runner


def file_equals_the_twin(script, runner, out):
    clip = video.YuvClip.from_y4m(out, on_device=False)
    assert (clip.n, clip.w, clip.h) == (N, W, H)
    geom, enc = video.yuv_desc(W, H, "i420"), video.YUV_ENC_COEFFS["bt601_limited"]
    for i in range(N):
        want = R.render_host(script["frames"][i:i + 1], *R.pack([runner.frame_marks(i)]), out=E.RENDER_YUV420, geom=geom, enc=enc)
        assert np.array_equal(clip._host_bytes(i, 1), want), i


@pytest.mark.parametrize("annotator", ANNOTATORS)
def test_every_annotator_is_drawn_as_the_twin_draws_it(gpu_engine, script, tmp_path, annotator):
    runner = run(script, tmp_path / "out.y4m", annotator)
    kinds = [m[0] for m in runner.frame_marks(5)]
    assert (E.MARK_BOX in kinds) == (annotator == "rectangle_bounding_box")
    assert (E.MARK_ARC in kinds) == (annotator in ("round_bounding_box", "ellipse"))
    file_equals_the_twin(script, runner, tmp_path / "out.y4m")
    if annotator == "rectangle_bounding_box":                # the default, named: the file written without the new arguments
        plain = run(script, tmp_path / "plain.y4m")
        assert plain.ball_trail == 0 and sorted(plain.timings) == sorted(runner.timings)
        assert (tmp_path / "plain.y4m").read_bytes() == (tmp_path / "out.y4m").read_bytes()
        assert [plain.frame_marks(i) for i in range(N)] == [runner.frame_marks(i) for i in range(N)]


def test_the_ball_trail_is_drawn_as_the_twin_draws_it(gpu_engine, script, tmp_path):
    runner = run(script, tmp_path / "trail.y4m", ball_trail=3)
    plain = run(script, tmp_path / "plain.y4m", ball_trail=0)
    for i in range(N):
        seen = [b for b in balls_script()[max(0, i - 2):i + 1][::-1] if b.visibility]
        trail = [m for b in seen for m in (R.disc(*b.asint(), 3, (0, 255, 255)), R.disc(*b.asint(), 2, (255, 255, 255)))]
        assert runner.frame_marks(i) == plain.frame_marks(i) + trail, i
    assert len(runner.frame_marks(10)) == len(plain.frame_marks(10)) + 2      # frames 9 and 10 unseen: only frame 8 is left of the trail
    file_equals_the_twin(script, runner, tmp_path / "trail.y4m")
    file_equals_the_twin(script, plain, tmp_path / "plain.y4m")
    assert (tmp_path / "trail.y4m").read_bytes() != (tmp_path / "plain.y4m").read_bytes()
