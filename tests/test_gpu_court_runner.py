"""``TrackingRunner(collect_data=True, render=...)`` on the GPU: the clip comes back with the court inset drawn on it — the blending
panel, the court, the projected players and ball — each frame equal to ``render.render_host`` under ``runner.frame_marks(i)``, and
``data_analytics`` holds the players' positions a per-frame loop written here computes.  640 x 360, 7 synthetic frames, 3 frames per
render batch (two whole batches and a short one, the homography carrying across them).  The players and ball detectors are the
synthetic checkpoints of test_gpu_render_runner.py (without the pose tracker, whose marks are what makes that file slow); they run
once for the module, the runners of the cases find their results stored."""
import numpy as np
import pytest

from padel_analytics_amd import checkpoint, detections as D, engine as E, render as R, video, yolo_arch
from padel_analytics_amd.trackers import BallDetectTracker, KeypointsTracker, PlayerTracker, TrackingRunner
from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)
from tests.court_script import Stored, court_for, frame_keypoints, plain_loop, true_homography

pytestmark = pytest.mark.gpu

N = 7
SRC = f"synthetic://?n={N}&h=360&w=640&fps=30&seed=15"
GEOM = video.yuv_desc(640, 360, "i420")
ENC = video.YUV_ENC_COEFFS["bt601_limited"]


def court_keypoints_in_the_frame(count, seed, n):
    """``n`` detections of ``count`` court keypoints as a camera over a 640 x 360 frame sees them (the host test's 1280 x 720 camera
    at half size), differing from frame to frame."""
    court = court_for(640, 360)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        S = np.diag([2.0, 2.0, 1.0])                                     # 640 x 360 frame coordinates -> the 1280 x 720 camera's
        H = true_homography(court, rng, jitter=3.0) @ S
        src, _ = frame_keypoints(court, count, H, rng, noise=0.5)
        out.append(Keypoints([Keypoint(j, (float(x), float(y))) for j, (x, y) in enumerate(src)]))
    return out


@pytest.fixture(scope="module")
def tracked(gpu_engine, tmp_path_factory):
    """The players and ball trackers with their results of the 7 frames stored."""
    d = tmp_path_factory.mktemp("court_runner")
    checkpoint.save_checkpoint(d / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None, "n", {0: "person"})
    checkpoint.save_checkpoint(d / "ball.pt", yolo_arch.synth_state_dict("n", 1, None, seed=5, cls_bias=0.5), "detect", 1, None, "n", {0: "ball"})
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    trackers = [PlayerTracker(str(d / "players.pt"), zone, batch_size=4), BallDetectTracker(str(d / "ball.pt"), batch_size=4)]
    TrackingRunner(trackers, SRC, d / "out.mp4").run()
    assert [len(t) for t in trackers] == [N, N]
    yield trackers
    for t in trackers:
        t.model.close()


@pytest.fixture(scope="module")
def clip_frames():
    return np.stack(list(video.get_video_frames_generator(SRC)))


def plain_marks(trackers, i):
    """What ``render=`` alone draws: the frame text, then every tracker's marks."""
    marks = R.text(f"FRAME: {i + 1}", 20, 30, 3, (0, 255, 255))
    for t in trackers:
        marks += t.results[i].marks(**t.draw_kwargs())
    return marks


def file_frames(path):
    clip = video.YuvClip.from_y4m(path, on_device=False)
    assert (clip.n, clip.w, clip.h, clip.fps) == (N, 640, 360, 30)
    return [clip._host_bytes(i, 1) for i in range(N)]


def host_frame(frames, i, marks):
    return R.render_host(frames[i:i + 1], *R.pack([marks]), out=E.RENDER_YUV420, geom=GEOM, enc=ENC)


def positions_by_hand(want):
    """into_dict of a per-frame loop's projections: metres from the court centre, ids 1..4 only."""
    ck = court_for(640, 360).court_keypoints
    expect = {"frame": list(range(N)), **{f"player{p}_{c}": [None] * N for p in (1, 2, 3, 4) for c in "xy"}}
    for i, (_, pp, _) in enumerate(want):
        for pid, (x, y) in pp:
            if pid in (1, 2, 3, 4):
                expect[f"player{pid}_x"][i] = (float(x) - ck.origin[0]) * 10 / ck.width
                expect[f"player{pid}_y"][i] = (float(y) - ck.origin[1]) * 10 / ck.width
    return expect


def test_fixed_keypoints_inset_and_collection(gpu_engine, tracked, clip_frames, tmp_path, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 3)
    fixed = court_keypoints_in_the_frame(12, seed=1, n=1)[0]
    keypoints = KeypointsTracker("no-model-is-needed.pt", batch_size=4, fixed_keypoints_detection=fixed)
    trackers = tracked + [keypoints]
    runner = TrackingRunner(trackers, SRC, tmp_path / "out.mp4", collect_data=True, render=tmp_path / "inset.y4m")
    assert runner.is_fixed_keypoints and runner.court_inset
    runner.run()
    assert len(keypoints) == N
    assert runner.timings["__render__"]["frames"] == N and runner.timings["__collect__"]["frames"] == N
    got = file_frames(tmp_path / "inset.y4m")
    court = court_for(640, 360)
    kinds = set()
    for i in range(N):
        marks = runner.frame_marks(i)
        base = plain_marks(trackers, i)
        assert marks[:len(base)] == base and marks[len(base):len(base) + 22] == court.inset_marks()
        kinds |= {m[0] for m in marks}
        assert np.array_equal(got[i], host_frame(clip_frames, i, marks)), i
    assert E.MARK_BLEND in kinds
    # the panel's pixels differ from the run without the inset (luma plane of frame 0)
    plain = TrackingRunner(trackers, SRC, tmp_path / "out.mp4", render=tmp_path / "plain.y4m")
    plain.run()
    without = file_frames(tmp_path / "plain.y4m")
    (x0, y0), (x1, y1) = court.background_position.top_left, court.background_position.bottom_right
    y_with, y_without = (b[:360 * 640].reshape(360, 640) for b in (got[0], without[0]))
    assert not np.array_equal(y_with[y0:y1 + 1, x0:x1 + 1], y_without[y0:y1 + 1, x0:x1 + 1])
    # the collected positions
    data = runner.data_analytics.into_dict()
    assert data["frame"] == list(range(N)) and len(runner.data_analytics) == N
    want, _ = plain_loop(court_for(640, 360), [fixed] * N, [t for t in tracked[0].results], [b for b in tracked[1].results], fixed=True)
    assert data == positions_by_hand(want)
    assert sum(v is not None for p in (1, 2, 3, 4) for v in data[f"player{p}_x"]) > 0
    assert all(p.projection is None for pl in tracked[0].results for p in pl)       # the stored results were not touched


def test_keypoints_per_frame_with_one_frame_that_has_none(gpu_engine, tracked, clip_frames, tmp_path, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 3)
    kps = court_keypoints_in_the_frame(22, seed=2, n=N)
    kps[3] = Keypoints([])                                                          # first frame of the second batch
    trackers = tracked + [Stored("keypoints_tracker", Keypoints, kps)]
    runner = TrackingRunner(trackers, SRC, tmp_path / "out.mp4", collect_data=True, render=tmp_path / "inset.y4m")
    assert not runner.is_fixed_keypoints
    runner.run()
    got = file_frames(tmp_path / "inset.y4m")
    inset = court_for(640, 360).inset_marks()
    for i in range(N):
        marks = runner.frame_marks(i)
        extra = marks[len(plain_marks(trackers, i)):]
        assert extra[:22] == inset
        if i == 3:
            assert len(extra) == 22                                                 # the inset, and no projections
        else:
            assert len(extra) > 22 + len(tracked[0].results[i])                    # a disc per player at least, and the ball
        if i in (2, 3, 4):
            assert np.array_equal(got[i], host_frame(clip_frames, i, marks)), i
    want, _ = plain_loop(court_for(640, 360), kps, list(tracked[0].results), list(tracked[1].results), fixed=False)
    data = runner.data_analytics.into_dict()
    assert data == positions_by_hand(want)
    assert all(data[f"player{p}_x"][3] is None for p in (1, 2, 3, 4)) and len(runner.data_analytics) == N


def test_without_collect_data_the_file_and_the_timings_are_what_they_were(gpu_engine, tracked, clip_frames, tmp_path, capsys):
    a = TrackingRunner(tracked, SRC, tmp_path / "out.mp4", render=tmp_path / "a.y4m")
    a.run()
    b = TrackingRunner(tracked, SRC, tmp_path / "out.mp4", collect_data=False, court_inset=None, render=tmp_path / "b.y4m")
    b.run()
    assert a.data_analytics is None and b.data_analytics is None and not b.court_inset
    assert set(a.timings) == set(b.timings) == {"__render__"}
    assert (tmp_path / "a.y4m").read_bytes() == (tmp_path / "b.y4m").read_bytes()
    got = file_frames(tmp_path / "b.y4m")
    for i in (0, N - 1):
        assert b.frame_marks(i) == plain_marks(tracked, i)
        assert np.array_equal(got[i], host_frame(clip_frames, i, plain_marks(tracked, i))), i
    capsys.readouterr()
    TrackingRunner(tracked, SRC, tmp_path / "out.mp4").run()
    assert "drawing / data collection is outside the hot path of this build (skipped)" in capsys.readouterr().out
