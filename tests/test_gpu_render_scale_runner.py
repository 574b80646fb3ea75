"""``TrackingRunner(render=..., render_scale=2)`` on the GPU: the ``.y4m`` holds ``render.render_host(scale=2)`` of every frame under
the runner's own ``frame_marks`` (the marks stay in source pixels), the ``.avi`` is ``mjpeg.encode_host`` of those planes, scale 1
writes the file the runner writes without the argument, and the collected data do not depend on the scale.  640 x 360, 5 synthetic
frames, 2 frames per render batch; a players tracker on synthetic weights and fixed court keypoints, which need no model."""
import numpy as np
import pytest

from padel_analytics_amd import checkpoint, detections as D, engine as E, mjpeg, render as R, video, yolo_arch
from padel_analytics_amd.trackers import KeypointsTracker, PlayerTracker, TrackingRunner
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)
from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
from tests.court_script import court_for, frame_keypoints, true_homography

pytestmark = pytest.mark.gpu

N = 5
SRC = f"synthetic://?n={N}&h=360&w=640&fps=30&seed=15"


def court_keypoints_in_the_frame(count, seed, n):
    """``n`` detections of ``count`` court keypoints as a camera over a 640 x 360 frame sees them (court_script's 1280 x 720 camera at
    half size)."""
    court = court_for(640, 360)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        H = true_homography(court, rng, jitter=3.0) @ np.diag([2.0, 2.0, 1.0])
        src, _ = frame_keypoints(court, count, H, rng, noise=0.5)
        out.append(Keypoints([Keypoint(j, (float(x), float(y))) for j, (x, y) in enumerate(src)]))
    return out


@pytest.fixture(scope="module")
def tracked(gpu_engine, tmp_path_factory):
    """The players tracker and the fixed-keypoints tracker with their results of the 5 frames stored."""
    d = tmp_path_factory.mktemp("scale_runner")
    checkpoint.save_checkpoint(d / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None, "n", {0: "person"})
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    players = PlayerTracker(str(d / "players.pt"), zone, batch_size=4)
    keypoints = KeypointsTracker("no-model-is-needed.pt", batch_size=4, fixed_keypoints_detection=court_keypoints_in_the_frame(12, seed=1, n=1)[0])
    trackers = [players, keypoints]
    TrackingRunner(trackers, SRC, d / "out.mp4").run()
    assert [len(t) for t in trackers] == [N, N]
    yield trackers
    players.model.close()


@pytest.fixture(scope="module")
def clip_frames():
    return np.stack(list(video.get_video_frames_generator(SRC)))


@pytest.fixture(scope="module")
def half_planes(tracked, clip_frames):
    """-> planes(runner, sink geometry, encode table): ``render_host(scale=2)`` of every frame under the runner's marks (the tracked
    results are the same for every runner of this module, so are the marks: computed once per encode table)."""
    cache = {}

    def planes(runner, desc, enc):
        key = tuple(enc)
        if key not in cache:
            cache[key] = [R.render_host(clip_frames[i:i + 1], *R.pack([runner.frame_marks(i)]), out=E.RENDER_YUV420, geom=desc, enc=enc, scale=2)
                          for i in range(N)]
        return cache[key]
    return planes


def test_the_y4m_at_half_size_is_the_twin_of_every_frame(gpu_engine, tracked, clip_frames, half_planes, tmp_path, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 2)                    # two whole batches and a short last one
    runner = TrackingRunner(tracked, SRC, tmp_path / "out.mp4", render=tmp_path / "half.y4m", render_scale=2)
    runner.run()
    assert runner.timings["__render__"]["frames"] == N
    assert runner.timings["__render__"]["bytes"] == (tmp_path / "half.y4m").stat().st_size
    clip = video.YuvClip.from_y4m(tmp_path / "half.y4m", on_device=False)
    assert (clip.n, clip.w, clip.h, clip.fps) == (N, 320, 180, 30)
    geom = video.yuv_desc(320, 180, "i420")
    want = half_planes(runner, geom, video.YUV_ENC_COEFFS["bt601_limited"])
    kinds = set()
    for i in range(N):
        kinds |= {m[0] for m in runner.frame_marks(i)}
        assert np.array_equal(clip._host_bytes(i, 1), want[i]), i
    assert {E.MARK_BOX, E.MARK_GLYPH} <= kinds                                # the players and their labels were drawn
    plain = video.bgr_to_yuv420_host(R.downscale_host(clip_frames[:1], 2), geom, video.YUV_ENC_COEFFS["bt601_limited"])
    assert not np.array_equal(clip._host_bytes(0, 1), plain)


def test_the_avi_at_half_size_is_the_encode_of_the_twins_planes(gpu_engine, tracked, half_planes, tmp_path):
    runner = TrackingRunner(tracked, SRC, tmp_path / "out.mp4", render=tmp_path / "half.avi", render_scale=2, render_quality=85)
    runner.run()
    desc = video.yuv_desc(320, 180, "i420", "bt601", "full")
    want = half_planes(runner, desc, video.YUV_ENC_COEFFS["bt601_full"])
    raw = (tmp_path / "half.avi").read_bytes()
    assert runner.timings["__render__"]["bytes"] == len(raw)
    at = 0
    for i in range(N):
        data, off = mjpeg.encode_host(want[i], 1, 180, 320, desc, 85)
        jpg = data[off[0]:off[1]].tobytes()
        at = raw.find(jpg, at)
        assert at > 0, i                                                      # every frame's JPEG, in order
        at += len(jpg)


def test_scale_1_writes_the_file_written_without_the_argument(gpu_engine, tracked, tmp_path):
    TrackingRunner(tracked, SRC, tmp_path / "out.mp4", render=tmp_path / "a.y4m").run()
    TrackingRunner(tracked, SRC, tmp_path / "out.mp4", render=tmp_path / "b.y4m", render_scale=1).run()
    assert (tmp_path / "a.y4m").read_bytes() == (tmp_path / "b.y4m").read_bytes()
    assert video.YuvClip.from_y4m(tmp_path / "a.y4m", on_device=False).w == 640


def test_the_collected_data_do_not_depend_on_the_scale(gpu_engine, tracked, clip_frames, tmp_path):
    got = {}
    for s in (1, 2):
        runner = TrackingRunner(tracked, SRC, tmp_path / "out.mp4", collect_data=True, render=tmp_path / f"inset{s}.y4m", render_scale=s)
        assert runner.is_fixed_keypoints and runner.court_inset
        runner.run()
        got[s] = (runner.data_analytics.into_dict(), [runner.frame_marks(i) for i in range(N)])
    assert got[1][0] == got[2][0] and len(got[1][0]["frame"]) == N
    assert got[1][1] == got[2][1]                                             # the marks too: they stay in source pixels
    assert E.MARK_BLEND in {m[0] for m in got[2][1][0]}                       # (the inset's panel is among them)
    clip = video.YuvClip.from_y4m(tmp_path / "inset2.y4m", on_device=False)
    want = R.render_host(clip_frames[:1], *R.pack([got[2][1][0]]), out=E.RENDER_YUV420, geom=video.yuv_desc(320, 180, "i420"),
                         enc=video.YUV_ENC_COEFFS["bt601_limited"], scale=2)
    assert np.array_equal(clip._host_bytes(0, 1), want)
