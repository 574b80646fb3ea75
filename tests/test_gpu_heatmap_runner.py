"""``TrackingRunner(heatmap=...)`` on the GPU, end to end over a 160 x 96 synthetic clip with fixed court keypoints.  No detector runs:
the ``Players`` and the ``Ball`` come from prediction caches the test writes (tests/identity_script.py's boxes).  With ``topdown=`` the
top-down ``.y4m`` equals ``warp_host``, then ``accumulate_host``, then ``render_host`` of every frame, the state carried from frame to
frame and from batch to batch; the ``.npy`` equals the CPU-path run's; the ``.jpg`` opens in Pillow at canvas size; and ``topdown=``
without ``heatmap=`` writes the bytes it wrote before ``heatmap=`` was ever given."""
import json

import numpy as np
import pytest

from padel_analytics_amd import engine as E, heatmap as HM, render as R, topdown as T, video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.ball_tracker import Ball
from tests import identity_script as S, synth  # noqa: F401  (synth registers the synthetic:// frame source)
from tests.test_gpu_topdown_runner import BallStub

pytestmark = pytest.mark.gpu

N, H, W = 11, S.H, S.W
SRC = f"synthetic://?n={N}&h={H}&w={W}&fps=30&seed=8"
OPTIONS = dict(px_per_m=8, margin_m=3, fill=(30, 60, 90))      # a 128 x 208 canvas: 16-byte accesses
CW, CH = 128, 208
HEAT = dict(radius_m=2.0, saturate_s=0.2)                      # r = 16 pixels, wider than the discs at the feet; full = 255 * 6


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    d = tmp_path_factory.mktemp("heatmap")
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


def test_the_clip_the_maps_and_the_picture(gpu_engine, script, tmp_path, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 4)                    # 11 frames: two whole batches and a short one
    for name in ("before", "shown", "after", "host", "picture"):
        (tmp_path / name).mkdir()
    run(script, tmp_path / "before", topdown=tmp_path / "before" / "top.y4m", topdown_options=OPTIONS)
    runner = run(script, tmp_path / "shown", topdown=tmp_path / "shown" / "top.y4m", topdown_options=OPTIONS, heatmap=tmp_path / "shown" / "h.npy",
                 heatmap_options=HEAT)
    assert gpu_engine.heat_last_path() == E.HEAT_PATH_VECTOR and runner.topdown_view.size == (CW, CH)
    assert (runner.heat.r, runner.heat.full, runner.heat.planes) == (16, 255 * 6, 4)
    assert {"__topdown__", "__heatmap__"} == set(runner.timings) and runner.timings["__heatmap__"]["frames"] == N
    assert sorted(p.name for p in (tmp_path / "shown").iterdir()) == ["h.npy", "top.y4m"]
    # the clip: warp_host, then accumulate_host with the state carried, then render_host, frame by frame
    heat, view = runner.heat, runner.topdown_view
    clip = video.YuvClip.from_y4m(tmp_path / "shown" / "top.y4m", on_device=False)
    assert (clip.n, clip.w, clip.h) == (N, CW, CH)
    geom, enc = video.yuv_desc(CW, CH, "i420"), video.YUV_ENC_COEFFS["bt601_limited"]
    state = heat.state()
    blended = 0
    for i in range(N):
        m, valid = view.matrices(runner._projected[i:i + 1])
        canvas = T.warp_host(script["frames"][i:i + 1], m, valid, CH, CW, view.fill)
        plain = canvas.copy()
        pts, first, hvalid = heat.batch(runner._projected[i:i + 1], [runner.trackers["players_tracker"].results[i]])
        assert len(pts) == 4 and hvalid[0] == 1
        HM.accumulate_host(canvas, state, pts, first, hvalid, **heat.call())
        blended += int((canvas != plain).any(axis=-1).sum())
        want = R.render_host(canvas, *R.pack([runner.topdown_marks(i)]), out=E.RENDER_YUV420, geom=geom, enc=enc)
        assert np.array_equal(clip._host_bytes(i, 1), want), i
    assert blended > 1000 * N                                 # four bumps of radius 16 a frame
    # the maps: the kernel's, the file's and the CPU-path run's (no topdown=: the stored results alone) are the twin's
    assert np.array_equal(runner.heat_state, state) and all(state[p].any() for p in range(4))
    assert np.array_equal(np.load(tmp_path / "shown" / "h.npy"), state)
    host = run(script, tmp_path / "host", heatmap=tmp_path / "host" / "h.npy", heatmap_options=HEAT, topdown_options=OPTIONS)
    assert np.array_equal(np.load(tmp_path / "host" / "h.npy"), state) and set(host.timings) == {"__heatmap__"}
    # the picture opens at canvas size, and it is the host path's, byte for byte
    run(script, tmp_path / "picture", topdown=tmp_path / "picture" / "top.y4m", topdown_options=OPTIONS, heatmap=tmp_path / "picture" / "h.jpg",
        heatmap_options=HEAT)
    from PIL import Image
    with Image.open(tmp_path / "picture" / "h.jpg") as im:
        assert im.size == (CW, CH) and im.format == "JPEG"
        rgb = np.asarray(im.convert("RGB")).astype(int)
    at = np.unravel_index(np.argmax(HM.shown_density(state, 15)), (CH, CW))
    assert rgb[at][0] > 150 and rgb[at][2] < 100              # the peak is at the ramp's red end; far from the players the fill
    assert np.abs(rgb[2, 2] - np.array(OPTIONS["fill"][::-1])).max() < 30
    run(script, tmp_path / "host", heatmap=tmp_path / "host" / "h.jpg", heatmap_options=HEAT, topdown_options=OPTIONS)
    assert (tmp_path / "picture" / "h.jpg").read_bytes() == (tmp_path / "host" / "h.jpg").read_bytes()
    # topdown= without heatmap=: the bytes of the run made before the argument was touched, and not the overlaid clip's
    run(script, tmp_path / "after", topdown=tmp_path / "after" / "top.y4m", topdown_options=OPTIONS)
    before = (tmp_path / "before" / "top.y4m").read_bytes()
    assert before == (tmp_path / "after" / "top.y4m").read_bytes() and before != (tmp_path / "shown" / "top.y4m").read_bytes()
