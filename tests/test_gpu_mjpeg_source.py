"""Motion-JPEG as the runner's source on the GPU: tracker results from an ``.avi`` path (frames decoded by csrc/jpeg_decode.hip into the
clip's staging buffer) are bit-identical to those from an ``ArrayClip`` of ``mjpeg.decode_host``'s frames; fan-out decodes each batch
once; and the ``.avi`` the runner renders is a source the runner reads."""
import json

import numpy as np
import pytest

from padel_analytics_amd import mjpeg, video
from tests import synth
from tests.test_gpu_yuv import H, N, W, _ball, _court, _players, _run
from tests.test_mjpeg_decode_host import write_clip

pytestmark = pytest.mark.gpu


class _Sources:
    """13 synthetic frames written by ``MjpegSink`` (host encoder) as ``clip.avi``; ``ref``: the twin's decoding of that file."""

    def __init__(self, tmp):
        paths, jpegs = write_clip(str(tmp / "clip.avi"), synth.synthetic_frames(N, H, W, seed=15), fps=30)
        self.avi = paths[0]
        self.ref = video.ArrayClip(mjpeg.decode_host(np.frombuffer(b"".join(jpegs), np.uint8), np.cumsum([0] + [len(j) for j in jpegs])))


@pytest.fixture(scope="module")
def sources(gpu_engine, tmp_path_factory):
    s = _Sources(tmp_path_factory.mktemp("mjpeg_source"))
    yield s
    video._open_mjpeg(s.avi).free()


def _close(trackers):
    for t in trackers:
        m = getattr(t, "model", None)
        if m is not None and hasattr(m, "close"):
            m.close()


@pytest.mark.parametrize("which", ["players", "ball", "court"])
def test_tracker_results_from_an_avi_path_are_bit_identical(gpu_engine, sources, tmp_path, which):
    t = {"players": _players, "ball": _ball, "court": _court}[which](tmp_path)
    try:
        want = _run([t], sources.ref, tmp_path)
        if which == "players":
            assert sum(len(f) for f in json.loads(want[str(t)])) > 0, "the reference run found no player to compare"
        clip = video._open_mjpeg(sources.avi)
        assert clip.on_device and (clip.n, clip.w, clip.h, clip.fps) == (N, W, H, 30)
        clip.invalidate()
        before = clip.decodes
        assert _run([t], sources.avi, tmp_path) == want
        assert clip.decodes - before >= 3 and clip._bgr is not None and not clip.corrupt      # the frames did come through the kernels
    finally:
        _close([t])


def test_fanout_over_an_avi_decodes_each_batch_once(gpu_engine, sources, tmp_path):
    trackers = [_players(tmp_path), _ball(tmp_path), _court(tmp_path)]
    try:
        want = _run(trackers, sources.ref, tmp_path, fanout=True, engine=gpu_engine)
        clip = video._open_mjpeg(sources.avi)
        clip.invalidate()
        asked, decoded = [], []
        real_view, real_decode = clip.device_view, clip._to_device
        clip.device_view = lambda first, count: (asked.append((first, count)), real_view(first, count))[1]
        clip._to_device = lambda eng, first, count: (decoded.append((first, count)), real_decode(eng, first, count))[1]
        try:
            got = _run(trackers, sources.avi, tmp_path, fanout=True, engine=gpu_engine)
        finally:
            del clip.device_view, clip._to_device
        assert got == want
        # the fan-out pass: the runner and the players tracker both ask for each of the 3 batches, each is decoded once (then the stream
        # trackers' own passes: tests/test_gpu_yuv.py counts the same requests for a YUV clip)
        assert asked[:6] == [(0, 5), (0, 5), (5, 5), (5, 5), (10, 3), (10, 3)], asked
        assert decoded[:3] == [(0, 5), (5, 5), (10, 3)] and len(decoded) >= 9 and len(asked) >= 13, (asked, decoded)
    finally:
        _close(trackers)


def test_the_avi_the_runner_renders_is_a_source_for_the_runner(gpu_engine, sources, tmp_path):
    from padel_analytics_amd.trackers import TrackingRunner
    t = _players(tmp_path)
    try:
        r = TrackingRunner([t], sources.avi, tmp_path / "out.mp4", render=tmp_path / "out.avi")
        r.restart()
        r.run()
        assert r.timings["__render__"]["frames"] == N
        out = str(tmp_path / "out.avi")
        info = video.VideoInfo.from_video_path(out)
        assert (info.width, info.height, info.fps, info.total_frames) == (W, H, 30, N)
        idx = mjpeg.index_file(out)
        want = video.ArrayClip(mjpeg.decode_host(*idx.batch(0, N)))
        assert not np.array_equal(want.array, sources.ref.array)                  # the players were drawn into it
        a = _run([t], want, tmp_path)
        assert _run([t], out, tmp_path) == a and not video._open_mjpeg(out).corrupt
        video._open_mjpeg(out).free()
    finally:
        _close([t])
