"""The runner's output step with every output on at once, without a GPU: ``render=`` at ``render_scale=2`` with the inset and the
ball's trail, ``topdown=`` with the heat maps shown on it, ``heatmap=`` as a picture and ``collect_data`` over one walk of a clip in
two segments, on the recording twin engine — against runs with one output on each, and what is freed and closed when the engine
raises in the middle of the walk."""
import numpy as np
import pytest

from padel_analytics_amd import video
from padel_analytics_amd.trackers import TrackingRunner
from tests import fake_engine, synth  # noqa: F401  (synth registers the synthetic:// frame source)
from tests.test_heatmap_host import CH, CW, H, HEAT, OPTIONS, SRC, W, scripted_trackers
from tests.twin_engine import StandInEngine, TwinEngine


# ---------------------------------------------------------------------------------------------- the sinks' one rule (video.py)
def test_every_suffix_is_recognised_in_either_case_and_a_sink_passes_through(tmp_path):
    assert video.MJPEG_SUFFIXES == (".avi", ".mjpeg", ".mjpg")
    for suffix in video.MJPEG_SUFFIXES + (".y4m", ".bin", ""):
        for name in ("x" + suffix, "X" + suffix.upper()):
            kind = video.MjpegSink if suffix in video.MJPEG_SUFFIXES else video.Y4mSink
            assert video.check_sink(tmp_path / name, 64, 48, 77) is None and not (tmp_path / name).exists()
            sink, own = video.open_sink(tmp_path / name, 64, 48, 24, 77)
            assert type(sink) is kind and own is True and (sink.w, sink.h, sink.fps, sink.path) == (64, 48, 24, str(tmp_path / name))
            assert sink.quality == 77 if kind is video.MjpegSink else sink.desc == video.yuv_desc(64, 48, "i420")
            sink.close()
            (tmp_path / name).unlink()
    with video.Y4mSink(tmp_path / "mine.y4m", 64, 48) as mine:
        assert video.open_sink(mine, 64, 48) == (mine, False) and video.open_sink(mine, 32, 24) == (mine, False)
        assert video.check_sink(mine, 64, 48) is None
        with pytest.raises(ValueError, match=r"^the sink takes 64 x 48 frames$"):
            video.check_sink(mine, 32, 24)
    assert video.check_sink(video.FrameSink(), 32, 24) is None            # a sink that states no size


@pytest.mark.parametrize("name, w, h, quality", [("wide.avi", 2562, 48, 90), ("wide.MJPG", 2562, 48, 90), ("odd.y4m", 63, 48, 90),
                                                 ("odd.bin", 64, 47, 90), ("odd.mjpeg", 64, 1, 90), ("q.avi", 64, 48, 0)])
def test_the_check_without_a_file_says_what_opening_says(tmp_path, name, w, h, quality):
    with pytest.raises(ValueError) as opening:
        video.open_sink(tmp_path / name, w, h, 30, quality)
    with pytest.raises(ValueError) as checking:
        video.check_sink(tmp_path / name, w, h, quality)
    assert str(checking.value) == str(opening.value) and str(opening.value)
    assert ("2560" in str(opening.value)) == name.startswith("wide") and ("even" in str(opening.value)) == name.startswith("odd")
    assert list(tmp_path.iterdir()) == []                     # neither created anything


# ---------------------------------------------------------------------------------------------- every output at once
KEPT = [(1, 2), (3, 5)]
EVERYTHING = dict(render_scale=2, collect_data=True, ball_trail=2, topdown_options=OPTIONS, heatmap_options=HEAT)


class CountingEngine(TwinEngine):
    """``TwinEngine`` that keeps every buffer it hands out, and raises in its ``fail_at``-th ``render``."""

    def __init__(self, fail_at=None):
        super().__init__()
        self.buffers, self.fail_at = [], fail_at

    def alloc(self, nbytes):
        self.buffers.append(super().alloc(nbytes))
        return self.buffers[-1]

    def render(self, *a, **kw):
        if sum(c[0] == "render" for c in self.calls) + 1 == self.fail_at:
            raise RuntimeError("the renderer gave up")
        super().render(*a, **kw)


def run(where, monkeypatch, eng, **kw):
    """One run over the kept frames of the 5-frame 96 x 160 clip in batches of 2 -> (runner, the ranges of the clip that were read)."""
    where.mkdir(exist_ok=True)
    walks = []
    real = video.get_video_frames_generator

    def recording(source, stride=1, start=0, end=None):
        walks.append((start, end))
        return real(source, stride=stride, start=start, end=end)
    trackers = scripted_trackers()
    for t in trackers:
        t.results.predictions = [t.results.predictions[i] for lo, hi in KEPT for i in range(lo, hi)]
    with monkeypatch.context() as m:
        m.setattr(video, "get_video_frames_generator", recording)
        m.setattr(TrackingRunner, "RENDER_BATCH", 2)
        runner = TrackingRunner(trackers, SRC, where / "out.mp4", engine=eng, segments=KEPT, **kw)
        runner.run()
    return runner, walks


def test_every_output_at_once_equals_one_output_at_a_time(tmp_path, monkeypatch):
    """The top-down clip shows the maps, so the run it is compared with has ``heatmap=`` beside ``topdown=``: the maps are part of that
    output.  The run of the heat maps alone makes the picture on the host, from the stored results."""
    eng = TwinEngine()
    both, walks = run(tmp_path, monkeypatch, eng, render=tmp_path / "r.y4m", topdown=tmp_path / "t.y4m", heatmap=tmp_path / "h.jpg", **EVERYTHING)
    assert walks == KEPT                                      # once per piece of the segments, not once per output
    # the pieces hold 1 and 2 frames: a batch of each.  Per batch the frame render, the warp, the heat call, the canvas render
    names = [c[0] for c in eng.calls]
    assert names == ["render", "warp", "heat", "render"] * 2 + ["heat", "render", "jpeg_encode"]
    assert [c[1] for c in eng.calls[:8]] == [s for n in (1, 2) for s in ((n, H, W), (n, H, W, CH, CW), (n, CH, CW, 4), (n, CH, CW))]
    assert [set(c[2]) for c in eng.calls if c[0] == "render"] == [{"out", "geom", "enc", "scale"}, {"out", "geom", "enc"}] * 2 + [{"out", "geom", "enc"}]
    assert eng.calls[0][2]["scale"] == 2 and [c[1] for c in eng.calls[-3:]] == [(1, CH, CW, 4), (1, CH, CW), (1, CH, CW)]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["h.jpg", "r.y4m", "t.y4m"]
    assert sorted(both.timings) == ["__collect__", "__heatmap__", "__render__", "__topdown__"]
    assert all(both.timings[k]["frames"] == 3 and both.timings[k]["seconds"] > 0 for k in both.timings)
    assert both.timings["__render__"]["bytes"] == (tmp_path / "r.y4m").stat().st_size
    assert both.timings["__topdown__"]["bytes"] == (tmp_path / "t.y4m").stat().st_size

    one = tmp_path / "one"
    clip, walks = run(one, monkeypatch, TwinEngine(), render=one / "r.y4m", court_inset=True, render_scale=2, ball_trail=2)
    assert walks == KEPT and (tmp_path / "r.y4m").read_bytes() == (one / "r.y4m").read_bytes()
    top, walks = run(one, monkeypatch, TwinEngine(), topdown=one / "t.y4m", heatmap=one / "h.npy", topdown_options=OPTIONS, heatmap_options=HEAT)
    assert walks == KEPT and (tmp_path / "t.y4m").read_bytes() == (one / "t.y4m").read_bytes()
    maps, walks = run(one, monkeypatch, StandInEngine(), heatmap=one / "h.jpg", topdown_options=OPTIONS, heatmap_options=HEAT)
    assert walks == [] and (tmp_path / "h.jpg").read_bytes() == (one / "h.jpg").read_bytes()
    assert both.heat_state.any() and np.array_equal(both.heat_state, maps.heat_state) and np.array_equal(both.heat_state, top.heat_state)
    assert np.array_equal(np.load(one / "h.npy"), both.heat_state)
    data, walks = run(one, monkeypatch, StandInEngine(), collect_data=True)
    assert walks == [] and both.data_analytics.frames == data.data_analytics.frames == [0, 1, 2]
    assert both.data_analytics.into_dict() == data.data_analytics.into_dict()
    assert clip.data_analytics is None and len(both._projected) == 3


@pytest.mark.parametrize("fail_at", [3, 4])
def test_an_engine_that_raises_in_the_second_batch_leaves_nothing_allocated_or_open(tmp_path, monkeypatch, fail_at):
    """The third ``render`` is the second batch's frame render, the fourth its canvas render."""
    sinks, freed = [], []

    class Recorded(video.Y4mSink):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            sinks.append(self)

    real_free = fake_engine.FakeBuffer.free
    monkeypatch.setattr(video, "Y4mSink", Recorded)
    monkeypatch.setattr(fake_engine.FakeBuffer, "free", lambda self: (freed.append(self), real_free(self))[1])
    eng = CountingEngine(fail_at=fail_at)
    with pytest.raises(RuntimeError, match="the renderer gave up"):
        run(tmp_path, monkeypatch, eng, render=tmp_path / "r.y4m", topdown=tmp_path / "t.y4m", heatmap=tmp_path / "h.jpg", **EVERYTHING)
    assert [c[0] for c in eng.calls] == ["render", "warp", "heat", "render"] + ["render", "warp", "heat"][:3 * (fail_at - 3)]
    # the rendered frames, the canvases, the canvas frames, the maps, and the walk's staging of the clip's frames
    assert len(eng.buffers) == 5 and all(b.arr is None for b in eng.buffers)
    assert len(freed) == len(eng.buffers) and {id(b) for b in freed} == {id(b) for b in eng.buffers}
    assert sorted(s.path for s in sinks) == [str(tmp_path / "r.y4m"), str(tmp_path / "t.y4m")] and all(s._fh is None for s in sinks)
    assert [s.frames_written for s in sorted(sinks, key=lambda s: s.path)] == [1 if fail_at == 3 else 3, 1] and not (tmp_path / "h.jpg").exists()
