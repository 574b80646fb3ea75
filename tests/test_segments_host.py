"""``TrackingRunner(segments=...)`` without a GPU: stub trackers that record what they are fed, no engine, ``render=None``."""
import numpy as np
import pytest

from padel_analytics_amd import video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.tracker import NoPredictFrames, NoPredictSample, Object, Tracker

SEGMENTS = [(0, 5), (9, 20), (23, 30)]
KEPT = [i for lo, hi in SEGMENTS for i in range(lo, hi)]


def clip(n=30):
    """Frame i is filled with the value i: a frame tells its own number."""
    return video.ArrayClip(np.arange(n, dtype=np.uint8)[:, None, None, None] * np.ones((1, 4, 6, 3), np.uint8))


class Seen(Object):
    def __init__(self, frame, source, state):
        self.frame, self.source, self.state = frame, source, state

    def serialize(self):
        return {"frame": self.frame, "source": self.source, "state": self.state}


class _Stub(Tracker):
    DEVICE = "cpu"

    def __init__(self, batch_size=8):
        super().__init__()
        self.batch_size = batch_size
        self.calls = []                    # the source frame numbers of every batch / stream it was handed
        self.count = 0                     # state carried from call to call, like ByteTrack's

    def video_info_post_init(self, video_info): return self
    def object(self): return Seen
    def draw_kwargs(self): return {}
    def restart(self): self.results.restart()
    def __str__(self): return type(self).__name__


class BatchStub(_Stub):
    def predict_sample(self, sample, **kwargs):
        nums = [int(f[0, 0, 0]) for f in sample]
        self.calls.append(nums)
        out = []
        for k in nums:
            out.append(Seen(None, k, self.count))
            self.count += 1
        return out

    def predict_frames(self, frame_generator, **kwargs):
        raise NoPredictFrames()


class StreamStub(_Stub):
    streams = True

    def predict_sample(self, sample, **kwargs):
        raise NoPredictSample()

    def predict_frames(self, frame_generator, **kwargs):
        nums = [int(f[0, 0, 0]) for f in frame_generator]
        self.calls.append(nums)
        out = []
        for i, k in enumerate(nums):
            out.append(Seen(i, k, self.count))           # frame: counted from the start of what it was fed, like Ball.frame
            self.count += 1
        return out


def test_trackers_see_only_the_kept_frames_and_no_batch_spans_a_cut(tmp_path):
    batch, stream = BatchStub(8), StreamStub(8)
    runner = TrackingRunner([batch, stream], clip(), tmp_path / "out.mp4", segments=SEGMENTS)
    assert runner.source_index.dtype == np.int64 and runner.source_index.tolist() == KEPT
    assert runner.n_available == runner.total_frames == 23
    runner.run()
    assert len(batch.results) == len(stream.results) == 23
    # in order, only kept frames
    assert [k for call in batch.calls for k in call] == KEPT
    assert [o.source for o in batch.results] == KEPT and [o.source for o in stream.results] == KEPT
    # every batch inside one segment, of at most batch_size frames: 5 | 8, 3 | 7
    assert batch.calls == [[0, 1, 2, 3, 4], list(range(9, 17)), [17, 18, 19], list(range(23, 30))]
    for call in batch.calls:
        assert any(lo <= call[0] and call[-1] < hi for lo, hi in SEGMENTS)
    # the stream tracker gets one stream per segment; its frame numbers are kept positions
    assert stream.calls == [list(range(lo, hi)) for lo, hi in SEGMENTS]
    assert [o.frame for o in stream.results] == list(range(23))
    # state carries over the cuts
    assert [o.state for o in batch.results] == list(range(23)) and [o.state for o in stream.results] == list(range(23))
    assert runner.timings["BatchStub"]["frames"] == 23


def test_start_and_end_bound_the_segments(tmp_path):
    t = BatchStub(4)
    runner = TrackingRunner([t], clip(), tmp_path / "out.mp4", start=3, end=25, segments=[(3, 6), (20, 25)])
    runner.run()
    assert runner.source_index.tolist() == [3, 4, 5, 20, 21, 22, 23, 24]
    assert t.calls == [[3, 4, 5], [20, 21, 22, 23], [24]]


def test_no_segments_leaves_everything_as_it_was(tmp_path):
    t = BatchStub(8)
    runner = TrackingRunner([t], clip(), tmp_path / "out.mp4")
    assert runner.segments is None and runner.source_index.tolist() == list(range(30)) and runner.n_available == 30
    runner.run()
    assert t.calls == [list(range(0, 8)), list(range(8, 16)), list(range(16, 24)), list(range(24, 30))]
    assert "__segments__" not in runner.timings


@pytest.mark.parametrize("segments,words", [
    ([(9, 20), (0, 5)], "(0, 5)"),                      # unsorted
    ([(0, 10), (9, 20)], "(9, 20)"),                    # overlapping
    ([(0, 5), (7, 7)], "(7, 7) is empty"),              # empty
    ([(0, 5), (8, 6)], "(8, 6) is empty"),
    ([(0, 5), (25, 31)], "(25, 31) leaves"),            # out of range
    ([(-1, 5)], "(-1, 5) leaves"),
])
def test_bad_segments_are_refused_naming_the_pair(tmp_path, segments, words):
    with pytest.raises(ValueError) as ex:
        TrackingRunner([BatchStub()], clip(), tmp_path / "out.mp4", segments=segments)
    assert words in str(ex.value)


def test_segments_outside_start_and_end_are_refused(tmp_path):
    with pytest.raises(ValueError, match=r"\(0, 5\) leaves the frames \[3, 25\)"):
        TrackingRunner([BatchStub()], clip(), tmp_path / "out.mp4", start=3, end=25, segments=[(0, 5)])
    with pytest.raises(ValueError, match=r"\(20, 26\) leaves"):
        TrackingRunner([BatchStub()], clip(), tmp_path / "out.mp4", start=3, end=25, segments=[(20, 26)])


@pytest.mark.parametrize("kw", [dict(distributed=True), dict(fanout=True)], ids=["distributed", "fanout"])
def test_segments_with_distributed_or_fanout_are_refused(tmp_path, kw):
    with pytest.raises(ValueError, match="distributed=True or fanout=True"):
        TrackingRunner([BatchStub()], clip(), tmp_path / "out.mp4", segments=SEGMENTS, **kw)
    with pytest.raises(ValueError, match="distributed=True or fanout=True"):
        TrackingRunner([BatchStub()], clip(), tmp_path / "out.mp4", segments="court", **kw)


def test_an_unknown_word_is_refused(tmp_path):
    with pytest.raises(ValueError, match="court"):
        TrackingRunner([BatchStub()], clip(), tmp_path / "out.mp4", segments="rallies")


def test_collection_without_render_walks_the_kept_frames(tmp_path):
    t = BatchStub(8)
    runner = TrackingRunner([t], clip(), tmp_path / "out.mp4", segments=SEGMENTS, collect_data=True)
    runner.run()
    assert runner.timings["__collect__"]["frames"] == 23
