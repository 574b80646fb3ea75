"""``video.ResidentBatches`` without a GPU — which samples pass through and which are staged, into which slots, what the look-ahead
may overwrite, and that every way out of the walk gives the staging back — over a stand-in engine that counts its live buffers; the
runner's fan-out pass when a tracker raises; and ``activity.scan`` / ``identity.scan`` over engines whose kernels are the numpy twins."""
import threading
import time

import numpy as np
import pytest

from padel_analytics_amd import activity as A, identity as I, video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.tracker import NoPredictFrames, Tracker
from tests import identity_script as S
from tests.fake_engine import FakeBuffer, FakeEngine

N, H, W, CAP = 11, 8, 12, 4                      # batches of 4 + 4 + 3
FB = H * W * 3


class CountedBuffer(FakeBuffer):
    def view(self, offset, nbytes):
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return CountedBuffer(self.engine, nbytes, _arr=self.arr[offset:offset + nbytes])

    def upload(self, arr, copy_stream=False):
        super().upload(arr, copy_stream)
        self.engine.uploads.append((threading.current_thread(), copy_stream))
        return self

    def free(self):
        if self.owner and self.arr is not None:
            self.engine.live -= 1
            self.engine.events.append("free")
        super().free()


class Counting(FakeEngine):
    """``live``: buffers allocated and not freed; ``allocs``: the size of each; ``events``: synchronize and free, in order."""

    def __init__(self):
        super().__init__()
        self.live, self.allocs, self.events, self.uploads = 0, [], [], []

    def alloc(self, nbytes):
        self.live += 1
        self.allocs.append(int(nbytes))
        return CountedBuffer(self, nbytes)

    def synchronize(self):
        self.events.append("sync")


def frames_of(n=N, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def down(handles):
    buf, n, h, w = video.device_batch(handles)
    return buf.download(np.empty((n, h, w, 3), np.uint8))


def walk_of(eng, clip, **kw):
    return video.ResidentBatches(eng, video.sampler(clip.frames(), CAP), CAP, (H, W), **kw)


# ------------------------------------------------------------------------------------------------ residency
def test_host_frames_are_staged():
    eng, src = Counting(), frames_of()
    got = []
    with walk_of(eng, video.ArrayClip(src)) as walk:
        for frames, host in walk:
            assert all(isinstance(f, video.DeviceFrame) for f in frames) and [f.index for f in frames] == list(range(len(frames)))
            assert np.array_equal(down(frames), host)
            got.append(down(frames))
    assert [len(g) for g in got] == [4, 4, 3] and np.array_equal(np.concatenate(got), src)
    assert eng.allocs == [CAP * FB] and eng.live == 0
    assert [c for _, c in eng.uploads] == [False] * 3            # on the compute stream, from this thread
    assert {t for t, _ in eng.uploads} == {threading.current_thread()}


def test_a_device_clip_passes_through_and_allocates_nothing():
    eng, src = Counting(), frames_of()
    clip = video.DeviceClip(eng, src)
    samples = list(video.sampler(clip.frames(), CAP))
    before = list(eng.allocs)
    with video.ResidentBatches(eng, samples, CAP, (H, W), prefetch=True) as walk:
        for sample, (frames, host) in zip(samples, walk):
            assert frames is sample and host is None and np.array_equal(down(frames), src[sample[0].index:sample[0].index + len(sample)])
    assert eng.allocs == before and eng.live == 1
    clip.free()


class _Untouchable:
    """A clip without ``h``, ``w``, ``buffer``, ``frame_bytes``, ...: whoever asks it for one is told."""
    def __getattr__(self, name):
        raise AssertionError(f"the walk looked at the clip of a DeviceFrame handle (.{name})")


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("clip", [None, _Untouchable()], ids=["none", "untouchable"])
def test_device_frame_handles_are_not_looked_at(clip, prefetch):
    samples = list(video.sampler((video.DeviceFrame(clip, i) for i in range(N)), CAP))
    with video.ResidentBatches(None, samples, CAP, (H, W), prefetch=prefetch) as walk:       # (no engine: none is resolved either)
        got = list(walk)
        assert walk.engine is None
    assert len(got) == 3 and all(g[0] is s and g[1] is None for g, s in zip(got, samples))


def test_lead_slots_are_the_callers():
    eng, src = Counting(), frames_of()
    mark = np.full((1, H, W, 3), 201, np.uint8)
    with walk_of(eng, video.ArrayClip(src), lead=1) as walk:
        stage = walk.staging()
        assert stage.n == 1 + CAP and walk.staging() is stage
        stage.upload(mark, first=0)
        at = 0
        for frames, host in walk:
            assert [f.index for f in frames] == list(range(1, 1 + len(frames))) and all(f.clip is stage for f in frames)
            assert np.array_equal(down(frames), src[at:at + len(frames)])
            assert np.array_equal(down([video.DeviceFrame(stage, 0)]), mark)
            at += len(frames)
    assert at == N and eng.allocs == [(1 + CAP) * FB] and eng.live == 0


# ------------------------------------------------------------------------------------------------ prefetch
def test_a_yielded_batch_keeps_its_bytes_while_the_next_one_goes_up():
    eng, src = Counting(), frames_of(5 * CAP)
    at = 0
    with walk_of(eng, video.ArrayClip(src), prefetch=True) as walk:
        for k, (frames, host) in enumerate(walk):
            assert np.array_equal(down(frames), src[at:at + CAP])
            deadline = time.monotonic() + 5.0
            while len(eng.uploads) < min(k + 2, 5) and time.monotonic() < deadline:      # the next upload has run
                time.sleep(0.001)
            assert len(eng.uploads) == min(k + 2, 5)                                   # ... and none beyond it was started
            assert np.array_equal(down(frames), src[at:at + CAP]) and np.array_equal(host, src[at:at + CAP])
            at += CAP
    assert at == 5 * CAP and eng.allocs == [CAP * FB] * 2 and eng.live == 0
    assert all(c for _, c in eng.uploads) and len({t for t, _ in eng.uploads}) == 1 and threading.current_thread() not in {t for t, _ in eng.uploads}


# ------------------------------------------------------------------------------------------------ ownership
@pytest.mark.parametrize("ending", ["raise", "break", "end"])
@pytest.mark.parametrize("prefetch", [False, True])
def test_every_way_out_frees_the_staging(prefetch, ending):
    eng = Counting()
    keep = eng.alloc(16)                                         # a caller's buffer: the starting value is not zero
    threads = set(threading.enumerate())
    seen = 0
    try:
        with walk_of(eng, video.ArrayClip(frames_of()), prefetch=prefetch) as walk:
            for frames, host in walk:
                seen += 1
                assert eng.live == 1 + (2 if prefetch else 1)
                if ending == "raise" and seen == 2:
                    raise KeyError("consumer")
                if ending == "break" and seen == 1:
                    break
    except KeyError:
        assert ending == "raise"
    assert seen == {"raise": 2, "break": 1, "end": 3}[ending]
    assert eng.live == 1 and keep.arr is not None
    assert eng.events == ["sync"] + ["free"] * (2 if prefetch else 1)
    assert not [t for t in set(threading.enumerate()) - threads if t.is_alive()]


# ------------------------------------------------------------------------------------------------ the runner
class _N(int):
    def serialize(self): return int(self)


class _RaisesOnItsSecondBatch(Tracker):
    streams = False
    batch_size = CAP

    def __init__(self):
        self.batches = 0
        super().__init__()

    def video_info_post_init(self, video_info): return self
    def object(self): return _N
    def draw_kwargs(self): return {}
    def __str__(self): return "toy"
    def restart(self): self.results.restart()
    def predict_frames(self, frame_generator, **kw): raise NoPredictFrames()
    def predict_sample(self, sample, **kw): return self.post_sample(self.infer_sample(sample))
    def _has_stages(self): return True
    def post_sample(self, raw, **kw): return [_N(v) for v in raw]

    def infer_sample(self, sample, **kw):
        self.batches += 1
        if self.batches == 2:
            raise RuntimeError("device stage failed")
        return [int(v) for v in down(sample)[:, 0, 0, 0]]


def test_a_tracker_that_raises_in_the_fanout_pass_leaves_no_staging_behind(tmp_path):
    eng, src = Counting(), frames_of()
    keep = eng.alloc(16)
    tracker = _RaisesOnItsSecondBatch()
    with pytest.raises(RuntimeError, match="device stage failed"):
        TrackingRunner([tracker], video.ArrayClip(src), tmp_path / "out.mp4", fanout=True, engine=eng).run()
    assert tracker.batches == 2 and eng.allocs == [16, CAP * FB, CAP * FB]      # it did run over staged frames
    assert eng.live == 1 and keep.arr is not None
    assert eng.events.index("sync") < eng.events.index("free")


def test_the_fanout_pass_over_host_frames_feeds_every_frame_once(tmp_path):
    eng, src = Counting(), frames_of()
    tracker = _RaisesOnItsSecondBatch()
    tracker.batches = 2                                          # (past the batch it would fail on)
    TrackingRunner([tracker], video.ArrayClip(src), tmp_path / "out.mp4", fanout=True, engine=eng).run()
    assert [int(p) for p in tracker.results.predictions] == src[:, 0, 0, 0].tolist() and eng.live == 0


# ------------------------------------------------------------------------------------------------ the scans
class ActivityTwin(Counting):
    """``frame_activity`` is the numpy twin on the bytes of the views it is handed."""

    def frame_activity(self, src, n, h, w, ref, prev=None, roi=None, tau=24, out=None):
        img = lambda b: b.arr[:h * w * 3].reshape(h, w, 3)
        return A.frame_activity_host(src.arr[:n * h * w * 3].reshape(n, h, w, 3), img(ref), prev=None if prev is None else img(prev), roi=roi, tau=tau)


def _yuv_clip(eng, src):
    desc = video.yuv_desc(W, H, "i420")
    return video.YuvClip(video.bgr_to_yuv420_host(src, desc, video.YUV_ENC_COEFFS["bt601_limited"]), W, H, layout="i420", engine=eng)


SCAN_REF = frames_of(1, seed=9)[0]


@pytest.mark.parametrize("kind", ["array", "device", "device-repeated", "yuv-on-a-stand-in-engine"])
def test_activity_scan_equals_the_twin_over_batch_borders(kind):
    eng, src = ActivityTwin(), frames_of()
    batch, want_frames, clip = CAP, src, None
    if kind == "array":
        source = video.ArrayClip(src)
    elif kind == "device":
        source = clip = video.DeviceClip(eng, src)
    elif kind == "device-repeated":                              # a batch's predecessor is not the stored frame before it
        source = clip = video.DeviceClip(eng, src[:6], repeat=3)
        batch, want_frames = 6, np.concatenate([src[:6]] * 3)
    else:                                                        # the engine has no conversion kernel: staged from the host conversion
        source = _yuv_clip(eng, src)
        want_frames = np.stack([np.asarray(f) for f in source.frames()])
    live = eng.live
    act = A.scan(source, ref=SCAN_REF, roi=(1, 2, 11, 7), tau=24, batch=batch, engine=eng)
    want = A.frame_activity_host(want_frames, SCAN_REF, roi=(1, 2, 11, 7), tau=24)
    assert len(act) == len(want_frames) and act.npix == 50
    assert np.array_equal(act.sad_ref, want[:, 0]) and np.array_equal(act.changed, want[:, 1])
    assert np.array_equal(act.sad_prev, want[:, 2]) and act.sad_prev[0] == 0 and all(act.sad_prev[batch::batch] > 0)
    assert eng.live == live
    if kind == "device":                                         # read where it lies: the reference image is the only allocation
        assert eng.allocs[1:] == [FB]
    if clip is not None:
        clip.free()


class HistogramTwin(Counting):
    def box_histograms(self, src, n, h, w, rects, out=None):
        return I.box_histograms_host(src.arr[:n * h * w * 3].reshape(n, h, w, 3), rects)


def test_identity_scan_stages_only_the_batches_that_hold_a_rectangle():
    frames, results = S.clip(24), S.players_script(range(24))
    results[8:16] = [None] * 8                                   # the middle batch of three holds no box
    want = I.scan(video.ArrayClip(frames), results, on_device=False, batch=8)
    eng = HistogramTwin()
    got = I.scan(video.ArrayClip(frames), results, engine=eng, batch=8)
    assert sorted(got) == sorted(want) and sum(t.boxes for t in want.values()) > 0
    assert all(np.array_equal(got[t].hist, want[t].hist) and got[t].boxes == want[t].boxes and got[t].frames == want[t].frames for t in want)
    assert len(eng.uploads) == 2 and eng.allocs == [8 * S.H * S.W * 3] and eng.live == 0
