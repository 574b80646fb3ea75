"""GPU: ``Engine.frame_activity`` (csrc/frame_activity.hip) equals its numpy twin exactly — every geometry, roi, content, tau, with and
without ``prev``, at any alignment of the frames, whatever the batch — ``Engine.frames_median`` equals ``np.median``, and
``activity.scan`` over a host clip, a device clip and a ``.y4m`` file equals the twin on the frames."""
import numpy as np
import pytest

from padel_analytics_amd import activity as A, engine as E, video

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (5, 7), (16, 16), (33, 65)]


def rois(h, w):
    """whole frame, one pixel, one column, the frame without its border, a roi whose byte offset is no multiple of 16"""
    out = {"whole": None, "pixel": (w - 1, h - 1, w, h), "column": (w // 2, 0, w // 2 + 1, h)}
    if w > 2 and h > 2:
        out["inner"] = (1, 1, w - 1, h - 1)
    if w > 3:
        out["odd-offset"] = (3, 0, w, h)               # 9 bytes into the row
    return out


def on_device(eng, frames, ref, prev=None, roi=None, tau=24, lead=0, out=None):
    """``frames`` behind ``lead`` other frames of one DeviceBuffer -> Engine.frame_activity."""
    n, h, w = frames.shape[:3]
    fb = h * w * 3
    junk = np.full((lead, h, w, 3), 171, np.uint8)
    buf = eng.alloc((lead + n) * fb).upload(np.concatenate([junk, frames]))
    d_ref = eng.alloc(fb).upload(ref)
    d_prev = eng.alloc(fb).upload(prev) if prev is not None else None
    try:
        return eng.frame_activity(buf.view(lead * fb, n * fb), n, h, w, d_ref, prev=d_prev, roi=roi, tau=tau, out=out)
    finally:
        for b in (buf, d_ref, d_prev):
            if b is not None:
                b.free()


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_kernel_equals_the_twin(gpu_engine, h, w):
    rng = np.random.default_rng(h * 100 + w)
    ref = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    prev = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    all_frames = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
    checked = 0
    for name, roi in rois(h, w).items():
        for n in (1, 2, 5):
            for tau in (0, 24, 255):
                for p in (None, prev):
                    for lead in (0, 1):                # lead = 1: the frames start h * w * 3 bytes into the buffer
                        frames = all_frames[:n]
                        got = on_device(gpu_engine, frames, ref, prev=p, roi=roi, tau=tau, lead=lead)
                        want = A.frame_activity_host(frames, ref, prev=p, roi=roi, tau=tau)
                        assert got.dtype == np.uint64 and got.shape == (n, 3)
                        assert np.array_equal(got, want), (name, n, tau, p is not None, lead, got, want)
                        checked += 1
    assert checked >= 3 * 3 * 3 * 2 * 2


def test_kernel_equals_the_twin_at_360x640(gpu_engine):
    """More than one band per frame (14 of 25 rows and one of 10), rows of 40 whole units."""
    rng = np.random.default_rng(7)
    h, w = 360, 640
    ref = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    prev = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
    for roi in (None, (1, 1, w - 1, h - 1), (3, 7, 610, 355)):
        got = on_device(gpu_engine, frames, ref, prev=prev, roi=roi, tau=24, lead=1)
        assert np.array_equal(got, A.frame_activity_host(frames, ref, prev=prev, roi=roi, tau=24)), roi


@pytest.mark.parametrize("h,w", [(5, 7), (33, 65)])
def test_known_contents(gpu_engine, h, w):
    ref = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    same = np.repeat(ref[None], 3, 0)
    assert not on_device(gpu_engine, same, ref, prev=ref, tau=0).any()                     # frame == ref: all zeros
    white, black = np.full((2, h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    a = on_device(gpu_engine, white, black, tau=254)
    assert a.tolist() == [[255 * h * w, h * w, 0], [255 * h * w, h * w, 0]]
    assert on_device(gpu_engine, white, black, tau=255)[:, 1].tolist() == [0, 0]
    assert on_device(gpu_engine, white, black, prev=black, tau=255)[:, 2].tolist() == [255 * h * w, 0]


def test_white_against_black_at_64x64(gpu_engine):
    white, black = np.full((1, 64, 64, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8)
    assert on_device(gpu_engine, white, black, tau=254).tolist() == [[255 * 4096, 4096, 0]]
    assert on_device(gpu_engine, white, black, tau=255).tolist() == [[255 * 4096, 0, 0]]


def test_a_difference_of_exactly_tau_is_not_counted(gpu_engine):
    tau, h, w = 24, 5, 7
    ref = np.full((h, w, 3), 100, np.uint8)
    frames = np.stack([np.full((h, w, 3), 100 + tau, np.uint8), np.full((h, w, 3), 100 + tau + 1, np.uint8)])
    assert on_device(gpu_engine, frames, ref, tau=tau)[:, 1].tolist() == [0, h * w]


def test_a_frame_alone_and_as_one_of_five_gives_the_same_numbers(gpu_engine):
    rng = np.random.default_rng(11)
    h, w = 33, 65
    ref = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
    five = on_device(gpu_engine, frames, ref, tau=24)
    for k in range(5):
        alone = on_device(gpu_engine, frames[k:k + 1], ref, prev=frames[k - 1] if k else None, tau=24)
        assert np.array_equal(alone[0], five[k]), k


def test_rows_of_out_beyond_n_are_untouched(gpu_engine):
    rng = np.random.default_rng(12)
    frames, ref = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    out = np.full((4, 3), 0xDEADBEEFDEADBEEF, np.uint64)
    got = on_device(gpu_engine, frames, ref, out=out)
    assert got is out and np.array_equal(out[:2], A.frame_activity_host(frames, ref)) and (out[2:] == 0xDEADBEEFDEADBEEF).all()


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=65536), dict(w=0), dict(h=16385), dict(roi=(0, 0, 8, 5)), dict(roi=(2, 1, 2, 3)), dict(tau=256),
                                dict(tau=-1)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals_carry_the_checks_text(gpu_engine, kw):
    a = dict(n=1, h=5, w=7, roi=None, tau=24)
    a.update(kw)
    why = E.frame_activity_check(**a)
    assert why is not None
    buf = gpu_engine.alloc(5 * 7 * 3 * 2)
    try:
        with pytest.raises(E.EngineError) as ex:
            gpu_engine.frame_activity(buf, a["n"], a["h"], a["w"], buf, roi=a["roi"], tau=a["tau"])
        assert str(ex.value) == why
        # ... and the library itself refuses, whoever calls it
        out = np.zeros((1, 3), np.uint64)
        roi = None if a["roi"] is None else np.array(a["roi"], np.int32)
        rc = gpu_engine.lib.pa_frame_activity(gpu_engine.handle, buf.ptr, a["n"], a["h"], a["w"], buf.ptr, None,
                                              roi.ctypes.data if roi is not None else None, a["tau"], out.ctypes.data)
        assert rc != 0 and gpu_engine.lib.pa_last_error(gpu_engine.handle).decode() == why
    finally:
        buf.free()


def test_short_buffers_are_refused(gpu_engine):
    buf, ref = gpu_engine.alloc(2 * 105), gpu_engine.alloc(104)
    try:
        with pytest.raises(E.EngineError, match="src holds"):
            gpu_engine.frame_activity(buf, 3, 5, 7, buf)
        with pytest.raises(E.EngineError, match="ref holds"):
            gpu_engine.frame_activity(buf, 2, 5, 7, ref)
    finally:
        buf.free()
        ref.free()


@pytest.mark.parametrize("n", [5, 6])
def test_frames_median_is_numpys(gpu_engine, n):
    frames = np.random.default_rng(n).integers(0, 256, (n, 7, 9, 3), dtype=np.uint8)
    src = gpu_engine.alloc(frames.nbytes).upload(frames)
    med = gpu_engine.frames_median(src, n, 7, 9)
    try:
        got = med.download(np.empty((7, 9, 3), np.uint8))
    finally:
        src.free()
        med.free()
    assert np.array_equal(got, np.median(frames, 0).astype(np.uint8))


@pytest.fixture(scope="module")
def scan_clip(tmp_path_factory):
    """20 frames of 32 x 48 that went through a .y4m file once, so that the file, a host clip and a device clip hold the same frames."""
    rng = np.random.default_rng(21)
    h, w = 32, 48
    raw = rng.integers(0, 256, (20, h, w, 3), dtype=np.uint8)
    path = tmp_path_factory.mktemp("scan") / "clip.y4m"
    with video.Y4mSink(path, w, h, fps=30) as sink:
        sink.write_host(video.bgr_to_yuv420_host(raw, sink.desc, sink.enc), 20)
    frames = np.stack([np.asarray(f) for f in video.get_video_frames_generator(str(path))])
    assert frames.shape == raw.shape
    ref = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return str(path), frames, ref


@pytest.mark.parametrize("kind", ["array", "device", "y4m", "device-repeated"])
def test_scan_equals_the_twin_over_batch_borders(gpu_engine, scan_clip, kind):
    path, frames, ref = scan_clip
    roi, want_frames = (5, 3, 40, 30), frames
    clip = None
    if kind == "array":
        source = video.ArrayClip(frames)
    elif kind == "device":
        source = clip = video.DeviceClip(gpu_engine, frames)
    elif kind == "device-repeated":                      # 6 stored frames shown 3 times: a batch's predecessor is not always the stored frame before it
        source = clip = video.DeviceClip(gpu_engine, frames[:6], repeat=3)
        want_frames = np.concatenate([frames[:6]] * 3)
    else:
        source = path
    try:
        act = A.scan(source, ref=ref, roi=roi, tau=24, batch=6 if kind == "device-repeated" else 8, engine=gpu_engine)
    finally:
        if clip is not None:
            clip.free()
    want = A.frame_activity_host(want_frames, ref, roi=roi, tau=24)
    assert len(act) == len(want_frames) and act.npix == 35 * 27
    assert np.array_equal(act.sad_ref, want[:, 0]) and np.array_equal(act.changed, want[:, 1])
    assert np.array_equal(act.sad_prev, want[:, 2]) and act.sad_prev[0] == 0 and act.sad_prev[8] > 0


def test_scan_without_ref_uses_the_median_of_sampled_frames(gpu_engine, scan_clip):
    path, frames, _ = scan_clip
    ref = A.reference_frame(video.ArrayClip(frames), samples=5, engine=gpu_engine)
    assert np.array_equal(ref, np.median(frames[[0, 4, 8, 12, 16]], 0).astype(np.uint8))
    act = A.scan(path, batch=8, engine=gpu_engine)                              # ref: the median of min(64, 20) = all frames
    want = A.frame_activity_host(frames, np.median(frames, 0).astype(np.uint8))
    assert np.array_equal(np.stack([act.sad_ref, act.changed, act.sad_prev], 1), want)
