"""GPU: the YUV 4:2:0 -> BGR kernel (csrc/yuv_convert.hip) byte for byte against the written specification (tests/yuv_ref.py),
on both of its paths, and the trackers fed from YUV clips — bit-identical to feeding them the converted frames.
Every comparison is exact: the outputs are integers."""
import contextlib
import json
import mmap

import numpy as np
import pytest

from padel_analytics_amd import checkpoint, detections as D, engine as E, video
from tests import synth, yuv_ref as Y

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (2, 6), (4, 4), (6, 10), (16, 34), (18, 64), (2, 130)]      # widths that are / are not multiples of 4, one block, a row beyond a workgroup's 128 pixels
MADE_UP = (7, 1100000, 1500000, -300000, -700000, 2000000)                   # no named table: the kernel reads the descriptor
COEFF_SETS = dict(Y.COEFFS, made_up=MADE_UP)
GUARD = 64                                                                   # bytes of 0xA5 before and after the destination


def _odd(x):
    return x + 1 if x % 2 == 0 else x + 2


# name -> (geometry keywords, bytes the source pointer is moved by)
def _geo(name, w, h, nv12):
    crow = w if nv12 else w // 2
    tight = w * h * 3 // 2
    return {
        "tight": ({}, 0),
        "odd_pitches": (dict(pitch=w + 3, pitch_c=_odd(crow), off_u=h * (w + 3)), 0),
        "aligned_pitches": (dict(pitch=w + 8, pitch_c=crow + 4, off_u=h * (w + 8)), 0),
        "padded_height": (dict(off_u=(h + 6) * w), 0),
        "frame_gap_6": (dict(frame_stride=tight + 6), 0),
        "src_plus_1": ({}, 1),
    }[name]


GEOS = ["tight", "odd_pitches", "aligned_pitches", "padded_height", "frame_gap_6", "src_plus_1"]


def _expect_vector(w, n, g, src_ptr, dst_ptr):
    """The launcher's rule, restated: dword loads / stores only where every address of the launch is aligned for them."""
    if w % 4 or src_ptr % 4 or dst_ptr % 4 or g["pitch"] % 4 or (n > 1 and g["frame_stride"] % 4):
        return False
    if g["layout"] == "nv12":
        return g["off_u"] % 4 == 0 and g["pitch_c"] % 4 == 0
    return g["off_u"] % 2 == 0 and g["off_v"] % 2 == 0 and g["pitch_c"] % 2 == 0


def _desc(w, h, g, coeffs):
    return video.yuv_desc(w, h, g["layout"], pitch=g["pitch"], pitch_c=g["pitch_c"], off_u=g["off_u"], off_v=g["off_v"],
                          frame_stride=g["frame_stride"], coeffs=coeffs)


def _convert(eng, raw, lead, n, h, w, g, coeffs, host_src=False, dst_shift=0):
    """-> (BGR frames the engine wrote, path it took).  The destination sits inside a larger buffer of 0xA5 whose guard bytes must
    come back untouched."""
    out_bytes = n * h * w * 3
    dst = eng.alloc(GUARD + dst_shift + out_bytes + GUARD)
    src = None
    try:
        dst.upload(np.full(dst.nbytes, 0xA5, np.uint8))
        if host_src:
            arg = raw[lead:]
        else:
            src = eng.alloc(raw.size).upload(raw)
            arg = src.view(lead, raw.size - lead)
        eng.yuv420_to_bgr(arg, n, h, w, _desc(w, h, g, coeffs), dst.view(GUARD + dst_shift, out_bytes))
        path = eng.yuv_last_path()
        if not host_src:
            assert (path == E.YUV_PATH_VECTOR) == _expect_vector(w, n, g, src.ptr + lead, dst.ptr + GUARD + dst_shift), (path, w, n, g)
        got = dst.download(np.empty(dst.nbytes, np.uint8))
        assert (got[:GUARD + dst_shift] == 0xA5).all() and (got[GUARD + dst_shift + out_bytes:] == 0xA5).all(), "guard bytes were written"
        return got[GUARD + dst_shift:GUARD + dst_shift + out_bytes].reshape(n, h, w, 3), path
    finally:
        dst.free()
        if src is not None:
            src.free()


def _known_planes(n, h, w, shift):
    """Every 2 x 2 block is one constant (Y, U, V) of the known-answer table, block k of frame i taking triple (k + i + shift) % 10."""
    k = (np.arange((h // 2) * (w // 2)).reshape(h // 2, w // 2)[None] + np.arange(n)[:, None, None] + shift) % len(Y.KNOWN)
    trip = np.array([t for t, _ in Y.KNOWN], np.uint8)
    return np.kron(trip[k, 0], np.ones((2, 2), np.uint8)), trip[k, 1], trip[k, 2], k


@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_kernel_equals_the_specification(gpu_engine, layout, geo):
    rng = np.random.default_rng(100 + 10 * GEOS.index(geo) + (layout == "nv12"))
    paths = set()
    for (h, w) in SIZES:
        for n in (1, 3):
            kw, lead = _geo(geo, w, h, layout == "nv12")
            g = Y.geometry(w, h, layout, **kw)
            # random bytes over 0..255 in all three planes (the out-of-nominal values clamp both ways), random bytes in every gap
            P = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))]
            raw = Y.pack(*P, g, rng=rng, lead=lead, tail=5)
            for name, coeffs in COEFF_SETS.items():
                got, path = _convert(gpu_engine, raw, lead, n, h, w, g, coeffs)
                paths.add(path)
                assert np.array_equal(got, Y.convert(raw[lead:], n, h, w, g, coeffs)), (h, w, n, name, path)
            # the ten constant triples, against the table itself and not only the oracle
            Yp, Up, Vp, k = _known_planes(n, h, w, shift=h + w)
            raw = Y.pack(Yp, Up, Vp, g, rng=rng, lead=lead, tail=5)
            for ti, table in enumerate(Y.TABLES):
                got, path = _convert(gpu_engine, raw, lead, n, h, w, g, Y.COEFFS[table])
                want = np.array([ans[ti] for _, ans in Y.KNOWN], np.uint8)[k]                      # (n, h/2, w/2, 3)
                want = want.repeat(2, axis=1).repeat(2, axis=2)
                assert np.array_equal(got, want), (h, w, n, table, path)
                assert np.array_equal(got, Y.convert(raw[lead:], n, h, w, g, Y.COEFFS[table]))
    # what each geometry is here to exercise (per case, _convert has already held the launcher to its rule)
    if geo in ("odd_pitches", "src_plus_1"):
        assert paths == {E.YUV_PATH_BYTE}
    else:
        assert paths == {E.YUV_PATH_VECTOR, E.YUV_PATH_BYTE}          # widths 4, 64: dwords; widths 2, 6, 10, 34, 130: bytes


def test_both_paths_ran_and_a_misaligned_destination_takes_bytes(gpu_engine):
    rng = np.random.default_rng(5)
    h, w, n = 18, 64, 3
    for layout in ("nv12", "i420"):
        g = Y.geometry(w, h, layout)
        raw = Y.pack(*[rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))], g)
        want = Y.convert(raw, n, h, w, g, Y.COEFFS["bt709_limited"])
        got, path = _convert(gpu_engine, raw, 0, n, h, w, g, Y.COEFFS["bt709_limited"])
        assert path == E.YUV_PATH_VECTOR and np.array_equal(got, want)
        got, path = _convert(gpu_engine, raw, 0, n, h, w, g, Y.COEFFS["bt709_limited"], dst_shift=2)
        assert path == E.YUV_PATH_BYTE and np.array_equal(got, want)
        g6 = Y.geometry(w, h, layout, frame_stride=g["frame_stride"] + 6)           # every second frame starts misaligned
        P = [np.stack([Y.planes(raw, i, h, w, g)[k] for i in range(n)]).astype(np.uint8) for k in range(3)]
        raw6 = Y.pack(*P, g6, rng=rng)
        got, path = _convert(gpu_engine, raw6, 0, n, h, w, g6, Y.COEFFS["bt709_limited"])
        assert path == E.YUV_PATH_BYTE and np.array_equal(got, want)
        got, path = _convert(gpu_engine, raw6, 0, 1, h, w, g6, Y.COEFFS["bt709_limited"])   # one frame: the stride does not matter
        assert path == E.YUV_PATH_VECTOR and np.array_equal(got, want[:1])


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_host_source_equals_device_source(gpu_engine, layout):
    rng = np.random.default_rng(9)
    for (h, w, kw) in ((16, 34, dict(pitch=37)), (18, 64, {}), (6, 10, dict(frame_stride=10 * 6 * 3 // 2 + 6))):
        if "pitch" in kw:
            kw = dict(kw, off_u=h * kw["pitch"])
        g = Y.geometry(w, h, layout, **kw)
        n = 3
        raw = Y.pack(*[rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))], g, rng=rng,
                     lead=1)
        dev, _ = _convert(gpu_engine, raw, 1, n, h, w, g, Y.COEFFS["bt601_limited"])
        host, _ = _convert(gpu_engine, raw, 1, n, h, w, g, Y.COEFFS["bt601_limited"], host_src=True)
        assert np.array_equal(dev, host) and np.array_equal(host, Y.convert(raw[1:], n, h, w, g, Y.COEFFS["bt601_limited"]))
    # a larger host source after a smaller one: the engine's raw staging grows
    g = Y.geometry(130, 18, layout)
    raw = Y.pack(*[rng.integers(0, 256, s, dtype=np.uint8) for s in ((4, 18, 130), (4, 9, 65), (4, 9, 65))], g)
    host, _ = _convert(gpu_engine, raw, 0, 4, 18, 130, g, Y.COEFFS["bt601_full"], host_src=True)
    assert np.array_equal(host, Y.convert(raw, 4, 18, 130, g, Y.COEFFS["bt601_full"]))


def test_refusals_launch_nothing(gpu_engine):
    eng = gpu_engine
    src = eng.alloc(4096).upload(np.arange(4096, dtype=np.uint8))
    dst = eng.alloc(4096).upload(np.full(4096, 0xA5, np.uint8))
    good = video.yuv_desc(8, 4)
    eng.yuv420_to_bgr(src, 2, 4, 8, good, dst.view(0, 2 * 4 * 8 * 3))
    before = dst.download(np.empty(4096, np.uint8)).copy()
    assert (before[:192] != 0xA5).any() and (before[192:] == 0xA5).all()
    dst.upload(np.full(4096, 0xA5, np.uint8))
    cases = [
        (2, 4, 7, video.yuv_desc(8, 4), "even"),                                               # odd w
        (2, 3, 8, video.yuv_desc(8, 4), "even"),                                               # odd h
        (2, 4, 0, video.yuv_desc(8, 4), "even"),
        (0, 4, 8, video.yuv_desc(8, 4), "n = 0"),
        (2, 4, 8, video.yuv_desc(8, 4, pitch=7, off_u=32), "pitch_y"),                         # a pitch shorter than its row
        (2, 4, 8, video.yuv_desc(8, 4, pitch_c=6), "pitch_c"),
        (2, 4, 8, video.yuv_desc(8, 4, "i420", pitch_c=3), "pitch_c"),
        (2, 4, 8, video.yuv_desc(8, 4, frame_stride=47), "frame_stride"),                      # the planes reach into the next frame
        (2, 4, 8, video.yuv_desc(8, 4, "i420", frame_stride=40), "frame_stride"),
        (2, 4, 8, video.yuv_desc(8, 4, off_v=40), "off_v"),                                    # NV12: V sits one byte behind U
        (2, 4, 8, video.yuv_desc(8, 4, coeffs=(16, 1 << 24, 0, 0, 0, 0)), "int32"),
    ]
    for n, h, w, d, word in cases:
        with pytest.raises(E.EngineError, match=word):
            eng.yuv420_to_bgr(src, n, h, w, d, dst)
    with pytest.raises(E.EngineError, match="src holds"):                                       # a source shorter than its description
        eng.yuv420_to_bgr(src.view(0, 95), 2, 4, 8, good, dst)
    with pytest.raises(E.EngineError, match="dst holds"):
        eng.yuv420_to_bgr(src, 2, 4, 8, good, dst.view(0, 191))
    assert (dst.download(np.empty(4096, np.uint8)) == 0xA5).all()                               # nothing was launched
    src.free()
    dst.free()


# ---------------------------------------------------------------------------------------------- clips and staging
def _anon_bytes(a: np.ndarray) -> np.ndarray:
    """A copy of ``a`` in an anonymous private mapping: memory that can be page-locked and unlocked without touching malloc's heap."""
    mm = mmap.mmap(-1, max(a.size, 1), flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, prot=mmap.PROT_READ | mmap.PROT_WRITE)
    out = np.frombuffer(mm, np.uint8)[:a.size]
    out[:] = a
    return out


@contextlib.contextmanager
def _counting(eng):
    """Frames per conversion the engine wrapper is asked for, in call order."""
    calls = []
    prev, real = eng.__dict__.get("yuv420_to_bgr"), eng.yuv420_to_bgr
    eng.yuv420_to_bgr = lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1]
    try:
        yield calls
    finally:
        if prev is None:
            del eng.yuv420_to_bgr
        else:
            eng.yuv420_to_bgr = prev


def _download(dev):
    buf, n, h, w = dev
    return buf.download(np.empty((n, h, w, 3), np.uint8))


def test_staging_follows_the_bytes(gpu_engine):
    """The clip's BGR staging remembers the range it holds; free() + a new clip, invalidate() after the bytes were rewritten and
    DeviceYuvClip.upload all make the next batch follow the new bytes."""
    h, w, n = 18, 64, 6
    A, gA = Y.bgr_to_yuv420(synth.synthetic_frames(n, h, w, seed=1), "nv12")
    B, _ = Y.bgr_to_yuv420(synth.synthetic_frames(n, h, w, seed=2), "nv12")
    refA, refB = (Y.convert(r, n, h, w, gA, Y.COEFFS["bt601_limited"]) for r in (A, B))
    assert not np.array_equal(refA, refB)
    with _counting(gpu_engine) as calls:
        clip = video.YuvClip(A.copy(), w, h, engine=gpu_engine)
        f = list(clip.frames())
        assert np.array_equal(_download(video.device_batch(f[:4])), refA[:4]) and calls == [4]
        assert np.array_equal(_download(video.device_batch(f[:4])), refA[:4]) and calls == [4]          # held: nothing converted
        assert np.array_equal(_download(video.device_batch(f[1:3])), refA[1:3]) and calls == [4]        # a part of what is held
        assert np.array_equal(_download(video.device_batch(f[2:6])), refA[2:6]) and calls == [4, 4]
        assert np.array_equal(_download(video.device_batch(f)), refA) and calls == [4, 4, 6]            # the staging grew
        clip.data[:] = B                                                                                   # the ring came round
        clip.invalidate()
        assert np.array_equal(_download(video.device_batch(f)), refB) and calls == [4, 4, 6, 6]
        clip.free()
        assert clip._bgr is None
        clip2 = video.YuvClip(B.copy(), w, h, engine=gpu_engine)
        assert np.array_equal(_download(video.device_batch(list(clip2.frames())[:4])), refB[:4])
        clip2.free()
        dclip = video.DeviceYuvClip(gpu_engine, A, w, h)
        df = list(dclip.frames())
        assert np.array_equal(_download(video.device_batch(df)), refA) and np.array_equal(np.asarray(df[3]), refA[3])
        dclip.upload(B)
        assert np.array_equal(_download(video.device_batch(df)), refB)
        assert np.array_equal(video.host_batch(df[1:5]), refB[1:5])
        with pytest.raises(ValueError, match="contiguous"):
            video.device_batch([df[0], df[2]])
        dclip.free()


# ---------------------------------------------------------------------------------------------- end to end, bitwise
H, W, N = 360, 640, 13


class _Sources:
    """One clip of 13 synthetic frames as the reference run sees it (an ArrayClip of the specification's BGR) and as the three YUV
    sources under test; ``calls`` counts the conversions the engine was asked for."""

    def __init__(self, eng, tmp):
        bgr = synth.synthetic_frames(N, H, W, seed=15)
        self.eng = eng
        nv12, g = Y.bgr_to_yuv420(bgr, "nv12", pitch=W + 64, pitch_c=W + 64, off_u=(H + 8) * (W + 64))     # a decoder surface: pitch, padded height
        self.ref = video.ArrayClip(Y.convert(nv12, N, H, W, g, Y.COEFFS["bt601_limited"]))
        self.pinned = _anon_bytes(nv12)
        kw = dict(pitch=g["pitch"], pitch_c=g["pitch_c"], off_u=g["off_u"])
        self.host = video.YuvClip(self.pinned, W, H, engine=eng, **kw).pin(eng)
        self.device = video.DeviceYuvClip(eng, nv12, W, H, **kw)
        self.y4m = str(tmp / "clip.y4m")
        Yp, Up, Vp = Y.planes_of_bgr(bgr)
        Y.write_y4m(self.y4m, Yp, Up, Vp)
        g4 = Y.geometry(W, H, "i420")
        assert np.array_equal(Y.convert(Y.pack(Yp, Up, Vp, g4), N, H, W, g4, Y.COEFFS["bt601_limited"]), self.ref.array)   # both encodings hold the same samples
        self.under_test = {"host_nv12_pinned": self.host, "y4m_path": self.y4m, "device_nv12": self.device}

    def close(self):
        self.host.unpin()
        self.host.free()
        self.device.free()
        video._open_y4m(self.y4m).free()


@pytest.fixture(scope="module")
def sources(gpu_engine, tmp_path_factory):
    s = _Sources(gpu_engine, tmp_path_factory.mktemp("yuv"))
    yield s
    s.close()


def _run(trackers, source, tmp, **kw):
    from padel_analytics_amd.trackers import TrackingRunner
    r = TrackingRunner(trackers, source, tmp / "out.mp4", **kw)
    r.restart()
    r.run()
    out = {str(t): json.dumps([o.serialize() for o in t.results]) for t in trackers}
    for t in trackers:
        assert len(t) == N, (str(t), len(t))
    return out


def _players(tmp):
    from padel_analytics_amd import yolo_arch
    from padel_analytics_amd.trackers import PlayerTracker
    checkpoint.save_checkpoint(tmp / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80, None, "n",
                               {0: "person"})
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(W, H))
    return PlayerTracker(str(tmp / "players.pt"), zone, batch_size=5)            # 13 frames: 5 + 5 + 3, submitted ahead of collection


def _ball(tmp):
    from oracle import tracknet_ref as tr
    from padel_analytics_amd.trackers import BallTracker
    checkpoint.save_checkpoint(tmp / "tracknet.pt", tr.synth_tracknet_state_dict(9), "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    # median over the first 6 frames (one conversion), then feeds of 5: the first lies inside what the staging holds, the others convert over it
    return BallTracker(str(tmp / "tracknet.pt"), None, batch_size=5, median_max_sample_num=6)


def _court(tmp):
    from padel_analytics_amd.trackers import KeypointsTracker
    from tests import resnet_synth as S
    S.save_plain(tmp / "court_resnet50.pt", S.clip_and_state_dict()[1])
    return KeypointsTracker(str(tmp / "court_resnet50.pt"), 5)


@pytest.mark.parametrize("which", ["players", "ball", "court"])
def test_tracker_results_from_yuv_sources_are_bit_identical(gpu_engine, sources, tmp_path, which):
    t = {"players": _players, "ball": _ball, "court": _court}[which](tmp_path)
    try:
        want = _run([t], sources.ref, tmp_path)
        if which == "players":
            assert sum(len(f) for f in json.loads(want[str(t)])) > 0, "the reference run found no player to compare"
        for name, src in sources.under_test.items():
            with _counting(gpu_engine) as calls:
                got = _run([t], src, tmp_path)
            assert got == want, (which, name)
            # the frames did come through the kernel: three batches of 5 + 5 + 3 (the ball tracker: its 6-frame median first, and
            # the feed of frames 0..4 lies inside what the staging holds by then)
            # (a prefix: a tracker that left the fp16 range runs its clip again on the full-range kernels)
            assert calls[:3] == ([6, 5, 3] if which == "ball" else [5, 5, 3]), (which, name, calls)
    finally:
        m = getattr(t, "model", None)
        if m is not None and hasattr(m, "close"):
            m.close()


def test_fanout_over_a_yuv_clip_converts_each_batch_once(gpu_engine, sources, tmp_path):
    trackers = [_players(tmp_path), _ball(tmp_path), _court(tmp_path)]
    try:
        want = _run(trackers, sources.ref, tmp_path, fanout=True, engine=gpu_engine)
        seq = _run(trackers, sources.ref, tmp_path)
        assert want == seq
        for name, src in sources.under_test.items():
            clip = src if not isinstance(src, str) else video._open_y4m(src)
            clip.invalidate()
            asked = []
            real = clip.device_view
            clip.device_view = lambda first, count: (asked.append((first, count)), real(first, count))[1]
            try:
                with _counting(gpu_engine) as calls:
                    got = _run(trackers, src, tmp_path, fanout=True, engine=gpu_engine)
            finally:
                del clip.device_view
            assert got == want, name
            # the fan-out pass: the runner and the players tracker both ask for each of the 3 batches, the engine converts 3 times;
            # then the two stream trackers' own passes: the court regressor's 3 batches, the ball tracker's median (6 frames) and
            # 3 feeds, of which the first lies inside the median's range: 13 requests, 9 conversions (more only if a tracker left
            # the fp16 range and ran again)
            assert asked[:6] == [(0, 5), (0, 5), (5, 5), (5, 5), (10, 3), (10, 3)], (name, asked)
            assert calls[:3] == [5, 5, 3] and len(calls) >= 9 and len(asked) >= 13, (name, asked, calls)
    finally:
        for t in trackers:
            m = getattr(t, "model", None)
            if m is not None and hasattr(m, "close"):
                m.close()
