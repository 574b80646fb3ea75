"""YUV 4:2:0 frame sources on the host: the integer conversion against its written specification (tests/yuv_ref.py) and the
hand-computed known answers, .y4m parsing, the video.py wiring, and a tracker over the CPU stand-in engine fed from a YuvClip.
Every comparison is exact: the outputs are integers."""
import json

import numpy as np
import pytest

from padel_analytics_amd import video
from tests import synth, yuv_ref as Y


def _desc(w, h, g, table="bt601_limited", coeffs=None):
    matrix, rng = table.split("_")
    return video.yuv_desc(w, h, g["layout"], matrix, rng, pitch=g["pitch"], pitch_c=g["pitch_c"], off_u=g["off_u"], off_v=g["off_v"],
                          frame_stride=g["frame_stride"], coeffs=coeffs)


def test_coefficient_tables_are_the_specification():
    assert video.YUV_COEFFS == Y.COEFFS
    assert list(video.YUV_COEFFS)[0] == "bt601_limited"


@pytest.mark.parametrize("ti", range(4))
def test_known_answers(ti):
    table = Y.TABLES[ti]
    for (yy, u, v), want in Y.KNOWN:
        assert Y.pixel(yy, u, v, Y.COEFFS[table]) == want[ti], (table, yy, u, v)
        for layout in ("nv12", "i420"):
            g = Y.geometry(4, 2, layout)
            raw = Y.pack(np.full((1, 2, 4), yy, np.uint8), np.full((1, 1, 2), u, np.uint8), np.full((1, 1, 2), v, np.uint8), g)
            got = video.yuv420_to_bgr_host(raw, 1, 2, 4, _desc(4, 2, g, table))
            assert got.shape == (1, 2, 4, 3) and (got.reshape(-1, 3) == np.array(want[ti])).all(), (table, layout, yy, u, v)
            assert (Y.convert(raw, 1, 2, 4, g, Y.COEFFS[table]).reshape(-1, 3) == np.array(want[ti])).all()


GEOMETRIES = {
    "tight": lambda w, h, nv12: {},
    "padded_pitch": lambda w, h, nv12: dict(pitch=w + 3, pitch_c=(w if nv12 else w // 2) + 5, off_u=h * (w + 3)),
    "padded_height": lambda w, h, nv12: dict(off_u=(h + 6) * w + 2),
    "frame_gap": lambda w, h, nv12: dict(frame_stride=w * h * 3 // 2 + 6),
}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_host_conversion_equals_the_reference_on_random_bytes(layout, geo):
    rng = np.random.default_rng(10 * list(GEOMETRIES).index(geo) + (layout == "nv12"))
    for (h, w) in ((2, 2), (6, 10), (16, 34)):
        g = Y.geometry(w, h, layout, **GEOMETRIES[geo](w, h, layout == "nv12"))
        n = 3
        P = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))]
        raw = Y.pack(*P, g, rng=rng, tail=3)
        for table in Y.TABLES:
            want = Y.convert(raw, n, h, w, g, Y.COEFFS[table])
            got = video.yuv420_to_bgr_host(raw, n, h, w, _desc(w, h, g, table))
            assert np.array_equal(got, want), (h, w, table)
        # full-range bytes through the limited table clamp both ways somewhere in this much data
        lim = Y.convert(raw, n, h, w, g, Y.COEFFS["bt601_limited"])
        if h * w >= 60:
            assert (lim == 0).any() and (lim == 255).any()


def test_host_conversion_refuses_bad_geometry():
    raw = np.zeros(64, np.uint8)
    for kw, word in ((dict(w=3, h=2), "even"), (dict(w=4, h=3), "even"), (dict(w=4, h=2, pitch=3), "pitch"),
                     (dict(w=4, h=2, frame_stride=8), "frame_stride")):
        w, h = kw.pop("w"), kw.pop("h")
        with pytest.raises(ValueError, match=word):
            video.yuv420_to_bgr_host(raw, 2, h, w, video.yuv_desc(w, h, **kw))
    with pytest.raises(ValueError, match="span"):
        video.yuv420_to_bgr_host(raw[:11], 1, 2, 4, video.yuv_desc(4, 2))


# ---------------------------------------------------------------------------------------------- .y4m
def _planes(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))]


def _ref_frames(P, table="bt601_limited"):
    n, h, w = P[0].shape
    g = Y.geometry(w, h, "i420")
    return Y.convert(Y.pack(*P, g), n, h, w, g, Y.COEFFS[table])


def test_y4m_round_trip(tmp_path):
    P = _planes(5, 6, 10)
    p = tmp_path / "a.y4m"
    Y.write_y4m(p, *P, header_tags="F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG")
    clip = video.YuvClip.from_y4m(p, on_device=False)
    assert (clip.w, clip.h, clip.fps, clip.n, clip.total_frames, clip.layout) == (10, 6, 25, 5, 5, "i420")
    assert clip.desc["y_off"] == 16 and clip.desc["cvr"] == Y.COEFFS["bt601_limited"][2]
    frames = list(clip.frames())
    assert [f.index for f in frames] == list(range(5)) and frames[0].shape == (6, 10, 3) and frames[0].clip is clip
    want = _ref_frames(P)
    for i, f in enumerate(frames):
        assert np.array_equal(np.asarray(f), want[i]) and np.array_equal(f.bgr(), want[i])
    assert np.array_equal(video.host_batch(frames[1:4]), want[1:4])
    assert np.array_equal(video.host_batch([frames[3], frames[0]]), want[[3, 0]])          # any order on the host
    assert video.device_batch(frames) is None                                              # on_device=False: host path


def test_y4m_header_variants(tmp_path):
    P = _planes(2, 4, 4, seed=1)
    p = tmp_path / "ntsc.y4m"
    Y.write_y4m(p, *P, header_tags="F30000:1001")                      # no C, no I: 4:2:0 progressive
    c = video.YuvClip.from_y4m(p, on_device=False)
    assert c.fps == 30 and c.n == 2 and np.array_equal(np.asarray(next(c.frames())), _ref_frames(P)[0])
    p = tmp_path / "full.y4m"
    Y.write_y4m(p, *P, header_tags="F30:1 I? C420mpeg2 XCOLORRANGE=FULL")
    c = video.YuvClip.from_y4m(p, on_device=False)
    assert c.desc["y_off"] == 0 and c.desc["cy"] == 1048576
    assert np.array_equal(np.asarray(list(c.frames())[1]), _ref_frames(P, "bt601_full")[1])
    c = video.YuvClip.from_y4m(p, matrix="bt709", range="limited", on_device=False)      # the caller's word beats the tag
    assert np.array_equal(np.asarray(next(c.frames())), _ref_frames(P, "bt709_limited")[0])


@pytest.mark.parametrize("tags,word", [("C422", "C422"), ("C444", "C444"), ("C420p10", "C420p10"), ("It C420", "It"), ("C420 Ib", "Ib"),
                                       ("Cmono", "Cmono")])
def test_y4m_refuses_what_it_cannot_convert(tmp_path, tags, word):
    p = tmp_path / "bad.y4m"
    Y.write_y4m(p, *_planes(1, 4, 4), header_tags=tags)
    with pytest.raises(ValueError, match=word):
        video.YuvClip.from_y4m(p, on_device=False)


def test_y4m_refuses_an_odd_width(tmp_path):
    p = tmp_path / "odd.y4m"
    p.write_bytes(b"YUV4MPEG2 W5 H4 F30:1 Ip C420\n" + b"FRAME\n" + bytes(5 * 4 * 3 // 2))
    with pytest.raises(ValueError, match="W5"):
        video.YuvClip.from_y4m(p, on_device=False)
    (tmp_path / "no.y4m").write_bytes(b"RIFF....")
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        video.YuvClip.from_y4m(tmp_path / "no.y4m")


def test_y4m_corrupted_marker_is_found_when_that_frame_is_yielded(tmp_path):
    P = _planes(3, 4, 6, seed=2)
    p = tmp_path / "c.y4m"
    head = Y.write_y4m(p, *P)
    b = bytearray(p.read_bytes())
    at = head + 2 * (6 + 36)
    assert b[at:at + 6] == b"FRAME\n"
    b[at + 2] = ord("x")
    p.write_bytes(bytes(b))
    clip = video.YuvClip.from_y4m(p, on_device=False)            # opening does not read the frames
    it = clip.frames()
    assert next(it).index == 0 and next(it).index == 1
    with pytest.raises(ValueError, match=f"byte offset {at}"):
        next(it)


def test_y4m_cut_mid_frame_yields_the_whole_frames(tmp_path):
    P = _planes(3, 4, 6, seed=3)
    p = tmp_path / "cut.y4m"
    Y.write_y4m(p, *P)
    p.write_bytes(p.read_bytes()[:-10])
    clip = video.YuvClip.from_y4m(p, on_device=False)
    assert clip.total_frames == 2 and len(list(clip.frames())) == 2
    assert np.array_equal(video.host_batch(list(clip.frames())), _ref_frames(P)[:2])
    Y.write_y4m(p, *P, trailing=b"FRAME\n" + bytes(5))
    assert video.YuvClip.from_y4m(p, on_device=False).total_frames == 3


def test_paths_ending_in_y4m_open_through_the_two_calls(tmp_path):
    P = _planes(7, 4, 8, seed=4)
    p = str(tmp_path / "x.y4m")
    Y.write_y4m(p, *P, header_tags="F50:1 C420")
    info = video.VideoInfo.from_video_path(p)
    assert (info.width, info.height, info.fps, info.total_frames) == (8, 4, 50, 7) and info.resolution_wh == (8, 4)
    want = _ref_frames(P)
    got = list(video.get_video_frames_generator(p, start=1, end=6, stride=2))
    assert [f.index for f in got] == [1, 3, 5]
    for f in got:
        assert isinstance(f, video.YuvFrame) and np.array_equal(np.asarray(f), want[f.index])
    assert len(list(video.get_video_frames_generator(p))) == 7
    assert len(list(video.get_video_frames_generator(p, end=100))) == 7
    # the clip objects themselves are sources too, with repeat
    g = Y.geometry(8, 4, "nv12")
    raw = Y.pack(*P, g)
    clip = video.YuvClip(raw, 8, 4, repeat=2, fps=24, on_device=False)
    assert video.VideoInfo.from_video_path(clip).total_frames == 14 and video.VideoInfo.from_video_path(clip).fps == 24
    assert [f.index for f in video.get_video_frames_generator(clip, start=5, end=9)] == [5, 6, 0, 1]
    assert np.array_equal(np.asarray(list(clip.frames())[8]), Y.convert(raw, 7, 4, 8, g, Y.COEFFS["bt601_limited"])[1])
    # a file that is rewritten is opened afresh
    Y.write_y4m(p, *_planes(2, 4, 8, seed=5))
    assert video.VideoInfo.from_video_path(p).total_frames == 2


def test_clip_geometry_header_and_count():
    P = _planes(3, 4, 6, seed=6)
    g = Y.geometry(6, 4, "nv12", pitch=9, pitch_c=7, off_u=4 * 9 + 5, frame_stride=4 * 9 + 5 + 2 * 7 + 6)
    raw = Y.pack(*P, g, rng=np.random.default_rng(0), lead=11, tail=2)
    clip = video.YuvClip(raw, 6, 4, pitch=9, pitch_c=7, off_u=g["off_u"], frame_stride=g["frame_stride"], header_bytes=11, on_device=False)
    assert clip.n == 3
    want = Y.convert(raw[11:], 3, 4, 6, g, Y.COEFFS["bt601_limited"])
    assert np.array_equal(video.host_batch(list(clip.frames())), want)
    with pytest.raises(ValueError, match="frame"):
        video.YuvClip(raw, 6, 4, pitch=9, pitch_c=7, off_u=g["off_u"], frame_stride=g["frame_stride"], header_bytes=11, n=4)
    with pytest.raises(ValueError, match="layout"):
        video.YuvClip(raw, 6, 4, layout="yuyv")


def test_device_batch_refuses_a_non_contiguous_yuv_batch():
    P = _planes(6, 4, 4, seed=7)
    raw = Y.pack(*P, Y.geometry(4, 4, "nv12"))
    clip, other = video.YuvClip(raw, 4, 4), video.YuvClip(raw, 4, 4)          # on_device=True; no engine is touched before the refusal
    f = list(clip.frames())
    for bad in ([f[0], f[2]], [f[1], f[0]], [f[0], next(other.frames())], [f[0], np.zeros((4, 4, 3), np.uint8)]):
        with pytest.raises(ValueError, match="contiguous"):
            video.device_batch(bad)


# ---------------------------------------------------------------------------------------------- a tracker over the stand-in engine
@pytest.fixture
def fake_engine(monkeypatch):
    from padel_analytics_amd import engine as E
    from tests import fake_engine as F
    eng = F.FakeEngine(0)
    monkeypatch.setattr(E, "Engine", F.FakeEngine)
    monkeypatch.setattr(E, "Model", F.FakeModel)
    monkeypatch.setattr(E, "DeviceBuffer", F.FakeBuffer)
    monkeypatch.setattr(E, "default_engine", lambda *a, **k: eng)
    monkeypatch.setattr(F.FakeModel, "STEP_SECONDS", 0.0)
    return eng


@pytest.mark.parametrize("fanout", [False, True])
def test_player_tracker_over_the_stand_in_engine_yuv_equals_bgr(fake_engine, tmp_path, fanout):
    from padel_analytics_amd import checkpoint, detections as D, yolo_arch
    from padel_analytics_amd.trackers import PlayerTracker, TrackingRunner
    h, w, n = 72, 128, 11
    raw, g = Y.bgr_to_yuv420(synth.synthetic_frames(n, h, w, seed=21), "nv12", pitch=w + 3, pitch_c=w + 1, off_u=(h + 2) * (w + 3))
    want_frames = Y.convert(raw, n, h, w, g, Y.COEFFS["bt601_limited"])
    checkpoint.save_checkpoint(tmp_path / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80,
                               None, "n", {0: "person"})
    zone = D.PolygonZone(np.array([[4, 4], [124, 4], [124, 68], [4, 68]]), frame_resolution_wh=(w, h))

    def run(source):
        t = PlayerTracker(str(tmp_path / "players.pt"), zone, batch_size=4)       # 11 frames: 4 + 4 + 3
        TrackingRunner([t], source, tmp_path / "out.mp4", fanout=fanout).run()
        assert len(t) == n
        return json.dumps([o.serialize() for o in t.results])

    want = run(video.ArrayClip(want_frames))
    clip = video.YuvClip(raw, w, h, pitch=g["pitch"], pitch_c=g["pitch_c"], off_u=g["off_u"], on_device=False)
    assert run(clip) == want
    assert want.count("[") > n                                                    # (there are detections to compare)
    # the stand-in's detections are a function of the pixels: other frames give other results
    assert run(video.ArrayClip(want_frames[::-1].copy())) != want
