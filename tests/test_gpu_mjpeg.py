"""``Engine.jpeg_encode`` (csrc/jpeg_encode.hip) against its numpy twin ``mjpeg.encode_host``: the same bytes and offsets for every
size, layout and content of tests/mjpeg_cases.py, whatever the bytes between the planes hold, in one batch or one call per frame;
a destination that is too small gets nothing but the size it needs; what ``pa_jpeg_check`` refuses, the engine refuses."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, video
from tests import mjpeg_cases as MC

pytestmark = pytest.mark.gpu


def encode(eng, raw, n, h, w, desc, quality, **kw):
    buf = eng.alloc(raw.size)
    try:
        buf.upload(raw)
        data, offsets = eng.jpeg_encode(buf, n, h, w, desc, quality, **kw)
        return data.copy(), offsets
    finally:
        buf.free()


@pytest.mark.parametrize("content", list(MC.CONTENTS))
@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("w,h", MC.SIZES)
def test_the_kernel_writes_the_twins_bytes(gpu_engine, w, h, layout, content):
    want, want_off = MC.expected(content, w, h, layout, 3)
    for sentinel in (0x00, 0xff):                      # the pitch padding and the gaps: the result must not depend on them
        raw, d = MC.raw_frames(content, w, h, layout, 3, sentinel)
        data, offsets = encode(gpu_engine, raw, 3, h, w, d, MC.CONTENTS[content])
        assert np.array_equal(offsets, want_off), (sentinel, offsets, want_off)
        assert np.array_equal(data, want), sentinel


@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("w,h", [(34, 18), (16, 144)])
def test_a_batch_of_three_is_three_batches_of_one(gpu_engine, w, h, layout):
    raw, d = MC.raw_frames("ramp", w, h, layout, 3, 0x3c)
    want, want_off = MC.expected("ramp", w, h, layout, 3)
    for i in range(3):
        one = raw[i * d["frame_stride"]:][:video.yuv_span(1, h, w, d)].copy()
        data, offsets = encode(gpu_engine, one, 1, h, w, d, 90)
        assert offsets.tolist() == [0, want_off[i + 1] - want_off[i]]
        assert np.array_equal(data, want[want_off[i]:want_off[i + 1]])


def test_a_destination_that_is_too_small_gets_the_size_and_nothing_else(gpu_engine):
    w, h = 34, 18
    raw, d = MC.raw_frames("noise_q100", w, h, "i420", 3, 0)
    want, want_off = MC.expected("noise_q100", w, h, "i420", 3)
    for cap in (0, 1, int(want_off[1]), int(want_off[-1]) - 1):
        out = np.full(max(cap, 1), 0xee, np.uint8)[:cap]
        with pytest.raises(E.EngineError, match="dst_host holds") as err:
            encode(gpu_engine, raw, 3, h, w, d, 100, out=out)
        assert err.value.needed == want_off[-1]
        assert (out == 0xee).all()
    out = np.full(int(want_off[-1]) + 3, 0xee, np.uint8)   # exactly enough and a little more: written, the rest untouched
    data, offsets = encode(gpu_engine, raw, 3, h, w, d, 100, out=out)
    assert np.array_equal(data, want) and np.array_equal(offsets, want_off) and (out[int(want_off[-1]):] == 0xee).all()


REFUSALS = {
    "odd width": dict(w=15), "odd height": dict(h=17), "too small": dict(w=0), "no frames": dict(n=0),
    "quality 0": dict(quality=0), "quality 101": dict(quality=101), "too wide": dict(w=E.JPEG_MAX_WIDTH + 2),
    "pitch_y": dict(desc=dict(pitch_y=15)), "pitch_c": dict(desc=dict(pitch_c=7)),
    "nv12 off_v": dict(layout="nv12", desc=dict(off_v=400)), "frame_stride": dict(desc=dict(frame_stride=100)),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_what_the_check_refuses_the_engine_refuses(gpu_engine, name):
    r = REFUSALS[name]
    n, h, w, quality = r.get("n", 2), r.get("h", 16), r.get("w", 16), r.get("quality", 90)
    d = video.yuv_desc(max(w, 2) & ~1, max(h, 2) & ~1, r.get("layout", "i420"))
    d.update(r.get("desc", {}))
    why = E.jpeg_check(n, h, w, d, quality)
    assert why is not None
    buf = gpu_engine.alloc(1 << 18)
    try:
        with pytest.raises(E.EngineError) as err:
            gpu_engine.jpeg_encode(buf, n, h, w, d, quality)
        assert str(err.value) == why
    finally:
        buf.free()
