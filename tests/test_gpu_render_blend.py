"""``PA_MARK_BLEND`` in csrc/render.hip on the GPU against ``render.render_host``, bit for bit — the one mark that reads the pixel it
writes.  Ramp frames whose channels take every value 0..255; 36 x 132 frames (two tiles across with a partial one, three down with
a partial one, vector path) and 36 x 130 (byte path, a 2-pixel tail), the path asserted through ``Engine.render_last_path``; BGR (also
in place), NV12 and I420 output; blends across the tile borders at x = 127 / 128 and y = 15 / 16, partly and wholly outside the
frame; stacked blends and blends under / over opaque marks in both orders; a blend and a fill over the same pixels on either side
of the boundary between two passes of the kernel's LDS list (256 marks a pass).  ``gpu_render`` checks the sentinel bytes around
the destination and that the source is not written."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, render as R, video
from tests.test_gpu_render import ENC, frames_of, gpu_render, host_render

pytestmark = pytest.mark.gpu

H = 36
OUTPUTS = [("bgr", None), ("nv12", "nv12"), ("i420", "i420")]


def ramp(n, h, w):
    """Frames whose three channels each take every value 0..255, differently."""
    i = np.arange(n * h * w, dtype=np.int64).reshape(n, h, w)
    f = np.stack([i & 255, (3 * i + 85) & 255, 255 - ((5 * i + 11) & 255)], -1).astype(np.uint8)
    assert all(len(np.unique(f[k, ..., c])) == 256 for k in range(n) for c in range(3))
    return f


def single_blends(w):
    white, col = 0xffffff, 0x2060c0
    return [R.blend(120, 10, 131, 20, white, 1), R.blend(125, 13, 129, 17, col, 128), R.blend(100, 14, 128, 16, 0x000000, 255),   # across x = 127 / 128, y = 15 / 16
            R.blend(-20, -9, 12, 7, col, 128), R.blend(w - 5, H - 3, w + 40, H + 40, white, 255), R.blend(60, 30, 70, 200, 0x00ff00, 1),  # partly outside
            R.blend(2, 20, 50, 34, white, 128), R.blend(0, 0, 0, 0, 0x0000ff, 200)]


OUTSIDE = [R.blend(-50, -50, -1, -1, 0xffffff, 128), R.blend(200, 0, 300, 35, 0xffffff, 255), R.blend(0, H, 131, H + 9, 0x123456, 1),
           R.blend(-8192, 40, 8191, 8191, 0, 128)]


def stacked(order):
    a, b = R.blend(90, 5, 131, 25, 0x10e020, 200), R.blend(110, 12, 140, 40, 0xf01080, 60)
    return [a, b] if order == "ab" else [b, a]


def with_disc(order):
    panel, disc = R.blend(100, 2, 131, 33, 0xffffff, 128), R.disc(127, 15, 9, 0x0000ff)
    return [panel, disc] if order == "blend first" else [disc, panel]


def across_passes(order):
    """300 marks: index 10 and index 290 cover the same pixels — one pass of the LDS list holds 256, so they meet in different passes."""
    rng = np.random.default_rng(21)
    many = [R.disc(int(rng.integers(0, 132)), int(rng.integers(0, H)), int(rng.integers(1, 4)), int(rng.integers(1, 1 << 24))) for _ in range(300)]
    blend, fill = R.blend(20, 4, 131, 30, 0xffffff, 128), R.fill(20, 4, 131, 30, 0x3050a0)
    many[10], many[290] = (blend, fill) if order == "blend at 10" else (fill, blend)
    for k in range(291, 300):                                            # (the marks behind index 290 stay clear of its rectangle)
        many[k] = R.disc(5, 3 * (k - 291) + 3, 2, 0x010101 * k & 0xffffff)
    return many


CASES = {
    "single blends": lambda w: [single_blends(w), single_blends(w)[::-1]],
    "wholly outside": lambda w: [OUTSIDE, OUTSIDE[:1]],
    "stacked ab": lambda w: [stacked("ab"), []],
    "stacked ba": lambda w: [stacked("ba"), stacked("ab")],
    "blend then disc": lambda w: [with_disc("blend first"), []],
    "disc then blend": lambda w: [with_disc("disc first"), []],
    "blend at 10, fill at 290": lambda w: [across_passes("blend at 10"), []],
    "fill at 10, blend at 290": lambda w: [across_passes("fill at 10"), across_passes("blend at 10")[:40]],
}


@pytest.fixture(scope="module")
def frames():
    return {132: ramp(2, H, 132), 130: ramp(2, H, 130)}


@pytest.fixture(scope="module")
def wanted(frames):
    """``render_host`` of every case and width in BGR, computed once."""
    return {(name, w): host_render(frames[w], make(w)).reshape(frames[w].shape) for name, make in CASES.items() for w in frames}


@pytest.mark.parametrize("w", [132, 130])
@pytest.mark.parametrize("name", list(CASES))
def test_blend_cases_in_every_output(gpu_engine, frames, wanted, name, w):
    f, per_frame, want = frames[w], CASES[name](w), wanted[(name, w)]
    path_wanted = E.RENDER_PATH_VECTOR if w % 4 == 0 else E.RENDER_PATH_BYTE
    for label, layout in OUTPUTS:
        geom = video.yuv_desc(w, H, layout) if layout else None
        got, path = gpu_render(gpu_engine, f, per_frame, E.RENDER_YUV420 if layout else E.RENDER_BGR, geom, ENC if layout else None)
        assert path == path_wanted, label
        expect = host_render(f, per_frame, E.RENDER_YUV420, geom, ENC) if layout else want.reshape(-1)
        assert np.array_equal(got, expect), label
    in_place, path = gpu_render(gpu_engine, f, per_frame, in_place=True)
    assert path == path_wanted and np.array_equal(in_place, want.reshape(-1))


def test_what_the_cases_show(frames, wanted):
    """The host results the kernel was compared with do distinguish what the cases are about (no GPU in this one)."""
    f = frames[132]
    assert np.array_equal(wanted[("wholly outside", 132)], f)                          # no byte changes
    assert not np.array_equal(wanted[("stacked ab", 132)][0], wanted[("stacked ba", 132)][0])
    a, b = wanted[("blend then disc", 132)][0], wanted[("disc then blend", 132)][0]
    assert tuple(a[15, 127]) == (255, 0, 0) and tuple(b[15, 127]) == (255, 128, 128)     # BGR: the red disc, and the disc seen through the panel
    a, b = wanted[("blend at 10, fill at 290", 132)][0], wanted[("fill at 10, blend at 290", 132)][0]
    inside = (slice(4, 31), slice(20, 132))
    assert (a[inside] == (0xa0, 0x50, 0x30)).all()                                     # the later fill hides the blend
    before = host_render(f[:1], [across_passes("fill at 10")[:290]]).reshape(H, 132, 3)   # the fill and the 279 discs on top of it
    assert (before[8, 60:70] == (0xa0, 0x50, 0x30)).any()
    through = (before[inside].astype(np.int64) * 128 + 255 * 128 + 128) >> 8
    assert np.array_equal(b[inside], through)                                          # the later blend sees what the first pass left
    w1 = wanted[("single blends", 132)][0]
    assert tuple(w1[0, 0]) != tuple(f[0, 0, 0]) and not np.array_equal(w1[14:17, 125:130], f[0, 14:17, 125:130])


def test_weights_outside_1_to_255_raise_and_nothing_is_launched(gpu_engine):
    eng = gpu_engine
    f = frames_of(1, 8, 16)
    src = eng.alloc(f.nbytes).upload(f)
    dst = eng.alloc(f.nbytes)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    for weight in (0, 256, -1):
        marks, first = R.pack([[R.blend(1, 1, 9, 6, 0xffffff, weight)]])
        with pytest.raises(E.EngineError, match="weight"):
            eng.render(src, 1, 8, 16, marks, first, dst)
    with pytest.raises(E.EngineError, match="unknown kind"):
        eng.render(src, 1, 8, 16, np.array([(7, 0, 0, 0, 0, 1, 0, 0)], E.MARK_DTYPE), [0, 1], dst)
    eng.synchronize()
    assert np.all(dst.download(np.empty(dst.nbytes, np.uint8)) == 0x5A)
    marks, first = R.pack([[R.blend(1, 1, 9, 6, 0xffffff, 128)]])
    eng.render(src, 1, 8, 16, marks, first, dst)                                       # and the engine still works
    assert np.array_equal(dst.download(np.empty(f.nbytes, np.uint8)), host_render(f, [[R.blend(1, 1, 9, 6, 0xffffff, 128)]]))
    src.free()
    dst.free()
