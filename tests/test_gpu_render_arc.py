"""``PA_MARK_ARC`` in csrc/render.hip on the GPU against ``render.render_host``, bit for bit: the elliptical ring cut to octants.
Frames of 2 x 48 x 272 (three tiles across with a partial one, three down: the vector path) and 2 x 48 x 270 (the byte path, a
2-pixel tail), the path asserted through ``Engine.render_last_path``; BGR (also in place), NV12 and I420 output.  Arcs of every
single-octant mask, the full mask and the ellipse annotator's 0x9F across the tile borders at x = 128 and 256 and y = 16 and 32, half
and wholly outside the frame; b = 1, no hole (t >= a), t = 1, and semi-axes of 4095 whose centre lies outside the frame (the 64-bit
range of the rule); an arc and a disc over the same pixels in both orders, within one pass of the kernel's LDS list (256 marks) and on
either side of the boundary between two; a blend over an arc.  ``gpu_render`` checks the sentinel bytes around the destination and
that the source is not written."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, render as R, video
from tests.test_gpu_render import ENC, frames_of, gpu_render, host_render

pytestmark = pytest.mark.gpu

H = 48
OUTPUTS = [("bgr", None), ("nv12", "nv12"), ("i420", "i420")]
MASKS = [1 << k for k in range(8)] + [0xFF, 0x9F]


def colour(k):
    return (0x3157 * (k + 1) * 977) & 0xffffff | 0x010101


def on_borders(w):
    """Every mask, centred on the tile corners and beside them: the ring crosses x = 128 and 256 and y = 16 and 32."""
    spots = [(128, 16, 20, 9), (256, 32, 13, 13), (127, 31, 40, 14), (255, 17, 9, 20), (192, 24, 70, 22)]
    return [R.arc(x, y, a, b, 1 + k % 3, colour(k), m) for k, (m, (x, y, a, b)) in enumerate((m, s) for s in spots for m in MASKS)]


def half_outside(w):
    spots = [(0, 0, 30, 12), (w - 1, H - 1, 25, 25), (w + 5, 20, 40, 18), (140, -6, 60, 20), (60, H + 3, 33, 12), (-10, 24, 44, 30)]
    return [R.arc(x, y, a, b, 2, colour(k), m) for k, (m, (x, y, a, b)) in enumerate((m, s) for s in spots for m in (0xFF, 0x9F, 0x01, 0x10, 0x44))]


OUTSIDE = [R.arc(-50, -50, 30, 30, 2, 0xffffff, 0xFF), R.arc(400, 20, 100, 10, 255, 0xffffff, 0xFF), R.arc(100, 80, 60, 31, 1, 0x123456, 0x9F),
           R.arc(-8192, -8192, 4095, 4095, 1, 0xffffff, 0xFF), R.arc(8191, 8191, 4095, 4095, 255, 0xffffff, 0xFF),
           R.arc(136, 60, 50, 11, 3, 0x00ff00, 0xF0)]


def special(w):
    return [R.arc(40, 10, 35, 1, 1, 0x0000ff, 0xFF), R.arc(130, 30, 1, 14, 3, 0x00ffff, 0xFF),                   # b = 1, a = 1
            R.arc(60, 30, 12, 7, 7, 0x00ff00, 0xFF), R.arc(150, 20, 9, 9, 255, 0xff00ff, 0x9F),                 # no hole
            R.arc(200, 24, 60, 21, 1, 0xffff00, 0xFF), R.arc(256, 16, 11, 4, 1, 0x80ff80, 0x9F),                 # t = 1
            R.arc(4095 + 100, 24, 4095, 4095, 1, 0xff8000, 0xFF), R.arc(130, -4095 + 40, 4095, 4095, 3, 0x0080ff, 0xFF),      # the int64 range, ring in sight
            R.arc(130 - 2895, 24 + 2895, 4095, 4095, 255, 0x8000ff, 0x81), R.arc(8191, 24, 4095, 4095, 2, 0x112233, 0xFF),
            R.arc(-8192, 8191, 4095, 4095, 1, 0x332211, 0xFF), R.arc(1, 1, 1, 1, 1, 0xffffff, 0xFF)]


def with_disc(order):
    arc, disc = R.arc(128, 16, 30, 12, 3, 0x0000ff, 0x9F), R.disc(128, 27, 8, 0x00ff00)
    return [arc, disc] if order == "arc first" else [disc, arc]


def across_passes(order):
    """300 marks: index 10 and index 290 cover some of the same pixels — one pass of the LDS list holds 256, so they meet in
    different passes."""
    rng = np.random.default_rng(33)
    many = [R.disc(int(rng.integers(0, 270)), int(rng.integers(0, H)), int(rng.integers(1, 4)), int(rng.integers(1, 1 << 24))) for _ in range(300)]
    arc, disc = R.arc(128, 20, 100, 18, 4, 0x3050a0, 0xFF), R.disc(128, 36, 12, 0xf0f000)
    many[10], many[290] = (arc, disc) if order == "arc at 10" else (disc, arc)
    for k in range(291, 300):                                            # (the marks behind index 290 stay clear of both)
        many[k] = R.disc(5, 4 * (k - 291) + 3, 1, 0x010101 * k & 0xffffff)
    return many


CASES = {
    "every mask on the tile borders": lambda w: [on_borders(w), on_borders(w)[::-1]],
    "half outside": lambda w: [half_outside(w), half_outside(w)[::3]],
    "wholly outside": lambda w: [OUTSIDE, OUTSIDE[:1]],
    "special shapes": lambda w: [special(w), special(w)[::-1]],
    "arc then disc": lambda w: [with_disc("arc first"), []],
    "disc then arc": lambda w: [with_disc("disc first"), with_disc("arc first")],
    "arc at 10, disc at 290": lambda w: [across_passes("arc at 10"), []],
    "disc at 10, arc at 290": lambda w: [across_passes("disc at 10"), across_passes("arc at 10")[:40]],
    "a blend over an arc": lambda w: [[R.arc(128, 16, 50, 14, 3, 0x0000ff, 0xFF), R.blend(100, 10, 140, 40, 0xffffff, 128)],
                                      [R.blend(100, 10, 140, 40, 0xffffff, 128), R.arc(128, 16, 50, 14, 3, 0x0000ff, 0xFF)]],
}


@pytest.fixture(scope="module")
def frames():
    return {272: frames_of(2, H, 272, seed=41), 270: frames_of(2, H, 270, seed=42)}


@pytest.fixture(scope="module")
def wanted(frames):
    """``render_host`` of every case and width in BGR, computed once."""
    return {(name, w): host_render(frames[w], make(w)).reshape(frames[w].shape) for name, make in CASES.items() for w in frames}


@pytest.mark.parametrize("w", [272, 270])
@pytest.mark.parametrize("name", list(CASES))
def test_arc_cases_in_every_output(gpu_engine, frames, wanted, name, w):
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
    f = frames[272]
    assert np.array_equal(wanted[("wholly outside", 272)], f)                          # no byte changes
    changed = lambda name, k=0: (wanted[(name, 272)][k] != f[k]).any(-1)
    b = changed("every mask on the tile borders")
    assert b[:, 127].any() and b[:, 128].any() and b[:, 255].any() and b[:, 256].any() and b[15].any() and b[16].any() and b[31].any() and b[32].any()
    assert changed("half outside")[0, 0:31].any() and changed("half outside")[H - 1, 240:].any()
    s = changed("special shapes")
    assert s[10, 5:76].all() and s[9, 5:76].sum() == 1 and s[11, 5:76].sum() == 1       # b = 1: a row of 71 pixels, one above and below the centre
    assert s[24, 100] and not s[24, 99]                                                # a = b = 4095 around (4195, 24): its left end at x = 100
    assert s[20:30, 120:140].any() and not s[20:30, 120:140].all()                     # the thick one cut at -45 degrees
    a, d = wanted[("arc then disc", 272)][0], wanted[("disc then arc", 272)][0]
    assert tuple(a[27, 128]) == (0, 255, 0) and tuple(d[27, 128]) == (255, 0, 0)       # BGR: the disc on top, and the arc on top
    a, d = wanted[("arc at 10, disc at 290", 272)][0], wanted[("disc at 10, arc at 290", 272)][0]
    assert tuple(a[37, 128]) == (0x00, 0xf0, 0xf0) and tuple(d[37, 128]) == (0xa0, 0x50, 0x30)
    over, under = wanted[("a blend over an arc", 272)]
    assert tuple(over[30, 128]) == (255, 128, 128) and tuple(under[30, 128]) == (255, 0, 0)


def test_arcs_out_of_range_raise_and_nothing_is_launched(gpu_engine):
    eng = gpu_engine
    f = frames_of(1, 8, 16)
    src = eng.alloc(f.nbytes).upload(f)
    dst = eng.alloc(f.nbytes)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    for mark, words in (((E.MARK_ARC, 8, 4, 0, 3, 1, 0xffffff, 0xFF), "semi-axis"), ((E.MARK_ARC, 8, 4, 5, 4096, 1, 0xffffff, 0xFF), "semi-axis"),
                        ((E.MARK_ARC, 8, 4, 5, 3, 0, 0xffffff, 0xFF), "size"), ((E.MARK_ARC, 8, 4, 5, 3, 256, 0xffffff, 0xFF), "size"),
                        ((E.MARK_ARC, 8, 4, 5, 3, 1, 0xffffff, 0), "octant mask"), ((E.MARK_ARC, 8, 4, 5, 3, 1, 0xffffff, 256), "octant mask")):
        with pytest.raises(E.EngineError, match=words):
            eng.render(src, 1, 8, 16, np.array([mark], E.MARK_DTYPE), [0, 1], dst)
    eng.synchronize()
    assert np.all(dst.download(np.empty(dst.nbytes, np.uint8)) == 0x5A)
    ring = [[R.arc(8, 4, 5, 3, 1, 0xffffff, 0xFF)]]
    eng.render(src, 1, 8, 16, *R.pack(ring), dst)                                      # and the engine still works
    got = dst.download(np.empty(f.nbytes, np.uint8))
    assert np.array_equal(got, host_render(f, ring)) and not np.array_equal(got, f.reshape(-1))
    src.free()
    dst.free()
