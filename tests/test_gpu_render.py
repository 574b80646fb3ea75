"""csrc/render.hip on the GPU against its numpy twin ``render.render_host``, bit for bit: BGR and YUV 4:2:0 output (NV12, I420), the
vector and the byte path (asserted through ``Engine.render_last_path``), partial edge tiles, marks across tile borders and outside
the frame, more marks than one pass of the LDS list holds, list order, the font, in-place rendering, bytes around the destination,
and the refusals.  A tile is 128 x 16 pixels: 136 x 36 frames are two tiles each way with partial edge tiles."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, render as R, video

pytestmark = pytest.mark.gpu

ENC = video.YUV_ENC_COEFFS["bt601_limited"]
PAD = 64            # sentinel bytes kept in front of and behind the destination


def frames_of(n, h, w, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def busy_marks(h, w, seed, count=24):
    """Marks of every kind: across the tile borders at x = 128 and y = 16 / 32, half outside and wholly outside the frame."""
    rng = np.random.default_rng(seed)
    col = lambda: int(rng.integers(1, 1 << 24))
    m = [R.segment(-20, -7, w + 9, h + 5, 3, col()), R.segment(120, 2, 135, 33, 2, col()), R.disc(128, 16, 9, col()), R.disc(0, 0, 6, col()),
         R.disc(w - 1, h - 1, 7, col()), R.box(100, 10, 133, 34, 2, col()), R.fill(126, 14, 130, 18, col()), R.fill(-50, -50, -10, -10, col()),
         R.disc(w + 300, 5, 20, col()), R.box(-30, 20, 40, h + 30, 4, col()), R.segment(3, 31, 70, 31, 1, col())] + R.text("AB-9", 118, 10, 2, col())
    for _ in range(count):
        x, y = int(rng.integers(-10, w + 10)), int(rng.integers(-10, h + 10))
        k = int(rng.integers(0, 5))
        m.append([R.disc(x, y, int(rng.integers(0, 12)), col()),
                  R.segment(x, y, int(rng.integers(-10, w + 10)), int(rng.integers(-10, h + 10)), int(rng.integers(1, 6)), col()),
                  R.fill(x, y, x + int(rng.integers(-9, 9)), y + int(rng.integers(-9, 9)), col()),
                  R.box(x, y, x + int(rng.integers(-30, 30)), y + int(rng.integers(-30, 30)), int(rng.integers(1, 4)), col()),
                  R.glyph(R.FONT_CHARS[int(rng.integers(0, 40))], x, y, int(rng.integers(1, 4)), col())][k])
    return m


def gpu_render(eng, frames, per_frame, out=E.RENDER_BGR, geom=None, enc=None, src_shift=0, dst_shift=0, in_place=False):
    """-> (result bytes, path): ``frames`` uploaded ``src_shift`` bytes into a buffer, rendered to ``dst_shift`` bytes into another one
    that is filled with 0x5A first; the PAD bytes on both sides of the destination must come back untouched, and the source unchanged."""
    n, h, w = frames.shape[:3]
    marks, first = R.pack(per_frame)
    src = eng.alloc(frames.nbytes + src_shift + 4)
    sv = src.view(src_shift, frames.nbytes)
    sv.upload(frames)
    span = frames.nbytes if out == E.RENDER_BGR else video.yuv_span(n, h, w, geom)
    if in_place:
        eng.render(sv, n, h, w, marks, first, sv)
        path = eng.render_last_path()
        got = sv.download(np.empty(span, np.uint8))
        src.free()
        return got, path
    dst = eng.alloc(span + 2 * PAD + dst_shift)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    eng.render(sv, n, h, w, marks, first, dst.view(PAD + dst_shift, span), out=out, geom=geom, enc=enc)
    path = eng.render_last_path()
    whole = dst.download(np.empty(dst.nbytes, np.uint8))
    assert np.all(whole[:PAD + dst_shift] == 0x5A) and np.all(whole[PAD + dst_shift + span:] == 0x5A), "bytes around dst were written"
    assert np.array_equal(sv.download(np.empty(frames.nbytes, np.uint8)), frames.reshape(-1)), "the source was written"
    src.free()
    dst.free()
    return whole[PAD + dst_shift:PAD + dst_shift + span], path


def host_render(frames, per_frame, out=E.RENDER_BGR, geom=None, enc=None):
    n, h, w = frames.shape[:3]
    marks, first = R.pack(per_frame)
    dst = None if out == E.RENDER_BGR else np.full(video.yuv_span(n, h, w, geom), 0x5A, np.uint8)      # the gaps keep what dst held
    return R.render_host(frames, marks, first, out, geom, enc, dst=dst).reshape(-1)


@pytest.fixture(scope="module")
def scene():
    frames = frames_of(3, 36, 136)
    per_frame = [busy_marks(36, 136, 1), [], busy_marks(36, 136, 2)]          # a frame with no marks between two with marks
    return frames, per_frame


def test_bgr_output(gpu_engine, scene):
    frames, per_frame = scene
    got, path = gpu_render(gpu_engine, frames, per_frame)
    assert path == E.RENDER_PATH_VECTOR
    want = host_render(frames, per_frame)
    assert np.array_equal(got, want)
    g = got.reshape(frames.shape)
    assert np.array_equal(g[1], frames[1]) and not np.array_equal(g[0], frames[0])


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_yuv_output(gpu_engine, scene, layout):
    frames, per_frame = scene
    geom = video.yuv_desc(136, 36, layout)
    got, path = gpu_render(gpu_engine, frames, per_frame, E.RENDER_YUV420, geom, ENC)
    assert path == E.RENDER_PATH_VECTOR
    assert np.array_equal(got, host_render(frames, per_frame, E.RENDER_YUV420, geom, ENC))
    s = geom["frame_stride"]
    plain = video.bgr_to_yuv420_host(frames[1:2], geom, ENC)                    # the frame without marks: the plain encode
    assert np.array_equal(got[s:s + plain.size], plain)


@pytest.mark.parametrize("out, layout", [(E.RENDER_BGR, None), (E.RENDER_YUV420, "nv12"), (E.RENDER_YUV420, "i420")])
def test_byte_path_with_a_two_pixel_tail(gpu_engine, out, layout):
    frames = frames_of(2, 18, 70, seed=3)
    per_frame = [busy_marks(18, 70, 3, 12), [R.disc(68, 9, 5, 0x123456), R.segment(60, 0, 69, 17, 2, 0xABCDEF)]]
    geom = video.yuv_desc(70, 18, layout) if layout else None
    got, path = gpu_render(gpu_engine, frames, per_frame, out, geom, ENC if layout else None)
    assert path == E.RENDER_PATH_BYTE
    assert np.array_equal(got, host_render(frames, per_frame, out, geom, ENC if layout else None))


def test_odd_sizes_in_bgr(gpu_engine):
    frames = frames_of(2, 19, 131, seed=4)                                     # a 3-pixel tail column block, a 1-row tail
    per_frame = [busy_marks(19, 131, 4, 12), busy_marks(19, 131, 5, 12)]
    got, path = gpu_render(gpu_engine, frames, per_frame)
    assert path == E.RENDER_PATH_BYTE
    assert np.array_equal(got, host_render(frames, per_frame))


@pytest.mark.parametrize("layout, kw", [("nv12", dict(pitch=144, pitch_c=152)), ("i420", dict(pitch=140, pitch_c=70))])
def test_vector_path_with_padded_pitches(gpu_engine, scene, layout, kw):
    frames, per_frame = scene
    geom = video.yuv_desc(136, 36, layout, **kw)
    got, path = gpu_render(gpu_engine, frames, per_frame, E.RENDER_YUV420, geom, ENC)
    assert path == E.RENDER_PATH_VECTOR
    assert np.array_equal(got, host_render(frames, per_frame, E.RENDER_YUV420, geom, ENC))


@pytest.mark.parametrize("out, layout, shifts", [(E.RENDER_BGR, None, (0, 1)), (E.RENDER_BGR, None, (1, 0)), (E.RENDER_YUV420, "nv12", (0, 1)),
                                                 (E.RENDER_YUV420, "i420", (0, 1)), (E.RENDER_YUV420, "nv12", (0, 0)),
                                                 (E.RENDER_YUV420, "i420", (0, 0))])
def test_misaligned_buffers_take_the_byte_path(gpu_engine, scene, out, layout, shifts):
    """A destination (or source) one byte off alignment, and for the last two cases an odd pitch behind aligned pointers."""
    frames, per_frame = scene
    geom = None
    if layout:
        geom = video.yuv_desc(136, 36, layout, **(dict(pitch=137) if shifts == (0, 0) else {}))
    got, path = gpu_render(gpu_engine, frames, per_frame, out, geom, ENC if layout else None, src_shift=shifts[0], dst_shift=shifts[1])
    assert path == E.RENDER_PATH_BYTE
    assert np.array_equal(got, host_render(frames, per_frame, out, geom, ENC if layout else None))


def test_more_marks_than_one_pass_keeps_list_order(gpu_engine):
    """300 overlapping marks on one frame (a pass of the LDS list holds 256): later marks must win across the pass boundary — mark
    255 / 256 overlap on purpose, and the last marks cover pixels of the first."""
    frames = frames_of(2, 36, 136, seed=9)
    rng = np.random.default_rng(9)
    many = [R.disc(int(rng.integers(0, 136)), int(rng.integers(0, 36)), int(rng.integers(3, 10)), int(rng.integers(1, 1 << 24))) for _ in range(300)]
    many[255] = R.fill(10, 5, 130, 30, 0x00FF00)
    many[256] = R.fill(20, 8, 131, 33, 0xFF0000)
    many[299] = R.segment(0, 0, 135, 35, 5, 0x0000FF)
    per_frame = [many, many[:7]]
    got, path = gpu_render(gpu_engine, frames, per_frame)
    want = host_render(frames, per_frame)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, host_render(frames, [many[:256][::-1] + many[256:], many[:7]]))     # (order does matter here)
    geom = video.yuv_desc(136, 36, "nv12")
    got, _ = gpu_render(gpu_engine, frames, per_frame, E.RENDER_YUV420, geom, ENC)
    assert np.array_equal(got, host_render(frames, per_frame, E.RENDER_YUV420, geom, ENC))


def test_two_overlapping_discs_in_both_orders(gpu_engine):
    frames = frames_of(1, 36, 136, seed=10)
    a, b = R.disc(124, 14, 9, 0x0000FF), R.disc(131, 18, 9, 0x00FF00)            # over the corner where four tiles meet
    res = {}
    for key, order in (("ab", [a, b]), ("ba", [b, a])):
        got, _ = gpu_render(gpu_engine, frames, [order])
        assert np.array_equal(got, host_render(frames, [order]))
        res[key] = got.reshape(36, 136, 3)
    assert tuple(res["ab"][16, 128]) == (0, 255, 0) and tuple(res["ba"][16, 128]) == (255, 0, 0)


@pytest.mark.parametrize("k", [1, 3])
def test_all_glyphs(gpu_engine, k):
    frames = frames_of(1, 36 if k == 1 else 76, 136 if k == 1 else 264, seed=11)      # room for every glyph: 2 rows of 22, 3 rows of 14
    w = frames.shape[2]
    per = w // (6 * k)
    marks = []
    for i, ch in enumerate(R.FONT_CHARS):
        marks += R.text(ch, 1 + (i % per) * 6 * k, 1 + (i // per) * 8 * k - (3 if i % 7 == 0 and i >= per else 0), k, 0xFFFFFF - i)
    got, _ = gpu_render(gpu_engine, frames, [marks])
    want = host_render(frames, [marks])
    assert np.array_equal(got, want) and not np.array_equal(want, frames.reshape(-1))


def test_in_place_equals_out_of_place(gpu_engine, scene):
    frames, per_frame = scene
    out_of_place, _ = gpu_render(gpu_engine, frames, per_frame)
    in_place, path = gpu_render(gpu_engine, frames, per_frame, in_place=True)
    assert path == E.RENDER_PATH_VECTOR
    assert np.array_equal(in_place, out_of_place)
    in_place, path = gpu_render(gpu_engine, frames, per_frame, in_place=True, src_shift=1)
    assert path == E.RENDER_PATH_BYTE and np.array_equal(in_place, out_of_place)


def test_one_image_alone_equals_the_second_of_a_batch(gpu_engine, scene):
    frames, per_frame = scene
    geom = video.yuv_desc(136, 36, "i420")
    batch, _ = gpu_render(gpu_engine, frames, per_frame, E.RENDER_YUV420, geom, ENC)
    alone, _ = gpu_render(gpu_engine, frames[2:3], per_frame[2:3], E.RENDER_YUV420, geom, ENC)
    s = geom["frame_stride"]
    assert np.array_equal(alone, batch[2 * s:2 * s + alone.size])
    bgr, _ = gpu_render(gpu_engine, frames, per_frame)
    one, _ = gpu_render(gpu_engine, frames[2:3], per_frame[2:3])
    assert np.array_equal(one, bgr[2 * frames[0].size:])


def test_refusals_raise(gpu_engine):
    eng = gpu_engine
    frames = frames_of(1, 8, 16)
    src = eng.alloc(frames.nbytes).upload(frames)
    dst = eng.alloc(frames.nbytes)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    ok, first = R.pack([[R.disc(1, 1, 1, 1)]])
    geom = video.yuv_desc(16, 8, "nv12")
    bad_mark = np.array([(9, 0, 0, 0, 0, 1, 0, 0)], E.MARK_DTYPE)
    far = np.array([(E.MARK_DISC, 9000, 0, 0, 0, 1, 0, 0)], E.MARK_DTYPE)
    cases = [dict(marks=bad_mark, words="unknown kind"), dict(marks=far, words="coordinate"), dict(first=[1, 1], words="first"),
             dict(n=0, first=[0], words="n = 0"), dict(w=15, h=8, out=E.RENDER_YUV420, geom=video.yuv_desc(16, 8, "nv12"), enc=ENC, words="even"),
             dict(out=E.RENDER_YUV420, geom=dict(geom, pitch_y=15), enc=ENC, words="pitch_y"),
             dict(out=E.RENDER_YUV420, geom=dict(geom, off_v=geom["off_u"] + 2), enc=ENC, words="off_u + 1"),
             dict(out=E.RENDER_YUV420, geom=None, enc=None, words="geometry")]
    for c in cases:
        with pytest.raises(E.EngineError, match=c["words"].replace("+", r"\+")):
            eng.render(src, c.get("n", 1), c.get("h", 8), c.get("w", 16), c.get("marks", ok), c.get("first", first), dst, out=c.get("out", E.RENDER_BGR),
                       geom=c.get("geom"), enc=c.get("enc"))
    with pytest.raises(E.EngineError, match="dst holds"):                      # a destination too small for what geom describes
        eng.render(src, 1, 8, 16, ok, first, dst.view(0, 100), out=E.RENDER_YUV420, geom=geom, enc=ENC)
    with pytest.raises(E.EngineError, match="overlaps"):
        eng.render(src, 1, 8, 16, ok, first, src.view(4, frames.nbytes - 4), out=E.RENDER_YUV420, geom=dict(geom, frame_stride=192), enc=ENC)
    eng.synchronize()
    assert np.all(dst.download(np.empty(dst.nbytes, np.uint8)) == 0x5A)        # nothing was launched
    eng.render(src, 1, 8, 16, ok, first, dst)                                  # and the engine still works
    assert np.array_equal(dst.download(np.empty(frames.nbytes, np.uint8)), host_render(frames, [[R.disc(1, 1, 1, 1)]]))
    src.free()
    dst.free()
