"""``Engine.render(scale=2, 3, 4)`` (csrc/render.hip, ``render_scaled_kernel``) on the GPU against its numpy twin
``render.render_host(scale=)``, bit for bit: BGR, NV12 and I420 output, the vector and the byte path (asserted through
``Engine.render_last_path``), the smallest legal frame, partial tiles, marks of every kind across block and tile borders and outside
the frame, more marks than one pass of the LDS list holds with a blend on either side of the pass boundary, list order, several
frames with their own marks, misaligned and padded destinations with sentinel bytes around them, the refusals, and one wide frame
through the Motion-JPEG encoder.  One thread owns one output pixel (s x s source pixels); a workgroup's tile is 32 s x 8 s source
pixels."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, mjpeg, render as R, video

pytestmark = pytest.mark.gpu

ENC = video.YUV_ENC_COEFFS["bt601_limited"]
PAD = 64            # sentinel bytes kept in front of and behind the destination
OUTS = [(E.RENDER_BGR, None), (E.RENDER_YUV420, "nv12"), (E.RENDER_YUV420, "i420")]
OUT_IDS = ["bgr", "nv12", "i420"]


def frames_of(n, h, w, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def busy_marks(h, w, s, seed, count=16):
    """One of every kind straddling the borders of the threads' s x s boxes and of the first tile (x = 32 s, y = 8 s), a one-pixel
    segment (fractional coverage of an output pixel), marks half and wholly outside the frame, then ``count`` seeded ones."""
    rng = np.random.default_rng(seed)
    col = lambda: int(rng.integers(1, 1 << 24))
    tx, ty = min(32 * s, w - 2), min(8 * s, h - 2)
    m = [R.segment(-20, -7, w + 9, h + 5, 1, col()), R.segment(tx - 9, 1, tx + 6, h - 2, 2, col()), R.disc(tx, ty, 5, col()), R.disc(0, 0, 4, col()),
         R.disc(w - 1, h - 1, 5, col()), R.box(tx - 11, ty - 5, tx + 7, ty + 6, 2, col()), R.fill(tx - 1, ty - 1, tx + s, ty + s, col()),
         R.blend(tx - 20, 2, tx + 13, ty + 3, col(), 77), R.arc(tx - 2, ty + 1, 12, 7, 2, col(), 0xB7), R.fill(-50, -50, -10, -10, col()),
         R.disc(w + 300, 5, 20, col()), R.box(-30, 5, 17, h + 30, 3, col()), R.segment(3, ty + 1, w - 5, ty + 1, 1, col()),
         R.arc(w + 2, h // 2, 9, 14, 3, col())] + R.text("A-9", tx - 8, ty - 4, 2, col())
    for _ in range(count):
        x, y = int(rng.integers(-10, w + 10)), int(rng.integers(-10, h + 10))
        k = int(rng.integers(0, 7))
        m.append([R.disc(x, y, int(rng.integers(0, 9)), col()),
                  R.segment(x, y, int(rng.integers(-10, w + 10)), int(rng.integers(-10, h + 10)), int(rng.integers(1, 5)), col()),
                  R.fill(x, y, x + int(rng.integers(-9, 9)), y + int(rng.integers(-9, 9)), col()),
                  R.box(x, y, x + int(rng.integers(-30, 30)), y + int(rng.integers(-30, 30)), int(rng.integers(1, 4)), col()),
                  R.glyph(R.FONT_CHARS[int(rng.integers(0, 40))], x, y, int(rng.integers(1, 4)), col()),
                  R.blend(x, y, x + int(rng.integers(-25, 25)), y + int(rng.integers(-25, 25)), col(), int(rng.integers(1, 256))),
                  R.arc(x, y, int(rng.integers(1, 20)), int(rng.integers(1, 20)), int(rng.integers(1, 4)), col(), int(rng.integers(1, 256)))][k])
    return m


def gpu_render(eng, frames, per_frame, s, out=E.RENDER_BGR, geom=None, enc=None, src_shift=0, dst_shift=0):
    """-> (result bytes, path): ``frames`` uploaded ``src_shift`` bytes into a buffer, rendered at scale ``s`` to ``dst_shift`` bytes into
    another one that is filled with 0x5A first; the PAD bytes on both sides of the destination must come back untouched, and the
    source unchanged."""
    n, h, w = frames.shape[:3]
    ho, wo = h // s, w // s
    marks, first = R.pack(per_frame)
    src = eng.alloc(frames.nbytes + src_shift + 4)
    sv = src.view(src_shift, frames.nbytes)
    sv.upload(frames)
    span = n * ho * wo * 3 if out == E.RENDER_BGR else video.yuv_span(n, ho, wo, geom)
    dst = eng.alloc(span + 2 * PAD + dst_shift)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    eng.render(sv, n, h, w, marks, first, dst.view(PAD + dst_shift, span), out=out, geom=geom, enc=enc, scale=s)
    path = eng.render_last_path()
    whole = dst.download(np.empty(dst.nbytes, np.uint8))
    assert np.all(whole[:PAD + dst_shift] == 0x5A) and np.all(whole[PAD + dst_shift + span:] == 0x5A), "bytes around dst were written"
    assert np.array_equal(sv.download(np.empty(frames.nbytes, np.uint8)), frames.reshape(-1)), "the source was written"
    src.free()
    dst.free()
    return whole[PAD + dst_shift:PAD + dst_shift + span], path


def host_render(frames, per_frame, s, out=E.RENDER_BGR, geom=None, enc=None):
    n, h, w = frames.shape[:3]
    marks, first = R.pack(per_frame)
    dst = None if out == E.RENDER_BGR else np.full(video.yuv_span(n, h // s, w // s, geom), 0x5A, np.uint8)      # the gaps keep what dst held
    return R.render_host(frames, marks, first, out, geom, enc, dst=dst, scale=s).reshape(-1)


def both(eng, frames, per_frame, s, out, layout, want_path, **kw):
    h, w = frames.shape[1:3]
    desc = kw.pop("desc", {})
    geom = video.yuv_desc(w // s, h // s, layout, **desc) if layout else None
    enc = ENC if layout else None
    got, path = gpu_render(eng, frames, per_frame, s, out, geom, enc, **kw)
    want = host_render(frames, per_frame, s, out, geom, enc)
    assert path == want_path
    assert np.array_equal(got, want)
    return got


# source sizes (w, h) per scale, and the path they take: wo % 4 == 0 is the vector path
SIZES = {2: [((96, 64), E.RENDER_PATH_VECTOR), ((100, 60), E.RENDER_PATH_BYTE)],       # 48 x 32; 50 x 30: wo no multiple of 4
         3: [((132, 72), E.RENDER_PATH_VECTOR)],                                        # 44 x 24: two tiles across, partial
         4: [((272, 48), E.RENDER_PATH_VECTOR)]}                                        # 68 x 12: two source tiles across, partial tiles
CASES = [(s, size, path) for s in (2, 3, 4) for size, path in SIZES[s]]


@pytest.mark.parametrize("out, layout", OUTS, ids=OUT_IDS)
@pytest.mark.parametrize("s, size, path", CASES, ids=[f"s{s}-{size[0]}x{size[1]}" for s, size, _ in CASES])
def test_every_scale_and_output_against_the_twin(gpu_engine, s, size, path, out, layout):
    """n = 3 with different marks per frame, one of them bare: that frame is the plain average."""
    w, h = size
    frames = frames_of(3, h, w, seed=s)
    per_frame = [busy_marks(h, w, s, 1), [], busy_marks(h, w, s, 2)]
    got = both(gpu_engine, frames, per_frame, s, out, layout, path)
    if out == E.RENDER_BGR:
        g = got.reshape(3, h // s, w // s, 3)
        assert np.array_equal(g[1], R.downscale_host(frames[1:2], s)[0]) and not np.array_equal(g[0], R.downscale_host(frames[:1], s)[0])


@pytest.mark.parametrize("out, layout", OUTS, ids=OUT_IDS)
@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_smallest_legal_frame(gpu_engine, s, out, layout):
    """2 s x 2 s: four output pixels, one chroma sample."""
    frames = frames_of(2, 2 * s, 2 * s, seed=20 + s)
    per_frame = [[R.disc(s, s - 1, 1, 0x40FF10), R.segment(0, 0, 2 * s - 1, 2 * s - 1, 1, 0xFF00FF)], [R.blend(-5, -5, s, 30, 0xFFFFFF, 128)]]
    both(gpu_engine, frames, per_frame, s, out, layout, E.RENDER_PATH_BYTE)


@pytest.mark.parametrize("s, size", [(2, (96, 64)), (3, (132, 72)), (4, (272, 48))])
@pytest.mark.parametrize("layout, kw", [("nv12", dict(pitch=80, pitch_c=88)), ("i420", dict(pitch=76, pitch_c=38))])
def test_vector_path_with_padded_pitches(gpu_engine, s, size, layout, kw):
    w, h = size
    frames = frames_of(2, h, w, seed=30 + s)
    both(gpu_engine, frames, [busy_marks(h, w, s, 3), busy_marks(h, w, s, 4)], s, E.RENDER_YUV420, layout, E.RENDER_PATH_VECTOR, desc=kw)


@pytest.mark.parametrize("out, layout, shifts, desc", [(E.RENDER_BGR, None, (0, 1), {}), (E.RENDER_BGR, None, (2, 0), {}),
                                                       (E.RENDER_YUV420, "nv12", (0, 1), {}), (E.RENDER_YUV420, "i420", (0, 3), {}),
                                                       (E.RENDER_YUV420, "nv12", (0, 0), dict(pitch=49)), (E.RENDER_YUV420, "i420", (0, 0), dict(pitch=51))])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_misaligned_buffers_take_the_byte_path(gpu_engine, s, out, layout, shifts, desc):
    """A destination or a source off alignment, and for the last two cases an odd pitch behind aligned pointers: output 48 x 16."""
    frames = frames_of(2, 16 * s, 48 * s, seed=40 + s)
    per_frame = [busy_marks(16 * s, 48 * s, s, 5), busy_marks(16 * s, 48 * s, s, 6, 4)]
    both(gpu_engine, frames, per_frame, s, out, layout, E.RENDER_PATH_BYTE, src_shift=shifts[0], dst_shift=shifts[1], desc=desc)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_more_marks_than_one_pass_keeps_list_order(gpu_engine, s):
    """300 overlapping marks on one frame (a pass of the LDS list holds 256), a blend on either side of the pass boundary: marks 255
    and 256 overlap on purpose, and the last marks cover pixels of the first."""
    w, h = 44 * s, 24 * s
    frames = frames_of(2, h, w, seed=50 + s)
    rng = np.random.default_rng(9)
    many = [R.disc(int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(3, 10)), int(rng.integers(1, 1 << 24))) for _ in range(300)]
    many[255] = R.blend(5, 3, w - 6, h - 9, 0x00FF00, 100)
    many[256] = R.blend(11, 7, w - 3, h - 2, 0xFF0000, 200)
    many[299] = R.segment(0, 0, w - 1, h - 1, 3, 0x0000FF)
    per_frame = [many, many[:7]]
    both(gpu_engine, frames, per_frame, s, E.RENDER_BGR, None, E.RENDER_PATH_VECTOR)
    both(gpu_engine, frames, per_frame, s, E.RENDER_YUV420, "nv12", E.RENDER_PATH_VECTOR)
    swapped = many[:255] + [many[256], many[255]] + many[257:]
    assert not np.array_equal(host_render(frames, per_frame, s), host_render(frames, [swapped, many[:7]], s))      # (order does matter here)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_two_overlapping_discs_in_both_orders(gpu_engine, s):
    w, h = 44 * s, 24 * s
    frames = frames_of(1, h, w, seed=60 + s)
    a, b = R.disc(32 * s - 4, 8 * s - 3, 3 * s, 0x0000FF), R.disc(32 * s + 3, 8 * s + 2, 3 * s, 0x00FF00)       # over the corner where four tiles meet
    res = {}
    for key, order in (("ab", [a, b]), ("ba", [b, a])):
        res[key] = both(gpu_engine, frames, [order], s, E.RENDER_BGR, None, E.RENDER_PATH_VECTOR).reshape(h // s, w // s, 3)
    assert tuple(res["ab"][8, 32]) == (0, 255, 0) and tuple(res["ba"][8, 32]) == (255, 0, 0)      # an output pixel wholly inside both


def test_scale_1_through_the_new_entry_is_pa_render(gpu_engine):
    eng = gpu_engine
    frames = frames_of(2, 36, 136, seed=70)
    marks, first = R.pack([busy_marks(36, 136, 1, 7), busy_marks(36, 136, 1, 8)])
    src = eng.alloc(frames.nbytes).upload(frames)
    geom = E._render_args(marks, first, video.yuv_desc(136, 36, "i420"), ENC)[2:]
    for out, g in ((E.RENDER_BGR, (None, None)), (E.RENDER_YUV420, geom)):
        span = frames.nbytes if out == E.RENDER_BGR else video.yuv_span(2, 36, 136, video.yuv_desc(136, 36, "i420"))
        got = []
        for scaled in (False, True):
            dst = eng.alloc(span)
            dst.upload(np.full(span, 0x5A, np.uint8))
            gp, ep = (E.C.byref(g[0]), E.C.byref(g[1])) if g[0] is not None else (None, None)
            head = (eng.handle, src.ptr, 2, 36, 136, marks.ctypes.data, first.ctypes.data)
            rc = eng.lib.pa_render_scaled(*head, 1, out, gp, ep, dst.ptr) if scaled else eng.lib.pa_render(*head, out, gp, ep, dst.ptr)
            assert rc == 0 and eng.render_last_path() == E.RENDER_PATH_VECTOR
            got.append(dst.download(np.empty(span, np.uint8)))
            dst.free()
        assert np.array_equal(got[0], got[1])
        assert np.array_equal(got[0], R.render_host(frames, marks, first, out, video.yuv_desc(136, 36, "i420") if out else None, ENC if out else None,
                                                    dst=None if out == E.RENDER_BGR else np.full(span, 0x5A, np.uint8)).reshape(-1))
    # in place, which only scale 1 does
    assert eng.lib.pa_render_scaled(eng.handle, src.ptr, 2, 36, 136, marks.ctypes.data, first.ctypes.data, 1, E.RENDER_BGR, None, None, src.ptr) == 0
    assert np.array_equal(src.download(np.empty(frames.nbytes, np.uint8)), R.render_host(frames, marks, first).reshape(-1))
    src.free()


def test_refusals_launch_nothing(gpu_engine):
    eng = gpu_engine
    frames = frames_of(1, 16, 24)
    whole = eng.alloc(4096)                                                    # room for the larger sources of the cases below
    src = whole.view(0, frames.nbytes)
    src.upload(frames)
    dst = eng.alloc(frames.nbytes)
    dst.upload(np.full(dst.nbytes, 0x5A, np.uint8))
    ok, first = R.pack([[R.disc(1, 1, 1, 1)]])
    geom = video.yuv_desc(12, 8, "nv12")
    bad_mark = np.array([(9, 0, 0, 0, 0, 1, 0, 0)], E.MARK_DTYPE)
    cases = [dict(scale=0, words="scale 0 outside"), dict(scale=5, words="scale 5 outside"), dict(scale=4, w=26, words="no multiple of scale 4"),
             dict(scale=3, h=17, words="no multiple of scale 3"), dict(scale=2, marks=bad_mark, words="unknown kind"),
             dict(scale=2, w=18, h=12, out=E.RENDER_YUV420, geom=video.yuv_desc(10, 6, "nv12"), enc=ENC, words="even output width"),
             dict(scale=2, out=E.RENDER_YUV420, geom=dict(geom, pitch_y=11), enc=ENC, words="pitch_y"),
             dict(scale=2, out=E.RENDER_YUV420, geom=None, enc=None, words="geometry"), dict(scale=2, dst=src, words="dst == src")]
    for c in cases:
        h, w = c.get("h", 16), c.get("w", 24)
        src_v = whole.view(0, h * w * 3)
        with pytest.raises(E.EngineError, match=c["words"]) as e:
            eng.render(src_v, 1, h, w, c.get("marks", ok), first, c.get("dst", dst), out=c.get("out", E.RENDER_BGR), geom=c.get("geom"),
                       enc=c.get("enc"), scale=c["scale"])
        # the host-only check says the same
        why = E.render_check(1, h, w, c.get("marks", ok), first, c.get("out", E.RENDER_BGR), c.get("geom"), c.get("enc"), scale=c["scale"],
                             in_place="dst" in c)
        assert why is not None and why in str(e.value)
    with pytest.raises(E.EngineError, match="dst holds"):                      # a destination too small for the scaled frames
        eng.render(src, 1, 16, 24, ok, first, dst.view(0, 100), out=E.RENDER_YUV420, geom=geom, enc=ENC, scale=2)
    with pytest.raises(E.EngineError, match="overlaps"):
        eng.render(src, 1, 16, 24, ok, first, src.view(4, 400), scale=2)
    eng.synchronize()
    assert np.all(dst.download(np.empty(dst.nbytes, np.uint8)) == 0x5A)        # nothing was launched
    assert np.array_equal(src.download(np.empty(frames.nbytes, np.uint8)), frames.reshape(-1))
    eng.render(src, 1, 16, 24, ok, first, dst, scale=2)                        # and the engine still works
    assert np.array_equal(dst.view(0, 12 * 8 * 3).download(np.empty(12 * 8 * 3, np.uint8)), host_render(frames, [[R.disc(1, 1, 1, 1)]], 2))
    whole.free()
    dst.free()


def test_a_frame_wider_than_the_jpeg_encoder_takes_goes_out_at_half_size(gpu_engine, tmp_path):
    """5120 x 32 at scale 2 is 2560 x 16: the Motion-JPEG encoder's widest frame.  The ``.avi`` holds ``mjpeg.encode_host`` of the
    twin's planes; 5136 x 32 gives 2568 x 16, which the sink refuses as it refuses any frame wider than 2560."""
    eng = gpu_engine
    w, h = 5120, 32
    frames = frames_of(2, h, w, seed=80)
    per_frame = [busy_marks(h, w, 2, 9, 8) + [R.segment(0, 31, 5119, 0, 3, 0x20C0FF), R.disc(5119, 16, 9, 0xFFFFFF)], [R.blend(2500, 0, 5119, 31, 0, 90)]]
    marks, first = R.pack(per_frame)
    with pytest.raises(ValueError, match="2560"):
        video.MjpegSink(tmp_path / "full.avi", w, h)
    with pytest.raises(ValueError, match="2560"):
        video.MjpegSink(tmp_path / "wider.avi", 5136 // 2, h // 2)
    src = eng.alloc(frames.nbytes).upload(frames)
    with video.MjpegSink(tmp_path / "half.avi", w // 2, h // 2, fps=30, quality=90) as sink:
        span = video.yuv_span(2, h // 2, w // 2, sink.desc)
        dst = eng.alloc(span)
        eng.render(src, 2, h, w, marks, first, dst, out=E.RENDER_YUV420, geom=sink.desc, enc=sink.enc, scale=2)
        assert eng.render_last_path() == E.RENDER_PATH_VECTOR
        planes = dst.download(np.empty(span, np.uint8))
        sink.write_device(dst, 2)
    want_planes = R.render_host(frames, marks, first, E.RENDER_YUV420, sink.desc, sink.enc, scale=2)
    assert np.array_equal(planes, want_planes)
    data, off = mjpeg.encode_host(want_planes, 2, h // 2, w // 2, sink.desc, 90)
    raw = (tmp_path / "half.avi").read_bytes()
    for i in range(2):
        jpg = data[off[i]:off[i + 1]].tobytes()
        assert jpg in raw, i
    assert sink.frames_written == 2
    src.free()
    dst.free()
