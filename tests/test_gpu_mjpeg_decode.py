"""csrc/jpeg_decode.hip against its numpy twin ``mjpeg.decode_host``, byte for byte (which tests/test_mjpeg_decode_host.py pins to Pillow's
pixels on the CPU): sizes from one pixel to partial MCUs on both edges, nine intervals and one interval at full width; restart intervals
per MCU row, none at all and of 3 MCUs; Annex K, optimised and absent Huffman tables; a batch whose frames differ in tables and quality;
more than 64 intervals and more than one sub-batch; a destination at an offset between sentinels, on the vector and on the byte path;
every status word zero; and the round trip ``jpeg_encode`` -> ``jpeg_decode`` on the device.  Well-formed streams only: damaged ones are
the CPU test's, where the sanitizers watch."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E
from padel_analytics_amd import mjpeg, video
from tests import mjpeg_cases as MC
from tests import test_mjpeg_decode_host as T

pytestmark = pytest.mark.gpu

SENTINEL = 0xa5


def decode(eng, jpegs: list, shift: int = 0):
    """(the frames ``Engine.jpeg_decode`` writes, status, what ``decode_host`` gives, the path the colour pass took); ``shift``: the
    destination starts that many bytes into its buffer; the bytes around it must stay as they were."""
    data = np.frombuffer(b"".join(jpegs), np.uint8)
    offsets = np.cumsum([0] + [len(j) for j in jpegs])
    want = mjpeg.decode_host(data, offsets)
    n, h, w = want.shape[:3]
    size = n * h * w * 3
    buf = eng.alloc(shift + size + 64)
    try:
        buf.upload(np.full(shift + size + 64, SENTINEL, np.uint8))
        status = eng.jpeg_decode(data, offsets, buf.view(shift, size))
        back = buf.download(np.empty(shift + size + 64, np.uint8))
    finally:
        buf.free()
    assert np.all(back[:shift] == SENTINEL) and np.all(back[shift + size:] == SENTINEL), "bytes outside the destination were written"
    return back[shift:shift + size].reshape(n, h, w, 3), status, want, eng.jpeg_decode_last_path()


@pytest.mark.parametrize("size", MC.SIZES + [(1, 1), (17, 17), (33, 19)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_the_twin_on_the_writers_streams(gpu_engine, size):
    """Restart interval = one MCU row, Annex K tables in a DHT and without any: every content of tests/mjpeg_cases.py in one batch."""
    w, h = size
    if size in MC.SIZES:
        jpegs = [T.streams()[f"own_{w}x{h}_{c}"] for c in MC.CONTENTS]
    else:
        jpegs = [T.streams()[f"own_{w}x{h}_noise_q90"], T.streams()[f"own_{w}x{h}_ramp_q50"]]
    jpegs = jpegs + [T.without_dht(j) for j in jpegs]
    got, status, want, path = decode(gpu_engine, jpegs)
    assert status.tolist() == [0] * len(jpegs)
    assert np.array_equal(got, want)
    assert path == (E.JPEG_DEC_PATH_VECTOR if w % 16 == 0 else E.JPEG_DEC_PATH_BYTE)


@pytest.mark.parametrize("name", [n for n in T.STREAM_NAMES if n.startswith("pil_")])
def test_kernels_equal_the_twin_on_pillows_streams(gpu_engine, name):
    """No restart markers (one wave decodes the frame), one MCU row, 3 MCUs (intervals across MCU rows); optimised tables; quality 1 .. 95."""
    got, status, want, _ = decode(gpu_engine, [T.streams()[name]])
    assert status.tolist() == [0] and np.array_equal(got, want)


def test_a_batch_whose_frames_differ_in_tables_and_quality(gpu_engine):
    jpegs = [T.pillow_stream(48, 32, quality=30), T.pillow_stream(48, 32, quality=95, optimize=True),
             T.pillow_stream(48, 32, quality=60, restart_marker_blocks=3), mjpeg.encode_frame(*MC.planes("noise_q1", 48, 32, 0), 70),
             T.without_dht(mjpeg.encode_frame(*MC.planes("ramp", 48, 32, 1), 100))]
    assert len({mjpeg.parse_frame(j)["quant"].tobytes() for j in jpegs}) == 5
    got, status, want, path = decode(gpu_engine, jpegs)
    assert status.tolist() == [0] * 5 and np.array_equal(got, want) and path == E.JPEG_DEC_PATH_VECTOR


def test_seventy_frames_are_more_than_one_sub_batch(gpu_engine):
    """70 frames of 16 x 16: more than 64 intervals, and the second sub-batch (frames 64 ..) reuses the scratch of the first."""
    jpegs = [mjpeg.encode_frame(*MC.planes("noise_q100" if i % 2 else "ramp", 16, 16, i), 50 + i % 50) for i in range(70)]
    got, status, want, _ = decode(gpu_engine, jpegs)
    assert not status.any() and np.array_equal(got, want)
    assert len({got[i].tobytes() for i in range(70)}) == 70


@pytest.mark.parametrize("w", [32, 30, 34, 16, 15])
def test_vector_and_byte_path_meet_at_a_multiple_of_sixteen(gpu_engine, w):
    """The colour pass stores 16 bytes at a time iff the width is a multiple of 16 and the destination 16-byte aligned; a view at an
    offset takes the byte path, and either way the sentinels before and after stay."""
    jpegs = [T.pillow_stream(w, 18, seed=s, restart_marker_rows=1) for s in (1, 2, 3)]
    for shift in (0, 16, 48 * 18, 1, 8, 3 * w):
        vector = w % 16 == 0 and shift % 16 == 0
        got, status, want, path = decode(gpu_engine, jpegs, shift)
        assert not status.any() and np.array_equal(got, want), (w, shift)
        assert path == (E.JPEG_DEC_PATH_VECTOR if vector else E.JPEG_DEC_PATH_BYTE), (w, shift)


def test_round_trip_on_the_device(gpu_engine):
    """``jpeg_encode`` of YUV frames in HBM, then ``jpeg_decode`` of those bytes: ``decode_host(encode_host(...))``."""
    for (w, h), content in (((34, 18), "noise_q100"), ((16, 144), "ramp"), ((1280, 16), "noise_q1")):
        raw, desc = MC.raw_frames(content, w, h, "nv12", 2, 0x5a)
        src = gpu_engine.alloc(raw.size)
        dst = gpu_engine.alloc(2 * h * w * 3)
        try:
            src.upload(raw)
            data, offsets = gpu_engine.jpeg_encode(src, 2, h, w, desc, MC.CONTENTS[content])
            want_data, want_offsets = MC.expected(content, w, h, "nv12", 2)
            assert data.tobytes() == want_data.tobytes() and offsets.tolist() == want_offsets.tolist()
            status = gpu_engine.jpeg_decode(data, offsets, dst)
            got = dst.download(np.empty((2, h, w, 3), np.uint8))
        finally:
            src.free()
            dst.free()
        assert not status.any() and np.array_equal(got, mjpeg.decode_host(want_data, want_offsets)), (w, h, content)


def test_refusals_launch_nothing(gpu_engine):
    a, b = T.streams()["own_34x18_ramp"], T.streams()["own_16x16_ramp"]
    buf = gpu_engine.alloc(2 * 18 * 34 * 3)
    try:
        buf.upload(np.full(buf.nbytes, SENTINEL, np.uint8))
        for jpegs, reason in (([a, b], "frame 1 is 16 x 16.*sizes differ"), ([a, T.refusals()["progressive"][0]], "frame 1.*progressive"),
                              ([a, a[:300]], "frame 1.*truncated header")):
            data = np.frombuffer(b"".join(jpegs), np.uint8)
            with pytest.raises(E.EngineError, match=reason):
                gpu_engine.jpeg_decode(data, np.cumsum([0] + [len(j) for j in jpegs]), buf)
        with pytest.raises(E.EngineError, match="dst holds"):
            gpu_engine.jpeg_decode(np.frombuffer(a * 3, np.uint8), [0, len(a), 2 * len(a), 3 * len(a)], buf)
        assert np.all(buf.download(np.empty(buf.nbytes, np.uint8)) == SENTINEL)
    finally:
        buf.free()


def test_clip_staging_decodes_a_held_range_once(gpu_engine):
    jpegs = [T.pillow_stream(48, 32, seed=s) for s in range(6)]
    want = mjpeg.decode_host(np.frombuffer(b"".join(jpegs), np.uint8), np.cumsum([0] + [len(j) for j in jpegs]))
    clip = video.MjpegClip(b"".join(jpegs), engine=gpu_engine)
    try:
        assert (clip.n, clip.w, clip.h, clip.fps) == (6, 48, 32, 30)
        f = list(clip.frames())
        down = lambda dev: dev[0].download(np.empty((dev[1], dev[2], dev[3], 3), np.uint8))
        assert np.array_equal(down(video.device_batch(f[:4])), want[:4]) and clip.decodes == 1
        assert np.array_equal(down(video.device_batch(f[1:3])), want[1:3]) and clip.decodes == 1      # held: nothing decoded
        assert np.array_equal(down(video.device_batch(f[2:6])), want[2:6]) and clip.decodes == 2
        assert np.array_equal(down(video.device_batch(f)), want) and clip.decodes == 3                # the staging grew
        assert np.array_equal(np.asarray(f[5]), want[5]) and not clip.corrupt
    finally:
        clip.free()
