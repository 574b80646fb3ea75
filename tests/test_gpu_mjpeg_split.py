"""The split entropy path of csrc/jpeg_decode.hip (``jpeg_entropy_split_kernel``, csrc/jpeg_entropy_split.h) against the numpy twin
``mjpeg.decode_host``, byte for byte: with ``jpeg_decode_set_split(min_bytes=1, sub_bytes=S)`` every interval of every frame takes it —
16 x 16 to 320 x 192, subsequences of 4, 8, 16 and 128 bytes, Pillow's streams without restart markers at quality 30 / 90 / 100 and
with optimised tables, a stream of the project's writer without DHT, restart intervals of 3 MCUs; every status word zero, the
sentinels around the destination intact, ``jpeg_decode_last_split()`` with the interval and subsequence counts the lengths give and
with the round count of the stand-alone program tests/jpeg_split_main.cpp for the same stream and S (the rounds depend on the data
only).  Then: a batch of frames with and without restart markers at the default threshold, 70 frames (more than one sub-batch),
``min_bytes=-1``, one MCU row at full width, and an ``.avi`` of frames without restart markers through ``video.MjpegClip``.
Well-formed streams only: damaged ones are the CPU test's, where the sanitizers watch."""
import functools

import numpy as np
import pytest

from padel_analytics_amd import engine as E
from padel_analytics_amd import mjpeg, video
from tests import mjpeg_cases as MC
from tests import test_mjpeg_decode_host as T
from tests import test_mjpeg_split_host as S
from tests.test_gpu_mjpeg_decode import decode

pytestmark = pytest.mark.gpu

SUB_BYTES = (4, 8, 16, 128)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {"pil_16x16_q90": T.pillow_stream(16, 16), "pil_34x18_q90": T.pillow_stream(34, 18), "pil_48x32_q30": T.pillow_stream(48, 32, quality=30),
           "pil_48x32_q90": T.pillow_stream(48, 32), "pil_48x32_q100": T.pillow_stream(48, 32, quality=100),
           "pil_48x32_optimize": T.pillow_stream(48, 32, optimize=True), "pil_320x192_q90": T.pillow_stream(320, 192),
           "pil_320x192_optimize": T.pillow_stream(320, 192, optimize=True), "nodht_34x18_noise_q100": T.streams()["nodht_34x18_noise_q100"],
           "pil_96x80_blocks3": T.streams()["pil_96x80_blocks3"], "crafted_16x16": S.crafted_stream()}
    return out


NAMES = sorted(cases())


@pytest.fixture(scope="module")
def program_answers(tmp_path_factory) -> dict:
    """name -> {S: counts} of the stand-alone program: one build, one run."""
    tmp = tmp_path_factory.mktemp("split_gpu")
    got = S.run_program(S.build(tmp / "jpeg_split_main"), [cases()[n] for n in NAMES], SUB_BYTES, tmp)
    return dict(zip(NAMES, got))


@pytest.fixture
def eng(gpu_engine):
    """The shared engine, handed back with the default split settings."""
    try:
        yield gpu_engine
    finally:
        gpu_engine.jpeg_decode_set_split(0, 0)


def expected_counts(jpegs: list, min_bytes: int, sub_bytes: int) -> tuple:
    """(intervals on the split path, their subsequences, intervals on the serial path) from the interval lengths."""
    split = subs = serial = 0
    for j in jpegs:
        for begin, end, _, mcus in mjpeg.parse_frame(j)["intervals"]:
            n = end - begin
            if min_bytes >= 0 and n > 0 and n >= min_bytes and mcus > 0:
                eff = max(sub_bytes, (-(-n // 4096) + 3) // 4 * 4)
                split, subs = split + 1, subs + -(-n // eff)
            else:
                serial += 1
    return split, subs, serial


@pytest.mark.parametrize("sub_bytes", SUB_BYTES)
@pytest.mark.parametrize("name", NAMES)
def test_split_kernel_equals_the_twin(eng, program_answers, name, sub_bytes):
    jpeg = cases()[name]
    eng.jpeg_decode_set_split(1, sub_bytes)
    got, status, want, _ = decode(eng, [jpeg], shift=16)
    report = eng.jpeg_decode_last_split()
    print(name, sub_bytes, report)
    assert status.tolist() == [0]
    assert np.array_equal(got, want)
    split, subs, serial = expected_counts([jpeg], 1, sub_bytes)
    prog = program_answers[name][sub_bytes]
    assert split == prog["intervals"] and subs == prog["subsequences"] and serial == 0
    assert report == {"split": split, "subsequences": subs, "rounds": prog["rounds"], "serial": 0}


def test_mixed_batch_at_the_default_threshold(eng):
    """Frames of the writer (one interval per MCU row, short) and of Pillow (none: one long interval) in one call."""
    w, h = 320, 192
    own = [mjpeg.encode_frame(*MC.planes("ramp", w, h, i), 90) for i in range(2)]
    pil = [T.pillow_stream(w, h, seed=s) for s in range(2)]
    jpegs = [own[0], pil[0], pil[1], own[1]]
    got, status, want, _ = decode(eng, jpegs)
    report = eng.jpeg_decode_last_split()
    print(report)
    assert not status.any() and np.array_equal(got, want)
    assert all(len(S.entropy_bytes(j)) >= E.JPEG_DEC_SPLIT_MIN_BYTES for j in pil)
    assert all(v[1] - v[0] < E.JPEG_DEC_SPLIT_MIN_BYTES for j in own for v in mjpeg.parse_frame(j)["intervals"])
    assert report["split"] == 2 and report["serial"] == 2 * 12 and report["rounds"] >= 1
    assert (report["split"], report["subsequences"], report["serial"]) == expected_counts(jpegs, E.JPEG_DEC_SPLIT_MIN_BYTES, E.JPEG_DEC_SPLIT_SUB_BYTES)


def test_seventy_frames_on_the_split_path_are_more_than_one_sub_batch(eng):
    jpegs = [T.pillow_stream(48, 32, quality=50 + i % 50, seed=i) for i in range(70)]
    eng.jpeg_decode_set_split(1, 16)
    got, status, want, _ = decode(eng, jpegs)
    report = eng.jpeg_decode_last_split()
    assert not status.any() and np.array_equal(got, want)
    assert len({got[i].tobytes() for i in range(70)}) == 70
    split, subs, serial = expected_counts(jpegs, 1, 16)
    assert (report["split"], report["subsequences"], report["serial"]) == (70, subs, 0) and split == 70


def test_never_split_is_the_serial_kernel_for_every_interval(eng):
    jpegs = [T.pillow_stream(320, 192), T.pillow_stream(320, 192, optimize=True)]
    eng.jpeg_decode_set_split(-1, 0)
    got, status, want, _ = decode(eng, jpegs)
    assert eng.jpeg_decode_last_split() == {"split": 0, "subsequences": 0, "rounds": 0, "serial": 2}
    assert not status.any() and np.array_equal(got, want)
    eng.jpeg_decode_set_split(1, 0)
    again, status, _, _ = decode(eng, jpegs)
    assert eng.jpeg_decode_last_split()["split"] == 2 and not status.any() and np.array_equal(again, got)


def test_one_mcu_row_at_full_width(eng):
    jpeg = T.pillow_stream(1280, 16)
    eng.jpeg_decode_set_split(1, 128)
    got, status, want, _ = decode(eng, [jpeg])
    report = eng.jpeg_decode_last_split()
    assert status.tolist() == [0] and np.array_equal(got, want)
    assert (report["split"], report["serial"]) == (1, 0) and report["subsequences"] == -(-len(S.entropy_bytes(jpeg)) // 128)


def test_set_split_refusals_leave_the_settings(eng):
    eng.jpeg_decode_set_split(1, 8)
    for args, reason in (((-2, 0), "min_bytes = -2"), ((0, 6), "not a multiple of 4"), ((0, 65536), "outside 4 .. 32768")):
        with pytest.raises(E.EngineError, match=reason):
            eng.jpeg_decode_set_split(*args)
    jpeg = T.pillow_stream(48, 32)
    decode(eng, [jpeg])
    assert eng.jpeg_decode_last_split()["subsequences"] == -(-len(S.entropy_bytes(jpeg)) // 8)


def test_avi_of_frames_without_restart_markers_through_the_clip(eng, tmp_path):
    w, h, n = 320, 192, 5
    jpegs = [T.pillow_stream(w, h, seed=s) for s in range(n)]
    data = np.frombuffer(b"".join(jpegs), np.uint8)
    offsets = np.cumsum([0] + [len(j) for j in jpegs])
    with video.MjpegSink(str(tmp_path / "phone.avi"), w, h, fps=30, on_device=False) as sink:
        sink.write_jpegs(data, offsets)
    want = mjpeg.decode_host(data, offsets)
    clip = video.MjpegClip(sink.paths[0], engine=eng)
    try:
        assert (clip.n, clip.w, clip.h) == (n, w, h)
        dev = video.device_batch(list(clip.frames()))
        got = dev[0].download(np.empty((n, h, w, 3), np.uint8))
        assert np.array_equal(got, want) and not clip.corrupt
        report = eng.jpeg_decode_last_split()
        assert report["split"] == n and report["serial"] == 0
    finally:
        clip.free()
