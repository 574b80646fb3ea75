"""The Motion-JPEG reader on the CPU (padel_analytics_amd/mjpeg.py ``parse_frame`` / ``decode_host`` / ``index_file``, csrc/jpeg_parse.cpp,
csrc/jpeg_entropy.h, csrc/jpeg_idct.h, ``video.MjpegClip``):

* ``decode_host`` gives Pillow's (libjpeg's) pixels byte for byte on streams of the project's own writer — every case of
  tests/mjpeg_cases.py, odd sizes, the same without their DHT segments — and of Pillow's encoder (default and optimised tables, restart
  intervals of one MCU row and of 3 MCUs, quality 1 / 50 / 95); every case keeps |IDCT output| below 384, where the specified clamp and
  libjpeg's wrapping table agree;
* the parser refuses what include/padel_hip.h says it refuses, each with its reason, in the twin and in the library alike, and both
  describe a well-formed stream in the same words; the interval table of a 3-MCU restart interval; COM and APP1 segments that carry a
  whole JPEG;
* the stand-alone program tests/jpeg_decode_main.cpp (g++ over the csrc files the kernels share) gives the twin's coefficients,
  statuses and pixels, and, rebuilt under the address and undefined-behaviour sanitizers, gets through some hundreds of seeded broken
  streams clean, refusing and flagging exactly what the twin refuses and flags;
* the containers: ``MjpegSink``'s ``.avi`` and ``.mjpeg`` read back, the roll-over followed, ``idx1`` cut off, odd- and zero-length
  chunks, an ``H264`` stream left to ``cv2``;
* the two ``video`` entry points and the runner over the stand-in engine from an ``.avi`` path."""
import functools
import io
import json
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

from padel_analytics_amd import engine as E
from padel_analytics_amd import mjpeg, video
from tests import mjpeg_cases as MC
from tests import synth

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
ODD_SIZES = [(17, 17), (33, 19), (31, 15), (1, 1), (49, 9)]                   # (w, h)
DHT_AT, DHT_BYTES = 2 + 18 + 134 + 19, 420                                  # the DHT segment inside mjpeg.frame_header


def pillow_bgr(jpeg: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))[..., ::-1]


def odd_stream(w, h, content, quality) -> bytes:
    """A frame of any size from the project's writer: planes of ceil size handed to ``mjpeg.encode_frame``."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if content == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        cy, cx = np.mgrid[0:ch, 0:cw]
        planes = ((7 * x + 3 * y) & 255, (5 * cx + 2 * cy + 60) & 255, 255 - ((3 * cx + 4 * cy) & 255))
    else:
        rng = np.random.default_rng([w, h, quality])
        planes = tuple(rng.integers(0, 256, s) for s in ((h, w), (ch, cw), (ch, cw)))
    return mjpeg.encode_frame(*(p.astype(np.uint8) for p in planes), quality)


def without_dht(jpeg: bytes) -> bytes:
    assert jpeg[DHT_AT:DHT_AT + 2] == b"\xff\xc4"
    return jpeg[:DHT_AT] + jpeg[DHT_AT + DHT_BYTES:]


def pillow_stream(w, h, quality=90, seed=0, **kw) -> bytes:
    """Pillow's own encoding (4:2:0) of smooth colour with noise on top: busy, and inside the range the IDCT precondition needs."""
    rng = np.random.default_rng([w, h, quality, seed])
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(3 * x + 2 * y) & 255, (x * y + 40) & 255, 255 - ((2 * x + 5 * y) & 255)], -1) // 2 + rng.integers(0, 128, (h, w, 3))
    out = io.BytesIO()
    Image.fromarray(img.astype(np.uint8)).save(out, "JPEG", quality=quality, subsampling=2, **kw)
    return out.getvalue()


@functools.lru_cache(maxsize=None)
def streams() -> dict:
    """name -> one well-formed JPEG: every stream the Pillow comparison runs on (built once, shared)."""
    out = {}
    for w, h in MC.SIZES:
        for content in MC.CONTENTS:
            data, offsets = MC.expected(content, w, h, "i420", 1)
            out[f"own_{w}x{h}_{content}"] = data[:int(offsets[1])].tobytes()
    for w, h in ODD_SIZES:
        out[f"own_{w}x{h}_noise_q90"] = odd_stream(w, h, "noise", 90)
        out[f"own_{w}x{h}_ramp_q50"] = odd_stream(w, h, "ramp", 50)
    for name in [k for k in out if k.startswith("own_")]:
        out["nodht_" + name[4:]] = without_dht(out[name])
    for w, h in [(48, 32), (33, 19), (1, 1)]:
        out[f"pil_{w}x{h}_default"] = pillow_stream(w, h)
        out[f"pil_{w}x{h}_optimize"] = pillow_stream(w, h, optimize=True)
        out[f"pil_{w}x{h}_rows1"] = pillow_stream(w, h, restart_marker_rows=1)
        for q in (1, 50, 95):
            out[f"pil_{w}x{h}_q{q}"] = pillow_stream(w, h, quality=q)
    out["pil_96x80_blocks3"] = pillow_stream(96, 80, restart_marker_blocks=3)                # 30 MCUs: 10 intervals
    out["pil_96x80_blocks3_optimize"] = pillow_stream(96, 80, restart_marker_blocks=3, optimize=True)
    out["pil_50x34_blocks3"] = pillow_stream(50, 34, restart_marker_blocks=3)                # 4 x 3 MCUs: intervals across MCU rows
    return out


STREAM_NAMES = sorted(streams())


# ---------------------------------------------------------------------------------------------- pixels
@pytest.mark.parametrize("name", STREAM_NAMES)
def test_decode_host_equals_pillow(name):
    jpeg = streams()[name]
    stats = {}
    got, status = mjpeg.decode_host_status(np.frombuffer(jpeg, np.uint8), [0, len(jpeg)], stats)
    print(name, "largest |IDCT output|", stats["max_abs_idct"])
    assert stats["max_abs_idct"] < 384                  # below it clamp and libjpeg's table agree
    assert status.tolist() == [0]
    want = pillow_bgr(jpeg)
    assert got.shape == (1,) + want.shape and got.dtype == np.uint8
    assert np.array_equal(got[0], want)


def test_streams_without_dht_decode_to_the_same_pixels():
    for name, jpeg in streams().items():
        if name.startswith("nodht_"):
            assert mjpeg.parse_frame(jpeg)["default_huffman"] == 1 and len(jpeg) == len(streams()["own_" + name[6:]]) - DHT_BYTES
            assert np.array_equal(mjpeg.decode_frame(jpeg)[0], mjpeg.decode_frame(streams()["own_" + name[6:]])[0])


def test_decode_host_of_several_frames_and_its_refusals():
    a, b = streams()["own_34x18_ramp"], streams()["own_34x18_noise_q1"]
    got = mjpeg.decode_host(np.frombuffer(a + b, np.uint8), [0, len(a), len(a) + len(b)])
    assert got.shape == (2, 18, 34, 3) and np.array_equal(got[1], pillow_bgr(b))
    c = streams()["own_16x16_ramp"]
    with pytest.raises(ValueError, match="frame 1.*sizes differ"):
        mjpeg.decode_host(np.frombuffer(a + c, np.uint8), [0, len(a), len(a) + len(c)])
    with pytest.raises(ValueError, match="frame 0.*no SOI"):
        mjpeg.decode_host(np.frombuffer(b"\0" * 8, np.uint8), [0, 8])


# ---------------------------------------------------------------------------------------------- the parser
def _segments(jpeg: bytes) -> dict:
    """marker -> offset of its FF, for the header of the project's writer."""
    out, pos = {}, 2
    while jpeg[pos + 1] != 0xda:
        out[jpeg[pos + 1]] = pos
        pos += 2 + (jpeg[pos + 2] << 8 | jpeg[pos + 3])
    out[0xda] = pos
    return out


def _patched(jpeg: bytes, at: int, new: bytes) -> bytes:
    return jpeg[:at] + new + jpeg[at + len(new):]


def refusals() -> dict:
    j = streams()["own_34x18_ramp"]
    s = _segments(j)
    sof, sos, dqt, dht = s[0xc0], s[0xda], s[0xdb], s[0xc4]
    scan = sos + 14
    return {
        "progressive": (_patched(j, sof + 1, b"\xc2"), "progressive"),
        "extended": (_patched(j, sof + 1, b"\xc1"), "extended"),
        "lossless": (_patched(j, sof + 1, b"\xc3"), "lossless"),
        "arithmetic": (_patched(j, sof + 1, b"\xc9"), "arithmetic"),
        "12-bit": (_patched(j, sof + 4, b"\x0c"), "12-bit"),
        "16-bit": (_patched(j, sof + 4, b"\x10"), "16-bit"),
        "16-bit DQT": (_patched(j, dqt + 4, b"\x10"), "16-bit quantisation"),
        "sampling": (_patched(j, sof + 11, b"\x21"), "sampling 2x1"),
        "4:4:4": (_patched(j, sof + 11, b"\x11"), "sampling 1x1"),
        "grey": (_patched(j, sof + 9, b"\x01"), "1 component"),
        "scan of one component": (j[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + j[scan:], "more than one scan"),
        "second scan": (j[:-2] + j[sos:], "more than one scan"),
        "spectral selection": (_patched(j, sos + 11, b"\x01"), "sequential scan"),
        "truncated in DHT": (j[:dht + 100], "truncated header"),
        "truncated before SOS": (j[:sos], "truncated header"),
        "truncated in SOS": (j[:sos + 6], "truncated header"),
        "missing DQT": (j[:dqt] + j[sof:], "missing table.*quantisation"),
        "missing chroma DQT": (_patched(j, sof + 15, b"\x02"), "missing table.*quantisation table 2"),
        "missing DHT table": (j[:dht + 2] + struct.pack(">H", 2 + 29 + 179 + 29) + j[dht + 4:dht + 4 + 29 + 179 + 29] + j[dht + DHT_BYTES:],
                              "missing table.*AC Huffman table 1"),
        "no SOI": (b"\x00" + j[1:], "no SOI"),
        "too large": (_patched(j, sof + 5, b"\x20\x00"), "outside 1"),
    }


@pytest.mark.parametrize("case", sorted(refusals()))
def test_parser_refuses(case):
    jpeg, reason = refusals()[case]
    with pytest.raises(ValueError, match=reason):
        mjpeg.parse_frame(jpeg)
    with pytest.raises(ValueError, match=reason):
        E.jpeg_parse(jpeg)


def _same_description(a: dict, b: dict) -> None:
    assert set(a) == set(b)
    for k in a:
        if k == "quant":
            assert np.array_equal(a[k], b[k])
        elif k in ("dc", "ac"):
            assert [(list(x), list(y)) for x, y in a[k]] == [(list(x), list(y)) for x, y in b[k]], k
        else:
            assert a[k] == b[k] or list(a[k]) == list(b[k]), k


@pytest.mark.parametrize("name", [n for n in STREAM_NAMES if "noise_q1" in n or "blocks3" in n or "optimize" in n or "q95" in n])
def test_library_and_twin_describe_a_frame_alike(name):
    jpeg = streams()[name]
    _same_description(mjpeg.parse_frame(jpeg), E.jpeg_parse(jpeg))


def test_interval_table_of_a_three_mcu_restart_interval():
    jpeg = streams()["pil_96x80_blocks3"]
    info = mjpeg.parse_frame(jpeg)
    assert (info["w"], info["h"], info["mcus_x"], info["mcus_y"], info["restart_interval"], info["n_intervals"]) == (96, 80, 6, 5, 3, 10)
    assert info["status"] == 0 and len(info["intervals"]) == 10
    at = info["scan_begin"]
    for k, (begin, end, first, mcus) in enumerate(info["intervals"]):
        assert (begin, first, mcus) == (at, 3 * k, 3) and end > begin
        assert jpeg[end:end + 2] == (bytes([0xff, 0xd0 + (k & 7)]) if k < 9 else b"\xff\xd9")      # RSTm wraps past 7
        at = end + 2
    assert info["scan_end"] == info["intervals"][-1][1] == len(jpeg) - 2
    # a stream without DRI is one interval over every MCU
    one = mjpeg.parse_frame(streams()["pil_48x32_default"])
    assert one["restart_interval"] == 0 and one["intervals"] == [(one["scan_begin"], one["scan_end"], 0, 6)]
    # the project's writer: one interval per MCU row, nine of them at 16 x 144
    own = mjpeg.parse_frame(streams()["own_16x144_ramp"])
    assert own["n_intervals"] == 9 and [v[2:] for v in own["intervals"]] == [(k, 1) for k in range(9)]


def test_com_and_app1_segments_with_a_whole_jpeg_inside_are_skipped():
    jpeg, thumb = streams()["pil_33x19_default"], streams()["own_16x16_ramp"]
    extra = b"\xff\xfe" + struct.pack(">H", 2 + len(thumb)) + thumb + b"\xff\xe1" + struct.pack(">H", 2 + 6 + len(thumb)) + b"Exif\0\0" + thumb
    both = jpeg[:2] + extra + jpeg[2:]
    a, b = mjpeg.parse_frame(jpeg), mjpeg.parse_frame(both)
    assert b["scan_begin"] == a["scan_begin"] + len(extra) and (b["w"], b["h"]) == (33, 19)
    _same_description(b, E.jpeg_parse(both))
    assert np.array_equal(mjpeg.decode_frame(both)[0], pillow_bgr(jpeg))
    # ... and do not split the frame when JPEGs stand back to back
    assert mjpeg.split_mjpeg(both + b"\0\0" + jpeg + both) == [(0, len(both)), (len(both) + 2, len(jpeg)), (len(both) + 2 + len(jpeg), len(both))]


# ---------------------------------------------------------------------------------------------- the stand-alone program
def build(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "jpeg_decode_main.cpp"),
                    str(CSRC / "jpeg_parse.cpp"), "-o", str(out)], check=True)
    return out


def run_program(exe: Path, jpegs: list, tmp: Path) -> list:
    """Per stream: None if the program refused it, else (status, w, h, intervals, coefficients, BGR)."""
    src, dst = tmp / "in.bin", tmp / "out.bin"
    src.write_bytes(b"".join(struct.pack("<I", len(j)) + j for j in jpegs))
    done = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr[-4000:]
    raw, at, out = dst.read_bytes(), 0, []
    for _ in jpegs:
        refused, status, w, h, ivls, ncoef = struct.unpack_from("<5iq", raw, at)
        at += 28
        if refused:
            out.append(None)
            continue
        coef = np.frombuffer(raw, np.int16, ncoef, at)
        at += 2 * ncoef
        out.append((status, w, h, ivls, coef, np.frombuffer(raw, np.uint8, h * w * 3, at).reshape(h, w, 3)))
        at += h * w * 3
    assert at == len(raw)
    return out


def twin_answer(jpeg: bytes):
    try:
        info = mjpeg.parse_frame(jpeg)
    except ValueError:
        return None
    coef, status = mjpeg.frame_coefficients_of(jpeg, info)
    return status, info["w"], info["h"], info["n_intervals"], coef.reshape(-1), mjpeg.decode_frame(jpeg)[0]


def same_answers(got: list, jpegs: list, names: list) -> None:
    for g, j, name in zip(got, jpegs, names):
        want = twin_answer(j)
        assert (g is None) == (want is None), name
        if g is not None:
            assert g[:4] == want[:4], (name, g[:4], want[:4])
            assert np.array_equal(g[4], want[4]), name
            assert np.array_equal(g[5], want[5]), name


def test_program_gives_the_twins_coefficients_statuses_and_pixels(tmp_path):
    exe = build(tmp_path / "jpeg_decode_main")
    names = [n for n in STREAM_NAMES if not n.startswith("own_1280")]
    jpegs = [streams()[n] for n in names]
    got = run_program(exe, jpegs, tmp_path)
    assert all(g is not None and g[0] == 0 for g in got)
    same_answers(got, jpegs, names)


def broken_streams() -> tuple:
    """Some hundreds of seeded damaged streams: cut at every kind of place, entropy bytes replaced by noise, single bit flips in
    header and scan, a DRI that lies."""
    rng = np.random.default_rng(20250)
    bases = {n: streams()[n] for n in ("own_34x18_noise_q100", "pil_48x32_optimize", "pil_50x34_blocks3", "pil_33x19_rows1", "nodht_16x144_ramp")}
    names, out = [], []

    def add(name, j):
        names.append(name)
        out.append(bytes(j))

    for n, j in bases.items():
        info = mjpeg.parse_frame(j)
        begin, end = info["scan_begin"], info["scan_end"]
        seg = _segments(j) if n.startswith(("own", "nodht")) else {}
        cuts = {0, 1, 2, 3, 4, 5, 20, begin - 1, begin, begin + 1, begin + 2, (begin + end) // 2, end - 1, end, end + 1, len(j) - 1}
        cuts |= {at + d for at in seg.values() for d in (0, 1, 2, 3, 4, 9)} | {v[1] + d for v in info["intervals"][:3] for d in (0, 1, 2)}
        cuts |= set(rng.integers(0, len(j), 12).tolist())
        for c in sorted(c for c in cuts if 0 <= c < len(j)):
            add(f"{n} cut at {c}", j[:c])
        for k in range(10):                              # a run of entropy bytes replaced by noise
            a = int(rng.integers(begin, end))
            b = min(end, a + int(rng.integers(1, 40)))
            add(f"{n} noise {a}:{b}", j[:a] + rng.integers(0, 256, b - a, dtype=np.uint8).tobytes() + j[b:])
        add(f"{n} all noise", j[:begin] + rng.integers(0, 256, end - begin, dtype=np.uint8).tobytes() + j[end:])
        add(f"{n} all ones", j[:begin] + b"\xff" * (end - begin) + j[end:])
        add(f"{n} all zeros", j[:begin] + bytes(end - begin) + j[end:])
        for k in range(24):                              # single bit flips: 16 in the scan, 8 in the header
            at = int(rng.integers(begin, end)) if k < 16 else int(rng.integers(2, begin))
            add(f"{n} bit {at}", _patched(j, at, bytes([j[at] ^ 1 << int(rng.integers(0, 8))])))
        dri = j.find(b"\xff\xdd\x00\x04")
        for ri in (0, 1, 2, 5, 1000, 65535):             # a DRI that lies (or one where there was none)
            if dri >= 0:
                add(f"{n} DRI {ri}", _patched(j, dri + 4, struct.pack(">H", ri)))
            elif ri:
                sos = j.rfind(b"\xff\xda", 0, begin)
                add(f"{n} DRI {ri} added", j[:sos] + b"\xff\xdd\x00\x04" + struct.pack(">H", ri) + j[sos:])
    return names, out


def test_program_under_the_sanitizers_gets_through_broken_streams_as_the_twin_does(tmp_path):
    exe = build(tmp_path / "jpeg_decode_main_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    names, jpegs = broken_streams()
    assert len(jpegs) > 300
    got = run_program(exe, jpegs, tmp_path)              # exit status 0 and nothing on stderr: no report from either sanitizer
    refused = sum(g is None for g in got)
    flagged = sum(g is not None and g[0] != 0 for g in got)
    print(f"{len(jpegs)} broken streams: {refused} refused, {flagged} flagged, {len(jpegs) - refused - flagged} decoded without a complaint")
    assert refused > 30 and flagged > 100
    for bit in (mjpeg.ST_CODE, mjpeg.ST_INDEX, mjpeg.ST_DATA, mjpeg.ST_MARKERS):      # every kind of complaint occurs
        assert any(g is not None and g[0] & bit for g in got), bit
    same_answers(got, jpegs, names)                      # refuses what the twin refuses, flags what it flags, the same coefficients


def test_a_damaged_frame_is_reported_not_raised():
    j = streams()["pil_33x19_rows1"]
    info = mjpeg.parse_frame(j)
    begin, end = info["intervals"][1][:2]
    bad = j[:begin] + b"\xff" * (end - begin) + j[end:]
    clip = video.MjpegClip(j + bad + j, on_device=False)
    assert clip.total_frames == 3
    with pytest.warns(RuntimeWarning, match="frame 1 is damaged"):
        frames = video.host_batch(list(clip.frames()))
    assert list(clip.corrupt) == [1] and clip.corrupt[1] & mjpeg.ST_DATA
    good = pillow_bgr(j)
    assert np.array_equal(frames[0], good) and np.array_equal(frames[2], good)
    assert np.array_equal(frames[1][:15], good[:15])     # the interval above the damaged one is whole (row 15 interpolates chroma row 8, the damaged one's)
    assert not np.array_equal(frames[1][16:], good[16:])


# ---------------------------------------------------------------------------------------------- containers
def _yuv(frames: np.ndarray):
    n, h, w = frames.shape[:3]
    desc = video.yuv_desc(w, h, "i420", "bt601", "full")
    return video.bgr_to_yuv420_host(frames, desc, video.YUV_ENC_COEFFS["bt601_full"]), desc


def write_clip(path, frames: np.ndarray, fps=25, quality=90, **kw) -> tuple:
    """``frames`` through ``MjpegSink`` on the host -> (the paths written, the JPEGs, one ``bytes`` per frame)."""
    n, h, w = frames.shape[:3]
    raw, desc = _yuv(frames)
    with video.MjpegSink(path, w, h, fps=fps, quality=quality, on_device=False, **kw) as sink:
        sink.write_host(raw, n)
    data, offsets = mjpeg.encode_host(raw, n, h, w, desc, quality)
    return sink.paths, [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(n)]


def test_avi_of_the_sink_reads_back(tmp_path):
    frames = synth.synthetic_frames(5, 18, 34, seed=3)
    paths, jpegs = write_clip(str(tmp_path / "a.avi"), frames, fps=25)
    idx = mjpeg.index_file(paths[0])
    assert (len(idx), idx.fps, idx.w, idx.h, idx.paths) == (5, 25, 34, 18, paths)
    assert [idx.read(i) for i in range(5)] == jpegs
    data, offsets = idx.batch(1, 3)
    assert data.tobytes() == b"".join(jpegs[1:4]) and offsets.tolist() == np.cumsum([0] + [len(j) for j in jpegs[1:4]]).tolist()


def test_roll_over_is_followed_through_its_parts(tmp_path):
    frames = synth.synthetic_frames(7, 16, 16, seed=4)
    size = len(write_clip(str(tmp_path / "probe.avi"), frames[:1])[1][0])
    paths, jpegs = write_clip(str(tmp_path / "b.avi"), frames, max_riff_bytes=224 + 3 * (size + 40))
    assert len(paths) >= 3 and paths[1].endswith("b.part002.avi")
    idx = mjpeg.index_file(paths[0])
    assert idx.paths == paths and [idx.read(i) for i in range(len(idx))] == jpegs
    assert len(mjpeg.index_file(paths[1])) < 7          # a part opened by itself is just that part


def test_avi_without_idx1_with_odd_and_empty_chunks(tmp_path):
    frames = synth.synthetic_frames(4, 18, 34, seed=5)
    paths, jpegs = write_clip(str(tmp_path / "c.avi"), frames)
    raw = Path(paths[0]).read_bytes()
    cut = raw[:raw.rfind(b"idx1")]
    (tmp_path / "noidx.avi").write_bytes(cut)
    assert [mjpeg.index_file(tmp_path / "noidx.avi").read(i) for i in range(4)] == jpegs
    # cut inside the last chunk, sizes never patched in: what a killed writer leaves
    dead = bytearray(cut[:-7])
    dead[4:8] = dead[216:220] = bytes(4)
    (tmp_path / "dead.avi").write_bytes(dead)
    idx = mjpeg.index_file(tmp_path / "dead.avi")
    assert len(idx) == 4 and [idx.read(i) for i in range(3)] == jpegs[:3] and idx.read(3) == jpegs[3][:len(idx.read(3))]
    # by hand: an odd-length chunk (padded), a zero-length chunk (repeats the previous frame), a chunk of another stream, '00db'
    odd = jpegs[0] if len(jpegs[0]) & 1 else jpegs[0] + b"\0"
    assert len(odd) & 1
    chunk = lambda cid, body: cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    movi = b"movi" + chunk(b"00dc", odd) + chunk(b"01wb", b"abc") + chunk(b"00dc", b"") + chunk(b"00db", jpegs[1]) + chunk(b"00dc", b"")
    head = raw[12:212]                                   # the sink's hdrl list
    body = b"AVI " + head + b"LIST" + struct.pack("<I", len(movi)) + movi
    (tmp_path / "hand.avi").write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    idx = mjpeg.index_file(tmp_path / "hand.avi")
    assert [idx.read(i) for i in range(len(idx))] == [odd, odd, jpegs[1], jpegs[1]]
    assert np.array_equal(mjpeg.decode_frame(idx.read(0))[0], mjpeg.decode_frame(jpegs[0])[0])


def test_raw_mjpeg_is_split(tmp_path):
    frames = synth.synthetic_frames(3, 18, 34, seed=6)
    paths, jpegs = write_clip(str(tmp_path / "d.mjpeg"), frames)
    idx = mjpeg.index_file(paths[0])
    assert (len(idx), idx.fps, idx.w, idx.h) == (3, 30, 34, 18) and [idx.read(i) for i in range(3)] == jpegs
    (tmp_path / "e.mjpg").write_bytes(b"junk" + jpegs[2] + b"\0\xff\0 between \xff\xd9" + jpegs[0])
    idx = mjpeg.index_file(tmp_path / "e.mjpg")
    assert [idx.read(i) for i in range(len(idx))] == [jpegs[2], jpegs[0]]


def test_avi_with_another_codec_still_needs_cv2(tmp_path):
    paths, _ = write_clip(str(tmp_path / "f.avi"), synth.synthetic_frames(2, 16, 16, seed=7))
    raw = Path(paths[0]).read_bytes()
    assert raw.count(b"MJPG") == 2
    p = tmp_path / "h264.avi"
    p.write_bytes(raw.replace(b"MJPG", b"H264"))
    with pytest.raises(mjpeg.NotMjpeg, match="H264"):
        mjpeg.index_file(p)
    for call in (video.VideoInfo.from_video_path, lambda q: list(video.get_video_frames_generator(q))):
        with pytest.raises(RuntimeError, match="opencv-python.*Motion-JPEG"):
            call(str(p))
    with pytest.raises(RuntimeError, match="opencv-python"):
        video.VideoInfo.from_video_path(str(tmp_path / "missing.avi"))
    with pytest.raises(RuntimeError, match="opencv-python"):
        video.VideoInfo.from_video_path(str(tmp_path / "clip.mp4"))


# ---------------------------------------------------------------------------------------------- entry points and the runner
def test_paths_open_through_the_two_calls(tmp_path):
    frames = synth.synthetic_frames(7, 18, 34, seed=8)
    for name, fps in (("x.avi", 50), ("x.mjpeg", 30), ("x.mjpg", 30)):
        paths, jpegs = write_clip(str(tmp_path / name), frames, fps=50)
        p = paths[0]
        want = mjpeg.decode_host(np.frombuffer(b"".join(jpegs), np.uint8), np.cumsum([0] + [len(j) for j in jpegs]))
        info = video.VideoInfo.from_video_path(p)
        assert (info.width, info.height, info.fps, info.total_frames) == (34, 18, fps, 7)
        video._open_mjpeg(p).on_device = False           # (no GPU here; the path itself opens with on_device=True)
        got = list(video.get_video_frames_generator(p, start=1, end=6, stride=2))
        assert [f.index for f in got] == [1, 3, 5]
        for f in got:
            assert isinstance(f, video.MjpegFrame) and f.shape == (18, 34, 3) and np.array_equal(np.asarray(f), want[f.index])
        assert len(list(video.get_video_frames_generator(p))) == 7 and len(list(video.get_video_frames_generator(p, end=100))) == 7
        assert video.device_batch(got[:1]) is None and np.array_equal(video.host_batch(list(video.get_video_frames_generator(p))), want)
        assert video._open_mjpeg(p) is video._open_mjpeg(p)                # one clip per file ...
    write_clip(p, frames[:2])
    assert video.VideoInfo.from_video_path(p).total_frames == 2           # ... until the file changes
    # the clip object is a source too, with repeat; a non-contiguous device batch is refused
    clip = video.MjpegClip(str(tmp_path / "x.avi"), on_device=False, repeat=2)
    assert video.VideoInfo.from_video_path(clip).total_frames == 14 and clip.fps == 50
    assert [f.index for f in video.get_video_frames_generator(clip, start=5, end=9)] == [5, 6, 0, 1]
    f = list(video.MjpegClip(str(tmp_path / "x.avi")).frames())
    with pytest.raises(ValueError, match="contiguous"):
        video.device_batch([f[0], f[2]])


@pytest.fixture
def fake_engine(monkeypatch):
    from tests import fake_engine as F
    eng = F.FakeEngine(0)
    monkeypatch.setattr(E, "Engine", F.FakeEngine)
    monkeypatch.setattr(E, "Model", F.FakeModel)
    monkeypatch.setattr(E, "DeviceBuffer", F.FakeBuffer)
    monkeypatch.setattr(E, "default_engine", lambda *a, **k: eng)
    monkeypatch.setattr(F.FakeModel, "STEP_SECONDS", 0.0)
    return eng


@pytest.mark.parametrize("fanout", [False, True])
def test_player_tracker_over_the_stand_in_engine_avi_equals_bgr(fake_engine, tmp_path, fanout):
    from padel_analytics_amd import checkpoint, detections as D, yolo_arch
    from padel_analytics_amd.trackers import PlayerTracker, TrackingRunner
    h, w, n = 72, 128, 11
    paths, jpegs = write_clip(str(tmp_path / "rally.avi"), synth.synthetic_frames(n, h, w, seed=21))
    want_frames = mjpeg.decode_host(np.frombuffer(b"".join(jpegs), np.uint8), np.cumsum([0] + [len(j) for j in jpegs]))
    checkpoint.save_checkpoint(tmp_path / "players.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5), "detect", 80,
                               None, "n", {0: "person"})
    zone = D.PolygonZone(np.array([[4, 4], [124, 4], [124, 68], [4, 68]]), frame_resolution_wh=(w, h))

    def run(source):
        t = PlayerTracker(str(tmp_path / "players.pt"), zone, batch_size=4)       # 11 frames: 4 + 4 + 3
        TrackingRunner([t], source, tmp_path / "out.mp4", fanout=fanout).run()
        assert len(t) == n
        return json.dumps([o.serialize() for o in t.results])

    want = run(video.ArrayClip(want_frames))
    assert run(paths[0]) == want                                                  # by path: the stand-in has no jpeg_decode, the host decodes
    assert run(video.MjpegClip(paths[0], on_device=False)) == want
    assert want.count("[") > n                                                    # (there are detections to compare)
    assert run(video.ArrayClip(want_frames[::-1].copy())) != want
