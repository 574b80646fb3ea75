"""The Motion-JPEG writer without a GPU: the bit stream ``include/padel_hip.h`` specifies for ``pa_jpeg_encode``, as its numpy twin
``mjpeg.encode_host`` states it (tests/test_gpu_mjpeg.py pins the kernels to that twin byte for byte).

* the tables of csrc/jpeg_tables.h, printed by the stand-alone program tests/jpeg_tables_main.cpp (g++; once more under the address and
  undefined-behaviour sanitizers), are the twin's, prefix-free and complete, and the quality rule gives the hand-computed values;
* the integer DCT and the quantisation agree with an fp64 DCT up to the integer transform's own rounding (``DCT_ERR``, derived below);
* Pillow (libjpeg) decodes every frame of every case of tests/mjpeg_cases.py to the true size as 4:2:0 without a warning — and to
  EXACTLY the pixels it decodes from its own encoding of the same planes at the same quality (the forward DCT, the tables and the
  quantisation are libjpeg's, bit for bit), so the mean squared error against the source is Pillow's own; the byte count stays within
  the margin of profiles/mjpeg_parity.txt;
* the ``.mjpeg`` and ``.avi`` containers of ``video.MjpegSink`` read back with a small RIFF walker, the AVI roll-over included;
* one refusal per reason of ``pa_jpeg_check``; the runner picks its sink by suffix."""
import io
import struct
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest
import scipy.fft
from PIL import Image

from padel_analytics_amd import engine as E, mjpeg, video
from padel_analytics_amd.trackers import TrackingRunner
from tests import mjpeg_cases as MC
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)
from tests.court_script import stub_trackers

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"


def build(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "jpeg_tables_main.cpp"),
                    str(CSRC / "jpeg_check.cpp"), "-o", str(out)], check=True)
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("jpeg_tables") / "jpeg_tables_main")


def run(exe, *args) -> str:
    done = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    return done.stdout


# ---------------------------------------------------------------------------------------------- tables
def printed_tables(exe):
    tables, zigzag = {}, None
    for line in run(exe, "tables").splitlines():
        name, *nums = line.split()
        if name == "zigzag":
            zigzag = [int(v) for v in nums]
        else:
            tables.setdefault(name, {})[int(nums[0])] = (int(nums[1]), int(nums[2]))
    return tables, zigzag


def test_the_huffman_tables_are_prefix_free_complete_and_the_twins(program):
    tables, zigzag = printed_tables(program)
    assert zigzag == mjpeg.ZIGZAG.tolist() and sorted(zigzag) == list(range(64))
    # zig-zag walks the anti-diagonals in turn, alternating direction
    assert [(i // 8 + i % 8) for i in zigzag] == sorted(i // 8 + i % 8 for i in range(64))
    specs = {"dc_luma": mjpeg.DC_LUMA, "dc_chroma": mjpeg.DC_CHROMA, "ac_luma": mjpeg.AC_LUMA, "ac_chroma": mjpeg.AC_CHROMA}
    ac_symbols = {0x00, 0xf0} | {r << 4 | s for r in range(16) for s in range(1, 11)}
    assert set(tables) == set(specs)
    for name, spec in specs.items():
        got = tables[name]
        assert set(got) == (set(range(12)) if name.startswith("dc") else ac_symbols), name
        code, length = mjpeg.huff_codes(spec)
        assert all(got[s] == (code[s], length[s]) for s in got), name
        assert sum(spec[0]) == len(spec[1]) == len(got)
        words = sorted(format(c, f"0{n}b") for c, n in got.values())
        assert len(set(words)) == len(words)
        assert not any(b.startswith(a) for a, b in zip(words, words[1:])), name       # sorted: a prefix sorts right before
        assert all(1 <= n <= 16 for _, n in got.values())
        # complete per T.81: the Kraft sum misses 1 by exactly the all-ones code word of the longest length, which is reserved
        longest = max(n for _, n in got.values())
        assert sum(2 ** (16 - n) for _, n in got.values()) == 2 ** 16 - 2 ** (16 - longest), name
        assert "1" * longest not in words


def by_hand(base, q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_the_quality_rule(program, q):
    luma, chroma = mjpeg.quant_tables(q)
    assert luma.tolist() == by_hand(mjpeg.QUANT_LUMA.tolist(), q) and chroma.tolist() == by_hand(mjpeg.QUANT_CHROMA.tolist(), q)
    lines = dict((ln.split()[0], [int(v) for v in ln.split()[1:]]) for ln in run(program, "quant", q).splitlines())
    assert lines == {"luma": luma.tolist(), "chroma": chroma.tolist()}
    # by hand: Q 1 -> s = 5000, every entry beyond 255; Q 50 -> s = 100, the Annex K tables themselves; Q 100 -> s = 0, all ones;
    # Q 90 -> s = 20: 16 -> (320 + 50) / 100 = 3, 11 -> 2, 10 -> 2, 99 -> 20, 17 -> 3
    if q == 1:
        assert set(luma) == set(chroma) == {255}
    if q == 50:
        assert luma.tolist() == mjpeg.QUANT_LUMA.tolist() and chroma.tolist() == mjpeg.QUANT_CHROMA.tolist()
    if q == 100:
        assert set(luma) == set(chroma) == {1}
    if q == 90:
        assert luma[:3].tolist() == [3, 2, 2] and chroma[0] == 3 and chroma[-1] == 20 and luma[63] == 20


def test_the_header_and_the_capacity_are_the_twins(program, tmp_path):
    run(program, "header", 18, 34, 77, tmp_path / "h.bin")
    assert (tmp_path / "h.bin").read_bytes() == mjpeg.frame_header(18, 34, 77)
    for w in (2, 16, 18, 1280, 2560):
        assert int(run(program, "bound", w)) == mjpeg.interval_max_bytes(w) == E.jpeg_interval_bytes(w)


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build(tmp_path / "jpeg_tables_asan", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
    assert run(exe, "tables").count("\n") == 2 * 12 + 2 * 162 + 1
    for q in (1, 50, 100):
        run(exe, "quant", q)
    blocks = dct_blocks()
    blocks.tofile(tmp_path / "in.bin")
    run(exe, "blocks", 100, 0, tmp_path / "in.bin", tmp_path / "out.bin")
    got = np.fromfile(tmp_path / "out.bin", np.int16).reshape(-1, 8, 8)
    assert np.array_equal(got, mjpeg.quantise_blocks(blocks, mjpeg.quant_tables(100)[0]))
    run(exe, "header", 65534, 2560, 1, tmp_path / "h.bin")
    run(exe, "bound", 2560)


# ---------------------------------------------------------------------------------------------- DCT and quantisation
def dct_blocks():
    """Noise, the extremes, ramps and every basis function at full swing."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:8, 0:8]
    out = [rng.integers(0, 256, (200, 8, 8)), np.zeros((1, 8, 8)), np.full((1, 8, 8), 255), (x * 36)[None], (y * 36)[None], ((x + y) * 18)[None],
           np.where((x + y) % 2, 255, 0)[None], np.where(x < 4, 0, 255)[None]]
    c = np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)
    out.append(np.array([np.rint(127.5 + 127.5 * np.sign(np.outer(c[u], c[v]))) for u in range(8) for v in range(8)]))
    return np.concatenate(out).astype(np.uint8)


# What the integer transform may differ from the exact one by, in units of its output (the exact DCT scaled by 8).  Constants carry
# 13 fractional bits, so each is off by at most 0.5 / 2^13.
#   row pass (results scaled by 4, descale by 11 bits): a rounding of 0.5, plus the constants: an odd output adds products over
#     t7, t4 + t7, t5 + t7 and t4 + t5 + t6 + t7, differences of samples of at most 255 each: (1 + 2 + 2 + 4) * 255 * 0.5 / 2^11
#   column pass (descale by 15 bits): its inputs are at most 4 * 8 * 128 + 1 (the DC sum) in magnitude, their differences twice that;
#     the same nine-fold sum gives 9 * 2 * 4097 * 0.5 / 2^15; a rounding of 0.5; and the row pass's error arrives through a transform
#     whose coefficients sum to at most 8 in magnitude (the DC row: eight ones), divided by the 4 the pass takes out
_ROW_ERR = 0.5 + 9 * 255 * 0.5 / 2 ** 11
_COL_ERR = 9 * 2 * 4097 * 0.5 / 2 ** 15 + 0.5 + 8 * _ROW_ERR / 4
DCT_ERR = _COL_ERR                                     # 3.75 in units of the x 8 output: DELTA = DCT_ERR / (8 q) levels


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_dct_and_quantisation_against_fp64(program, tmp_path, q, comp):
    blocks = dct_blocks()
    table = mjpeg.quant_tables(q)[comp].reshape(8, 8)
    ours = mjpeg.quantise_blocks(blocks, table)
    exact = scipy.fft.dctn(blocks.astype(np.float64) - 128, axes=(-2, -1), norm="ortho")
    assert np.abs(mjpeg.fdct_blocks(blocks) - 8 * exact).max() <= DCT_ERR          # the bound itself holds
    quotient = exact / table
    want = np.round(quotient)
    delta = DCT_ERR / (8 * table)
    differ = ours != want
    assert np.abs(ours - want).max() <= 1
    assert (np.abs(np.abs(quotient - np.floor(quotient)) - 0.5) <= delta)[differ].all()
    assert differ.mean() < 0.02 or q == 100
    # and the C++ of csrc/jpeg_tables.h, which the kernel compiles, computes the twin's numbers
    blocks.tofile(tmp_path / "in.bin")
    run(program, "blocks", q, comp, tmp_path / "in.bin", tmp_path / "out.bin")
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.int16).reshape(-1, 8, 8), ours)


# ---------------------------------------------------------------------------------------------- Pillow
def pillow_decode(jpg: bytes):
    """(Y, Cb, Cr at full resolution, the image) as Pillow decodes them, no colour conversion; any warning is an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(jpg))
        im.draft("YCbCr", None)                            # the decoder's own planes: no conversion to RGB
        im.load()
    assert im.mode == "YCbCr" and im.format == "JPEG"
    return np.asarray(im), im


def pillow_encode(y, cb, cr, quality) -> bytes:
    src = np.stack([y, cb.repeat(2, 0).repeat(2, 1), cr.repeat(2, 0).repeat(2, 1)], -1)
    buf = io.BytesIO()
    Image.fromarray(src, "YCbCr").save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def parity(content, w, h, layout, n=3):
    """Per frame: (ours decoded, Pillow's own decoded, the source, bytes of ours, bytes of Pillow's)."""
    data, offsets = MC.expected(content, w, h, layout, n)
    for i in range(n):
        jpg = data[offsets[i]:offsets[i + 1]].tobytes()
        y, cb, cr = MC.planes(content, w, h, i)
        ours, im = pillow_decode(jpg)
        assert im.size == (w, h)
        assert im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]                # 4:2:0: Y 2 x 2, Cb and Cr 1 x 1
        ref = pillow_encode(y, cb, cr, MC.CONTENTS[content])
        src = np.stack([y, cb.repeat(2, 0).repeat(2, 1), cr.repeat(2, 0).repeat(2, 1)], -1)
        yield ours, pillow_decode(ref)[0], src, len(jpg), len(ref)


# Bytes: ours may exceed Pillow's by the restart markers, the padding of every interval and the DRI segment — and, where the width
# or height is no multiple of 16, by the blocks that lie wholly outside the frame: libjpeg codes those as empty, the specification
# here as repeated edge pixels.  Margins: the larger of 1 % and twice the largest excess measured over the contents and layouts
# (profiles/mjpeg_parity.txt, written by tools/mjpeg_parity.py: 4.24 %, 6.30 % and 8.10 % at 2 x 2, 34 x 18 and 16 x 144 — files of a
# few hundred bytes, where nine restart markers weigh — and none at the two other sizes).
BYTE_MARGIN = {(16, 16): 0.01, (2, 2): 0.0847, (34, 18): 0.1260, (16, 144): 0.1619, (1280, 16): 0.01}


@pytest.mark.parametrize("content", list(MC.CONTENTS))
@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("w,h", MC.SIZES)
def test_pillow_decodes_every_frame_to_what_it_decodes_from_its_own_encoding(w, h, layout, content):
    for ours, theirs, src, nbytes, ref_bytes in parity(content, w, h, layout):
        assert np.array_equal(ours, theirs)                  # identical pixels: the mean squared error is Pillow's own
        assert nbytes <= ref_bytes * (1 + BYTE_MARGIN[(w, h)]), (nbytes, ref_bytes)


def scan_of(jpg: bytes):
    """(the entropy-coded intervals of one frame, the RST numbers between them)."""
    at = jpg.index(b"\xff\xda") + 14
    assert at == mjpeg.HEADER_BYTES and jpg[-2:] == b"\xff\xd9"
    body, ivls, rst, start, i = jpg[at:-2], [], [], 0, 0
    while i < len(body) - 1:
        if body[i] == 0xff and body[i + 1] != 0:
            assert 0xd0 <= body[i + 1] <= 0xd7
            ivls.append(body[start:i])
            rst.append(body[i + 1] - 0xd0)
            start = i = i + 2
        else:
            i += 2 if body[i] == 0xff else 1
    return ivls + [body[start:]], rst


def test_what_the_contents_are_there_for():
    # flat grey: the same few bytes in every interval — per MCU six blocks of DC 0 + EOB
    data, off = MC.expected("grey", 16, 144, "i420", 3)
    ivls, rst = scan_of(data[:off[1]].tobytes())
    assert len(ivls) == 9 and rst == [0, 1, 2, 3, 4, 5, 6, 7] and len(set(ivls)) == 1           # RSTm wraps after 7 ... the 9th ends in EOI
    z = mjpeg.frame_coefficients(*MC.planes("grey", 16, 144, 0), 90)
    assert not z.any()
    vals, lens = mjpeg.interval_entries(z[0])
    assert lens.tolist() == [2, 4] * 4 + [2, 2] * 2 and vals.tolist() == [0, 0b1010] * 4 + [0, 0] * 2   # DC category 0, EOB
    # the (7, 7) basis function: one coefficient at the end of the zig-zag, three ZRL in front of it
    z = mjpeg.frame_coefficients(*MC.planes("basis63", 16, 16, 0), 90)
    assert (z[0, 0, :5, 1:63] == 0).all() and (z[0, 0, :5, 63] != 0).all()
    vals, lens = mjpeg.interval_entries(z[0])
    assert vals[1:4].tolist() == [0x7f9] * 3 and lens[1:4].tolist() == [11] * 3                   # ZRL of the luminance table
    # noise at quality 100: stuffed bytes occur, and no interval comes near the capacity of its slot
    stuffed = 0
    for w, h in MC.SIZES:
        data, off = MC.expected("noise_q100", w, h, "nv12", 3)
        for i in range(3):
            ivls, _ = scan_of(data[off[i]:off[i + 1]].tobytes())
            assert len(ivls) == (h + 15) // 16
            stuffed += sum(iv.count(b"\xff\x00") for iv in ivls)
            assert max(len(iv) for iv in ivls) + 2 <= mjpeg.interval_max_bytes(w)
    assert stuffed >= 1
    # all 0 / all 255: nothing but DCs, of the largest magnitude a block can have, negative and positive
    for content, sign in (("zeros", -1), ("ones", 1)):
        z = mjpeg.frame_coefficients(*MC.planes(content, 16, 16, 0), 90)
        assert (np.sign(z[..., 0]) == sign).all() and not z[..., 1:].any()


# ---------------------------------------------------------------------------------------------- containers
def riff_chunks(buf: bytes, at: int, end: int):
    """[(fourcc, data offset, size)] of the chunks in buf[at:end]; a LIST's entry carries its type and its children follow."""
    out = []
    while at < end:
        four, size = buf[at:at + 4], struct.unpack_from("<I", buf, at + 4)[0]
        if four in (b"RIFF", b"LIST"):
            out.append((four + b":" + buf[at + 8:at + 12], at + 12, size - 4))
            out += riff_chunks(buf, at + 12, at + 8 + size)
        else:
            out.append((four, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end
    return out


def read_avi(path: Path, w, h, fps):
    """The JPEGs of one AVI file, everything the header and the index say checked."""
    buf = path.read_bytes()
    chunks = riff_chunks(buf, 0, len(buf))
    names = [c[0] for c in chunks]
    frames = [c for c in chunks if c[0] == b"00dc"]
    assert names == [b"RIFF:AVI ", b"LIST:hdrl", b"avih", b"LIST:strl", b"strh", b"strf", b"LIST:movi"] + [b"00dc"] * len(frames) + [b"idx1"]
    assert chunks[0][2] + 12 == len(buf)
    avih = struct.unpack_from("<14I", buf, chunks[2][1])
    assert chunks[2][2] == 56 and avih[0] == 1000000 // fps and avih[3] & 0x10 and avih[4] == len(frames) and avih[6] == 1 and avih[8:10] == (w, h)
    strh = struct.unpack_from("<4s4sIHHIIIIIIII4h", buf, chunks[4][1])
    assert chunks[4][2] == 56 and strh[:2] == (b"vids", b"MJPG") and strh[6:8] == (1, fps) and strh[9] == len(frames) and strh[-2:] == (w, h)
    strf = struct.unpack_from("<IiiHH4sI", buf, chunks[5][1])
    assert chunks[5][2] == 40 and strf == (40, w, h, 1, 24, b"MJPG", w * h * 3)
    assert avih[7] == strh[10] == max(c[2] for c in frames)
    movi = chunks[6][1] - 4                                   # the 'movi' fourcc
    idx = chunks[-1]
    assert idx[2] == 16 * len(frames)
    for k, (_, at, size) in enumerate(frames):
        assert (at - 8) % 2 == 0                              # every chunk starts on an even offset: odd sizes are padded
        four, flags, off, n = struct.unpack_from("<4sIII", buf, idx[1] + 16 * k)
        assert (four, flags & 0x10, n) == (b"00dc", 0x10, size) and movi + off == at - 8 and buf[movi + off:movi + off + 4] == b"00dc"
    return [buf[at:at + size] for _, at, size in frames]


def test_the_containers_read_back(tmp_path):
    w, h, n = 34, 18, 5
    raw, d = MC.raw_frames("ramp", w, h, "nv12", n, 0x11)
    data, off = mjpeg.encode_host(raw, n, h, w, d, 90)
    want = [data[off[i]:off[i + 1]].tobytes() for i in range(n)]
    assert {len(j) & 1 for j in want} == {0, 1}               # both paddings occur
    geom = dict(layout="nv12", pitch=d["pitch_y"], pitch_c=d["pitch_c"])
    # MjpegSink takes the planes where yuv_desc puts them: repack without the padded plane height
    packed = video.yuv_desc(w, h, **geom)
    tight = np.zeros(video.yuv_span(n, h, w, packed), np.uint8)
    for i in range(n):
        for dst, src in zip(mjpeg.planes(tight, i, h, w, packed), mjpeg.planes(raw, i, h, w, d)):
            dst[...] = src
    for name in ("clip.mjpeg", "clip.avi"):
        with video.MjpegSink(tmp_path / name, w, h, fps=25, on_device=False, **geom) as sink:
            sink.write_host(tight, 2)
            sink.write_host(tight[2 * packed["frame_stride"]:], 3)
        assert sink.frames_written == n and sink.paths == [str(tmp_path / name)]
        assert sink.bytes_written == (tmp_path / name).stat().st_size
        assert sink.enc == video.YUV_ENC_COEFFS["bt601_full"]
    assert (tmp_path / "clip.mjpeg").read_bytes() == b"".join(want)
    got = read_avi(tmp_path / "clip.avi", w, h, 25)
    assert got == want
    for jpg, i in zip(got, range(n)):
        ours, im = pillow_decode(jpg)
        assert im.size == (w, h)


def test_the_avi_rolls_over_into_complete_parts(tmp_path):
    w, h, n = 64, 48, 30
    d = video.yuv_desc(w, h, "i420")
    raw = np.random.default_rng(3).integers(0, 256, video.yuv_span(n, h, w, d), dtype=np.uint8)
    data, off = mjpeg.encode_host(raw, n, h, w, d, 90)
    want = [data[off[i]:off[i + 1]].tobytes() for i in range(n)]
    sink = video.MjpegSink(tmp_path / "roll.avi", w, h, on_device=False, max_riff_bytes=65536)
    sink.write_host(raw, n)
    sink.close()
    assert len(sink.paths) >= 2 and sink.paths[:2] == [str(tmp_path / "roll.avi"), str(tmp_path / "roll.part002.avi")]
    got = []
    for p in sink.paths:
        assert Path(p).stat().st_size <= 65536
        got += read_avi(Path(p), w, h, 30)
    assert got == want
    assert sink.bytes_written == sum(Path(p).stat().st_size for p in sink.paths)
    with pytest.raises(ValueError, match="suffix"):
        video.MjpegSink(tmp_path / "x.mp4", w, h)


# ---------------------------------------------------------------------------------------------- refusals and the runner
REFUSALS = {
    "odd width": (dict(w=15), "even"), "odd height": (dict(h=17), "even"), "too small": (dict(w=0), "at least 2"),
    "no frames": (dict(n=0), "n = 0"), "quality 0": (dict(quality=0), "quality"), "quality 101": (dict(quality=101), "quality"),
    "too wide": (dict(w=E.JPEG_MAX_WIDTH + 2), "2560"), "pitch_y": (dict(desc=dict(pitch_y=15)), "pitch_y"),
    "pitch_c": (dict(desc=dict(pitch_c=7)), "pitch_c"), "nv12 off_v": (dict(layout="nv12", desc=dict(off_v=400)), "off_v == off_u + 1"),
    "frame_stride": (dict(desc=dict(frame_stride=100)), "frame_stride"), "layout": (dict(desc=dict(layout=2)), "layout"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_one_refusal_per_reason(name):
    r, said = REFUSALS[name]
    n, h, w, quality = r.get("n", 2), r.get("h", 16), r.get("w", 16), r.get("quality", 90)
    d = video.yuv_desc(max(w, 2) & ~1, max(h, 2) & ~1, r.get("layout", "i420"))
    assert E.jpeg_check(max(n, 1), max(h, 2) & ~1, min(max(w, 2) & ~1, 2560), d, 90) is None
    d.update(r.get("desc", {}))
    why = E.jpeg_check(n, h, w, d, quality)
    assert why is not None and said in why
    if name != "layout":                                       # the twin refuses the same calls (it takes the layout from yuv_desc)
        with pytest.raises(ValueError):
            mjpeg.encode_host(np.zeros(1 << 18, np.uint8), n, h, w, d, quality)


def test_the_runner_picks_the_sink_by_suffix(tmp_path):
    src = "synthetic://?n=3&h=48&w=64&fps=24&seed=1"
    for name, kind in (("x.avi", video.MjpegSink), ("x.mjpeg", video.MjpegSink), ("x.MJPG", video.MjpegSink), ("x.y4m", video.Y4mSink),
                       ("x.bin", video.Y4mSink)):
        runner = TrackingRunner(stub_trackers([], [], []), src, tmp_path / "out.mp4", render=tmp_path / name, render_quality=77)
        sink, own = video.open_sink(runner.render, *runner.render_size(), runner.video_info.fps, runner.render_quality)
        assert type(sink) is kind and own and (sink.w, sink.h, sink.fps) == (64, 48, 24)
        if kind is video.MjpegSink:
            assert sink.quality == 77 and sink.enc == video.YUV_ENC_COEFFS["bt601_full"]
        sink.close()
    mine = video.MjpegSink(tmp_path / "mine.avi", 64, 48, on_device=False)
    runner = TrackingRunner(stub_trackers([], [], []), src, tmp_path / "out.mp4", render=mine)
    assert video.open_sink(runner.render, *runner.render_size()) == (mine, False) and runner.render_quality == 90
    mine.close()
