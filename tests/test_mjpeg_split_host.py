"""The split entropy path of the Motion-JPEG reader on the CPU (csrc/jpeg_entropy_split.h, ``decode_interval_split_host``) through the
stand-alone program tests/jpeg_split_main.cpp (g++ over the csrc files the kernels share), against the serial decoder
``decode_interval_host`` of csrc/jpeg_entropy.h:

* coefficients and status equal the serial decoder's on every well-formed stream of tests/test_mjpeg_decode_host.py (but the
  1280-wide), on two Pillow streams of 320 x 192 without restart markers, on a 48 x 32 stream at quality 100 and on a stream built
  symbol by symbol here, for subsequences of 4, 8, 16 and 128 bytes;
* those streams hold the hard cases, asserted from their bytes and from the program's counts: a stuffed FF 00 pair across a
  subsequence boundary (the subsequence starts on the 00), a symbol that covers a whole following subsequence, a block over three
  and more subsequences, three and more rounds, a speculative lane that went dead and started again from its guess;
* convergence as a condition: at 128 bytes the two 320 x 192 streams need at most a quarter as many rounds as they have
  subsequences (the serial chains of the issue: 14 of 364, 34 of 345), the 48 x 32 quality-100 stream, which never falls into step,
  at most subsequences + 1, and is exact all the same;
* the broken streams of tests/test_mjpeg_decode_host.py: the same coefficients and status as the serial decoder at 8 and 128 bytes,
  and the program rebuilt under the address and undefined-behaviour sanitizers gets through them with exit status 0 and nothing on
  stderr;
* what ``pa_jpeg_decode_set_split`` refuses, through the library, each with its reason (no GPU: the arguments are judged first)."""
import ctypes as C
import functools
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E
from padel_analytics_amd import mjpeg
from tests import test_mjpeg_decode_host as T

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
SUB_BYTES = (4, 8, 16, 128)
FIELDS = ("equal", "serial_status", "split_status", "serial_digest", "split_digest", "intervals", "subsequences", "rounds", "symbols",
          "restarts", "passed", "stuffed_starts", "longest_block", "sub_bytes")


def crafted_stream() -> bytes:
    """16 x 16, one MCU, written symbol by symbol with the Annex K tables so that, cut into 4-byte subsequences, the 26-bit symbol
    (run 0, size 10, value 1023) begins on the last bit of subsequence 0, fills subsequence 1 (FF 00 07 FF: 24 bits, one stuffed
    byte) and ends in subsequence 2, which starts on the 00 of the second FF 00 pair."""
    dcl, acl = mjpeg.huff_codes(mjpeg.DC_LUMA), mjpeg.huff_codes(mjpeg.AC_LUMA)
    dcc, acc = mjpeg.huff_codes(mjpeg.DC_CHROMA), mjpeg.huff_codes(mjpeg.AC_CHROMA)
    sym = lambda table, s: (int(table[0][s]), int(table[1][s]))
    entries = [sym(dcl, 0)] + [sym(acl, 0x01), (0, 1)] * 7 + [sym(acl, 0x02), (0, 2)] * 2 + [sym(acl, 0x0a), (1023, 10)] + [sym(acl, 0)]
    entries += [sym(dcl, 0), sym(acl, 0)] * 3 + [sym(dcc, 0), sym(acc, 0)] * 2
    assert sum(n for _, n in entries[:1 + 14 + 4]) == 31 and sym(acl, 0x0a)[1] == 16
    data = mjpeg.pack_interval(np.array([v for v, _ in entries], np.int64), np.array([n for _, n in entries], np.int64))
    return mjpeg.frame_header(16, 16, 100) + data + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def split_streams() -> dict:
    out = {n: j for n, j in T.streams().items() if not n.startswith("own_1280")}
    out["pil_320x192_q90"] = T.pillow_stream(320, 192)
    out["pil_320x192_q90_optimize"] = T.pillow_stream(320, 192, optimize=True)
    out["pil_48x32_q100"] = T.pillow_stream(48, 32, quality=100)
    out["crafted_16x16"] = crafted_stream()
    return out


def build(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "jpeg_split_main.cpp"),
                    str(CSRC / "jpeg_parse.cpp"), "-o", str(out)], check=True)
    return out


def run_program(exe: Path, jpegs: list, sub_bytes, tmp: Path) -> list:
    """Per stream: None if the program refused it, else {sub_bytes: {field: value}}."""
    src = tmp / "in.bin"
    src.write_bytes(b"".join(struct.pack("<I", len(j)) + j for j in jpegs))
    done = subprocess.run([str(exe), str(src), *(str(s) for s in sub_bytes)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr[-4000:]
    out = [{} for _ in jpegs]
    lines = done.stdout.splitlines()
    assert len(lines) == len(jpegs) * len(sub_bytes)
    for line in lines:
        f = line.split()
        if f[2] == "refused":
            out[int(f[0])] = None
        else:
            vals = [v if "digest" in k else int(v) for k, v in zip(FIELDS, f[2:])]
            out[int(f[0])][int(f[1])] = dict(zip(FIELDS, vals))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory) -> dict:
    """name -> {sub_bytes: counts} for every well-formed stream: one build, one run, shared."""
    tmp = tmp_path_factory.mktemp("split")
    names = sorted(split_streams())
    got = run_program(build(tmp / "jpeg_split_main"), [split_streams()[n] for n in names], SUB_BYTES, tmp)
    return dict(zip(names, got))


def entropy_bytes(jpeg: bytes) -> bytes:
    info = mjpeg.parse_frame(jpeg)
    assert info["n_intervals"] == 1
    begin, end = info["intervals"][0][:2]
    return jpeg[begin:end]


@pytest.mark.parametrize("name", sorted(split_streams()))
def test_split_equals_serial_on_well_formed_streams(answers, name):
    assert answers[name] is not None
    for s in SUB_BYTES:
        a = answers[name][s]
        print(name, s, a)
        assert a["equal"] == 1 and a["serial_status"] == a["split_status"] == 0 and a["serial_digest"] == a["split_digest"], (name, s, a)
        assert a["sub_bytes"] >= s and a["subsequences"] >= a["intervals"] and 1 <= a["rounds"] <= a["subsequences"] + 1


def test_serial_answer_of_the_program_is_the_twins(answers):
    """The digests compare the program's two decoders; the serial one is pinned to the numpy twin by test_mjpeg_decode_host — and
    here once, through the digest."""
    jpeg = split_streams()["crafted_16x16"]
    coef, status = mjpeg.frame_coefficients_of(jpeg)
    assert status == 0 and coef.reshape(-1, 64)[0, 10] == 1023 and np.count_nonzero(coef) == 10
    h = 1469598103934665603
    for b in coef.astype("<i2").tobytes():
        h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    assert f"{h ^ 1469598103934665603:016x}" == answers["crafted_16x16"][4]["serial_digest"]


def test_stuffed_pair_across_a_boundary_and_a_start_on_the_stuffed_zero(answers):
    for name, s in (("crafted_16x16", 4), ("pil_48x32_q100", 4), ("pil_320x192_q90", 4)):
        data = entropy_bytes(split_streams()[name])
        eff = answers[name][s]["sub_bytes"]
        starts = [t for t in range(eff, len(data), eff) if data[t - 1] == 0xff and data[t] == 0]
        assert starts and answers[name][s]["stuffed_starts"] == len(starts), (name, starts)
        assert answers[name][s]["equal"] == 1
    data = entropy_bytes(split_streams()["crafted_16x16"])
    # DC 00, seven times 00 0, twice 01 00, then 1111111110000011 1111111111, the block's end 1010, the next block's 00 1010 ...
    assert data[:10] == bytes([0, 0, 0, 0x89, 0xff, 0, 0x07, 0xff, 0, 0xd1])


def test_symbol_that_covers_a_whole_following_subsequence(answers):
    """The 26 bits of (run 0, size 10, 1023) of the crafted stream: bit 31, all 24 bits of subsequence 1, one bit of subsequence 2."""
    a = answers["crafted_16x16"][4]
    assert a["passed"] >= 1 and a["equal"] == 1 and a["sub_bytes"] == 4
    assert answers["crafted_16x16"][8]["passed"] == 0


def test_blocks_over_three_subsequences_three_rounds_and_dead_lanes(answers):
    a = answers["pil_48x32_q100"]
    assert a[4]["longest_block"] >= 3 and a[8]["longest_block"] >= 3
    for name in ("pil_320x192_q90", "pil_320x192_q90_optimize", "pil_48x32_default"):
        for s in (4, 8, 16, 128):
            b = answers[name][s]
            if name.startswith("pil_320") or s < 128:
                assert b["rounds"] >= 3 and b["restarts"] >= 1, (name, s, b)
            assert b["symbols"] > 0


def test_convergence(answers):
    for name in ("pil_320x192_q90", "pil_320x192_q90_optimize"):
        a = answers[name][128]
        print(name, a)
        assert a["sub_bytes"] == 128 and a["subsequences"] > 300
        assert a["rounds"] <= a["subsequences"] / 4
    for s in SUB_BYTES:
        a = answers["pil_48x32_q100"][s]
        print("pil_48x32_q100", s, a)
        assert a["rounds"] <= a["subsequences"] + 1 and a["equal"] == 1


def test_an_interval_of_more_than_4096_subsequences_gets_longer_ones(answers):
    a = answers["pil_320x192_q90"][4]
    assert a["sub_bytes"] > 4 and a["sub_bytes"] % 4 == 0 and a["subsequences"] <= 4096 and a["equal"] == 1


def test_broken_streams_equal_serial_and_the_sanitizers_stay_silent(tmp_path):
    names, jpegs = T.broken_streams()
    assert len(jpegs) > 300
    plain = run_program(build(tmp_path / "jpeg_split_main"), jpegs, (8, 128), tmp_path)
    san = run_program(build(tmp_path / "jpeg_split_main_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), jpegs,
                      (8, 128), tmp_path)                 # exit status 0 and nothing on stderr: no report from either sanitizer
    assert san == plain
    refused = sum(g is None for g in plain)
    flagged = sum(g is not None and g[8]["serial_status"] != 0 for g in plain)
    print(f"{len(jpegs)} broken streams: {refused} refused, {flagged} flagged")
    assert refused > 30 and flagged > 100
    for bit in (mjpeg.ST_CODE, mjpeg.ST_INDEX, mjpeg.ST_DATA, mjpeg.ST_MARKERS):          # every kind of complaint occurs
        assert any(g is not None and g[8]["serial_status"] & bit for g in plain), bit
    for g, name in zip(plain, names):
        if g is not None:
            for s in (8, 128):
                assert g[s]["equal"] == 1 and g[s]["split_status"] == g[s]["serial_status"], (name, s, g[s])
                assert g[s]["split_digest"] == g[s]["serial_digest"], (name, s)


# ---------------------------------------------------------------------------------------------- pa_jpeg_decode_set_split
def _refused(min_bytes: int, sub_bytes: int) -> str:
    lib = E.load_library()
    assert lib.pa_jpeg_decode_set_split(None, min_bytes, sub_bytes) != 0
    return lib.pa_last_error(None).decode()


def test_set_split_refuses_a_negative_length():
    assert "min_bytes = -2" in _refused(-2, 0)


def test_set_split_refuses_subsequences_that_are_no_multiple_of_four():
    assert "sub_bytes = 130 is not a multiple of 4" in _refused(0, 130)


def test_set_split_refuses_subsequences_that_are_too_short():
    assert "sub_bytes = 2 outside 4 .. 32768" in _refused(0, 2)
    assert "sub_bytes = -4 outside 4 .. 32768" in _refused(-1, -4)


def test_set_split_refuses_subsequences_that_are_too_long():
    assert "sub_bytes = 32772 outside 4 .. 32768" in _refused(4096, 32772)


def test_set_split_with_good_arguments_needs_an_engine():
    for args in ((0, 0), (-1, 0), (1, 4), (1 << 40, 32768)):
        assert "engine is NULL" in _refused(*args)
    out = (C.c_int64 * 4)()
    assert E.load_library().pa_jpeg_decode_last_split(None, out) != 0
