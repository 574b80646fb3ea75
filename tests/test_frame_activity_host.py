"""The court-view filter without a GPU: the numpy twin of the frame statistic (``activity.frame_activity_host``) against a second,
per-pixel statement of include/padel_hip.h and against known answers; the refusals of ``pa_frame_activity_check`` through ctypes and
through the stand-alone program tests/activity_check_main.cpp (plain, and under -fsanitize=address,undefined: a plain executable,
nothing is preloaded); ``court_view_mask`` / ``segments`` known answers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import activity as A, engine as E

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"


def per_pixel(frames, ref, prev, roi, tau):
    """The specification once more, one pixel at a time in Python integers."""
    n, h, w = frames.shape[:3]
    x0, y0, x1, y1 = roi if roi is not None else (0, 0, w, h)
    Y = lambda p: (29 * int(p[0]) + 150 * int(p[1]) + 77 * int(p[2]) + 128) >> 8
    out = []
    for i in range(n):
        before = frames[i - 1] if i else prev
        s = [0, 0, 0]
        for y in range(y0, y1):
            for x in range(x0, x1):
                d = abs(Y(frames[i, y, x]) - Y(ref[y, x]))
                s[0] += d
                s[1] += d > tau
                if before is not None:
                    s[2] += abs(Y(frames[i, y, x]) - Y(before[y, x]))
        out.append(s)
    return np.array(out, np.uint64)


@pytest.mark.parametrize("roi", [None, (1, 0, 4, 3), (2, 1, 3, 2)])
@pytest.mark.parametrize("with_prev", [False, True])
def test_twin_equals_the_per_pixel_statement(roi, with_prev):
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (4, 3, 5, 3), dtype=np.uint8)
    ref = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    prev = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8) if with_prev else None
    for tau in (0, 24, 255):
        got = A.frame_activity_host(frames, ref, prev=prev, roi=roi, tau=tau)
        assert got.dtype == np.uint64 and np.array_equal(got, per_pixel(frames, ref, prev, roi, tau))
    if not with_prev:
        assert got[0, 2] == 0


def test_luma_weights_sum_to_256():
    assert A.luma(np.array([255, 255, 255], np.uint8)) == 255 and A.luma(np.array([0, 0, 0], np.uint8)) == 0
    assert A.luma(np.array([255, 0, 0], np.uint8)) == (29 * 255 + 128) >> 8


def test_white_against_black():
    frames, ref = np.full((1, 64, 64, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8)
    a = A.frame_activity_host(frames, ref, tau=254)
    assert a[0, 0] == 255 * 4096 and a[0, 1] == 4096 and a[0, 2] == 0
    assert A.frame_activity_host(frames, ref, tau=255)[0, 1] == 0
    assert A.frame_activity_host(frames, ref, prev=ref)[0, 2] == 255 * 4096


def test_a_difference_of_exactly_tau_is_not_counted():
    tau = 24
    ref = np.full((2, 2, 3), 100, np.uint8)                   # grey g has luma g
    frames = np.stack([np.full((2, 2, 3), 100 + tau, np.uint8), np.full((2, 2, 3), 100 + tau + 1, np.uint8),
                       np.full((2, 2, 3), 100 - tau, np.uint8), np.full((2, 2, 3), 100 - tau - 1, np.uint8)])
    a = A.frame_activity_host(frames, ref, tau=tau)
    assert a[:, 1].tolist() == [0, 4, 0, 4] and a[:, 0].tolist() == [4 * tau, 4 * (tau + 1), 4 * tau, 4 * (tau + 1)]


def test_twin_refuses_what_the_library_refuses():
    f, r = np.zeros((1, 4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="roi"):
        A.frame_activity_host(f, r, roi=(0, 0, 5, 4))
    with pytest.raises(ValueError, match="tau"):
        A.frame_activity_host(f, r, tau=256)


REFUSALS = [
    ("no frames", dict(n=0, h=4, w=6), "n = 0 frames outside [1, 65535]"),
    ("too many frames", dict(n=65536, h=4, w=6), "n = 65536 frames outside"),
    ("no width", dict(n=1, h=4, w=0), "width and height must lie in [1, 16384]"),
    ("too tall", dict(n=1, h=16385, w=6), "width and height must lie in [1, 16384]"),
    ("roi beyond the frame", dict(n=1, h=4, w=6, roi=(0, 0, 7, 4)), "roi (0, 0, 7, 4) is empty or leaves the 6 x 4 frame"),
    ("empty roi", dict(n=1, h=4, w=6, roi=(2, 1, 2, 3)), "roi (2, 1, 2, 3) is empty or leaves"),
    ("negative roi", dict(n=1, h=4, w=6, roi=(-1, 0, 3, 3)), "roi (-1, 0, 3, 3) is empty or leaves"),
    ("tau above 255", dict(n=1, h=4, w=6, tau=256), "tau = 256 outside [0, 255]"),
    ("negative tau", dict(n=1, h=4, w=6, tau=-1), "tau = -1 outside [0, 255]"),
]


@pytest.mark.parametrize("case,kw,words", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case, kw, words):
    why = E.frame_activity_check(**kw)
    assert why is not None and why.startswith("pa_frame_activity: ") and words in why


def test_accepted_calls():
    assert E.frame_activity_check(1, 1, 1) is None
    assert E.frame_activity_check(65535, 16384, 16384, roi=(16383, 16383, 16384, 16384), tau=255) is None
    assert E.frame_activity_check(3, 4, 6, roi=(0, 0, 6, 4), tau=0) is None
    assert {"pa_frame_activity", "pa_frame_activity_check", "pa_frames_median"} <= set(E.ABI_SYMBOLS)


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_check_as_a_stand_alone_program(tmp_path, extra):
    exe = tmp_path / "activity_check_main"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(ROOT / "tests" / "activity_check_main.cpp"),
                    str(CSRC / "activity_check.cpp"), "-o", str(exe)], check=True)
    run = lambda *a: subprocess.run([str(exe), *map(str, a)], capture_output=True, text=True)
    r = run()
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    for case, kw, words in REFUSALS:                       # the program and the library give the same text
        roi = kw.get("roi")
        if roi is not None and roi[0] < 0:
            continue                                       # (the program's command line spells "no roi" as x0 < 0)
        r = run("check", kw["n"], kw["h"], kw["w"], *(roi or (-1, 0, 0, 0)), kw.get("tau", 24))
        assert r.returncode == 0 and r.stdout.strip() == E.frame_activity_check(**kw), case
    assert run("check", 2, 4, 6, 1, 1, 5, 3, 24).stdout.strip() == "ok"


def act(flags):
    """A FrameActivity of 100-pixel frames whose frame i counts as court view iff flags[i]."""
    flags = np.asarray(flags, bool)
    changed = np.where(flags, 10, 90).astype(np.uint64)
    return A.FrameActivity(sad_ref=changed * 3, changed=changed, sad_prev=np.zeros(len(flags), np.uint64), npix=100)


def bits(s):
    return [c == "1" for c in s]


def test_threshold_is_inclusive():
    a = A.FrameActivity(sad_ref=np.zeros(3, np.uint64), changed=np.array([34, 35, 36], np.uint64), sad_prev=np.zeros(3, np.uint64), npix=100)
    assert A.court_view_mask(a, max_changed=0.35, max_gap=0, min_keep=1).tolist() == [True, True, False]


def test_a_gap_of_max_gap_is_filled_a_longer_one_is_kept():
    assert A.court_view_mask(act(bits("1110011")), max_gap=2, min_keep=1).tolist() == bits("1111111")
    assert A.court_view_mask(act(bits("11100011")), max_gap=2, min_keep=1).tolist() == bits("11100011")
    # a gap at either end lies between no two True runs
    assert A.court_view_mask(act(bits("0011100")), max_gap=2, min_keep=1).tolist() == bits("0011100")


def test_a_run_of_min_keep_is_kept_a_shorter_one_is_dropped():
    assert A.court_view_mask(act(bits("0001110000")), max_gap=0, min_keep=3).tolist() == bits("0001110000")
    assert A.court_view_mask(act(bits("0001100000")), max_gap=0, min_keep=3).tolist() == bits("0000000000")


def test_gaps_are_filled_before_short_runs_are_dropped():
    # two runs of 2 with a gap of 1: filled first they are one run of 5, which min_keep = 4 keeps; dropped first nothing would be left
    assert A.court_view_mask(act(bits("000110110000")), max_gap=1, min_keep=4).tolist() == bits("000111110000")


def test_defaults_follow_fps():
    flags = bits("1" * 30 + "0" * 5 + "1" * 30 + "0" * 6 + "1" * 19 + "0" * 10)
    got = A.court_view_mask(act(flags), fps=10)                # max_gap = 5, min_keep = 20
    assert got.tolist() == bits("1" * 65 + "0" * 6 + "0" * 19 + "0" * 10)


def test_all_false_and_all_true():
    assert A.court_view_mask(act([False] * 9), max_gap=2, min_keep=3).tolist() == [False] * 9
    assert A.court_view_mask(act([True] * 9), max_gap=2, min_keep=3).tolist() == [True] * 9
    assert A.segments([False] * 9) == [] and A.segments([True] * 9) == [(0, 9)] and A.segments([]) == []
    assert A.court_view_mask(act([]), max_gap=2, min_keep=3).tolist() == []


def test_segments_are_the_true_runs():
    assert A.segments(bits("0110001011")) == [(1, 3), (6, 7), (8, 10)]
    assert A.segments(bits("1000000001")) == [(0, 1), (9, 10)]
