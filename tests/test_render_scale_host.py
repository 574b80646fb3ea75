"""``render_scale`` without a GPU (include/padel_hip.h, ``pa_render_scaled``): the box average and its rounding (csrc/render_scale.h,
evaluated by the stand-alone program tests/render_scale_main.cpp built with g++, once more under the address and undefined-behaviour
sanitizers), the numpy twin ``render.render_host(scale=)`` against the pipeline it is defined as, a known answer worked out by hand,
one case per refusal in the twin and in ``pa_render_scaled_check``, and what ``TrackingRunner(render_scale=)`` decides before any
tracker runs."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E, render as R, video
from padel_analytics_amd.trackers import TrackingRunner
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)
from tests.court_script import stub_trackers
from tests.twin_engine import StandInEngine

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
ENC = video.YUV_ENC_COEFFS["bt601_limited"]
SCALES = (2, 3, 4)


def frames_of(n, h, w, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the average
@pytest.mark.parametrize("s", SCALES)
def test_downscale_host_is_the_mean_rounded_half_up(s):
    """floor(mean + 0.5) in fp64: sums of at most 16 bytes and their quotients by 4 and 16 are exact, and a sum over 9 is never
    half-way between two integers (2 sum + 9 is odd), so the fp64 value decides the same way the integers do."""
    frames = frames_of(2, 12 * s, 10 * s, seed=s)
    frames[0, :s, :s] = 255                              # the extremes, and a tie for s = 2 and 4: half the block 1, half 0
    frames[0, :s, s:2 * s] = 0
    frames[0, :s, 2 * s:3 * s] = 0
    frames[0, :s // 2 or 1, 2 * s:3 * s] = 1
    got = R.downscale_host(frames, s)
    assert got.shape == (2, 12, 10, 3) and got.dtype == np.uint8
    mean = frames.reshape(2, 12, s, 10, s, 3).astype(np.float64).mean(axis=(2, 4))
    assert np.array_equal(got, np.floor(mean + 0.5).astype(np.uint8))
    assert tuple(got[0, 0, 0]) == (255, 255, 255) and tuple(got[0, 0, 1]) == (0, 0, 0)
    if s != 3:
        assert tuple(got[0, 0, 2]) == (1, 1, 1)          # 0.5 rounds up
    assert np.array_equal(R.downscale_host(frames, 1), frames)


def test_downscale_host_refuses_what_has_no_answer():
    f = frames_of(1, 12, 12)
    for s in (0, 5, -1):
        with pytest.raises(ValueError, match="scale"):
            R.downscale_host(f, s)
    with pytest.raises(ValueError, match="multiple"):
        R.downscale_host(frames_of(1, 12, 14), 4)
    with pytest.raises(ValueError, match="uint8"):
        R.downscale_host(f.astype(np.int32), 2)


def build_table(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "render_scale_main.cpp"), "-o", str(out)],
                   check=True)
    return out


def check_table(text):
    rows = np.array([[int(v) for v in line.split()] for line in text.splitlines()], np.int64)
    assert len(rows) == sum(255 * s * s + 1 for s in SCALES)
    for s in SCALES:
        mine = rows[rows[:, 0] == s]
        assert np.array_equal(mine[:, 1], np.arange(255 * s * s + 1))                  # every possible sum, once
        assert np.array_equal(mine[:, 2], (mine[:, 1] + s * s // 2) // (s * s))
        assert mine[-1, 2] == 255 and mine[0, 2] == 0


def test_the_shared_header_rounds_every_sum_like_the_division(tmp_path):
    done = subprocess.run([str(build_table(tmp_path / "render_scale_main"))], check=True, capture_output=True, text=True)
    check_table(done.stdout)


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build_table(tmp_path / "render_scale_asan", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    check_table(done.stdout)


# ---------------------------------------------------------------------------------------------- the twin
def some_marks(h, w):
    return [R.segment(-5, 3, w + 4, h - 2, 1, 0x10F0A0), R.disc(w // 2, h // 2, 5, 0x0000FF), R.blend(2, 2, w - 3, h // 2, 0xFFFFFF, 128),
            R.box(1, 1, w - 2, h - 2, 2, 0xFF8000), R.arc(w // 3, h // 2, 9, 6, 2, 0x00FFFF, 0x3C), R.fill(w - 4, -3, w + 5, 4, 0x123456),
            *R.text("S4", 3, 3, 1, 0xFFFFFF), R.disc(-40, -40, 6, 0xFFFFFF)]


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("layout", [None, "nv12", "i420"])
def test_render_host_scaled_is_draw_then_average_then_encode(s, layout):
    h, w = 8 * s, 12 * s
    frames = frames_of(2, h, w, seed=10 + s)
    marks, first = R.pack([some_marks(h, w), some_marks(h, w)[::-1]])
    small = R.downscale_host(R.render_host(frames, marks, first), s)
    assert not np.array_equal(small, R.downscale_host(frames, s))                       # (the marks show)
    if layout is None:
        got = R.render_host(frames, marks, first, scale=s)
        assert got.shape == (2, 8, 12, 3) and np.array_equal(got, small)
        return
    geom = video.yuv_desc(12, 8, layout, pitch=16, pitch_c=16 if layout == "nv12" else 9)
    dst = np.full(video.yuv_span(2, 8, 12, geom), 0x5A, np.uint8)
    got = R.render_host(frames, marks, first, E.RENDER_YUV420, geom, ENC, dst=dst.copy(), scale=s)
    assert np.array_equal(got, video.bgr_to_yuv420_host(small, geom, ENC, out=dst.copy()))


def test_a_known_answer_worked_out_by_hand():
    """4 x 4 -> 2 x 2.  The frame is 100 everywhere; a one-pixel disc of colour (B, G, R) = (255, 0, 30) sits at (1, 0); then a blend
    of white at weight 128 over the right half (columns 2, 3): (100 * 128 + 255 * 128 + 128) >> 8 = 178.
    Output (0, 0): three pixels of 100 and the disc: B (300 + 255 + 2) >> 2 = 139, G (300 + 0 + 2) >> 2 = 75, R (330 + 2) >> 2 = 83.
    Output (1, 0) and (1, 1): four pixels of 178.  Output (0, 1): untouched, 100."""
    frames = np.full((1, 4, 4, 3), 100, np.uint8)
    marks, first = R.pack([[R.disc(1, 0, 0, (255, 0, 30)), R.blend(2, 0, 3, 3, (255, 255, 255), 128)]])
    got = R.render_host(frames, marks, first, scale=2)
    assert got.shape == (1, 2, 2, 3)
    assert got[0].tolist() == [[[139, 75, 83], [178, 178, 178]], [[100, 100, 100], [178, 178, 178]]]
    # and as I420 with the limited-range BT.601 table: one chroma sample from the sums of the four output pixels
    geom = video.yuv_desc(2, 2, "i420")
    yuv = R.render_host(frames, marks, first, E.RENDER_YUV420, geom, ENC, scale=2)
    assert np.array_equal(yuv, video.bgr_to_yuv420_host(got, geom, ENC)) and yuv.size == 6


@pytest.mark.parametrize("out, layout", [(E.RENDER_BGR, None), (E.RENDER_YUV420, "i420")])
def test_scale_1_is_the_call_without_the_argument(out, layout):
    frames = frames_of(2, 16, 24, seed=5)
    marks, first = R.pack([some_marks(16, 24), []])
    geom = video.yuv_desc(24, 16, layout) if layout else None
    enc = ENC if layout else None
    assert np.array_equal(R.render_host(frames, marks, first, out, geom, enc, scale=1), R.render_host(frames, marks, first, out, geom, enc))
    assert E.render_check(2, 16, 24, marks, first, out, geom, enc, scale=1) is None
    assert E.render_check(2, 15, 24, marks, first, E.RENDER_YUV420, video.yuv_desc(24, 16), ENC, scale=1) == \
        E.render_check(2, 15, 24, marks, first, E.RENDER_YUV420, video.yuv_desc(24, 16), ENC)


# ---------------------------------------------------------------------------------------------- the refusals
OK_MARKS, OK_FIRST = R.pack([[R.disc(1, 1, 1, 1)]])
REFUSALS = {
    "scale 0": (dict(scale=0), "scale 0 outside"),
    "scale 5": (dict(scale=5), "scale 5 outside"),
    "width no multiple": (dict(w=26, scale=4), "no multiple of scale 4"),
    "height no multiple": (dict(h=17, scale=3), "no multiple of scale 3"),
    "odd output width": (dict(w=18, h=12, scale=2, yuv=(10, 6)), "even output width"),
    "odd output height": (dict(w=24, h=18, scale=2, yuv=(12, 10)), "even output width and height"),
    "output too small": (dict(w=3, h=6, scale=3, yuv=(2, 2)), "at least 2"),
    "in place": (dict(scale=2, in_place=True), "dst == src"),
    "source too large": (dict(w=8194, scale=2), "8192"),
    "a mark the renderer refuses": (dict(scale=2, marks=np.array([(9, 0, 0, 0, 0, 1, 0, 0)], E.MARK_DTYPE)), "unknown kind"),
    "pitch of the output": (dict(scale=2, yuv=(12, 8), desc=dict(pitch_y=11)), "pitch_y 11 is smaller than a luma row of 12"),
    "geometry missing": (dict(scale=2, yuv=None), "geometry descriptor"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_one_refusal_per_reason_in_the_check_and_in_the_twin(name):
    r, said = REFUSALS[name]
    h, w, s = r.get("h", 16), r.get("w", 24), r["scale"]
    marks = r.get("marks", OK_MARKS)
    out, geom, enc = E.RENDER_BGR, None, None
    if "yuv" in r:
        out = E.RENDER_YUV420
        if r["yuv"] is not None:
            geom, enc = dict(video.yuv_desc(*r["yuv"], "i420"), **r.get("desc", {})), ENC
    why = E.render_check(1, h, w, marks, OK_FIRST, out, geom, enc, scale=s, in_place=r.get("in_place", False))
    assert why is not None and said in why, why
    if not r.get("in_place"):                              # (the twin has no destination to be its source)
        with pytest.raises(ValueError) as twin:
            R.render_host(np.zeros((1, h, w, 3), np.uint8), marks, OK_FIRST, out, geom, enc, scale=s)
        assert str(twin.value) == why                        # the same words


def test_what_is_accepted():
    geom = video.yuv_desc(12, 8, "nv12")
    for s in SCALES:
        assert E.render_check(1, 8 * s, 12 * s, OK_MARKS, OK_FIRST, E.RENDER_YUV420, geom, ENC, scale=s) is None
        assert E.render_check(1, 3 * s, 5 * s, OK_MARKS, OK_FIRST, scale=s) is None      # BGR: odd output sizes are fine
    assert E.render_check(1, 2160, 3840, OK_MARKS, OK_FIRST, E.RENDER_YUV420, video.yuv_desc(1920, 1080, "i420"), ENC, scale=2) is None


# ---------------------------------------------------------------------------------------------- the runner
SRC_720P = "synthetic://?n=3&h=720&w=1280&fps=25&seed=1"


def make_sink(runner):
    """The sink the rendered frames go to, as the render step opens it: at ``render_size()``."""
    return video.open_sink(runner.render, *runner.render_size(), runner.video_info.fps, runner.render_quality)


def make_runner(tmp_path, src=SRC_720P, **kw):
    return TrackingRunner(stub_trackers([], [], []), src, tmp_path / "out.mp4", engine=StandInEngine(), **kw)


@pytest.mark.parametrize("s, size", [(1, (1280, 720)), (2, (640, 360)), (4, (320, 180))])
def test_the_runner_builds_its_sink_at_the_scaled_size(tmp_path, s, size):
    for name, kind in (("x.y4m", video.Y4mSink), ("x.avi", video.MjpegSink)):
        runner = make_runner(tmp_path, render=tmp_path / name, render_scale=s)
        assert runner.render_scale == s and runner.render_size() == size
        sink, own = make_sink(runner)
        assert type(sink) is kind and own and (sink.w, sink.h, sink.fps) == (*size, 25)
        assert sink.desc == video.yuv_desc(*size, "i420", "bt601", "full" if kind is video.MjpegSink else "limited")
        sink.close()


def test_a_4k_clip_gets_its_avi_at_half_size(tmp_path):
    src = "synthetic://?n=1&h=2160&w=3840&fps=30&seed=1"
    with pytest.raises(ValueError, match="2560"):                              # today's rule: the JPEG encoder's width limit
        make_sink(make_runner(tmp_path, src, render=tmp_path / "full.avi"))
    sink, _ = make_sink(make_runner(tmp_path, src, render=tmp_path / "half.avi", render_scale=2))
    assert (sink.w, sink.h) == (1920, 1080)
    sink.close()


def test_a_scale_the_clip_does_not_allow_is_refused_before_any_tracker_runs(tmp_path):
    with pytest.raises(ValueError, match=r"render_scale=3.*1280 x 720.*works for this clip: 1, 2, 4"):
        make_runner(tmp_path, render=tmp_path / "x.y4m", render_scale=3)
    with pytest.raises(ValueError, match=r"works for this clip: 1, 2, 3$|works for this clip: 1, 2, 3\)"):
        make_runner(tmp_path, "synthetic://?n=2&h=36&w=60&fps=30&seed=1", render=tmp_path / "x.y4m", render_scale=4)      # 15 x 9: odd
    assert not (tmp_path / "x.y4m").exists()
    for bad in (0, 5, -2, 2.5, "2", None, True):
        with pytest.raises(ValueError, match="render_scale"):
            make_runner(tmp_path, render_scale=bad)
    assert make_runner(tmp_path, render_scale=3).render_scale == 3              # nothing is rendered: nothing to fit


def test_a_sink_of_another_size_is_refused(tmp_path):
    with video.Y4mSink(tmp_path / "full.y4m", 1280, 720) as full, video.Y4mSink(tmp_path / "half.y4m", 640, 360) as half:
        with pytest.raises(ValueError, match=r"sink takes 1280 x 720.*render_scale=2 gives 640 x 360"):
            make_runner(tmp_path, render=full, render_scale=2)
        with pytest.raises(ValueError, match=r"sink takes 640 x 360.*render_scale=1 gives 1280 x 720"):
            make_runner(tmp_path, render=half)
        assert make_sink(make_runner(tmp_path, render=half, render_scale=2)) == (half, False)
        assert make_sink(make_runner(tmp_path, render=full)) == (full, False)
