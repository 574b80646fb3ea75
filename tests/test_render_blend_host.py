"""``PA_MARK_BLEND`` without a GPU: the one mark of the renderer that is not opaque (include/padel_hip.h).

``mark_apply`` (csrc/render_marks.h) is what the render kernel calls on a covered pixel register; the stand-alone program
tests/render_blend_main.cpp, built with g++ over that header and csrc/render_check.cpp, evaluates it on the CPU.  The expected values
are stated here once more, in numpy, straight from the rule — per channel ``(p * (256 - a) + c * a + 128) >> 8`` — independently of
``render.draw_host`` and of the C++; all three must agree bit for bit.  List order (a blend sees what the marks before it left, a
later mark sees the blended value), the refusals of the weight, and a sanitizer build of the program are checked too."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E, render as R

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
WEIGHTS = (1, 2, 127, 128, 129, 254, 255)
W, H = 40, 24


def build(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "render_blend_main.cpp"),
                    str(CSRC / "render_check.cpp"), "-o", str(out)], check=True)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("render_blend") / "render_blend_main")


def rule(p, c, a):
    """The rule of include/padel_hip.h on integer arrays."""
    return (np.asarray(p, np.int64) * (256 - a) + np.asarray(c, np.int64) * a + 128) >> 8


def pairs():
    """The harness's 65 536 pixels and colours, as (65536, 3) B G R."""
    p, c = (v.reshape(-1) for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    return np.stack([p, 255 - p, p ^ 0x55], 1), np.stack([c, 255 - c, c ^ 0xaa], 1)


def run_apply(exe, a, tmp_path):
    out = tmp_path / f"apply_{a}.bin"
    subprocess.run([str(exe), "apply", str(a), str(out)], check=True, capture_output=True)
    return np.fromfile(out, np.uint8).reshape(65536, 3)


def ramp(h=H, w=W, seed=0):
    """A frame whose channels differ from each other and take many values."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(7 * x + 3 * y + seed) & 255, (255 - 5 * x + 11 * y) & 255, (13 * x * y + 31) & 255], -1).astype(np.uint8)


def run_draw(exe, frame, marks, tmp_path):
    np.array([tuple(m) for m in marks], E.MARK_DTYPE).tofile(tmp_path / "marks.bin")
    frame.tofile(tmp_path / "in.bin")
    subprocess.run([str(exe), "draw", str(frame.shape[1]), str(frame.shape[0]), str(tmp_path / "marks.bin"), str(tmp_path / "in.bin"),
                    str(tmp_path / "out.bin")], check=True, capture_output=True)
    return np.fromfile(tmp_path / "out.bin", np.uint8).reshape(frame.shape)


def host(frame, marks):
    return R.render_host(frame[None], *R.pack([marks]))[0]


@pytest.mark.parametrize("a", WEIGHTS)
def test_apply_equals_the_rule_for_every_pixel_and_colour(harness, tmp_path, a):
    p, c = pairs()
    got = run_apply(harness, a, tmp_path)
    want = rule(p, c, a)
    assert want.min() >= 0 and want.max() <= 255
    assert np.array_equal(got, want.astype(np.uint8))
    # the twin in render.py, on the same 65 536 pixels: one frame of 256 x 256 per colour would be 256 calls — one row per colour instead
    g = p.reshape(256, 256, 3).astype(np.uint8)                          # [p, c]: row p holds the same pixel 256 times
    for col in (0, 77, 255):
        bgr = (int(c[col, 0]), int(c[col, 1]), int(c[col, 2]))
        drawn = host(g[:, col:col + 1].copy(), [R.blend(0, 0, 0, 255, bgr, a)])
        assert np.array_equal(drawn[:, 0], want.reshape(256, 256, 3)[:, col].astype(np.uint8))


@pytest.mark.parametrize("a", WEIGHTS)
def test_blending_a_colour_into_itself_changes_nothing_and_the_result_is_monotone(a):
    v = np.arange(256)
    assert np.array_equal(rule(v, v, a), v)                              # blend(p, p) == p
    grid = rule(v[:, None], v[None, :], a)                               # [p, c]
    assert (np.diff(grid, axis=0) >= 0).all()                            # monotone in p for every c
    assert (np.diff(grid, axis=1) >= 0).all()                            # and in c for every p
    assert ((grid >= np.minimum(v[:, None], v[None, :])) & (grid <= np.maximum(v[:, None], v[None, :]))).all()


def test_two_stacked_blends_depend_on_their_order(harness, tmp_path):
    frame = ramp()
    b1 = R.blend(2, 3, 30, 20, (250, 10, 40), 200)
    b2 = R.blend(10, 0, 39, 12, (5, 240, 90), 60)
    c1, c2 = np.array([250, 10, 40]), np.array([5, 240, 90])
    both = (slice(3, 13), slice(10, 31))                                 # rows 3..12, columns 10..30: under both
    results = []
    for marks, first, second in (([b1, b2], (c1, 200), (c2, 60)), ([b2, b1], (c2, 60), (c1, 200))):
        got = host(frame, marks)
        want = rule(rule(frame[both], *first), *second)
        assert np.array_equal(got[both], want.astype(np.uint8))
        assert np.array_equal(run_draw(harness, frame, marks, tmp_path), got)
        results.append(got)
    assert not np.array_equal(results[0][both], results[1][both])
    only1 = (slice(13, 21), slice(2, 31))                                # under b1 alone
    assert np.array_equal(results[0][only1], rule(frame[only1], c1, 200).astype(np.uint8))
    assert np.array_equal(results[0][22:], frame[22:])                   # outside both


def test_a_blend_under_and_over_an_opaque_disc(harness, tmp_path):
    frame = ramp(seed=9)
    panel = R.blend(5, 2, 34, 21, (255, 255, 255), 128)
    disc = R.disc(20, 12, 6, (0, 0, 255))
    inside = R.coverage(disc, H, W)
    dmask = np.zeros((H, W), bool)
    dmask[inside[0]:inside[0] + inside[2].shape[0], inside[1]:inside[1] + inside[2].shape[1]] = inside[2]
    assert dmask.sum() == 137
    pmask = np.zeros((H, W), bool)
    pmask[2:22, 5:35] = True
    white = np.array([255, 255, 255])
    # blend, then disc: the disc is opaque on top
    want = frame.copy()
    want[pmask] = rule(frame[pmask], white, 128)
    want[dmask] = (0, 0, 255)
    got = host(frame, [panel, disc])
    assert np.array_equal(got, want)
    assert np.array_equal(run_draw(harness, frame, [panel, disc], tmp_path), want)
    # disc, then blend: the disc is seen through the panel
    want = frame.copy()
    want[dmask] = (0, 0, 255)
    want[pmask] = rule(want[pmask], white, 128)
    got = host(frame, [disc, panel])
    assert np.array_equal(got, want)
    assert np.array_equal(run_draw(harness, frame, [disc, panel], tmp_path), want)
    assert tuple(got[12, 20]) == (128, 128, 255)


def test_the_blend_covers_the_fill_rectangle_with_its_corners(harness, tmp_path):
    frame = ramp(seed=4)
    for m in (R.blend(30, 20, 4, 6, (1, 2, 3), 77), R.blend(-5, -5, 3, 3, (9, 9, 9), 1), R.blend(38, 22, 100, 100, (0, 0, 0), 255),
              R.blend(50, 0, 60, 10, (0, 0, 0), 128)):
        fill = R.coverage((E.MARK_FILL,) + tuple(m[1:6]) + (0, 0), H, W)
        assert (fill is None) == (R.coverage(m, H, W) is None)
        got = run_draw(harness, frame, [m], tmp_path)
        assert np.array_equal(got, host(frame, [m]))
        changed = (got != frame).any(-1)
        if fill is None:
            assert not changed.any()
        else:
            inside = np.zeros((H, W), bool)
            inside[fill[0]:fill[0] + fill[2].shape[0], fill[1]:fill[1] + fill[2].shape[1]] = True
            assert not changed[~inside].any()


REFUSALS = [("weight 0", 0), ("weight 256", 256), ("weight -1", -1)]


@pytest.mark.parametrize("name,weight", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_weight_outside_1_to_255_is_refused(harness, tmp_path, name, weight):
    marks, first = R.pack([[R.blend(1, 1, 5, 5, (1, 2, 3), weight)]])
    why = E.render_check(1, 16, 16, marks, first)
    assert why is not None and "weight" in why and str(weight) in why
    with pytest.raises(ValueError, match="weight"):
        R.render_host(np.zeros((1, 16, 16, 3), np.uint8), marks, first)
    marks.tofile(tmp_path / "marks.bin")
    said = subprocess.run([str(harness), "check", str(tmp_path / "marks.bin")], check=True, capture_output=True, text=True).stdout
    assert "weight" in said
    done = subprocess.run([str(harness), "apply", str(weight), str(tmp_path / "x.bin")], capture_output=True, text=True)
    assert done.returncode == 3 and "weight" in done.stderr


def test_what_else_the_checks_say_about_kind_6():
    def why(mark):
        return E.render_check(1, 16, 16, *R.pack([[mark]]))
    for size in (0, 255):                                                # accepted and ignored, as for a fill
        assert why((E.MARK_BLEND, 1, 1, 5, 5, size, 0x102030, 128)) is None
    assert "size" in why((E.MARK_BLEND, 1, 1, 5, 5, 256, 0, 128))
    assert "size" in why((E.MARK_BLEND, 1, 1, 5, 5, -1, 0, 128))
    assert "coordinate" in why((E.MARK_BLEND, 1, 1, 9000, 5, 0, 0, 128))
    assert "colour" in why((E.MARK_BLEND, 1, 1, 5, 5, 0, 0x1000000, 128))
    for kind in (0, 7, 9):
        assert "unknown kind" in why((kind, 0, 0, 0, 0, 1, 0, 0))
    for kind in (E.MARK_DISC, E.MARK_SEGMENT, E.MARK_FILL, E.MARK_BOX):  # a non-zero arg on the opaque non-glyph kinds stays refused
        assert "arg" in why((kind, 1, 1, 5, 5, 1, 0, 128))
    assert E.MARK_BLEND == 6 and R.blend(1, 2, 3, 4, (5, 6, 7), 8) == (6, 1, 2, 3, 4, 0, 0x070605, 8)
    frame = ramp()
    a = R.render_host(frame[None], *R.pack([[(E.MARK_BLEND, 1, 1, 9, 9, 0, 0x102030, 99)]]))
    b = R.render_host(frame[None], *R.pack([[(E.MARK_BLEND, 1, 1, 9, 9, 255, 0x102030, 99)]]))
    assert np.array_equal(a, b)


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build(tmp_path / "render_blend_asan", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
    p, c = pairs()
    for a in WEIGHTS:
        done = subprocess.run([str(exe), "apply", str(a), str(tmp_path / "a.bin")], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        assert np.array_equal(np.fromfile(tmp_path / "a.bin", np.uint8).reshape(65536, 3), rule(p, c, a).astype(np.uint8))
    frame = ramp(seed=2)
    marks = [R.blend(-8192, -8192, 8191, 8191, (255, 255, 255), 128), R.disc(20, 12, 6, (0, 0, 255)), R.blend(38, 22, 100, 100, (0, 0, 0), 255),
             R.segment(-3, 2, 60, 30, 3, (1, 2, 3)), *R.text("A1", 30, 15, 2, (9, 8, 7)), R.blend(0, 0, 39, 23, (7, 7, 7), 1)]
    np.array([tuple(m) for m in marks], E.MARK_DTYPE).tofile(tmp_path / "marks.bin")
    frame.tofile(tmp_path / "in.bin")
    done = subprocess.run([str(exe), "draw", str(W), str(H), str(tmp_path / "marks.bin"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                          capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(H, W, 3), host(frame, marks))
    for weight in (0, 256, -1):
        done = subprocess.run([str(exe), "apply", str(weight), str(tmp_path / "x.bin")], capture_output=True, text=True)
        assert done.returncode == 3 and "weight" in done.stderr and "runtime error" not in done.stderr and "Sanitizer" not in done.stderr
