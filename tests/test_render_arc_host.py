"""``PA_MARK_ARC`` without a GPU: the elliptical ring cut to octants (include/padel_hip.h), and what is composed of it on the host —
the players' ``round_bounding_box``, ``corner_bounding_box`` and ``ellipse`` annotators and the runner's ``ball_trail``.

``mark_covers`` / ``mark_bbox`` (csrc/render_marks.h) are what the render kernel covers and culls by; the stand-alone program
tests/render_arc_main.cpp, built with g++ over that header and csrc/render_check.cpp, evaluates them on the CPU, once more under the
address and undefined-behaviour sanitizers.  ``render.coverage`` states the rule a second time, in numpy; the two must agree bit for
bit, and the properties below (octants that tile the ring, rotations, a thin ring that is closed) are stated on the pixels alone."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

from padel_analytics_amd import engine as E, render as R, video
from padel_analytics_amd.detections import Detections
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.ball_tracker import Ball
from padel_analytics_amd.trackers.players_tracker import Player, Players
from tests.court_script import Stored

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
W, H = 64, 48
FAR = (8192 - W, 8192 - H)                   # the window in the far corner of the largest frame
EIGHT, FOUR = np.ones((3, 3)), ndimage.generate_binary_structure(2, 1)


def build(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "render_arc_main.cpp"),
                    str(CSRC / "render_check.cpp"), "-o", str(out)], check=True)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("render_arc") / "render_arc_main")


def run_cover(exe, marks, tmp_path, origin=(0, 0), w=W, h=H):
    """-> (covered (k, h, w) bool, boxes (k, 4)) of the program over the window at ``origin``."""
    np.array([tuple(m) for m in marks], E.MARK_DTYPE).tofile(tmp_path / "marks.bin")
    done = subprocess.run([str(exe), "cover", str(origin[0]), str(origin[1]), str(w), str(h), str(tmp_path / "marks.bin"), str(tmp_path / "cover.bin"),
                           str(tmp_path / "boxes.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr)
    return (np.fromfile(tmp_path / "cover.bin", np.uint8).reshape(len(marks), h, w).astype(bool),
            np.fromfile(tmp_path / "boxes.bin", np.int32).reshape(len(marks), 4))


def cov(mark, h, w):
    """``render.coverage`` as a whole (h, w) frame."""
    out = np.zeros((h, w), bool)
    c = R.coverage(mark, h, w)
    if c is not None:
        out[c[0]:c[0] + c[2].shape[0], c[1]:c[1] + c[2].shape[1]] = c[2]
    return out


def union(marks, h, w):
    out = np.zeros((h, w), bool)
    for m in marks:
        out |= cov(m, h, w)
    return out


def window(mark, origin, w=W, h=H):
    """``render.coverage`` over the window at ``origin`` (of a frame that ends with the window)."""
    x0, y0 = origin
    c = R.coverage(mark, y0 + h, x0 + w)
    out = np.zeros((h, w), bool)
    if c is None:
        return out
    ay, ax, m = c
    for y in range(max(ay, y0), min(ay + m.shape[0], y0 + h)):
        lo, hi = max(ax, x0), min(ax + m.shape[1], x0 + w)
        if lo < hi:
            out[y - y0, lo - x0:hi - x0] = m[y - ay, lo - ax:hi - ax]
    return out


def seeded_arcs(seed=5, count=3060):
    """Arcs whose ring crosses the 64 x 48 frame: every mask twelve times, semi-axes from 1 to 4095, thicknesses from 1 to 255, the
    centre wherever that puts it (clipped to the coordinate range), then centres at random and at the coordinate limits."""
    rng = np.random.default_rng(seed)
    lim = (R.COORD_MIN, R.COORD_MAX)

    def axis():
        r = rng.random()
        return int(rng.integers(1, 40)) if r < 0.4 else int(rng.integers(1, 600)) if r < 0.7 else int(rng.choice([1, 2, 4094, 4095, int(rng.integers(1, 4096))]))

    marks = []
    for k in range(count):
        a, b, t = axis(), axis(), int(rng.choice([1, 1, 2, 3, 4, 254, 255, int(rng.integers(1, 256))]))
        r = rng.random()
        if r < 0.8:                                                      # a point of the ring (somewhere in its thickness) on a pixel in or near the frame
            th, s = rng.uniform(0, 2 * np.pi), 1 - rng.random() * min(t, min(a, b)) / min(a, b)
            x = int(rng.integers(-4, W + 4)) - int(round(s * a * np.cos(th)))
            y = int(rng.integers(-4, H + 4)) - int(round(s * b * np.sin(th)))
        elif r < 0.93:
            x, y = int(rng.integers(-300, 300)), int(rng.integers(-300, 300))
        else:
            x, y = int(rng.choice([lim[0], lim[1], 0, int(rng.integers(*lim))])), int(rng.choice([lim[0], lim[1], H - 1, int(rng.integers(*lim))]))
        marks.append(R.arc(x, y, a, b, t, 1 + k, 1 + k % 255))
    # what the rule singles out: the centre pixel, one pixel, no hole, the thinnest hole, both limits of every field
    marks += [R.arc(30, 20, 1, 1, 1, 1, 0x01), R.arc(30, 20, 1, 1, 1, 1, 0xFE), R.arc(30, 20, 9, 9, 9, 1, 0xFF), R.arc(30, 20, 9, 9, 8, 1, 0xFF),
              R.arc(30, 20, 9, 1, 1, 1, 0xFF), R.arc(30, 20, 1, 9, 255, 1, 0xFF), R.arc(30, 20, 40, 14, 2, 1, 0x9F), R.arc(30, 20, 20, 20, 1, 1, 0x80),
              R.arc(4095 + 10, 24, 4095, 4095, 1, 1, 0xFF), R.arc(32, -4095 + 20, 4095, 4095, 255, 1, 0xFF), R.arc(32, 4095 + 20, 4095, 1, 1, 1, 0xFF),
              R.arc(lim[0], lim[0], 4095, 4095, 255, 1, 0xFF), R.arc(lim[1], lim[1], 4095, 4095, 1, 1, 0xFF), R.arc(lim[0], 24, 4095, 4095, 1, 1, 0x01)]
    return marks


def far_arcs(seed=6, count=300):
    """Arcs for the window in the far corner of an 8192 x 8192 frame: modest semi-axes around it (the twin evaluates the box's whole
    overlap with the frame), and the largest ones centred at the opposite coordinate limit, |dx| and |dy| as large as they get."""
    rng = np.random.default_rng(seed)
    marks = []
    for k in range(count):
        a, b = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        th = rng.uniform(0, 2 * np.pi)
        x = min(FAR[0] + int(rng.integers(-4, W + 4)) - int(round(a * np.cos(th))), R.COORD_MAX)
        y = min(FAR[1] + int(rng.integers(-4, H + 4)) - int(round(b * np.sin(th))), R.COORD_MAX)
        marks.append(R.arc(x, y, a, b, int(rng.choice([1, 2, 3, 255])), 1, 1 + (7 * k) % 255))
    marks += [R.arc(R.COORD_MAX, R.COORD_MAX, 60, 40, 2, 1, 0xFF), R.arc(R.COORD_MAX, R.COORD_MAX, 1, 1, 1, 1, 0xFF),
              R.arc(R.COORD_MIN, R.COORD_MIN, 4095, 4095, 1, 1, 0xFF), R.arc(R.COORD_MIN, R.COORD_MAX, 4095, 1, 255, 1, 0xFF),
              R.arc(R.COORD_MAX, R.COORD_MIN, 1, 4095, 1, 1, 0xFF)]
    return marks


def test_kind_8_is_the_arc_and_its_fields():
    assert E.MARK_ARC == 8
    assert R.arc(3, -4, 10, 5, 2, (1, 2, 3), 0x9F) == (8, 3, -4, 10, 5, 2, 0x030201, 0x9F)
    assert R.arc(3, 4, 10, 5, 2, 7)[7] == 0xFF                           # the whole ring unless a mask says otherwise
    marks, first = R.pack([[R.arc(8, 8, 5, 3, 1, 0x102030, 0xFF)]])
    assert E.render_check(1, 16, 16, marks, first) is None
    for kind in (7, 9):
        assert "unknown kind" in E.render_check(1, 16, 16, *R.pack([[(kind, 8, 8, 5, 3, 1, 0, 0xFF)]]))


def test_seeded_arcs_equal_the_twin_bit_for_bit(harness, tmp_path):
    marks = seeded_arcs()
    assert len(marks) > 3000 and {m[7] for m in marks} == set(range(1, 256))
    got, boxes = run_cover(harness, marks, tmp_path)
    drew = 0
    for k, m in enumerate(marks):
        assert np.array_equal(got[k], cov(m, H, W)), (k, m)
        assert tuple(boxes[k]) == (m[1] - m[3], m[2] - m[4], m[1] + m[3], m[2] + m[4]), (k, m)
        ys, xs = np.nonzero(got[k])                                      # (the program has checked it for every pixel: status 2)
        if len(ys):
            drew += 1
            assert xs.min() >= boxes[k][0] and xs.max() <= boxes[k][2] and ys.min() >= boxes[k][1] and ys.max() <= boxes[k][3], (k, m)
    assert drew > 1500, drew                                             # the seeds do put rings into the frame


def test_arcs_at_the_far_corner_and_the_coordinate_limits(harness, tmp_path):
    marks = far_arcs()
    got, boxes = run_cover(harness, marks, tmp_path, origin=FAR)
    drew = 0
    for k, m in enumerate(marks):
        assert np.array_equal(got[k], window(m, FAR)), (k, m)
        drew += int(got[k].any())
    assert drew > 100, drew                                              # the seeds do put rings into the window
    assert got[300].any() and got[301].sum() == 3 and not got[302:].any()


SHAPES = [(40, 14), (20, 20), (9, 9), (7, 30), (33, 1), (1, 6), (1, 1), (2, 2), (12, 5)]


@pytest.mark.parametrize("a,b", SHAPES)
def test_the_eight_octants_are_disjoint_and_their_union_is_the_ring(a, b):
    h, w = 2 * b + 5, 2 * a + 6
    cx, cy = a + 3, b + 2
    for t in (1, 2, 3, 255):
        full = cov(R.arc(cx, cy, a, b, t, 1, 0xFF), h, w)
        parts = [cov(R.arc(cx, cy, a, b, t, 1, 1 << k), h, w) for k in range(8)]
        assert np.array_equal(np.sum(parts, axis=0), full.astype(int)), (a, b, t)      # each ring pixel in exactly one octant
        assert full[cy, cx + a] and full[cy, cx - a] and full[cy - b, cx] and full[cy + b, cx]
        assert parts[0][cy, cx + a] and parts[2][cy + b, cx] and parts[4][cy, cx - a] and parts[6][cy - b, cx]      # an octant starts ON its axis
        for mask in (0x9F, 0x30, 0x55, 0xC3):
            want = np.any([parts[k] for k in range(8) if mask >> k & 1], axis=0)
            assert np.array_equal(cov(R.arc(cx, cy, a, b, t, 1, mask), h, w), want), (a, b, t, mask)
        if t >= min(a, b):                                               # no hole: the filled ellipse
            y, x = np.mgrid[0:h, 0:w].astype(np.int64)
            assert np.array_equal(full, (x - cx) ** 2 * b * b + (y - cy) ** 2 * a * a <= a * a * b * b)


@pytest.mark.parametrize("a,b", SHAPES)
def test_rotating_the_mask_rotates_the_image(a, b):
    h = w = 2 * max(a, b) + 7
    c = max(a, b) + 3
    centre = np.zeros((h, w), bool)
    centre[c, c] = True
    rot4 = lambda m: ((m << 4) | (m >> 4)) & 0xFF
    rot2 = lambda m: ((m << 2) | (m >> 6)) & 0xFF
    for t in (1, 3, 255):
        for mask in (0x01, 0x02, 0x9F, 0x30, 0x6D, 0x80):
            img = cov(R.arc(c, c, a, b, t, 1, mask), h, w) & ~centre
            half = cov(R.arc(c, c, a, b, t, 1, rot4(mask)), h, w) & ~centre
            assert np.array_equal(half, img[::-1, ::-1]), (a, b, t, mask)
            if a == b:                                                   # a quarter turn from +x towards +y (y points down)
                quarter = cov(R.arc(c, c, a, b, t, 1, rot2(mask)), h, w) & ~centre
                assert np.array_equal(quarter, np.rot90(img, -1)), (a, t, mask)


def ring_shapes():
    """a = 1..299 with b = 7a/20, a, a/2, a/8 and 1 (each at least 1): 1 471 different shapes."""
    return sorted({(a, max(1, b)) for a in range(1, 300) for b in (7 * a // 20, a, a // 2, a // 8, 1)})


def test_a_thin_full_ring_is_closed_and_thicker_ones_need_no_rim_rule():
    shapes = ring_shapes()
    assert len(shapes) == 1471
    gaps = 0
    for a, b in shapes:
        h, w = 2 * b + 3, 2 * a + 3                                      # one pixel of outside all round
        y, x = np.mgrid[0:h, 0:w].astype(np.int64)
        dx, dy = x - (a + 1), y - (b + 1)
        inside = lambda A, B: dx * dx * B * B + dy * dy * A * A <= A * A * B * B
        outer = inside(a, b)
        two = lambda t: outer & ~inside(a - t, b - t) if a - t >= 1 and b - t >= 1 else outer      # the two-ellipse ring alone
        ring = cov(R.arc(a + 1, b + 1, a, b, 1, 1, 0xFF), h, w)
        assert not (ring & ~outer).any() and not (two(1) & ~ring).any(), (a, b)
        assert ndimage.label(ring, structure=EIGHT)[1] == 1, (a, b)      # 8-connected
        gaps += int(ndimage.label(two(1), structure=EIGHT)[1] != 1 or _leaks(two(1), outer))
        assert not _leaks(ring, outer), (a, b)                           # and it separates inside from outside
        for t in (2, 3, 4, 6):
            assert np.array_equal(cov(R.arc(a + 1, b + 1, a, b, t, 1, 0xFF), h, w), two(t)), (a, b, t)
    assert gaps > 100, gaps                                              # without the rim rule many of these rings are open


def _leaks(ring, outer) -> bool:
    """Does some pixel inside the outer ellipse that the ring leaves free hang together (4-connected) with the outside?"""
    free, n = ndimage.label(~ring, structure=FOUR)
    return bool((free[outer & ~ring] == free[0, 0]).any())


# ------------------------------------------------------------------------------------------ the annotators
BLUE, WHITE = 0x0000FF, 0xFFFFFF
ANNOTATORS = ("rectangle_bounding_box", "round_bounding_box", "corner_bounding_box", "ellipse")


class _Info:
    def __init__(self, w, h): self.width, self.height = w, h


def player(x0=100.7, y0=60.2, x1=180.9, y1=200.5, tid=7):
    return Player(Detections(xyxy=np.array([[x0, y0, x1, y1]], np.float32), confidence=np.array([0.876], np.float32), class_id=np.array([0]),
                             tracker_id=np.array([tid])))


def test_known_answers_of_the_three_annotators():
    p, info = player(), _Info(1280, 720)
    rect = p.marks(video_info=info)
    assert rect[0] == (E.MARK_BOX, 100, 60, 180, 200, 2, BLUE, 0) and rect == p.marks(video_info=info, annotator="rectangle_bounding_box")
    label = rect[1:]                                                     # plate and text: the same under every annotator
    ell = p.marks(video_info=info, annotator="ellipse")
    assert ell[0] == (E.MARK_ARC, 140, 200, 80, 28, 2, BLUE, 0x9F) and ell[1:] == label
    assert ell[0][0] != E.MARK_BOX
    rnd = p.marks(video_info=info, annotator="round_bounding_box")
    fill = lambda *c: (E.MARK_FILL, *c, 0, BLUE, 0)
    arc = lambda x, y, m: (E.MARK_ARC, x, y, 24, 24, 2, BLUE, m)
    assert rnd[:8] == [fill(124, 60, 156, 61), fill(124, 199, 156, 200), fill(100, 84, 101, 176), fill(179, 84, 180, 176),
                       arc(124, 84, 0x30), arc(156, 84, 0xC0), arc(156, 176, 0x03), arc(124, 176, 0x0C)]
    assert rnd[8:] == label
    cor = p.marks(video_info=info, annotator="corner_bounding_box")
    assert cor[:8] == [fill(100, 60, 114, 61), fill(100, 60, 101, 74), fill(166, 60, 180, 61), fill(179, 60, 180, 74),
                       fill(166, 199, 180, 200), fill(179, 186, 180, 200), fill(100, 199, 114, 200), fill(100, 186, 101, 200)]
    assert cor[8:] == label
    thick = p.marks(video_info=_Info(1920, 1080), annotator="ellipse")[0]
    assert thick[5] == 4
    small = player(10, 10, 16, 40)                                       # w = 6: corner length 3, radius 3 * 3 // 5 = 1
    assert small.marks(video_info=info, annotator="corner_bounding_box")[0] == fill(10, 10, 12, 11)
    assert small.marks(video_info=info, annotator="round_bounding_box")[4] == (E.MARK_ARC, 11, 11, 1, 1, 2, BLUE, 0x30)
    assert small.marks(video_info=info, annotator="ellipse")[0] == (E.MARK_ARC, 13, 40, 6, 2, 2, BLUE, 0x9F)
    flat = player(10, 10, 10, 40)                                        # w = 0: the ellipse keeps a semi-axis of 1
    assert flat.marks(video_info=info, annotator="ellipse")[0][3:5] == (1, 1)
    ps = Players([p, small])
    assert Player.ANNOTATORS == ANNOTATORS
    for name in ANNOTATORS:
        kw = dict(video_info=info, annotator=name, show_confidence=False)
        assert ps.marks(**kw) == p.marks(**kw) + small.marks(**kw)
        assert E.render_check(1, 720, 1280, *R.pack([ps.marks(**kw)])) is None


def test_an_unknown_annotator_is_refused_by_name():
    with pytest.raises(ValueError) as e:
        player().marks(video_info=_Info(1280, 720), annotator="triangle")
    for name in ("triangle", "rectangle_bounding_box", "round_bounding_box", "corner_bounding_box", "ellipse"):
        assert name in str(e.value)


def outline(name, x0, y0, x1, y1, t, h, w):
    marks = Player.outline_marks(name, x0, y0, x1, y1, t, 1)
    assert E.render_check(1, h, w, *R.pack([marks])) is None
    return union(marks, h, w), marks


def test_the_rounded_box_is_the_box_at_radius_0_and_a_closed_curve_above():
    h, w = 70, 90
    seen_round = 0
    for bw in (0, 1, 2, 3, 4, 5, 7, 10, 11, 16, 23, 40, 61):
        for bh in (0, 3, 4, 6, 9, 10, 17, 33, 52):
            for t in (1, 2, 4):
                x0, y0 = 5, 6
                x1, y1 = x0 + bw, y0 + bh
                got, marks = outline("round_bounding_box", x0, y0, x1, y1, t, h, w)
                r = 3 * (min(bw, bh) // 2) // 5
                box = cov(R.box(x0, y0, x1, y1, t, 1), h, w)
                inside = np.zeros((h, w), bool)
                inside[y0:y1 + 1, x0:x1 + 1] = True
                assert not (got & ~inside).any(), (bw, bh, t)
                if r == 0:
                    assert len(marks) == 4 and np.array_equal(got, box), (bw, bh, t)
                    continue
                seen_round += 1
                assert len(marks) == 8 and all(m[0] == E.MARK_ARC and m[3] == m[4] == r for m in marks[4:])
                assert ndimage.label(got, structure=EIGHT)[1] == 1, (bw, bh, t)
                free, _ = ndimage.label(~got, structure=FOUR)
                cy, cx = (y0 + y1) // 2, (x0 + x1) // 2                  # the middle of the box, where the curve leaves it free: fenced in
                assert got[cy, cx] or free[cy, cx] != free[0, 0], (bw, bh, t)
                assert not got[cy, cx] or min(bw, bh) < 2 * t + 2, (bw, bh, t)
                assert not got[y0, x0] and not got[y1, x1] and got[y0, x0 + r] and got[y0 + r, x0] and got[y1, x1 - r]      # the corners are cut
    assert seen_round > 150


def test_the_corner_box_and_the_ellipse_on_pixels():
    h, w = 70, 90
    for t in (1, 2, 4):
        got, marks = outline("corner_bounding_box", 5, 6, 65, 46, t, h, w)
        box = cov(R.box(5, 6, 65, 46, t, 1), h, w)
        assert len(marks) == 8 and not (got & ~box).any() and ndimage.label(got, structure=EIGHT)[1] == 4
        assert got[6, 5:20].all() and not got[6, 20] and got[6:21, 5].all() and not got[21, 5] and got[46, 51:66].all() and not got[46, 50]
        assert got.sum() == 4 * (2 * 15 * t - t * t)
    got, marks = outline("corner_bounding_box", 5, 6, 11, 46, 4, h, w)   # w = 6: length 3, the thickness cut to the box
    assert not (got & ~cov(R.fill(5, 6, 11, 46, 1), h, w)).any() and got[6, 5:12].all() and got[46, 5:12].all() and not got[10:43].any()
    assert outline("corner_bounding_box", 5, 6, 6, 46, 2, h, w)[1] == []
    got, marks = outline("ellipse", 30, 10, 60, 40, 2, h, w)             # centre (45, 40), a = 30, b = 10
    full = cov(R.arc(45, 40, 30, 10, 2, 1, 0xFF), h, w)
    assert marks == [R.arc(45, 40, 30, 10, 2, 1, 0x9F)] and not (got & ~full).any()
    assert np.array_equal(got[40:], full[40:])                           # everything from the centre's row down (octants 0..3) ...
    assert got[40, 15] and got[40, 75] and got[50, 45] and not got[30, 45] and full[30, 45]      # ... and the top is open
    assert got[:40].any() and ndimage.label(got, structure=EIGHT)[1] == 1


# ------------------------------------------------------------------------------------------ the refusals
REFUSALS = [("a = 0", (E.MARK_ARC, 8, 8, 0, 3, 1, 0, 0xFF), "semi-axis"), ("a = 4096", (E.MARK_ARC, 8, 8, 4096, 3, 1, 0, 0xFF), "semi-axis"),
            ("b = 0", (E.MARK_ARC, 8, 8, 3, 0, 1, 0, 0xFF), "semi-axis"), ("b = -1", (E.MARK_ARC, 8, 8, 3, -1, 1, 0, 0xFF), "semi-axis"),
            ("b = 4096", (E.MARK_ARC, 8, 8, 3, 4096, 1, 0, 0xFF), "semi-axis"),
            ("t = 0", (E.MARK_ARC, 8, 8, 5, 3, 0, 0, 0xFF), "size"), ("t = 256", (E.MARK_ARC, 8, 8, 5, 3, 256, 0, 0xFF), "size"),
            ("mask 0", (E.MARK_ARC, 8, 8, 5, 3, 1, 0, 0), "octant mask"), ("mask 256", (E.MARK_ARC, 8, 8, 5, 3, 1, 0, 256), "octant mask"),
            ("mask -1", (E.MARK_ARC, 8, 8, 5, 3, 1, 0, -1), "octant mask"),
            ("centre", (E.MARK_ARC, 8192, 8, 5, 3, 1, 0, 0xFF), "coordinate"), ("colour", (E.MARK_ARC, 8, 8, 5, 3, 1, 0x1000000, 0xFF), "colour")]


@pytest.mark.parametrize("name,mark,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_an_arc_out_of_range_is_refused_with_the_reason(harness, tmp_path, name, mark, words):
    marks, first = R.pack([[R.disc(3, 3, 2, 1), mark]])
    why = E.render_check(1, 16, 16, marks, first)
    assert why is not None and words in why and "mark 1" in why, why
    with pytest.raises(ValueError, match=words):
        R.render_host(np.zeros((1, 16, 16, 3), np.uint8), marks, first)
    marks.tofile(tmp_path / "marks.bin")
    said = subprocess.run([str(harness), "check", str(tmp_path / "marks.bin")], check=True, capture_output=True, text=True).stdout
    assert said.strip() == why
    marks[1:].tofile(tmp_path / "one.bin")
    done = subprocess.run([str(harness), "cover", "0", "0", "16", "16", str(tmp_path / "one.bin"), str(tmp_path / "c.bin"), str(tmp_path / "b.bin")],
                          capture_output=True, text=True)
    assert done.returncode == 3 and words in done.stderr


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build(tmp_path / "render_arc_asan", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
    marks = seeded_arcs()
    got, _ = run_cover(exe, marks, tmp_path)                             # (asserts status 0 and an empty stderr)
    for k in range(0, len(marks), 97):
        assert np.array_equal(got[k], cov(marks[k], H, W)), k
    far = far_arcs()
    got, _ = run_cover(exe, far, tmp_path, origin=FAR)
    assert np.array_equal(got[300], window(far[300], FAR))
    np.array([REFUSALS[1][1]], E.MARK_DTYPE).tofile(tmp_path / "bad.bin")
    done = subprocess.run([str(exe), "cover", "0", "0", "16", "16", str(tmp_path / "bad.bin"), str(tmp_path / "c.bin"), str(tmp_path / "b.bin")],
                          capture_output=True, text=True)
    assert done.returncode == 3 and "semi-axis" in done.stderr and "runtime error" not in done.stderr and "Sanitizer" not in done.stderr


# ------------------------------------------------------------------------------------------ the runner's marks
N_CLIP = 12
BALLS = [(10, 11, 1), (12, 13, 1), (0, 0, 0), (16, 17, 1), (18, 19, 1), (20, 21, 1), (22, 23, 0), (24, 25, 1), (26, 27, 1), (28, 29, 1), (30, 31, 1), (32, 33, 1)]
YELLOW = (0, 255, 255)                       # BGR of RGB (255, 255, 0)


def stub_runner(**kw):
    frames = np.zeros((N_CLIP, 32, 48, 3), np.uint8)
    players = [Players([player(4 + i, 5, 24 + i, 29, tid=3)]) for i in range(N_CLIP)]
    balls = [Ball(i, (float(x) + 0.5, float(y) + 0.25), v) for i, (x, y, v) in enumerate(BALLS)]
    seg = kw.get("segments")
    keep = [i for lo, hi in seg for i in range(lo, hi)] if seg else range(N_CLIP)
    trackers = [Stored("players_tracker", Players, [players[i] for i in keep]), Stored("ball_tracker", Ball, [balls[i] for i in keep])]
    annotator = kw.pop("annotator", "rectangle_bounding_box")
    trackers[0].draw_kwargs = lambda: {"video_info": None, "annotator": annotator, "show_confidence": False}
    return TrackingRunner(trackers, video.ArrayClip(frames), "unused.mp4", **kw), players, balls


def trail(*xy):
    return [m for x, y in xy for m in (R.disc(x, y, 3, YELLOW), R.disc(x, y, 2, WHITE))]


def test_frame_marks_with_a_ball_trail():
    plain, players, balls = stub_runner()
    label = lambda i: R.text(f"FRAME: {i + 1}", 20, 30, 3, (0, 255, 255))
    base = lambda i: label(i) + players[i].marks(video_info=None, annotator="rectangle_bounding_box", show_confidence=False) + balls[i].marks()
    assert plain.ball_trail == 0 and all(plain.frame_marks(i) == base(i) for i in range(N_CLIP))       # the default: nothing is added
    assert balls[4].marks() == [R.disc(18, 19, 6, (0, 255, 0))]
    r, _, _ = stub_runner(ball_trail=3)
    assert r.frame_marks(0) == base(0) + trail((10, 11))                 # the first frames of a clip: what there is
    assert r.frame_marks(1) == base(1) + trail((12, 13), (10, 11))       # newest first
    assert r.frame_marks(2) == base(2) + trail((12, 13), (10, 11))       # an invisible ball is not drawn ...
    assert r.frame_marks(3) == base(3) + trail((16, 17), (12, 13))       # ... and keeps its place in the queue
    assert r.frame_marks(5) == base(5) + trail((20, 21), (18, 19), (16, 17))
    assert r.frame_marks(6) == base(6) + trail((20, 21), (18, 19))
    assert stub_runner(ball_trail=1)[0].frame_marks(6) == base(6)
    assert stub_runner(ball_trail=1)[0].frame_marks(7) == base(7) + trail((24, 25))
    assert stub_runner(ball_trail=50)[0].frame_marks(4) == base(4) + trail((18, 19), (16, 17), (12, 13), (10, 11))
    assert E.render_check(1, 32, 48, *R.pack([r.frame_marks(5)])) is None
    with pytest.raises(ValueError, match="ball_trail"):
        stub_runner(ball_trail=-1)


def test_a_trail_does_not_reach_across_a_cut():
    r, players, balls = stub_runner(ball_trail=3, segments=[(0, 2), (7, 12)])
    kept = [0, 1, 7, 8, 9, 10, 11]
    own = lambda k: balls[kept[k]].marks()
    assert r.frame_marks(1)[-4:] == trail((12, 13), (10, 11))
    assert r.frame_marks(2)[-3:] == own(2) + trail((24, 25))             # kept position 2 is source frame 7: the segment's first
    assert r.frame_marks(3)[-5:] == own(3) + trail((26, 27), (24, 25))
    assert r.frame_marks(4)[-7:] == own(4) + trail((28, 29), (26, 27), (24, 25))
    assert r.frame_marks(6)[-7:] == own(6) + trail((32, 33), (30, 31), (28, 29))
    assert [chr(g[7]) for g in r.frame_marks(2)[:8]] == list("FRAME: 8")


@pytest.mark.parametrize("name", ANNOTATORS)
def test_frame_marks_under_every_annotator(name):
    r, players, balls = stub_runner(annotator=name)
    for i in (0, 5):
        m = r.frame_marks(i)
        own = players[i].marks(video_info=None, annotator=name, show_confidence=False)
        assert m[8:8 + len(own)] == own and m[8 + len(own):] == balls[i].marks()
        assert (own[0][0] == E.MARK_BOX) == (name == "rectangle_bounding_box")
        assert E.render_check(1, 32, 48, *R.pack([m])) is None
