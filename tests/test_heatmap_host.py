"""The heat maps without a GPU (include/padel_hip.h, ``pa_heat_accumulate``): answers known beforehand, the numpy twin
``heatmap.accumulate_host`` against an independent per-pixel loop, the shared header csrc/heat_math.h through the stand-alone program
tests/heat_main.cpp (g++; once more under the address and undefined-behaviour sanitizers) bit for bit against the twin, the state
carried over calls, the level at and around ``full``, the saturating sum, ``alpha`` 0 and 256, frames that are not valid, one case per
refusal of ``pa_heat_check`` with the twin raising the same words, the ramp, ``HeatMap.points`` against ``TopDownView.to_canvas``, and
the runner over a stand-in engine that records its calls and answers them with the twins."""
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E, heatmap as HM, mjpeg, projected_court as PC, render as R, topdown as T, video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.ball_tracker import Ball
from padel_analytics_amd.trackers.players_tracker import Players
from tests import heat_cases as HC, identity_script as S, synth  # noqa: F401  (synth registers the synthetic:// frame source)
from tests.court_script import Stored, court_for, stub_trackers
from tests.twin_engine import StandInEngine, TwinEngine

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
LUT = HM.heat_lut()


def one_point(oh, ow, x, y, r, planes=1, plane=0, state=None, **call):
    state = np.zeros((planes, oh, ow), np.uint32) if state is None else state
    canvases = np.full((1, oh, ow, 3), 50, np.uint8)
    HM.accumulate_host(canvases, state, [[x, y, plane]], [0, 1], [1], **dict(dict(r=r, full=255, alpha=160, show_mask=(1 << planes) - 1, lut=LUT), **call))
    return canvases, state


@pytest.fixture(scope="module")
def seeded():
    """The seeded cases and the twin's answers, computed once."""
    cases = HC.seeded_cases()
    return cases, [HC.twin(c) for c in cases]


# ---------------------------------------------------------------------------------------------- answers known beforehand
def test_the_bump_of_radius_2_worked_by_hand():
    """r r = 4: the centre adds 255 * 4 / 4 = 255, a neighbour (d2 = 1) 255 * 3 / 4 = 191, a diagonal (d2 = 2) 255 * 2 / 4 = 127, d2 = 4
    is the rim: nothing.  255 + 4 * 191 + 4 * 127 = 1527."""
    _, state = one_point(7, 9, 4, 3, 2)
    assert state[0, 2:5, 3:6].tolist() == [[127, 191, 127], [191, 255, 191], [127, 191, 127]]
    assert int(state.sum()) == 1527
    assert HM.splat(2).tolist() == [[127, 191, 127], [191, 255, 191], [127, 191, 127]]


@pytest.mark.parametrize("r", [1, 2, 255])
def test_the_centre_gets_255_and_the_rim_nothing(r):
    oh = ow = 2 * r + 3
    _, state = one_point(oh, ow, r + 1, r + 1, r)
    assert state[0, r + 1, r + 1] == 255
    assert state[0, r + 1, 1] == 0 and state[0, 1, r + 1] == 0 and state[0, r + 1, 2 * r + 1] == 0        # d2 = r r: the rim
    assert (state[0, r + 1, 2] == (255 * (2 * r - 1)) // (r * r)) if r > 1 else int(state.sum()) == 255   # one inside it: r r - (r - 1)^2 = 2 r - 1
    assert not state[0, 0].any() and not state[0, :, 0].any() and not state[0, -1].any() and not state[0, :, -1].any()


def test_the_twin_against_an_independent_loop(seeded):
    cases, answers = seeded
    assert len(cases) >= 40
    moved = 0
    for c, (canvases, state) in zip(cases, answers):
        want_canvases, want_state = HC.reference(c)
        assert np.array_equal(state, want_state) and np.array_equal(canvases, want_canvases), c.name
        moved += int((canvases != c.canvases).any(axis=-1).sum())
    assert moved > 10000                                      # the picture was blended, not only left alone
    for name, c in HC.named_cases().items():
        if "r = 255" not in name:                             # (the loop over 3 discs of 200 000 pixels: the program below covers it)
            got, want = HC.twin(c), HC.reference(c)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


# ---------------------------------------------------------------------------------------------- the shared header
def build_program(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "heat_main.cpp"),
                    str(CSRC / "heat_check.cpp"), "-o", str(out)], check=True)
    return out


def check_program(exe: Path, tmp_path, seeded) -> None:
    cases, answers = seeded
    named = list(HC.named_cases().values())
    cases, answers = list(cases) + named, list(answers) + [HC.twin(c) for c in named]
    refused = HC.make("refused", np.random.default_rng(1), 2, 5, 6, 2, [[(1, 1, 0)], [(2, 2, 2)]], 3)
    HC.write_cases(tmp_path / "cases.bin", cases + [refused])
    done = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True)
    assert done.returncode == 0 and done.stderr == b"", done.stderr.decode()
    got = HC.read_answers(done.stdout, cases + [refused])
    for c, g, (canvases, state) in zip(cases, got, answers):
        assert isinstance(g, tuple), (c.name, g)
        assert np.array_equal(g[0], canvases) and np.array_equal(g[1], state), c.name
    assert got[-1] == E.heat_check(2, 5, 6, 2, refused.points, refused.first, refused.valid, **refused.call) and "no plane of 2" in got[-1]


def test_the_shared_header_equals_the_twin_bit_for_bit(tmp_path, seeded):
    check_program(build_program(tmp_path / "heat_main"), tmp_path, seeded)


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path, seeded):
    exe = build_program(tmp_path / "heat_asan", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
    check_program(exe, tmp_path, seeded)


# ---------------------------------------------------------------------------------------------- the rule's corners
def test_one_call_of_16_frames_equals_four_calls_of_4():
    rng = np.random.default_rng(2)
    c = HC.make("16", rng, 16, 33, 50, 3, HC.random_points(rng, 16, 33, 50, 3, 6), 6, full=255 * 5)
    want_canvases, want_state = HC.twin(c)
    canvases, state = c.canvases.copy(), c.state.copy()
    for lo in range(0, 16, 4):
        k0, k1 = int(c.first[lo]), int(c.first[lo + 4])
        HM.accumulate_host(canvases[lo:lo + 4], state, c.points[k0:k1], c.first[lo:lo + 5] - k0, c.valid[lo:lo + 4], **c.call)
    assert np.array_equal(state, want_state) and np.array_equal(canvases, want_canvases)
    assert int(state.sum()) > 0 and not np.array_equal(canvases[15], c.canvases[15])


def test_the_level_below_at_and_far_above_full():
    """full = 1000, alpha 256, a grey 50 pixel: D = 999 -> level 254 (999 * 255 // 1000), a = 254; D = 1000 and D = 2^32 - 1 -> level
    255, a = 255.  The pixel is (50 (256 - a) + lut[level] a + 128) >> 8."""
    state = np.zeros((1, 1, 4), np.uint32)
    state[0, 0] = [999, 1000, 2 ** 32 - 1, 0]
    canvases = np.full((1, 1, 4, 3), 50, np.uint8)
    HM.accumulate_host(canvases, state, None, [0, 0], [1], r=1, full=1000, alpha=256, show_mask=1, lut=LUT)
    mix = lambda level, a: [(50 * (256 - a) + int(LUT[level, k]) * a + 128) >> 8 for k in range(3)]
    assert canvases[0, 0].tolist() == [mix(254, 254), mix(255, 255), mix(255, 255), [50, 50, 50]]
    assert state[0, 0].tolist() == [999, 1000, 2 ** 32 - 1, 0]


def test_the_sums_saturate():
    state = np.zeros((2, 5, 5), np.uint32)
    state[0, 2, 2], state[0, 2, 1], state[1, 2, 2] = 2 ** 32 - 100, 2 ** 32 - 192, 2 ** 32 - 1
    canvases, state = one_point(5, 5, 2, 2, 2, planes=2, state=state, full=HM.E.HEAT_MAX_FULL)
    assert state[0, 2, 2] == 2 ** 32 - 1                      # + 255 would wrap
    assert state[0, 2, 1] == 2 ** 32 - 1 and state[0, 2, 3] == 191 and state[0, 1, 2] == 191      # 2^32 - 192 + 191 just fits
    assert state[1, 2, 2] == 2 ** 32 - 1
    # shown: plane 0 + plane 1 saturates as well, so the pixel is at level 255 — not at the level of a wrapped sum
    a = (160 * 255) >> 8
    assert canvases[0, 2, 2].tolist() == [(50 * (256 - a) + int(LUT[255, k]) * a + 128) >> 8 for k in range(3)]


def test_alpha_0_leaves_the_pixels_and_updates_the_state_and_alpha_256():
    canvases, state = one_point(9, 9, 4, 4, 3, alpha=0)
    assert (canvases == 50).all() and state[0, 4, 4] == 255 and int(state.sum()) == int(HM.splat(3).sum())
    canvases, state = one_point(9, 9, 4, 4, 3, alpha=256)
    assert canvases[0, 4, 4].tolist() == [(50 * 1 + int(LUT[255, k]) * 255 + 128) >> 8 for k in range(3)]
    assert (canvases[0, 0] == 50).all()                       # level 0: weight 0


def test_a_frame_that_is_not_valid_is_untouched_and_adds_nothing():
    rng = np.random.default_rng(4)
    c = HC.make("valid", rng, 3, 12, 20, 1, [[(5, 5, 0)], [], [(6, 5, 0)]], 4, full=300, valid=[1, 0, 1])
    canvases, state = HC.twin(c)
    assert np.array_equal(canvases[1], c.canvases[1]) and not np.array_equal(canvases[0], c.canvases[0])
    alone = HC.make("valid", rng, 2, 12, 20, 1, [[(5, 5, 0)], [(6, 5, 0)]], 4, full=300)
    assert np.array_equal(HC.twin(alone)[1], state)


# ---------------------------------------------------------------------------------------------- the refusals
PTS = np.array([[5, 5, 0], [6, 6, 1]], np.int32)
OK = dict(n=2, oh=10, ow=12, planes=2, points=PTS, first=[0, 1, 2], valid=[1, 1], r=3, full=500, alpha=160, show_mask=3, lut=LUT)
REFUSALS = {
    "no frame": (dict(n=0, first=[0], valid=[], points=None), "n = 0, at least one frame is needed"),
    "oh": (dict(oh=4097), "oh = 4097 outside [1, 4096]"),
    "ow": (dict(ow=0), "ow = 0 outside [1, 4096]"),
    "no plane": (dict(planes=0), "planes = 0 outside [1, 4]"),
    "five planes": (dict(planes=5), "planes = 5 outside [1, 4]"),
    "r = 0": (dict(r=0), "r = 0 outside [1, 255]"),
    "r = 256": (dict(r=256), "r = 256 outside [1, 255]"),
    "full = 0": (dict(full=0), "full = 0 outside [1, 16777215]"),
    "full = 2^24": (dict(full=1 << 24), "full = 16777216 outside [1, 16777215]"),
    "alpha = -1": (dict(alpha=-1), "alpha = -1 outside [0, 256]"),
    "alpha = 257": (dict(alpha=257), "alpha = 257 outside [0, 256]"),
    "a bit at planes": (dict(show_mask=4), "show_mask = 4 names no plane or one at or above planes = 2"),
    "no bit": (dict(show_mask=0), "show_mask = 0 names no plane"),
    "no first": (dict(first=None), "is NULL"),
    "no valid": (dict(valid=None), "is NULL"),
    "no lut": (dict(lut=None), "is NULL"),
    "no points": (dict(points=None), "announces 2 points and the points are NULL"),
    "first from 1": (dict(first=[1, 1, 2]), "first[0] = 1, it must be 0"),
    "first decreases": (dict(first=[0, 2, 1]), "first[2] = 1 is below first[1] = 2"),
    "65 points": (dict(points=np.tile(PTS[:1], (65, 1)), first=[0, 65, 65]), "frame 0 has 65 points, at most 64 are taken"),
    "x beyond": (dict(points=[[32768, 5, 0], [6, 6, 1]]), "point 0 (frame 0) is (32768, 5) on plane 0"),
    "y beyond": (dict(points=[[5, 5, 0], [6, -32768, 1]]), "point 1 (frame 1) is (6, -32768) on plane 1"),
    "a plane that is not there": (dict(points=[[5, 5, 0], [6, 6, 2]]), "on plane 2: beyond +/-32767 or no plane of 2"),
    "a negative plane": (dict(points=[[5, 5, -1], [6, 6, 1]]), "on plane -1"),
    "points in a frame that is not valid": (dict(valid=[1, 0]), "frame 1 is not valid and carries 1 points"),
    "overlap": (dict(overlap=True), "the state overlaps the canvases"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_one_refusal_per_reason_in_the_check_and_in_the_twin(name):
    change, said = REFUSALS[name]
    a = dict(OK, **{k: v for k, v in change.items() if k != "overlap"})
    n, oh, ow, planes = a["n"], a["oh"], a["ow"], a["planes"]
    sized = 1 <= oh <= 4096 and 1 <= ow <= 4096
    shape = (oh, ow) if sized else (1, 1)
    # (the twin takes n, planes, oh and ow from its arrays: for the sizes the library refuses they are described, not allocated)
    canvases, state = np.zeros((n, *shape, 3), np.uint8), np.zeros((max(min(planes, 4), 1), *shape), np.uint32)
    if change.get("overlap"):                                 # canvases and maps out of one block: the maps begin at the canvases' last word
        block = np.zeros(n * oh * ow * 3 + planes * oh * ow * 4, np.uint8)
        canvases = block[:n * oh * ow * 3].reshape(n, oh, ow, 3)
        state = block[n * oh * ow * 3 - 4:][:planes * oh * ow * 4].view(np.uint32).reshape(planes, oh, ow)
    call = dict(r=a["r"], full=a["full"], alpha=a["alpha"], show_mask=a["show_mask"], lut=a["lut"])
    why = E.heat_check(n, oh, ow, planes, a["points"], a["first"], a["valid"], **call, canvas=canvases.ctypes.data or 1, state=state.ctypes.data)
    assert why is not None and why.startswith("pa_heat_accumulate: ") and said in why, why
    if sized and 1 <= planes <= 4:                            # what the twin's own arrays can state
        with pytest.raises(ValueError) as twin_said:
            HM.accumulate_host(canvases, state, a["points"], a["first"], a["valid"], **call)
        assert str(twin_said.value) == why                    # the same words


def test_null_canvases_and_states_are_refused_and_touching_buffers_accepted():
    args = (2, 10, 12, 2, PTS, [0, 1, 2], [1, 1], 3, 500, 160, 3, LUT)
    for kw in (dict(canvas=None), dict(state=None)):
        why = E.heat_check(*args, **kw)
        assert why is not None and "is NULL" in why
    canvas_bytes, state_bytes = 2 * 10 * 12 * 3, 2 * 10 * 12 * 4
    assert E.heat_check(*args, canvas=4096, state=4096 + canvas_bytes) is None          # the maps begin where the canvases end
    assert E.heat_check(*args, canvas=4096, state=4096 + canvas_bytes - 1) is not None
    assert E.heat_check(*args, canvas=4096 + state_bytes, state=4096) is None
    assert E.heat_check(1, 4096, 4096, 4, None, [0, 0], [1], 255, E.HEAT_MAX_FULL, 256, 15, LUT) is None
    assert E.heat_check(1, 10, 12, 2, None, [0, 0], [0], 3, 500, 160, 3, LUT) is None    # a frame that is not valid, without points


def test_the_symbols_are_part_of_the_abi():
    assert {"pa_heat_accumulate", "pa_heat_check", "pa_heat_last_path"} <= set(E.ABI_SYMBOLS)
    assert (E.HEAT_MAX_POINTS, E.HEAT_MAX_PLANES, E.HEAT_MAX_RADIUS, E.HEAT_MAX_COORD, E.HEAT_MAX_FULL) == (64, 4, 255, 32767, 2 ** 24 - 1)
    header = (ROOT / "include" / "padel_hip.h").read_text()
    for name, value in (("POINTS", 64), ("PLANES", 4), ("RADIUS", 255), ("COORD", 32767), ("FULL", 16777215)):
        assert f"#define PA_HEAT_MAX_{name} {value}\n" in header


# ---------------------------------------------------------------------------------------------- the ramp
def test_the_ramp_hits_its_anchors_and_is_linear_between_them():
    assert LUT.shape == (256, 3) and LUT.dtype == np.uint8
    for level, bgr in HM.LUT_ANCHORS:
        assert tuple(LUT[level]) == bgr
    assert tuple(LUT[0]) == (128, 0, 0) and tuple(LUT[255]) == (0, 0, 255)
    # monotone per channel between two anchors; the steepest piece is 255 over 63 levels = 4.05 a level: a floored step is 4 or 5
    for (l0, _), (l1, _) in zip(HM.LUT_ANCHORS, HM.LUT_ANCHORS[1:]):
        d = np.diff(LUT[l0:l1 + 1].astype(int), axis=0)
        assert ((d >= 0).all(axis=0) | (d <= 0).all(axis=0)).all() and np.abs(d).max() <= 5
    assert tuple(LUT[32]) == (128 + (127 * 32) // 64, (255 * 32) // 64, 0)
    two = HM.heat_lut(((0, (0, 0, 0)), (255, (255, 255, 255))))
    assert np.array_equal(two[:, 0], np.arange(256)) and np.array_equal(two[:, 0], two[:, 2])
    for bad in (((1, (0, 0, 0)), (255, (1, 1, 1))), ((0, (0, 0, 0)), (254, (1, 1, 1))), ((0, (0, 0, 0)), (0, (1, 1, 1)), (255, (2, 2, 2))),
                ((0, (0, 0, 256)), (255, (1, 1, 1)))):
        with pytest.raises(ValueError, match="heat_lut"):
            HM.heat_lut(bad)


# ---------------------------------------------------------------------------------------------- HeatMap
def view_and_camera():
    court = court_for(1280, 720)
    view = T.TopDownView(court)
    S_ = np.array([[0.4, 0, 10.3], [0, 1.2, -20.6], [0, 0, 1.0]])             # A H is (x, y) -> (0.4 x + 10.3, 1.2 y - 20.6)
    return view, np.linalg.inv(view.A) @ S_


def test_the_parameters_in_canvas_units():
    view, _ = view_and_camera()
    heat = HM.HeatMap(view, fps=30)
    assert (heat.r, heat.full, heat.alpha, heat.planes, heat.show_mask, heat.ids) == (24, 255 * 600, 160, 4, 15, (1, 2, 3, 4))
    assert heat.state().shape == (4, 1104, 624) and heat.state().dtype == np.uint32 and not heat.state().any()
    heat = HM.HeatMap(view, radius_m=0.26, saturate_s=1.5, fps=25, alpha=0, ids=(7, 3), show=(3,))
    assert (heat.r, heat.full, heat.alpha, heat.planes, heat.show_mask) == (12, 255 * 38, 0, 2, 2)        # 12.48 -> 12, 37.5 -> 38
    assert heat.call() == dict(r=12, full=255 * 38, alpha=0, show_mask=2, lut=heat.lut) and heat.call(overlay=False)["alpha"] == 0
    assert HM.HeatMap(view, fps=30).call(overlay=False)["alpha"] == 0 and np.array_equal(heat.lut, LUT)
    for bad, said in ((dict(radius_m=0), "radius"), (dict(radius_m=6), "radius"), (dict(saturate_s=0), "full"), (dict(saturate_s=3000), "full"),
                      (dict(alpha=257), "alpha"), (dict(alpha=1.5), "alpha"), (dict(ids=()), "ids"), (dict(ids=(1, 2, 3, 4, 5)), "ids"),
                      (dict(ids=(1, 1)), "ids"), (dict(show=(9,)), "show"), (dict(show=()), "show")):
        with pytest.raises(ValueError, match=said):
            HM.HeatMap(view, fps=30, **bad)


def test_points_are_the_feet_where_to_canvas_puts_them():
    """Player 3's box (100, 200) .. (160, 400) has its feet at (130, 400) -> (62.3, 459.4) -> (62, 459); player 1's (600, 100) ..
    (700, 300) at (650, 300) -> (270.3, 339.4): the centres of the discs the top-down clip draws (test_topdown_host.py).  Player 9 has no
    plane; player 2's feet at (-100, 300) -> (-29.7, 339.4) lie 30 pixels left of the canvas: with r = 24 the bump misses it."""
    view, H = view_and_camera()
    heat = HM.HeatMap(view, fps=30)
    rows = np.array([[100, 200, 160, 400, 0.9, 0], [600, 100, 700, 300, 0.8, 0], [10, 10, 20, 20, 0.8, 0], [-130, 100, -70, 300, 0.8, 0]], np.float32)
    players = Players(rows=rows, ids=np.array([3, 1, 9, 2]))
    fp = PC.FrameProjection(H, None, None)
    assert heat.points(fp, players) == [(62, 459, 2), (270, 339, 0)]
    M = view.canvas_from_frame(H)
    assert [p[:2] for p in heat.points(fp, players)] == [view.to_canvas(p.feet, M) for p in list(players)[:2]]
    assert HM.HeatMap(view, radius_m=0.7, fps=30).points(fp, players)[-1] == (-30, 339, 1)      # r = 34 reaches the canvas
    assert heat.points(PC.FrameProjection(None, None, None), players) == [] and heat.points(fp, None) == []
    assert heat.points(PC.FrameProjection(np.zeros((3, 3)), None, None), players) == []         # no inverse: not valid for the warp either
    pts, first, valid = heat.batch([fp, PC.FrameProjection(None, None, None), fp], [players, players, None])
    assert pts.tolist() == [[62, 459, 2], [270, 339, 0]] and first.tolist() == [0, 2, 2, 2] and valid.tolist() == [1, 0, 1]
    assert pts.dtype == np.int32 and E.heat_check(3, view.h, view.w, 4, pts, first, valid, **heat.call()) is None


def test_the_first_64_points_are_kept_with_one_warning():
    view, H = view_and_camera()
    heat = HM.HeatMap(view, fps=30, ids=(1,))
    rows = np.tile(np.array([[100, 200, 160, 400, 0.9, 0]], np.float32), (70, 1))
    rows[:, 0] += np.arange(70)
    crowd = Players(rows=rows, ids=np.ones(70, int))
    fp = PC.FrameProjection(H, None, None)
    with pytest.warns(UserWarning, match="70 players' feet, the first 64"):
        got = heat.points(fp, crowd)
    assert len(got) == 64 and got[0] == (62, 459, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert len(heat.points(fp, crowd)) == 64              # said once


# ---------------------------------------------------------------------------------------------- the runner, before anything runs
SRC_720P = "synthetic://?n=3&h=720&w=1280&fps=25&seed=1"


def make_runner(tmp_path, trackers=None, **kw):
    return TrackingRunner(stub_trackers([], [], []) if trackers is None else trackers, SRC_720P, tmp_path / "out.mp4", engine=StandInEngine(), **kw)


def test_what_the_runner_refuses_before_any_tracker_runs(tmp_path):
    players, ball, keypoints = stub_trackers([], [], [])
    with pytest.raises(ValueError, match="no tracker gives Keypoints"):
        make_runner(tmp_path, trackers=[players, ball], heatmap=tmp_path / "h.npy")
    with pytest.raises(ValueError, match="no tracker gives Players"):
        make_runner(tmp_path, trackers=[ball, keypoints], heatmap=tmp_path / "h.npy")
    with pytest.raises(ValueError, match="fanout"):
        make_runner(tmp_path, heatmap=tmp_path / "h.npy", fanout=True)
    for bad in ("h.png", "h", "h.jpeg", "h.y4m"):
        with pytest.raises(ValueError, match=r"must end in \.npy"):
            make_runner(tmp_path, heatmap=tmp_path / bad)
    with pytest.raises(ValueError, match="heatmap_options: unknown colour"):
        make_runner(tmp_path, heatmap=tmp_path / "h.npy", heatmap_options=dict(colour=1))
    with pytest.raises(ValueError, match="radius"):
        make_runner(tmp_path, heatmap=tmp_path / "h.npy", heatmap_options=dict(radius_m=9))
    with pytest.raises(ValueError, match=r"3000 x 4000 canvas cannot be written to .*h\.jpg.*2560"):
        make_runner(tmp_path, heatmap=tmp_path / "h.jpg", topdown_options=dict(px_per_m=100, margin_m=10))
    with pytest.raises(TypeError):                            # an unknown key in topdown_options stays what it was
        make_runner(tmp_path, heatmap=tmp_path / "h.npy", topdown_options=dict(pixels=3))
    runner = make_runner(tmp_path, heatmap=tmp_path / "H.NPY", heatmap_options=dict(radius_m=0.25, overlay=False), topdown_options=dict(px_per_m=20, margin_m=1))
    assert runner.heat.view.size == (240, 440) and runner.heat.r == 5 and runner.heat.full == 255 * 500 and runner.topdown_view is None
    runner = make_runner(tmp_path, heatmap=tmp_path / "h.jpg", topdown=tmp_path / "t.y4m")
    assert runner.heat.view is runner.topdown_view
    assert make_runner(tmp_path).heatmap is None and make_runner(tmp_path).heat is None and make_runner(tmp_path).heat_state is None
    assert sorted(p.name for p in tmp_path.iterdir()) == []   # nothing is created in __init__


# ---------------------------------------------------------------------------------------------- the runner over a recording engine
N, H, W = 5, 96, 160
SRC = f"synthetic://?n={N}&h={H}&w={W}&fps=30&seed=4"
OPTIONS = dict(px_per_m=6, margin_m=4, fill=(9, 8, 7))        # a 108 x 168 canvas: the four scripted players' feet all fall into it
CW, CH = 108, 168
HEAT = dict(radius_m=2.5, saturate_s=0.1)                     # r = 15 pixels — wider than the discs the clip draws at the feet —, full = 255 * 3


def scripted_trackers():
    balls = [Ball(i, (40.0 + 17 * i, 50.0 + 6 * i), 1) for i in range(N)]
    return [Stored("players_tracker", Players, S.players_script(range(N))), Stored("ball_tracker", Ball, balls), S.keypoints_tracker(N, H, W)]


def run(tmp_path, monkeypatch, batch=2, eng=None, trackers=None, **kw):
    eng = TwinEngine() if eng is None else eng
    walks = []
    real = video.get_video_frames_generator

    def recording(source, stride=1, start=0, end=None):
        walks.append((start, end))
        return real(source, stride=stride, start=start, end=end)
    monkeypatch.setattr(video, "get_video_frames_generator", recording)
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", batch)
    runner = TrackingRunner(scripted_trackers() if trackers is None else trackers, SRC, tmp_path / "out.mp4", engine=eng, **kw)
    runner.run()
    return runner, eng, walks


def expected_maps(runner, overlay_frames=None):
    """The maps — and, given the clip's frames, the canvases under them — frame by frame from the runner's projections and results."""
    heat = runner.heat
    state = heat.state()
    canvases = []
    for i in range(N):
        pts, first, valid = heat.batch(runner._projected[i:i + 1], [runner.trackers["players_tracker"].results[i]])
        canvas = None
        if overlay_frames is not None:
            m, v = heat.view.matrices(runner._projected[i:i + 1])
            canvas = T.warp_host(overlay_frames[i:i + 1], m, v, heat.view.h, heat.view.w, heat.view.fill)
        HM.accumulate_host(canvas, state, pts, first, valid, **heat.call(overlay_frames is not None))
        canvases.append(canvas)
    return state, canvases


def test_one_walk_with_heat_between_warp_and_render(tmp_path, monkeypatch, capsys):
    runner, eng, walks = run(tmp_path, monkeypatch, topdown=tmp_path / "t.y4m", topdown_options=OPTIONS, heatmap=tmp_path / "h.npy", heatmap_options=HEAT)
    assert walks == [(0, None)]                               # the clip was read once
    assert [c[0] for c in eng.calls] == ["warp", "heat", "render"] * 3
    assert [c[1] for c in eng.calls if c[0] == "heat"] == [(n, CH, CW, 4) for n in (2, 2, 1)]
    call = eng.calls[1][2]
    assert (call["r"], call["full"], call["alpha"], call["show_mask"]) == (15, 255 * 3, 160, 15) and len(call["points"]) == 8
    frames = np.stack(list(video.get_video_frames_generator(SRC)))
    state, canvases = expected_maps(runner, frames)
    assert state.any() and all(state[p].any() for p in range(4))                     # the four players each left a map
    assert np.array_equal(runner.heat_state, state) and np.array_equal(np.load(tmp_path / "h.npy"), state)
    assert np.load(tmp_path / "h.npy").dtype == np.uint32 and np.load(tmp_path / "h.npy").shape == (4, CH, CW)
    # the clip shows the map growing: every frame is the warped picture under the maps as they stood, then the marks
    top = video.YuvClip.from_y4m(tmp_path / "t.y4m", on_device=False)
    geom, enc = video.yuv_desc(CW, CH, "i420"), video.YUV_ENC_COEFFS["bt601_limited"]
    plain = T.warp_host(frames[4:5], *runner.topdown_view.matrices(runner._projected[4:5]), CH, CW, (9, 8, 7))
    assert not np.array_equal(canvases[4], plain)
    for i in range(N):
        want = R.render_host(canvases[i], *R.pack([runner.topdown_marks(i)]), out=E.RENDER_YUV420, geom=geom, enc=enc)
        assert np.array_equal(top._host_bytes(i, 1), want), i
    t = runner.timings["__heatmap__"]
    assert t["frames"] == N and t["seconds"] > 0 and runner.timings["__topdown__"]["frames"] == N
    assert "runner: heat maps of 5 frames (4 of 108 x 168)" in capsys.readouterr().out


def test_overlay_false_accumulates_with_alpha_0(tmp_path, monkeypatch):
    runner, eng, _ = run(tmp_path, monkeypatch, topdown=tmp_path / "t.y4m", topdown_options=OPTIONS, heatmap=tmp_path / "h.npy",
                         heatmap_options=dict(HEAT, overlay=False))
    assert [c[2]["alpha"] for c in eng.calls if c[0] == "heat"] == [0, 0, 0]
    shown = tmp_path / "shown"
    shown.mkdir()
    with_it, _, _ = run(shown, monkeypatch, topdown=shown / "t.y4m", topdown_options=OPTIONS, heatmap=shown / "h.npy", heatmap_options=HEAT)
    plain = tmp_path / "plain"
    plain.mkdir()
    run(plain, monkeypatch, topdown=plain / "t.y4m", topdown_options=OPTIONS)
    assert np.array_equal(runner.heat_state, with_it.heat_state) and runner.heat_state.any()
    assert (tmp_path / "t.y4m").read_bytes() == (plain / "t.y4m").read_bytes() != (shown / "t.y4m").read_bytes()


def test_nothing_new_without_the_argument(tmp_path, monkeypatch, capsys):
    runner, eng, _ = run(tmp_path, monkeypatch, render=tmp_path / "r.y4m", topdown=tmp_path / "t.y4m", topdown_options=OPTIONS)
    # today's calls with today's arguments: no heat, and no keyword the engines of the other tests do not know
    assert [c[0] for c in eng.calls] == ["render", "warp", "render"] * 3
    assert all(set(c[2]) == {"out", "geom", "enc"} for c in eng.calls if c[0] == "render") and all(set(c[2]) == {"fill"} for c in eng.calls if c[0] == "warp")
    assert "__heatmap__" not in runner.timings and runner.heat_state is None and "heat map" not in capsys.readouterr().out
    assert sorted(p.name for p in tmp_path.iterdir()) == ["r.y4m", "t.y4m"]


def test_heatmap_alone_needs_no_engine_and_reads_no_frame(tmp_path, monkeypatch):
    runner, _, walks = run(tmp_path, monkeypatch, eng=StandInEngine(), heatmap=tmp_path / "h.npy", heatmap_options=HEAT, topdown_options=OPTIONS)
    assert walks == []                                        # the stored results alone
    state, _ = expected_maps(runner)
    assert state.any() and np.array_equal(runner.heat_state, state) and np.array_equal(np.load(tmp_path / "h.npy"), state)
    assert runner.timings["__heatmap__"]["frames"] == N and "__topdown__" not in runner.timings and "__render__" not in runner.timings
    # the same maps as the run that showed them, and as a run beside render= alone (which walks the clip for render's sake)
    both = tmp_path / "both"
    both.mkdir()
    beside, eng, walks = run(both, monkeypatch, render=both / "r.y4m", heatmap=both / "h.npy", heatmap_options=HEAT, topdown_options=OPTIONS)
    assert walks == [(0, None)] and [c[0] for c in eng.calls] == ["render"] * 3 and np.array_equal(beside.heat_state, state)
    # a second draw_and_collect_data starts over: the maps are not added twice
    runner.draw_and_collect_data()
    assert np.array_equal(runner.heat_state, state)


def test_the_picture(tmp_path, monkeypatch):
    """``.jpg``: a fill canvas under the final maps at full = their largest density, the court's lines over it — the same bytes from
    the stand-in engine's renderer and encoder as from the host path."""
    runner, eng, _ = run(tmp_path, monkeypatch, topdown=tmp_path / "t.y4m", topdown_options=OPTIONS, heatmap=tmp_path / "h.jpg", heatmap_options=HEAT)
    assert [c[0] for c in eng.calls][-3:] == ["heat", "render", "jpeg_encode"] and eng.calls[-3][1] == (1, CH, CW, 4)
    heat = runner.heat
    peak = int(HM.shown_density(runner.heat_state, 15).max())
    assert eng.calls[-3][2]["full"] == peak == heat.picture_full(runner.heat_state) and eng.calls[-3][2]["points"] == [] and eng.calls[-3][2]["alpha"] == 160
    alone = tmp_path / "alone"
    alone.mkdir()
    run(alone, monkeypatch, eng=StandInEngine(), heatmap=alone / "h.jpg", heatmap_options=HEAT, topdown_options=OPTIONS)
    data = (tmp_path / "h.jpg").read_bytes()
    assert data == (alone / "h.jpg").read_bytes() and data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    picture, status = mjpeg.decode_frame(np.frombuffer(data, np.uint8))
    assert picture.shape == (CH, CW, 3) and status == 0
    blank = np.empty((1, CH, CW, 3), np.uint8)
    blank[:] = (9, 8, 7)
    HM.accumulate_host(blank, runner.heat_state.copy(), None, [0, 0], [1], **dict(heat.call(), full=peak))
    at = np.unravel_index(np.argmax(HM.shown_density(runner.heat_state, 15)), (CH, CW))
    a = (160 * 255) >> 8
    assert blank[0][at].tolist() == [([9, 8, 7][k] * (256 - a) + int(LUT[255, k]) * a + 128) >> 8 for k in range(3)]      # the peak is at the ramp's top
    assert heat.picture_full(heat.state()) == 1 and heat.picture_full(np.full((4, 2, 2), 2 ** 31, np.uint32)) == E.HEAT_MAX_FULL


def test_segments_and_identities_come_first(tmp_path, monkeypatch):
    kept = [(1, 2), (3, 5)]
    tr = scripted_trackers()
    for t in tr:
        t.results.predictions = [t.results.predictions[i] for lo, hi in kept for i in range(lo, hi)]
    runner = TrackingRunner(tr, SRC, tmp_path / "out.mp4", engine=StandInEngine(), heatmap=tmp_path / "h.npy", heatmap_options=HEAT,
                            topdown_options=OPTIONS, segments=kept)
    runner.run()
    state = runner.heat.state()
    for i in range(3):
        HM.accumulate_host(None, state, *runner.heat.batch(runner._projected[i:i + 1], [tr[0].results[i]]), **runner.heat.call(False))
    assert np.array_equal(runner.heat_state, state) and state.any() and runner.timings["__heatmap__"]["frames"] == 3
    # ids outside `ids` leave no map: the planes are the ids as the results carry them when the step runs (after identities=True)
    only = TrackingRunner(scripted_trackers(), SRC, tmp_path / "out.mp4", engine=StandInEngine(), heatmap=tmp_path / "two.npy",
                          heatmap_options=dict(HEAT, ids=(2, 4)), topdown_options=OPTIONS)
    only.run()
    assert only.heat_state.shape == (2, CH, CW) and only.heat_state[0].any() and only.heat_state[1].any()
