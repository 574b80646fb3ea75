"""Player identities without a GPU: the numpy twin of the box histograms (``identity.box_histograms_host``) against a per-pixel
statement of include/padel_hip.h; ``torso_rect`` known answers; ``assign`` on scripted tracks; the refusals of
``pa_box_histograms_check`` through ctypes, through ``Engine.box_histograms``'s wrapper and through the stand-alone program
tests/box_histogram_check_main.cpp (plain, and under -fsanitize=address,undefined: a plain executable, nothing is preloaded); and
``TrackingRunner(identities=True)`` over a stub tracker with ``on_device=False`` (tests/identity_script.py)."""
import json
import random
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E, identity as I, video
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.players_tracker import Player, Players
from tests import identity_script as S

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"


# ------------------------------------------------------------------------------------------------ the twin
def per_pixel(frames, rects):
    """The specification once more, one pixel at a time in Python integers."""
    out = np.zeros((len(rects), 512), np.uint32)
    for j, (fi, x0, y0, x1, y1) in enumerate(rects):
        for y in range(y0, y1):
            for x in range(x0, x1):
                b, g, r = (int(v) for v in frames[fi, y, x])
                out[j, ((b >> 5) << 6) | ((g >> 5) << 3) | (r >> 5)] += 1
    return out


def test_twin_equals_the_per_pixel_statement():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    rects = [(0, 0, 0, 7, 5), (2, 1, 1, 4, 3), (1, 6, 4, 7, 5), (2, 0, 2, 7, 3), (1, 3, 0, 4, 5), (0, 0, 0, 7, 5)]
    got = I.box_histograms_host(frames, rects)
    assert got.dtype == np.uint32 and got.shape == (6, 512) and np.array_equal(got, per_pixel(frames, rects))
    assert got.sum(1).tolist() == [35, 6, 1, 7, 5, 35] and np.array_equal(got[0], got[5])
    assert I.box_histograms_host(frames, []).shape == (0, 512)


def test_bins_known_answers():
    f = np.zeros((1, 1, 4, 3), np.uint8)
    f[0, 0] = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (31, 32, 224)]
    got = I.box_histograms_host(f, [(0, x, 0, x + 1, 1) for x in range(4)])
    assert [int(np.flatnonzero(r)[0]) for r in got] == [7 << 6, 7 << 3, 7, (0 << 6) | (1 << 3) | 7]


def test_twin_refuses_what_the_library_refuses():
    f = np.zeros((2, 4, 6, 3), np.uint8)
    for rect, word in (((2, 0, 0, 1, 1), "names frame 2"), ((-1, 0, 0, 1, 1), "names frame -1"), ((0, 0, 0, 7, 4), "is empty or leaves"),
                       ((0, 2, 1, 2, 3), "is empty or leaves"), ((0, 0, -1, 3, 3), "is empty or leaves")):
        with pytest.raises(ValueError, match=word):
            I.box_histograms_host(f, [rect])


# ------------------------------------------------------------------------------------------------ torso_rect
@pytest.mark.parametrize("xyxy,want", [
    ((10, 10, 50, 90), (20, 20, 40, 60)),                  # bw 40, bh 80: a quarter off each side, 1/8 .. 5/8 of the height
    ((10.25, 10.5, 49.75, 89.5), (20, 20, 40, 60)),        # floor / ceil give the same integer box
    ((10, 20, 17, 29), (11, 21, 16, 25)),                  # bw 7 -> 7 // 4 = 1; bh 9 -> 9 // 8 = 1, 45 // 8 = 5
    ((0, 0, 160, 96), (40, 12, 120, 60)),                  # touches every edge
    ((-20, -8, 20, 56), (5, 7, 15, 35)),                   # leaves at the top left: clipped to (0, 0, 20, 56) first
    ((140, 60, 200, 130), (145, 64, 155, 82)),             # leaves at the bottom right: clipped to (140, 60, 160, 96)
    ((3, 3, 4, 11), (3, 4, 4, 8)),                         # one pixel wide
    ((3, 3, 11, 4), None),                                 # one pixel high: (5 * 1) // 8 = 0 rows
    ((200, 10, 240, 50), None),                            # outside the frame
    ((-40, -40, 0, 0), None),
    ((50, 50, 50, 90), None),                              # no width
    ((60, 50, 50, 90), None),                              # inverted
    ((float("nan"), 0, 10, 10), None),
])
def test_torso_rect_known_answers(xyxy, want):
    assert I.torso_rect(xyxy, 96, 160) == want
    assert I.torso_rect(np.array(xyxy, np.float32), 96, 160) == want


# ------------------------------------------------------------------------------------------------ assign
def hist(*bins):
    h = np.zeros(512, np.uint64)
    for b, c in bins:
        h[b] = c
    return h


def track(lo, hi, h, boxes=None):
    return I.Track(frames=list(range(lo, hi)), hist=h.copy(), boxes=hi - lo if boxes is None else boxes)


SHIRT = {p: hist((10 * p, 100)) for p in (1, 2, 3, 4)}


def test_no_loss_gives_the_identity_map():
    tracks = {p: track(0, 50, SHIRT[p]) for p in (1, 2, 3, 4)}
    mapping, dist = I.assign(tracks)
    assert mapping == {1: 1, 2: 2, 3: 3, 4: 4} and dist == {}


def test_the_seed_numbers_by_ascending_bytetrack_id():
    tracks = {9: track(0, 50, SHIRT[1]), 3: track(0, 50, SHIRT[2]), 12: track(0, 50, SHIRT[3]), 7: track(0, 50, SHIRT[4])}
    assert I.assign(tracks)[0] == {3: 1, 7: 2, 9: 3, 12: 4}


def test_a_player_lost_and_reborn_gets_the_old_number():
    tracks = {1: track(0, 50, SHIRT[1]), 2: track(0, 20, SHIRT[2]), 3: track(0, 50, SHIRT[3]), 4: track(0, 50, SHIRT[4]),
              5: track(30, 50, SHIRT[2])}
    mapping, dist = I.assign(tracks)
    assert mapping == {1: 1, 2: 2, 3: 3, 4: 4, 5: 2}
    assert dist == {5: {2: 0.0}}                           # the only identity that is free in frames 30 .. 49


def test_two_players_reborn_in_the_same_frame_with_crossed_ids():
    tracks = {1: track(0, 50, SHIRT[1]), 2: track(0, 50, SHIRT[2]), 3: track(0, 20, SHIRT[3]), 4: track(0, 20, SHIRT[4]),
              6: track(30, 50, SHIRT[4]), 7: track(30, 50, SHIRT[3])}
    mapping, dist = I.assign(tracks)
    assert mapping == {1: 1, 2: 2, 3: 3, 4: 4, 6: 4, 7: 3}
    assert dist == {6: {3: 1.0, 4: 0.0}, 7: {3: 0.0}}       # 6 first (same first frame, lower id); 4 is then taken for 7


def test_a_fifth_person_stays_5():
    tracks = {p: track(0, 50, SHIRT[p]) for p in (1, 2, 3, 4)}
    tracks[5] = track(10, 30, SHIRT[2])                    # looks like player 2, but player 2 is on court at the same time
    mapping, dist = I.assign(tracks)
    assert mapping == {1: 1, 2: 2, 3: 3, 4: 4, 5: 5} and dist == {5: {}}


def test_a_reborn_track_too_far_from_the_free_identity_stays_unassigned():
    far = hist((20, 40), (300, 60))                        # shares 40 % with shirt 2: distance 0.6
    tracks = {1: track(0, 50, SHIRT[1]), 2: track(0, 20, SHIRT[2]), 3: track(0, 50, SHIRT[3]), 4: track(0, 50, SHIRT[4]),
              8: track(30, 40, far), 9: track(42, 50, SHIRT[2])}
    mapping, dist = I.assign(tracks)
    assert dist[8] == {2: pytest.approx(0.6, abs=1e-12)}
    assert mapping == {1: 1, 2: 2, 3: 3, 4: 4, 8: 5, 9: 2}  # 8 took nothing: identity 2 is still free for 9
    assert I.assign(tracks, max_distance=0.6 + 1e-9)[0][8] == 2
    near = hist((20, 50), (300, 50))                       # distance exactly 0.5: "at most" includes it
    tracks[8] = track(30, 40, near)
    assert I.assign(tracks)[0][8] == 2 and I.assign(tracks, max_distance=0.49)[0][8] == 5


def test_unassigned_tracks_count_on_from_n_players():
    tracks = {p: track(0, 50, SHIRT[p]) for p in (1, 2, 3, 4)}
    tracks[20] = track(12, 20, SHIRT[1])
    tracks[11] = track(12, 20, SHIRT[1])
    tracks[15] = track(5, 8, SHIRT[1])
    assert I.assign(tracks)[0] == {1: 1, 2: 2, 3: 3, 4: 4, 15: 5, 11: 6, 20: 7}      # by first frame, ties by id


def test_a_track_without_pixels_matches_nobody():
    tracks = {1: track(0, 50, SHIRT[1]), 2: track(0, 20, SHIRT[2]), 3: track(0, 50, SHIRT[3]), 4: track(0, 50, SHIRT[4]),
              5: track(30, 50, hist(), boxes=0)}
    mapping, dist = I.assign(tracks)
    assert mapping[5] == 5 and dist[5] == {2: 1.0}
    assert I.distance(hist(), hist()) == 1.0 and I.distance(SHIRT[1], SHIRT[1] * 3) == 0.0 and I.distance(SHIRT[1], SHIRT[2]) == 1.0


def test_the_seed_is_the_earliest_frame_with_exactly_n_players():
    # frames 0 .. 4 show three players, 5 .. 9 five: the seed is frame 10; the early track 6 is taken afterwards
    tracks = {1: track(0, 50, SHIRT[1]), 2: track(0, 50, SHIRT[2]), 3: track(0, 50, SHIRT[3]), 4: track(5, 50, SHIRT[4]),
              6: track(5, 10, SHIRT[4])}
    mapping, _ = I.assign(tracks)
    assert mapping == {1: 1, 2: 2, 3: 3, 4: 4, 6: 5}


def test_no_seed_frame_warns_and_changes_nothing():
    tracks = {p: track(0, 50, SHIRT[p]) for p in (1, 2, 3)}
    tracks[9] = track(60, 70, SHIRT[1])
    with pytest.warns(UserWarning, match="no frame shows exactly 4"):
        mapping, dist = I.assign(tracks)
    assert mapping == {1: 1, 2: 2, 3: 3, 9: 9} and dist == {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert I.assign(tracks, n_players=3)[0] == {1: 1, 2: 2, 3: 3, 9: 1}


def test_the_result_does_not_depend_on_the_order_of_the_dict():
    tracks = {1: track(0, 50, SHIRT[1]), 2: track(0, 20, SHIRT[2]), 3: track(0, 25, SHIRT[3]), 4: track(0, 25, SHIRT[4]),
              5: track(30, 50, SHIRT[2]), 6: track(30, 50, SHIRT[4]), 7: track(30, 50, SHIRT[3]), 8: track(35, 40, SHIRT[1])}
    want = I.assign(tracks)
    assert want[0] == {1: 1, 2: 2, 3: 3, 4: 4, 5: 2, 6: 4, 7: 3, 8: 5}
    keys = list(tracks)
    for seed in range(5):
        random.Random(seed).shuffle(keys)
        got = I.assign({k: tracks[k] for k in keys})
        assert got == want
    assert all(np.array_equal(tracks[p].hist, SHIRT[p]) for p in (1, 2, 3, 4))        # the input is not written to


# ------------------------------------------------------------------------------------------------ the refusals
RECT = [(0, 0, 0, 6, 4)]
REFUSALS = [
    ("no frames", dict(n=0, h=4, w=6, rects=RECT), "n = 0 frames outside [1, 65535]"),
    ("too many frames", dict(n=65536, h=4, w=6, rects=RECT), "n = 65536 frames outside"),
    ("no width", dict(n=1, h=4, w=0, rects=RECT), "width and height must lie in [1, 16384]"),
    ("too tall", dict(n=1, h=16385, w=6, rects=RECT), "width and height must lie in [1, 16384]"),
    ("too many rectangles", dict(n=1, h=4, w=6, rects=RECT * 16385), "k = 16385 rectangles outside [0, 16384]"),
    ("frame beyond the batch", dict(n=2, h=4, w=6, rects=RECT + [(2, 0, 0, 6, 4)]), "rectangle 1 names frame 2, outside [0, 2)"),
    ("negative frame", dict(n=2, h=4, w=6, rects=[(-1, 0, 0, 6, 4)]), "rectangle 0 names frame -1"),
    ("rectangle beyond the frame", dict(n=1, h=4, w=6, rects=[(0, 0, 0, 7, 4)]), "rectangle 0 (0, 0, 7, 4) is empty or leaves the 6 x 4 frame"),
    ("empty rectangle", dict(n=1, h=4, w=6, rects=RECT + [(0, 2, 1, 2, 3)]), "rectangle 1 (2, 1, 2, 3) is empty or leaves"),
    ("negative rectangle", dict(n=1, h=4, w=6, rects=[(0, -1, 0, 3, 3)]), "rectangle 0 (-1, 0, 3, 3) is empty or leaves"),
    ("a NULL list", dict(n=1, h=4, w=6, rects=None), "frames, rects or out is NULL"),
]


@pytest.mark.parametrize("case,kw,words", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case, kw, words):
    why = E.box_histograms_check(**kw)
    assert why is not None and why.startswith("pa_box_histograms: ") and words in why


class _NoEngine(E.Engine):
    """``Engine.box_histograms`` up to the library call: what it refuses it refuses before it touches an engine."""
    def __init__(self):
        self.lib, self.handle = E.load_library(), None


@pytest.mark.parametrize("case,kw,words", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_the_wrapper_refuses_with_the_same_reason(case, kw, words):
    with pytest.raises(E.EngineError) as ex:
        _NoEngine().box_histograms(E.DeviceBuffer(None, 1 << 20, _ptr=1), kw["n"], kw["h"], kw["w"], kw["rects"])
    assert str(ex.value) == E.box_histograms_check(**kw)


def test_the_wrapper_checks_its_buffers():
    eng = _NoEngine()
    with pytest.raises(E.EngineError, match="src holds 71 bytes, 1 BGR frames need 72"):
        eng.box_histograms(E.DeviceBuffer(None, 71, _ptr=1), 1, 4, 6, RECT)
    for out in (np.zeros((1, 512), np.uint64), np.zeros((1, 511), np.uint32), np.zeros((0, 512), np.uint32), np.zeros((2, 1024), np.uint32)[:, ::2]):
        with pytest.raises(E.EngineError, match="out must be"):
            eng.box_histograms(E.DeviceBuffer(None, 72, _ptr=1), 1, 4, 6, RECT, out=out)
    with pytest.raises(ValueError, match=r"\(k, 5\)"):
        eng.box_histograms(E.DeviceBuffer(None, 72, _ptr=1), 1, 4, 6, [(0, 0, 6, 4)])


def test_accepted_calls():
    assert E.box_histograms_check(1, 1, 1, [(0, 0, 0, 1, 1)]) is None
    assert E.box_histograms_check(65535, 16384, 16384, [(65534, 16383, 16383, 16384, 16384)] * 16384) is None
    assert E.box_histograms_check(3, 4, 6, []) is None                     # k = 0
    assert E.box_histograms_check(3, 4, 6, [(2, 5, 3, 6, 4), (2, 5, 3, 6, 4)]) is None
    assert {"pa_box_histograms", "pa_box_histograms_check"} <= set(E.ABI_SYMBOLS)
    assert (E.BOX_HIST_BINS, E.BOX_HIST_MAX_RECTS) == (512, 16384) == (I.BINS, I.MAX_RECTS)


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_the_check_as_a_stand_alone_program(tmp_path, extra):
    exe = tmp_path / "box_histogram_check_main"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(ROOT / "tests" / "box_histogram_check_main.cpp"),
                    str(CSRC / "box_histogram_check.cpp"), "-o", str(exe)], check=True)
    run = lambda *a: subprocess.run([str(exe), *map(str, a)], capture_output=True, text=True)
    r = run()
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    for case, kw, words in REFUSALS:                       # the program and the library give the same text
        if kw["rects"] is None:
            r = run("check", kw["n"], kw["h"], kw["w"], 1, "null")
        elif len(kw["rects"]) > 100:
            continue                                       # (too long for a command line; the program's own run covers k above the limit)
        else:
            r = run("check", kw["n"], kw["h"], kw["w"], len(kw["rects"]), *[v for rc in kw["rects"] for v in rc])
        assert r.returncode == 0 and r.stdout.strip() == E.box_histograms_check(**kw), case
    assert run("check", 2, 4, 6, 2, 0, 1, 1, 5, 3, 1, 0, 0, 6, 4).stdout.strip() == "ok"
    assert run("check", 2, 4, 6, 0).stdout.strip() == "ok"


# ------------------------------------------------------------------------------------------------ scan and relabel
def test_scan_sums_the_twin_per_track_and_every_thins_it():
    frames = S.clip()
    results = S.players_script()
    tracks = I.scan(video.ArrayClip(frames), results, on_device=False, batch=10)
    assert sorted(tracks) == [1, 2, 3, 4, 5, 6, 7]
    assert tracks[2].frames == list(range(30)) and tracks[5].frames == list(range(40, 96)) and tracks[7].frames == list(range(66, 96))
    torso = (S.BW - 2 * (S.BW // 4)) * ((5 * S.BH) // 8 - S.BH // 8)
    bin_of = lambda c: ((c[0] >> 5) << 6) | ((c[1] >> 5) << 3) | (c[2] >> 5)
    for t, p in ((1, 0), (2, 1), (3, 2), (4, 3), (5, 1), (6, 3), (7, 2)):
        assert tracks[t].boxes == len(tracks[t].frames)
        assert tracks[t].hist.dtype == np.uint64 and tracks[t].hist[bin_of(S.COLOURS[p])] == torso * tracks[t].boxes == tracks[t].hist.sum()
    thin = I.scan(video.ArrayClip(frames), results, on_device=False, every=4, batch=7)
    assert thin[1].boxes == 24 and thin[1].frames == list(range(96)) and thin[5].boxes == 14 and thin[2].boxes == 8
    assert I.assign(thin)[0] == I.assign(tracks)[0] == S.WANT_MAP
    # positions: the results belong to frames 56 .. 95 of the clip
    late = I.scan(video.ArrayClip(frames), results[56:], on_device=False, positions=np.arange(56, 96))
    assert sorted(late) == [1, 3, 4, 5, 6, 7] and late[3].frames == [0, 1, 2, 3] and late[7].hist.sum() == torso * 30
    with pytest.raises(ValueError, match="the source ends"):
        I.scan(video.ArrayClip(frames[:90]), results, on_device=False)


def test_a_crowded_batch_goes_to_the_engine_in_several_calls(monkeypatch):
    """The device path over a stand-in engine whose ``box_histograms`` is the twin: at most ``MAX_RECTS`` rectangles per call, the
    same tracks as in one."""
    from tests.fake_engine import FakeEngine
    calls = []

    class Twin(FakeEngine):
        def box_histograms(self, src, n, h, w, rects, out=None):
            calls.append(len(rects))
            return I.box_histograms_host(src.arr[:n * h * w * 3].reshape(n, h, w, 3), rects)
    frames, results = S.clip(24), S.players_script(range(24))
    want = I.scan(video.ArrayClip(frames), results, on_device=False)
    monkeypatch.setattr(I, "MAX_RECTS", 5)
    got = I.scan(video.ArrayClip(frames), results, engine=Twin(), batch=8)
    assert calls == [5, 5, 5, 5, 5, 5, 2] * 3 and I.MAX_RECTS == 5 and E.BOX_HIST_MAX_RECTS == 16384
    assert sorted(got) == sorted(want) and all(np.array_equal(got[t].hist, want[t].hist) and got[t].boxes == want[t].boxes for t in want)


def test_relabel_keeps_rows_order_and_the_id_0_rule():
    rows = np.array([[1, 2, 3, 4, 0.9, 0], [5, 6, 7, 8, 0.8, 0], [9, 10, 11, 12, 0.7, 0]], np.float32)
    lazy = Players(rows=rows, ids=np.array([5, 0, 9]))
    got = I.relabel(lazy, {5: 2, 9: 6, 0: 3})
    assert got._players is None and got._rows is rows and got._ids.tolist() == [2, 0, 6] and lazy._ids.tolist() == [5, 0, 9]
    assert [p.id for p in got] == [2, None, 6] and [p.confidence for p in got] == [p.confidence for p in lazy]
    built = Players.from_json(lazy.serialize())                         # the form a prediction cache loads into
    built[0].projection = (3, 4)
    got = I.relabel(built, {5: 2})
    assert [p.id for p in got] == [2, None, 9] and got[0].projection == (3, 4) and [p.id for p in built] == [5, None, 9]
    assert all(a.xyxy is b.xyxy and a.confidence == b.confidence and a.class_id == b.class_id for a, b in zip(got, built))
    assert json.dumps(got.serialize()) == json.dumps(built.serialize()).replace('"id": 5', '"id": 2')
    assert isinstance(got[0], Player) and I.relabel(None, {}) is None and len(I.relabel(Players(), {1: 2})) == 0


# ------------------------------------------------------------------------------------------------ the runner
def run_stub(tmp_path, name="cache.json", **kw):
    tracker = S.PlayersStub(batch_size=8, save_path=tmp_path / name)
    runner = TrackingRunner([tracker], video.ArrayClip(S.clip()), tmp_path / "out.mp4", **kw)
    runner.run()
    return runner, tracker


def test_the_runner_relabels_and_leaves_everything_else_as_it_is(tmp_path, capsys):
    plain, before = run_stub(tmp_path, "plain.json")
    assert plain.identity_map is None and set(plain.timings) == {"players_tracker"}
    assert json.dumps([p.serialize() for p in before.results]) == json.dumps([p.serialize() for p in S.players_script()])
    capsys.readouterr()
    runner, tracker = run_stub(tmp_path, identities=True, identity_options=dict(on_device=False))
    assert runner.identity_map == S.WANT_MAP
    assert runner.identity_distances == {5: {2: 0.0}, 6: {3: 1.0, 4: 0.0}, 7: {3: 0.0}}
    assert "runner: identities: 7 tracks over 96 frames -> 7 assigned, 0 unassigned" in capsys.readouterr().out
    assert set(runner.timings) == {"players_tracker", "__identities__"}
    t = runner.timings["__identities__"]
    assert set(t) == {"seconds", "frames", "boxes", "tracks", "assigned", "unassigned"}
    assert (t["frames"], t["tracks"], t["assigned"], t["unassigned"]) == (96, 7, 7, 0)
    assert t["boxes"] == sum(len(p) for p in before.results) == 4 * 96 - 10 - 2 * 6
    # every box carries its person's number; rows, order and confidences are bit-identical
    assert len(tracker.results) == 96
    for i, (got, was) in enumerate(zip(tracker.results, before.results)):
        assert [p.id for p in got] == S.person(i, got) == S.person(i, was)
        assert np.array_equal(np.stack([p.xyxy for p in got]), np.stack([p.xyxy for p in was]))
        assert [(p.confidence, p.class_id) for p in got] == [(p.confidence, p.class_id) for p in was]
    assert {p.id for pl in before.results for p in pl} == {1, 2, 3, 4, 5, 6, 7}
    # the caches hold ByteTrack's ids, so a cached run gives the same answer as a fresh one
    assert (tmp_path / "cache.json").read_text() == (tmp_path / "plain.json").read_text()
    cached = S.PlayersStub(load_path=tmp_path / "cache.json")
    again = TrackingRunner([cached], video.ArrayClip(S.clip()), tmp_path / "out.mp4", identities=True, identity_options=dict(on_device=False))
    again.run()
    assert cached.fed == 0 and again.identity_map == S.WANT_MAP
    assert json.dumps([p.serialize() for p in cached.results]) == json.dumps([p.serialize() for p in tracker.results])


def test_identities_with_segments_read_only_kept_frames(tmp_path, monkeypatch):
    segments = [(0, 40), (56, 96)]
    kept = [i for lo, hi in segments for i in range(lo, hi)]
    asked = []
    real = video.get_video_frames_generator

    def recording(source, stride=1, start=0, end=None):
        asked.append((start, end))
        return real(source, stride=stride, start=start, end=end)
    monkeypatch.setattr(video, "get_video_frames_generator", recording)
    tracker = S.PlayersStub(batch_size=8, frames=kept)
    runner = TrackingRunner([tracker], video.ArrayClip(S.clip()), tmp_path / "out.mp4", segments=segments, identities=True,
                            identity_options=dict(on_device=False, batch=16))
    runner.run()
    assert runner.identity_map == S.WANT_MAP and len(tracker.results) == 80
    assert all([p.id for p in pl] == S.person(kept[i], pl) for i, pl in enumerate(tracker.results))
    assert set(asked) == {(0, 40), (56, 96)}


@pytest.mark.parametrize("kw", [dict(distributed=True), dict(fanout=True)], ids=["distributed", "fanout"])
def test_identities_with_distributed_or_fanout_are_refused(tmp_path, kw):
    with pytest.raises(ValueError, match="identities=True is not available with distributed=True or fanout=True"):
        TrackingRunner([S.PlayersStub()], video.ArrayClip(S.clip(8)), tmp_path / "out.mp4", identities=True, **kw)


def test_collected_positions_come_back_for_the_reborn_players(tmp_path):
    def collected(**kw):
        tracker = S.PlayersStub(batch_size=8)
        runner = TrackingRunner([tracker, S.keypoints_tracker(S.N)], video.ArrayClip(S.clip()), tmp_path / "out.mp4", collect_data=True, **kw)
        runner.run()
        return runner.data_analytics.into_dict()
    fixed, broken = collected(identities=True, identity_options=dict(on_device=False)), collected()
    for p in range(4):
        has_box = [S.bytetrack_id(p, i) is not None for i in range(S.N)]
        reborn = [(S.bytetrack_id(p, i) or 0) > 4 for i in range(S.N)]
        for c in "xy":
            assert [v is not None for v in fixed[f"player{p + 1}_{c}"]] == has_box
            assert [v is not None for v in broken[f"player{p + 1}_{c}"]] == [b and not r for b, r in zip(has_box, reborn)]
            assert all(a == b for a, b in zip(fixed[f"player{p + 1}_{c}"], broken[f"player{p + 1}_{c}"]) if b is not None)
    assert sum(any(r) for r in ([(S.bytetrack_id(p, i) or 0) > 4 for i in range(S.N)] for p in range(4))) == 3
