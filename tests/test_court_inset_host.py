"""The court inset and the collection of player positions without a GPU: ``ProjectedCourt.inset_marks`` (known answers),
``find_homography_batch`` against ``find_homography``, ``ProjectedCourt.project_batch`` against a plain per-frame loop (tests/court_script.py),
the homography state machine of the reference (projected_court.py:633-647), and ``TrackingRunner(collect_data=True)`` over stub
trackers that only hold scripted results — no engine, no frame read."""
import copy
import json
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E, projected_court as PC, render as R, video
from padel_analytics_amd.analytics import DataAnalytics
from padel_analytics_amd.trackers import TrackingRunner
from padel_analytics_amd.trackers.ball_tracker import Ball
from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
from padel_analytics_amd.trackers.players_tracker import Player, Players
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)
from tests.court_script import (court_for, frame_keypoints, plain_loop, project, scale_clip, scripted_clip, stub_trackers,
                                true_homography)

SRC = "synthetic://?n=7&h=360&w=640&fps=30&seed=15"

GOLDEN = json.loads((Path(__file__).parent / "golden" / "court_golden.json").read_text())


# ------------------------------------------------------------------------------------------------ inset_marks
# 640 x 360 is not in the golden; by hand from the reference's arithmetic: WIDTH = int(.14 * 640) = 89, HEIGHT = int(.47 * 360) = 169,
# the panel ends at x = 640 - 50 and y = 50 + 169
BACKGROUNDS = {(1280, 720): next(g["background"] for g in GOLDEN["geometry"] if (g["width"], g["height"]) == (1280, 720)),
               (640, 360): [[501, 50], [590, 219]]}


@pytest.mark.parametrize("w,h", sorted(BACKGROUNDS))
def test_inset_marks_known_answers(w, h):
    court = court_for(w, h)
    marks = court.inset_marks()
    (x0, y0), (x1, y1) = BACKGROUNDS[(w, h)]
    if (w, h) == (1280, 720):
        assert [[x0, y0], [x1, y1]] == [[1051, 50], [1230, 388]]        # int(.14 * 1280) = 179, int(.47 * 720) = 338
    assert marks[0] == (E.MARK_BLEND, x0, y0, x1, y1, 0, 0xffffff, 128)  # corners inclusive, white at 128 / 256
    assert [m[0] for m in marks] == [E.MARK_BLEND] + [E.MARK_DISC] * 13 + [E.MARK_SEGMENT] * 8
    ck = court.court_keypoints
    discs = marks[1:14]
    assert [(m[1], m[2]) for m in discs] == [tuple(getattr(ck, f"k{i}")) for i in range(1, 13)] + [tuple(ck.origin)]
    assert all(m[5] == 5 and m[7] == 0 for m in discs)
    assert [m[6] for m in discs] == [0xff0000] * 12 + [0x00ff00]         # RGB (255, 0, 0) and (0, 255, 0) as B | G << 8 | R << 16
    segs = marks[14:]
    assert [((m[1], m[2]), (m[3], m[4])) for m in segs] == [(tuple(a), tuple(b)) for a, b in ck.lines()]
    assert all(m[5] == 2 and m[6] == 0 and m[7] == 0 for m in segs)
    # every part of the court lies inside the panel, and the engine's checks accept the list
    assert all(x0 <= m[1] <= x1 and y0 <= m[2] <= y1 for m in marks[1:])
    assert E.render_check(1, h, w, *R.pack([marks])) is None
    assert court.inset_marks() == marks and court.inset_marks() is not marks


def test_the_panel_halves_the_way_to_white():
    frame = np.full((1, 360, 640, 3), (10, 100, 201), np.uint8)
    drawn = R.render_host(frame, *R.pack([court_for(640, 360).inset_marks()[:1]]))[0]
    assert tuple(drawn[50, 501]) == tuple(drawn[219, 590]) == (133, 178, 228)       # (p * 128 + 255 * 128 + 128) >> 8
    changed = (drawn != frame[0]).any(-1)
    assert changed.sum() == 90 * 170 and changed[50:220, 501:591].all()


def test_projection_marks_of_a_player_and_a_ball():
    p = Player.from_row(np.array([100, 50, 140, 150], np.float32), 0.9, 0, 3)
    assert p.projection_marks() == []                                    # nothing at all without a projection
    p.projection = (540, 130)
    assert p.projection_marks() == [R.disc(540, 130, 8, (255, 0, 0))] + R.text("3", 540, 130 - 10 - 13, 2, (255, 0, 0))
    assert Players([p, Player.from_row(np.array([0, 0, 1, 1], np.float32), 0.9, 0, 4)]).projection_marks() == p.projection_marks()
    b = Ball(0, (1.0, 2.0), 1)
    assert b.projection_marks() == []
    b.projection = (520, 100)
    assert b.projection_marks() == [R.disc(520, 100, 6, (0, 255, 255))]   # RGB (255, 255, 0)


# ------------------------------------------------------------------------------------------------ homographies
@pytest.mark.parametrize("count", [12, 18, 22])
def test_batch_solve_agrees_with_the_single_solve(count):
    court = court_for(1280, 720)
    rng = np.random.default_rng(100 + count)
    n = 9
    src = np.empty((n, count, 2))
    for i in range(n):
        src[i], dst = frame_keypoints(court, count, true_homography(court, rng, jitter=15.0), rng, noise=1.5)
    got = PC.find_homography_batch(src, dst)
    assert got.shape == (n, 3, 3) and np.all(got[:, 2, 2] == 1.0)
    probe = np.array([[x, y] for x in (100, 640, 1200) for y in (250, 450, 700)], np.float64)
    worst = 0.0
    for i in range(n):
        one = PC.find_homography(src[i], dst)
        worst = max(worst, float(np.abs(project(got[i], np.r_[src[i], probe]) - project(one, np.r_[src[i], probe])).max()))
    print(f"{count} points: batch vs single reprojection differs by at most {worst:.3e} px")
    assert worst < 1e-6
    assert PC.find_homography_batch(src[:0], dst).shape == (0, 3, 3)
    with pytest.raises(ValueError):
        PC.find_homography_batch(src[:, :5], dst)


@pytest.mark.parametrize("count", [12, 18, 22])
def test_batch_solve_recovers_an_exact_homography(count):
    court = court_for(1280, 720)
    rng = np.random.default_rng(7)
    Hs = [true_homography(court, rng, jitter=20.0) for _ in range(5)]
    src = np.stack([frame_keypoints(court, count, H, rng, noise=0.0)[0] for H in Hs])
    dst = np.array([k.xy for k in court.court_keypoints.keypoints(number_keypoints=count)])
    got = PC.find_homography_batch(src, dst)
    for H, g in zip(Hs, got):
        assert np.abs(g - H / H[2, 2]).max() < 1e-8 * np.abs(H / H[2, 2]).max()
        assert np.abs(project(g, src[0]) - project(H, src[0])).max() < 1e-8


# ------------------------------------------------------------------------------------------------ project_batch
def test_project_batch_equals_a_plain_per_frame_loop():
    n = 64
    kps, players, balls = scripted_clip(n)
    want, raw = plain_loop(court_for(1280, 720), kps, players, balls, fixed=False)
    assert len(raw) == n * 10
    assert np.abs(raw - np.round(raw)).min() > 1e-6                      # for ALL of them: int() cannot flip on a rounding difference
    court = court_for(1280, 720)
    got = court.project_batch(kps[:40], players[:40], balls[:40], False) + court.project_batch(kps[40:], players[40:], balls[40:], False)
    assert len(got) == n
    for fp, (H, pp, bp) in zip(got, want):
        assert [(p.id, p.projection) for p in fp.players] == pp
        assert fp.ball.projection == bp
        assert np.abs(fp.H - H).max() < 1e-6 * np.abs(H).max()
    assert all(isinstance(v, int) for fp in got for p in fp.players for v in p.projection)
    # the projections land in the drawn court's neighbourhood (a sanity check of the scripted camera, not of the code under test)
    bp = court.background_position
    xs = np.array([p.projection for fp in got for p in fp.players])
    assert (xs[:, 0] > bp.top_left[0] - 100).all() and (xs[:, 0] < bp.bottom_right[0] + 100).all()


def count_solves(monkeypatch):
    calls = []
    real = PC.find_homography_batch

    def counting(src, dst, *a, **kw):
        calls.append(len(src))
        return real(src, dst, *a, **kw)
    monkeypatch.setattr(PC, "find_homography_batch", counting)
    return calls


def test_fixed_keypoints_cost_one_solve_for_the_whole_clip(monkeypatch):
    calls = count_solves(monkeypatch)
    kps, players, balls = scripted_clip(10, count=12, same_keypoints=True)
    kps[4] = None                                                        # fixed: a frame without keypoints changes nothing
    court = court_for(1280, 720)
    got = court.project_batch(kps[:3], players[:3], balls[:3], True) + court.project_batch(kps[3:], players[3:], balls[3:], True)
    assert calls == [1]
    assert all(fp.H is got[0].H for fp in got) and court.H is got[0].H
    want, _ = plain_loop(court_for(1280, 720), kps, players, balls, fixed=True)
    for fp, (H, pp, bp) in zip(got, want):
        assert [(p.id, p.projection) for p in fp.players] == pp and fp.ball.projection == bp


def test_a_frame_without_keypoints_resets_the_homography(monkeypatch):
    calls = count_solves(monkeypatch)
    kps, players, balls = scripted_clip(8, count=18, missing=(0, 3, 4, 7))
    kps[4] = Keypoints([])                                               # an empty detection counts as missing, like None
    players[5] = Players([])                                             # a frame with a homography and nobody to project
    before = [copy.deepcopy([p.serialize() for p in pl]) for pl in players], [b.serialize() for b in balls]
    court = court_for(1280, 720)
    got = court.project_batch(kps[:4], players[:4], balls[:4], False)
    assert court.H is None                                               # frame 3 had no keypoints: carried into the next batch as None
    got += court.project_batch(kps[4:], players[4:], balls[4:], False)
    assert [fp.H is not None for fp in got] == [False, True, True, False, False, True, True, False]
    assert sum(calls) == 4                                               # one solve per frame that has keypoints
    for i, fp in enumerate(got):
        if fp.H is None:
            assert fp.players is None and fp.ball is None                # no projections for it
        elif i == 5:
            assert fp.players is None and fp.ball.projection is not None
        else:
            assert len(fp.players) == 4 and all(p.projection for p in fp.players) and fp.ball.projection
    want, _ = plain_loop(court_for(1280, 720), kps, players, balls, fixed=False)
    assert [[(p.id, p.projection) for p in (fp.players or [])] for fp in got] == [pp for _, pp, _ in want]
    assert [None if fp.ball is None else fp.ball.projection for fp in got] == [bp for _, _, bp in want]
    # the stored results are not touched: the projections are on copies
    assert ([[p.serialize() for p in pl] for pl in players], [b.serialize() for b in balls]) == before
    assert all(p.projection is None for pl in players for p in pl) and all(b.projection is None for b in balls)
    with pytest.raises(ValueError):
        court.project_batch([Keypoints([Keypoint(j, (1.0 * j, 2.0)) for j in range(13)])], [None], [None], False)
    with pytest.raises(ValueError):
        court.project_batch(kps, players[:3], balls, False)


# ------------------------------------------------------------------------------------------------ the runner
def test_the_runner_collects_from_stored_results_alone(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(TrackingRunner, "RENDER_BATCH", 3)
    monkeypatch.setattr(E, "default_engine", lambda *a, **kw: pytest.fail("the collection must not touch an engine"))
    monkeypatch.setattr(video, "get_video_frames_generator", lambda *a, **kw: pytest.fail("the collection must not read a frame"))
    kps, players, balls = scale_clip(*scripted_clip(7, missing=(4,)))
    players[2] = Players(rows=np.concatenate([players[2]._rows, players[2]._rows[:2]]), ids=np.array(list(players[2]._ids) + [11, 12]))
    runner = TrackingRunner(stub_trackers(kps, players, balls), SRC, tmp_path / "out.mp4", collect_data=True)
    assert isinstance(runner.data_analytics, DataAnalytics) and runner.court_inset and not runner.is_fixed_keypoints
    runner.run()
    said = capsys.readouterr().out
    assert "skipped" not in said and "collected the players' positions of 7 frames" in said
    assert said.count("no homography for some frames") == 1
    assert len(runner.data_analytics) == 7
    assert set(runner.timings) == {"__collect__"} and runner.timings["__collect__"]["frames"] == 7
    # by hand: a per-frame loop, positions in metres from the court centre
    court = court_for(640, 360)
    want, _ = plain_loop(court, kps, players, balls, fixed=False)
    ck = court.court_keypoints
    expect = {"frame": list(range(7)), **{f"player{p}_{c}": [None] * 7 for p in (1, 2, 3, 4) for c in "xy"}}
    for i, (_, pp, _) in enumerate(want):
        for pid, (x, y) in pp:
            if pid in (1, 2, 3, 4):
                expect[f"player{pid}_x"][i] = (float(x) - ck.origin[0]) * 10 / ck.width
                expect[f"player{pid}_y"][i] = (float(y) - ck.origin[1]) * 10 / ck.width
    got = runner.data_analytics.into_dict()
    assert got == expect
    assert [v is None for v in got["player1_x"]] == [False, False, False, False, True, False, False]
    # frame_marks carries the inset: panel and court always, the projections where there is a homography
    for i in range(7):
        marks = runner.frame_marks(i)
        inset = runner.inset_marks(i)
        assert marks[-len(inset):] == inset and inset[:22] == court.inset_marks()
        assert len(inset) == 22 + (0 if i == 4 else 4 * 2 + (2 * 3 if i == 2 else 0) + 1)      # ids 11 and 12: a disc and two glyphs each
    runner.restart()
    assert len(runner.data_analytics) == 1 and runner.projected_court.H is None and runner._projected == []


def test_the_hand_over_of_the_references_main(tmp_path, capsys):
    """``collect_data=True``, ``run()``, then ``data_analytics.into_dataframe(fps).to_csv(...)`` as the reference's ``main.py`` does."""
    import pandas
    kps, players, balls = scale_clip(*scripted_clip(7))
    runner = TrackingRunner(stub_trackers(kps, players, balls), SRC, tmp_path / "out.mp4", collect_data=True)
    runner.run()
    df = runner.data_analytics.into_dataframe(runner.video_info.fps)
    assert isinstance(df, pandas.DataFrame) and len(df) == 7 and len(df.columns) == 178
    df.to_csv(tmp_path / "data.csv")
    back = pandas.read_csv(tmp_path / "data.csv", index_col=0)
    assert list(back.columns) == list(df.columns) and list(back["frame"]) == list(range(7))
    assert back["player1_x"].notna().all() and np.allclose(back["player3_y"], df["player3_y"], rtol=0, atol=1e-12)


def test_drawing_twice_collects_once_and_an_empty_clip_restarts(tmp_path, capsys):
    kps, players, balls = scale_clip(*scripted_clip(7))
    runner = TrackingRunner(stub_trackers(kps, players, balls), SRC, tmp_path / "out.mp4", collect_data=True)
    assert len(runner.frame_marks(2)) > 22                               # asked before the step ran: must not stay in the way
    runner.draw_and_collect_data()
    first = runner.data_analytics.into_dict()
    runner.draw_and_collect_data()                                       # a second pass starts over: nothing is appended twice
    assert runner.data_analytics.into_dict() == first and len(runner.data_analytics) == 7 and first["frame"] == list(range(7))
    empty = TrackingRunner(stub_trackers([], [], []), SRC, tmp_path / "out.mp4", collect_data=True, start=7)
    assert empty.n_available == 0
    empty.draw_and_collect_data()
    assert len(empty.data_analytics) == 0                                # falsy through __len__ ...
    empty.restart()
    assert len(empty.data_analytics) == 1 and empty.data_analytics.frames == [0]      # ... and restarted all the same


def test_fixed_keypoints_in_the_runner(tmp_path, capsys, monkeypatch):
    calls = count_solves(monkeypatch)
    kps, players, balls = scale_clip(*scripted_clip(7, count=12, same_keypoints=True))
    runner = TrackingRunner(stub_trackers(kps, players, balls, fixed=kps[0]), SRC, tmp_path / "out.mp4", collect_data=True)
    assert runner.is_fixed_keypoints
    runner.draw_and_collect_data()
    assert calls == [1] and len(runner.data_analytics) == 7
    assert all(v is not None for v in runner.data_analytics.into_dict()["player4_y"])


def test_without_collect_data_nothing_changes(tmp_path, capsys):
    kps, players, balls = scale_clip(*scripted_clip(7))
    runner = TrackingRunner(stub_trackers(kps, players, balls), SRC, tmp_path / "out.mp4")
    assert runner.data_analytics is None and runner.court_inset is False
    runner.run()
    assert "drawing / data collection is outside the hot path of this build (skipped)" in capsys.readouterr().out
    assert runner.timings == {}
    assert E.MARK_BLEND not in {m[0] for m in runner.frame_marks(0)}
    assert list(tmp_path.iterdir()) == []
