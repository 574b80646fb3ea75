"""``TrackingRunner(identities=True)`` on the GPU, end to end over the scripted clip of tests/identity_script.py: 96 frames of
160 x 96, four rectangles in four saturated colours on a grey court.  No detector runs: the ``Players`` come from a prediction cache
the test writes (ByteTrack's ids: player 2 returns as 5, players 3 and 4 as 7 and 6), the court keypoints are fixed.  The clip went
through a .y4m file once, so that the file, a device clip and host frames hold the same pixels."""
import json

import numpy as np
import pytest

from padel_analytics_amd import engine as E, identity as I, render as R, video
from padel_analytics_amd.trackers import TrackingRunner
from tests import identity_script as S

pytestmark = pytest.mark.gpu

N, H, W = S.N, S.H, S.W
SEGMENTS = [(0, 40), (56, 96)]
KEPT = [i for lo, hi in SEGMENTS for i in range(lo, hi)]


@pytest.fixture(scope="module")
def script(tmp_path_factory):
    d = tmp_path_factory.mktemp("identity")
    with video.Y4mSink(d / "clip.y4m", W, H, fps=30) as sink:
        sink.write_host(video.bgr_to_yuv420_host(S.clip(), sink.desc, sink.enc), N)
    frames = np.stack([np.asarray(f) for f in video.get_video_frames_generator(str(d / "clip.y4m"))])
    assert frames.shape == (N, H, W, 3)
    S.write_cache(d / "players.json")
    S.write_cache(d / "kept.json", KEPT)
    # what the twin says about the stored boxes (computed once)
    tracks = I.scan(video.ArrayClip(frames), S.players_script(), on_device=False)
    return dict(dir=d, path=str(d / "clip.y4m"), frames=frames, tracks=tracks)


def run(script, source, tmp_path, cache="players.json", **kw):
    players = S.PlayersStub(load_path=script["dir"] / cache)
    runner = TrackingRunner([players, S.keypoints_tracker(len(players))], source, tmp_path / "out.mp4", collect_data=True, **kw)
    runner.run()
    assert players.fed == 0                                  # the cache was used: nothing was predicted
    return runner, players


def same_tracks(a: dict, b: dict) -> bool:
    return sorted(a) == sorted(b) and all(a[t].frames == b[t].frames and a[t].boxes == b[t].boxes and np.array_equal(a[t].hist, b[t].hist)
                                          for t in a)


def test_the_twin_tells_the_players_apart(script):
    t = script["tracks"]
    for a in t:
        for b in t:
            same = S.WANT_MAP[a] == S.WANT_MAP[b]
            assert I.distance(t[a].hist, t[b].hist) == (0.0 if same else 1.0), (a, b)


def test_every_player_keeps_their_number(gpu_engine, script, tmp_path, capsys):
    clip = video.DeviceClip(gpu_engine, script["frames"])
    try:
        runner, players = run(script, clip, tmp_path, identities=True)
        on_gpu = I.scan(clip, S.players_script(), engine=gpu_engine, batch=20)
    finally:
        clip.free()
    assert runner.identity_map == S.WANT_MAP
    assert all(d in (0.0, 1.0) for c in runner.identity_distances.values() for d in c.values())
    assert same_tracks(on_gpu, script["tracks"])             # the device scan's histograms equal the twin's
    assert "runner: identities: 7 tracks over 96 frames -> 7 assigned, 0 unassigned" in capsys.readouterr().out
    t = runner.timings["__identities__"]
    assert (t["frames"], t["boxes"], t["tracks"], t["assigned"], t["unassigned"]) == (N, 4 * N - 10 - 12, 7, 7, 0)
    script_players = S.players_script()
    assert len(players.results) == N
    for i, pl in enumerate(players.results):
        assert [p.id for p in pl] == S.person(i, pl), i
        assert json.dumps([dict(s, id=None) for s in pl.serialize()]) == json.dumps([dict(s, id=None) for s in script_players[i].serialize()])
    # a position for each of the four players in every frame where that player has a box; without the repair None for the reborn
    fixed = runner.data_analytics.into_dict()
    broken = run(script, video.ArrayClip(script["frames"]), tmp_path)[0]
    assert broken.identity_map is None and "__identities__" not in broken.timings
    broken = broken.data_analytics.into_dict()
    lost = 0
    for p in range(4):
        has_box = [S.bytetrack_id(p, i) is not None for i in range(N)]
        reborn = [(S.bytetrack_id(p, i) or 0) > 4 for i in range(N)]
        lost += sum(reborn)
        for c in "xy":
            assert [v is not None for v in fixed[f"player{p + 1}_{c}"]] == has_box
            assert [v is not None for v in broken[f"player{p + 1}_{c}"]] == [b and not r for b, r in zip(has_box, reborn)]
    assert lost == 56 + 30 + 30


@pytest.mark.parametrize("kind", ["y4m", "host"])
def test_the_same_clip_as_a_file_and_as_host_frames(gpu_engine, script, tmp_path, kind):
    source = script["path"] if kind == "y4m" else video.ArrayClip(script["frames"])
    runner, players = run(script, source, tmp_path, identities=True, identity_options=dict(batch=40))
    assert runner.identity_map == S.WANT_MAP
    assert all([p.id for p in pl] == S.person(i, pl) for i, pl in enumerate(players.results))
    assert same_tracks(I.scan(source, S.players_script(), engine=gpu_engine, batch=7), script["tracks"])
    thin = I.scan(source, S.players_script(), engine=gpu_engine, every=5)
    assert same_tracks(thin, I.scan(video.ArrayClip(script["frames"]), S.players_script(), every=5, on_device=False))


def test_segments_read_kept_frames_only(gpu_engine, script, tmp_path, monkeypatch):
    asked = []
    real = video.get_video_frames_generator

    def recording(source, stride=1, start=0, end=None):
        asked.append((start, end))
        return real(source, stride=stride, start=start, end=end)
    monkeypatch.setattr(video, "get_video_frames_generator", recording)
    runner, players = run(script, script["path"], tmp_path, cache="kept.json", identities=True, segments=SEGMENTS)
    assert set(asked) == set(SEGMENTS)
    assert runner.identity_map == S.WANT_MAP and len(players.results) == len(KEPT) == runner.timings["__identities__"]["frames"]
    assert all([p.id for p in pl] == S.person(KEPT[i], pl) for i, pl in enumerate(players.results))
    data = runner.data_analytics.into_dict()
    assert [v is not None for v in data["player2_x"]] == [S.bytetrack_id(1, i) is not None for i in KEPT]


def test_the_rendered_clip_shows_the_repaired_ids(gpu_engine, script, tmp_path):
    runner, players = run(script, script["path"], tmp_path, identities=True, render=tmp_path / "out.y4m")
    assert runner.timings["__render__"]["frames"] == N
    clip = video.YuvClip.from_y4m(tmp_path / "out.y4m", on_device=False)
    assert (clip.n, clip.w, clip.h) == (N, W, H)
    geom, enc = video.yuv_desc(W, H, "i420"), video.YUV_ENC_COEFFS["bt601_limited"]
    for i in (0, 29, 40, 65, 66, 95):
        marks = runner.frame_marks(i)
        label = R.text(f"FRAME: {i + 1}", 20, 30, 3, (0, 255, 255))
        drawn = label + players.results[i].marks(**players.draw_kwargs())
        assert marks[:len(drawn)] == drawn, i
        want = R.render_host(script["frames"][i:i + 1], *R.pack([marks]), out=E.RENDER_YUV420, geom=geom, enc=enc)
        assert np.array_equal(clip._host_bytes(i, 1), want), i
    # frame 95 is labelled 1 .. 4, the way frame 0 is
    names = lambda i: sorted(str(p.id) for p in players.results[i])
    assert names(95) == names(0) == ["1", "2", "3", "4"]
