#!/usr/bin/env python
"""What drawing the annotated clip costs (csrc/render.hip), alone and as the runner's render step.  GPU only.

(a) the kernel on 64 frames of 1280 x 720 resident in HBM, for a scene of four players with labels and skeletons, a ball, 22 court
    keypoints and the frame text (the mark count is printed) and for no marks at all, to NV12, I420 and BGR: warm-up calls, then
    --reps calls between one pair of HIP events on the engine's stream (``pa_engine_timer_start / _stop``).  Reported: microseconds per
    call, frames/s, GB/s of the 4.5 bytes per pixel a YUV pass must move (3 read, 1.5 written; 6 for BGR) and that as a share of the
    HBM peak.  The calls rotate over three source / destination sets so that a repetition does not find its bytes in the 256 MB
    last-level cache.  Every call also copies its marks to the device first (on the same stream), which the event pair includes.
    A third scene adds the court inset (``TrackingRunner(collect_data=True)``: the blending panel, the drawn court, the projected
    players and ball) to the first; a library that refuses the blending mark skips it and says so.  Two more draw the first scene's
    players with ``annotator="ellipse"`` and with ``"round_bounding_box"`` (arc marks; skipped likewise by a library without them).
(b) ``TrackingRunner``'s render step on the same clip and marks, end to end — render + download + write of the ``.y4m`` — with a
    host clock; the frames come from a ``DeviceClip``.  Then the same with ``collect_data=True`` — projection, collection and the inset
    on top — once with fixed court keypoints (one homography per clip) and once with keypoints that differ per frame (one per frame).
    Then the first once more with ``annotator="ellipse"``.

    python tools/render_bench.py [--frames 64] [--reps 50] [--warmup 5] [--passes 3] [--skip-runner] [--kernel-only] [--scale]

``--kernel-only`` runs (a) with few repetitions and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``.
``--scale`` runs ``scale_mode`` instead: ``Engine.render(scale=)`` and ``TrackingRunner(render_scale=)`` at scales 1, 2, 4 (1280 x 720)
and 1, 3 (1920 x 1080) — profiles/render_scale.txt.
"""
import argparse, contextlib, json, statistics, sys, tempfile, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12          # bytes/s, the MI355X's HBM3E specification


def scene(i: int, w: int, h: int):
    """The result objects of frame ``i``: (Players, PlayersKeypoints, Ball, Keypoints) of a plausible padel frame."""
    from padel_analytics_amd.trackers.ball_tracker import Ball
    from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
    from padel_analytics_amd.trackers.players_keypoints_tracker import PlayerKeypoint, PlayerKeypoints, PlayersKeypoints
    from padel_analytics_amd.trackers.players_tracker import Player, Players
    rng = np.random.default_rng(1000 + i)
    players, skeletons = [], []
    for k in range(4):
        cx, cy = w * (0.2 + 0.2 * k) + rng.integers(-20, 20), h * (0.35 + 0.1 * (k % 2)) + rng.integers(-10, 10)
        bw, bh = 70 + 10 * k, 170 + 15 * k
        players.append(Player.from_row(np.array([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], np.float32), 0.8 + 0.04 * k, 0, k + 1))
        names = PlayerKeypoints.KEYPOINTS_NAMES
        skeletons.append(PlayerKeypoints([PlayerKeypoint(j, n, (cx + rng.integers(-bw // 2, bw // 2), cy + rng.integers(-bh // 2, bh // 2)))
                                          for j, n in enumerate(names)]))
    court = Keypoints([Keypoint(j, (w * (0.1 + 0.8 * (j % 6) / 5), h * (0.3 + 0.6 * (j // 6) / 3))) for j in range(22)])
    return Players(players), PlayersKeypoints(skeletons), Ball(i, (w * 0.5 + 5 * i, h * 0.4 + 2 * i), 1), court


class Stored:
    """A tracker that only holds results (what ``TrackingRunner`` finds after its trackers ran, or loaded their caches)."""

    def __init__(self, name, results, kwargs=None, kind=None, fixed_keypoints_detection=None):
        from padel_analytics_amd.trackers.tracker import TrackingResults
        self.name, self.kwargs, self.kind = name, kwargs or {}, kind
        self.results = TrackingResults()
        self.results.predictions = results
        self.fixed_keypoints_detection = fixed_keypoints_detection

    def object(self): return self.kind

    def video_info_post_init(self, video_info):
        if "video_info" in self.kwargs:
            self.kwargs["video_info"] = video_info
        return self

    def draw_kwargs(self): return self.kwargs
    def __len__(self): return len(self.results)
    def __str__(self): return self.name
    def restart(self): pass


def court_view(i: int, w: int, h: int, court):
    """22 court keypoints as a camera behind the baseline sees them in frame ``i`` (the drawn court's corners as a trapezoid that
    sways a little from frame to frame, half a pixel of detector noise): what ``project_batch`` solves a homography from."""
    from padel_analytics_amd import projected_court as PC
    from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
    rng = np.random.default_rng(5000 + i)
    ck = court.court_keypoints
    corners = np.array([ck.k1, ck.k2, ck.k11, ck.k12], np.float64)
    seen = np.array([[0.14, 0.92], [0.86, 0.9], [0.33, 0.32], [0.67, 0.33]]) * (w, h) + rng.normal(0, 2.0, (4, 2))
    back = np.linalg.inv(PC.find_homography(seen, corners))
    dst = np.array([k.xy for k in ck.keypoints(number_keypoints=22)])
    q = np.c_[dst, np.ones(22)] @ back.T
    xy = q[:, :2] / q[:, 2:] + rng.normal(0, 0.5, (22, 2))
    return Keypoints([Keypoint(j, (float(x), float(y))) for j, (x, y) in enumerate(xy)])


class Joints:
    """The 13 joints of every skeleton as discs (``PlayerKeypoint.marks``): the reference's own ``PlayersKeypoints.draw`` paints the
    lines only, a user who wants the joints adds them like this."""

    def __init__(self, pk): self.pk = pk
    def marks(self, **kw): return [m for p in self.pk for k in p for m in k.marks()]


def scale_mode(a, eng) -> None:
    """``--scale``: the scaled pass (``Engine.render(scale=)``) beside the full-size pass of the same scene, and the runner's render step
    to ``.y4m`` and ``.avi`` at each scale.  Scales 1, 2, 4 on 1280 x 720 and 1, 3 on 1920 x 1080 (720 is no multiple of 3 that gives
    even frames of a 1280-wide clip); scenes: no marks, the 206-mark scene, the same with ``annotator="round_bounding_box"``.
    (a) the kernel: as in the plain run, --reps calls between one pair of HIP events over three rotating buffer sets; the algorithmic
        bytes are 3 read per SOURCE pixel plus 1.5 (YUV) or 3 (BGR) written per OUTPUT pixel.
    (b) ``TrackingRunner(render_scale=s)``'s render step, host clock, median of --passes passes after an untimed one, with the bytes
        written per frame."""
    from padel_analytics_amd import engine as E, render as R, video
    from padel_analytics_amd.trackers import TrackingRunner
    from padel_analytics_amd.trackers.ball_tracker import Ball
    from padel_analytics_amd.trackers.keypoints_tracker import Keypoints
    from padel_analytics_amd.trackers.players_tracker import Players
    from tests import synth
    n = a.frames
    tmp = Path(tempfile.mkdtemp(prefix="render_bench_scale_"))
    enc = video.YUV_ENC_COEFFS["bt601_limited"]
    SETS = 3
    for (w, h), scales in (((1280, 720), (1, 2, 4)), ((1920, 1080), (1, 3))):
        bgr = synth.synthetic_frames(n, h, w, seed=1000)
        info = video.VideoInfo(w, h, 30, n)
        scenes = [scene(i, w, h) for i in range(n)]
        clip = video.DeviceClip(eng, bgr)

        def trackers_for(annotator):
            return [Stored("players_tracker", [s[0] for s in scenes], {"video_info": info, "annotator": annotator, "show_confidence": True}, Players),
                    Stored("players_keypoints_tracker", [s[1] for s in scenes]), Stored("joints", [Joints(s[1]) for s in scenes]),
                    Stored("ball_tracker", [s[2] for s in scenes], kind=Ball), Stored("keypoints_tracker", [s[3] for s in scenes], kind=Keypoints)]

        def runner_for(annotator, target, s):
            return TrackingRunner(trackers_for(annotator), clip, tmp / "out.mp4", render=target, engine=eng, render_scale=s)
        timed = [("no marks", R.pack([[] for _ in range(n)]))]
        for label, annotator in (("scene", "rectangle_bounding_box"), ("scene, annotator=round_bounding_box", "round_bounding_box")):
            r = runner_for(annotator, tmp / "out.y4m", 1)
            timed.append((label, R.pack([r.frame_marks(i) for i in range(n)])))
            print(json.dumps({"what": label, "h": h, "w": w, "marks_per_frame": int(timed[-1][1][1][1])}))
        src = [clip.buffer] + [eng.alloc(bgr.nbytes).upload(bgr) for _ in range(SETS - 1)]
        for out_name in ("i420", "nv12", "bgr"):
            yuv = out_name != "bgr"
            for s in scales:
                ho, wo = h // s, w // s
                geom = video.yuv_desc(wo, ho, out_name) if yuv else None
                span = video.yuv_span(n, ho, wo, geom) if yuv else n * ho * wo * 3
                dst = [eng.alloc(span) for _ in range(SETS)]
                moved = n * (h * w * 3 + ho * wo * (1.5 if yuv else 3.0))
                for label, (marks, first) in timed:
                    call = lambda i: eng.render(src[i % SETS], n, h, w, marks, first, dst[i % SETS], out=E.RENDER_YUV420 if yuv else E.RENDER_BGR,
                                                geom=geom, enc=enc if yuv else None, scale=s)
                    for i in range(a.warmup):
                        call(i)
                    eng.synchronize()
                    assert eng.render_last_path() == E.RENDER_PATH_VECTOR
                    runs = []
                    for _ in range(3):                          # three windows of --reps calls: their spread is printed
                        eng.timer_start()
                        for i in range(a.reps):
                            call(i)
                        runs.append(eng.timer_stop() / a.reps)
                    ms = statistics.median(runs)
                    print(json.dumps({"what": "render, HIP events around %d calls, 3 windows" % a.reps, "scale": s, "out": out_name, "marks": label,
                                      "frames": n, "h": h, "w": w, "us_per_call": round(1e3 * ms, 1),
                                      "us_windows": [round(1e3 * r, 1) for r in runs], "source_frames_per_s": round(n / (ms * 1e-3)),
                                      "bytes_moved": int(moved), "GB_per_s_algorithmic": round(moved / (ms * 1e-3) / 1e9, 1)}))
                for b in dst:
                    b.free()
        for b in src[1:]:
            b.free()
        if not a.skip_runner:
            for suffix in (".y4m", ".avi"):
                for s in scales:
                    target = tmp / ("out" + suffix)
                    r = runner_for("rectangle_bounding_box", target, s)
                    secs = []
                    with contextlib.redirect_stdout(sys.stderr):
                        for k in range(a.passes + 1):           # one untimed pass first
                            eng.synchronize()
                            t0 = time.perf_counter()
                            r.draw_and_collect_data()
                            secs.append(time.perf_counter() - t0)
                    med = statistics.median(secs[1:])
                    size = target.stat().st_size
                    print(json.dumps({"what": "TrackingRunner render step to " + suffix + " (host clock)", "render_scale": s, "frames": n, "h": h, "w": w,
                                      "out_h": h // s, "out_w": w // s, "seconds_median": round(med, 4), "seconds_passes": [round(x, 4) for x in secs[1:]],
                                      "frames_per_s": round(n / med, 1), "bytes_per_frame": size // n, "MB_per_s_written": round(size / med / 1e6, 1)}))
                    target.unlink()
        clip.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", action="store_true", help="the scaled pass and the runner's render_scale instead of the plain run (scale_mode)")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3, help="(b): timed passes over the clip")
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    from padel_analytics_amd import engine as E, render as R, video
    from padel_analytics_amd.trackers import TrackingRunner
    from tests import synth                                     # seeded frames (setup only)
    eng = E.default_engine(0)
    n, h, w = a.frames, a.height, a.width
    if a.kernel_only:
        a.reps, a.skip_runner = min(a.reps, 10), True
    print("# " + " ".join(["python", "tools/render_bench.py"] + sys.argv[1:]))
    if a.scale:
        scale_mode(a, eng)
        sys.exit(0)
    bgr = synth.synthetic_frames(n, h, w, seed=1000)
    info = video.VideoInfo(w, h, 30, n)
    scenes = [scene(i, w, h) for i in range(n)]
    from padel_analytics_amd.trackers.ball_tracker import Ball
    from padel_analytics_amd.trackers.keypoints_tracker import Keypoints
    from padel_analytics_amd.trackers.players_tracker import Players
    trackers = [Stored("players_tracker", [s[0] for s in scenes], {"video_info": info, "annotator": "rectangle_bounding_box", "show_confidence": True}, Players),
                Stored("players_keypoints_tracker", [s[1] for s in scenes]), Stored("joints", [Joints(s[1]) for s in scenes]),
                Stored("ball_tracker", [s[2] for s in scenes], kind=Ball), Stored("keypoints_tracker", [s[3] for s in scenes], kind=Keypoints)]
    clip = video.DeviceClip(eng, bgr)
    tmp = Path(tempfile.mkdtemp(prefix="render_bench_"))
    runner = TrackingRunner(trackers, clip, tmp / "out.mp4", render=tmp / "out.y4m", engine=eng)
    per_frame = [runner.frame_marks(i) for i in range(n)]
    full = R.pack(per_frame)
    none = R.pack([[] for _ in range(n)])
    kinds = {k: int((full[0]["kind"] == k).sum()) // n for k in range(1, 6)}
    print(json.dumps({"what": "scene", "marks_per_frame": len(per_frame[0]), "by_kind_disc_segment_fill_box_glyph": list(kinds.values())}))

    # the same scene seen by a camera (keypoints a homography can be solved from), for the court inset and the collection
    def collecting_runner(fixed: bool):
        views = [court_view(0 if fixed else i, w, h, runner.projected_court) for i in range(n)]
        ts = trackers[:-1] + [Stored("keypoints_tracker", views, kind=Keypoints, fixed_keypoints_detection=views[0] if fixed else None)]
        with contextlib.redirect_stdout(sys.stderr):                # (the runner says that it is ready: not a line of this tool's JSON)
            return TrackingRunner(ts, clip, tmp / "out.mp4", render=tmp / "out.y4m", engine=eng, collect_data=True)
    scenes_timed = [("scene", full), ("no marks", none)]
    inset_runner = collecting_runner(False)
    with_inset = [inset_runner.frame_marks(i) for i in range(n)]
    inset = R.pack(with_inset)
    refused = E.render_check(n, h, w, inset[0], inset[1])
    if refused is None:
        scenes_timed.append(("scene + court inset", inset))
        print(json.dumps({"what": "scene + court inset", "marks_per_frame": len(with_inset[0]), "of_them_blending": int((inset[0]["kind"] == 6).sum()) // n}))
    else:
        print(json.dumps({"what": "scene + court inset", "skipped": "this library refuses it: " + refused}))

    # the first scene under the annotators that draw arcs
    def annotated_runner(name: str):
        ts = [Stored("players_tracker", [s[0] for s in scenes], {"video_info": info, "annotator": name, "show_confidence": True}, Players)] + trackers[1:]
        return TrackingRunner(ts, clip, tmp / "out.mp4", render=tmp / "out.y4m", engine=eng)
    arcs_refused = None
    for name in ("ellipse", "round_bounding_box"):
        marks_of = [annotated_runner(name).frame_marks(i) for i in range(n)]
        packed = R.pack(marks_of)
        arcs_refused = E.render_check(n, h, w, packed[0], packed[1])
        if arcs_refused is None:
            scenes_timed.append((f"scene, annotator={name}", packed))
            print(json.dumps({"what": f"scene, annotator={name}", "marks_per_frame": len(marks_of[0]), "of_them_arcs": int((packed[0]["kind"] == 8).sum()) // n}))
        else:
            print(json.dumps({"what": f"scene, annotator={name}", "skipped": "this library refuses it: " + arcs_refused}))

    # ---- (a) the kernel
    SETS = 3
    enc = video.YUV_ENC_COEFFS["bt601_limited"]
    src = [clip.buffer] + [eng.alloc(bgr.nbytes).upload(bgr) for _ in range(SETS - 1)]
    for out_name in ("nv12", "i420", "bgr"):
        yuv = out_name != "bgr"
        geom = video.yuv_desc(w, h, out_name) if yuv else None
        span = video.yuv_span(n, h, w, geom) if yuv else bgr.nbytes
        dst = [eng.alloc(span) for _ in range(SETS)]
        moved = n * h * w * (4.5 if yuv else 6.0)
        for label, (marks, first) in scenes_timed:
            call = lambda i: eng.render(src[i % SETS], n, h, w, marks, first, dst[i % SETS], out=E.RENDER_YUV420 if yuv else E.RENDER_BGR,
                                        geom=geom, enc=enc if yuv else None)
            for i in range(a.warmup):
                call(i)
            eng.synchronize()
            assert eng.render_last_path() == E.RENDER_PATH_VECTOR
            eng.timer_start()
            for i in range(a.reps):
                call(i)
            ms = eng.timer_stop() / a.reps
            each = []
            for i in range(min(a.reps, 20)):
                eng.timer_start()
                call(i)
                each.append(eng.timer_stop())
            print(json.dumps({"what": "render, HIP events around %d calls" % a.reps, "out": out_name, "marks": label, "frames": n, "h": h, "w": w,
                              "us_per_call": round(1e3 * ms, 1), "us_single_call_median_min_max": [round(1e3 * statistics.median(each), 1),
                                                                                                    round(1e3 * min(each), 1), round(1e3 * max(each), 1)],
                              "frames_per_s": round(n / (ms * 1e-3)), "bytes_moved": int(moved),
                              "GB_per_s_algorithmic": round(moved / (ms * 1e-3) / 1e9, 1),
                              "share_of_HBM_peak_8TBps": round(moved / (ms * 1e-3) / HBM_PEAK, 3)}))
        for b in dst:
            b.free()
    for b in src[1:]:
        b.free()

    # ---- (b) the runner's render step: render + download + write; then with projection, collection and the inset
    if not a.skip_runner:
        runs = [("render + download + write of the .y4m", runner)]
        if refused is None:
            runs += [("the same with collect_data=True, fixed court keypoints", collecting_runner(True)),
                     ("the same with collect_data=True, court keypoints per frame", collecting_runner(False))]
        if arcs_refused is None:
            runs.append(("render + download + write of the .y4m, annotator=ellipse", annotated_runner("ellipse")))
        for what, r in runs:
            secs, collect = [], []
            with contextlib.redirect_stdout(sys.stderr):
                for k in range(a.passes + 1):                       # one untimed pass first
                    eng.synchronize()
                    t0 = time.perf_counter()
                    r.draw_and_collect_data()
                    secs.append(time.perf_counter() - t0)
                    collect.append(r.timings.get("__collect__", {}).get("seconds"))
            secs = secs[1:]
            med = statistics.median(secs)
            size = (tmp / "out.y4m").stat().st_size
            marks_per_frame = len(r.frame_marks(0))
            row = {"what": "TrackingRunner render step: " + what + " (host clock)", "frames": n, "h": h, "w": w,
                   "marks_per_frame": marks_per_frame, "seconds_median": round(med, 4), "seconds_passes": [round(s, 4) for s in secs],
                   "frames_per_s": round(n / med, 1), "file_bytes": size, "MB_per_s_written": round(size / med / 1e6, 1)}
            if collect[-1] is not None:
                row["collect_seconds_passes"] = [round(c, 4) for c in collect[1:]]
            print(json.dumps(row))
            (tmp / "out.y4m").unlink()
    clip.free()
