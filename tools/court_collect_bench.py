#!/usr/bin/env python
"""Host cost of the court projection per 64 frames: ``ProjectedCourt.project_batch`` — 22 keypoints that differ per frame, four
players and a ball — beside 64 single calls of ``find_homography`` on the same keypoints, and beside the same batch with fixed
keypoints (one solve).  CPU only: no engine, no GPU.

    python tools/court_collect_bench.py [--frames 64] [--reps 20] > profiles/court_collect.txt
"""
import argparse, json, platform, statistics, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from padel_analytics_amd import projected_court as PC, video
    from padel_analytics_amd.analytics import DataAnalytics
    from tests.court_script import scripted_clip
    n = a.frames
    kps, players, balls = scripted_clip(n, count=22)
    court = PC.ProjectedCourt(video.VideoInfo(1280, 720, 30, n))
    dst = np.array([k.xy for k in court.court_keypoints.keypoints(number_keypoints=22)])
    srcs = [np.array([k.xy for k in kp.keypoints]) for kp in kps]

    def batch(fixed):
        def run():
            court.H = None
            court.project_batch(kps, players, balls, fixed)
        return run

    def collect():
        court.H = None
        da = DataAnalytics()
        shift = court.court_keypoints.shift_point_origin
        for fp in court.project_batch(kps, players, balls, False):
            for p in fp.players:
                da.add_player_position(p.id, shift(tuple(float(v) for v in p.projection), "meters"))
            da.step(1)

    import contextlib, io
    rows = [("find_homography, %d single calls (22 points each)" % n, lambda: [PC.find_homography(s, dst) for s in srcs]),
            ("find_homography_batch, one call over the %d frames" % n, lambda: PC.find_homography_batch(np.stack(srcs), dst)),
            ("project_batch, keypoints per frame: %d solves + 4 players and a ball projected per frame" % n, batch(False)),
            ("project_batch, fixed keypoints: 1 solve + the same projections", batch(True)),
            ("project_batch per frame + DataAnalytics collection (the runner's __collect__)", collect)]
    print("# " + " ".join(["python", "tools/court_collect_bench.py"] + sys.argv[1:]))
    print(f"# CPU time on the host this was run on ({platform.processor() or platform.machine()}, numpy {np.__version__}); no GPU involved")
    base = None
    for what, fn in rows:
        with contextlib.redirect_stdout(io.StringIO()):
            t = timed(fn, a.reps)
        med = statistics.median(t)
        base = base or med
        print(json.dumps({"what": what, "frames": n, "ms_median": round(1e3 * med, 3), "ms_min": round(1e3 * min(t), 3), "ms_max": round(1e3 * max(t), 3),
                          "vs_single_calls": round(med / base, 3)}))
