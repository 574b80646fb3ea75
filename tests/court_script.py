"""Scripted courts, cameras, clips and result-holding trackers for the court inset tests (test_court_inset_host.py,
test_gpu_court_runner.py) and for tools/court_collect_bench.py: a plausible camera over the drawn court, keypoints / players / balls
per frame from a seed, the reference's per-frame projection procedure restated without batching, and a tracker that only holds
results.  numpy and the package alone: nothing here needs pytest, an engine or a GPU."""
import numpy as np

from padel_analytics_amd import projected_court as PC, video
from padel_analytics_amd.trackers.ball_tracker import Ball
from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
from padel_analytics_amd.trackers.players_tracker import Players
from padel_analytics_amd.trackers.tracker import TrackingResults


def court_for(w, h):
    return PC.ProjectedCourt(video.VideoInfo(w, h, 30, 7))


def true_homography(court, rng, jitter=0.0):
    """A plausible camera: the drawn court's corners k1, k2, k11, k12 seen as a trapezoid in a 1280 x 720 frame -> H (frame -> court)."""
    ck = court.court_keypoints
    corners = np.array([ck.k1, ck.k2, ck.k11, ck.k12], np.float64)
    seen = np.array([[180, 660], [1100, 650], [420, 230], [860, 236]], np.float64) + rng.normal(0, jitter, (4, 2))
    return PC.find_homography(seen, corners)


def project(H, pts):
    q = np.c_[np.asarray(pts, np.float64), np.ones(len(pts))] @ H.T
    return q[:, :2] / q[:, 2:]


def frame_keypoints(court, count, H, rng, noise):
    """Where the ``count`` court keypoints appear in the frame under H (frame -> court), plus detector noise."""
    dst = np.array([k.xy for k in court.court_keypoints.keypoints(number_keypoints=count)])
    return project(np.linalg.inv(H), dst) + rng.normal(0, noise, (count, 2)), dst


SEED = 3        # chosen on the CPU: no projected coordinate of these inputs lies within 1e-6 of an integer (test_court_inset_host.py asserts it, for all)


def scripted_clip(n, count=22, seed=SEED, missing=(), same_keypoints=False):
    """Per frame: ``count`` keypoints that differ from frame to frame, four players (ids 1..4) and a ball, in a 1280 x 720 frame."""
    court = court_for(1280, 720)
    rng = np.random.default_rng(seed)
    kps, players, balls = [], [], []
    fixed = None
    for i in range(n):
        src, _ = frame_keypoints(court, count, true_homography(court, rng, jitter=3.0), rng, noise=1.0)
        k = Keypoints([Keypoint(j, (float(x), float(y))) for j, (x, y) in enumerate(src)])
        fixed = fixed or k
        kps.append(None if i in missing else (fixed if same_keypoints else k))
        rows = []
        for pid in range(4):
            cx, cy = 300 + 200 * pid + rng.uniform(-40, 40), 330 + 90 * (pid % 2) + rng.uniform(-30, 30)
            rows.append([cx - 30, cy - 80, cx + 30, cy + 80, 0.9, 0])
        order = rng.permutation(4)
        players.append(Players(rows=np.array(rows, np.float32)[order], ids=(np.arange(1, 5)[order])))
        balls.append(Ball(i, (float(rng.uniform(300, 900)), float(rng.uniform(250, 600))), 1))
    return kps, players, balls


def plain_loop(court, kps, players, balls, fixed):
    """The reference's per-frame procedure, restated without batching: -> per frame (H or None, [(id, (px, py))], ball (px, py) or None)
    and the unrounded coordinates."""
    H, out, raw = None, [], []
    for k, pl, b in zip(kps, players, balls):
        if H is None:
            if k:
                H = court.homography_matrix(k)
        elif not fixed:
            H = court.homography_matrix(k) if k else None
        pp, bp = [], None
        if H is not None and pl:
            for p in pl:
                x, y = court.project_point(p.feet, H)
                raw += [x, y]
                pp.append((p.id, (int(x), int(y))))
        if H is not None and b:
            x, y = court.project_point(b.asint(), H)
            raw += [x, y]
            bp = (int(x), int(y))
        out.append((None if H is None else H.copy(), pp, bp))
    return out, np.array(raw)


class Stored:
    """A tracker that only holds scripted results."""

    def __init__(self, name, kind, results, fixed_keypoints_detection=None):
        self.name, self.kind = name, kind
        self.results = TrackingResults()
        self.results.predictions = list(results)
        self.fixed_keypoints_detection = fixed_keypoints_detection

    def video_info_post_init(self, video_info): return self
    def object(self): return self.kind
    def draw_kwargs(self): return {}
    def restart(self): pass
    def __len__(self): return len(self.results)
    def __str__(self): return self.name


def stub_trackers(kps, players, balls, fixed=None):
    return [Stored("players_tracker", Players, players), Stored("ball_tracker", Ball, balls),
            Stored("keypoints_tracker", Keypoints, kps, fixed_keypoints_detection=fixed)]


def scale_clip(kps, players, balls):
    """The 1280 x 720 script at half size, for the 640 x 360 source (a frame without keypoints: an empty detection)."""
    kps = [Keypoints([]) if k is None else Keypoints([Keypoint(q.id, (q.xy[0] / 2, q.xy[1] / 2)) for q in k]) for k in kps]
    players = [Players(rows=np.concatenate([pl._rows[:, :4] / 2, pl._rows[:, 4:]], 1), ids=pl._ids) for pl in players]
    return kps, players, [Ball(b.frame, (b.xy[0] / 2, b.xy[1] / 2), 1) for b in balls]
