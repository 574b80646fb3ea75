"""The scripted clip of the identity tests (test_identity_host.py, test_gpu_identity_runner.py) and of tools/identity_bench.py: four
filled rectangles in four saturated colours on a grey court, moving slowly, and ByteTrack's ids for them as a script — player 2 is
lost for 10 frames and returns as id 5, players 3 and 4 vanish together and return as 7 and 6.  The colours fall into four different
bins, so two players are at distance 1.0 and a player is at distance 0 from themself: nothing here rests on ``max_distance``.
numpy and the package alone: nothing here needs pytest, an engine or a GPU."""
import json

import numpy as np

from padel_analytics_amd import projected_court as PC, video
from padel_analytics_amd.trackers.keypoints_tracker import Keypoint, Keypoints
from padel_analytics_amd.trackers.players_tracker import Players
from padel_analytics_amd.trackers.tracker import NoPredictFrames, Tracker
from tests.court_script import Stored, project

N, H, W = 96, 96, 160
COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255))            # BGR of players 1..4
BW, BH = 16, 32
WANT_MAP = {1: 1, 2: 2, 3: 3, 4: 4, 5: 2, 6: 4, 7: 3}


def corner(p: int, i: int) -> tuple:
    """Top-left pixel of player p's (0..3) rectangle in frame i: even players drift right, odd ones left, all of them down."""
    return 4 + 38 * p + (i // 8 if p % 2 == 0 else -(i // 8)) + (11 if p % 2 else 0), 20 + 8 * (p % 2) + i // 12


def clip(n: int = N, h: int = H, w: int = W) -> np.ndarray:
    frames = np.full((n, h, w, 3), 128, np.uint8)
    for i in range(n):
        for p in range(4):
            x, y = corner(p, i)
            frames[i, y:y + BH, x:x + BW] = COLOURS[p]
    return frames


def bytetrack_id(p: int, i: int):
    """What ByteTrack calls player p (0..3) in source frame i; None where the track is lost."""
    if p == 1:
        return 2 if i < 30 else (None if i < 40 else 5)
    if p >= 2:
        return p + 1 if i < 60 else (None if i < 66 else (7 if p == 2 else 6))
    return 1


def players_script(frames=range(N)) -> list:
    """One ``Players`` per listed source frame: boxes with fractional corners around the rectangles (floor / ceil give the rectangle
    back), rows in an order that rotates from frame to frame, confidences that tell the rows apart."""
    out = []
    for i in frames:
        rows, ids = [], []
        for p in np.roll(np.arange(4), i):
            t = bytetrack_id(int(p), i)
            if t is None:
                continue
            x, y = corner(int(p), i)
            rows.append([x + 0.25, y + 0.5, x + BW - 0.25, y + BH - 0.5, 0.5 + 0.1 * p + 0.001 * i, 0])
            ids.append(t)
        out.append(Players(rows=np.array(rows, np.float32).reshape(-1, 6), ids=np.array(ids, np.int64)))
    return out


def person(i: int, players) -> list:
    """The player number (1..4) behind each row of frame i's ``Players``, by where the box is."""
    where = {corner(p, i): p + 1 for p in range(4)}
    return [where[(int(np.floor(q.xyxy[0])), int(np.floor(q.xyxy[1])))] for q in players]


def write_cache(path, frames=range(N)) -> None:
    with open(path, "w") as f:
        json.dump([pl.serialize() for pl in players_script(frames)], f)


class PlayersStub(Tracker):
    """A batch tracker that gives the script's ``Players`` for the frames it is fed (it counts them: the runner feeds ``frames`` in
    order), or loads them through ``load_path``; ``save_path`` works as for any tracker."""
    DEVICE = "cpu"
    streams = False

    def __init__(self, batch_size=8, frames=range(N), **kw):
        self.batch_size, self.order, self.fed = batch_size, list(frames), 0
        super().__init__(**kw)

    def video_info_post_init(self, video_info): return self
    def object(self): return Players
    def draw_kwargs(self): return {"video_info": None, "annotator": "rectangle_bounding_box", "show_confidence": True}
    def restart(self): self.results.restart()
    def __str__(self): return "players_tracker"

    def predict_sample(self, sample, **kwargs):
        out = players_script(self.order[self.fed:self.fed + len(sample)])
        self.fed += len(sample)
        return out

    def predict_frames(self, frame_generator, **kwargs):
        raise NoPredictFrames()


def keypoints_tracker(n: int, h: int = H, w: int = W):
    """Fixed court keypoints: the drawn court's twelve points seen through one plausible camera, the same in every frame."""
    court = PC.ProjectedCourt(video.VideoInfo(w, h, 30, n))
    ck = court.court_keypoints
    seen = np.array([[0.14 * w, 0.92 * h], [0.86 * w, 0.9 * h], [0.33 * w, 0.32 * h], [0.67 * w, 0.33 * h]], np.float64)
    Hm = PC.find_homography(seen, np.array([ck.k1, ck.k2, ck.k11, ck.k12], np.float64))
    dst = np.array([k.xy for k in ck.keypoints(number_keypoints=12)])
    k = Keypoints([Keypoint(j, (float(x), float(y))) for j, (x, y) in enumerate(project(np.linalg.inv(Hm), dst))])
    return Stored("keypoints_tracker", Keypoints, [k] * n, fixed_keypoints_detection=k)
