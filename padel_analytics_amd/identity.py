"""Player identities that survive a lost track.

ByteTrack never gives a lost track its old id back: a player who is hidden at the net, or leaves the polygon zone for longer than
the lost-track buffer, comes back as id 5, then 6, ... — and ``analytics.DataAnalytics`` drops every id outside 1..4 by design, so
that player's columns are empty for the rest of the clip.  The reference has the same defect and nothing to repair it; nothing here
has a counterpart there, and no parity with it is claimed.

The repair is a second pass over the clip.  Every stored player box gets a colour histogram of its shirt (``torso_rect``), computed
on the GPU from the BGR bytes that are in HBM anyway (``csrc/box_histogram.hip``, ``Engine.box_histograms``; the specification is
``include/padel_hip.h``, its executable form ``box_histograms_host`` below — all integer, so the GPU and the twin agree exactly).
``scan`` sums them per ByteTrack id, ``assign`` — pure host logic — maps the ids to ``n_players`` identities, ``relabel`` rewrites a
frame's ``Players``.  ``TrackingRunner(identities=True)`` runs the three between the trackers and the render / collection step.

``max_distance = 0.5`` and the torso fractions (the middle half of the box's width, from 1/8 to 5/8 of its height) are parameters,
not findings: the project has no real footage to set them by, and they were not tuned against synthetic clips.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import engine as E, video

BINS = 512
MAX_RECTS = 16384          # engine.BOX_HIST_MAX_RECTS: the rectangles one Engine.box_histograms call takes


def _rects(rects) -> np.ndarray:
    rects = np.asarray(rects, np.int64)
    if rects.size == 0:
        return rects.reshape(0, 5)
    if rects.ndim != 2 or rects.shape[1] != 5:
        raise ValueError(f"rects must be (k, 5): frame, x0, y0, x1, y1; got shape {rects.shape}")
    return rects


def box_histograms_host(frames, rects) -> np.ndarray:
    """The numpy twin of ``Engine.box_histograms``, and the CPU path: ``frames`` (n, h, w, 3) uint8 BGR, ``rects`` (k, 5) integers
    ``(frame, x0, y0, x1, y1)``, half-open -> (k, 512) uint32, row j counting the pixels of rectangle j per bin
    ``((B >> 5) << 6) | ((G >> 5) << 3) | (R >> 5)``.  A frame index outside the frames, and a rectangle that is empty or leaves the
    frame, is a ``ValueError``."""
    frames = np.asarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    rects = _rects(rects)
    out = np.zeros((len(rects), BINS), np.uint32)
    for j, (fi, x0, y0, x1, y1) in enumerate(rects.tolist()):
        if not 0 <= fi < n:
            raise ValueError(f"rectangle {j} names frame {fi}, outside [0, {n})")
        if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
            raise ValueError(f"rectangle {j} ({x0}, {y0}, {x1}, {y1}) is empty or leaves the {w} x {h} frame (x0, y0, x1, y1, half-open)")
        q = frames[fi, y0:y1, x0:x1].astype(np.int64) >> 5
        out[j] = np.bincount(((q[..., 0] << 6) | (q[..., 1] << 3) | q[..., 2]).ravel(), minlength=BINS)
    return out


def torso_rect(xyxy, h: int, w: int) -> Optional[tuple]:
    """The rectangle of a box that is sampled — the shirt, not the legs, the court or the neighbour — as half-open integers
    ``(x0, y0, x1, y1)``, or None where it is empty.  The integer box is ``X0 = floor(x0)``, ``Y0 = floor(y0)``, ``X1 = ceil(x1)``,
    ``Y1 = ceil(y1)``, clipped to the frame; with ``bw = X1 - X0`` and ``bh = Y1 - Y0`` the rectangle is
    ``[X0 + bw // 4, X1 - bw // 4) x [Y0 + bh // 8, Y0 + (5 * bh) // 8)``.  The fractions are parameters, not findings."""
    x0, y0, x1, y1 = (float(v) for v in xyxy)
    if not all(np.isfinite((x0, y0, x1, y1))):
        return None
    X0, Y0 = min(max(int(np.floor(x0)), 0), w), min(max(int(np.floor(y0)), 0), h)
    X1, Y1 = min(max(int(np.ceil(x1)), 0), w), min(max(int(np.ceil(y1)), 0), h)
    bw, bh = X1 - X0, Y1 - Y0
    if bw <= 0 or bh <= 0:
        return None
    rx0, rx1, ry0, ry1 = X0 + bw // 4, X1 - bw // 4, Y0 + bh // 8, Y0 + (5 * bh) // 8
    return (rx0, ry0, rx1, ry1) if rx0 < rx1 and ry0 < ry1 else None


@dataclass
class Track:
    """What ``scan`` knows of one ByteTrack id: ``frames`` — every position at which it has a box, ascending; ``hist`` — the summed
    histogram of its torso rectangles on the sampled positions; ``boxes`` — how many rectangles that sum holds."""
    frames: list = field(default_factory=list)
    hist: np.ndarray = field(default_factory=lambda: np.zeros(BINS, np.uint64))
    boxes: int = 0


def _runs(positions) -> list:
    """[(first index, source frame, count)] of the maximal runs of consecutive source frames in ``positions``."""
    out, i, n = [], 0, len(positions)
    while i < n:
        j = i + 1
        while j < n and positions[j] == positions[j - 1] + 1:
            j += 1
        out.append((i, int(positions[i]), j - i))
        i = j
    return out


def scan(source, players_results, every: int = 1, batch: int = 64, engine=None, positions=None, on_device: bool = True) -> dict:
    """``{bytetrack_id: Track}`` of a clip's stored player boxes.  ``players_results[i]`` — a ``Players`` (or None) — belongs to
    source frame ``positions[i]`` of ``source`` (anything ``video.get_video_frames_generator`` accepts; ``positions=None``: frame
    ``i``; the runner passes its ``source_index``, so that only kept frames are read).  Every box with an id counts towards its
    track's ``frames``; on every ``every``-th position its ``torso_rect`` gets a histogram, summed into the track's ``hist``.

    The clip is walked in batches of ``batch`` frames; the batches that hold a rectangle — the others are never handed to the walk,
    so they are not read, staged or converted — come through ``video.ResidentBatches``.  One ``Engine.box_histograms`` call per batch
    (one per ``MAX_RECTS`` rectangles of it).
    ``on_device=False`` runs ``box_histograms_host`` on host frames instead (no engine, no GPU) and gives the same numbers."""
    results = list(players_results)
    positions = np.arange(len(results), dtype=np.int64) if positions is None else np.asarray(positions, np.int64)
    if len(positions) < len(results):
        raise ValueError(f"scan: {len(results)} results but {len(positions)} positions")
    every, batch = max(1, int(every)), max(1, int(batch))
    info = video.VideoInfo.from_video_path(source)
    h, w = info.height, info.width
    tracks: dict = {}
    todo: list = []                    # (rectangles, their tracks) of the samples handed out and not yet summed

    def samples():
        for first, src, count in _runs(positions[:len(results)]):
            done = 0
            for sample in video.sampler(video.get_video_frames_generator(source, start=src, end=src + count), batch):
                rects, owners = [], []
                for k in range(len(sample)):
                    i = first + done + k
                    for p in results[i] or ():
                        if p.id is None:
                            continue
                        t = tracks.setdefault(int(p.id), Track())
                        t.frames.append(i)
                        r = torso_rect(p.xyxy, h, w) if i % every == 0 else None
                        if r is not None:
                            rects.append((k,) + r)
                            owners.append(t)
                done += len(sample)
                if rects:
                    todo.append((rects, owners))
                    yield sample
            if done != count:
                raise ValueError(f"scan: the source ends at frame {src + done}, the results go on to {src + count}")

    def add(hists) -> None:
        for t, row in zip(todo.pop()[1], hists):
            t.hist += row
            t.boxes += 1

    if not on_device:
        for sample in samples():
            host = [video.host_frame(f) for f in sample] if isinstance(sample[0], video.DeviceFrame) else video.host_batch(sample)
            add(box_histograms_host(np.asarray(host), todo[-1][0]))
        return tracks
    cap = MAX_RECTS                                  # what one call takes: a crowded batch goes in several
    with video.ResidentBatches(engine, samples(), batch, (h, w)) as walk:
        for frames, _ in walk:
            engine = engine or E.default_engine()
            buf, rects = video.device_batch(frames)[0], todo[-1][0]
            add(np.concatenate([engine.box_histograms(buf, len(frames), h, w, rects[lo:lo + cap]) for lo in range(0, len(rects), cap)]))
    return tracks


def distance(a, b) -> float:
    """Half the L1 distance of the two histograms normalised to sum 1, in float64: 0 for equal colour shares, 1 for disjoint ones.
    An empty histogram is at distance 1 from everything: no evidence is no match."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sa, sb = a.sum(), b.sum()
    if sa <= 0 or sb <= 0:
        return 1.0
    return float(0.5 * np.abs(a / sa - b / sb).sum())


def assign(tracks: dict, n_players: int = 4, max_distance: float = 0.5) -> tuple:
    """Relabel ByteTrack's tracks to ``n_players`` identities -> ``(mapping, distances)``: ``mapping[bytetrack_id]`` is the new id of
    every track, ``distances[bytetrack_id]`` the ``{identity: distance}`` of the candidates a track was decided among (seed tracks
    have none).  ``tracks``: ``{bytetrack_id: Track}`` as ``scan`` gives it.  The order of the dict does not matter.

    * Seed: the earliest frame in which exactly ``n_players`` ids are present.  Those ids become identities 1..n in ascending
      ByteTrack id — a run in which no track is ever lost keeps every id it has.
    * The other tracks are taken in order of their first frame, ties by ascending id.  The candidates are the identities none of
      whose member tracks shares a frame with the track; the nearest one (``distance``; ties: the lower identity) wins if its
      distance is at most ``max_distance``, and the track's counts are added to that identity's descriptor.  Otherwise the track
      is unassigned and gets ``n_players + 1``, ``+ 2``, ... in that order: never an identity's number, and
      ``analytics.DataAnalytics`` drops it as it drops any foreigner.
    * Without a seed frame nothing is relabelled (the mapping is the identity) and a warning says so.

    ``max_distance`` is a parameter, not a finding (see the module's docstring)."""
    n_players = int(n_players)
    ids = sorted(int(t) for t in tracks)
    frames = {t: set(int(f) for f in tracks[t].frames) for t in ids}
    present: dict = {}
    for t in ids:
        for f in frames[t]:
            present.setdefault(f, []).append(t)
    seed = next((f for f in sorted(present) if len(present[f]) == n_players), None)
    if seed is None:
        warnings.warn(f"identity.assign: no frame shows exactly {n_players} tracked players: nothing is relabelled", stacklevel=2)
        return {t: t for t in ids}, {}
    mapping, distances = {}, {}
    desc, taken = {}, {}                      # per identity: the summed histogram, the frames of its member tracks
    for k, t in enumerate(sorted(present[seed]), 1):
        mapping[t] = k
        desc[k] = np.asarray(tracks[t].hist, np.uint64).copy()
        taken[k] = set(frames[t])
    spare = n_players
    for t in sorted((t for t in ids if t not in mapping), key=lambda t: (min(frames[t]) if frames[t] else 0, t)):
        cand = {k: distance(tracks[t].hist, desc[k]) for k in sorted(desc) if not (taken[k] & frames[t])}
        distances[t] = cand
        best = min(cand, key=lambda k: (cand[k], k)) if cand else None
        if best is not None and cand[best] <= max_distance:
            mapping[t] = best
            desc[best] += np.asarray(tracks[t].hist, np.uint64)
            taken[best] |= frames[t]
        else:
            spare += 1
            mapping[t] = spare
    return mapping, distances


def relabel(players, mapping: dict):
    """A frame's ``Players`` with every id replaced by ``mapping[id]`` (an id the mapping does not know stays).  Rows, their order,
    confidences and the rule that id 0 reads as None are untouched; the box arrays are shared, not copied."""
    from .trackers.players_tracker import Player, Players
    if players is None:
        return None
    if players._players is None:                       # still arrays: stays lazy
        ids = players._ids
        if ids is not None:
            ids = np.array([mapping.get(int(t), int(t)) if t else 0 for t in np.asarray(ids).tolist()], np.asarray(ids).dtype).reshape(np.shape(ids))
        return Players(rows=players._rows, ids=ids)
    out = []
    for p in players._players:
        q = Player.from_row(p.xyxy, p.confidence, p.class_id, p._tid if p.id is None else mapping.get(p.id, p.id))
        q.projection = p.projection
        out.append(q)
    return Players(out)
