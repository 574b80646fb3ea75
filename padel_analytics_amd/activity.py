"""Court-view filter: which frames of a broadcast clip show the court camera?

The reference leaves this open (``main.py:122``: ``# FILTER FRAMES OF INTEREST (TODO)``).  A replay, a close-up or a graphic differs
from the court camera's picture almost everywhere; a rally differs from it where the players and the ball are.  So each frame is
compared, in luma, with a reference image of the empty court (by default the per-pixel median of frames spread over the clip), and
the share of pixels that changed decides.  The statistic is one streaming reduction over bytes that are in HBM anyway
(``csrc/frame_activity.hip``, ``Engine.frame_activity``); its specification is ``include/padel_hip.h`` and its executable form
``frame_activity_host`` below.  All integer, so the GPU and the twin agree exactly.

``scan`` computes the statistic for a whole clip, ``court_view_mask`` turns it into a decision per frame, ``segments`` into runs of
kept frames — what ``TrackingRunner(segments=...)`` takes.

The defaults ``tau = 24``, ``max_changed = 0.35``, ``max_gap = fps // 2`` and ``min_keep = 2 * fps`` are parameters, not findings:
the project has no real footage to set them by, and they were not tuned against synthetic clips.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import engine as E, video


def luma(bgr: np.ndarray) -> np.ndarray:
    """``Y = (29 B + 150 G + 77 R + 128) >> 8`` of (..., 3) uint8 BGR -> (...) int64."""
    p = np.asarray(bgr).astype(np.int64)
    return (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8


def _roi(roi, h: int, w: int) -> tuple:
    if roi is None:
        return 0, 0, w, h
    x0, y0, x1, y1 = (int(v) for v in roi)
    if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
        raise ValueError(f"roi ({x0}, {y0}, {x1}, {y1}) is empty or leaves the {w} x {h} frame (x0, y0, x1, y1, half-open)")
    return x0, y0, x1, y1


def frame_activity_host(frames, ref, prev=None, roi=None, tau: int = 24) -> np.ndarray:
    """The numpy twin of ``Engine.frame_activity``: ``frames`` (n, h, w, 3) uint8 BGR, ``ref`` (h, w, 3), ``prev`` (h, w, 3) or None
    -> (n, 3) uint64 ``[sad_ref, changed, sad_prev]`` per frame over the half-open ``roi = (x0, y0, x1, y1)`` (None: everything):

    * ``sad_ref[i]  = sum |Y(f_i) - Y(ref)|``
    * ``changed[i]  = #{ |Y(f_i) - Y(ref)| > tau }`` (strict)
    * ``sad_prev[i] = sum |Y(f_i) - Y(f_{i-1})|``, ``f_{-1} = prev``; without ``prev``, ``sad_prev[0] = 0``."""
    frames = np.asarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    if not 0 <= int(tau) <= 255:
        raise ValueError(f"tau = {tau} outside [0, 255]")
    x0, y0, x1, y1 = _roi(roi, h, w)
    cut = lambda a: luma(np.asarray(a, np.uint8)[..., y0:y1, x0:x1, :])
    yf, yr = cut(frames), cut(ref)
    out = np.zeros((n, 3), np.uint64)
    d = np.abs(yf - yr[None])
    out[:, 0] = d.sum(axis=(1, 2))
    out[:, 1] = (d > int(tau)).sum(axis=(1, 2))
    if n > 1:
        out[1:, 2] = np.abs(yf[1:] - yf[:-1]).sum(axis=(1, 2))
    if prev is not None and n:
        out[0, 2] = np.abs(yf[0] - cut(prev)).sum()
    return out


@dataclass
class FrameActivity:
    """The statistic of a clip's frames, one entry per frame, and the number of pixels each was summed over."""
    sad_ref: np.ndarray
    changed: np.ndarray
    sad_prev: np.ndarray
    npix: int

    def __len__(self) -> int:
        return len(self.changed)


def reference_frame(source, samples: int = 64, engine=None, start: int = 0, end: Optional[int] = None) -> np.ndarray:
    """(h, w, 3) uint8 BGR: the per-pixel median (``Engine.frames_median``: ``np.median(...).astype(uint8)``) of the frames at
    indices ``start + k * total // samples``, k = 0 .. samples - 1, of the ``total`` frames of ``source`` in [start, end).

    A median is the court only if the court camera holds more than half of the sampled frames.  If more than half of them are
    cutaways this is NOT the court, and every later decision is made against the wrong picture: callers who know better pass their
    own ``ref`` to ``scan`` (a frame they picked, a median over a range they trust)."""
    info = video.VideoInfo.from_video_path(source)
    stop = info.total_frames if end is None else min(int(end), info.total_frames)
    total = stop - int(start)
    if total < 1 or samples < 1:
        raise ValueError(f"reference_frame: no frames in [{start}, {stop}) or samples = {samples}")
    idx = sorted({int(start) + k * total // int(samples) for k in range(int(samples))})
    frames = []
    for i in idx:
        frames += [video.host_frame(f) for f in video.get_video_frames_generator(source, start=i, end=i + 1)]
    stack = np.stack(frames)
    eng = engine or E.default_engine()
    n, h, w = stack.shape[:3]
    src = eng.alloc(stack.nbytes)
    med = None
    try:
        src.upload(stack)
        med = eng.frames_median(src, n, h, w)
        return med.download(np.empty((h, w, 3), np.uint8))
    finally:
        src.free()
        if med is not None:
            med.free()


def _follows(a, b) -> bool:
    """Frame handle ``b`` is the stored frame behind ``a`` in the same device-resident clip."""
    return (type(a) is type(b) and isinstance(a, (video.DeviceFrame, video.YuvFrame)) and a.clip is b.clip and b.index == a.index + 1
            and getattr(a.clip, "on_device", True))


def scan(source, ref=None, roi=None, tau: int = 24, batch: int = 64, engine=None, start: int = 0, end: Optional[int] = None) -> FrameActivity:
    """``frame_activity`` of every frame of ``source`` in [start, end) — anything ``video.get_video_frames_generator`` accepts —
    against ``ref`` ((h, w, 3) uint8 BGR; None: ``reference_frame(source)`` over the same range), ``batch`` frames per call.

    The frames come through ``video.ResidentBatches``.  A batch finds its predecessor either as the stored frame in front of it —
    then it is asked for as part of the batch — or in slot 0 of the walk's staging clip (host frames, a device clip that
    repeats).  ``sad_prev`` is therefore continuous over the clip (0 for its first frame)."""
    eng = engine or E.default_engine()
    info = video.VideoInfo.from_video_path(source)
    h, w = info.height, info.width
    fb = h * w * 3
    x0, y0, x1, y1 = _roi(roi, h, w)
    if ref is None:
        ref = reference_frame(source, engine=eng, start=start, end=end)
    ref = np.ascontiguousarray(ref, np.uint8)
    if ref.shape != (h, w, 3):
        raise ValueError(f"ref has shape {ref.shape}, the clip's frames are {(h, w, 3)}")
    batch = max(1, int(batch))
    rows, laps, carry = [], [], None

    def samples():
        """The batches; one whose predecessor is the stored frame in front of it starts with that frame (``laps``: 1 for those),
        so that a YUV or Motion-JPEG clip converts the two as one range."""
        last = None
        for sample in video.sampler(video.get_video_frames_generator(source, start=start, end=end), batch):
            laps.append(int(last is not None and _follows(last, sample[0])))
            yield [last] + sample if laps[-1] else sample
            last = sample[-1]

    d_ref = eng.alloc(fb).upload(ref)
    try:
        with video.ResidentBatches(eng, samples(), batch + 1, (h, w), lead=1) as walk:
            for frames, host in walk:
                lap = laps.pop()
                n = len(frames) - lap
                buf = video.device_batch(frames)[0]
                prev = buf.view(0, fb) if lap else None
                if carry is not None and not lap:        # host frames, a clip that repeats: the predecessor goes to slot 0
                    stage = walk.staging()
                    stage.upload(video.host_frame(carry)[None], first=0, copy_stream=False)
                    prev = stage.buffer.view(0, fb)
                rows.append(eng.frame_activity(buf.view(lap * fb, n * fb), n, h, w, d_ref, prev=prev, roi=roi, tau=tau))
                carry = frames[-1] if host is None else np.array(host[-1])
    finally:
        eng.synchronize()
        d_ref.free()
    a = np.concatenate(rows) if rows else np.zeros((0, 3), np.uint64)
    return FrameActivity(sad_ref=a[:, 0].copy(), changed=a[:, 1].copy(), sad_prev=a[:, 2].copy(), npix=(x1 - x0) * (y1 - y0))


def _runs(mask: np.ndarray) -> list:
    """[(lo, hi, value)] of the maximal constant runs of a bool array."""
    out, n, lo = [], len(mask), 0
    for i in range(1, n + 1):
        if i == n or mask[i] != mask[lo]:
            out.append((lo, i, bool(mask[lo])))
            lo = i
    return out if n else []


def court_view_mask(act: FrameActivity, max_changed: float = 0.35, max_gap: Optional[int] = None, min_keep: Optional[int] = None,
                    fps: int = 30) -> np.ndarray:
    """bool[n]: True where the frame counts as court view.  In this order:

    1. ``changed[i] <= max_changed * npix``;
    2. runs of False of at most ``max_gap`` frames (default ``fps // 2``) that lie between two True runs become True (a flash, a
       wipe, a player close to the camera);
    3. runs of True shorter than ``min_keep`` frames (default ``2 * fps``) become False (too short for a rally).

    The defaults are parameters, not findings (see the module's docstring)."""
    max_gap = int(fps) // 2 if max_gap is None else int(max_gap)
    min_keep = 2 * int(fps) if min_keep is None else int(min_keep)
    mask = np.asarray(act.changed).astype(np.float64) <= float(max_changed) * float(act.npix)
    runs = _runs(mask)
    for k, (lo, hi, v) in enumerate(runs):
        if not v and hi - lo <= max_gap and 0 < k < len(runs) - 1:
            mask[lo:hi] = True
    for lo, hi, v in _runs(mask):
        if v and hi - lo < min_keep:
            mask[lo:hi] = False
    return mask


def segments(mask) -> list:
    """The True runs of ``mask`` as half-open ``(lo, hi)`` pairs, ascending."""
    return [(lo, hi) for lo, hi, v in _runs(np.asarray(mask, bool)) if v]
