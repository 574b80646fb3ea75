"""Where on the court each player spent the match (``TrackingRunner(heatmap=...)``): density maps on the metric canvas of ``topdown.py``.

* ``accumulate_host`` is the numpy twin of ``Engine.heat`` / ``pa_heat_accumulate`` (csrc/heat.hip) and the CPU path: the readable
  statement of the rule include/padel_hip.h specifies — all integer: an Epanechnikov bump ``(255 (r r - d2)) / (r r)`` per point,
  saturating sums, ``level = (D 255) / full``, the renderer's blend.  The kernel equals it bit for bit, canvases and state.
* ``heat_lut`` is the colour ramp, ``HeatMap`` the parameters of one clip's maps: the radius and the saturation in canvas units, the
  plane of each player id, the points of a frame.

The reference promises heat maps and computes none: no parity with it is claimed.  Out of scope: decay over time, maps of the ball or
of strokes, a colour per plane, normalisation by a running maximum in the clip, heat maps on the inset."""
from __future__ import annotations

import warnings
from typing import Optional

import numpy as np

from . import engine as E, topdown as T

#: the anchors of ``heat_lut``: (level, (B, G, R)) — PARAMETERS, NOT FINDINGS: a blue - cyan - green - yellow - red ramp, nothing measured
LUT_ANCHORS = ((0, (128, 0, 0)), (64, (255, 255, 0)), (128, (0, 255, 0)), (192, (0, 255, 255)), (255, (0, 0, 255)))


def heat_lut(anchors=LUT_ANCHORS) -> np.ndarray:
    """(256, 3) uint8 BGR: piecewise linear through ``anchors`` — ascending levels from 0 to 255 — in integers: between (l0, c0) and
    (l1, c1) level l is ``c0 + ((c1 - c0) (l - l0)) // (l1 - l0)``, floor division, so every anchor is hit exactly."""
    anchors = [(int(l), tuple(int(c) for c in bgr)) for l, bgr in anchors]
    levels = [l for l, _ in anchors]
    if levels[0] != 0 or levels[-1] != 255 or any(b <= a for a, b in zip(levels, levels[1:])) or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for _, c in anchors):
        raise ValueError("heat_lut: the anchors must run from level 0 to level 255 in ascending order, each with a (B, G, R) of bytes")
    lut = np.zeros((256, 3), np.uint8)
    for (l0, c0), (l1, c1) in zip(anchors, anchors[1:]):
        for l in range(l0, l1 + 1):
            lut[l] = [c0[k] + ((c1[k] - c0[k]) * (l - l0)) // (l1 - l0) for k in range(3)]
    return lut


def splat(r: int) -> np.ndarray:
    """(2 r - 1, 2 r - 1) uint32: what a point adds around itself, ``[r - 1, r - 1]`` its own pixel (255); 0 where d2 >= r r."""
    r = int(r)
    o = np.arange(-(r - 1), r, dtype=np.int64)
    d2 = o[:, None] ** 2 + o[None, :] ** 2
    return np.where(d2 < r * r, (255 * (r * r - d2)) // (r * r), 0).astype(np.uint32)


def _add_saturating(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.minimum(a.astype(np.uint64) + b.astype(np.uint64), 0xffffffff).astype(np.uint32)


def shown_density(state: np.ndarray, show_mask: int) -> np.ndarray:
    """The saturating sum of the planes of ``state`` whose bit is set in ``show_mask``."""
    d = np.zeros(state.shape[1:], np.uint32)
    for p in range(state.shape[0]):
        if (int(show_mask) >> p) & 1:
            d = _add_saturating(d, state[p])
    return d


def accumulate_host(canvases: Optional[np.ndarray], state: np.ndarray, points, first, valid, r: int, full: int, alpha: int, show_mask: int,
                    lut) -> np.ndarray:
    """``Engine.heat`` on the host, in place: frame by frame, the frame's ``points`` — (x, y, plane) triples, frame i owning
    ``points[first[i]:first[i + 1]]`` — are added to ``state`` ((planes, oh, ow) uint32, C-contiguous), then canvas i of ``canvases``
    ((n, oh, ow, 3) uint8 BGR, C-contiguous) is blended under the maps as they stand.  ``canvases`` None: the state alone (``n`` is
    ``len(first) - 1``) — what a run without a clip to show needs.  ``valid[i] == 0``: canvas i stays, and the frame may carry no
    point.  -> ``state``.  ``ValueError`` with the library's words for what ``pa_heat_accumulate`` refuses (``pa_heat_check``)."""
    if not (isinstance(state, np.ndarray) and state.ndim == 3 and state.dtype == np.uint32 and state.flags.c_contiguous and state.flags.writeable):
        raise ValueError("accumulate_host: state must be a writable C-contiguous (planes, oh, ow) uint32 array")
    planes, oh, ow = state.shape
    if canvases is not None:
        if not (isinstance(canvases, np.ndarray) and canvases.ndim == 4 and canvases.dtype == np.uint8 and canvases.flags.c_contiguous
                and canvases.shape[1:] == (oh, ow, 3)):
            raise ValueError(f"accumulate_host: canvases must be a C-contiguous (n, {oh}, {ow}, 3) uint8 array")
        n = canvases.shape[0]
    else:
        n = np.asarray(first).size - 1
    points, first, valid, lut = E._heat_args(n, points, first, valid, lut)
    # (an empty array has no address worth comparing; canvases None: an address just behind the state)
    at = (canvases.ctypes.data or 1) if canvases is not None else (state.ctypes.data or 1 << 59) + max(state.nbytes, 1)
    why = E.heat_check(n, oh, ow, planes, points, first, valid, r, full, alpha, show_mask, lut, canvas=at, state=state.ctypes.data or 1 << 59)
    if why is not None:
        raise ValueError(why)
    r, full, alpha = int(r), int(full), int(alpha)
    bump = splat(r)
    lut3 = lut.reshape(256, 3).astype(np.uint32)
    pts = points.reshape(-1, 3) if points is not None else np.zeros((0, 3), np.int32)
    for i in range(n):
        if not valid[i]:
            continue
        for x, y, p in pts[first[i]:first[i + 1]].tolist():
            # the bump covers columns x - r + 1 .. x + r - 1: cut to the canvas
            u0, u1, v0, v1 = max(x - r + 1, 0), min(x + r, ow), max(y - r + 1, 0), min(y + r, oh)
            if u0 < u1 and v0 < v1:
                part = bump[v0 - (y - r + 1):v1 - (y - r + 1), u0 - (x - r + 1):u1 - (x - r + 1)]
                state[p, v0:v1, u0:u1] = _add_saturating(state[p, v0:v1, u0:u1], part)
        if canvases is None or alpha == 0:
            continue
        d = shown_density(state, show_mask).astype(np.uint64)
        level = np.where(d >= full, 255, (d * 255) // full).astype(np.uint32)
        a = ((alpha * level) >> 8)[..., None]
        mixed = (canvases[i].astype(np.uint32) * (256 - a) + lut3[level] * a + 128) >> 8
        canvases[i] = np.where(a > 0, mixed, canvases[i]).astype(np.uint8)
    return state


class HeatMap:
    """The density maps of one clip on the canvas of ``view`` (a ``topdown.TopDownView``).

    ``radius_m`` (the splat's radius in metres), ``saturate_s`` (seconds a player must stand still for a pixel to reach the top of the
    ramp), ``alpha`` (the weight, of 256, of the ramp's top over the picture), the ramp itself (``heat_lut``) and ``ids`` are
    PARAMETERS, NOT FINDINGS: nothing was measured to choose them.  ``r = round(radius_m * px_per_m)`` canvas pixels;
    ``full = 255 * round(saturate_s * fps)``: the density under the feet of a player who stood still for that long.  The plane of a
    player is the position of its id in ``ids`` (1 .. 4 planes; other ids are dropped); ``show``: the ids whose planes are summed for
    display (None: all).  ``ValueError`` for values the kernel refuses."""

    def __init__(self, view: T.TopDownView, radius_m: float = 0.5, saturate_s: float = 20.0, *, fps: float, alpha: int = 160,
                 ids=(1, 2, 3, 4), show=None):
        self.view = view
        self.ids = tuple(int(i) for i in ids)
        self.planes = len(self.ids)
        if not 1 <= self.planes <= E.HEAT_MAX_PLANES or len(set(self.ids)) != self.planes:
            raise ValueError(f"heatmap: ids={ids!r}: 1 to {E.HEAT_MAX_PLANES} different player ids")
        self.r = T._nearest(float(radius_m) * view.px_per_m)
        if not 1 <= self.r <= E.HEAT_MAX_RADIUS:
            raise ValueError(f"heatmap: radius_m={radius_m!r} at {view.px_per_m} pixels per metre is {self.r} pixels; the radius must lie in "
                             f"[1, {E.HEAT_MAX_RADIUS}]")
        self.full = 255 * T._nearest(float(saturate_s) * float(fps))
        if not 1 <= self.full <= E.HEAT_MAX_FULL:
            raise ValueError(f"heatmap: saturate_s={saturate_s!r} at {fps} frames per second gives full = {self.full}; it must lie in "
                             f"[1, {E.HEAT_MAX_FULL}]")
        if isinstance(alpha, bool) or int(alpha) != alpha or not 0 <= int(alpha) <= 256:
            raise ValueError(f"heatmap: alpha={alpha!r}: an integer in [0, 256]")
        self.alpha = int(alpha)
        shown = self.ids if show is None else tuple(int(i) for i in show)
        if not shown or any(i not in self.ids for i in shown):
            raise ValueError(f"heatmap: show={show!r}: at least one of the ids {self.ids}")
        self.show_mask = sum(1 << self.ids.index(i) for i in set(shown))
        self.lut = heat_lut()
        self._warned = False

    def state(self) -> np.ndarray:
        """The maps at the start: (planes, h, w) uint32 of zeros."""
        return np.zeros((self.planes, self.view.h, self.view.w), np.uint32)

    def points(self, frame_projection, players) -> list:
        """[(x, y, plane)] of one frame: the feet of the ``players`` whose id is in ``ids``, through ``A @ H`` in float64 and rounded
        as ``TopDownView.to_canvas`` rounds them (the disc the top-down clip draws has the same centre).  Empty without a valid
        homography; points whose bump misses the canvas are dropped; the first ``engine.HEAT_MAX_POINTS`` are kept (one warning)."""
        view = self.view
        if frame_projection.H is None or not view.matrices([frame_projection])[1][0]:
            return []
        M = view.canvas_from_frame(frame_projection.H)
        out = []
        for p in players or ():
            if int(p.id) not in self.ids:
                continue
            at = view.to_canvas(p.feet, M)
            if at is None:
                continue
            x, y = at
            if x + self.r <= 0 or x - self.r >= view.w - 1 or y + self.r <= 0 or y - self.r >= view.h - 1:
                continue
            out.append((x, y, self.ids.index(int(p.id))))
        if len(out) > E.HEAT_MAX_POINTS:
            if not self._warned:
                self._warned = True
                warnings.warn(f"heatmap: a frame has {len(out)} players' feet, the first {E.HEAT_MAX_POINTS} are taken")
            out = out[:E.HEAT_MAX_POINTS]
        return out

    def batch(self, projections, players) -> tuple:
        """One ``FrameProjection`` and one ``Players`` (or None) per frame -> (``points`` (k, 3) int32, ``first`` (n + 1,) int32, ``valid``
        (n,) int32) for ``Engine.heat`` / ``accumulate_host``; ``valid`` is the warp's (``TopDownView.matrices``)."""
        first = np.zeros(len(projections) + 1, np.int32)
        flat: list = []
        for i, (fp, pl) in enumerate(zip(projections, players)):
            flat += self.points(fp, pl)
            first[i + 1] = len(flat)
        return np.array(flat, np.int32).reshape(-1, 3), first, self.view.matrices(projections)[1]

    def call(self, overlay: bool = True) -> dict:
        """The keyword arguments of ``Engine.heat`` / ``accumulate_host`` that do not change from batch to batch."""
        return dict(r=self.r, full=self.full, alpha=self.alpha if overlay else 0, show_mask=self.show_mask, lut=self.lut)

    def picture_full(self, state: np.ndarray) -> int:
        """``full`` of the still picture: the largest shown density of ``state``, 1 for maps that are zero throughout, and at most
        ``engine.HEAT_MAX_FULL`` (a pixel beyond that — a player who did not move for half an hour — shows level 255 like it)."""
        return int(min(max(int(shown_density(state, self.show_mask).max()), 1), E.HEAT_MAX_FULL))

    def save(self, path, state: np.ndarray, quality: int = 90, eng=None, canvas=None, state_dev=None) -> None:
        """``state`` into the file ``path`` names.  ``.npy``: the array.  ``.jpg``: a ``fill`` canvas under the maps at ``full`` = their
        largest density (``picture_full``), the court's lines on it, as full-range BT.601 YUV 4:2:0 through the JPEG encoder — with
        ``eng`` on the device (``canvas``: a buffer of one canvas at least, ``state_dev``: the maps there), else by the numpy twins;
        the same bytes either way."""
        from . import mjpeg, render as R, video
        view = self.view
        if str(path).lower().endswith(".npy"):
            with open(path, "wb") as fh:                     # (a handle: np.save would add a second suffix to "MAPS.NPY")
                np.save(fh, state)
            return
        h, w = view.h, view.w
        desc, enc = video.yuv_desc(w, h, "i420", "bt601", "full"), video.YUV_ENC_COEFFS["bt601_full"]
        blank = np.empty((1, h, w, 3), np.uint8)
        blank[:] = view.fill
        call = dict(self.call(), full=self.picture_full(state))
        nothing = (np.zeros((0, 3), np.int32), np.zeros(2, np.int32), np.ones(1, np.int32))
        marks, first = R.pack([view.court_marks()])
        if eng is None:
            accumulate_host(blank, state, *nothing, **call)
            raw = R.render_host(blank, marks, first, E.RENDER_YUV420, desc, enc).reshape(-1)
            data, _ = mjpeg.encode_host(raw, 1, h, w, desc, quality)
        else:
            yuv = eng.alloc(video.yuv_span(1, h, w, desc))
            try:
                canvas.upload(blank)
                eng.heat(canvas, 1, h, w, state_dev, self.planes, *nothing, **call)
                eng.render(canvas, 1, h, w, marks, first, yuv, out=E.RENDER_YUV420, geom=desc, enc=enc)
                data, _ = eng.jpeg_encode(yuv, 1, h, w, desc, quality)
            finally:
                eng.synchronize()
                yuv.free()
        with open(path, "wb") as fh:
            fh.write(np.asarray(data, np.uint8).tobytes())
