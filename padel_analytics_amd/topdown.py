"""The clip seen from above (``TrackingRunner(topdown=...)``): every frame warped through its court homography into a metric canvas of
the court, with the court's lines, the players and the ball drawn on it by the renderer.

* ``warp_host`` is the numpy twin of ``Engine.warp`` / ``pa_warp_perspective`` (csrc/warp.hip) and the CPU path: the readable statement
  of the rule include/padel_hip.h specifies — coordinates in float64, every operation rounded on its own, the cell and the weights
  from ``floor(32 s)`` in integers, the bilinear sum in integers, rounded half up.  The kernel equals it bit for bit.
* ``TopDownView`` holds the canvas: its size, the affine map ``A`` from the inset's drawn court (``ProjectedCourt.court_position``) onto
  the canvas's court, the matrix the kernel takes for a frame's homography, and the marks of a canvas frame.

The reference has no such view (its 2-D court is a drawing): no parity with it is claimed.  Bilinear only — no area filter, so the far
end of the court, which the warp minifies strongly, aliases; no lens distortion."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import engine as E, projected_court as PC, render as R


def warp_host(frames: np.ndarray, matrices, valid, oh: int, ow: int, fill=(0, 0, 0), out: Optional[np.ndarray] = None) -> np.ndarray:
    """``frames`` (n, h, w, 3) uint8 BGR -> (n, oh, ow, 3): frame i through ``matrices[i]`` (3 x 3, CANVAS pixel -> SOURCE pixel),
    ``fill`` (B, G, R) where ``valid[i]`` is 0, where the pixel falls behind the horizon (not Z > 0) or outside -1 < sx < w,
    -1 < sy < h, and for the taps of a border cell that lie outside the frame.  ``out``: an array to write into (it may not share
    memory with ``frames``).  ``ValueError`` with the library's words for what ``pa_warp_perspective`` refuses (``pa_warp_check``)."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
        raise ValueError("warp_host: frames must be (n, h, w, 3) uint8")
    frames = np.ascontiguousarray(frames)
    n, h, w = frames.shape[:3]
    oh, ow = int(oh), int(ow)
    matrices, valid = E._warp_args(n, matrices, valid)
    if out is None and n >= 1 and 1 <= oh <= E.WARP_MAX_DIM and 1 <= ow <= E.WARP_MAX_DIM:
        out = np.empty((n, oh, ow, 3), np.uint8)
    if out is not None and (out.dtype != np.uint8 or not out.flags.c_contiguous or out.size != n * oh * ow * 3):
        raise ValueError(f"warp_host: out must be a C-contiguous uint8 array of {n} x {oh} x {ow} x 3")
    # (an empty array has no address worth comparing: the refusals of n, h and w come before the pointers are looked at)
    why = E.warp_check(n, h, w, oh, ow, matrices, valid, src=frames.ctypes.data or 1, dst=(out.ctypes.data or 1 << 60) if out is not None else 1 << 60)
    if why is not None:
        raise ValueError(why)
    fw = E.fill_word(fill)
    fill3 = np.array([fw & 0xff, (fw >> 8) & 0xff, (fw >> 16) & 0xff], np.int32)
    res = out.reshape(n, oh, ow, 3)
    u = np.arange(ow, dtype=np.float64)[None, :]
    v = np.arange(oh, dtype=np.float64)[:, None]
    for i in range(n):
        if not valid[i]:
            res[i] = fill3
            continue
        m = matrices[9 * i:9 * i + 9]
        with np.errstate(all="ignore"):                      # 0 / 0, x / 0 and overflow give the NaN and infinities the comparisons refuse
            X = (m[0] * u + m[1] * v) + m[2]
            Y = (m[3] * u + m[4] * v) + m[5]
            Z = (m[6] * u + m[7] * v) + m[8]
            ok = Z > 0
            sx, sy = X / Z, Y / Z
            ok = ok & (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
        qx = np.floor(np.where(ok, sx, 0.0) * 32).astype(np.int32)      # never sx - floor(sx): that rounds to 1 for a tiny negative sx
        qy = np.floor(np.where(ok, sy, 0.0) * 32).astype(np.int32)
        x0, y0, wx, wy = qx >> 5, qy >> 5, (qx & 31)[..., None], (qy & 31)[..., None]
        P = np.empty((h + 2, w + 2, 3), np.int32)            # P(x, y) at [y + 1, x + 1]: the frame inside a border of fill
        P[:] = fill3
        P[1:-1, 1:-1] = frames[i]
        top = P[y0 + 1, x0 + 1] * (32 - wx) + P[y0 + 1, x0 + 2] * wx
        bot = P[y0 + 2, x0 + 1] * (32 - wx) + P[y0 + 2, x0 + 2] * wx
        val = (top * (32 - wy) + bot * wy + 512) >> 10
        res[i] = np.where(ok[..., None], val, fill3)
    return res


def _even(x: float) -> int:
    """The nearest even number (halves up)."""
    return 2 * int(np.floor(x / 2 + 0.5))


def _nearest(x: float) -> int:
    return int(np.floor(x + 0.5))


class TopDownView:
    """The metric canvas of the court for one clip.  ``projected_court``: the runner's ``ProjectedCourt`` — homographies take frame
    pixels into ITS drawn court (``court_position``), and ``A`` takes that rectangle onto the canvas's.

    ``px_per_m`` (canvas pixels per metre), ``margin_m`` (metres of floor shown around the court), ``fill`` (B, G, R of what the
    camera does not show) and the colours and sizes of the marks below are PARAMETERS, NOT FINDINGS: nothing was measured to choose
    them.  The canvas is (10 + 2 margin) px_per_m by (20 + 2 margin) px_per_m, each rounded to the nearest even number (the sinks
    take YUV 4:2:0), with the court centred; ``ValueError`` for a canvas the warp cannot make (a side outside 2 .. 4096)."""

    LINE_BGR, LINE_THICKNESS = (0, 0, 0), 2              # the inset's lines
    PLAYER_BGR, PLAYER_RADIUS, ID_SCALE = (255, 0, 0), 8, 2      # the inset's colour and radius for a player; the labels' scale
    BALL_BGR, BALL_RADIUS = (0, 255, 255), 6             # the ball as the inset draws it
    TEXT_BGR = (255, 255, 255)

    def __init__(self, projected_court, px_per_m: float = 48, margin_m: float = 1.5, fill=(40, 40, 40)):
        if not (px_per_m > 0 and margin_m >= 0):
            raise ValueError(f"topdown: px_per_m={px_per_m!r} must be positive and margin_m={margin_m!r} not negative")
        self.projected_court = projected_court
        self.px_per_m, self.margin_m = float(px_per_m), float(margin_m)
        self.fill = tuple(int(c) & 0xff for c in fill)
        self.w = _even((PC.BASE_LINE + 2 * self.margin_m) * self.px_per_m)
        self.h = _even((PC.SIDE_LINE + 2 * self.margin_m) * self.px_per_m)
        if not (2 <= self.w <= E.WARP_MAX_DIM and 2 <= self.h <= E.WARP_MAX_DIM):
            raise ValueError(f"topdown: px_per_m={px_per_m!r}, margin_m={margin_m!r} give a {self.w} x {self.h} canvas; each side must lie in "
                             f"[2, {E.WARP_MAX_DIM}]")
        cw, ch = PC.BASE_LINE * self.px_per_m, PC.SIDE_LINE * self.px_per_m
        left, top = (self.w - cw) / 2, (self.h - ch) / 2
        #: the canvas's court: (left, top, right, bottom) in canvas pixels
        self.court = (left, top, left + cw, top + ch)
        cp = projected_court.court_position
        (l, t), (r, b) = cp.top_left, cp.bottom_right
        ax, ay = cw / (r - l), ch / (b - t)
        #: affine, inset pixels -> canvas pixels
        self.A = np.array([[ax, 0.0, left - l * ax], [0.0, ay, top - t * ay], [0.0, 0.0, 1.0]])

    @property
    def size(self) -> tuple:
        """(width, height) of the canvas."""
        return self.w, self.h

    def canvas_from_frame(self, H: np.ndarray) -> np.ndarray:
        """Frame pixels -> canvas pixels: ``A @ H``, ``H`` the frame's homography into the drawn court."""
        return self.A @ np.asarray(H, np.float64)

    def frame_from_canvas(self, H: np.ndarray) -> np.ndarray:
        """Its inverse, canvas pixels -> frame pixels: the matrix ``Engine.warp`` / ``warp_host`` take for the frame."""
        return np.linalg.inv(self.canvas_from_frame(H))

    def matrices(self, projections) -> tuple:
        """One ``FrameProjection`` per frame -> (``matrices`` (n, 3, 3) float64, ``valid`` (n,) int32) for the warp: a frame without
        a homography, or with one that has no finite inverse, is not valid (its canvas is ``fill`` throughout)."""
        n = len(projections)
        m, valid = np.tile(np.eye(3), (n, 1, 1)), np.zeros(n, np.int32)
        for i, fp in enumerate(projections):
            if fp.H is None:
                continue
            try:
                inv = self.frame_from_canvas(fp.H)
            except np.linalg.LinAlgError:
                continue
            if np.isfinite(inv).all():
                m[i], valid[i] = inv, 1
        return m, valid

    def to_canvas(self, point, M: np.ndarray) -> Optional[tuple]:
        """``point`` through ``M`` (``project_point``: float64), rounded to the nearest canvas pixel; None where it has no finite image."""
        with np.errstate(all="ignore"):
            x, y = PC.ProjectedCourt.project_point(point, M)
        if not (np.isfinite(x) and np.isfinite(y)):
            return None
        return _nearest(x), _nearest(y)

    def court_marks(self) -> list:
        """The inset's 8 ``lines()`` through ``A``, drawn ON the warped picture: whether they fall on the floor's own lines is what
        the view is for."""
        marks = []
        for a, b in self.projected_court.court_keypoints.lines():
            pa, pb = self.to_canvas(a, self.A), self.to_canvas(b, self.A)
            marks.append(R.segment(*pa, *pb, self.LINE_THICKNESS, self.LINE_BGR))
        return marks

    def marks(self, frame_projection, players, ball) -> list:
        """The marks of one canvas frame.  With a homography: the court's lines; every one of the frame's ``players`` as a disc at
        its feet with the id beside it; the ``ball`` as a disc — feet and ball projected through ``A @ H`` in float64 and rounded to
        the nearest pixel THERE (not the inset's ``int()`` projections scaled up: those step by about 7 cm for a 1280-pixel clip).
        Without one: ``NO COURT`` in the top-left corner of a canvas that is ``fill`` throughout."""
        if frame_projection.H is None or not self.matrices([frame_projection])[1][0]:
            return R.text("NO COURT", 8, 8, self.ID_SCALE, self.TEXT_BGR)
        marks = self.court_marks()
        M = self.canvas_from_frame(frame_projection.H)
        for p in players or ():
            at = self.to_canvas(p.feet, M)
            if at is not None:
                marks.append(R.disc(*at, self.PLAYER_RADIUS, self.PLAYER_BGR))
                marks += R.text(str(p.id), at[0] + self.PLAYER_RADIUS + 4, at[1] - (R.GLYPH_H * self.ID_SCALE) // 2, self.ID_SCALE, self.PLAYER_BGR)
        if ball is not None:
            at = self.to_canvas(ball.asint(), M)
            if at is not None:
                marks.append(R.disc(*at, self.BALL_RADIUS, self.BALL_BGR))
        return marks
