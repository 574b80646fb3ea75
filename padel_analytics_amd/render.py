"""Marks for the renderer (``Engine.render`` / ``pa_render``, csrc/render.hip) and its numpy twin.

A mark is one record of ``engine.MARK_DTYPE`` — kind, x0, y0, x1, y1, size, bgr, arg — built here by ``disc``, ``segment``,
``box``, ``fill``, ``blend``, ``arc`` and ``text``; ``pack`` turns one list of marks per frame into the (``marks``, ``first``) pair the engine takes.
``render_host`` applies them with numpy: the CPU path, and the readable statement of the integer coverage rules that
include/padel_hip.h specifies (``pa_mark``) — marks applied in list order, a later mark overwriting an earlier one, or, for the
one kind that is not opaque (``blend``), mixing its colour into what the earlier ones left.  ``render_host(scale=2 | 3 | 4)`` and
``downscale_host`` state the scaled pass (``pa_render_scaled``): drawn at full size, then the rounded mean of every s x s block.
Parity with cv2 / supervision drawing is not pinned (neither is installed); these rules are the specification."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import engine as E, video

COORD_MIN, COORD_MAX = -8192, 8191
GLYPH_W, GLYPH_H, GLYPH_ADVANCE = 5, 7, 6
ARC_MAX_AXIS = 4095                                  # an arc's semi-axis: 1..4095
FONT_CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ :.-"


def _c(v) -> int:
    """A coordinate as the engine takes it: an integer, clipped to the range a mark may carry (a point that far outside an at most
    8192 x 8192 frame is invisible either way; a segment ending there changes its slope, not whether it is drawn)."""
    return min(max(int(v), COORD_MIN), COORD_MAX)


def _bgr(bgr) -> int:
    if isinstance(bgr, (tuple, list)):
        b, g, r = (int(c) & 0xff for c in bgr)
        return b | g << 8 | r << 16
    return int(bgr) & 0xffffff


def disc(x, y, r: int, bgr) -> tuple:
    return (E.MARK_DISC, _c(x), _c(y), 0, 0, int(r), _bgr(bgr), 0)


def segment(x0, y0, x1, y1, t: int, bgr) -> tuple:
    return (E.MARK_SEGMENT, _c(x0), _c(y0), _c(x1), _c(y1), int(t), _bgr(bgr), 0)


def fill(x0, y0, x1, y1, bgr) -> tuple:
    return (E.MARK_FILL, _c(x0), _c(y0), _c(x1), _c(y1), 0, _bgr(bgr), 0)


def blend(x0, y0, x1, y1, bgr, weight: int) -> tuple:
    """The rectangle of ``fill`` with ``bgr`` mixed in at ``weight`` / 256, ``weight`` in 1..255 (128 over white: cv2's ``addWeighted``
    at 0.5): per channel ``(p * (256 - weight) + c * weight + 128) >> 8``."""
    return (E.MARK_BLEND, _c(x0), _c(y0), _c(x1), _c(y1), 0, _bgr(bgr), int(weight))


def box(x0, y0, x1, y1, t: int, bgr) -> tuple:
    return (E.MARK_BOX, _c(x0), _c(y0), _c(x1), _c(y1), int(t), _bgr(bgr), 0)


def arc(x, y, a: int, b: int, t: int, bgr, mask: int = 0xFF) -> tuple:
    """An axis-parallel elliptical ring cut to octants: centre (x, y), OUTER semi-axes ``a``, ``b`` in 1..4095, thickness ``t`` in
    1..255 growing inwards, opaque.  Bit k of ``mask`` (1..255) keeps octant k: the parameter angle [45 k, 45 (k + 1)) degrees, 0 at
    +x, y pointing down (so octants 0..3 are the lower half of the ring on the screen, 0xFF the whole ring)."""
    return (E.MARK_ARC, _c(x), _c(y), int(a), int(b), int(t), _bgr(bgr), int(mask))


def glyph(ch: str, x, y, scale: int, bgr) -> tuple:
    return (E.MARK_GLYPH, _c(x), _c(y), 0, 0, int(scale), _bgr(bgr), ord(ch))


def text(s: str, x, y, scale: int, bgr) -> list:
    """One glyph mark per character of ``s`` (upper-cased), the first cell's top-left at (x, y), advancing 6 * scale pixels per
    character.  ``ValueError`` for a character the font does not have (``FONT_CHARS``)."""
    s = str(s).upper()
    for ch in s:
        if ch not in FONT_CHARS:
            raise ValueError(f"text {s!r}: the renderer's font has no {ch!r} (render.FONT_CHARS: {FONT_CHARS!r})")
    k = int(scale)
    return [glyph(ch, int(x) + i * GLYPH_ADVANCE * k, y, k, bgr) for i, ch in enumerate(s)]


def text_width(s: str, scale: int) -> int:
    """Pixels from the first glyph's left edge to the last one's right edge."""
    return max(0, len(str(s)) * GLYPH_ADVANCE - 1) * int(scale)


def pack(per_frame: Sequence[Sequence[tuple]]) -> tuple:
    """One list of marks per frame -> (``marks``: array of ``engine.MARK_DTYPE``, ``first``: (n + 1,) int32) for ``Engine.render`` /
    ``render_host``: frame i owns ``marks[first[i]:first[i + 1]]``."""
    first = np.zeros(len(per_frame) + 1, np.int32)
    flat: list = []
    for i, ms in enumerate(per_frame):
        flat.extend(ms)
        first[i + 1] = len(flat)
    marks = np.array([tuple(m) for m in flat], E.MARK_DTYPE) if flat else np.zeros(0, E.MARK_DTYPE)
    return marks, first


_FONT_CACHE: dict = {}


def _glyph_bits(code: int) -> np.ndarray:
    """(7, 5) bool bitmap of one glyph, from the library's font (``pa_glyph_rows``: the font lives there, once)."""
    if code not in _FONT_CACHE:
        rows = E.glyph_rows(code)
        if rows is None:
            raise ValueError(f"the renderer's font has no character code {code}")
        _FONT_CACHE[code] = ((rows[:, None] >> np.arange(GLYPH_W)[None, :]) & 1).astype(bool)
    return _FONT_CACHE[code]


def _arc_rule(dx, dy, a: int, b: int, t: int, mask: int):
    """PA_MARK_ARC on int64 offsets from the centre (broadcast against each other), as include/padel_hip.h words it."""
    def inside(X, Y, A, B):
        return X * X * (B * B) + Y * Y * (A * A) <= A * A * B * B

    outer = inside(dx, dy, a, b)
    hole = np.full(outer.shape, True) if (a - t < 1 or b - t < 1) else ~inside(dx, dy, a - t, b - t)
    rim = ~(inside(dx + 1, dy, a, b) & inside(dx - 1, dy, a, b) & inside(dx, dy + 1, a, b) & inside(dx, dy - 1, a, b))
    u, v = np.broadcast_arrays(dx * b, dy * a)
    octant = np.zeros(outer.shape, bool)
    for k in range(4):                                   # (u, v) after k turns (u, v) -> (v, -u)
        if mask >> (2 * k) & 1:
            octant |= (u > 0) & (v >= 0) & (v < u)
        if mask >> (2 * k + 1) & 1:
            octant |= (u > 0) & (v >= u)
        u, v = v, -u
    if mask & 1:
        octant |= (u == 0) & (v == 0)                    # the centre pixel counts as octant 0
    return outer & (hole | rim) & octant


def coverage(mark, h: int, w: int) -> tuple:
    """-> (y0, x0, mask): the pixels of an ``h`` x ``w`` frame that ``mark`` covers are ``mask`` (bool) placed at row ``y0``, column
    ``x0``; None when the mark's bounding box misses the frame.  All int64, the rules of include/padel_hip.h as they stand there."""
    kind, x0, y0, x1, y1, size, _, arg = (int(v) for v in mark)
    if kind == E.MARK_DISC:
        bb = (x0 - size, y0 - size, x0 + size, y0 + size)
    elif kind == E.MARK_SEGMENT:
        e = size // 2
        bb = (min(x0, x1) - e, min(y0, y1) - e, max(x0, x1) + e, max(y0, y1) + e)
    elif kind in (E.MARK_FILL, E.MARK_BOX, E.MARK_BLEND):
        bb = (min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1))
    elif kind == E.MARK_GLYPH:
        bb = (x0, y0, x0 + GLYPH_W * size - 1, y0 + GLYPH_H * size - 1)
    elif kind == E.MARK_ARC:
        bb = (x0 - x1, y0 - y1, x0 + x1, y0 + y1)
    else:
        raise ValueError(f"unknown mark kind {kind}")
    ax, ay, bx, by = max(bb[0], 0), max(bb[1], 0), min(bb[2], w - 1), min(bb[3], h - 1)
    if ax > bx or ay > by:
        return None
    x = np.arange(ax, bx + 1, dtype=np.int64)[None, :]
    y = np.arange(ay, by + 1, dtype=np.int64)[:, None]
    if kind == E.MARK_DISC:
        m = (x - x0) ** 2 + (y - y0) ** 2 <= size * size + size
    elif kind == E.MARK_SEGMENT:
        dx, dy, px, py, t2 = x1 - x0, y1 - y0, x - x0, y - y0, size * size
        L2 = dx * dx + dy * dy
        s = px * dx + py * dy
        near0 = 4 * (px * px + py * py) <= t2
        near1 = 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= t2
        cross = px * dy - py * dx
        m = np.where((L2 == 0) | (s <= 0), near0, np.where(s >= L2, near1, 4 * cross * cross <= t2 * L2))
    elif kind in (E.MARK_FILL, E.MARK_BLEND):
        m = np.ones((by - ay + 1, bx - ax + 1), bool)
    elif kind == E.MARK_BOX:
        inner = (x >= bb[0] + size) & (x <= bb[2] - size) & (y >= bb[1] + size) & (y <= bb[3] - size)
        m = ~inner
    elif kind == E.MARK_ARC:
        m = _arc_rule(x - x0, y - y0, x1, y1, size, arg)
    else:
        m = _glyph_bits(arg)[(y - y0) // size, (x - x0) // size]
    return ay, ax, np.broadcast_to(m, (by - ay + 1, bx - ax + 1))


def draw_host(frame: np.ndarray, marks) -> np.ndarray:
    """Apply ``marks`` (records or tuples) to one (h, w, 3) uint8 BGR frame in place, in list order."""
    h, w = frame.shape[:2]
    for mk in marks:
        c = coverage(mk, h, w)
        if c is None:
            continue
        y0, x0, m = c
        bgr = int(mk[6])
        c = np.array([bgr & 0xff, (bgr >> 8) & 0xff, (bgr >> 16) & 0xff], np.int64)
        region = frame[y0:y0 + m.shape[0], x0:x0 + m.shape[1]]
        if int(mk[0]) == E.MARK_BLEND:
            a = int(mk[7])
            region[m] = ((region[m].astype(np.int64) * (256 - a) + c * a + 128) >> 8).astype(np.uint8)
        else:
            region[m] = c.astype(np.uint8)
    return frame


RENDER_SCALES = (1, 2, 3, 4)                          # what ``scale=`` may be (``pa_render_scaled``)


def downscale_host(frames: np.ndarray, s: int) -> np.ndarray:
    """(n, h, w, 3) uint8 -> (n, h // s, w // s, 3): every output channel the rounded mean of its ``s`` x ``s`` block,
    ``(sum + s * s // 2) // (s * s)`` in integers (include/padel_hip.h, ``pa_render_scaled``; halves round up).  ``ValueError`` for an
    ``s`` outside 1..4 or a size that is no multiple of it."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
        raise ValueError("downscale_host: frames must be (n, h, w, 3) uint8")
    s = int(s)
    n, h, w = frames.shape[:3]
    if s not in RENDER_SCALES:
        raise ValueError(f"downscale_host: scale {s} outside [1, 4]")
    if h % s or w % s:
        raise ValueError(f"downscale_host: {w} x {h} frames are no multiple of scale {s} each way")
    sums = frames.reshape(n, h // s, s, w // s, s, 3).astype(np.int64).sum(axis=(2, 4))
    return ((sums + (s * s) // 2) // (s * s)).astype(np.uint8)


def render_host(frames: np.ndarray, marks, first, out: int = E.RENDER_BGR, geom=None, enc=None, dst: Optional[np.ndarray] = None,
                scale: int = 1) -> np.ndarray:
    """The numpy twin of ``Engine.render``: ``frames`` (n, h, w, 3) uint8 BGR with frame i's ``marks[first[i]:first[i + 1]]`` drawn on
    it -> a new (n, h, w, 3) array (``out=RENDER_BGR``) or the 1-D byte array of the frames as YUV 4:2:0 laid out by ``geom`` and
    encoded with ``enc`` (``out=RENDER_YUV420``; bytes between planes and rows stay as ``dst`` has them).  ``scale`` 2, 3, 4: drawn at
    full size, then ``downscale_host``, then encoded — ``geom`` describes the ``h // scale`` x ``w // scale`` output.  ``ValueError``
    for what the engine refuses (``pa_render_check`` / ``pa_render_scaled_check``)."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
        raise ValueError("render_host: frames must be (n, h, w, 3) uint8")
    n, h, w = frames.shape[:3]
    why = E.render_check(n, h, w, marks, first, out, geom, enc, scale=scale)
    if why is not None:
        raise ValueError(why)
    marks = np.ascontiguousarray(marks, E.MARK_DTYPE).reshape(-1)
    drawn = frames.copy()
    for i in range(n):
        draw_host(drawn[i], marks[int(first[i]):int(first[i + 1])])
    if int(scale) != 1:
        drawn = downscale_host(drawn, scale)
    if out == E.RENDER_BGR:
        return drawn
    enc = tuple(int(getattr(enc, f)) for f, _ in E.pa_yuv_enc._fields_) if isinstance(enc, E.pa_yuv_enc) else tuple(int(c) for c in enc)
    return video.bgr_to_yuv420_host(drawn, geom, enc, out=dst)
