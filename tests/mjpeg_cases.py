"""The frames the Motion-JPEG tests encode (tests/test_mjpeg_host.py on the CPU, tests/test_gpu_mjpeg.py on the GPU): five sizes, two
layouts with padding everywhere, seven contents."""
import functools

import numpy as np

from padel_analytics_amd import mjpeg, video

#: (w, h): one MCU; the smallest frame; partial MCUs on both edges; nine intervals (RSTm wraps past 7); one interval at full width
SIZES = [(16, 16), (2, 2), (34, 18), (16, 144), (1280, 16)]
LAYOUTS = ["i420", "nv12"]
#: name -> JPEG quality
CONTENTS = {"grey": 90, "zeros": 90, "ones": 90, "ramp": 90, "basis63": 90, "noise_q100": 100, "noise_q1": 1}


def geometry(w, h, layout):
    """``pitch > w``, a padded plane height and a gap between frames."""
    pitch = w + 6
    pitch_c = w + 10 if layout == "nv12" else w // 2 + 3
    off_u = (h + 3) * pitch
    if layout == "nv12":
        return video.yuv_desc(w, h, layout, pitch=pitch, pitch_c=pitch_c, off_u=off_u, frame_stride=off_u + (h // 2 + 1) * pitch_c + 37)
    off_v = off_u + (h // 2 + 2) * pitch_c
    return video.yuv_desc(w, h, layout, pitch=pitch, pitch_c=pitch_c, off_u=off_u, off_v=off_v, frame_stride=off_v + (h // 2 + 1) * pitch_c + 37)


def basis63(h, w):
    """Every 8 x 8 block the basis function of coefficient (7, 7) around 128."""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.rint(128 + 110 * np.outer(c, c)).astype(np.uint8)
    return np.tile(tile, ((h + 7) // 8, (w + 7) // 8))[:h, :w]


def planes(content, w, h, i):
    """(Y, Cb, Cr) of frame ``i``."""
    y, x = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    if content in ("grey", "zeros", "ones"):
        v = {"grey": 128, "zeros": 0, "ones": 255}[content]
        return tuple(np.full(s, v, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    if content == "ramp":
        return (((3 * x + 5 * y + 17 * i) & 255).astype(np.uint8), ((2 * cx + cy + 40 * i) & 255).astype(np.uint8),
                (255 - ((cx + 3 * cy + 9 * i) & 255)).astype(np.uint8))
    if content == "basis63":
        return basis63(h, w), basis63(h // 2, w // 2), np.full((h // 2, w // 2), 128, np.uint8)
    rng = np.random.default_rng([w, h, i, len(content)])
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def raw_frames(content, w, h, layout, n, sentinel):
    """(the bytes of ``n`` frames with ``sentinel`` in every byte no plane owns, desc)."""
    d = geometry(w, h, layout)
    raw = np.full(video.yuv_span(n, h, w, d) + 5, sentinel, np.uint8)
    for i in range(n):
        for dst, src in zip(mjpeg.planes(raw, i, h, w, d), planes(content, w, h, i)):
            np.lib.stride_tricks.as_strided(dst, dst.shape, dst.strides, writeable=True)[...] = src
    return raw, d


@functools.lru_cache(maxsize=None)
def expected(content, w, h, layout, n):
    """``mjpeg.encode_host`` of the case (computed once, shared, read-only)."""
    raw, d = raw_frames(content, w, h, layout, n, 0xa5)
    data, offsets = mjpeg.encode_host(raw, n, h, w, d, CONTENTS[content])
    data.flags.writeable = False
    offsets.flags.writeable = False
    return data, offsets
