"""YUV 4:2:0 -> BGR reference and test-data helpers (TEST INFRASTRUCTURE; imports nothing from the package).

``convert`` restates the written specification of the conversion (include/padel_hip.h, pa_yuv_desc) independently of
``video.yuv420_to_bgr_host`` and of the kernel: plain indexing, int64, Python's floor ``>>``.

    y = max(0, Y - y_off) * CY          u = U - 128      v = V - 128      h = 1 << 19
    R = clamp((y + h + CVR*v)         >> 20, 0, 255)
    G = clamp((y + h + CUG*u + CVG*v) >> 20, 0, 255)
    B = clamp((y + h + CUB*u)         >> 20, 0, 255)            each 2 x 2 block of pixels shares one (U, V)

``bgr_to_yuv420`` / ``write_y4m`` only have to produce plausible content, so that clips can be made from tests/synth.py frames."""
from __future__ import annotations

import numpy as np

# (y_off, CY, CVR, CUG, CVG, CUB), copied from the specification — NOT imported from video.YUV_COEFFS, which is under test
COEFFS = {
    "bt601_limited": (16, 1220542, 1673527, -409993, -852492, 2116026),
    "bt709_limited": (16, 1220542, 1880096, -223346, -558891, 2214592),
    "bt601_full": (0, 1048576, 1470103, -360852, -748825, 1858076),
    "bt709_full": (0, 1048576, 1651297, -196423, -490863, 1945737),
}
TABLES = tuple(COEFFS)

# (Y, U, V) -> (B, G, R) per table, computed by hand from the formula (the specification's known answers, verbatim)
KNOWN = [
    ((16, 128, 128), ((0, 0, 0), (0, 0, 0), (16, 16, 16), (16, 16, 16))),
    ((235, 128, 128), ((255, 255, 255), (255, 255, 255), (235, 235, 235), (235, 235, 235))),
    ((126, 128, 128), ((128, 128, 128), (128, 128, 128), (126, 126, 126), (126, 126, 126))),
    ((81, 90, 240), ((0, 0, 254), (0, 24, 255), (14, 14, 238), (10, 36, 255))),
    ((145, 54, 34), ((1, 255, 0), (0, 216, 0), (14, 238, 13), (8, 203, 0))),
    ((41, 240, 110), ((255, 0, 0), (255, 15, 0), (239, 15, 16), (249, 28, 13))),
    ((0, 0, 0), ((0, 154, 0), (0, 95, 0), (0, 135, 0), (0, 84, 0))),
    ((255, 255, 255), ((255, 125, 255), (255, 183, 255), (255, 121, 255), (255, 172, 255))),
    ((255, 0, 0), ((20, 255, 74), (8, 255, 49), (28, 255, 76), (17, 255, 53))),
    ((0, 255, 255), ((255, 0, 203), (255, 0, 228), (225, 0, 178), (236, 0, 200))),
]


def pixel(Y: int, U: int, V: int, coeffs) -> tuple:
    """One pixel, plain Python integers -> (B, G, R)."""
    y_off, CY, CVR, CUG, CVG, CUB = coeffs
    y = max(0, Y - y_off) * CY
    u, v, h = U - 128, V - 128, 1 << 19
    clamp = lambda x: min(max(x, 0), 255)
    return (clamp((y + h + CUB * u) >> 20), clamp((y + h + CUG * u + CVG * v) >> 20), clamp((y + h + CVR * v) >> 20))


def geometry(w: int, h: int, layout: str, pitch=None, pitch_c=None, off_u=None, off_v=None, frame_stride=None) -> dict:
    """Byte geometry of one frame; the defaults are tightly packed planes."""
    nv12 = layout == "nv12"
    pitch = w if pitch is None else pitch
    pitch_c = (w if nv12 else w // 2) if pitch_c is None else pitch_c
    off_u = h * pitch if off_u is None else off_u
    off_v = (off_u + 1 if nv12 else off_u + (h // 2) * pitch_c) if off_v is None else off_v
    end = (off_u if nv12 else max(off_u, off_v)) + (h // 2) * pitch_c
    return dict(layout=layout, pitch=pitch, pitch_c=pitch_c, off_u=off_u, off_v=off_v,
                frame_stride=end if frame_stride is None else frame_stride)


def planes(raw: np.ndarray, i: int, h: int, w: int, g: dict):
    """(Y (h, w), U (h/2, w/2), V (h/2, w/2)) of frame i as int64, gathered byte by byte from the geometry."""
    base = i * g["frame_stride"]
    step = 2 if g["layout"] == "nv12" else 1
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    Y = raw[base + yy * g["pitch"] + xx]
    U = raw[base + g["off_u"] + cy * g["pitch_c"] + cx * step]
    V = raw[base + g["off_v"] + cy * g["pitch_c"] + cx * step]
    return Y.astype(np.int64), U.astype(np.int64), V.astype(np.int64)


def convert(raw: np.ndarray, n: int, h: int, w: int, g: dict, coeffs) -> np.ndarray:
    """(n, h, w, 3) uint8 BGR of n frames in the byte array ``raw`` (geometry ``g``, six coefficients)."""
    y_off, CY, CVR, CUG, CVG, CUB = (int(c) for c in coeffs)
    out = np.empty((n, h, w, 3), np.uint8)
    half = 1 << 19
    for i in range(n):
        Y, U, V = planes(raw, i, h, w, g)
        u = np.kron(U - 128, np.ones((2, 2), np.int64))
        v = np.kron(V - 128, np.ones((2, 2), np.int64))
        y = np.maximum(0, Y - y_off) * CY
        out[i, ..., 0] = np.clip((y + half + CUB * u) >> 20, 0, 255)
        out[i, ..., 1] = np.clip((y + half + CUG * u + CVG * v) >> 20, 0, 255)
        out[i, ..., 2] = np.clip((y + half + CVR * v) >> 20, 0, 255)
    return out


def pack(Y: np.ndarray, U: np.ndarray, V: np.ndarray, g: dict, rng=None, lead: int = 0, tail: int = 0) -> np.ndarray:
    """Lay n frames' planes (Y (n, h, w), U / V (n, h/2, w/2) uint8) out as raw bytes with geometry ``g``; every byte that is no
    sample — row padding, gaps between planes and frames, ``lead`` / ``tail`` bytes around — is random (``rng``) or zero.  With
    ``lead`` the frames start at raw[lead:]."""
    n, h, w = Y.shape
    nv12 = g["layout"] == "nv12"
    crow = w if nv12 else w // 2
    extent = max((h - 1) * g["pitch"] + w, g["off_u"] + (h // 2 - 1) * g["pitch_c"] + crow,
                 0 if nv12 else g["off_v"] + (h // 2 - 1) * g["pitch_c"] + crow)
    size = lead + (n - 1) * g["frame_stride"] + extent + tail
    raw = rng.integers(0, 256, size, dtype=np.uint8) if rng is not None else np.zeros(size, np.uint8)
    step = 2 if nv12 else 1
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    for i in range(n):
        base = lead + i * g["frame_stride"]
        raw[base + yy * g["pitch"] + xx] = Y[i]
        raw[base + g["off_u"] + cy * g["pitch_c"] + cx * step] = U[i]
        raw[base + g["off_v"] + cy * g["pitch_c"] + cx * step] = V[i]
    return raw


def bgr_to_yuv420(frames: np.ndarray, layout: str = "nv12", **geo):
    """(raw bytes, geometry) of BGR frames (n, h, w, 3) encoded as limited-range BT.601 4:2:0: float forward matrix, rounding,
    chroma = mean of each 2 x 2 block.  Plausible content for clips, nothing more."""
    f = np.asarray(frames, np.float64)
    n, h, w, _ = f.shape
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = 16 + (65.481 * R + 128.553 * G + 24.966 * B) / 255
    U = 128 + (-37.797 * R - 74.203 * G + 112.0 * B) / 255
    V = 128 + (112.0 * R - 93.786 * G - 18.214 * B) / 255
    sub = lambda p: p.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    g = geometry(w, h, layout, **geo)
    return pack(q(Y), q(sub(U)), q(sub(V)), g), g


def write_y4m(path, Y: np.ndarray, U: np.ndarray, V: np.ndarray, header_tags: str = "F30:1 Ip A1:1 C420jpeg",
              trailing: bytes = b"") -> int:
    """Write planes (n, h, w) / (n, h/2, w/2) as a YUV4MPEG2 file; returns the length of the header line."""
    n, h, w = Y.shape
    head = f"YUV4MPEG2 W{w} H{h}{' ' + header_tags if header_tags else ''}\n".encode()
    with open(path, "wb") as fh:
        fh.write(head)
        for i in range(n):
            fh.write(b"FRAME\n")
            fh.write(Y[i].tobytes() + U[i].tobytes() + V[i].tobytes())
        fh.write(trailing)
    return len(head)


def planes_of_bgr(frames: np.ndarray):
    """(Y, U, V) planes of BGR frames, as ``bgr_to_yuv420`` encodes them (for ``write_y4m``)."""
    n, h, w, _ = frames.shape
    raw, g = bgr_to_yuv420(frames, "i420")
    P = [planes(raw, i, h, w, g) for i in range(n)]
    return tuple(np.stack([p[k] for p in P]).astype(np.uint8) for k in range(3))
