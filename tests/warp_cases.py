"""Cases for the perspective warp (test_warp_host.py, test_gpu_warp.py): the named ones whose answers are known, seeded matrices with
perspective terms up to a horizon inside the canvas, an independent per-pixel statement of the rule, and the case file of the
stand-alone program tests/warp_main.cpp.  numpy alone: nothing here needs pytest, an engine or a GPU."""
import math
import struct
from typing import NamedTuple

import numpy as np

IDENTITY = np.eye(3)


class Case(NamedTuple):
    name: str
    frames: np.ndarray          # (n, h, w, 3) uint8
    matrices: np.ndarray        # (n, 3, 3) float64, canvas -> source
    valid: np.ndarray           # (n,) int32
    oh: int
    ow: int
    fill: tuple                 # (B, G, R)


def frames_of(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def translation(dx, dy):
    """Canvas (u, v) reads the source at (u + dx, v + dy)."""
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def horizon_matrix(h, w, oh, ow, at=0.4):
    """A camera-like map whose horizon (Z = 0) crosses the canvas at row ``at * oh``: Z > 0 below it."""
    vh = at * oh
    return np.array([[w / ow * 0.9, 0.21, -0.07 * w], [0.05, h / oh * 1.3, -0.4 * h], [0.0003, 1.0 / max(oh - vh, 1.0), -vh / max(oh - vh, 1.0)]])


def one(name, frames, m, oh, ow, fill=(7, 99, 201), valid=1):
    return Case(name, frames, np.asarray(m, np.float64).reshape(1, 3, 3), np.array([valid], np.int32), oh, ow, fill)


def named_cases() -> dict:
    f = frames_of(1, 9, 13, 1)
    huge = np.array([[1e308, -1e308, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])       # X = inf - inf = NaN from (10, 10) on
    cases = [
        one("identity", f, IDENTITY, 9, 13),
        one("translation by (3, -2)", f, translation(3, -2), 9, 13),
        one("half a pixel", np.array([[[[10, 20, 30], [20, 40, 60]], [[30, 60, 90], [41, 81, 121]]]], np.uint8), translation(0.5, 0.5), 2, 2, fill=(0, 0, 0)),
        one("a hair below zero", f, translation(-1e-20, -1e-20), 9, 13),
        one("behind the horizon", f, np.array([[1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 4.0]]), 9, 13),      # Z = 4 - v: rows 4.. are not Z > 0
        one("zero over zero", f, np.zeros((3, 3)), 9, 13),
        one("infinity minus infinity", f, huge, 12, 12),
        one("not valid", f, IDENTITY, 9, 13, valid=0),
    ]
    return {c.name: c for c in cases}


def seeded_cases(count=300, seed=11) -> list:
    """Sources from 1 x 1 to 67 x 45, canvases up to 23 x 19, affine parts that magnify and minify, perspective terms that put the
    horizon inside the canvas in about a third of the cases, two frames in some."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        w, h = (1, 1) if k == 0 else (67, 45) if k == 1 else (int(rng.integers(1, 68)), int(rng.integers(1, 46)))
        ow, oh = int(rng.integers(1, 24)), int(rng.integers(1, 20))
        n = 2 if k % 7 == 3 else 1
        ms = []
        for _ in range(n):
            s = rng.uniform(0.2, 4.0, 2) * (w / ow, h / oh)
            m = np.array([[s[0], rng.normal(0, 0.3), rng.uniform(-0.5 * w, 0.5 * w)],
                          [rng.normal(0, 0.3), s[1], rng.uniform(-0.5 * h, 0.5 * h)],
                          [0.0, 0.0, 1.0]])
            kind = k % 3
            if kind == 1:                                    # mild perspective, Z > 0 everywhere
                m[2, :2] = rng.uniform(0, 0.5, 2) / (ow, oh)
            elif kind == 2:                                  # the horizon crosses the canvas
                g = rng.uniform(-1.0, 1.0, 2)
                at = rng.uniform(0, 1, 2) * (ow, oh)
                m[2] = [g[0], g[1], -(g[0] * at[0] + g[1] * at[1])]
            ms.append(m)
        out.append(Case(f"seeded {k}", frames_of(n, h, w, 1000 + k), np.array(ms), np.ones(n, np.int32), oh, ow,
                        tuple(int(c) for c in rng.integers(0, 256, 3))))
    return out


def reference(case: Case) -> np.ndarray:
    """The rule stated independently, pixel by pixel in Python floats (IEEE double, nothing fused): float64 bilinear interpolation
    at the coordinates quantised to 1 / 32, ``floor(32 s) / 32``, rounded half up.  Weights that are multiples of 1 / 32 times bytes
    are exact in float64, so this IS the integer formula's value: no tolerance."""
    n, h, w = case.frames.shape[:3]
    out = np.empty((n, case.oh, case.ow, 3), np.uint8)
    fill = np.array(case.fill, np.float64)

    def P(i, x, y):
        return case.frames[i, y, x].astype(np.float64) if 0 <= x < w and 0 <= y < h else fill

    for i in range(n):
        m = [float(x) for x in case.matrices[i].reshape(-1)]
        for v in range(case.oh):
            for u in range(case.ow):
                out[i, v, u] = case.fill
                if not case.valid[i]:
                    continue
                X, Y, Z = (m[0] * u + m[1] * v) + m[2], (m[3] * u + m[4] * v) + m[5], (m[6] * u + m[7] * v) + m[8]
                if not Z > 0:
                    continue
                sx, sy = X / Z, Y / Z
                if not (-1 < sx < w and -1 < sy < h):
                    continue
                qx, qy = math.floor(sx * 32) / 32, math.floor(sy * 32) / 32
                x0, y0 = math.floor(qx), math.floor(qy)
                fx, fy = qx - x0, qy - y0
                val = (1 - fy) * ((1 - fx) * P(i, x0, y0) + fx * P(i, x0 + 1, y0)) + fy * ((1 - fx) * P(i, x0, y0 + 1) + fx * P(i, x0 + 1, y0 + 1))
                out[i, v, u] = np.floor(val + 0.5)
    return out


def fill_word(fill) -> int:
    return int(fill[0]) | int(fill[1]) << 8 | int(fill[2]) << 16


def case_bytes(n, h, w, oh, ow, fill, matrices, valid, frames) -> bytes:
    """One case of tests/warp_main.cpp's file."""
    return (struct.pack("<5iI", n, h, w, oh, ow, fill_word(fill)) + np.ascontiguousarray(matrices, "<f8").tobytes() +
            np.ascontiguousarray(valid, "<i4").tobytes() + np.ascontiguousarray(frames, np.uint8).tobytes())


def write_cases(path, cases) -> None:
    with open(path, "wb") as f:
        for c in cases:
            f.write(case_bytes(c.frames.shape[0], c.frames.shape[1], c.frames.shape[2], c.oh, c.ow, c.fill, c.matrices, c.valid, c.frames))


def read_answers(raw: bytes, sizes) -> list:
    """The program's stdout -> per case the (n, oh, ow, 3) canvas, or the words of the refusal.  ``sizes``: (n, oh, ow) per case."""
    out, at = [], 0
    for n, oh, ow in sizes:
        (refused,) = struct.unpack_from("<i", raw, at)
        at += 4
        if refused:
            (length,) = struct.unpack_from("<i", raw, at)
            out.append(raw[at + 4:at + 4 + length].decode())
            at += 4 + length
        else:
            size = n * oh * ow * 3
            out.append(np.frombuffer(raw, np.uint8, size, at).reshape(n, oh, ow, 3))
            at += size
    assert at == len(raw), (at, len(raw))
    return out
