"""Frame sources: the reference reads video through ``supervision`` (``sv.VideoInfo.from_video_path``
``trackers/runner.py:52``, ``sv.get_video_frames_generator`` ``runner.py:215-220``), which needs OpenCV.
Neither is available here or on the GPU box, and the checkout ships no video, so this module provides the
same two calls over (a) ``.npy`` frame stacks (N,H,W,3 uint8 BGR, memory-mapped), (b) URL-style sources whose
scheme somebody registered with ``register_source`` (the tests and the bench register ``synthetic://?n=64&h=720&w=1280&
fps=30&seed=0``: tests/synth.py — generated frames are test infrastructure, not product) and (c) real video files when
``cv2`` happens to be importable, (d) ``DeviceClip`` objects: a clip already resident in HBM (the bench's device-resident mode; the
runner's fan-out mode uploads each batch once and hands the same ``DeviceFrame`` handles to every tracker), (e) 8-bit YUV 4:2:0 —
what decoders, capture cards and ``ffmpeg -f rawvideo`` actually emit, 1.5 bytes per pixel: ``YuvClip`` (NV12 / I420 bytes in host
memory, any pitch / padded plane height / gap between frames), ``DeviceYuvClip`` (the same bytes resident in HBM: a hardware
decoder's surfaces) and ``.y4m`` files by path (``YuvClip.from_y4m``: the one self-describing raw format, no codec).  Their
frames are ``YuvFrame`` handles; ``device_batch`` converts a batch to BGR on the GPU (csrc/yuv_convert.hip), ``host_batch`` /
``np.asarray(frame)`` on the host with the same integer formula (``yuv420_to_bgr_host``), (f) Motion-JPEG — ``.avi`` files with an
``MJPG`` stream, raw ``.mjpeg`` / ``.mjpg`` files, by path or as ``MjpegClip``: what ``MjpegSink`` writes, ``ffmpeg -c:v mjpeg``
produces from anything and capture cards emit.  Only the compressed bytes are uploaded; the frames are decoded to BGR on the GPU
(csrc/jpeg_decode.hip) into the clip's staging buffer, or on the host by the numpy twin ``mjpeg.decode_host``.
Frames are HWC uint8 **BGR**, exactly what supervision yields."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Iterator, Optional

import numpy as np


# scheme -> (info(url) -> VideoInfo, frames(url, start, end, stride) -> iterator of HWC uint8 BGR frames)
_SOURCES: dict = {}


def register_source(scheme: str, info, frames) -> None:
    """Make ``scheme://...`` paths readable by ``VideoInfo.from_video_path`` / ``get_video_frames_generator``."""
    _SOURCES[scheme] = (info, frames)


def _scheme(p: str):
    i = p.find("://")
    if i <= 0:
        return None
    if p[:i] not in _SOURCES:
        raise FileNotFoundError(f"no frame source registered for '{p[:i]}://' (video.register_source; the synthetic clips of "
                                f"the tests register themselves on `import tests.synth`)")
    return _SOURCES[p[:i]]


@dataclass
class VideoInfo:
    width: int
    height: int
    fps: int
    total_frames: Optional[int] = None

    @property
    def resolution_wh(self) -> tuple:
        return self.width, self.height

    @classmethod
    def from_video_path(cls, video_path) -> "VideoInfo":
        if isinstance(video_path, (DeviceClip, ArrayClip, _StagedSource)):
            return cls(video_path.w, video_path.h, video_path.fps, video_path.total_frames)
        p = str(video_path)
        src = _scheme(p)
        if src is not None:
            return src[0](p)
        if p.endswith(".y4m"):
            c = _open_y4m(p)
            return cls(c.w, c.h, c.fps, c.total_frames)
        if p.endswith(".npy"):
            a = np.load(p, mmap_mode="r")
            return cls(int(a.shape[2]), int(a.shape[1]), 30, int(a.shape[0]))
        c = _open_mjpeg(p)
        if c is not None:
            return cls(c.w, c.h, c.fps, c.total_frames)
        cv2 = _cv2()
        cap = cv2.VideoCapture(p)
        if not cap.isOpened():
            raise FileNotFoundError(f"Could not open video at {p}")
        info = cls(int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)), int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT)),
                   int(cap.get(cv2.CAP_PROP_FPS)), int(cap.get(cv2.CAP_PROP_FRAME_COUNT)))
        cap.release()
        return info


def _cv2():
    try:
        import cv2
        return cv2
    except ImportError as e:
        raise RuntimeError("reading encoded video needs opencv-python, which is not installed; use a Motion-JPEG file (.avi with an "
                           "'MJPG' stream, .mjpeg, .mjpg: `ffmpeg -i in.mp4 -c:v mjpeg -q:v 3 out.avi`), a .y4m file, a .npy frame "
                           "stack or a registered frame source") from e


class DeviceFrame:
    """Handle of one HWC uint8 BGR frame that lives in HBM (frame ``index`` of ``clip.buffer``).  Quacks like the
    ndarray the trackers expect as far as they look at it on the host (``.shape``)."""
    __slots__ = ("clip", "index")

    def __init__(self, clip: "DeviceClip", index: int):
        self.clip, self.index = clip, index

    @property
    def shape(self) -> tuple:
        return (self.clip.h, self.clip.w, 3)


class DeviceClip:
    """``n`` frames resident in HBM, presented as a clip of ``n * repeat`` frames (frame i = stored frame i % n)."""

    def __init__(self, engine, frames: Optional[np.ndarray] = None, *, shape: Optional[tuple] = None, repeat: int = 1,
                 fps: int = 30):
        if frames is not None:
            frames = np.ascontiguousarray(frames, np.uint8)
            shape = frames.shape
        self.n, self.h, self.w = int(shape[0]), int(shape[1]), int(shape[2])
        self.repeat, self.fps = int(repeat), int(fps)
        self.frame_bytes = self.h * self.w * 3
        self.buffer = engine.alloc(self.n * self.frame_bytes)
        if frames is not None:
            self.buffer.upload(frames)

    @property
    def total_frames(self) -> int:
        return self.n * self.repeat

    def alias(self, repeat: int) -> "DeviceClip":
        """The same frames in HBM (no copy, not an owner: never ``free()`` it) presented with another ``repeat`` — the
        bench's sharded leg shows every rank a clip of world x K x n frames of which it only ever reads its own shard."""
        c = object.__new__(DeviceClip)
        c.__dict__.update(self.__dict__)
        c.repeat = int(repeat)
        return c

    def upload(self, frames: np.ndarray, first: int = 0, copy_stream: bool = True) -> None:
        """Overwrite stored frames [first, first + len(frames)) (prefetch thread of the runner's fan-out mode)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape[1:] == (self.h, self.w, 3) and first + len(frames) <= self.n
        self.buffer.view(first * self.frame_bytes, frames.nbytes).upload(frames, copy_stream=copy_stream)

    def frames(self, start: int = 0, end: Optional[int] = None, stride: int = 1) -> Iterator[DeviceFrame]:
        stop = self.total_frames if end is None else min(end, self.total_frames)
        for i in range(start, stop, stride):
            yield DeviceFrame(self, i % self.n)

    def free(self) -> None:
        self.buffer.free()


class ArrayClip:
    """Host-memory clip: ``frames`` (n, h, w, 3) uint8 BGR presented as ``n * repeat`` frames (bench: the
    PCIe-inclusive rate; tests)."""

    def __init__(self, frames: np.ndarray, repeat: int = 1, fps: int = 30):
        self.array = np.ascontiguousarray(frames, np.uint8)
        self.n, self.h, self.w = self.array.shape[:3]
        self.repeat, self.fps = int(repeat), int(fps)
        self._pinned_by = None

    def pin(self, engine) -> "ArrayClip":
        """Page-lock the clip (a decoder writing into pinned memory): batches of consecutive frames then go up without a
        staging copy (``host_batch``) and at PCIe speed."""
        if self._pinned_by is None:
            engine.pin(self.array)
            self._pinned_by = engine
        elif self._pinned_by is not engine:
            raise ValueError("ArrayClip is page-locked through another engine: unpin() it first")
        return self

    def unpin(self) -> None:
        if self._pinned_by is not None:
            eng, self._pinned_by = self._pinned_by, None
            eng.unpin(self.array)

    # a page-locked range must be unregistered before numpy frees it (a stale registration makes later registrations /
    # copies of recycled pages fail): `with ArrayClip(...).pin(eng) as clip:` or let the finaliser do it
    def __enter__(self) -> "ArrayClip":
        return self

    def __exit__(self, *exc) -> None:
        self.unpin()

    def __del__(self):
        try:
            self.unpin()
        except Exception:
            pass

    @property
    def total_frames(self) -> int:
        return self.n * self.repeat

    def frames(self, start: int = 0, end: Optional[int] = None, stride: int = 1) -> Iterator[np.ndarray]:
        stop = self.total_frames if end is None else min(end, self.total_frames)
        for i in range(start, stop, stride):
            yield self.array[i % self.n]


# ---------------------------------------------------------------------------------------------- YUV 4:2:0 sources
# name -> (y_off, CY, CVR, CUG, CVG, CUB): 20-bit fixed point, trunc(c * 2^20) of the 3-decimal coefficients (limited range) or of
# the standard's own (full range).  The formula (include/padel_hip.h, pa_yuv_desc) is the specification; bt601_limited uses the
# constants of OpenCV's COLOR_YUV2BGR_NV12 / _I420 as recalled — parity with cv2 is unpinned.
YUV_COEFFS = {
    "bt601_limited": (16, 1220542, 1673527, -409993, -852492, 2116026),
    "bt709_limited": (16, 1220542, 1880096, -223346, -558891, 2214592),
    "bt601_full": (0, 1048576, 1470103, -360852, -748825, 1858076),
    "bt709_full": (0, 1048576, 1651297, -196423, -490863, 1945737),
}
YUV_LAYOUTS = {"nv12": 0, "i420": 1}          # enum pa_yuv_layout
# The other direction (include/padel_hip.h, pa_yuv_enc; csrc/render.hip): name -> (y_off, YR, YG, YB, UR, UG, UB, VR, VG, VB), each
# round(c * 2^20) of the standard matrix for (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722): Y = Kr R + Kg G + Kb B,
# U = (B - Y) / (2 (1 - Kb)), V = (R - Y) / (2 (1 - Kr)); limited range scales luma by 219 / 255 and chroma by 224 / 255.  The U
# row and the V row each sum to 0 — grey encodes to U = V = 128 exactly.
YUV_ENC_COEFFS = {
    "bt601_limited": (16, 269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897),
    "bt709_limited": (16, 191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230),
    "bt601_full": (0, 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262),
    "bt709_full": (0, 222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074),
}
_DESC_FIELDS = ("layout", "pitch_y", "pitch_c", "off_u", "off_v", "frame_stride", "y_off", "cy", "cvr", "cug", "cvg", "cub")


def yuv_desc(w: int, h: int, layout: str = "nv12", matrix: str = "bt601", range: str = "limited", pitch: Optional[int] = None,
             pitch_c: Optional[int] = None, off_u: Optional[int] = None, off_v: Optional[int] = None,
             frame_stride: Optional[int] = None, coeffs: Optional[tuple] = None) -> dict:
    """The fields of ``pa_yuv_desc`` for ``h`` x ``w`` frames.  The defaults describe tightly packed frames: rows as long as
    their pixels, chroma straight behind the last luma row, the next frame straight behind the last chroma row.  ``coeffs``:
    six integers in place of the named table ``YUV_COEFFS[f"{matrix}_{range}"]``."""
    if layout not in YUV_LAYOUTS:
        raise ValueError(f"YUV layout {layout!r}: expected 'nv12' or 'i420'")
    if coeffs is None:
        name = f"{matrix}_{range}"
        if name not in YUV_COEFFS:
            raise ValueError(f"no YUV coefficient table {name!r} (video.YUV_COEFFS: {', '.join(YUV_COEFFS)})")
        coeffs = YUV_COEFFS[name]
    w, h = int(w), int(h)
    nv12 = layout == "nv12"
    pitch = w if pitch is None else int(pitch)
    pitch_c = (w if nv12 else w // 2) if pitch_c is None else int(pitch_c)
    off_u = h * pitch if off_u is None else int(off_u)
    off_v = (off_u + 1 if nv12 else off_u + (h // 2) * pitch_c) if off_v is None else int(off_v)
    if frame_stride is None:
        frame_stride = (off_u if nv12 else max(off_u, off_v)) + (h // 2) * pitch_c
    y_off, cy, cvr, cug, cvg, cub = (int(c) for c in coeffs)
    return dict(layout=YUV_LAYOUTS[layout], pitch_y=pitch, pitch_c=pitch_c, off_u=off_u, off_v=off_v, frame_stride=int(frame_stride),
                y_off=y_off, cy=cy, cvr=cvr, cug=cug, cvg=cvg, cub=cub)


def _desc_dict(desc) -> dict:
    return dict(desc) if isinstance(desc, dict) else {k: int(getattr(desc, k)) for k in _DESC_FIELDS}


def yuv_span(n: int, h: int, w: int, desc) -> int:
    """Bytes that ``n`` frames described by ``desc`` reach from the start of the first; ValueError for geometry that no
    conversion accepts (the cases ``pa_yuv420_to_bgr`` refuses)."""
    d = _desc_dict(desc)
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise ValueError(f"{w} x {h} frames: 4:2:0 needs an even width and height of at least 2")
    if n < 1:
        raise ValueError(f"n = {n} frames")
    nv12 = d["layout"] == YUV_LAYOUTS["nv12"]
    crow = w if nv12 else w // 2
    if d["pitch_y"] < w or d["pitch_c"] < crow:
        raise ValueError(f"pitch smaller than its row (pitch_y {d['pitch_y']} for {w} bytes, pitch_c {d['pitch_c']} for {crow})")
    if d["off_u"] < 0 or d["off_v"] < 0 or (nv12 and d["off_v"] != d["off_u"] + 1):
        raise ValueError(f"bad plane offsets off_u {d['off_u']}, off_v {d['off_v']} (NV12: off_v = off_u + 1)")
    c_len = (h // 2 - 1) * d["pitch_c"] + crow
    extent = max((h - 1) * d["pitch_y"] + w, d["off_u"] + c_len, 0 if nv12 else d["off_v"] + c_len)
    if d["frame_stride"] < extent:
        raise ValueError(f"frame_stride {d['frame_stride']} is smaller than the {extent} bytes the planes of one frame span")
    return (n - 1) * d["frame_stride"] + extent


def yuv420_to_bgr_host(raw, n: int, h: int, w: int, desc) -> np.ndarray:
    """(n, h, w, 3) uint8 BGR of ``n`` frames of 8-bit YUV 4:2:0 in the 1-D byte array ``raw``, geometry and coefficients as in
    ``pa_yuv_desc`` (``yuv_desc``).  The CPU path and the readable twin of csrc/yuv_convert.hip — the same integers:
    nearest-neighbour chroma, 20-bit fixed point in int32, ``>>`` arithmetic."""
    d = _desc_dict(desc)
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.ndim != 1:
        raise ValueError("raw YUV bytes must be a 1-D uint8 array")
    if yuv_span(n, h, w, d) > raw.size:
        raise ValueError(f"{n} frames as described span {yuv_span(n, h, w, d)} bytes, the array holds {raw.size}")
    nv12 = d["layout"] == YUV_LAYOUTS["nv12"]
    strided = np.lib.stride_tricks.as_strided
    cs = 2 if nv12 else 1                                   # NV12: U and V alternate inside a chroma row
    out = np.empty((n, h, w, 3), np.uint8)
    half = np.int32(1 << 19)
    for i in range(n):
        f = raw[i * d["frame_stride"]:]
        Y = strided(f, (h, w), (d["pitch_y"], 1)).astype(np.int32)
        U = strided(f[d["off_u"]:], (h // 2, w // 2), (d["pitch_c"], cs)).astype(np.int32)
        V = strided(f[d["off_v"]:], (h // 2, w // 2), (d["pitch_c"], cs)).astype(np.int32)
        u = (U - 128).repeat(2, axis=0).repeat(2, axis=1)     # each 2 x 2 block of pixels shares one (U, V)
        v = (V - 128).repeat(2, axis=0).repeat(2, axis=1)
        y = np.maximum(0, Y - np.int32(d["y_off"])) * np.int32(d["cy"]) + half
        out[i, ..., 2] = np.clip((y + np.int32(d["cvr"]) * v) >> 20, 0, 255)
        out[i, ..., 1] = np.clip((y + np.int32(d["cug"]) * u + np.int32(d["cvg"]) * v) >> 20, 0, 255)
        out[i, ..., 0] = np.clip((y + np.int32(d["cub"]) * u) >> 20, 0, 255)
    return out


def bgr_to_yuv420_host(frames: np.ndarray, desc, enc, out: Optional[np.ndarray] = None) -> np.ndarray:
    """``frames`` (n, h, w, 3) uint8 BGR -> the 1-D byte array of ``n`` frames of 8-bit YUV 4:2:0 laid out by ``desc`` (bytes between
    the planes and rows stay as ``out`` has them, zero without ``out``), coefficients ``enc`` = (y_off, yr, yg, yb, ur, ug, ub, vr, vg,
    vb).  The readable twin of the encode half of csrc/render.hip — the same integers (include/padel_hip.h, pa_yuv_enc): int32,
    ``>>`` arithmetic, chroma from the sums over each 2 x 2 block."""
    d = _desc_dict(desc)
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    span = yuv_span(n, h, w, d)
    if out is None:
        out = np.zeros(span, np.uint8)
    if out.dtype != np.uint8 or out.ndim != 1 or out.size < span:
        raise ValueError(f"{n} frames as described span {span} bytes")
    y_off, yr, yg, yb, ur, ug, ub, vr, vg, vb = (np.int32(c) for c in enc)
    nv12 = d["layout"] == YUV_LAYOUTS["nv12"]
    strided = np.lib.stride_tricks.as_strided
    cs = 2 if nv12 else 1
    for i in range(n):
        f = out[i * d["frame_stride"]:]
        B, G, R = (frames[i, ..., c].astype(np.int32) for c in range(3))
        Y = np.clip(((yr * R + yg * G + yb * B + np.int32(1 << 19)) >> 20) + y_off, 0, 255)
        Bs, Gs, Rs = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] for p in (B, G, R))      # sums over each 2 x 2 block
        U = np.clip(((ur * Rs + ug * Gs + ub * Bs + np.int32(1 << 21)) >> 22) + 128, 0, 255)
        V = np.clip(((vr * Rs + vg * Gs + vb * Bs + np.int32(1 << 21)) >> 22) + 128, 0, 255)
        strided(f, (h, w), (d["pitch_y"], 1))[...] = Y
        strided(f[d["off_u"]:], (h // 2, w // 2), (d["pitch_c"], cs))[...] = U
        strided(f[d["off_v"]:], (h // 2, w // 2), (d["pitch_c"], cs))[...] = V
    return out


class YuvFrame:
    """Handle of one frame of a YUV clip — or of any clip whose frames become BGR on their way to the trackers (``MjpegClip`` hands
    out its subclass ``MjpegFrame``) — stored frame ``index`` of ``clip``.  ``.shape`` is the BGR frame's; ``np.asarray(f)`` /
    ``f.bgr()`` convert it on the host; a batch of them goes through ``device_batch`` / ``host_batch``."""
    __slots__ = ("clip", "index")

    def __init__(self, clip: "_StagedSource", index: int):
        self.clip, self.index = clip, index

    @property
    def shape(self) -> tuple:
        return (self.clip.h, self.clip.w, 3)

    def bgr(self) -> np.ndarray:
        return self.clip.host_bgr(self.index, 1)[0]

    def __array__(self, dtype=None, copy=None):
        a = self.bgr()
        return a if dtype is None else a.astype(dtype)


class _StagedSource:
    """A clip of ``n`` stored frames (presented ``repeat`` times over) that reach the trackers as BGR through one staging buffer in
    HBM: the frame handles, the staging buffer and the memory of which stored range it holds.  A subclass says how a range gets
    there (``_to_device``, through the engine method named ``_engine_call``) and what it is on the host (``host_bgr``)."""
    _engine_call = "yuv420_to_bgr"
    _frame_type = YuvFrame

    def _init_staging(self, fps, repeat) -> None:
        self.fps, self.repeat = int(fps), int(repeat)
        self.frame_bytes = self.h * self.w * 3
        self._bgr = None                 # DeviceBuffer: BGR frames of the stored range _bgr_range = (first, count)
        self._bgr_range = None

    @property
    def total_frames(self) -> int:
        return self.n * self.repeat

    def frames(self, start: int = 0, end: Optional[int] = None, stride: int = 1) -> Iterator[YuvFrame]:
        stop = self.total_frames if end is None else min(end, self.total_frames)
        for i in range(start, stop, stride):
            k = i % self.n
            self._check_marker(k)
            yield self._frame_type(self, k)

    def _check_marker(self, k: int) -> None:
        pass

    def _engine_or_default(self):
        if self.engine is None:
            from . import engine as E
            self.engine = E.default_engine()
        return self.engine

    def invalidate(self) -> None:
        """The clip's bytes were rewritten (a decoder's ring came round): forget which range the BGR staging holds."""
        self._bgr_range = None

    def device_view(self, first: int, count: int):
        """(DeviceBuffer view over the BGR of stored frames [first, first + count), count, h, w): converted on the GPU into the
        clip's staging buffer, on the engine's compute stream — the stream every later reader of the view and the next
        conversion into it are queued on, which is what makes one staging buffer enough (include/padel_hip.h,
        pa_yuv420_to_bgr).  A range the staging already holds converts nothing (fan-out: every tracker asks for the same batch)."""
        assert 0 <= first and count >= 1 and first + count <= self.n, (first, count, self.n)
        eng = self._engine_or_default()
        if not hasattr(eng, self._engine_call):      # a stand-in engine without kernels (tests/fake_engine.py): host path
            return None
        held = self._bgr_range
        if held is None or first < held[0] or first + count > held[0] + held[1]:
            need = count * self.frame_bytes
            if self._bgr is None or self._bgr.nbytes < need:
                if self._bgr is not None:
                    eng.synchronize()                # readers of the old staging may still be queued
                    self._bgr.free()
                self._bgr_range = None
                self._bgr = eng.alloc(need)
            self._bgr_range = None
            self._to_device(eng, first, count)
            held = self._bgr_range = (first, count)
        return self._bgr.view((first - held[0]) * self.frame_bytes, count * self.frame_bytes), count, self.h, self.w

    def free(self) -> None:
        """Release the BGR staging buffer (and what else the clip owns in HBM)."""
        if self._bgr is not None:
            if self.engine is not None:
                self.engine.synchronize()
            self._bgr.free()
        self._bgr, self._bgr_range = None, None


class _YuvSource(_StagedSource):
    """What ``YuvClip`` and ``DeviceYuvClip`` share: the geometry of the raw bytes and their conversion."""

    def _init_geometry(self, nbytes: int, w, h, layout, matrix, range, pitch, pitch_c, off_u, off_v, frame_stride, header_bytes, n,
                       fps, repeat, coeffs=None) -> None:
        self.w, self.h = int(w), int(h)
        self.layout = layout
        self.desc = yuv_desc(w, h, layout, matrix, range, pitch, pitch_c, off_u, off_v, frame_stride, coeffs)
        self.header_bytes = int(header_bytes)
        self.frame_stride = self.desc["frame_stride"]
        self.extent = yuv_span(1, self.h, self.w, self.desc)
        fit = (nbytes - self.header_bytes - self.extent) // self.frame_stride + 1 if nbytes - self.header_bytes >= self.extent else 0
        self.n = fit if n is None else int(n)
        if self.n < 1 or self.n > fit:
            raise ValueError(f"{nbytes} bytes hold {fit} frame(s) of this geometry behind a {self.header_bytes}-byte header; n = {self.n}")
        self._init_staging(fps, repeat)
        self._marker = None              # .y4m: the bytes every frame record starts with, checked when the frame is yielded

    def _offset(self, i: int) -> int:
        return self.header_bytes + i * self.frame_stride

    def host_bgr(self, first: int, count: int) -> np.ndarray:
        """(count, h, w, 3) uint8 BGR of stored frames [first, first + count), converted on the host."""
        return yuv420_to_bgr_host(self._host_bytes(first, count), count, self.h, self.w, self.desc)

    def _to_device(self, eng, first: int, count: int) -> None:
        eng.yuv420_to_bgr(self._device_source(first, count), count, self.h, self.w, self.desc, self._bgr)


class YuvClip(_YuvSource):
    """Host-memory clip of 8-bit YUV 4:2:0 frames: ``data`` is a 1-D uint8 array (or ``np.memmap``) of raw bytes, frame i at
    ``header_bytes + i * frame_stride``, planes inside a frame as ``yuv_desc`` describes (defaults: tightly packed).  Presented
    as ``n * repeat`` frames.  ``on_device=True``: batches are uploaded raw — half the bytes of BGR — and converted on the GPU
    of ``engine`` (default: the default engine, the one the trackers' models run on: the conversion is ordered with them by that
    engine's stream); ``on_device=False``: converted on the host (boxes without a GPU)."""

    def __init__(self, data, w: int, h: int, layout: str = "nv12", matrix: str = "bt601", range: str = "limited",
                 pitch: Optional[int] = None, pitch_c: Optional[int] = None, off_u: Optional[int] = None, off_v: Optional[int] = None,
                 frame_stride: Optional[int] = None, header_bytes: int = 0, n: Optional[int] = None, fps: int = 30, repeat: int = 1,
                 on_device: bool = True, engine=None, coeffs: Optional[tuple] = None):
        if not isinstance(data, np.ndarray) or data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError("YuvClip: data must be a 1-D uint8 array of raw bytes")
        self.data = data
        self.on_device, self.engine = bool(on_device), engine
        self._pinned_by = None
        self._init_geometry(data.size, w, h, layout, matrix, range, pitch, pitch_c, off_u, off_v, frame_stride, header_bytes, n, fps,
                            repeat, coeffs)

    # ---- .y4m: "YUV4MPEG2 W.. H.. F..:.. I. A..:.. C.. X..\n", then per frame "FRAME\n" + the planes of one I420 frame
    @classmethod
    def from_y4m(cls, path, matrix: Optional[str] = None, range: Optional[str] = None, **kw) -> "YuvClip":
        """Memory-map a ``.y4m`` file (``ffmpeg -i rally.mp4 rally.y4m`` writes one).  8-bit 4:2:0 progressive only; ``matrix``
        defaults to bt601, ``range`` to the file's ``XCOLORRANGE`` tag, else limited."""
        path = str(path)
        size = os.path.getsize(path)
        with open(path, "rb") as fh:
            head = fh.read(4096)
        eol = head.find(b"\n")
        if not head.startswith(b"YUV4MPEG2") or eol < 0:
            raise ValueError(f"{path}: not a YUV4MPEG2 file (no 'YUV4MPEG2 ...' header line in the first 4096 bytes)")
        w = h = None
        fps, tag_range = 30, None
        for tok in head[:eol].decode("ascii", "replace").split()[1:]:
            key, val = tok[0], tok[1:]
            if key == "W":
                w = int(val)
            elif key == "H":
                h = int(val)
            elif key == "F":
                num, _, den = val.partition(":")
                if int(num) > 0 and int(den or 1) > 0:
                    fps = int(round(int(num) / int(den or 1)))
            elif key == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"{path}: interlacing I{val} is not supported (progressive frames only)")
            elif key == "C":
                if val not in ("420", "420jpeg", "420mpeg2", "420paldv"):
                    raise ValueError(f"{path}: chroma format C{val} is not supported (8-bit 4:2:0 only)")
            elif tok.startswith("XCOLORRANGE="):
                tag_range = {"FULL": "full", "LIMITED": "limited"}.get(tok.split("=", 1)[1].upper())
            # A (pixel aspect) and other X tags: ignored
        if w is None or h is None:
            raise ValueError(f"{path}: the header names no W / H")
        if w < 2 or h < 2 or w % 2 or h % 2:
            raise ValueError(f"{path}: odd or too small frame size W{w} H{h} (4:2:0 needs an even width and height)")
        fb = w * h * 3 // 2
        header = eol + 1
        if (size - header) // (6 + fb) < 1:
            raise ValueError(f"{path}: no whole frame behind the header ({size} bytes)")
        data = np.memmap(path, np.uint8, "r")
        clip = cls(data, w, h, layout="i420", matrix=matrix or "bt601", range=range or tag_range or "limited",
                   frame_stride=6 + fb, header_bytes=header + 6, fps=kw.pop("fps", fps), **kw)
        clip._marker = b"FRAME\n"
        clip.path = path
        return clip

    def _check_marker(self, k: int) -> None:
        if self._marker is not None:
            at = self._offset(k) - len(self._marker)
            if self.data[at:at + len(self._marker)].tobytes() != self._marker:
                raise ValueError(f"{getattr(self, 'path', 'y4m')}: frame {k} does not start with 'FRAME\\n' at byte offset {at} "
                                 f"(frame parameters or a damaged file)")

    def pin(self, engine) -> "YuvClip":
        """Page-lock the raw bytes (a decoder writing into pinned memory): batches then go up at PCIe speed.  The memory
        must be writable (not a read-only mapping of a file)."""
        if self._pinned_by is None:
            engine.pin(self.data)
            self._pinned_by = engine
        elif self._pinned_by is not engine:
            raise ValueError("YuvClip is page-locked through another engine: unpin() it first")
        return self

    def unpin(self) -> None:
        if self._pinned_by is not None:
            eng, self._pinned_by = self._pinned_by, None
            eng.synchronize()                        # an upload from these pages may still be queued
            eng.unpin(self.data)

    def __enter__(self) -> "YuvClip":
        return self

    def __exit__(self, *exc) -> None:
        self.unpin()

    def __del__(self):
        try:
            self.unpin()
            self.free()
        except Exception:
            pass

    def _host_bytes(self, first: int, count: int) -> np.ndarray:
        o = self._offset(first)
        return self.data[o:o + (count - 1) * self.frame_stride + self.extent]

    _device_source = _host_bytes                     # the engine copies them to its raw staging buffer on the compute stream


class DeviceYuvClip(_YuvSource):
    """The raw YUV bytes resident in HBM — what a hardware decoder hands over.  ``data_or_buffer``: a 1-D uint8 array (uploaded
    once, from ``header_bytes`` on, into a buffer the clip owns) or a ``DeviceBuffer`` that already holds the bytes (not owned:
    ``free()`` leaves it alone).  Geometry arguments as for ``YuvClip``."""
    on_device = True

    def __init__(self, engine, data_or_buffer, w: int, h: int, layout: str = "nv12", matrix: str = "bt601", range: str = "limited",
                 pitch: Optional[int] = None, pitch_c: Optional[int] = None, off_u: Optional[int] = None, off_v: Optional[int] = None,
                 frame_stride: Optional[int] = None, header_bytes: int = 0, n: Optional[int] = None, fps: int = 30, repeat: int = 1,
                 coeffs: Optional[tuple] = None):
        self.engine = engine
        host = isinstance(data_or_buffer, np.ndarray)
        if host and (data_or_buffer.dtype != np.uint8 or data_or_buffer.ndim != 1):
            raise ValueError("DeviceYuvClip: data must be a 1-D uint8 array of raw bytes or a DeviceBuffer")
        nbytes = data_or_buffer.size if host else data_or_buffer.nbytes
        self._init_geometry(nbytes, w, h, layout, matrix, range, pitch, pitch_c, off_u, off_v, frame_stride, header_bytes, n, fps,
                            repeat, coeffs)
        if host:
            span = (self.n - 1) * self.frame_stride + self.extent
            self.buffer = engine.alloc(span)
            self.buffer.upload(np.ascontiguousarray(data_or_buffer[self.header_bytes:self.header_bytes + span]))
            self.header_bytes = 0
            self._owns = True
        else:
            self.buffer, self._owns = data_or_buffer, False

    def upload(self, raw: np.ndarray, first: int = 0) -> None:
        """Overwrite the bytes from stored frame ``first`` on (a decoder refilling its surfaces); forgets the converted range."""
        raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
        o = self._offset(first)
        assert o + raw.size <= self.buffer.nbytes
        self.engine.synchronize()                    # a conversion still queued reads the bytes about to change
        self.buffer.view(o, raw.size).upload(raw)
        self.invalidate()

    def _device_source(self, first: int, count: int):
        o = self._offset(first)
        return self.buffer.view(o, (count - 1) * self.frame_stride + self.extent)

    def _host_bytes(self, first: int, count: int) -> np.ndarray:
        v = self._device_source(first, count)
        return v.download(np.empty(v.nbytes, np.uint8))

    def free(self) -> None:
        super().free()
        if self._owns and self.buffer is not None:
            self.buffer.free()
        self.buffer = None


# ---------------------------------------------------------------------------------------------- Motion-JPEG sources
class MjpegFrame(YuvFrame):
    """Handle of one frame of an ``MjpegClip``: everything a ``YuvFrame`` is (``device_batch`` / ``host_batch`` / ``np.asarray``)."""
    __slots__ = ()


class MjpegClip(_StagedSource):
    """A Motion-JPEG clip: ``path_or_bytes`` is the path of a ``.avi`` (AVI 1.0, ``MJPG`` stream; ``MjpegSink``'s ``.partNNN`` files are
    followed) or ``.mjpeg`` / ``.mjpg`` file, or the JPEGs back to back as ``bytes`` / a 1-D uint8 array.  Baseline JPEG, 4:2:0, all
    frames of one size (``mjpeg.parse_frame`` says what else is refused).  Presented as ``n * repeat`` frames.  ``on_device=True``:
    a batch's compressed bytes are uploaded and decoded on the GPU of ``engine`` (default: the default engine) into one BGR staging
    buffer — ``Engine.jpeg_decode``; ``on_device=False``: decoded on the host by ``mjpeg.decode_host``, the same bytes (boxes
    without a GPU).  ``corrupt`` collects {stored frame: status word} of frames whose entropy-coded data was damaged: they are
    reported (a warning, once per frame) and decoded as far as they go, never an error."""
    _engine_call = "jpeg_decode"
    _frame_type = MjpegFrame

    def __init__(self, path_or_bytes, on_device: bool = True, engine=None, repeat: int = 1, fps: Optional[int] = None):
        from . import mjpeg
        if isinstance(path_or_bytes, (bytes, bytearray, np.ndarray)):
            raw = np.frombuffer(path_or_bytes, np.uint8) if not isinstance(path_or_bytes, np.ndarray) else path_or_bytes
            if raw.dtype != np.uint8 or raw.ndim != 1:
                raise ValueError("MjpegClip: the bytes must be a 1-D uint8 array")
            buf = raw.tobytes()
            self.index = mjpeg.MjpegIndex(["<bytes>"], [(0, off, n) for off, n in mjpeg.split_mjpeg(buf)], 30, [raw])
            self.path = None
        else:
            self.path = str(path_or_bytes)
            self.index = mjpeg.index_file(self.path)
        self.w, self.h, self.n = self.index.w, self.index.h, len(self.index)
        self.on_device, self.engine = bool(on_device), engine
        self.corrupt: dict = {}
        self.decodes = 0                     # batches decoded so far (a range the staging already held is not one)
        self._init_staging(self.index.fps if fps is None else fps, repeat)

    def _report(self, first: int, status) -> None:
        import warnings
        for k in np.nonzero(status)[0]:
            if first + int(k) not in self.corrupt:
                self.corrupt[first + int(k)] = int(status[k])
                warnings.warn(f"{self.path or 'MjpegClip'}: frame {first + int(k)} is damaged (status 0x{int(status[k]):x}: mjpeg.ST_*); "
                              f"what could not be decoded is grey", RuntimeWarning, stacklevel=3)

    def host_bgr(self, first: int, count: int) -> np.ndarray:
        """(count, h, w, 3) uint8 BGR of stored frames [first, first + count), decoded on the host."""
        from . import mjpeg
        frames, status = mjpeg.decode_host_status(*self.index.batch(first, count))
        if frames.shape[1:3] != (self.h, self.w):
            raise ValueError(f"{self.path or 'MjpegClip'}: frames {first}.. are {frames.shape[2]} x {frames.shape[1]}, the clip is "
                             f"{self.w} x {self.h}: frame sizes differ within the clip")
        self.decodes += 1
        self._report(first, status)
        return frames

    def _to_device(self, eng, first: int, count: int) -> None:
        data, offsets = self.index.batch(first, count)
        self.decodes += 1
        self._report(first, eng.jpeg_decode(data, offsets, self._bgr, h=self.h, w=self.w))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------- sinks for rendered frames
#: the suffixes of Motion-JPEG files, to write (``MjpegSink``, ``open_sink``) and to read (``_open_mjpeg``); any other path is a ``.y4m``
MJPEG_SUFFIXES = (".avi", ".mjpeg", ".mjpg")


def jpeg_desc(w: int, h: int, quality: int = 90, layout: str = "i420", pitch: Optional[int] = None, pitch_c: Optional[int] = None) -> dict:
    """``yuv_desc`` of the full-range BT.601 frames the JPEG encoder is handed; ``ValueError`` with the encoder's words for frames or a
    ``quality`` it refuses (``mjpeg.check``)."""
    from . import mjpeg
    desc = yuv_desc(w, h, layout, "bt601", "full", pitch, pitch_c)
    mjpeg.check(1, int(h), int(w), desc, int(quality))
    return desc


class FrameSink:
    """Where rendered frames go (``TrackingRunner(render=...)``).  A sink states the form it takes them in — ``w``, ``h``, ``desc``
    (the ``pa_yuv_desc`` fields the renderer writes by: ``yuv_desc``) and ``enc`` (the ten integers of ``pa_yuv_enc``) — and receives
    them ``n`` at a time as one ``DeviceBuffer`` of YUV 4:2:0 bytes in HBM.  ``Y4mSink`` downloads and writes them to a file; a
    hardware encoder's input surfaces would be another sink."""
    w: int
    h: int
    desc: dict
    enc: tuple

    def write_device(self, buffer, n: int) -> None:
        raise NotImplementedError

    def close(self) -> None:
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class Y4mSink(FrameSink):
    """Writes a ``.y4m`` file: the header ``YuvClip.from_y4m`` reads back (its colour-range tag included), then ``FRAME\\n`` plus the
    Y, U and V planes for every frame.  ``layout`` / ``pitch`` / ``pitch_c`` describe the frames it is HANDED (``desc``: tightly
    packed by default; NV12's interleaved chroma is split into the file's planes on the host); ``matrix`` and ``range`` pick the
    encode table ``YUV_ENC_COEFFS`` (.y4m has no tag for the matrix: bt601 is what ``from_y4m`` assumes)."""

    def __init__(self, path, w: int, h: int, fps: int = 30, layout: str = "i420", matrix: str = "bt601", range: str = "limited",
                 pitch: Optional[int] = None, pitch_c: Optional[int] = None):
        name = f"{matrix}_{range}"
        if name not in YUV_ENC_COEFFS:
            raise ValueError(f"no YUV encode table {name!r} (video.YUV_ENC_COEFFS: {', '.join(YUV_ENC_COEFFS)})")
        self.path, self.w, self.h, self.fps, self.layout = str(path), int(w), int(h), int(fps), layout
        self.desc = yuv_desc(w, h, layout, matrix, range, pitch, pitch_c)
        self.enc = YUV_ENC_COEFFS[name]
        self.extent = yuv_span(1, self.h, self.w, self.desc)
        self.frames_written = 0
        self._host = None
        self._fh = open(self.path, "wb")
        self._fh.write(f"YUV4MPEG2 W{self.w} H{self.h} F{self.fps}:1 Ip A1:1 C420jpeg XCOLORRANGE={range.upper()}\n".encode("ascii"))

    def write_host(self, raw: np.ndarray, n: int) -> None:
        """``n`` frames in the 1-D byte array ``raw``, laid out by ``desc``."""
        d, h, w = self.desc, self.h, self.w
        strided = np.lib.stride_tricks.as_strided
        cs = 2 if self.layout == "nv12" else 1
        for i in range(n):
            f = raw[i * d["frame_stride"]:]
            self._fh.write(b"FRAME\n")
            self._fh.write(np.ascontiguousarray(strided(f, (h, w), (d["pitch_y"], 1))).tobytes())
            self._fh.write(np.ascontiguousarray(strided(f[d["off_u"]:], (h // 2, w // 2), (d["pitch_c"], cs))).tobytes())
            self._fh.write(np.ascontiguousarray(strided(f[d["off_v"]:], (h // 2, w // 2), (d["pitch_c"], cs))).tobytes())
        self.frames_written += n

    def write_device(self, buffer, n: int) -> None:
        span = yuv_span(n, self.h, self.w, self.desc)
        if self._host is None or self._host.size < span:
            self._host = np.empty(span, np.uint8)
        buffer.download(self._host[:span])             # (synchronous: the render queued before it has finished)
        self.write_host(self._host, n)

    def close(self) -> None:
        if self._fh is not None:
            self._fh.close()
            self._fh = None


class MjpegSink(FrameSink):
    """Writes the frames as Motion-JPEG: every frame one baseline JPEG (``include/padel_hip.h``, ``pa_jpeg_encode``), encoded on the GPU
    from the renderer's output (``Engine.jpeg_encode``) — only the compressed bytes cross to the host — or, with ``on_device=False``,
    by the numpy twin ``mjpeg.encode_host``.  The renderer is asked for full-range BT.601 (``enc``), the matrix JFIF decoders assume.
    The suffix of ``path`` picks the container:

    * ``.mjpeg`` / ``.mjpg``: the JPEGs back to back (``ffmpeg -f mjpeg`` reads that); unbounded.
    * ``.avi``: AVI 1.0 — ``RIFF 'AVI '``, ``hdrl`` (``avih``, one ``strl`` with ``strh`` ``vids`` / ``MJPG`` and ``strf``, a
      BITMAPINFOHEADER with ``biCompression = 'MJPG'``), a ``movi`` list of ``00dc`` chunks padded to even length, ``idx1``; the frame
      count and the sizes are patched in ``close()``.  AVI 1.0 ends at 2 GiB: when the next frame would take the RIFF past
      ``max_riff_bytes`` the file is finished and the clip continues in ``<stem>.part002.avi``, ``.part003.avi``, ...

    ``paths`` lists the files written.  ``layout`` / ``pitch`` / ``pitch_c`` describe the frames the sink is HANDED, as for
    ``Y4mSink``."""
    _MOVI_AT = 220                                     # offset of the 'movi' fourcc: 12 + 12 + 64 + 12 + 64 + 48 + 8

    def __init__(self, path, w: int, h: int, fps: int = 30, quality: int = 90, layout: str = "i420", pitch: Optional[int] = None,
                 pitch_c: Optional[int] = None, max_riff_bytes: int = 2 ** 31 - 2 ** 24, on_device: bool = True):
        self.path, self.w, self.h, self.fps, self.layout = str(path), int(w), int(h), int(fps), layout
        self.quality, self.on_device = int(quality), bool(on_device)
        suffix = os.path.splitext(self.path)[1].lower()
        if suffix not in MJPEG_SUFFIXES:
            raise ValueError(f"MjpegSink: {self.path!r}: the suffix must be .avi, .mjpeg or .mjpg")
        self.avi = suffix == ".avi"
        self.desc = jpeg_desc(w, h, quality, layout, pitch, pitch_c)
        self.enc = YUV_ENC_COEFFS["bt601_full"]
        self.max_riff_bytes = int(max_riff_bytes)
        self.frames_written = 0
        self._closed_bytes = 0                         # of the files finished so far
        self.paths: list = []
        self._host = None
        self._fh = None
        self._open(self.path)

    @property
    def bytes_written(self) -> int:
        """Bytes of every file written so far (the open one: up to its last frame)."""
        return self._closed_bytes + (self._pos if self._fh is not None else 0)

    # ---- the container
    def _open(self, path: str) -> None:
        import struct
        self._fh = open(path, "wb")
        self.paths.append(path)
        self._index: list = []                         # (offset of the chunk from the 'movi' fourcc, size of its data)
        if self.avi:
            w, h = self.w, self.h
            avih = struct.pack("<14I", 1000000 // max(self.fps, 1), 0, 0, 0x10, 0, 0, 1, 0, w, h, 0, 0, 0, 0)
            strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, 0, 0, 0xffffffff, 0, 0, 0, w, h)
            strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
            strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
            hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
            head = b"RIFF" + struct.pack("<I", 0) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
            head += b"LIST" + struct.pack("<I", 0) + b"movi"
            assert len(head) == self._MOVI_AT + 4
            self._fh.write(head)
        self._pos = self._fh.tell()

    def _finish(self) -> None:
        """The index and the patched sizes of the open file; closes it."""
        import struct
        fh = self._fh
        if self.avi:
            n = len(self._index)
            movi_end = self._pos
            fh.write(b"idx1" + struct.pack("<I", 16 * n))
            fh.write(b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self._index))
            end = fh.tell()
            biggest = max((size for _, size in self._index), default=0)
            for at, value in ((4, end - 8), (self._MOVI_AT - 4, movi_end - self._MOVI_AT),
                              (32 + 16, n), (32 + 28, biggest),         # avih: dwTotalFrames, dwSuggestedBufferSize (data at 32)
                              (108 + 32, n), (108 + 36, biggest)):      # strh: dwLength, dwSuggestedBufferSize (data at 108)
                fh.seek(at)
                fh.write(struct.pack("<I", value))
            self._pos = end
        fh.close()
        self._fh = None
        self._closed_bytes += self._pos

    def _part_path(self, k: int) -> str:
        stem, suffix = os.path.splitext(self.path)
        return f"{stem}.part{k:03d}{suffix}"

    def write_jpegs(self, data: np.ndarray, offsets) -> None:
        """Append the JPEGs ``data[offsets[i]:offsets[i + 1]]``."""
        import struct
        for i in range(len(offsets) - 1):
            jpg = data[int(offsets[i]):int(offsets[i + 1])].tobytes()
            if not self.avi:
                self._fh.write(jpg)
                self._pos += len(jpg)
            else:
                chunk = 8 + len(jpg) + (len(jpg) & 1)
                if self._index and self._pos + chunk + 8 + 16 * (len(self._index) + 1) > self.max_riff_bytes:
                    self._finish()
                    self._open(self._part_path(len(self.paths) + 1))
                self._index.append((self._pos - self._MOVI_AT, len(jpg)))
                self._fh.write(b"00dc" + struct.pack("<I", len(jpg)) + jpg + (b"\0" if len(jpg) & 1 else b""))
                self._pos += chunk
            self.frames_written += 1

    def write_host(self, raw: np.ndarray, n: int) -> None:
        """``n`` frames in the 1-D byte array ``raw``, laid out by ``desc``: encoded on the host."""
        from . import mjpeg
        self.write_jpegs(*mjpeg.encode_host(raw, n, self.h, self.w, self.desc, self.quality))

    def write_device(self, buffer, n: int) -> None:
        if not self.on_device:
            span = yuv_span(n, self.h, self.w, self.desc)
            if self._host is None or self._host.size < span:
                self._host = np.empty(span, np.uint8)
            buffer.download(self._host[:span])
            return self.write_host(self._host[:span], n)
        if self._host is None:                         # the compressed frames of a batch: grown when a batch needs more
            self._host = np.empty(n * (self.w * self.h // 4 + 4096), np.uint8)
        from .engine import EngineError
        try:
            data, offsets = buffer.engine.jpeg_encode(buffer, n, self.h, self.w, self.desc, self.quality, out=self._host)
        except EngineError as e:
            if getattr(e, "needed", None) is None:
                raise
            self._host = np.empty(e.needed * 2, np.uint8)
            data, offsets = buffer.engine.jpeg_encode(buffer, n, self.h, self.w, self.desc, self.quality, out=self._host)
        self.write_jpegs(data, offsets)

    def close(self) -> None:
        if self._fh is not None:
            self._finish()


def _is_mjpeg(target) -> bool:
    return os.path.splitext(str(target))[1].lower() in MJPEG_SUFFIXES


def open_sink(target, w: int, h: int, fps: int = 30, quality: int = 90) -> tuple:
    """(the sink ``target`` names, whether the caller owns — and closes — it).  A ``FrameSink`` is the caller's own.  A path ending in
    ``.avi``, ``.mjpeg`` or ``.mjpg`` gives a ``MjpegSink`` of ``quality``, any other path a ``Y4mSink``, of ``w`` x ``h`` frames."""
    if isinstance(target, FrameSink):
        return target, False
    return (MjpegSink(target, w, h, fps=fps, quality=quality) if _is_mjpeg(target) else Y4mSink(target, w, h, fps=fps)), True


def check_sink(target, w: int, h: int, quality: int = 90) -> None:
    """The ``ValueError`` ``open_sink`` would give for the path ``target`` — frames the file's format cannot hold —, without creating
    the file; for a ``FrameSink`` that states another size than ``w`` x ``h``: "the sink takes ... frames"."""
    if isinstance(target, FrameSink):
        sw, sh = getattr(target, "w", None), getattr(target, "h", None)
        if sw is not None and sh is not None and (int(sw), int(sh)) != (int(w), int(h)):
            raise ValueError(f"the sink takes {sw} x {sh} frames")
    elif _is_mjpeg(target):
        jpeg_desc(w, h, quality)
    else:
        yuv_span(1, int(h), int(w), yuv_desc(w, h, "i420"))


# .y4m files opened by path: one clip per file as it is on disk now (every read of the path — VideoInfo, each tracker's pass — shares
# the mapping, the BGR staging and its memory of what it holds); a file that changed is opened afresh
_Y4M_OPEN: dict = {}


def _open_y4m(p: str) -> YuvClip:
    st = os.stat(p)
    key = (os.path.abspath(p), st.st_mtime_ns, st.st_size)
    hit = _Y4M_OPEN.get(key[0])
    if hit is None or hit[0] != key:
        if hit is not None:
            hit[1].free()
        hit = _Y4M_OPEN[key[0]] = (key, YuvClip.from_y4m(p))
    return hit[1]


# Motion-JPEG files opened by path, kept like _Y4M_OPEN; None for what is no Motion-JPEG file (the caller goes on to cv2)
_MJPEG_OPEN: dict = {}


def _open_mjpeg(p: str) -> Optional["MjpegClip"]:
    from . import mjpeg
    if not p.lower().endswith(MJPEG_SUFFIXES) or not os.path.exists(p):
        return None
    st = os.stat(p)
    key = (os.path.abspath(p), st.st_mtime_ns, st.st_size)
    hit = _MJPEG_OPEN.get(key[0])
    if hit is None or hit[0] != key:
        if hit is not None:
            hit[1].free()
        try:
            clip = MjpegClip(p)
        except mjpeg.NotMjpeg:
            return None
        hit = _MJPEG_OPEN[key[0]] = (key, clip)
    return hit[1]


def device_batch(sample):
    """If ``sample`` is a list of DeviceFrame handles of ONE clip with consecutive stored indices, return
    (DeviceBuffer view over exactly those frames, n, h, w); None for host frames.  Anything else is an error: a
    device batch must be one contiguous range (batch sizes that divide the stored clip length always are).
    ``YuvFrame`` handles of a clip with ``on_device=True`` follow the same rule: the range is converted to BGR on the GPU
    into the clip's staging buffer (once: asking for a range the staging already holds converts nothing) and the view over it
    comes back; with ``on_device=False`` the answer is None and ``host_batch`` converts on the host."""
    if isinstance(sample, np.ndarray) or not len(sample):
        return None
    if isinstance(sample[0], YuvFrame):
        clip, i0 = sample[0].clip, sample[0].index
        if not clip.on_device:
            return None
        for k, f in enumerate(sample):
            if not isinstance(f, YuvFrame) or f.clip is not clip or f.index != i0 + k:
                raise ValueError("a batch of device-converted YUV frames must be a contiguous range of one clip")
        return clip.device_view(i0, len(sample))
    if not isinstance(sample[0], DeviceFrame):
        return None
    clip, i0 = sample[0].clip, sample[0].index
    for k, f in enumerate(sample):
        if not isinstance(f, DeviceFrame) or f.clip is not clip or f.index != i0 + k:
            raise ValueError("a batch of device-resident frames must be a contiguous range of one DeviceClip")
    n = len(sample)
    return clip.buffer.view(i0 * clip.frame_bytes, n * clip.frame_bytes), n, clip.h, clip.w


def host_batch(sample) -> np.ndarray:
    """(n, h, w, 3) uint8 array of a batch of host frames.  Frames that are consecutive in memory — views of ONE
    contiguous array: an ``ArrayClip``, a memory-mapped .npy stack, a decoder's ring — come back as a view over them: no
    staging copy, and if that memory is page-locked the upload runs straight from it; anything else is stacked."""
    if isinstance(sample, np.ndarray):
        return sample
    sample = list(sample)
    f0 = sample[0]
    if any(isinstance(f, YuvFrame) for f in sample):
        if all(isinstance(f, YuvFrame) and f.clip is f0.clip and f.index == f0.index + k for k, f in enumerate(sample)):
            return f0.clip.host_bgr(f0.index, len(sample))          # one pass over one contiguous range of raw bytes
        return np.stack([np.asarray(f) for f in sample])
    if isinstance(f0, np.ndarray) and f0.flags.c_contiguous and f0.dtype == np.uint8 and f0.base is not None:
        fb, p0 = f0.nbytes, f0.ctypes.data
        root = f0.base
        if fb and all(isinstance(f, np.ndarray) and f.base is root and f.shape == f0.shape and f.flags.c_contiguous and
                      f.ctypes.data == p0 + k * fb for k, f in enumerate(sample)):
            return np.lib.stride_tricks.as_strided(f0, shape=(len(sample),) + f0.shape, strides=(fb,) + f0.strides, writeable=False)
    return np.stack(sample)


def host_frame(f) -> np.ndarray:
    """One frame of any source as an (h, w, 3) uint8 array on the host."""
    if isinstance(f, DeviceFrame):
        out = np.empty(f.shape, np.uint8)
        return f.clip.buffer.view(f.index * f.clip.frame_bytes, f.clip.frame_bytes).download(out)
    return np.ascontiguousarray(np.asarray(f), np.uint8)


def sampler(generator, sequence_length: int) -> Iterator[list]:
    """Chop a frame stream into lists of ``sequence_length`` frames; the last one may be short."""
    w: list = []
    for x in generator:
        w.append(x)
        if len(w) == sequence_length:
            yield w
            w = []
    if w:
        yield w


class ResidentBatches:
    """A walk over a clip as batches resident in HBM, and the one owner of the staging memory such a walk needs:
    ``with ResidentBatches(engine, samples, capacity, (h, w)) as walk: for frames, host in walk: ...``.  ``samples``: non-empty lists of
    at most ``capacity`` frames (``sampler``).  ``frames`` are handles ``device_batch`` gives a view over; ``host`` is None for a sample
    that was resident as it came, else the (n, h, w, 3) array that was uploaded.

    * ``DeviceFrame`` handles pass through, not looked at.
    * ``YuvFrame`` / ``MjpegFrame`` handles get one ``device_batch(sample)`` when it is their turn — converted or decoded into their
      clip's own BGR staging — and pass through if that answers.
    * Everything else is staged: ``host_batch(sample)`` goes up behind ``lead`` slots that are the caller's (``staging()`` reaches
      them); ``frames`` are ``DeviceFrame(staging, lead + k)``.

    A staging clip of ``lead + capacity`` frames is created by the first sample that needs one, on ``engine`` (None: the default
    engine, resolved then).  ``prefetch``: two of them, filled by turns on the copy stream by a worker thread that starts with the
    first; host frames go up before the sample in front of them is handed out, and a sample's bytes stay until the next one is asked
    for.  A sample is made resident when it is drawn, so who reads only some (``identity.scan``) leaves the others out of ``samples``.
    Leaving the ``with`` — at the end, by an error, by a ``break`` — joins the worker, synchronises the engine, then frees the staging."""

    def __init__(self, engine, samples, capacity: int, hw: tuple, lead: int = 0, prefetch: bool = False):
        self.engine, self._samples, self._lead, self._prefetch = engine, iter(samples), int(lead), bool(prefetch)
        self._shape = (self._lead + int(capacity), int(hw[0]), int(hw[1]), 3)
        self._clips, self._pool, self._uploads = [], None, 0

    def __enter__(self) -> "ResidentBatches":
        return self

    def __exit__(self, *exc) -> None:
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
        if self.engine is not None:
            self.engine.synchronize()                # readers of the staging may still be queued
        while self._clips:
            self._clips.pop().free()

    def staging(self, k: int = 0) -> DeviceClip:
        """Staging clip ``k``, created if need be."""
        while len(self._clips) <= k:
            if self.engine is None:
                from . import engine as E
                self.engine = E.default_engine()
            self._clips.append(DeviceClip(self.engine, shape=self._shape))
        return self._clips[k]

    def _stage(self, sample, clip: DeviceClip) -> tuple:
        host = host_batch(sample)
        clip.upload(host, first=self._lead, copy_stream=self._prefetch)
        return [DeviceFrame(clip, self._lead + k) for k in range(len(sample))], host

    def _submit(self, sample):
        """The upload of ``sample`` on the worker thread, into the staging clip the upload before it did not take."""
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=1)
        self._uploads += 1
        return self._pool.submit(self._stage, sample, self.staging(self._uploads % 2))

    def _resident(self, sample) -> Optional[tuple]:
        """``(sample, None)`` if its frames are in HBM as they are (after their conversion), else None."""
        f = sample[0]
        return (sample, None) if isinstance(f, DeviceFrame) or (isinstance(f, YuvFrame) and device_batch(sample) is not None) else None

    def __iter__(self):
        if not self._prefetch:
            for sample in self._samples:
                yield self._resident(sample) or self._stage(sample, self.staging())
            return
        # one sample ahead: `fut` is the upload of `nxt`, if `nxt` is host frames (handles are resolved at their turn: a clip's
        # own staging holds one range)
        ahead = lambda s: None if s is None or isinstance(s[0], (DeviceFrame, YuvFrame)) else self._submit(s)
        nxt = next(self._samples, None)
        fut = ahead(nxt)
        while nxt is not None:
            cur, cur_fut = nxt, fut
            nxt = next(self._samples, None)
            fut = ahead(nxt)
            yield cur_fut.result() if cur_fut is not None else self._resident(cur) or self._submit(cur).result()


def get_video_frames_generator(source_path, stride: int = 1, start: int = 0, end: Optional[int] = None) -> Iterator[np.ndarray]:
    if isinstance(source_path, (DeviceClip, ArrayClip, _StagedSource)):
        yield from source_path.frames(start, end, stride)
        return
    p = str(source_path)
    src = _scheme(p)
    if src is not None:
        yield from src[1](p, start, end, stride)
        return
    if p.endswith(".y4m"):
        yield from _open_y4m(p).frames(start, end, stride)
        return
    if p.endswith(".npy"):
        a = np.load(p, mmap_mode="r")
        stop = a.shape[0] if end is None else min(end, a.shape[0])
        for i in range(start, stop, stride):
            yield np.ascontiguousarray(a[i])
        return
    c = _open_mjpeg(p)
    if c is not None:
        yield from c.frames(start, end, stride)
        return
    cv2 = _cv2()
    cap = cv2.VideoCapture(p)
    total = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
    stop = total if end is None else min(end, total)
    cap.set(cv2.CAP_PROP_POS_FRAMES, start)
    i = start
    while i < stop:
        ok, frame = cap.read()
        if not ok:
            break
        if (i - start) % stride == 0:
            yield frame
        i += 1
    cap.release()
