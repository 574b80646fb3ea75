"""ctypes binding of ``libpadel_hip.so`` (C-ABI: ``include/padel_hip.h``).

This is the only place the package talks to the GPU.  There is deliberately NO CPU fallback: if
the shared library or a GPU is missing every entry point raises ``EngineUnavailable`` (the product
path must fail loudly rather than silently route through a CPU restatement).
"""
from __future__ import annotations

import ctypes as C
import sys as _sys
import os
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import graph as G

# PADEL_LIB: tuning tools only (A/B runs against a second build of the library, e.g. tools/ab/*.so)
_LIB_PATH = Path(os.environ["PADEL_LIB"]).resolve() if os.environ.get("PADEL_LIB") else Path(__file__).resolve().parent / "libpadel_hip.so"
_lib = None


class EngineUnavailable(RuntimeError):
    pass


class EngineError(RuntimeError):
    pass


class RangeOverflow(EngineError):
    """An activation of an h2 model (fp16 pairs, |x| <= 65504) did not fit: the results of that call are invalid and
    the caller repeats it on the full-range fp32 (bf16x3) model (yolo.py / trackers/ball_tracker.py do)."""


def fp32_mode() -> str:
    """Arithmetic of the fp32-equivalent path: "h2" (default: fp16 pairs, three MFMA products, csrc/h2_common.h) or
    "bx3" (exact bf16 triples, six products: full fp32 range, the fallback of the former).  PADEL_FP32_MODE overrides."""
    m = os.environ.get("PADEL_FP32_MODE", "h2").lower()
    if m not in ("h2", "bx3"):
        raise ValueError(f"PADEL_FP32_MODE={m!r}: expected 'h2' or 'bx3'")
    return m


class pa_buf_desc(C.Structure):
    _fields_ = [("level", C.c_int32), ("channels", C.c_int32)]


class pa_op_desc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("in_buf", C.c_int32), ("in_choff", C.c_int32), ("cin", C.c_int32),
                ("out_buf", C.c_int32), ("out_choff", C.c_int32), ("cout", C.c_int32),
                ("ksize", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32),
                ("res_buf", C.c_int32), ("res_choff", C.c_int32), ("npad", C.c_int32), ("reserved", C.c_int32),
                ("w_off", C.c_int64), ("b_off", C.c_int64), ("flags", C.c_int32), ("pad_", C.c_int32)]


class pa_model_desc(C.Structure):
    _fields_ = [("task", C.c_int32), ("nc", C.c_int32), ("nk", C.c_int32), ("kpt_dim", C.c_int32),
                ("n_bufs", C.c_int32), ("bufs", C.POINTER(pa_buf_desc)),
                ("n_ops", C.c_int32), ("ops", C.POINTER(pa_op_desc)),
                ("head_buf", C.c_int32 * 3), ("in_channels", C.c_int32), ("dtype", C.c_int32)]


class pa_yolo_params(C.Structure):
    _fields_ = [("imgsz", C.c_int32), ("pre_mode", C.c_int32), ("channel_reverse", C.c_int32),
                ("letterbox_auto", C.c_int32), ("conf", C.c_float), ("iou", C.c_float),
                ("max_det", C.c_int32), ("n_classes", C.c_int32), ("classes", C.POINTER(C.c_int32)),
                ("frames_on_device", C.c_int32)]


class pa_yuv_desc(C.Structure):
    _fields_ = [("layout", C.c_int32), ("pitch_y", C.c_int32), ("pitch_c", C.c_int32), ("off_u", C.c_int32),
                ("off_v", C.c_int32), ("reserved", C.c_int32), ("frame_stride", C.c_int64),
                ("y_off", C.c_int32), ("cy", C.c_int32), ("cvr", C.c_int32), ("cug", C.c_int32), ("cvg", C.c_int32),
                ("cub", C.c_int32)]


class pa_mark(C.Structure):
    _fields_ = [("kind", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("size", C.c_int32), ("bgr", C.c_uint32), ("arg", C.c_int32)]


class pa_yuv_enc(C.Structure):
    _fields_ = [("y_off", C.c_int32), ("yr", C.c_int32), ("yg", C.c_int32), ("yb", C.c_int32), ("ur", C.c_int32), ("ug", C.c_int32),
                ("ub", C.c_int32), ("vr", C.c_int32), ("vg", C.c_int32), ("vb", C.c_int32)]


#: numpy view of ``pa_mark`` (32 bytes): what ``render.pack`` returns and ``Engine.render`` takes
MARK_DTYPE = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"), ("bgr", "<u4"),
                       ("arg", "<i4")])
MARK_DISC, MARK_SEGMENT, MARK_FILL, MARK_BOX, MARK_GLYPH, MARK_BLEND = 1, 2, 3, 4, 5, 6
MARK_ARC = 8                                       # (7 and 9 are no kinds)
RENDER_BGR, RENDER_YUV420 = 0, 1
#: ``Engine.render_last_path()``
RENDER_PATH_VECTOR, RENDER_PATH_BYTE = 1, 2

PRE_LETTERBOX, PRE_PIL_STRETCH = 0, 1
YUV_NV12, YUV_I420 = 0, 1
#: ``Model.last_post_path()``: decode_kernel over head maps, or the heads' last convs + decode as one kernel
POST_PATH_DECODE, POST_PATH_FUSED = 0, 1
#: ``Engine.yuv_last_path()``: which instantiation of the conversion kernel the launcher chose
YUV_PATH_VECTOR, YUV_PATH_BYTE = 1, 2

# every symbol include/padel_hip.h declares (tests check the .so exports all of them)
ABI_SYMBOLS = [
    "pa_abi_version", "pa_device_count", "pa_engine_create", "pa_engine_destroy", "pa_last_error",
    "pa_engine_synchronize", "pa_device_malloc", "pa_device_free", "pa_memcpy_h2d", "pa_memcpy_d2h",
    "pa_model_create", "pa_model_destroy", "pa_model_set_max_batch", "pa_yolo_infer", "pa_yolo_head_shape",
    "pa_yolo_read_head", "pa_tracknet_infer", "pa_engine_set_profiling", "pa_model_last_profile",
    "pa_model_profile_text", "pa_ball_create", "pa_ball_destroy", "pa_ball_set_background", "pa_ball_feed",
    "pa_ball_locate", "pa_ball_background_from_frames",
    "pa_upload", "pa_engine_set_tuning", "pa_engine_set_timeline_path", "pa_model_plan_bytes",
    "pa_yolo_netin_shape", "pa_yolo_read_netin",
    "pa_comm_unique_id", "pa_engine_comm_init", "pa_engine_comm_destroy", "pa_engine_bcast_weights",
    "pa_engine_bcast", "pa_engine_allreduce_max", "pa_engine_gather_sizes", "pa_engine_gather",
    "pa_bytetrack_create", "pa_bytetrack_destroy", "pa_bytetrack_reset", "pa_bytetrack_update_batch",
    "pa_model_take_overflow", "pa_yolo_postprocess", "pa_host_register", "pa_host_unregister",
    "pa_engine_bcast_weights_from", "pa_model_fill_arena", "pa_yolo_submit", "pa_yolo_wait",
    "pa_resnet_infer", "pa_resnet_read_netin", "pa_resnet_read_fc", "pa_resnet_read_head", "pa_pil_coeffs",
    "pa_yuv420_to_bgr", "pa_yuv_last_path", "pa_engine_timer_start", "pa_engine_timer_stop",
    "pa_render", "pa_render_check", "pa_render_last_path", "pa_glyph_rows", "pa_ball_read_resized",
    "pa_jpeg_encode", "pa_jpeg_check", "pa_jpeg_interval_bytes",
    "pa_jpeg_parse", "pa_jpeg_decode", "pa_jpeg_decode_last_path", "pa_jpeg_decode_last_times",
    "pa_yolo_last_post_path", "pa_jpeg_decode_set_split", "pa_jpeg_decode_last_split",
    "pa_model_lanes_allocated", "pa_model_last_lane", "pa_model_last_stem_path", "pa_yolo_resample_passes", "pa_device_bytes_live",
    "pa_frame_activity", "pa_frame_activity_check", "pa_frames_median",
    "pa_box_histograms", "pa_box_histograms_check",
    "pa_render_scaled", "pa_render_scaled_check",
    "pa_warp_perspective", "pa_warp_check", "pa_warp_last_path",
    "pa_heat_accumulate", "pa_heat_check", "pa_heat_last_path",
]


def lib_path() -> Path:
    return _LIB_PATH


def load_library():
    """dlopen libpadel_hip.so (once).  torch is imported first so that the process holds a single
    HIP runtime (torch's bundled libamdhip64.so.7 satisfies our DT_NEEDED by SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise EngineUnavailable(f"{_LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
    if os.environ.get("PADEL_HIP_STANDALONE") != "1":
        import torch  # noqa: F401  (shares one libamdhip64 with RCCL/torch.distributed users)
    lib = C.CDLL(str(_LIB_PATH))
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.pa_abi_version.restype = i32
    lib.pa_device_count.restype = i32
    lib.pa_engine_create.argtypes = [i32, C.POINTER(vp)]
    lib.pa_engine_destroy.argtypes = [vp]
    lib.pa_engine_destroy.restype = None
    lib.pa_last_error.argtypes = [vp]
    lib.pa_last_error.restype = C.c_char_p
    lib.pa_engine_synchronize.argtypes = [vp]
    lib.pa_device_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.pa_device_free.argtypes = [vp, vp]
    lib.pa_device_bytes_live.argtypes = []
    lib.pa_device_bytes_live.restype = sz
    lib.pa_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    lib.pa_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    lib.pa_model_create.argtypes = [vp, C.POINTER(pa_model_desc), vp, sz, C.POINTER(vp)]
    lib.pa_model_destroy.argtypes = [vp]
    lib.pa_model_destroy.restype = None
    lib.pa_model_set_max_batch.argtypes = [vp, i32]
    lib.pa_yolo_infer.argtypes = [vp, vp, i32, i32, i32, C.POINTER(pa_yolo_params), vp, vp, vp]
    lib.pa_yolo_submit.argtypes = [vp, vp, i32, i32, i32, C.POINTER(pa_yolo_params), vp, vp, vp, C.POINTER(C.c_int)]
    lib.pa_yolo_wait.argtypes = [vp, i32, C.POINTER(C.c_int)]
    lib.pa_yolo_head_shape.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.pa_yolo_read_head.argtypes = [vp, i32, i32, vp]
    lib.pa_yolo_last_post_path.argtypes = [vp]
    lib.pa_model_lanes_allocated.argtypes = [vp]
    lib.pa_model_last_lane.argtypes = [vp]
    lib.pa_model_last_stem_path.argtypes = [vp]
    lib.pa_yolo_resample_passes.argtypes = [vp]
    lib.pa_tracknet_infer.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32]
    lib.pa_resnet_infer.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    lib.pa_resnet_read_netin.argtypes = [vp, i32, vp]
    lib.pa_resnet_read_fc.argtypes = [vp, i32, vp, vp]
    lib.pa_resnet_read_head.argtypes = [vp, i32, vp]
    lib.pa_pil_coeffs.argtypes = [i32, i32, i32, vp, vp, i32, C.POINTER(i32)]
    lib.pa_engine_set_profiling.argtypes = [vp, i32]
    lib.pa_model_last_profile.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.pa_model_profile_text.argtypes = [vp, C.c_char_p, sz]
    lib.pa_ball_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.pa_ball_destroy.argtypes = [vp]
    lib.pa_ball_destroy.restype = None
    lib.pa_ball_set_background.argtypes = [vp, vp]
    lib.pa_ball_feed.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, C.POINTER(i32)]
    lib.pa_ball_locate.argtypes = [vp, vp, i32, vp]
    lib.pa_ball_background_from_frames.argtypes = [vp, vp, i32, i32, vp]
    lib.pa_ball_read_resized.argtypes = [vp, C.c_longlong, vp]
    lib.pa_upload.argtypes = [vp, vp, vp, sz]
    lib.pa_engine_set_tuning.argtypes = [vp, C.c_char_p, i32]
    lib.pa_engine_set_timeline_path.argtypes = [vp, C.c_char_p]
    lib.pa_model_plan_bytes.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    lib.pa_yolo_netin_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.pa_yolo_read_netin.argtypes = [vp, i32, vp]
    lib.pa_comm_unique_id.argtypes = [vp, sz]
    lib.pa_engine_comm_init.argtypes = [vp, vp, sz, i32, i32]
    lib.pa_engine_comm_destroy.argtypes = [vp]
    lib.pa_engine_comm_destroy.restype = None
    lib.pa_engine_bcast_weights.argtypes = [vp, vp, i32]
    lib.pa_engine_bcast.argtypes = [vp, vp, sz, i32]
    lib.pa_engine_bcast_weights_from.argtypes = [vp, vp, vp, i32]
    lib.pa_engine_allreduce_max.argtypes = [vp, C.POINTER(C.c_double)]
    lib.pa_engine_gather_sizes.argtypes = [vp, sz, C.POINTER(C.c_uint64)]
    lib.pa_engine_gather.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_uint64), i32]
    lib.pa_bytetrack_create.argtypes = [C.c_double, i32, C.c_double, i32, C.POINTER(vp)]
    lib.pa_bytetrack_destroy.argtypes = [vp]
    lib.pa_bytetrack_destroy.restype = None
    lib.pa_bytetrack_reset.argtypes = [vp]
    lib.pa_bytetrack_reset.restype = None
    lib.pa_bytetrack_update_batch.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.pa_model_fill_arena.argtypes = [vp, i32]
    lib.pa_host_register.argtypes = [vp, vp, sz]
    lib.pa_host_unregister.argtypes = [vp, vp]
    lib.pa_model_take_overflow.argtypes = [vp, C.POINTER(i32)]
    lib.pa_yolo_postprocess.argtypes = [vp, C.POINTER(vp), i32, i32, i32, C.POINTER(pa_yolo_params), vp, vp, vp]
    lib.pa_yuv420_to_bgr.argtypes = [vp, vp, i32, i32, i32, i32, C.POINTER(pa_yuv_desc), vp]
    lib.pa_yuv_last_path.argtypes = [vp]
    lib.pa_render.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, C.POINTER(pa_yuv_desc), C.POINTER(pa_yuv_enc), vp]
    lib.pa_render_check.argtypes = [i32, i32, i32, vp, vp, i32, C.POINTER(pa_yuv_desc), C.POINTER(pa_yuv_enc), C.c_char_p, sz]
    lib.pa_render_last_path.argtypes = [vp]
    if hasattr(lib, "pa_render_scaled"):           # (an older build under PADEL_LIB, for an A/B run of what it does have: asking it for a scale raises)
        lib.pa_render_scaled.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, C.POINTER(pa_yuv_desc), C.POINTER(pa_yuv_enc), vp]
        lib.pa_render_scaled_check.argtypes = [i32, i32, i32, vp, vp, i32, i32, C.POINTER(pa_yuv_desc), C.POINTER(pa_yuv_enc), i32, C.c_char_p, sz]
    lib.pa_glyph_rows.argtypes = [i32, vp]
    if hasattr(lib, "pa_warp_perspective"):        # (an older build under PADEL_LIB, likewise: asking it for a warp raises)
        lib.pa_warp_perspective.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.c_uint32, vp, i32, i32]
        lib.pa_warp_check.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_char_p, sz]
        lib.pa_warp_last_path.argtypes = [vp]
    if hasattr(lib, "pa_heat_accumulate"):         # (an older build under PADEL_LIB, likewise: asking it for a heat map raises)
        lib.pa_heat_accumulate.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, i32, C.c_uint32, i32, i32, vp]
        lib.pa_heat_check.argtypes = [i32, i32, i32, i32, vp, vp, vp, i32, C.c_uint32, i32, i32, vp, vp, vp, C.c_char_p, sz]
        lib.pa_heat_last_path.argtypes = [vp]
    lib.pa_jpeg_encode.argtypes = [vp, vp, i32, i32, i32, C.POINTER(pa_yuv_desc), i32, vp, sz, vp]
    lib.pa_jpeg_check.argtypes = [i32, i32, i32, C.POINTER(pa_yuv_desc), i32, C.c_char_p, sz]
    lib.pa_jpeg_interval_bytes.argtypes = [i32]
    lib.pa_jpeg_interval_bytes.restype = sz
    lib.pa_jpeg_parse.argtypes = [vp, sz, C.POINTER(pa_jpeg_frame_info), vp, sz, C.c_char_p, sz]
    lib.pa_jpeg_decode.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.pa_jpeg_decode_last_path.argtypes = [vp]
    lib.pa_jpeg_decode_last_times.argtypes = [vp, vp]
    lib.pa_jpeg_decode_set_split.argtypes = [vp, C.c_int64, i32]
    lib.pa_jpeg_decode_last_split.argtypes = [vp, vp]
    lib.pa_frame_activity_check.argtypes = [i32, i32, i32, vp, i32]
    lib.pa_frame_activity_check.restype = C.c_char_p
    lib.pa_frame_activity.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.pa_frames_median.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.pa_box_histograms_check.argtypes = [i32, i32, i32, vp, i32]
    lib.pa_box_histograms_check.restype = C.c_char_p
    lib.pa_box_histograms.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp]
    lib.pa_engine_timer_start.argtypes = [vp]
    lib.pa_engine_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    if lib.pa_abi_version() != 5:
        raise EngineUnavailable("libpadel_hip.so ABI version mismatch")
    _lib = lib
    return lib


def device_bytes_live() -> int:
    """Device bytes the library holds in this process right now (``pa_device_bytes_live``): everything its models, sessions and
    engines own, not the ``DeviceBuffer`` s of the caller.  It returns to its earlier value when what was created since is closed."""
    return int(load_library().pa_device_bytes_live())


PIL_BICUBIC, PIL_BILINEAR = 0, 1


def pil_coeffs(in_size: int, out_size: int, filter: int = PIL_BICUBIC):
    """(bounds (out, 2) int32 {first input index, taps}, coefs (out, ksize) int32, 22-bit fixed point) of one Pillow resample
    pass as the device kernels use them (``pa_pil_coeffs``: host code, no GPU needed)."""
    lib = load_library()
    ks = C.c_int(0)
    if lib.pa_pil_coeffs(in_size, out_size, filter, None, None, 0, C.byref(ks)) != 0:
        raise EngineError("pa_pil_coeffs: bad arguments")
    bounds = np.zeros((out_size, 2), np.int32)
    coefs = np.zeros((out_size, ks.value), np.int32)
    if lib.pa_pil_coeffs(in_size, out_size, filter, bounds.ctypes.data, coefs.ctypes.data, coefs.size, C.byref(ks)) != 0:
        raise EngineError("pa_pil_coeffs failed")
    return bounds, coefs


def graph_dtype(mode: Optional[str] = None) -> str:
    """graph.build_yolov8 / build_tracknet ``dtype`` of the fp32-equivalent path in arithmetic ``mode`` (default: fp32_mode())."""
    return {"h2": "h2", "bx3": "f32"}[mode or fp32_mode()]


def yuv_span_bytes(n: int, h: int, w: int, d: "pa_yuv_desc") -> Optional[int]:
    """Bytes of the source that ``n`` frames described by ``d`` reach (the last frame's start plus the extent of one frame's
    planes); None where the geometry is one the library refuses anyway."""
    if n < 1 or h < 2 or w < 2 or h % 2 or w % 2 or d.layout not in (YUV_NV12, YUV_I420):
        return None
    crow = w if d.layout == YUV_NV12 else w // 2
    if d.pitch_y < w or d.pitch_c < crow or d.off_u < 0 or d.off_v < 0:
        return None
    c_len = (h // 2 - 1) * d.pitch_c + crow
    extent = max((h - 1) * d.pitch_y + w, d.off_u + c_len, 0 if d.layout == YUV_NV12 else d.off_v + c_len)
    if d.frame_stride < extent:
        return None
    return (n - 1) * d.frame_stride + extent


def glyph_rows(code) -> Optional[np.ndarray]:
    """The 7 rows (top first; column i in bit i, 0 = leftmost) of one glyph of the renderer's 5 x 7 font, None for a character
    the font does not have (``pa_glyph_rows``: host code, no GPU needed)."""
    rows = np.zeros(7, np.uint8)
    code = ord(code) if isinstance(code, str) else int(code)
    return rows if load_library().pa_glyph_rows(code, rows.ctypes.data) == 0 else None


def _render_args(marks, first, geom, enc):
    marks = np.ascontiguousarray(marks, MARK_DTYPE).reshape(-1)
    first = np.ascontiguousarray(first, np.int32).reshape(-1)
    if geom is not None and not isinstance(geom, pa_yuv_desc):
        geom = pa_yuv_desc(**{k: int(v) for k, v in geom.items()})
    if enc is not None and not isinstance(enc, pa_yuv_enc):
        enc = pa_yuv_enc(*(int(c) for c in enc))
    return marks, first, geom, enc


def render_check(n: int, h: int, w: int, marks, first, out: int = RENDER_BGR, geom=None, enc=None, scale: int = 1,
                 in_place: bool = False) -> Optional[str]:
    """None if ``pa_render`` — with ``scale`` other than 1: ``pa_render_scaled``, ``h`` x ``w`` being the source and ``geom`` the
    ``h // scale`` x ``w // scale`` output — would accept the call, else its reason for refusing it (``pa_render_check`` /
    ``pa_render_scaled_check``: host code, no GPU).  ``in_place``: the caller means ``dst`` to be ``src``."""
    marks, first, geom, enc = _render_args(marks, first, geom, enc)
    if first.size != max(int(n), 0) + 1:
        return f"pa_render: first has {first.size} entries, n + 1 = {int(n) + 1} are needed"
    if marks.size < int(first[-1]):
        return f"pa_render: first[] announces {int(first[-1])} marks, marks holds {marks.size}"
    why = C.create_string_buffer(512)
    tail = (C.byref(geom) if geom is not None else None, C.byref(enc) if enc is not None else None)
    head = (int(n), int(h), int(w), marks.ctypes.data if marks.size else None, first.ctypes.data)
    if int(scale) == 1:
        rc = load_library().pa_render_check(*head, int(out), *tail, why, 512)
    else:
        rc = load_library().pa_render_scaled_check(*head, int(scale), int(out), *tail, 1 if in_place else 0, why, 512)
    return why.value.decode() if rc else None


#: ``pa_warp_perspective`` refuses larger frames and canvases (PA_WARP_MAX_DIM)
WARP_MAX_DIM = 4096
#: ``Engine.warp_last_path()``: how the last warp stored its pixels
WARP_PATH_VECTOR, WARP_PATH_BYTE = 1, 2


def _warp_args(n, matrices, valid):
    """(matrices as (n, 9) float64 or None, valid as (n,) int32 or None); ``ValueError`` for another count than ``n`` frames' worth."""
    if matrices is not None:
        matrices = np.ascontiguousarray(matrices, np.float64).reshape(-1)
        if matrices.size != 9 * max(int(n), 0):
            raise ValueError(f"warp: matrices holds {matrices.size} numbers, {n} frames need {9 * max(int(n), 0)}")
    if valid is not None:
        valid = np.ascontiguousarray(valid, np.int32).reshape(-1)
        if valid.size != max(int(n), 0):
            raise ValueError(f"warp: valid holds {valid.size} words, {n} frames need {max(int(n), 0)}")
    return matrices, valid


def fill_word(fill) -> int:
    """(B, G, R) or an integer -> B | G << 8 | R << 16."""
    if isinstance(fill, (tuple, list, np.ndarray)):
        b, g, r = (int(c) & 0xff for c in fill)
        return b | g << 8 | r << 16
    return int(fill) & 0xffffff


def warp_check(n: int, h: int, w: int, oh: int, ow: int, matrices, valid, src: Optional[int] = 1, dst: Optional[int] = 1 << 60) -> Optional[str]:
    """None if ``pa_warp_perspective`` would accept the call, else its reason for refusing it (``pa_warp_check``: host code, no GPU).
    ``src``, ``dst``: the addresses of the frames and of the canvases (compared, never read through; None is NULL, as it is for
    ``matrices`` and ``valid``); the default is a source at address 1 and a destination far behind it."""
    matrices, valid = _warp_args(n, matrices, valid)
    why = C.create_string_buffer(512)
    rc = load_library().pa_warp_check(int(n), int(h), int(w), int(oh), int(ow), None if matrices is None else matrices.ctypes.data,
                                      None if valid is None else valid.ctypes.data, src, dst, why, 512)
    return why.value.decode() if rc else None


#: the limits of ``pa_heat_accumulate`` (PA_HEAT_MAX_POINTS per frame, PA_HEAT_MAX_PLANES, PA_HEAT_MAX_RADIUS, PA_HEAT_MAX_COORD, PA_HEAT_MAX_FULL)
HEAT_MAX_POINTS, HEAT_MAX_PLANES, HEAT_MAX_RADIUS, HEAT_MAX_COORD, HEAT_MAX_FULL = 64, 4, 255, 32767, (1 << 24) - 1
#: ``Engine.heat_last_path()``: how the last heat call moved its pixels
HEAT_PATH_VECTOR, HEAT_PATH_BYTE = 1, 2


def _heat_args(n, points, first, valid, lut):
    """(points as (k, 3) int32 flattened or None, first as (n + 1,) int32 or None, valid as (n,) int32 or None, lut as 768 bytes or
    None); ``ValueError`` for an array of another size than ``n`` frames, the points ``first`` announces, or 256 colours need."""
    n = max(int(n), 0)
    if first is not None:
        first = np.ascontiguousarray(first, np.int32).reshape(-1)
        if first.size != n + 1:
            raise ValueError(f"heat: first has {first.size} entries, n + 1 = {n + 1} are needed")
    if valid is not None:
        valid = np.ascontiguousarray(valid, np.int32).reshape(-1)
        if valid.size != n:
            raise ValueError(f"heat: valid holds {valid.size} words, {n} frames need {n}")
    if points is not None:
        points = np.ascontiguousarray(points, np.int32).reshape(-1)
        if points.size % 3 or (first is not None and points.size < 3 * int(first[-1])):
            raise ValueError(f"heat: points holds {points.size} numbers: (x, y, plane) triples, as many as first[] announces, are needed")
    if lut is not None:
        lut = np.ascontiguousarray(lut, np.uint8).reshape(-1)
        if lut.size != 768:
            raise ValueError(f"heat: the lut holds {lut.size} bytes, 256 colours of B, G, R are 768")
    return points, first, valid, lut


def heat_check(n: int, oh: int, ow: int, planes: int, points, first, valid, r: int, full: int, alpha: int, show_mask: int, lut,
               canvas: Optional[int] = 1, state: Optional[int] = 1 << 60) -> Optional[str]:
    """None if ``pa_heat_accumulate`` would accept the call, else its reason for refusing it (``pa_heat_check``: host code, no GPU).
    ``canvas``, ``state``: the addresses of the canvases and of the maps (compared, never read through; None is NULL, as it is for
    the arrays; empty ``points`` are NULL too); the default is canvases at address 1 and a state far behind them."""
    points, first, valid, lut = _heat_args(n, points, first, valid, lut)
    lib = load_library()
    if not hasattr(lib, "pa_heat_check"):
        raise EngineError("heat_check: this build of the library has no pa_heat_check")
    why = C.create_string_buffer(512)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    rc = lib.pa_heat_check(int(n), int(oh), int(ow), int(planes), ptr(points), ptr(first), ptr(valid), int(r),
                           min(max(int(full), 0), 0xffffffff), int(alpha), int(show_mask), ptr(lut), canvas, state, why, 512)
    return why.value.decode() if rc else None


#: ``pa_frame_activity`` / ``pa_frames_median`` refuse larger frames and longer batches (PA_ACTIVITY_MAX_SIDE, PA_ACTIVITY_MAX_FRAMES)
ACTIVITY_MAX_SIDE, ACTIVITY_MAX_FRAMES = 16384, 65535


def _roi_arg(roi):
    """None, or the rectangle as four int32 (x0, y0, x1, y1)."""
    if roi is None:
        return None
    roi = np.ascontiguousarray(roi, np.int32).reshape(-1)
    if roi.size != 4:
        raise ValueError(f"roi must be (x0, y0, x1, y1), got {roi.size} numbers")
    return roi


def frame_activity_check(n: int, h: int, w: int, roi=None, tau: int = 24) -> Optional[str]:
    """None if ``pa_frame_activity`` would accept these arguments, else its reason for refusing them (``pa_frame_activity_check``:
    host code, no GPU)."""
    roi = _roi_arg(roi)
    why = load_library().pa_frame_activity_check(int(n), int(h), int(w), roi.ctypes.data if roi is not None else None, int(tau))
    return why.decode() if why else None


#: a row of ``pa_box_histograms`` (PA_BOX_HIST_BINS) and the rectangles one call takes at most (PA_BOX_HIST_MAX_RECTS)
BOX_HIST_BINS, BOX_HIST_MAX_RECTS = 512, 16384


def _rects_arg(rects) -> np.ndarray:
    """The rectangle list as a C-contiguous (k, 5) int32 array (frame, x0, y0, x1, y1)."""
    rects = np.ascontiguousarray(rects, np.int32)
    if rects.size == 0:
        return rects.reshape(0, 5)
    if rects.ndim != 2 or rects.shape[1] != 5:
        raise ValueError(f"rects must be (k, 5): frame, x0, y0, x1, y1; got shape {rects.shape}")
    return rects


def box_histograms_check(n: int, h: int, w: int, rects) -> Optional[str]:
    """None if ``pa_box_histograms`` would accept these arguments, else its reason for refusing them (``pa_box_histograms_check``:
    host code, no GPU).  ``rects=None`` stands for a NULL list of one rectangle."""
    if rects is None:
        ptr, k = None, 1
    else:
        rects = _rects_arg(rects)
        ptr, k = (rects.ctypes.data if len(rects) else None), len(rects)
    why = load_library().pa_box_histograms_check(int(n), int(h), int(w), ptr, int(k))
    return why.decode() if why else None


#: ``pa_jpeg_encode`` refuses wider frames (PA_JPEG_MAX_WIDTH)
JPEG_MAX_WIDTH = 2560


def _yuv_desc_arg(desc):
    return desc if desc is None or isinstance(desc, pa_yuv_desc) else pa_yuv_desc(**{k: int(v) for k, v in desc.items()})


def jpeg_check(n: int, h: int, w: int, desc, quality: int = 90) -> Optional[str]:
    """None if ``pa_jpeg_encode`` would accept the call, else its reason for refusing it (``pa_jpeg_check``: host code, no GPU)."""
    desc = _yuv_desc_arg(desc)
    why = C.create_string_buffer(512)
    rc = load_library().pa_jpeg_check(int(n), int(h), int(w), C.byref(desc) if desc is not None else None, int(quality), why, 512)
    return why.value.decode() if rc else None


def jpeg_interval_bytes(w: int) -> int:
    """The most bytes one restart interval (one MCU row) of a JPEG of width ``w`` can take — the capacity of the slot the encode
    kernel writes it to (``pa_jpeg_interval_bytes``: host code, no GPU)."""
    return int(load_library().pa_jpeg_interval_bytes(int(w)))


#: ``pa_jpeg_parse`` / ``pa_jpeg_decode`` refuse larger frames (PA_JPEG_DEC_MAX_DIM)
JPEG_DEC_MAX_DIM = 4096
#: ``Engine.jpeg_decode_last_path()``: how the colour pass of the last decode stored its pixels
JPEG_DEC_PATH_VECTOR, JPEG_DEC_PATH_BYTE = 1, 2
#: the defaults of ``Engine.jpeg_decode_set_split`` (PA_JPEG_DEC_SPLIT_MIN_BYTES, PA_JPEG_DEC_SPLIT_SUB_BYTES)
JPEG_DEC_SPLIT_MIN_BYTES, JPEG_DEC_SPLIT_SUB_BYTES = 7168, 128


class pa_jpeg_huff(C.Structure):
    _fields_ = [("bits", C.c_uint8 * 16), ("vals", C.c_uint8 * 256), ("nvals", C.c_int32)]


class pa_jpeg_interval(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("first_mcu", C.c_int32), ("mcus", C.c_int32)]


class pa_jpeg_frame_info(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("restart_interval", C.c_int32),
                ("n_intervals", C.c_int32), ("default_huffman", C.c_int32), ("status", C.c_int32), ("scan_begin", C.c_int64),
                ("scan_end", C.c_int64), ("quant", (C.c_uint8 * 64) * 3), ("comp_dc", C.c_uint8 * 3), ("comp_ac", C.c_uint8 * 3),
                ("pad_", C.c_uint8 * 2), ("dc", pa_jpeg_huff * 2), ("ac", pa_jpeg_huff * 2)]


def jpeg_parse(jpeg) -> dict:
    """The description ``pa_jpeg_parse`` gives of one baseline JPEG (host code, no GPU), in the form of ``mjpeg.parse_frame``;
    ``ValueError`` with the library's reason for what it refuses."""
    raw = np.frombuffer(bytes(jpeg), np.uint8)
    info, why = pa_jpeg_frame_info(), C.create_string_buffer(512)
    lib = load_library()
    if lib.pa_jpeg_parse(raw.ctypes.data, raw.size, C.byref(info), None, 0, why, 512):
        raise ValueError(why.value.decode())
    ivls = (pa_jpeg_interval * max(info.n_intervals, 1))()
    if lib.pa_jpeg_parse(raw.ctypes.data, raw.size, C.byref(info), ivls, info.n_intervals, why, 512):
        raise ValueError(why.value.decode())
    table = lambda t: (list(t.bits), list(t.vals)[:t.nvals])
    return dict(w=info.w, h=info.h, mcus_x=info.mcus_x, mcus_y=info.mcus_y, restart_interval=info.restart_interval,
                n_intervals=info.n_intervals, default_huffman=info.default_huffman, status=info.status, scan_begin=info.scan_begin,
                scan_end=info.scan_end, quant=np.array([list(q) for q in info.quant], np.uint8), comp_dc=list(info.comp_dc),
                comp_ac=list(info.comp_ac), dc=[table(t) for t in info.dc], ac=[table(t) for t in info.ac],
                intervals=[(v.begin, v.end, v.first_mcu, v.mcus) for v in ivls[:info.n_intervals]])


class DeviceBuffer:
    """Raw HBM allocation owned by an Engine (bench keeps frame batches resident with it).  ``view(off, n)``
    gives a non-owning window of the same memory (a batch of frames inside a resident clip)."""

    def __init__(self, engine: "Engine", nbytes: int, _ptr: Optional[int] = None):
        self.engine, self.nbytes = engine, nbytes
        self.owner = _ptr is None
        if _ptr is None:
            p = C.c_void_p()
            engine._check(engine.lib.pa_device_malloc(engine.handle, nbytes, C.byref(p)))
            _ptr = p.value
        self.ptr = _ptr

    def view(self, offset: int, nbytes: int) -> "DeviceBuffer":
        assert 0 <= offset and offset + nbytes <= self.nbytes
        return DeviceBuffer(self.engine, nbytes, _ptr=self.ptr + offset)

    def upload(self, arr: np.ndarray, copy_stream: bool = False) -> "DeviceBuffer":
        """copy_stream=True: use the engine's copy stream (pa_upload) — the copy does not queue behind inference
        launched from another host thread."""
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        f = self.engine.lib.pa_upload if copy_stream else self.engine.lib.pa_memcpy_h2d
        self.engine._check(f(self.engine.handle, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, arr: np.ndarray) -> np.ndarray:
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        self.engine._check(self.engine.lib.pa_memcpy_d2h(self.engine.handle, arr.ctypes.data, self.ptr, arr.nbytes))
        return arr

    def free(self):
        if self.ptr and self.owner:
            self.engine.lib.pa_device_free(self.engine.handle, self.ptr)
        self.ptr = None


class Engine:
    """One engine (HIP stream + device) per GPU."""

    def __init__(self, device_id: int = 0):
        self.lib = load_library()
        if self.lib.pa_device_count() <= 0:
            raise EngineUnavailable("no HIP device visible: the padel_analytics_amd engine needs an AMD GPU (gfx950)")
        h = C.c_void_p()
        if self.lib.pa_engine_create(device_id, C.byref(h)) != 0:
            raise EngineUnavailable(self.lib.pa_last_error(None).decode())
        self.handle = h
        self.device_id = device_id

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(self.lib.pa_last_error(self.handle).decode())

    def synchronize(self):
        self._check(self.lib.pa_engine_synchronize(self.handle))

    def set_profiling(self, on: bool):
        self._check(self.lib.pa_engine_set_profiling(self.handle, 1 if on else 0))
        self.profiling = bool(on)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def pin(self, arr: np.ndarray) -> None:
        """Page-lock a host array in place (hipHostRegister): uploads from it run at PCIe speed.  unpin() before freeing."""
        assert arr.flags.c_contiguous
        self._check(self.lib.pa_host_register(self.handle, arr.ctypes.data, arr.nbytes))

    def unpin(self, arr: np.ndarray) -> None:
        self._check(self.lib.pa_host_unregister(self.handle, arr.ctypes.data))

    def yuv420_to_bgr(self, src, n: int, h: int, w: int, desc, dst: DeviceBuffer) -> None:
        """``n`` frames of 8-bit YUV 4:2:0 -> packed BGR in ``dst`` (``pa_yuv420_to_bgr``).  ``src``: a 1-D uint8 ndarray of
        raw bytes (copied to the engine's staging buffer on the compute stream first) or a ``DeviceBuffer``; ``desc``: a
        ``pa_yuv_desc`` or a dict of its fields (``video.yuv_desc`` builds one).  Asynchronous: ordered with every later call
        of this engine by its one compute stream.  Geometry the kernel cannot run is an ``EngineError``, nothing is launched."""
        if not isinstance(desc, pa_yuv_desc):
            desc = pa_yuv_desc(**{k: int(v) for k, v in desc.items()})
        on_dev = isinstance(src, DeviceBuffer)
        if on_dev:
            ptr, have = src.ptr, src.nbytes
        else:
            if not (isinstance(src, np.ndarray) and src.dtype == np.uint8 and src.ndim == 1 and src.flags.c_contiguous):
                raise TypeError("yuv420_to_bgr: src must be a contiguous 1-D uint8 array of raw bytes or a DeviceBuffer")
            ptr, have = src.ctypes.data, src.nbytes
        need = yuv_span_bytes(n, h, w, desc)
        if need is not None and have < need:          # (geometry that has no span is refused by the library, with its reason)
            raise EngineError(f"yuv420_to_bgr: {n} frames as described span {need} bytes, src holds {have}")
        if n >= 1 and h >= 1 and w >= 1 and dst.nbytes < n * h * w * 3:
            raise EngineError(f"yuv420_to_bgr: dst holds {dst.nbytes} bytes, {n} BGR frames need {n * h * w * 3}")
        self._check(self.lib.pa_yuv420_to_bgr(self.handle, ptr, int(on_dev), int(n), int(h), int(w), C.byref(desc), dst.ptr))

    def yuv_last_path(self) -> int:
        """YUV_PATH_VECTOR / YUV_PATH_BYTE: what the last successful ``yuv420_to_bgr`` launched (0: none yet)."""
        return int(self.lib.pa_yuv_last_path(self.handle))

    def render(self, src: DeviceBuffer, n: int, h: int, w: int, marks, first, dst: DeviceBuffer, out: int = RENDER_BGR, geom=None,
               enc=None, scale: int = 1) -> None:
        """Draw ``marks`` on ``n`` packed BGR frames of ``h`` x ``w`` in ``src`` and write them to ``dst`` as packed BGR or, with
        ``out=RENDER_YUV420``, as 8-bit YUV 4:2:0 laid out by ``geom`` (a ``pa_yuv_desc`` or a dict of its fields: ``video.yuv_desc``)
        with the encode table ``enc`` (``pa_yuv_enc`` or its ten integers: ``video.YUV_ENC_COEFFS``) — ``pa_render``.  ``marks``: an
        array of ``MARK_DTYPE`` records, frame i owning ``marks[first[i]:first[i + 1]]`` (``render.pack`` builds both).  ``dst`` may be
        ``src`` itself for BGR output (in place).  Asynchronous: ordered with every later call of this engine by its one compute
        stream; the mark arrays are consumed before the call returns.  What the kernel cannot run is an ``EngineError``, nothing is
        launched.
        ``scale`` 2, 3 or 4 (``pa_render_scaled``): the frames come out at ``h // scale`` x ``w // scale``, every output pixel the
        rounded mean of the ``scale`` x ``scale`` rendered source pixels under it; the marks stay in source pixels, ``geom`` and
        ``dst`` are the output's, ``h`` and ``w`` must be multiples of ``scale``, and ``dst`` may not be ``src``."""
        marks, first, geom, enc = _render_args(marks, first, geom, enc)
        scale = int(scale)
        if first.size != max(int(n), 0) + 1:
            raise EngineError(f"render: first has {first.size} entries, n + 1 = {int(n) + 1} are needed")
        if marks.size < int(first[-1]):
            raise EngineError(f"render: first[] announces {int(first[-1])} marks, marks holds {marks.size}")
        if n >= 1 and h >= 1 and w >= 1 and src.nbytes < n * h * w * 3:
            raise EngineError(f"render: src holds {src.nbytes} bytes, {n} BGR frames need {n * h * w * 3}")
        # (a scale the library refuses has no output size: it says why)
        ho, wo = (h // scale, w // scale) if 1 <= scale <= 4 and h % scale == 0 and w % scale == 0 else (0, 0)
        if out == RENDER_YUV420 and geom is not None:
            need = yuv_span_bytes(n, ho, wo, geom)
        else:
            need = n * ho * wo * 3 if (n >= 1 and ho >= 1 and wo >= 1) else None
        if need is not None and dst.nbytes < need:     # (geometry that has no span is refused by the library, with its reason)
            raise EngineError(f"render: {n} frames as described span {need} bytes, dst holds {dst.nbytes}")
        tail = (C.byref(geom) if geom is not None else None, C.byref(enc) if enc is not None else None, dst.ptr)
        head = (self.handle, src.ptr, int(n), int(h), int(w), marks.ctypes.data if marks.size else None, first.ctypes.data)
        if scale == 1:
            self._check(self.lib.pa_render(*head, int(out), *tail))
        else:
            self._check(self.lib.pa_render_scaled(*head, scale, int(out), *tail))

    def render_last_path(self) -> int:
        """RENDER_PATH_VECTOR / RENDER_PATH_BYTE: what the last successful ``render`` launched (0: none yet)."""
        return int(self.lib.pa_render_last_path(self.handle))

    def warp(self, src: DeviceBuffer, n: int, h: int, w: int, matrices, valid, dst: DeviceBuffer, oh: int, ow: int, fill=(0, 0, 0)) -> None:
        """``n`` packed BGR frames of ``h`` x ``w`` in ``src`` -> ``n`` packed BGR frames of ``oh`` x ``ow`` in ``dst``, frame i through
        its own 3 x 3 matrix ``matrices[i]`` that takes CANVAS pixels to SOURCE pixels (float64; bilinear with weights in 1 / 32 pixel:
        include/padel_hip.h, ``pa_warp_perspective``; the numpy twin is ``topdown.warp_host``).  A frame with ``valid[i] == 0``, and every
        pixel that falls outside the source or behind the horizon, is ``fill`` (B, G, R).  Not in place.  Asynchronous: ordered with
        every later call of this engine by its one compute stream; the arrays are consumed before the call returns.  What the
        kernel cannot run is an ``EngineError``, nothing is launched."""
        matrices, valid = _warp_args(n, matrices, valid)
        if n >= 1 and h >= 1 and w >= 1 and src.nbytes < n * h * w * 3:
            raise EngineError(f"warp: src holds {src.nbytes} bytes, {n} BGR frames need {n * h * w * 3}")
        if n >= 1 and oh >= 1 and ow >= 1 and dst.nbytes < n * oh * ow * 3:
            raise EngineError(f"warp: dst holds {dst.nbytes} bytes, {n} BGR canvases need {n * oh * ow * 3}")
        if not hasattr(self.lib, "pa_warp_perspective"):
            raise EngineError("warp: this build of the library has no pa_warp_perspective")
        self._check(self.lib.pa_warp_perspective(self.handle, src.ptr, int(n), int(h), int(w), None if matrices is None else matrices.ctypes.data,
                                                 None if valid is None else valid.ctypes.data, fill_word(fill), dst.ptr, int(oh), int(ow)))

    def warp_last_path(self) -> int:
        """WARP_PATH_VECTOR (16 bytes at a time) / WARP_PATH_BYTE: what the last successful ``warp`` launched (0: none yet)."""
        return int(self.lib.pa_warp_last_path(self.handle))

    def heat(self, canvas: DeviceBuffer, n: int, oh: int, ow: int, state: DeviceBuffer, planes: int, points, first, valid, r: int,
             full: int, alpha: int, show_mask: int, lut) -> None:
        """Add the ``points`` of ``n`` frames to the ``planes`` density maps of ``oh`` x ``ow`` uint32 in ``state`` and blend the maps,
        as they stand after each frame, into that frame's packed BGR canvas in ``canvas``, in place (``pa_heat_accumulate``,
        include/padel_hip.h; the numpy twin is ``heatmap.accumulate_host``).  ``points``: (x, y, plane) int32 triples, frame i owning
        ``points[first[i]:first[i + 1]]``; ``valid[i] == 0`` leaves canvas i alone; ``r`` the splat's radius, ``full`` the density shown
        at level 255, ``alpha`` 0..256 (0: the state alone), ``show_mask`` the planes summed for display, ``lut`` 256 x 3 bytes of BGR.
        ``state`` is the caller's: zero at the start, carried from call to call.  Asynchronous: ordered with every later call of this
        engine by its one compute stream; the arrays are consumed before the call returns.  What the kernel cannot run is an
        ``EngineError``, nothing is launched."""
        points, first, valid, lut = _heat_args(n, points, first, valid, lut)
        if n >= 1 and oh >= 1 and ow >= 1 and canvas.nbytes < n * oh * ow * 3:
            raise EngineError(f"heat: canvas holds {canvas.nbytes} bytes, {n} BGR canvases need {n * oh * ow * 3}")
        if 1 <= planes <= HEAT_MAX_PLANES and oh >= 1 and ow >= 1 and state.nbytes < planes * oh * ow * 4:
            raise EngineError(f"heat: state holds {state.nbytes} bytes, {planes} maps need {planes * oh * ow * 4}")
        if not hasattr(self.lib, "pa_heat_accumulate"):
            raise EngineError("heat: this build of the library has no pa_heat_accumulate")
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        self._check(self.lib.pa_heat_accumulate(self.handle, canvas.ptr, int(n), int(oh), int(ow), state.ptr, int(planes), ptr(points),
                                                ptr(first), ptr(valid), int(r), min(max(int(full), 0), 0xffffffff), int(alpha),
                                                int(show_mask), ptr(lut)))

    def heat_last_path(self) -> int:
        """HEAT_PATH_VECTOR (16 bytes at a time) / HEAT_PATH_BYTE: what the last successful ``heat`` launched (0: none yet)."""
        return int(self.lib.pa_heat_last_path(self.handle))

    def frame_activity(self, src: DeviceBuffer, n: int, h: int, w: int, ref: DeviceBuffer, prev: Optional[DeviceBuffer] = None, roi=None,
                       tau: int = 24, out: Optional[np.ndarray] = None) -> np.ndarray:
        """(n, 3) uint64 — ``sad_ref``, ``changed``, ``sad_prev`` of each of the ``n`` packed BGR frames of ``h`` x ``w`` in ``src``
        against the reference image ``ref`` and the frame before it (``prev`` for frame 0; without it ``sad_prev[0]`` is 0), over
        the half-open rectangle ``roi = (x0, y0, x1, y1)`` (None: the whole frame) — ``pa_frame_activity``; the specification is
        ``include/padel_hip.h``, its executable form ``activity.frame_activity_host``.  Synchronous, on the compute stream.  ``out``:
        a C-contiguous uint64 array of at least ``n`` rows of 3 to write into (rows beyond ``n`` stay as they are).  What the
        library refuses (``frame_activity_check``) is an ``EngineError``, nothing is launched."""
        roi = _roi_arg(roi)
        why = frame_activity_check(n, h, w, roi, tau)
        if why is not None:
            raise EngineError(why)
        fb = h * w * 3
        if src.nbytes < n * fb:
            raise EngineError(f"frame_activity: src holds {src.nbytes} bytes, {n} BGR frames need {n * fb}")
        for name, buf in (("ref", ref), ("prev", prev)):
            if buf is not None and buf.nbytes < fb:
                raise EngineError(f"frame_activity: {name} holds {buf.nbytes} bytes, one BGR frame needs {fb}")
        if out is None:
            out = np.zeros((n, 3), np.uint64)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous and out.ndim == 2
                  and out.shape[1] == 3 and out.shape[0] >= n):
            raise EngineError("frame_activity: out must be a C-contiguous uint64 array of at least n rows of 3")
        self._check(self.lib.pa_frame_activity(self.handle, src.ptr, int(n), int(h), int(w), ref.ptr, prev.ptr if prev is not None else None,
                                               roi.ctypes.data if roi is not None else None, int(tau), out.ctypes.data))
        return out

    def box_histograms(self, src: DeviceBuffer, n: int, h: int, w: int, rects, out: Optional[np.ndarray] = None) -> np.ndarray:
        """(k, 512) uint32 — for each of the ``k`` rectangles ``rects[j] = (frame, x0, y0, x1, y1)``, half-open, of the ``n`` packed
        BGR frames of ``h`` x ``w`` in ``src``, the number of its pixels per colour bin ``((B >> 5) << 6) | ((G >> 5) << 3) | (R >> 5)``
        — ``pa_box_histograms``; the specification is ``include/padel_hip.h``, its executable form
        ``identity.box_histograms_host``.  Synchronous, on the compute stream.  ``out``: a C-contiguous uint32 array of at least
        ``k`` rows of 512 to write into (rows beyond ``k`` stay as they are).  What the library refuses (``box_histograms_check``)
        is an ``EngineError``, nothing is launched."""
        if rects is None:
            raise EngineError(box_histograms_check(n, h, w, None))
        rects = _rects_arg(rects)
        k = len(rects)
        why = box_histograms_check(n, h, w, rects)
        if why is not None:
            raise EngineError(why)
        if src.nbytes < n * h * w * 3:
            raise EngineError(f"box_histograms: src holds {src.nbytes} bytes, {n} BGR frames need {n * h * w * 3}")
        if out is None:
            out = np.zeros((k, BOX_HIST_BINS), np.uint32)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous and out.ndim == 2
                  and out.shape[1] == BOX_HIST_BINS and out.shape[0] >= k):
            raise EngineError("box_histograms: out must be a C-contiguous uint32 array of at least k rows of 512")
        self._check(self.lib.pa_box_histograms(self.handle, src.ptr, int(n), int(h), int(w), rects.ctypes.data if k else None, int(k),
                                               out.ctypes.data))
        return out

    def frames_median(self, src: DeviceBuffer, n: int, h: int, w: int, out: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """The per-pixel, per-channel median of ``n`` packed BGR frames in ``src`` — ``np.median(frames, 0).astype(np.uint8)``, BGR —
        into ``out`` (allocated if None; the caller frees it), ``pa_frames_median``.  Synchronous."""
        fb = h * w * 3
        if n >= 1 and h >= 1 and w >= 1 and src.nbytes < n * fb:
            raise EngineError(f"frames_median: src holds {src.nbytes} bytes, {n} BGR frames need {n * fb}")
        own = out is None
        if own:
            out = self.alloc(max(fb, 1))
        elif out.nbytes < fb:
            raise EngineError(f"frames_median: out holds {out.nbytes} bytes, one BGR frame needs {fb}")
        try:
            self._check(self.lib.pa_frames_median(self.handle, src.ptr, int(n), int(h), int(w), out.ptr))
        except EngineError:
            if own:
                out.free()
            raise
        return out

    def jpeg_encode(self, buffer: DeviceBuffer, n: int, h: int, w: int, desc, quality: int = 90, out: Optional[np.ndarray] = None):
        """``n`` frames of 8-bit YUV 4:2:0 in ``buffer``, laid out by ``desc`` (a ``pa_yuv_desc`` or a dict of its fields; what
        ``render`` wrote with ``out=RENDER_YUV420``, ``enc`` = ``video.YUV_ENC_COEFFS["bt601_full"]``), -> (the baseline JPEGs back to
        back as a uint8 array, offsets (n + 1,) int64: frame i is ``bytes[offsets[i]:offsets[i + 1]]``) — ``pa_jpeg_encode``, the same
        bytes as ``mjpeg.encode_host``.  Ordered behind the ``render`` that produced ``buffer`` by the engine's compute stream;
        returns when the bytes are on the host.  ``out``: a 1-D uint8 array to write into (the result is a view of it); if it is too
        small nothing is written and the ``EngineError`` carries the size in ``.needed``.  Without ``out`` the array is sized by a
        guess and, if that was too small, the call is repeated once with the size it asked for."""
        desc = _yuv_desc_arg(desc)
        need = yuv_span_bytes(n, h, w, desc)
        if need is not None and buffer.nbytes < need:   # (geometry that has no span is refused by the library, with its reason)
            raise EngineError(f"jpeg_encode: {n} frames as described span {need} bytes, the buffer holds {buffer.nbytes}")
        offsets = np.zeros(max(int(n), 0) + 1, np.int64)
        own = out is None
        if own:
            out = np.empty(max(int(n), 1) * (max(int(h), 1) * max(int(w), 1) // 4 + 4096), np.uint8)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.ndim == 1 and out.flags.c_contiguous):
            raise TypeError("jpeg_encode: out must be a contiguous 1-D uint8 array")
        for attempt in (0, 1):
            rc = self.lib.pa_jpeg_encode(self.handle, buffer.ptr, int(n), int(h), int(w), C.byref(desc), int(quality), out.ctypes.data,
                                         out.size, offsets.ctypes.data)
            if rc == 0:
                return out[:int(offsets[-1])], offsets
            needed = int(offsets[-1])
            if needed <= out.size or not own or attempt:
                err = EngineError(self.lib.pa_last_error(self.handle).decode())
                err.needed = needed if needed > out.size else None
                raise err
            out = np.empty(needed, np.uint8)

    def jpeg_decode(self, data, offsets, dst: DeviceBuffer, h: Optional[int] = None, w: Optional[int] = None) -> np.ndarray:
        """The baseline JPEGs ``data[offsets[i]:offsets[i + 1]]`` (``data``: a 1-D uint8 array or bytes in host memory; all frames of one
        size, 4:2:0) -> packed BGR frames in ``dst``, decoded on the GPU (``pa_jpeg_decode``; the same bytes as ``mjpeg.decode_host``).
        Returns the status words (n,) int32: 0, or the ``mjpeg.ST_*`` bits of a frame whose entropy-coded data is damaged — such a
        frame is reported, its undecodable intervals are grey, and the call succeeds.  The frame size is read from the first JPEG
        unless ``h`` and ``w`` say what it has to be (a clip that knows its size).
        Synchronous, on the engine's compute stream.  What the library refuses is an ``EngineError``, nothing is launched."""
        data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data
        if not (isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1 and data.flags.c_contiguous):
            raise TypeError("jpeg_decode: data must be bytes or a contiguous 1-D uint8 array")
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = offsets.size - 1
        if n < 1 or offsets[0] < 0 or np.any(np.diff(offsets) < 0) or offsets[-1] > data.size:
            raise EngineError(f"jpeg_decode: offsets must be n + 1 >= 2 ascending positions inside the {data.size} bytes of data")
        if h is None or w is None:
            try:
                info = jpeg_parse(data[int(offsets[0]):int(offsets[1])].tobytes())
            except ValueError as e:
                raise EngineError(f"jpeg_decode: frame 0: {e}") from None
            h, w = info["h"], info["w"]
        h, w = int(h), int(w)
        if dst.nbytes < n * h * w * 3:
            raise EngineError(f"jpeg_decode: dst holds {dst.nbytes} bytes, {n} BGR frames of {w} x {h} need {n * h * w * 3}")
        status = np.zeros(n, np.int32)
        self._check(self.lib.pa_jpeg_decode(self.handle, data.ctypes.data, offsets.ctypes.data, n, h, w, dst.ptr, status.ctypes.data))
        return status

    def jpeg_decode_last_path(self) -> int:
        """JPEG_DEC_PATH_VECTOR / JPEG_DEC_PATH_BYTE: how the last successful ``jpeg_decode`` stored its pixels (0: none yet)."""
        return int(self.lib.pa_jpeg_decode_last_path(self.handle))

    def jpeg_decode_last_times(self) -> dict:
        """Tools: milliseconds the stages of the last ``jpeg_decode`` took while ``set_profiling(True)`` was on — ``parse`` (host clock),
        ``upload``, ``entropy``, ``idct``, ``colour`` (HIP events)."""
        ms = (C.c_double * 5)()
        self._check(self.lib.pa_jpeg_decode_last_times(self.handle, ms))
        return dict(zip(("parse", "upload", "entropy", "idct", "colour"), (float(v) for v in ms)))

    def jpeg_decode_set_split(self, min_bytes: int = 0, sub_bytes: int = 0) -> None:
        """Which restart intervals of later ``jpeg_decode`` calls are split among the lanes of a workgroup
        (``pa_jpeg_decode_set_split``): those of at least ``min_bytes`` bytes (0: the default, -1: none, today's one wave per interval
        for all), in subsequences of ``sub_bytes`` bytes (0: the default, else a multiple of 4 in 4 .. 32768).  The pixels do not
        depend on either."""
        self._check(self.lib.pa_jpeg_decode_set_split(self.handle, int(min_bytes), int(sub_bytes)))

    def jpeg_decode_last_split(self) -> dict:
        """Of the last ``jpeg_decode``: ``split`` intervals on the split path, their ``subsequences``, the most ``rounds`` any of
        them took, ``serial`` intervals on the one-wave kernel."""
        out = (C.c_int64 * 4)()
        self._check(self.lib.pa_jpeg_decode_last_split(self.handle, out))
        return dict(zip(("split", "subsequences", "rounds", "serial"), (int(v) for v in out)))

    def timer_start(self) -> None:
        """Tools: mark the compute stream with a HIP event; ``timer_stop`` -> milliseconds of device time queued since."""
        self._check(self.lib.pa_engine_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = C.c_float(0.0)
        self._check(self.lib.pa_engine_timer_stop(self.handle, C.byref(ms)))
        return float(ms.value)

    def set_tuning(self, **kv):
        """Tests / tools only: impl (2 bx3, 0 tap; 1 — the retired LDS kernel — is refused), variant (tile id, -1 auto), tune, tap_pd, graph, alias, fold_up, timeline, fuse_stem, fuse_stem_cv1, fuse_sppf, fuse_head,
        lanes (2: alternate in-flight YOLO tickets run on two streams with their own activation memory, 1: one lane; same results)."""
        for k, v in kv.items():
            self._check(self.lib.pa_engine_set_tuning(self.handle, k.encode(), int(v)))
            if k == "timeline":
                self.timeline = bool(v)              # (pa_yolo_submit refuses then: yolo.YOLO.submit_frames falls back to infer_frames)

    # ---- multi-GPU: RCCL communicator owned by the library (include/padel_hip.h "multi-GPU")
    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        buf = C.create_string_buffer(bytes(unique_id), len(unique_id))
        self._check(self.lib.pa_engine_comm_init(self.handle, buf, len(unique_id), nranks, rank))
        self.nranks, self.rank = nranks, rank
        if nranks > 1:                     # the sharded runner's gathers travel over this communicator from now on (dist.gather_bytes)
            from . import dist as _dist
            _dist.use_engine_comm(self)

    def bcast_weights(self, model: "Model", root: int = 0):
        self._check(self.lib.pa_engine_bcast_weights(self.handle, model.handle, root))

    def bcast_weights_from(self, src: Optional["Model"], dst: "Model", root: int = 0):
        """Root sends ``src``'s blob, every rank (root included) receives into ``dst`` (created with empty=True)."""
        self._check(self.lib.pa_engine_bcast_weights_from(self.handle, src.handle if src is not None else None, dst.handle, root))

    def bcast(self, buf: DeviceBuffer, nbytes: int, root: int = 0):
        self._check(self.lib.pa_engine_bcast(self.handle, buf.ptr, nbytes, root))

    def gather_bytes(self, buf: np.ndarray, root: int = 0):
        """Variable-length uint8 buffers of every rank -> on `root` the list of them in rank order (None elsewhere), over the
        library's RCCL communicator (``pa_engine_gather_sizes`` + ``pa_engine_gather``: lengths by all-gather, payload by send /
        recv, no padding; torch.distributed is not in this path)."""
        buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        n = max(getattr(self, "nranks", 1), 1)
        me = getattr(self, "rank", 0)
        sizes = (C.c_uint64 * n)()
        self._check(self.lib.pa_engine_gather_sizes(self.handle, int(buf.size), sizes))
        total = int(sum(sizes))
        recv = np.empty(max(total, 1), np.uint8) if me == root else None
        self._check(self.lib.pa_engine_gather(self.handle, buf.ctypes.data if buf.size else None, int(buf.size),
                                              recv.ctypes.data if recv is not None else None, total if recv is not None else 0, sizes, root))
        if me != root:
            return None
        out, off = [], 0
        for k in range(n):
            out.append(recv[off:off + int(sizes[k])])
            off += int(sizes[k])
        return out

    def allreduce_max(self, value: float) -> float:
        v = C.c_double(value)
        self._check(self.lib.pa_engine_allreduce_max(self.handle, C.byref(v)))
        return v.value

    def close(self):
        if self.handle:
            from . import dist as _dist
            if _dist._comm_engine is self:
                _dist.use_engine_comm(None)
            self.lib.pa_engine_destroy(self.handle)
            self.handle = None


_default_engines: dict = {}


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id (rank 0 creates it; ship it to the other ranks out of band)."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    if lib.pa_comm_unique_id(buf, 128) != 0:
        raise EngineError(lib.pa_last_error(None).decode())
    return buf.raw


def default_engine(device_id: Optional[int] = None) -> Engine:
    if device_id is None:
        device_id = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("PADEL_DEVICE") is None \
            else int(os.environ["PADEL_DEVICE"])
        load_library()
        n = _lib.pa_device_count()
        if n > 0:
            device_id %= n
    if device_id not in _default_engines:
        _default_engines[device_id] = Engine(device_id)
    return _default_engines[device_id]


_PAGE = 4096


def _round_up(x: int, a: int) -> int:
    return (int(x) + a - 1) // a * a


def _frames_arg(frames, n: Optional[int], h: int, w: int):
    """frames: (n, h, w, 3) uint8 ndarray (``n`` None: as many as it holds), or a DeviceBuffer holding ``n`` such frames
    -> (what the pointer points into, pointer, n, on_device); the caller holds on to the first over the native call."""
    if isinstance(frames, DeviceBuffer):
        assert n is not None and frames.nbytes >= n * h * w * 3
        return frames, frames.ptr, n, True
    frames = np.ascontiguousarray(frames, np.uint8)
    n = len(frames) if n is None else n
    assert frames.shape == (n, h, w, 3), frames.shape
    return frames, frames.ctypes.data, n, False


def _yolo_params(classes: Optional[Sequence[int]], **fields):
    """-> (pa_yolo_params, the ctypes array its ``classes`` points to | None); the caller holds on to both over the native call."""
    cls_arr = (C.c_int32 * len(classes))(*[int(c) for c in classes]) if classes is not None and len(classes) else None
    return pa_yolo_params(n_classes=0 if cls_arr is None else len(cls_arr), classes=cls_arr, **fields), cls_arr


class _PinnedBlock:
    """Whole pages of host memory, page-locked for one engine (hipHostRegister locks pages: small arrays that share a page
    cannot be registered / unregistered independently).  Unregistered by ``release()`` or when the object dies — always
    before the memory itself can be freed, which the views handed out keep alive."""

    def __init__(self, engine, nbytes: int):
        import mmap
        size = _round_up(max(int(nbytes), 1), _PAGE)
        # an anonymous mapping of its own, not malloc memory: glibc serves numpy arrays of this size from the brk heap once its
        # dynamic mmap threshold has grown (after the first multi-megabyte array was freed), and pages of the heap that were
        # registered, unregistered and then handed to an unrelated array made a later pageable hipMemcpy from that array fault
        # on the GPU (round 5, tests/test_gpu_pipeline.py::test_close_with_a_ticket_in_flight_then_reuse_the_pages).  A private
        # mapping is page-aligned, zero-filled, and its addresses go back to the kernel — not to malloc — when the views die
        # MAP_PRIVATE | MAP_ANONYMOUS explicitly: Python's default for fileno -1 is MAP_SHARED — shmem-backed pages that a forked child
        # (multiprocessing, the gloo test workers) would share with the parent's result arrays
        self._mm = mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, prot=mmap.PROT_READ | mmap.PROT_WRITE)
        self.block = np.frombuffer(self._mm, np.uint8)
        self.engine = engine
        engine.pin(self.block)
        self._pinned = True

    def release(self) -> None:
        if self._pinned:
            self._pinned = False
            try:
                self.engine.unpin(self.block)
            except Exception as exc:
                # the pages stay registered and their memory is about to be freed: say so (a later copy from memory that
                # lands on these addresses fails inside the runtime) — except at interpreter shutdown, when the engine is gone
                if _sys is not None and getattr(_sys, "meta_path", None) is not None and getattr(self.engine, "handle", None):
                    print(f"padel_analytics_amd: hipHostUnregister of a result block failed ({exc}); pages left registered", file=_sys.stderr)

    def __del__(self):
        self.release()


class Model:
    """A graph + weights resident in HBM on one engine."""

    def __init__(self, engine: Engine, graph: G.Graph, blob: Optional[np.ndarray] = None, *, empty: bool = False):
        """empty=True: allocate the weight blob in HBM without uploading anything — it arrives through
        ``engine.bcast_weights(model)`` from the rank that loaded the checkpoint."""
        self.engine, self.graph = engine, graph
        if not empty:
            blob = graph.blob() if blob is None else np.ascontiguousarray(blob, np.float32)
        bufs = (pa_buf_desc * len(graph.bufs))(*[pa_buf_desc(l, c) for l, c in graph.bufs])
        ops = (pa_op_desc * len(graph.ops))()
        for i, o in enumerate(graph.ops):
            for k, v in o.items():
                setattr(ops[i], k, int(v))
        d = pa_model_desc(task=graph.task, nc=graph.nc, nk=graph.nk, kpt_dim=graph.kpt_dim, n_bufs=len(graph.bufs),
                          bufs=bufs, n_ops=len(graph.ops), ops=ops, in_channels=graph.in_channels,
                          dtype=graph.dtype)
        for i in range(3):
            d.head_buf[i] = graph.head_buf[i] if i < len(graph.head_buf) else -1
        h = C.c_void_p()
        engine._check(engine.lib.pa_model_create(engine.handle, C.byref(d), None if empty else blob.ctypes.data,
                                                 graph.n_floats if empty else blob.size, C.byref(h)))
        self.handle = h
        self.max_batch = 64
        self._out_ring: dict = {}        # (n, max_det) -> [three page-locked (boxes, kpts, counts) sets, next slot]

    #: tickets a model may have in flight (PA_MAX_INFLIGHT of include/padel_hip.h)
    MAX_INFLIGHT = 4
    #: recycled result sets per (n, max_det): every ticket in flight owns one, plus the set whose results the host stage is
    #: still reading and the one collected just before it — a set is handed out again OUT_RING calls later
    OUT_RING = MAX_INFLIGHT + 2

    def _ring_outputs(self, n: int, max_det: int):
        key = (int(n), int(max_det))
        ring = self._out_ring.get(key)
        if ring is None:
            nk = self.graph.nk
            sizes = [n * max_det * 6 * 4, n * max_det * nk * 4, n * 4]
            offs = [0, _round_up(sizes[0], 64), 0]
            offs[2] = offs[1] + _round_up(sizes[1], 64)
            sets = []
            for _ in range(self.OUT_RING):
                pb = _PinnedBlock(self.engine, offs[2] + sizes[2])
                block = pb.block
                boxes = block[offs[0]:offs[0] + sizes[0]].view(np.float32).reshape(n, max_det, 6)
                kpts = block[offs[1]:offs[1] + sizes[1]].view(np.float32).reshape(n, max_det, nk) if nk else None
                counts = block[offs[2]:offs[2] + sizes[2]].view(np.int32).reshape(n)
                sets.append((boxes, kpts, counts, pb))
            ring = self._out_ring[key] = [sets, 0]
        sets, i = ring
        ring[1] = (i + 1) % self.OUT_RING
        return sets[i][:3]

    def _fresh_outputs(self, n: int, max_det: int):
        nk = self.graph.nk
        return (np.zeros((n, max_det, 6), np.float32), np.zeros((n, max_det, nk), np.float32) if nk else None,
                np.zeros((n,), np.int32))

    def _free_rings(self):
        for sets, _ in self._out_ring.values():
            for arrs in sets:
                arrs[3].release()
        self._out_ring = {}

    def __del__(self):
        # a model dropped without close(): its page-locked result blocks must be unregistered BEFORE their memory goes back
        # to the allocator (a stale registration makes later copies to / from whatever reuses those pages fail) — and AFTER
        # the stream has drained: a ticket still queued copies its results into exactly those pages
        # (only that: destroying the HBM side here could outlive its engine)
        try:
            if self._out_ring and getattr(self, "handle", None) and self.engine.handle:
                self.engine.synchronize()
        except Exception:
            pass
        try:
            self._free_rings()
        except Exception:
            pass

    def set_max_batch(self, n: int):
        self.engine._check(self.engine.lib.pa_model_set_max_batch(self.handle, int(n)))
        self.max_batch = int(n)

    def yolo_infer(self, frames, n: int, h: int, w: int, *, imgsz: int, conf: float, iou: float,
                   classes: Optional[Sequence[int]] = None, max_det: int = 300, pre_mode: int = PRE_LETTERBOX,
                   channel_reverse: bool = False, letterbox_auto: bool = True, reuse_outputs: bool = False):
        """frames: (n,h,w,3) uint8 ndarray, or a DeviceBuffer holding the same bytes.
        Returns (boxes (n,max_det,6), kpts (n,max_det,nk) | None, counts (n,)).

        ``reuse_outputs=True`` (the trackers' batch loops): the arrays are one of ``OUT_RING`` page-locked sets this model
        keeps per (n, max_det) — the device copies its results straight into them (no staging copy, no 3.5 MB of fresh
        zeros per pose batch) — and are overwritten by the ``OUT_RING``-th next such call; copy what must live longer."""
        frames, ptr, n, on_dev = _frames_arg(frames, n, h, w)
        p, cls_arr = _yolo_params(classes, imgsz=imgsz, pre_mode=pre_mode, channel_reverse=int(channel_reverse),
                                  letterbox_auto=int(letterbox_auto), conf=conf, iou=iou, max_det=max_det,
                                  frames_on_device=int(on_dev))
        boxes, kpts, counts = self._ring_outputs(n, max_det) if reuse_outputs else self._fresh_outputs(n, max_det)
        self.engine._check(self.engine.lib.pa_yolo_infer(
            self.handle, ptr, n, h, w, C.byref(p), boxes.ctypes.data,
            kpts.ctypes.data if kpts is not None else None, counts.ctypes.data))
        return boxes, kpts, counts

    def yolo_submit(self, frames: "DeviceBuffer", n: int, h: int, w: int, *, imgsz: int, conf: float, iou: float,
                    classes: Optional[Sequence[int]] = None, max_det: int = 300, pre_mode: int = PRE_LETTERBOX,
                    channel_reverse: bool = False, letterbox_auto: bool = True):
        """``yolo_infer`` in two halves (pa_yolo_submit / pa_yolo_wait): enqueue the whole call behind what the engine's stream
        still holds and return a ticket at once; ``yolo_wait(ticket)`` -> (boxes, kpts, counts, overflow).  Frames must be in
        HBM; the results land in one of the model's recycled page-locked sets (``reuse_outputs`` rules).  Submit batch k + 1
        before waiting for batch k and the GPU never waits for the host between batches."""
        assert isinstance(frames, DeviceBuffer) and frames.nbytes >= n * h * w * 3
        p, cls_arr = _yolo_params(classes, imgsz=imgsz, pre_mode=pre_mode, channel_reverse=int(channel_reverse),
                                  letterbox_auto=int(letterbox_auto), conf=conf, iou=iou, max_det=max_det, frames_on_device=1)
        boxes, kpts, counts = self._ring_outputs(n, max_det)
        t = C.c_int(-1)
        self.engine._check(self.engine.lib.pa_yolo_submit(
            self.handle, frames.ptr, n, h, w, C.byref(p), boxes.ctypes.data,
            kpts.ctypes.data if kpts is not None else None, counts.ctypes.data, C.byref(t)))
        return (t.value, boxes, kpts, counts)

    def yolo_wait(self, ticket):
        t, boxes, kpts, counts = ticket
        ovf = C.c_int(0)
        self.engine._check(self.engine.lib.pa_yolo_wait(self.handle, t, C.byref(ovf)))
        return boxes, kpts, counts, bool(ovf.value)

    def head_shapes(self, h: int, w: int, imgsz: int, pre_mode: int = PRE_LETTERBOX, letterbox_auto: bool = True) -> list:
        """[(H_l, W_l, c)] of the three head maps for source size h x w (host arithmetic of the planner)."""
        if pre_mode == PRE_PIL_STRETCH or not letterbox_auto:
            nh = nw = imgsz
        else:
            r = min(imgsz / h, imgsz / w)
            rw, rh = int(round(w * r)), int(round(h * r))
            nw, nh = rw + (imgsz - rw) % 32, rh + (imgsz - rh) % 32
        c = self.graph.bufs[self.graph.head_buf[0]][1]
        return [(nh >> (3 + l), nw >> (3 + l), c) for l in range(3)]

    def yolo_postprocess(self, heads, h: int, w: int, *, imgsz: int, conf: float, iou: float,
                         classes: Optional[Sequence[int]] = None, max_det: int = 300, pre_mode: int = PRE_LETTERBOX):
        """Decode + NMS + rescale of caller-supplied head maps (``heads[l]``: (n, H_l, W_l, c) fp32, ``head_shapes``):
        the Detect / Pose inference branch alone — tests feed hand-derived cases through it."""
        heads = [np.ascontiguousarray(x, np.float32) for x in heads]
        n = heads[0].shape[0]
        assert [x.shape[1:] for x in heads] == [tuple(s) for s in self.head_shapes(h, w, imgsz, pre_mode)], [x.shape for x in heads]
        p, cls_arr = _yolo_params(classes, imgsz=imgsz, pre_mode=pre_mode, channel_reverse=0, letterbox_auto=1, conf=conf, iou=iou,
                                  max_det=max_det, frames_on_device=0)
        ptrs = (C.c_void_p * 3)(*[x.ctypes.data for x in heads])
        boxes, kpts, counts = self._fresh_outputs(n, max_det)
        self.engine._check(self.engine.lib.pa_yolo_postprocess(self.handle, ptrs, n, h, w, C.byref(p), boxes.ctypes.data,
                                                               kpts.ctypes.data if kpts is not None else None, counts.ctypes.data))
        return boxes, kpts, counts

    def fill_arena(self, byte_value: int = 0xFF) -> None:
        """Tests: overwrite the planned activation arena (0xFF = NaN patterns) and the u8 network input: a following inference
        must not notice."""
        self.engine._check(self.engine.lib.pa_model_fill_arena(self.handle, int(byte_value)))

    def take_overflow(self) -> bool:
        """h2 and fp16 models: True if an activation written since the last call did not fit the fp16 range (clears the flag);
        fp16 models test the fp32 value they clamp, ``not (|x| <= 65504)``, NaN included.  Always False for fp32 models."""
        v = C.c_int(0)
        self.engine._check(self.engine.lib.pa_model_take_overflow(self.handle, C.byref(v)))
        return bool(v.value)

    def read_head(self, level: int, n: int) -> np.ndarray:
        hh, ww, cc = C.c_int(), C.c_int(), C.c_int()
        self.engine._check(self.engine.lib.pa_yolo_head_shape(self.handle, level, C.byref(hh), C.byref(ww), C.byref(cc)))
        out = np.empty((n, hh.value, ww.value, cc.value), np.float32)
        self.engine._check(self.engine.lib.pa_yolo_read_head(self.handle, level, n, out.ctypes.data))
        return out

    def last_post_path(self) -> int:
        """POST_PATH_DECODE / POST_PATH_FUSED: what the last ``yolo_infer`` / ``yolo_submit`` / ``postprocess`` of this model ran
        after the network — ``decode_kernel`` over head maps, or the fused head tail (tuning ``fuse_head``)."""
        return int(self.engine.lib.pa_yolo_last_post_path(self.handle))

    def last_stem_path(self) -> int:
        """1: the last replay of this model's op list ran the 1x1 conv behind layer 1 (model.2.cv1) inside the fused stem kernel
        (tuning ``fuse_stem_cv1``), 0: it did not (that conv was a launch of its own, or the graph has none)."""
        return int(self.engine.lib.pa_model_last_stem_path(self.handle))

    def lanes_allocated(self) -> int:
        """How many lanes (sets of per-batch device memory) the current plan has: 0 before a plan, 1, or 2 once a ``yolo_submit``
        found the previous ticket still in flight (tuning ``lanes``)."""
        return int(self.engine.lib.pa_model_lanes_allocated(self.handle))

    def resample_passes(self) -> int:
        """Tests: passes of the Pillow resample of the current plan (0 none, 1 one axis, 2 both axes through a temporary)."""
        return int(self.engine.lib.pa_yolo_resample_passes(self.handle))

    def last_lane(self) -> int:
        """The lane (0 | 1) the model's last ``yolo_infer`` / ``yolo_submit`` / ``postprocess`` ran on."""
        return int(self.engine.lib.pa_model_last_lane(self.handle))

    def read_netin(self, n: int) -> np.ndarray:
        """u8 NHWC4 network input of the first n frames of the last yolo_infer call."""
        hh, ww = C.c_int(), C.c_int()
        self.engine._check(self.engine.lib.pa_yolo_netin_shape(self.handle, C.byref(hh), C.byref(ww)))
        out = np.empty((n, hh.value, ww.value, 4), np.uint8)
        self.engine._check(self.engine.lib.pa_yolo_read_netin(self.handle, n, out.ctypes.data))
        return out

    def plan_bytes(self) -> tuple:
        """(arena bytes allocated, sum of the logical buffers) of the current activation plan."""
        a, l = C.c_size_t(), C.c_size_t()
        self.engine._check(self.engine.lib.pa_model_plan_bytes(self.handle, C.byref(a), C.byref(l)))
        return a.value, l.value

    def tracknet_infer(self, x: np.ndarray) -> np.ndarray:
        """x: (n, H, W, C_in) NHWC (fp32; fp16 for a graph with dtype f16) -> (n, H, W, C_out) fp32."""
        x = np.ascontiguousarray(x, np.float16 if self.graph.dtype == G.DTYPE_F16 else np.float32)
        n, h, w, c = x.shape
        assert c == self.graph.bufs[0][1], (c, self.graph.bufs[0])
        lvl, cout = self.graph.bufs[self.graph.head_buf[0]]
        out = np.empty((n, h >> lvl, w >> lvl, cout), np.float32)
        self.engine._check(self.engine.lib.pa_tracknet_infer(self.handle, x.ctypes.data, n, h, w, 0, out.ctypes.data, 0))
        return out

    # ---- court keypoints (PA_TASK_RESNET graphs: graph.build_resnet50)
    def resnet_infer(self, frames, n: int, h: int, w: int, *, want_logits: bool = False):
        """frames: (n, h, w, 3) uint8 BGR ndarray, or a DeviceBuffer holding the same bytes -> (xy (n, c) fp32 sigmoid outputs,
        logits (n, c) | None); c = outputs of the graph's pooled linear head (24).  A graph without one (unit tests) gives
        (None, None): read its head buffer with ``resnet_read_head``."""
        frames, ptr, n, on_dev = _frames_arg(frames, n, h, w)
        c = next((o["cout"] for o in self.graph.ops if o["kind"] == G.OP_GAP_FC), 0)
        xy = np.zeros((n, c), np.float32) if c else None
        logits = np.zeros((n, c), np.float32) if (c and want_logits) else None
        self.engine._check(self.engine.lib.pa_resnet_infer(self.handle, ptr, n, h, w, int(on_dev),
                                                           xy.ctypes.data if c else None,
                                                           logits.ctypes.data if logits is not None else None))
        return xy, logits

    def resnet_read_netin(self, n: int) -> np.ndarray:
        """u8 NHWC4 (R, G, B, 0) 224 x 224 network input of the first n frames of the last resnet_infer call."""
        out = np.empty((n, G.RESNET_INPUT, G.RESNET_INPUT, 4), np.uint8)
        self.engine._check(self.engine.lib.pa_resnet_read_netin(self.handle, n, out.ctypes.data))
        return out

    def read_fc(self, n: int):
        """(xy, logits), each (n, c): what the pooled linear head of the graph wrote during the last replay."""
        c = next(o["cout"] for o in self.graph.ops if o["kind"] == G.OP_GAP_FC)
        xy, logits = np.empty((n, c), np.float32), np.empty((n, c), np.float32)
        self.engine._check(self.engine.lib.pa_resnet_read_fc(self.handle, n, xy.ctypes.data, logits.ctypes.data))
        return xy, logits

    def resnet_read_head(self, n: int) -> np.ndarray:
        """Tests: buffer head_buf[0] of a PA_TASK_RESNET graph after the last resnet_infer call, (n, H, W, channels) fp32."""
        lvl, ch = self.graph.bufs[self.graph.head_buf[0]]
        out = np.empty((n, G.RESNET_INPUT >> lvl, G.RESNET_INPUT >> lvl, ch), np.float32)
        self.engine._check(self.engine.lib.pa_resnet_read_head(self.handle, n, out.ctypes.data))
        return out

    def last_profile(self, cap: int = 4096):
        kinds = np.zeros(cap, np.int32)
        ms = np.zeros(cap, np.float32)
        fl = np.zeros(cap, np.float64)
        ks = np.zeros(cap, np.int32)
        n = self.engine.lib.pa_model_last_profile(self.handle, cap, kinds.ctypes.data, ms.ctypes.data, fl.ctypes.data,
                                                  ks.ctypes.data)
        return [dict(kind=int(kinds[i]), ms=float(ms[i]), flops=float(fl[i]), ksize=int(ks[i])) for i in range(n)]

    def profile_rows(self):
        """Per-op records of the last profiled inference: dicts with shape, tile and milliseconds."""
        buf = C.create_string_buffer(1 << 20)
        self.engine.lib.pa_model_profile_text(self.handle, buf, len(buf))
        return parse_profile_text(buf.value.decode())

    def close(self):
        """Drain first, unpin second: pa_model_destroy synchronizes the engine's stream, so tickets still queued (the
        overflow fallback closes a model with batch k + 1 in flight) have finished their copies into the page-locked result
        sets before those pages are unregistered (tests/test_gpu_pipeline.py closes a model with a ticket out)."""
        if self.handle:
            self.engine.lib.pa_model_destroy(self.handle)
            self.handle = None
            self._free_rings()


# ``kind`` of the profile rows that are not ops of the graph (csrc/engine_internal.h: PROF_PRE, PROF_DECODE, PROF_NMS)
PROF_PRE, PROF_DECODE, PROF_NMS = 100, 101, 102


def parse_profile_text(text: str):
    """``pa_model_profile_text`` lines -> dicts.  Columns 1-11: kind, ksize, M, cout, cin, stride, mf, nf (the REQUESTED tile's
    pixels and channels), ms, flops, res; 12 and 13 (convs): ``tile`` — the tile id the dispatcher launched after every
    fall-through — and ``family`` — the tag of the kernel template that ran (csrc/kernels.h ConvLaunched).  Lines of older
    libraries have 10 or 11 columns: res 0, tile -1, family ""."""
    rows = []
    for line in text.splitlines():
        f = line.split(",")
        k, ks, M, co, ci, st, mf, nf, ms, fl, res = (f + ["0"])[:11]
        rows.append(dict(kind=int(k), ksize=int(ks), M=int(M), cout=int(co), cin=int(ci), stride=int(st),
                         mf=int(mf), nf=int(nf), ms=float(ms), flops=float(fl), res=int(res),
                         tile=int(f[11]) if len(f) > 11 and f[11] else -1, family=f[12] if len(f) > 12 else ""))
    return rows


class NativeByteTrack:
    """``pa_bytetrack_*``: the host-native (C++) twin of ``padel_analytics_amd.bytetrack.ByteTrack`` — same
    algorithm, orderings and id semantics (tests/test_bytetrack_golden.py pins both to the same fixtures); consumes
    a whole batch of frames per call.  Host code inside libpadel_hip.so: works without a GPU."""

    def __init__(self, track_activation_threshold: float = 0.25, lost_track_buffer: int = 30,
                 minimum_matching_threshold: float = 0.8, frame_rate: int = 30):
        self.lib = load_library()
        h = C.c_void_p()
        if self.lib.pa_bytetrack_create(track_activation_threshold, lost_track_buffer, minimum_matching_threshold,
                                        int(frame_rate), C.byref(h)) != 0:
            raise EngineError("pa_bytetrack_create failed")
        self.handle = h

    def reset(self) -> None:
        self.lib.pa_bytetrack_reset(self.handle)

    def update_batch(self, boxes: np.ndarray, counts: np.ndarray, keep: Optional[np.ndarray] = None) -> np.ndarray:
        """boxes (n, stride, 6) fp32, counts (n,) int32, keep (n, stride) bool/uint8 | None -> ids (n, stride) int32."""
        boxes = np.ascontiguousarray(boxes, np.float32)
        counts = np.ascontiguousarray(counts, np.int32)
        n, stride, six = boxes.shape
        assert six == 6 and counts.shape == (n,)
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8)
            assert keep.shape == (n, stride)
            kp = keep.ctypes.data
        ids = np.empty((n, stride), np.int32)
        if self.lib.pa_bytetrack_update_batch(self.handle, boxes.ctypes.data, counts.ctypes.data, kp, n, stride,
                                              ids.ctypes.data) != 0:
            raise EngineError("pa_bytetrack_update_batch failed")
        return ids

    def update_with_detections(self, detections):
        """Single-frame form with the signature of ``sv.ByteTrack.update_with_detections`` (players_tracker.py:367)."""
        n = len(detections)
        boxes = np.zeros((1, max(n, 1), 6), np.float32)
        boxes[0, :n, :4] = detections.xyxy
        boxes[0, :n, 4] = 1.0 if detections.confidence is None else detections.confidence
        ids = self.update_batch(boxes, np.array([n], np.int32))[0, :n]
        out = detections[np.nonzero(ids >= 0)[0]]
        out.tracker_id = ids[ids >= 0].astype(int)
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.pa_bytetrack_destroy(self.handle)
            self.handle = None


class BallSession:
    """Streaming TrackNet session on one engine (``pa_ball_*``): resize + windows + network + temporal
    ensemble + threshold on the GPU; yields one 288x512 uint8 mask (and optionally the fp32 heat map) per frame."""

    H, W = 288, 512

    def __init__(self, model: Model, src_h: int, src_w: int):
        self.model, self.src_h, self.src_w = model, src_h, src_w
        h = C.c_void_p()
        model.engine._check(model.engine.lib.pa_ball_create(model.handle, src_h, src_w, C.byref(h)))
        self.handle = h
        self.max_feed = model.max_batch

    def set_background(self, median_rgb: np.ndarray):
        m = np.ascontiguousarray(median_rgb, np.uint8)
        assert m.shape == (self.src_h, self.src_w, 3), m.shape
        self.model.engine._check(self.model.engine.lib.pa_ball_set_background(self.handle, m.ctypes.data))

    def background_from_frames(self, frames_bgr, want_median: bool = False, n: Optional[int] = None):
        """Median background of (n, h, w, 3) uint8 BGR frames on the device (np.median + uint8 truncation).
        ``frames_bgr``: ndarray, or a DeviceBuffer holding ``n`` frames."""
        on_dev = isinstance(frames_bgr, DeviceBuffer)
        frames_bgr, ptr, n, _ = _frames_arg(frames_bgr, n if on_dev else None, self.src_h, self.src_w)
        med = np.empty((self.src_h, self.src_w, 3), np.uint8) if want_median else None
        self.model.engine._check(self.model.engine.lib.pa_ball_background_from_frames(
            self.handle, ptr, n, int(on_dev), med.ctypes.data if want_median else None))
        return med

    def feed(self, frames_bgr, flush: bool = False, want_heat: bool = False,
             want_rects: bool = False, want_masks: bool = True, n: Optional[int] = None):
        """frames_bgr: (n, h, w, 3) uint8 with n <= max_feed, a DeviceBuffer holding ``n`` such frames, or None with
        flush=True.  Returns (masks (k,288,512) uint8 | None, heat (k,288,512) fp32 | None[, rects (k,4) int32]):
        outputs for the next k frames in order; rects = predict_location of each mask computed on the device."""
        on_dev = isinstance(frames_bgr, DeviceBuffer)
        ptr = None
        if not on_dev:
            n = 0 if frames_bgr is None else len(frames_bgr)
        if on_dev or n:
            frames_bgr, ptr, n, _ = _frames_arg(frames_bgr, n, self.src_h, self.src_w)
            assert 0 < n <= self.max_feed
        masks = np.empty((n + 7, self.H, self.W), np.uint8) if (want_masks or not want_rects) else None
        heat = np.empty((n + 7, self.H, self.W), np.float32) if want_heat else None
        rects = np.empty((n + 7, 4), np.int32) if want_rects else None
        cnt = C.c_int(0)
        self.model.engine._check(self.model.engine.lib.pa_ball_feed(
            self.handle, ptr, n, int(on_dev), int(flush), masks.ctypes.data if masks is not None else None,
            heat.ctypes.data if want_heat else None, rects.ctypes.data if want_rects else None, C.byref(cnt)))
        k = cnt.value
        out = (None if masks is None else masks[:k], heat[:k] if want_heat else None)
        return out + (rects[:k],) if want_rects else out

    def locate(self, masks: np.ndarray) -> np.ndarray:
        """predict_location of (n,288,512) uint8 masks on the device -> (n,4) int32 {x, y, w, h}."""
        masks = np.ascontiguousarray(masks, np.uint8)
        n = len(masks)
        assert masks.shape == (n, self.H, self.W)
        rects = np.empty((n, 4), np.int32)
        self.model.engine._check(self.model.engine.lib.pa_ball_locate(self.handle, masks.ctypes.data, n, rects.ctypes.data))
        return rects

    def read_resized(self, frame: Optional[int] = None) -> np.ndarray:
        """Tests: the (288, 512, 3) uint8 RGB image the session's Pillow resize made of the background (``frame`` None) or of
        frame ``frame`` (counted from 0 since the background was set; the ring keeps the last max_feed + 7 frames fed)."""
        out = np.empty((self.H, self.W, 3), np.uint8)
        self.model.engine._check(self.model.engine.lib.pa_ball_read_resized(self.handle, -1 if frame is None else int(frame),
                                                                            out.ctypes.data))
        return out

    def close(self):
        if self.handle:
            self.model.engine.lib.pa_ball_destroy(self.handle)
            self.handle = None
