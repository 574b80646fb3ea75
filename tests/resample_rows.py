"""Geometries of the two-pass Pillow resample (csrc/kernels_misc.hip: resample_pass_kernel, resample_vpass4_kernel; planned and
enqueued by csrc/engine_pre.cpp) that the sources of the other tests never produce: a horizontal pass that is also the last one, a
single vertical pass, a source of the target size, odd widths and heights, frames whose byte count is odd, one axis up and the other
down, both channel orders, many taps.  tests/test_resample_geometry_host.py checks the table itself on the CPU (tables replayed in
numpy against Pillow, which kernel each row reaches, tap counts, that the clip is exercised); tests/test_gpu_resample_geometry.py
runs every row through the kernels.

A row: ``family`` (which engine path plans it), source ``hw``, ``target`` (h, w), ``filter``, ``out_c`` (bytes per output pixel),
``batch``, ``taps`` = (horizontal, vertical) table widths worked out by hand from Pillow's rule
``ksize = 2 * ceil(support * max(in / out, 1)) + 1`` (support 2 bicubic, 1 bilinear; 0: the pass does not run), ``reach`` = the
launches the row is meant to cause, in order (``launches`` restates the engine's choice), and ``src_offset``: the byte offset of
the frames inside their device allocation (0: wherever the engine stages host frames).
"""
import functools

import numpy as np

from padel_analytics_amd import engine as E

YOLO_S = 160
RESNET_S = 224
BALL_HW = (288, 512)

# names of the launches
COPY = "letterbox copy"                     # a source of the target size on the YOLO / ResNet path: the letterbox kernel in copy mode
H_LAST = "horizontal generic, last"        # writes out_c bytes per pixel, applies the channel order
H_TMP = "horizontal generic, to the temporary"
VPASS4 = "vertical vpass4"
V_GENERIC = "vertical generic"
V_IDENTITY = "vertical generic, one-tap identity"


def _row(family, hw, reach, taps, batch=3, src_offset=0):
    target, filt, out_c = {"yolo": ((YOLO_S, YOLO_S), E.PIL_BICUBIC, 4), "resnet": ((RESNET_S, RESNET_S), E.PIL_BILINEAR, 4),
                           "ball": (BALL_HW, E.PIL_BICUBIC, 3)}[family]
    name = f"{family} {hw[0]}x{hw[1]}" + (f" +{src_offset}" if src_offset else "")
    return dict(name=name, family=family, hw=hw, target=target, filter=filt, out_c=out_c, batch=batch, taps=taps, reach=reach,
                src_offset=src_offset)


YOLO_ROWS = [
    _row("yolo", (160, 160), (COPY,), (0, 0)),
    _row("yolo", (160, 253), (H_LAST,), (9, 0)),               # 253 / 160 = 1.58; 2 x 1.58 = 3.16 -> 4; 9 taps
    _row("yolo", (160, 101), (H_LAST,), (5, 0)),               # upscale: support 2 -> 5 taps
    _row("yolo", (117, 160), (VPASS4,), (0, 5)),
    _row("yolo", (333, 160), (VPASS4,), (0, 11)),              # 333 / 160 = 2.08; 4.16 -> 5; 11 taps
    _row("yolo", (117, 160), (V_GENERIC,), (0, 5), src_offset=1),
    _row("yolo", (97, 131), (H_TMP, VPASS4), (5, 5)),
    _row("yolo", (333, 517), (H_TMP, VPASS4), (15, 11)),       # 517 / 160 = 3.23; 6.46 -> 7; 15 taps.  516 483 bytes per frame
    _row("yolo", (90, 250), (H_TMP, VPASS4), (9, 5)),          # 250 / 160 = 1.56; 3.13 -> 4; 9 taps
    _row("yolo", (250, 90), (H_TMP, VPASS4), (5, 9)),
    _row("yolo", (1080, 1917), (H_TMP, VPASS4), (49, 29), batch=2),    # 11.98 x 2 = 23.96 -> 24; 6.75 x 2 = 13.5 -> 14
]
RESNET_ROWS = [
    _row("resnet", (224, 301), (H_LAST,), (5, 0)),             # 301 / 224 = 1.34 -> 2; 5 taps
    _row("resnet", (199, 224), (VPASS4,), (0, 3)),
    _row("resnet", (75, 93), (H_TMP, VPASS4), (3, 3)),
    _row("resnet", (451, 333), (H_TMP, VPASS4), (5, 7)),       # 333 / 224 = 1.49 -> 2; 451 / 224 = 2.01 -> 3
]
BALL_ROWS = [
    _row("ball", (288, 512), (V_IDENTITY,), (0, 1), batch=2),
    _row("ball", (288, 640), (H_LAST,), (7, 0), batch=2),      # 1.25 x 2 = 2.5 -> 3; 7 taps
    _row("ball", (360, 512), (V_GENERIC,), (0, 7), batch=2),
    _row("ball", (97, 131), (H_TMP, V_GENERIC), (5, 5), batch=2),
    _row("ball", (301, 517), (H_TMP, V_GENERIC), (7, 7), batch=2),     # 1.01 x 2 = 2.02 -> 3; 1.05 x 2 = 2.09 -> 3
]
ROWS = YOLO_ROWS + RESNET_ROWS + BALL_ROWS
BALL_FRAMES = 11            # fed 2 at a time to a ring of 2 + 7 slots: the fifth feed wraps (one frame to slot 8, one to slot 0)

#: the one bicubic row whose passes are not required to overshoot (49 and 29 taps average the checkerboard away)
NO_OVERSHOOT = "yolo 1080x1917"


# ---------------------------------------------------------------------------------------- which kernels a row reaches
def launches(row):
    """resample_enqueue + launch_resample_pass + the same-size special cases of engine_yolo.cpp / engine_resnet.cpp / pa_ball_create,
    restated: the launches a batch of the row's frames causes.  Pointers: host frames are staged in a hipMalloc'ed buffer, the
    temporary and the network input are hipMalloc'ed (256-byte aligned); ``src_offset`` moves the source pointer."""
    (sh, sw), (dh, dw), out_c = row["hw"], row["target"], row["out_c"]
    if (sh, sw) == (dh, dw):
        return (V_IDENTITY,) if row["family"] == "ball" else (COPY,)
    out = []
    in_align, in_w = row["src_offset"] % 4, sw
    if sw != dw:
        out.append(H_LAST if sh == dh else H_TMP)
        in_align, in_w = 0, dw
    if sh != dh:
        in_c, vertical, out_w, out_align = 3, True, in_w, 0
        vpass4 = (vertical and in_c == 3 and out_c == 4 and in_w % 4 == 0 and out_w == in_w and in_align == 0 and out_align % 16 == 0
                  and (sh * in_w * 3) % 4 == 0)
        out.append(VPASS4 if vpass4 else V_GENERIC)
    return tuple(out)


# ---------------------------------------------------------------------------------------- frames
def noise_frames(n, h, w, seed):
    """Uniform noise; rows 0 .. (h + 1) // 2 a 0 / 255 checkerboard of 3-row by 5-column cells (bicubic overshoot on both sides)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:(h + 1) // 2, 0:w]
    f[:, :(h + 1) // 2] = ((((yy // 3) + (xx // 5)) & 1) * 255).astype(np.uint8)[None, :, :, None]
    return f


@functools.lru_cache(maxsize=None)
def frames_of(name, variant=0):
    """The frames of a row as the engine gets them (read-only; every frame different in its noise half).  Ball rows: the BALL_FRAMES
    frames fed; ``variant`` 1: another set of the same geometry (the background of a ball row, the earlier contents of the network
    input of the same-size row)."""
    row = next(r for r in ROWS if r["name"] == name)
    n = BALL_FRAMES if row["family"] == "ball" and variant == 0 else row["batch"]
    # (seeded by the geometry, not the row: the two 117 x 160 rows get the same frames)
    f = noise_frames(n, *row["hw"], seed=[*row["hw"], ("yolo", "resnet", "ball").index(row["family"]), variant])
    f.setflags(write=False)
    return f


# ---------------------------------------------------------------------------------------- Pillow
def _pil_filter(filt):
    from PIL import Image
    return {E.PIL_BICUBIC: Image.BICUBIC, E.PIL_BILINEAR: Image.BILINEAR}[filt]


def pillow_resize(img, target, filt):
    """Image.resize of one (h, w, 3) uint8 image in one step."""
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((target[1], target[0]), _pil_filter(filt)))


def pillow_two_step(img, target, filt):
    """The width first, then the height: the order the engine's passes run in."""
    return pillow_resize(pillow_resize(img, (img.shape[0], target[1]), filt), target, filt)


@functools.lru_cache(maxsize=None)
def pillow_of(name, variant=0):
    """Pillow's resize of every frame of ``frames_of(name, variant)``, in the channel order of the frames."""
    row = next(r for r in ROWS if r["name"] == name)
    out = np.stack([pillow_resize(f, row["target"], row["filter"]) for f in frames_of(name, variant)])
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------- the tables, replayed
def replay_pass(imgs, out_size, axis, filt):
    """One resample pass over (n, h, w, 3) images along ``axis`` (1 vertical, 2 horizontal) in numpy over the tables the device
    kernels use (22-bit fixed point, accumulator from 1 << 21) -> (u8 result, least and greatest value before the clip, table width)."""
    bounds, coefs = E.pil_coeffs(imgs.shape[axis], out_size, filt)
    src = np.moveaxis(imgs, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    lo_v, hi_v = 0, 255
    for o in range(out_size):
        lo, n = bounds[o]
        acc = ((1 << 21) + np.tensordot(coefs[o, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))) >> 22
        lo_v, hi_v = min(lo_v, int(acc.min())), max(hi_v, int(acc.max()))
        out[o] = np.clip(acc, 0, 255)
    return np.moveaxis(out, 0, axis), lo_v, hi_v, coefs.shape[1]
