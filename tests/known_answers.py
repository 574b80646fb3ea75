"""Hand-derived known answers for the [upstream] pieces that cannot be pinned against ultralytics / torchvision here
(reference call sites players_tracker.py:351-359, players_keypoints_tracker.py:285-299): the
Detect / Pose inference branch (DFL expectation, dist2bbox, keypoint decode), ops.non_max_suppression (strict
``score > conf``, strict ``IoU > thr``, stable order on equal scores, the per-class 7680 offset, ``classes=``) and
scale_boxes / scale_coords (rounded vs unrounded letterbox pads, clamping).  Every expected number below is worked out
in the comments from the published formulas — none is produced by running code.  The same cases go through the CPU
oracle (tests/test_known_answers_oracle.py) and through the HIP decode / NMS kernels (tests/test_gpu_known_answers.py).

Head-map layout (pa_yolo_head_shape): per level (n, H_l, W_l, c): channels [0, 64) = DFL logits, side-major
(left, top, right, bottom) x 16 bins; [64, 64 + nc) class logits; then nk keypoint values.  Source frames are
720 x 1280 -> network 384 x 640 (gain 1/2, letterbox pads: x 0, y 12), levels 48x80 / 24x40 / 12x20 at strides 8 / 16 / 32.
GEOMETRY_ODD, odd_detect_cases and odd_pose_cases are the same for sources where the left pad is not 0, top != bottom, the rounded and
the unrounded pad differ, the frame is upscaled or the head maps are taller than wide (tests/test_letterbox_geometry_host.py on the CPU,
tests/test_gpu_geometry.py through the kernels)."""
import numpy as np

H0, W0, IMGSZ = 720, 1280, 640
LEVELS = [(48, 80, 8), (24, 40, 16), (12, 20, 32)]
OFF = -20.0            # class logit of every untouched anchor: sigmoid = 2e-9, far below any threshold
HOT = 50.0             # DFL logit of the chosen bin: softmax = 1 - 15 e^-50, expectation == the bin index in fp32


def blank_heads(n, c):
    heads = [np.zeros((n, h, w, c), np.float32) for (h, w, _) in LEVELS]
    return heads


def put(heads, img, level, y, x, ltrb=None, cls_logits=None, nc=1, kpts=None):
    """One anchor: DFL one-hot at integer distances ltrb (None: all-zero logits = uniform bins, expectation 7.5 each)."""
    t = heads[level][img, y, x]
    if ltrb is not None:
        for side, d in enumerate(ltrb):
            t[side * 16 + d] = HOT
    for k, v in enumerate(cls_logits):
        t[64 + k] = v
    if kpts is not None:
        t[64 + nc:64 + nc + len(kpts)] = kpts


def detect_cases():
    """nc = 2.  Returns (heads, expected) with expected[img] = list of rows [x1, y1, x2, y2, score, cls] in output
    order, for conf = 0.5, iou = 0.7, classes = None."""
    nc, c = 2, 68
    heads = blank_heads(4, c)
    for hd in heads:
        hd[..., 64:64 + nc] = OFF
    sig = lambda v: float(1.0 / (1.0 + np.exp(-np.float64(v))))
    exp = {}
    # ---- image 0: dist2bbox + scale_boxes.
    # level 0 (stride 8), cell (y 10, x 20): anchor centre (20.5, 10.5); l, t, r, b = 2, 3, 4, 5 cells
    #   x1 = 20.5 - 2 = 18.5, y1 = 10.5 - 3 = 7.5, x2 = 24.5, y2 = 15.5  -> x 8: (148, 60, 196, 124) network px
    #   scale_boxes: minus pad (0, 12) -> (148, 48, 196, 112); / gain 0.5 -> (296, 96, 392, 224)
    put(heads, 0, 0, 10, 20, (2, 3, 4, 5), (2.0, OFF), nc)
    # level 1 (stride 16), cell (5, 5), all DFL logits zero: uniform over bins 0..15 -> every distance 7.5
    #   (5.5 -+ 7.5) * 16 = (-32, -32, 208, 208); minus pad -> (-32, -44, 208, 196); / 0.5 -> (-64, -88, 416, 392); clamp to
    #   [0, 1280] x [0, 720] -> (0, 0, 416, 392).  class 1 wins (logit 1.0 vs 0.5)
    put(heads, 0, 1, 5, 5, None, (0.5, 1.0), nc)
    # an anchor whose best logit is exactly 0: sigmoid = 0.5, and the filter is STRICT (score > conf) -> no detection
    put(heads, 0, 0, 30, 60, (1, 1, 1, 1), (0.0, OFF), nc)
    # bottom-right corner cell of level 2 (stride 32), cell (11, 19): centre (19.5, 11.5), l, t, r, b = 1, 1, 15, 15
    #   (18.5, 10.5, 34.5, 26.5) * 32 = (592, 336, 1104, 848); minus pad -> (592, 324, 1104, 836); / 0.5 ->
    #   (1184, 648, 2208, 1672) -> clamp (1184, 648, 1280, 720)
    put(heads, 0, 2, 11, 19, (1, 1, 15, 15), (3.0, OFF), nc)
    exp[0] = [[1184, 648, 1280, 720, sig(3.0), 0], [296, 96, 392, 224, sig(2.0), 0], [0, 0, 416, 392, sig(1.0), 1]]
    # ---- image 1: NMS.  All on level 2 (stride 32), class 0.
    #   A: cell (5, 5), l t r b = 5 5 5 5: (0.5, 0.5, 10.5, 10.5) * 32 = (16, 16, 336, 336), area 102400, score sig(2.2)
    #   B: cell (4, 5) [y 4, x 5], l t r b = 5 4 5 3: x (0.5, 10.5), y (0.5, 7.5) -> (16, 16, 336, 240), area 71680 = 0.7 * area A,
    #      B inside A: IoU(A, B) = 71680 / 102400 = float32(0.7) — NOT greater than the threshold float32(0.7): B is KEPT
    #   C: cell (5, 4) [y 5, x 4], l t r b = 4 5 6 3: x (0.5, 10.5), y (0.5, 8.5) -> (16, 16, 336, 272), area 81920:
    #      IoU(A, C) = 0.8 > 0.7 -> suppressed by A (higher score)
    #   D: far away, same score as B (equal logits): stable order -> B (lower anchor index) before D
    put(heads, 1, 2, 5, 5, (5, 5, 5, 5), (2.2, OFF), nc)
    put(heads, 1, 2, 4, 5, (5, 4, 5, 3), (1.5, OFF), nc)
    put(heads, 1, 2, 5, 4, (4, 5, 6, 3), (2.0, OFF), nc)
    put(heads, 1, 2, 9, 15, (1, 1, 1, 1), (1.5, OFF), nc)
    #   scale: A (16, 16, 336, 336) -> minus (0, 12) -> (16, 4, 336, 324) -> x2: (32, 8, 672, 648)
    #          B (16, 16, 336, 240) -> (16, 4, 336, 228) -> (32, 8, 672, 456)
    #          D cell (9, 15): centre (15.5, 9.5) -+ 1 -> (14.5, 8.5, 16.5, 10.5) * 32 = (464, 272, 528, 336) -> (464, 260, 528, 324) -> (928, 520, 1056, 648)
    exp[1] = [[32, 8, 672, 648, sig(2.2), 0], [32, 8, 672, 456, sig(1.5), 0], [928, 520, 1056, 648, sig(1.5), 0]]
    # ---- image 2: the class offset.  Two anchors produce the SAME box (16, 16, 336, 336): cell (5, 5) with l r = 5 5 and
    #   cell (5, 4) with l r = 4 6; one is class 0, the other class 1 -> boxes are shifted by cls * 7680 before NMS:
    #   no overlap, both kept.  A third, class-0 copy of the box from cell (5, 6) [l r = 6 4] with a lower score IS suppressed (IoU 1).
    put(heads, 2, 2, 5, 5, (5, 5, 5, 5), (2.0, OFF), nc)
    put(heads, 2, 2, 5, 4, (4, 5, 6, 5), (OFF, 1.0), nc)
    put(heads, 2, 2, 5, 6, (6, 5, 4, 5), (0.8, OFF), nc)
    exp[2] = [[32, 8, 672, 648, sig(2.0), 0], [32, 8, 672, 648, sig(1.0), 1]]
    # ---- image 3: nothing above the threshold
    exp[3] = []
    return nc, heads, exp


def detect_cases_class_filter():
    """The same heads with classes=[1]: only class-1 rows survive (upstream filters BEFORE nms)."""
    nc, heads, exp = detect_cases()
    return nc, heads, {i: [r for r in rows if r[5] == 1] for i, rows in exp.items()}


def pose_cases():
    """nc = 1, 13 keypoints x 3.  One anchor; conf 0.25.
    level 0 (stride 8), cell (y 10, x 20): box l t r b = 2 3 4 5 -> (296, 96, 392, 224) as in detect image 0.
    keypoint k raw (vx, vy, vl): x = (vx * 2 + 20) * 8, y = (vy * 2 + 10) * 8 (anchor - 0.5 = the cell index), vis = sigmoid(vl);
    scale_coords uses the UNROUNDED pads (0, 12.0): ((x - 0) / 0.5, (y - 12) / 0.5), clamped to the frame.
      k0: (0.25, 0.75, 4.0)  -> x = 20.5 * 8 = 164 -> 328;  y = 11.5 * 8 = 92 -> (92 - 12) / 0.5 = 160
      k1: (-1.0, -0.5, -4.0) -> x = 18 * 8 = 144 -> 288;    y = 9 * 8 = 72 -> 120        (visibility 0.018: Keypoints.xy zeroes it)
      k2: (100, 100, 0.0)    -> clamp: x -> 1280, y -> 720   (visibility exactly 0.5: NOT < 0.5, kept)
      others: (0, 0, OFF)    -> x = 160 -> 320, y = 80 -> 136"""
    nc, nk, c = 1, 39, 104
    heads = blank_heads(1, c)
    for hd in heads:
        hd[..., 64] = OFF
    k = np.zeros((13, 3), np.float32)
    k[:, 2] = OFF
    k[0] = (0.25, 0.75, 4.0)
    k[1] = (-1.0, -0.5, -4.0)
    k[2] = (100.0, 100.0, 0.0)
    put(heads, 0, 0, 10, 20, (2, 3, 4, 5), (1.0,), nc, k.reshape(-1))
    sig = lambda v: float(1.0 / (1.0 + np.exp(-np.float64(v))))
    ek = np.zeros((13, 3), np.float64)
    ek[:, 0], ek[:, 1], ek[:, 2] = 320.0, 136.0, sig(OFF)
    ek[0] = (328.0, 160.0, sig(4.0))
    ek[1] = (288.0, 120.0, sig(-4.0))
    ek[2] = (1280.0, 720.0, 0.5)
    return nc, (13, 3), heads, [[296, 96, 392, 224, sig(1.0), 0]], ek


GEOMETRY = [
    # (h0, w0) -> LetterBox(640, auto, stride 32): resized (w, h), (top, bottom, left, right), network (h, w); scale_boxes gain, pads
    # 720p: r = min(640/720, 640/1280) = 0.5 -> 640 x 360; dh = 280 % 32 = 24 -> 12 + 12 (round(11.9), round(12.1))
    ((720, 1280), (640, 360), (12, 12, 0, 0), (384, 640), 0.5, (0, 12)),
    # 1080p: r = 1/3 -> 640 x 360, same pads; scale_boxes gain = min(384/1080, 640/1920) = 1/3, pad_y = round((384 - 360)/2 - 0.1) = 12
    ((1080, 1920), (640, 360), (12, 12, 0, 0), (384, 640), 1.0 / 3.0, (0, 12)),
    # 480 x 854: r = min(1.333, 0.74941) -> round(854 r) = 640, round(480 r) = round(359.72) = 360; same pads;
    # scale_boxes gain = min(384/480, 640/854) = 0.749414..., pad_y = round((384 - 359.719) / 2 - 0.1) = round(12.04) = 12
    ((480, 854), (640, 360), (12, 12, 0, 0), (384, 640), 640.0 / 854.0, (0, 12)),
    # square: nothing to do
    ((640, 640), (640, 640), (0, 0, 0, 0), (640, 640), 1.0, (0, 0)),
    # 600 x 800 (odd pad): r = 0.8 -> 640 x 480; dh = 160 % 32 = 0 -> no pad
    ((600, 800), (640, 480), (0, 0, 0, 0), (480, 640), 0.8, (0, 0)),
    # 500 x 1000: r = 0.64 -> 640 x 320; dh = 320 % 32 = 0
    ((500, 1000), (640, 320), (0, 0, 0, 0), (320, 640), 0.64, (0, 0)),
    # 700 x 1000: r = 0.64 -> 640 x 448; dh = 192 % 32 = 0
    ((700, 1000), (640, 448), (0, 0, 0, 0), (448, 640), 0.64, (0, 0)),
    # 725 x 1280: r = 0.5 -> 640 x round(362.5) = 362 (banker's rounding of Python's round); dh = 278 % 32 = 22 -> 11 + 11
    ((725, 1280), (640, 362), (11, 11, 0, 0), (384, 640), 0.5, (0, 11)),
]


# Odd source geometries: the smallest sizes at which a left pad, top != bottom, a rounded pad that differs from the unrounded one, an
# upscale and a portrait network input appear (all of them absent from the four sources above).  One dict per row:
#   hw (h0, w0), imgsz, auto (LetterBox auto: pad to a multiple of 32 instead of to imgsz), resized (w, h), pads (top, bottom, left,
#   right), net (h, w), mode (0 copy, 1 exact 2 x 2 area, 2 bilinear tables), gain, box_pad (x, y) = what scale_boxes subtracts
#   (rounded), kpt_pad (x, y) = what scale_coords subtracts (unrounded).
# The formulas ([upstream] LetterBox.__call__, ops.scale_boxes, ops.scale_coords; round = Python's, half to even):
#   r = min(S / h0, S / w0); resized = (round(w0 r), round(h0 r)); dw, dh = S - resized w, h; auto: both mod 32; halved;
#   top, bottom = round(dh - 0.1), round(dh + 0.1); left, right = round(dw - 0.1), round(dw + 0.1); net = resized + pads;
#   mode 0 if nothing is resized, 1 if the source is exactly twice the resized size in both directions (cv2's area path), else 2;
#   gain = min(net h / h0, net w / w0); kpt_pad = ((net w - w0 gain) / 2, (net h - h0 gain) / 2); box_pad = round(kpt_pad - 0.1).
# gain and kpt_pad of the rows with a gain that is no binary fraction are written as the exact quotient (the decimal beside it).
def _row(name, hw, imgsz, resized, pads, net, mode, gain, box_pad, kpt_pad, auto=True):
    return dict(name=name, hw=hw, imgsz=imgsz, auto=auto, resized=resized, pads=pads, net=net, mode=mode, gain=gain, box_pad=box_pad,
                kpt_pad=kpt_pad)


GEOMETRY_ODD = [
    # 1. 77 x 160 @160 — copy mode, odd pad.  r = min(2.078, 1) = 1 -> 160 x 77, nothing resized (mode 0); dw = 0;
    #    dh = 83 mod 32 = 19 -> 9.5: top = round(9.4) = 9, bottom = round(9.6) = 10; net = (77 + 19) x 160 = 96 x 160.
    #    gain = min(96/77 = 1.247, 160/160) = 1; kpt_pad = (0, (96 - 77) / 2) = (0, 9.5); box_pad = (round(-0.1), round(9.4)) = (0, 9)
    _row("1: 77x160@160", (77, 160), 160, (160, 77), (9, 10, 0, 0), (96, 160), 0, 1.0, (0, 9), (0.0, 9.5)),
    # 2. 320 x 200 @320 — copy mode, portrait.  r = min(1, 1.6) = 1 -> 200 x 320 (mode 0); dh = 0; dw = 120 mod 32 = 24 -> 12:
    #    left = round(11.9) = 12, right = round(12.1) = 12; net = 320 x 224.  gain = min(1, 224/200 = 1.12) = 1; kpt_pad = (12, 0);
    #    box_pad = (round(11.9), 0) = (12, 0)
    _row("2: 320x200@320", (320, 200), 320, (200, 320), (0, 0, 12, 12), (320, 224), 0, 1.0, (12, 0), (12.0, 0.0)),
    # 3. 362 x 640 @320 — the 2 x 2 area mode with an odd pad.  r = min(0.884, 0.5) = 0.5 -> 320 x 181, the source is exactly twice
    #    that (mode 1); dh = 139 mod 32 = 11 -> 5.5: top = round(5.4) = 5, bottom = round(5.6) = 6; net = 192 x 320.
    #    gain = min(192/362 = 0.530, 0.5) = 0.5; kpt_pad = (0, (192 - 181) / 2) = (0, 5.5); box_pad = (0, round(5.4)) = (0, 5)
    _row("3: 362x640@320", (362, 640), 320, (320, 181), (5, 6, 0, 0), (192, 320), 1, 0.5, (0, 5), (0.0, 5.5)),
    # 4. 201 x 333 @320 — bilinear downscale.  r = min(1.592, 320/333 = 0.960960...) -> w = 320, h = round(201 * 0.96096 = 193.153) = 193
    #    (mode 2); dh = 127 mod 32 = 31 -> 15.5: top = round(15.4) = 15, bottom = round(15.6) = 16; net = (193 + 31) x 320 = 224 x 320.
    #    gain = min(224/201 = 1.114, 320/333) = 320/333; kpt_pad y = (224 - 201 * 320/333) / 2 = (224 - 193.153153) / 2 = 15.423423...;
    #    box_pad y = round(15.323) = 15; x: (320 - 333 * 320/333) / 2 = 0
    _row("4: 201x333@320", (201, 333), 320, (320, 193), (15, 16, 0, 0), (224, 320), 2, 320.0 / 333.0, (0, 15),
         (0.0, (224.0 - 201.0 * 320.0 / 333.0) / 2.0)),
    # 5. 333 x 201 @320 — row 4 transposed: resized 193 x 320, left 15, right 16, net 320 x 224, pads and gain with x and y swapped
    _row("5: 333x201@320", (333, 201), 320, (193, 320), (0, 0, 15, 16), (320, 224), 2, 320.0 / 333.0, (15, 0),
         ((224.0 - 201.0 * 320.0 / 333.0) / 2.0, 0.0)),
    # 6. 97 x 131 @320 — upscale 2.44 x.  r = min(3.299, 320/131 = 2.442748) -> w = 320, h = round(97 * 2.442748 = 236.947) = 237 (mode 2);
    #    dh = 83 mod 32 = 19 -> 9.5: top 9, bottom 10; net = (237 + 19) x 320 = 256 x 320.  gain = min(256/97 = 2.639, 320/131) = 320/131;
    #    kpt_pad y = (256 - 97 * 320/131) / 2 = (256 - 236.946565) / 2 = 9.526718; box_pad y = round(9.427) = 9
    _row("6: 97x131@320", (97, 131), 320, (320, 237), (9, 10, 0, 0), (256, 320), 2, 320.0 / 131.0, (0, 9),
         (0.0, (256.0 - 97.0 * 320.0 / 131.0) / 2.0)),
    # 7. 363 x 640 @320 — r = 0.5 but not the 2 x 2 mode.  w = 320, h = round(181.5) = 182 (half to even); 363 != 2 * 182 -> mode 2;
    #    dh = 138 mod 32 = 10 -> 5: top = round(4.9) = 5, bottom = round(5.1) = 5; net = 192 x 320.  gain = min(192/363 = 0.529, 0.5) = 0.5;
    #    kpt_pad y = (192 - 181.5) / 2 = 5.25; box_pad y = round(5.15) = 5
    _row("7: 363x640@320", (363, 640), 320, (320, 182), (5, 5, 0, 0), (192, 320), 2, 0.5, (0, 5), (0.0, 5.25)),
    # 8. 64 x 48 @160 — upscale 2.5 x, portrait.  r = min(2.5, 3.333) = 2.5 -> 120 x 160 (mode 2); dh = 0; dw = 40 mod 32 = 8 -> 4:
    #    left = round(3.9) = 4, right = round(4.1) = 4; net = 160 x 128.  gain = min(2.5, 128/48 = 2.667) = 2.5;
    #    kpt_pad x = (128 - 120) / 2 = 4; box_pad x = round(3.9) = 4
    _row("8: 64x48@160", (64, 48), 160, (120, 160), (0, 0, 4, 4), (160, 128), 2, 2.5, (4, 0), (4.0, 0.0)),
    # 9. 131 x 97 @160 — the rounded pad ABOVE the unrounded one.  r = min(160/131 = 1.221374, 1.649) -> h = 160,
    #    w = round(97 * 1.221374 = 118.473) = 118 (mode 2); dw = 42 mod 32 = 10 -> 5: left = round(4.9) = 5, right = round(5.1) = 5;
    #    net = 160 x 128.  gain = min(160/131, 128/97 = 1.320) = 160/131; kpt_pad x = (128 - 97 * 160/131) / 2 = (128 - 118.473282) / 2
    #    = 4.763359; box_pad x = round(4.663) = 5
    _row("9: 131x97@160", (131, 97), 160, (118, 160), (0, 0, 5, 5), (160, 128), 2, 160.0 / 131.0, (5, 0),
         ((128.0 - 97.0 * 160.0 / 131.0) / 2.0, 0.0)),
    # 10. 768 x 1366 @640 — a laptop panel.  r = min(0.833, 640/1366 = 0.468521) -> w = 640, h = round(768 * 0.468521 = 359.824) = 360
    #    (mode 2); dh = 280 mod 32 = 24 -> 12: top = round(11.9) = 12, bottom = round(12.1) = 12; net = 384 x 640.
    #    gain = min(0.5, 640/1366) = 640/1366; kpt_pad y = (384 - 768 * 640/1366) / 2 = (384 - 359.824305) / 2 = 12.087848;
    #    box_pad y = round(11.988) = 12
    _row("10: 768x1366@640", (768, 1366), 640, (640, 360), (12, 12, 0, 0), (384, 640), 2, 640.0 / 1366.0, (0, 12),
         (0.0, (384.0 - 768.0 * 640.0 / 1366.0) / 2.0)),
]
# LetterBox(auto=False) (what upstream uses when the shapes of a batch differ): the pads fill up to imgsz x imgsz.  For the network
# input only — scale_boxes / scale_coords of these are not part of the rows' use.
#   1: dh = 83 -> 41.5: top = round(41.4) = 41, bottom = round(41.6) = 42; net 160 x 160; gain = min(160/77, 1) = 1, kpt_pad y = 41.5
#   4: dh = 320 - 193 = 127 -> 63.5: top = round(63.4) = 63, bottom = round(63.6) = 64; net 320 x 320; gain = min(320/201, 320/333)
#      = 320/333, kpt_pad y = (320 - 193.153153) / 2 = 63.423423, box_pad y = round(63.323) = 63
GEOMETRY_ODD_NO_AUTO = [
    _row("1 auto=False: 77x160@160", (77, 160), 160, (160, 77), (41, 42, 0, 0), (160, 160), 0, 1.0, (0, 41), (0.0, 41.5), auto=False),
    _row("4 auto=False: 201x333@320", (201, 333), 320, (320, 193), (63, 64, 0, 0), (320, 320), 2, 320.0 / 333.0, (0, 63),
         (0.0, (320.0 - 201.0 * 320.0 / 333.0) / 2.0), auto=False),
]



# Rescale known answers at rows of GEOMETRY_ODD (index, 0-based): decode + scale_boxes / scale_coords where the left pad is not 0, the
# rounded and the unrounded pad differ, the head maps are taller than wide and the frame edge is not 1280 / 720.  Where the gain is a
# binary fraction or 2.5 the expected numbers are literal; at row 9 (gain 160/131) the NUMERATORS (network pixels minus the pad) are
# literal and the expectation is their float32 quotient by float32(gain) — the one rounding scale_boxes / scale_coords make
# (keypoints: float32(x) - float32(kpt_pad) first, then the quotient); the decimals in the comments are the real-number values.
def levels_of(net):
    return [(net[0] >> (3 + l), net[1] >> (3 + l), 8 << l) for l in range(3)]


def blank_heads_net(net, n, nc, nk):
    """Head maps for a network input ``net`` (h, w), 64 + nc + nk channels rounded up to 4 (the engine's head buffers), every class
    logit OFF."""
    c = (64 + nc + nk + 3) // 4 * 4
    heads = [np.zeros((n, h, w, c), np.float32) for (h, w, _) in levels_of(net)]
    for hd in heads:
        hd[..., 64:64 + nc] = OFF
    return heads


def _sig(v):
    return float(1.0 / (1.0 + np.exp(-np.float64(v))))


def _q(num, gain):
    """float32(num) / float32(gain), the quotient scale_boxes / scale_coords compute."""
    return float(np.float32(num) / np.float32(gain))


def _qk(x, kpad, gain):
    return float((np.float32(x) - np.float32(kpad)) / np.float32(gain))


def odd_detect_cases():
    """nc = 2, conf 0.5, iou 0.7, one image per row.  -> list of (row index into GEOMETRY_ODD, heads, expected rows
    [x1, y1, x2, y2, score, cls] in output order = descending score)."""
    nc, out = 2, []
    # ---- row 1 (index 0): 77 x 160, net 96 x 160, levels 12x20 / 6x10 / 3x5, gain 1, box pad (0, 9); frame edges w0 160, h0 77
    g = GEOMETRY_ODD[0]
    heads = blank_heads_net(g["net"], 1, nc, 0)
    # level 0 (stride 8), cell (y 6, x 10): centre (10.5, 6.5), l t r b = 2 3 4 4 -> (8.5, 3.5, 14.5, 10.5) * 8 = (68, 28, 116, 84);
    #   minus (0, 9) -> (68, 19, 116, 75); gain 1; inside the frame.  (With the unrounded 9.5 it would be y 18.5 / 74.5.)
    put(heads, 0, 0, 6, 10, (2, 3, 4, 4), (2.0, OFF), nc)
    # level 2 (stride 32), its last row and column, cell (y 2, x 4): centre (4.5, 2.5), l t r b = 1 1 15 15 ->
    #   (3.5, 1.5, 19.5, 17.5) * 32 = (112, 48, 624, 560); minus (0, 9) -> (112, 39, 624, 551); clamp to w0 160, h0 77 -> (112, 39, 160, 77)
    put(heads, 0, 2, 2, 4, (1, 1, 15, 15), (3.0, OFF), nc)
    # level 1 (stride 16), cell (0, 0), all-zero DFL logits: every distance 7.5 -> (0.5 -+ 7.5) * 16 = (-112, -112, 128, 128);
    #   minus (0, 9) -> (-112, -121, 128, 119); clamp -> (0, 0, 128, 77).  class 1.
    #   (NMS, network pixels: the level-0 box lies inside this one, IoU = 48 * 56 / 240^2 = 0.047; other class anyway)
    put(heads, 0, 1, 0, 0, None, (OFF, 1.0), nc)
    out.append((0, heads, [[112, 39, 160, 77, _sig(3.0), 0], [68, 19, 116, 75, _sig(2.0), 0], [0, 0, 128, 77, _sig(1.0), 1]]))
    # ---- row 2 (index 1): 320 x 200, net 320 x 224, levels 40x28 / 20x14 / 10x7 (taller than wide), gain 1, box pad (12, 0);
    #      frame edges w0 200, h0 320
    g = GEOMETRY_ODD[1]
    heads = blank_heads_net(g["net"], 1, nc, 0)
    # level 0, last row and column, cell (y 39, x 27): centre (27.5, 39.5), l t r b = 3 2 1 1 -> (24.5, 37.5, 28.5, 40.5) * 8 =
    #   (196, 300, 228, 324); minus (12, 0) -> (184, 300, 216, 324); clamp -> (184, 300, 200, 320)
    put(heads, 0, 0, 39, 27, (3, 2, 1, 1), (3.0, OFF), nc)
    # level 1, last row and column, cell (y 19, x 13): centre (13.5, 19.5), l t r b = 5 6 0 0 -> (8.5, 13.5, 13.5, 19.5) * 16 =
    #   (136, 216, 216, 312); minus (12, 0) -> (124, 216, 204, 312); clamp -> (124, 216, 200, 312).  class 1
    put(heads, 0, 1, 19, 13, (5, 6, 0, 0), (OFF, 2.5), nc)
    # level 2, last row and column, cell (y 9, x 6): centre (6.5, 9.5), l t r b = 4 7 0 0 -> (2.5, 2.5, 6.5, 9.5) * 32 = (80, 80, 208, 304);
    #   minus (12, 0) -> (68, 80, 196, 304); inside the frame
    put(heads, 0, 2, 9, 6, (4, 7, 0, 0), (2.0, OFF), nc)
    # level 0, cell (y 20, x 3) — row 20 of a map 28 wide is anchor 563; read with the map's HEIGHT (40) as the row length it would be
    #   (y 14, x 3): centre (3.5, 20.5), l t r b = 1 1 1 1 -> (2.5, 19.5, 4.5, 21.5) * 8 = (20, 156, 36, 172); minus (12, 0) -> (8, 156, 24, 172)
    #   (NMS: level-0 corner vs level-2 box overlap 12 x 4 px, level-2 vs level-1 72 x 88 = 6336 of a union 30016: IoU 0.21)
    put(heads, 0, 0, 20, 3, (1, 1, 1, 1), (1.5, OFF), nc)
    out.append((1, heads, [[184, 300, 200, 320, _sig(3.0), 0], [124, 216, 200, 312, _sig(2.5), 1], [68, 80, 196, 304, _sig(2.0), 0],
                           [8, 156, 24, 172, _sig(1.5), 0]]))
    # ---- row 9 (index 8): 131 x 97, net 160 x 128, levels 20x16 / 10x8 / 5x4, gain 160/131 (1 / gain = 0.81875), box pad (5, 0) —
    #      ABOVE the unrounded 4.763; frame edges w0 97, h0 131
    g = GEOMETRY_ODD[8]
    gn = g["gain"]
    heads = blank_heads_net(g["net"], 1, nc, 0)
    # level 0, cell (y 10, x 6): centre (6.5, 10.5), l t r b = 2 3 4 5 -> (4.5, 7.5, 10.5, 15.5) * 8 = (36, 60, 84, 124); minus (5, 0) ->
    #   (31, 60, 79, 124); * 0.81875 -> (25.38125, 49.125, 64.68125, 101.525)        (with 4.763: x 25.575 / 64.875)
    put(heads, 0, 0, 10, 6, (2, 3, 4, 5), (2.0, OFF), nc)
    # level 2, last row and column, cell (y 4, x 3): centre (3.5, 4.5), l t r b = 1 1 15 15 -> (2.5, 3.5, 18.5, 19.5) * 32 =
    #   (80, 112, 592, 624); minus (5, 0) -> (75, 112, 587, 624); * 0.81875 -> (61.40625, 91.7, 480.6, 510.9) -> clamp (.., .., 97, 131)
    put(heads, 0, 2, 4, 3, (1, 1, 15, 15), (3.0, OFF), nc)
    out.append((8, heads, [[_q(75, gn), _q(112, gn), 97, 131, _sig(3.0), 0], [_q(31, gn), _q(60, gn), _q(79, gn), _q(124, gn), _sig(2.0), 0]]))
    # ---- row 8 (index 7), the bilinear row: 64 x 48, net 160 x 128, levels as above, gain 2.5, box pad (4, 0); edges w0 48, h0 64
    g = GEOMETRY_ODD[7]
    heads = blank_heads_net(g["net"], 1, nc, 0)
    # level 0, cell (y 10, x 6), l t r b = 2 3 4 5: (36, 60, 84, 124) as above; minus (4, 0) -> (32, 60, 80, 124); / 2.5 -> (12.8, 24, 32, 49.6)
    put(heads, 0, 0, 10, 6, (2, 3, 4, 5), (2.0, OFF), nc)
    # level 1, last row and column, cell (y 9, x 7): centre (7.5, 9.5), l t r b = 3 4 0 0 -> (4.5, 5.5, 7.5, 9.5) * 16 = (72, 88, 120, 152);
    #   minus (4, 0) -> (68, 88, 116, 152); / 2.5 -> (27.2, 35.2, 46.4, 60.8).  class 1
    put(heads, 0, 1, 9, 7, (3, 4, 0, 0), (OFF, 2.5), nc)
    # level 2, last row and column, cell (y 4, x 3), l t r b = 1 1 15 15: (80, 112, 592, 624); minus (4, 0) -> (76, 112, 588, 624); / 2.5 ->
    #   (30.4, 44.8, 235.2, 249.6) -> clamp (30.4, 44.8, 48, 64)
    put(heads, 0, 2, 4, 3, (1, 1, 15, 15), (3.0, OFF), nc)
    out.append((7, heads, [[30.4, 44.8, 48, 64, _sig(3.0), 0], [27.2, 35.2, 46.4, 60.8, _sig(2.5), 1], [12.8, 24, 32, 49.6, _sig(2.0), 0]]))
    return nc, out


def odd_pose_cases(kpt_shape=(13, 3)):
    """nc = 1, conf 0.25, one anchor per row.  keypoint k raw (vx, vy[, vl]) at cell (cx, cy), stride s: x = (2 vx + cx) s, y = (2 vy + cy) s
    in network pixels; scale_coords subtracts the UNROUNDED pad, divides by the gain and clamps to the frame.  The first four keypoints
    are set, the others are raw (0, 0[, OFF]).  -> list of (row index, heads, [box row], expected (K, dim) array)."""
    K, dim = kpt_shape
    nc, nk, out = 1, K * dim, []

    def case(row, level, y, x, ltrb, raw4, box, xy4, rest):
        g = GEOMETRY_ODD[row]
        heads = blank_heads_net(g["net"], 1, nc, nk)
        k = np.zeros((K, dim), np.float32)
        vis = (4.0, -4.0, 0.0, 0.0)
        if dim == 3:
            k[:, 2] = OFF
        for i, v in enumerate(raw4):
            k[i, :2] = v
            if dim == 3:
                k[i, 2] = vis[i]
        put(heads, 0, level, y, x, ltrb, (1.0,), nc, k.reshape(-1))
        ek = np.zeros((K, dim), np.float64)
        ek[:, :2] = rest
        ek[:4, :2] = xy4
        if dim == 3:
            ek[:, 2] = _sig(OFF)
            ek[:4, 2] = [_sig(v) for v in vis]
        out.append((row, heads, [list(box) + [_sig(1.0), 0]], ek))

    # ---- row 1 (index 0): gain 1, keypoint pad (0, 9.5), box pad (0, 9).  level 0 (stride 8), cell (y 6, x 10), box as in odd_detect_cases:
    #   (68, 19, 116, 75).
    #   k0 (0.25, 0.75): x = (0.5 + 10) * 8 = 84, y = (1.5 + 6) * 8 = 60 -> (84, 60 - 9.5) = (84, 50.5)      [the box moved by 9, this by 9.5]
    #   k1 (-1, -0.5):   x = (-2 + 10) * 8 = 64,  y = (-1 + 6) * 8 = 40  -> (64, 30.5)
    #   k2 (100, 100):   far outside -> clamp to (w0, h0) = (160, 77)
    #   k3 (-100, -100): -> clamp (0, 0)
    #   others (0, 0):   x = 80, y = 48 -> (80, 38.5)
    case(0, 0, 6, 10, (2, 3, 4, 4), [(0.25, 0.75), (-1.0, -0.5), (100.0, 100.0), (-100.0, -100.0)], (68, 19, 116, 75),
         [(84, 50.5), (64, 30.5), (160, 77), (0, 0)], (80, 38.5))
    # ---- row 2 (index 1): gain 1, both pads (12, 0).  level 1 (stride 16), last row and column, cell (y 19, x 13), l t r b = 5 6 0 0:
    #   box (124, 216, 200, 312) as in odd_detect_cases.
    #   k0 (-1.5, -2): x = (-3 + 13) * 16 = 160, y = (-4 + 19) * 16 = 240 -> (148, 240)
    #   k1 (0.25, 0.75): x = 13.5 * 16 = 216 -> 204 -> clamp 200 (w0); y = 20.5 * 16 = 328 -> clamp 320 (h0)
    #   k2 (100, 100) -> (200, 320);  k3 (-100, -100) -> (0, 0)
    #   others (0, 0): x = 208 - 12 = 196 (a row length of 20 instead of 14 would put the cell at x 19 * 14 + 13 = 279 -> 279 % 20 = 19), y = 304
    case(1, 1, 19, 13, (5, 6, 0, 0), [(-1.5, -2.0), (0.25, 0.75), (100.0, 100.0), (-100.0, -100.0)], (124, 216, 200, 312),
         [(148, 240), (200, 320), (200, 320), (0, 0)], (196, 304))
    # ---- row 9 (index 8): gain 160/131, keypoint pad (4.763359, 0), box pad (5, 0).  level 0, cell (y 10, x 6), l t r b = 2 3 4 5:
    #   box numerators (31, 60, 79, 124) as in odd_detect_cases.
    #   k0 (0.25, 0.75): x = 6.5 * 8 = 52, y = 11.5 * 8 = 92 -> ((52 - 4.763359) * 0.81875, 92 * 0.81875) = (38.675, 75.325)
    #                    (with the box's pad 5: x 38.481 — 0.19 px away)
    #   k1 (-1, -0.5):   x = 4 * 8 = 32, y = 9 * 8 = 72 -> (22.300, 58.95)
    #   k2 (100, 100) -> (97, 131);  k3 (-100, -100) -> (0, 0)
    #   others (0, 0):   x = 48, y = 80 -> (35.400, 65.5)
    g = GEOMETRY_ODD[8]
    gn, kx = g["gain"], g["kpt_pad"][0]
    case(8, 0, 10, 6, (2, 3, 4, 5), [(0.25, 0.75), (-1.0, -0.5), (100.0, 100.0), (-100.0, -100.0)],
         (_q(31, gn), _q(60, gn), _q(79, gn), _q(124, gn)),
         [(_qk(52, kx, gn), _q(92, gn)), (_qk(32, kx, gn), _q(72, gn)), (97, 131), (0, 0)], (_qk(48, kx, gn), _q(80, gn)))
    # ---- row 8 (index 7), the bilinear row: gain 2.5, both pads (4, 0).  level 0, cell (y 10, x 6), l t r b = 2 3 4 5: box (12.8, 24, 32, 49.6)
    #   k0 (0.25, 0.75): (52, 92) -> (48 / 2.5, 92 / 2.5) = (19.2, 36.8)
    #   k1 (-1, -0.5):   (32, 72) -> (28 / 2.5, 72 / 2.5) = (11.2, 28.8)
    #   k2 (100, 100) -> (48, 64);  k3 (-100, -100) -> (0, 0)
    #   others (0, 0):   (48, 80) -> (17.6, 32)
    case(7, 0, 10, 6, (2, 3, 4, 5), [(0.25, 0.75), (-1.0, -0.5), (100.0, 100.0), (-100.0, -100.0)], (12.8, 24, 32, 49.6),
         [(19.2, 36.8), (11.2, 28.8), (48, 64), (0, 0)], (17.6, 32))
    return nc, out


# ---------------------------------------------------------------------------------------------------------------------
# Heat-map decode ties (reference predict.py:21-33): ``predict_location`` keeps the FIRST rectangle of maximal w * h
# (strict ``>``, bounding-box area, not pixel count) in the order ``cv2.findContours(mask, RETR_EXTERNAL, ...)`` returns the
# contours.  cv2 is not installable here; the CHOSEN rule (oracle/ball_ref.py, trackers/ball_tracker.py:predict_location, the
# device kernel csrc/tracknet_post.hip:ball_locate_kernel): contours come back in REVERSE raster-discovery order — a raster
# scan (row by row, left to right) discovers a component at its first foreground pixel, the component discovered LAST is
# returned first — so among equal-area rectangles the winner is the component whose first pixel comes LAST in raster order.
# Every expectation below is worked out from that sentence alone.  (mask size 288 x 512; rectangles as (x, y, w, h).)
def _paint(rects, extra=()):
    import numpy as np
    m = np.zeros((288, 512), np.uint8)
    for x, y, w, h in rects:
        m[y:y + h, x:x + w] = 255
    for x, y in extra:
        m[y, x] = 255
    return m


BALL_TIE_CASES = [
    # two 4 x 4 squares, first pixels at (row 5, col 5) and (row 200, col 400): the lower one is discovered last -> wins
    ("two equal squares", _paint([(5, 5, 4, 4), (400, 200, 4, 4)]), (400, 200, 4, 4)),
    # same row of first pixels (row 50): the scan meets col 60 before col 300 -> the right one is discovered last -> wins
    ("same first row", _paint([(60, 50, 4, 4), (300, 50, 4, 4)]), (300, 50, 4, 4)),
    # three equal areas (16): 4x4 at row 50, 4x4 at row 50 further right, 8x2 at row 250: the 8x2 is discovered last
    ("three equal areas, different shapes", _paint([(60, 50, 4, 4), (300, 50, 4, 4), (10, 250, 8, 2)]), (10, 250, 8, 2)),
    # the component discovered last is SMALLER: strict '>' lets an earlier-returned... no — it is returned first but loses
    # to the larger one found later in the list: 9 x 4 = 36 beats 3 x 3 = 9 wherever it sits
    ("larger beats later", _paint([(20, 10, 9, 4), (300, 100, 3, 3)]), (20, 10, 9, 4)),
    # tie on BOUNDING-BOX area, not pixel count: an L of 7 pixels spanning 4 x 4 (area 16) starting at row 20 and a full
    # 4 x 4 square (16 pixels) starting at row 10: equal box areas -> the one discovered last (the L, row 20) wins
    ("bounding box area, not pixel count", _paint([(100, 10, 4, 4), (200, 20, 1, 4), (200, 23, 4, 1)]), (200, 20, 4, 4)),
    # discovery order is decided by the FIRST pixel, not by the rectangle's top-left corner: component P = a column
    # x = 105, rows 10..13 plus a foot at (row 13, col 102..105) -> box (102, 10, 4, 4), first pixel (row 10, col 105);
    # component Q = the square (103, 10, 4, 4) shifted right: box (300, 10, 4, 4), first pixel (row 10, col 300).
    # Both first pixels are on row 10, col 105 < col 300 -> Q is discovered last -> Q wins although P's box starts further left
    ("first pixel decides", _paint([(105, 10, 1, 4), (102, 13, 4, 1), (300, 10, 4, 4)]), (300, 10, 4, 4)),
    # a diagonal link makes ONE component (8-connectivity): squares (10,10,3,3) and (13,13,3,3) touch at a corner -> box
    # (10, 10, 6, 6) = 36 > the lone 5 x 5 = 25 further down
    ("diagonal link merges", _paint([(10, 10, 3, 3), (13, 13, 3, 3), (200, 200, 5, 5)]), (10, 10, 6, 6)),
]
