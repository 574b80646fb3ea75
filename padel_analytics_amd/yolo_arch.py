"""YOLOv8 detect / pose architecture table and checkpoint naming.

The reference never defines the network itself: ``players_tracker.py:303`` and
``players_keypoints_tracker.py:238`` call ``ultralytics.YOLO(model_path)`` and the
graph comes out of the pickled checkpoint.  This module restates the published
YOLOv8 layer table so the engine can (a) build its op list
from a plain ``state_dict`` and (b) manufacture seeded synthetic checkpoints with
the exact Ultralytics key names / shapes (there are no real ``.pt`` files offline).

Nothing in here touches a device.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional

import numpy as np

# (depth, width, max_channels) — SURVEY.md Appendix A "Scales".
SCALES = {
    "n": (0.33, 0.25, 1024),
    "s": (0.33, 0.50, 1024),
    "m": (0.67, 0.75, 768),
    "l": (1.00, 1.00, 512),
    "x": (1.00, 1.25, 512),
}

REG_MAX = 16
BN_EPS = 1e-3          # ultralytics initialize_weights() sets BatchNorm2d.eps = 1e-3
STRIDES = (8, 16, 32)


def make_divisible(x: float, divisor: int = 8) -> int:
    return int(math.ceil(x / divisor) * divisor)


@dataclass(frozen=True)
class ArchDims:
    """Channel widths / repeat counts of one YOLOv8 scale."""
    scale: str
    c1: int   # "64"   stem
    c2: int   # "128"  P2
    c3: int   # "256"  P3
    c4: int   # "512"  P4
    c5: int   # "1024" P5
    n3: int   # repeats of the n=3 C2f blocks
    n6: int   # repeats of the n=6 C2f blocks


def arch_dims(scale: str) -> ArchDims:
    depth, width, max_ch = SCALES[scale]
    c = lambda x: make_divisible(min(x, max_ch) * width, 8)
    n = lambda r: max(round(r * depth), 1)
    return ArchDims(scale, c(64), c(128), c(256), c(512), c(1024), n(3), n(6))


def head_dims(d: ArchDims, nc: int, kpt_shape: Optional[tuple]) -> tuple:
    """(c2 box-branch width, c3 cls-branch width, c4 kpt-branch width or 0, nk)."""
    ch0 = d.c3
    c2 = max(16, ch0 // 4, REG_MAX * 4)
    c3 = max(ch0, min(nc, 100))
    if kpt_shape is None:
        return c2, c3, 0, 0
    nk = int(kpt_shape[0]) * int(kpt_shape[1])
    return c2, c3, max(ch0 // 4, nk), nk


# --------------------------------------------------------------------------------------
# state_dict specification (Ultralytics key names)
# --------------------------------------------------------------------------------------

def _conv_bn(spec, prefix, cin, cout, k):
    spec[f"{prefix}.conv.weight"] = (cout, cin, k, k)
    spec[f"{prefix}.bn.weight"] = (cout,)
    spec[f"{prefix}.bn.bias"] = (cout,)
    spec[f"{prefix}.bn.running_mean"] = (cout,)
    spec[f"{prefix}.bn.running_var"] = (cout,)
    spec[f"{prefix}.bn.num_batches_tracked"] = ()


def _c2f(spec, prefix, cin, cout, n):
    c = cout // 2
    _conv_bn(spec, f"{prefix}.cv1", cin, 2 * c, 1)
    _conv_bn(spec, f"{prefix}.cv2", (2 + n) * c, cout, 1)
    for j in range(n):
        _conv_bn(spec, f"{prefix}.m.{j}.cv1", c, c, 3)
        _conv_bn(spec, f"{prefix}.m.{j}.cv2", c, c, 3)


def yolov8_state_spec(scale: str, nc: int, kpt_shape: Optional[tuple] = None) -> "OrderedDict[str, tuple]":
    """Ordered ``name -> shape`` of every tensor in an Ultralytics YOLOv8 detect/pose state_dict."""
    d = arch_dims(scale)
    s: "OrderedDict[str, tuple]" = OrderedDict()
    _conv_bn(s, "model.0", 3, d.c1, 3)
    _conv_bn(s, "model.1", d.c1, d.c2, 3)
    _c2f(s, "model.2", d.c2, d.c2, d.n3)
    _conv_bn(s, "model.3", d.c2, d.c3, 3)
    _c2f(s, "model.4", d.c3, d.c3, d.n6)
    _conv_bn(s, "model.5", d.c3, d.c4, 3)
    _c2f(s, "model.6", d.c4, d.c4, d.n6)
    _conv_bn(s, "model.7", d.c4, d.c5, 3)
    _c2f(s, "model.8", d.c5, d.c5, d.n3)
    _conv_bn(s, "model.9.cv1", d.c5, d.c5 // 2, 1)
    _conv_bn(s, "model.9.cv2", (d.c5 // 2) * 4, d.c5, 1)
    _c2f(s, "model.12", d.c5 + d.c4, d.c4, d.n3)
    _c2f(s, "model.15", d.c4 + d.c3, d.c3, d.n3)
    _conv_bn(s, "model.16", d.c3, d.c3, 3)
    _c2f(s, "model.18", d.c3 + d.c4, d.c4, d.n3)
    _conv_bn(s, "model.19", d.c4, d.c4, 3)
    _c2f(s, "model.21", d.c4 + d.c5, d.c5, d.n3)
    c2, c3, c4, nk = head_dims(d, nc, kpt_shape)
    chs = (d.c3, d.c4, d.c5)
    for branch, width, nout in (("cv2", c2, 4 * REG_MAX), ("cv3", c3, nc)):
        for l, ch in enumerate(chs):
            _conv_bn(s, f"model.22.{branch}.{l}.0", ch, width, 3)
            _conv_bn(s, f"model.22.{branch}.{l}.1", width, width, 3)
            s[f"model.22.{branch}.{l}.2.weight"] = (nout, width, 1, 1)
            s[f"model.22.{branch}.{l}.2.bias"] = (nout,)
    s["model.22.dfl.conv.weight"] = (1, REG_MAX, 1, 1)
    if kpt_shape is not None:
        for l, ch in enumerate(chs):
            _conv_bn(s, f"model.22.cv4.{l}.0", ch, c4, 3)
            _conv_bn(s, f"model.22.cv4.{l}.1", c4, c4, 3)
            s[f"model.22.cv4.{l}.2.weight"] = (nk, c4, 1, 1)
            s[f"model.22.cv4.{l}.2.bias"] = (nk,)
    return s


def count_parameters(spec) -> int:
    """Trainable-parameter count the way Ultralytics reports it (BN running stats excluded)."""
    total = 0
    for k, shp in spec.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            continue
        total += int(np.prod(shp)) if len(shp) else 1
    return total


def infer_arch_from_state_dict(sd) -> dict:
    """Recover (scale, nc, kpt nk) from tensor shapes of a YOLOv8 state_dict."""
    c1 = int(sd["model.0.conv.weight"].shape[0])
    c5 = int(sd["model.7.conv.weight"].shape[0])
    n3 = 0
    while f"model.2.m.{n3}.cv1.conv.weight" in sd:
        n3 += 1
    scale = None
    for sc in SCALES:
        d = arch_dims(sc)
        if d.c1 == c1 and d.c5 == c5 and d.n3 == n3:
            scale = sc
            break
    if scale is None:
        raise ValueError(f"unrecognised YOLOv8 scale (stem={c1}, P5={c5}, n3={n3})")
    nc = int(sd["model.22.cv3.0.2.weight"].shape[0])
    nk = int(sd["model.22.cv4.0.2.weight"].shape[0]) if "model.22.cv4.0.2.weight" in sd else 0
    return {"scale": scale, "nc": nc, "nk": nk}


# --------------------------------------------------------------------------------------
# conv inventory (for FLOP accounting: bench roofline + known-answer tests)
# --------------------------------------------------------------------------------------

def conv_inventory(scale: str, nc: int, kpt_shape: Optional[tuple], net_h: int, net_w: int):
    """List of (name, cin, cout, k, stride, hout, wout) for every conv of the graph at a
    given network-input size.  2*MAC summed over it reproduces the published GFLOPs
    (SURVEY.md §8(c) known-answer 1)."""
    d = arch_dims(scale)
    out = []

    def conv(name, cin, cout, k, s, h, w):
        ho, wo = (h + s - 1) // s if k == 3 else h // s, (w + s - 1) // s if k == 3 else w // s
        out.append((name, cin, cout, k, s, ho, wo))
        return ho, wo

    def c2f(name, cin, cout, n, h, w):
        c = cout // 2
        conv(f"{name}.cv1", cin, 2 * c, 1, 1, h, w)
        for j in range(n):
            conv(f"{name}.m.{j}.cv1", c, c, 3, 1, h, w)
            conv(f"{name}.m.{j}.cv2", c, c, 3, 1, h, w)
        conv(f"{name}.cv2", (2 + n) * c, cout, 1, 1, h, w)

    h, w = conv("model.0", 3, d.c1, 3, 2, net_h, net_w)
    h, w = conv("model.1", d.c1, d.c2, 3, 2, h, w)
    c2f("model.2", d.c2, d.c2, d.n3, h, w)
    h3, w3 = conv("model.3", d.c2, d.c3, 3, 2, h, w)
    c2f("model.4", d.c3, d.c3, d.n6, h3, w3)
    h4, w4 = conv("model.5", d.c3, d.c4, 3, 2, h3, w3)
    c2f("model.6", d.c4, d.c4, d.n6, h4, w4)
    h5, w5 = conv("model.7", d.c4, d.c5, 3, 2, h4, w4)
    c2f("model.8", d.c5, d.c5, d.n3, h5, w5)
    conv("model.9.cv1", d.c5, d.c5 // 2, 1, 1, h5, w5)
    conv("model.9.cv2", (d.c5 // 2) * 4, d.c5, 1, 1, h5, w5)
    c2f("model.12", d.c5 + d.c4, d.c4, d.n3, h4, w4)
    c2f("model.15", d.c4 + d.c3, d.c3, d.n3, h3, w3)
    conv("model.16", d.c3, d.c3, 3, 2, h3, w3)
    c2f("model.18", d.c3 + d.c4, d.c4, d.n3, h4, w4)
    conv("model.19", d.c4, d.c4, 3, 2, h4, w4)
    c2f("model.21", d.c4 + d.c5, d.c5, d.n3, h5, w5)
    c2, c3, c4, nk = head_dims(d, nc, kpt_shape)
    branches = [("cv2", c2, 4 * REG_MAX), ("cv3", c3, nc)]
    if kpt_shape is not None:
        branches.append(("cv4", c4, nk))
    for l, (ch, hh, ww) in enumerate(((d.c3, h3, w3), (d.c4, h4, w4), (d.c5, h5, w5))):
        for br, width, nout in branches:
            conv(f"model.22.{br}.{l}.0", ch, width, 3, 1, hh, ww)
            conv(f"model.22.{br}.{l}.1", width, width, 3, 1, hh, ww)
            conv(f"model.22.{br}.{l}.2", width, nout, 1, 1, hh, ww)
    return out


def conv_flops(inv) -> float:
    """2 * MACs over a conv inventory."""
    return float(sum(2 * cin * cout * k * k * ho * wo for (_, cin, cout, k, _, ho, wo) in inv))


# --------------------------------------------------------------------------------------
# synthetic checkpoints (SURVEY.md §8(d) recipe)
# --------------------------------------------------------------------------------------

# conv init variance = gain / fan_in.  The running BN statistics are random (not matched to the data),
# so activation scale drifts exponentially with depth; these per-scale gains keep features O(1..10)
# and head logits O(10) through the 60-90 conv layers (measured with the oracle).
SYNTH_GAIN = {"n": 1.8, "s": 1.6, "m": 1.4, "l": 1.3, "x": 1.3}


def synth_state_dict(scale: str, nc: int, kpt_shape: Optional[tuple] = None, seed: int = 0,
                     cls_bias: float = -4.0, gain: Optional[float] = None) -> "OrderedDict[str, np.ndarray]":
    """Seeded random weights with Ultralytics names/shapes.

    conv ~ N(0, gain/fan_in) (SYNTH_GAIN); BN gamma~U(.8,1.6), beta~U(-.3,.3), mean~U(-.2,.2), var~U(.5,1.5);
    every value is rounded through fp16 the way real checkpoints are stored.  ``cls_bias``
    shifts the classification logits so only a small fraction of anchors pass ``conf``
    (bench/tests calibrate it with the oracle).
    """
    rng = np.random.default_rng(seed)
    gain = SYNTH_GAIN[scale] if gain is None else gain
    spec = yolov8_state_spec(scale, nc, kpt_shape)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    r16 = lambda a: a.astype(np.float16).astype(np.float32)
    for name, shp in spec.items():
        if name.endswith("num_batches_tracked"):
            sd[name] = np.array(0, dtype=np.int64)
        elif name.endswith("dfl.conv.weight"):
            sd[name] = np.arange(REG_MAX, dtype=np.float32).reshape(shp)
        elif name.endswith("conv.weight") or (name.endswith(".2.weight")):
            fan_in = shp[1] * shp[2] * shp[3]
            sd[name] = r16(rng.normal(0.0, math.sqrt(gain / fan_in), size=shp).astype(np.float32))
        elif name.endswith("bn.weight"):
            sd[name] = r16(rng.uniform(0.8, 1.6, size=shp).astype(np.float32))
        elif name.endswith("bn.bias"):
            sd[name] = r16(rng.uniform(-0.3, 0.3, size=shp).astype(np.float32))
        elif name.endswith("running_mean"):
            sd[name] = r16(rng.uniform(-0.2, 0.2, size=shp).astype(np.float32))
        elif name.endswith("running_var"):
            sd[name] = r16(rng.uniform(0.5, 1.5, size=shp).astype(np.float32))
        elif name.endswith(".2.bias"):
            if ".cv3." in name:
                sd[name] = r16(np.full(shp, cls_bias, dtype=np.float32)
                               + rng.uniform(-0.5, 0.5, size=shp).astype(np.float32))
            elif ".cv2." in name:
                sd[name] = r16(rng.uniform(0.5, 1.5, size=shp).astype(np.float32))
            else:
                sd[name] = r16(rng.uniform(-0.5, 0.5, size=shp).astype(np.float32))
        else:
            raise AssertionError(name)
    return sd


# --------------------------------------------------------------------------------------
# YOLO11 (the default family of the ultralytics 8.3 line the reference's requirements.txt resolves to): same Conv / SPPF /
# Detect-Pose decode as YOLOv8, with C3k2 instead of C2f, a C2PSA attention block behind SPPF, the shortcut on in EVERY C3k2 and
# a depthwise class branch in the head.  Ultralytics is not installable here: this restates the published yolo11.yaml and
# modules and is pinned by the published parameter / GFLOPs table (tests/test_yolo11_host.py), not by upstream itself.
# --------------------------------------------------------------------------------------

SCALES11 = {
    "n": (0.50, 0.25, 1024),
    "s": (0.50, 0.50, 1024),
    "m": (0.50, 1.00, 512),
    "l": (1.00, 1.00, 512),
    "x": (1.00, 1.50, 512),
}
PSA_KEY_DIM = 32       # Attention(dim, num_heads = dim // 64, attn_ratio = 0.5): head_dim 64, key_dim 32
PSA_HEAD_DIM = 64
HEAD_LAYER = {"yolov8": 22, "yolo11": 23}


@dataclass(frozen=True)
class Arch11Dims:
    """Channel widths / repeat count of one YOLO11 scale."""
    scale: str
    c1: int    # "64"   stem
    c2: int    # "128"  P2 conv
    c3: int    # "256"  layers 2, 3, 16, 17 (P3)
    c4: int    # "512"  layers 4, 5, 6, 13, 19, 20 (P4)
    c5: int    # "1024" layers 7 .. 10, 22 (P5)
    n: int     # repeats of every C3k2 / PSABlocks of C2PSA ("2" in the yaml)
    big: bool  # m, l, x: c3k = True in every C3k2


def arch11_dims(scale: str) -> Arch11Dims:
    depth, width, max_ch = SCALES11[scale]
    c = lambda x: make_divisible(min(x, max_ch) * width, 8)
    return Arch11Dims(scale, c(64), c(128), c(256), c(512), c(1024), max(round(2 * depth), 1), scale in "mlx")


def c3k2_layers(d: Arch11Dims):
    """(layer index, cin, cout, c3k, e) of the eight C3k2 blocks."""
    return [(2, d.c2, d.c3, d.big, 0.25), (4, d.c3, d.c4, d.big, 0.25), (6, d.c4, d.c4, True, 0.5), (8, d.c5, d.c5, True, 0.5),
            (13, d.c5 + d.c4, d.c4, d.big, 0.5), (16, d.c4 + d.c4, d.c3, d.big, 0.5), (19, d.c3 + d.c4, d.c4, d.big, 0.5),
            (22, d.c4 + d.c5, d.c5, True, 0.5)]


def _dwconv_bn(spec, prefix, c, k):
    _conv_bn(spec, prefix, 1, c, k)          # groups = c: weight (c, 1, k, k)


def _c3k2(spec, prefix, cin, cout, n, c3k, e):
    c = int(cout * e)
    _conv_bn(spec, f"{prefix}.cv1", cin, 2 * c, 1)
    _conv_bn(spec, f"{prefix}.cv2", (2 + n) * c, cout, 1)
    for j in range(n):
        p = f"{prefix}.m.{j}"
        if c3k:                               # C3k(c, c, n = 2): hidden c / 2, two 3x3 / 3x3 bottlenecks at e = 1.0
            h = int(c * 0.5)
            _conv_bn(spec, f"{p}.cv1", c, h, 1)
            _conv_bn(spec, f"{p}.cv2", c, h, 1)
            _conv_bn(spec, f"{p}.cv3", 2 * h, c, 1)
            for k in range(2):
                _conv_bn(spec, f"{p}.m.{k}.cv1", h, h, 3)
                _conv_bn(spec, f"{p}.m.{k}.cv2", h, h, 3)
        else:                                 # Bottleneck(c, c, e = 0.5)
            h = int(c * 0.5)
            _conv_bn(spec, f"{p}.cv1", c, h, 3)
            _conv_bn(spec, f"{p}.cv2", h, c, 3)


def _c2psa(spec, prefix, c1, n):
    c = c1 // 2
    heads = c // PSA_HEAD_DIM
    _conv_bn(spec, f"{prefix}.cv1", c1, 2 * c, 1)
    _conv_bn(spec, f"{prefix}.cv2", 2 * c, c1, 1)
    for j in range(n):
        p = f"{prefix}.m.{j}"
        _conv_bn(spec, f"{p}.attn.qkv", c, c + 2 * PSA_KEY_DIM * heads, 1)
        _conv_bn(spec, f"{p}.attn.proj", c, c, 1)
        _dwconv_bn(spec, f"{p}.attn.pe", c, 3)
        _conv_bn(spec, f"{p}.ffn.0", c, 2 * c, 1)
        _conv_bn(spec, f"{p}.ffn.1", 2 * c, c, 1)


def yolo11_state_spec(scale: str, nc: int, kpt_shape: Optional[tuple] = None) -> "OrderedDict[str, tuple]":
    """Ordered ``name -> shape`` of every tensor in an Ultralytics YOLO11 detect / pose state_dict."""
    d = arch11_dims(scale)
    s: "OrderedDict[str, tuple]" = OrderedDict()
    blocks = {i: (cin, cout, c3k, e) for i, cin, cout, c3k, e in c3k2_layers(d)}
    _conv_bn(s, "model.0", 3, d.c1, 3)
    _conv_bn(s, "model.1", d.c1, d.c2, 3)
    _c3k2(s, "model.2", *blocks[2][:2], d.n, *blocks[2][2:])
    _conv_bn(s, "model.3", d.c3, d.c3, 3)
    _c3k2(s, "model.4", *blocks[4][:2], d.n, *blocks[4][2:])
    _conv_bn(s, "model.5", d.c4, d.c4, 3)
    _c3k2(s, "model.6", *blocks[6][:2], d.n, *blocks[6][2:])
    _conv_bn(s, "model.7", d.c4, d.c5, 3)
    _c3k2(s, "model.8", *blocks[8][:2], d.n, *blocks[8][2:])
    _conv_bn(s, "model.9.cv1", d.c5, d.c5 // 2, 1)
    _conv_bn(s, "model.9.cv2", (d.c5 // 2) * 4, d.c5, 1)
    _c2psa(s, "model.10", d.c5, d.n)
    _c3k2(s, "model.13", *blocks[13][:2], d.n, *blocks[13][2:])
    _c3k2(s, "model.16", *blocks[16][:2], d.n, *blocks[16][2:])
    _conv_bn(s, "model.17", d.c3, d.c3, 3)
    _c3k2(s, "model.19", *blocks[19][:2], d.n, *blocks[19][2:])
    _conv_bn(s, "model.20", d.c4, d.c4, 3)
    _c3k2(s, "model.22", *blocks[22][:2], d.n, *blocks[22][2:])
    c2, c3, c4, nk = head_dims(d, nc, kpt_shape)           # (the same widths as YOLOv8's head: ch0 = P3 channels)
    chs = (d.c3, d.c4, d.c5)
    for l, ch in enumerate(chs):
        _conv_bn(s, f"model.23.cv2.{l}.0", ch, c2, 3)
        _conv_bn(s, f"model.23.cv2.{l}.1", c2, c2, 3)
        s[f"model.23.cv2.{l}.2.weight"] = (4 * REG_MAX, c2, 1, 1)
        s[f"model.23.cv2.{l}.2.bias"] = (4 * REG_MAX,)
    for l, ch in enumerate(chs):
        _dwconv_bn(s, f"model.23.cv3.{l}.0.0", ch, 3)
        _conv_bn(s, f"model.23.cv3.{l}.0.1", ch, c3, 1)
        _dwconv_bn(s, f"model.23.cv3.{l}.1.0", c3, 3)
        _conv_bn(s, f"model.23.cv3.{l}.1.1", c3, c3, 1)
        s[f"model.23.cv3.{l}.2.weight"] = (nc, c3, 1, 1)
        s[f"model.23.cv3.{l}.2.bias"] = (nc,)
    s["model.23.dfl.conv.weight"] = (1, REG_MAX, 1, 1)
    if kpt_shape is not None:
        for l, ch in enumerate(chs):
            _conv_bn(s, f"model.23.cv4.{l}.0", ch, c4, 3)
            _conv_bn(s, f"model.23.cv4.{l}.1", c4, c4, 3)
            s[f"model.23.cv4.{l}.2.weight"] = (nk, c4, 1, 1)
            s[f"model.23.cv4.{l}.2.bias"] = (nk,)
    return s


def infer_family(sd) -> str:
    """"yolo11" if the state_dict has the C2PSA attention block at model.10, else "yolov8"."""
    return "yolo11" if "model.10.m.0.attn.qkv.conv.weight" in sd else "yolov8"


def infer_arch11_from_state_dict(sd) -> dict:
    """Recover (scale, nc, kpt nk) from tensor shapes of a YOLO11 state_dict."""
    c1 = int(sd["model.0.conv.weight"].shape[0])
    c5 = int(sd["model.7.conv.weight"].shape[0])
    n = 0
    while f"model.2.m.{n}.cv1.conv.weight" in sd:
        n += 1
    big = "model.2.m.0.cv3.conv.weight" in sd
    scale = None
    for sc in SCALES11:
        d = arch11_dims(sc)
        if (d.c1, d.c5, d.n, d.big) == (c1, c5, n, big):
            scale = sc
            break
    if scale is None:
        raise ValueError(f"unrecognised YOLO11 scale (stem={c1}, P5={c5}, n={n}, c3k={big})")
    if "model.23.cv3.0.2.weight" not in sd:
        raise ValueError("YOLO11 state_dict without a Detect / Pose head at model.23 (seg / cls / obb heads are not supported)")
    nc = int(sd["model.23.cv3.0.2.weight"].shape[0])
    nk = int(sd["model.23.cv4.0.2.weight"].shape[0]) if "model.23.cv4.0.2.weight" in sd else 0
    return {"scale": scale, "nc": nc, "nk": nk}


def infer_model(sd) -> dict:
    """{"family", "scale", "nc", "nk"} of a YOLOv8 or YOLO11 state_dict: the family first (the scales of the two families share
    stem and P5 widths), then the scale inside it."""
    fam = infer_family(sd)
    info = infer_arch11_from_state_dict(sd) if fam == "yolo11" else infer_arch_from_state_dict(sd)
    return dict(info, family=fam)


def conv_inventory11(scale: str, nc: int, kpt_shape: Optional[tuple], net_h: int, net_w: int):
    """(name, cin, cout, k, stride, hout, wout, groups) of every convolution of a YOLO11 graph, DFL projection included:
    2 * MAC summed over it reproduces the published GFLOPs."""
    d = arch11_dims(scale)
    out = []

    def conv(name, cin, cout, k, s, h, w, groups=1):
        ho, wo = ((h + s - 1) // s, (w + s - 1) // s) if k == 3 else (h // s, w // s)
        out.append((name, cin, cout, k, s, ho, wo, groups))
        return ho, wo

    def c3k2(i, cin, cout, c3k, e, h, w):
        c = int(cout * e)
        p = f"model.{i}"
        conv(f"{p}.cv1", cin, 2 * c, 1, 1, h, w)
        for j in range(d.n):
            hd = int(c * 0.5)
            if c3k:
                conv(f"{p}.m.{j}.cv1", c, hd, 1, 1, h, w)
                conv(f"{p}.m.{j}.cv2", c, hd, 1, 1, h, w)
                for k in range(2):
                    conv(f"{p}.m.{j}.m.{k}.cv1", hd, hd, 3, 1, h, w)
                    conv(f"{p}.m.{j}.m.{k}.cv2", hd, hd, 3, 1, h, w)
                conv(f"{p}.m.{j}.cv3", 2 * hd, c, 1, 1, h, w)
            else:
                conv(f"{p}.m.{j}.cv1", c, hd, 3, 1, h, w)
                conv(f"{p}.m.{j}.cv2", hd, c, 3, 1, h, w)
        conv(f"{p}.cv2", (2 + d.n) * c, cout, 1, 1, h, w)

    blocks = {i: (cin, cout, c3k, e) for i, cin, cout, c3k, e in c3k2_layers(d)}
    h, w = conv("model.0", 3, d.c1, 3, 2, net_h, net_w)
    h, w = conv("model.1", d.c1, d.c2, 3, 2, h, w)
    c3k2(2, *blocks[2], h, w)
    h3, w3 = conv("model.3", d.c3, d.c3, 3, 2, h, w)
    c3k2(4, *blocks[4], h3, w3)
    h4, w4 = conv("model.5", d.c4, d.c4, 3, 2, h3, w3)
    c3k2(6, *blocks[6], h4, w4)
    h5, w5 = conv("model.7", d.c4, d.c5, 3, 2, h4, w4)
    c3k2(8, *blocks[8], h5, w5)
    conv("model.9.cv1", d.c5, d.c5 // 2, 1, 1, h5, w5)
    conv("model.9.cv2", (d.c5 // 2) * 4, d.c5, 1, 1, h5, w5)
    c = d.c5 // 2
    heads = c // PSA_HEAD_DIM
    conv("model.10.cv1", d.c5, 2 * c, 1, 1, h5, w5)
    for j in range(d.n):
        p = f"model.10.m.{j}"
        conv(f"{p}.attn.qkv", c, c + 2 * PSA_KEY_DIM * heads, 1, 1, h5, w5)
        conv(f"{p}.attn.pe", c, c, 3, 1, h5, w5, groups=c)
        conv(f"{p}.attn.proj", c, c, 1, 1, h5, w5)
        conv(f"{p}.ffn.0", c, 2 * c, 1, 1, h5, w5)
        conv(f"{p}.ffn.1", 2 * c, c, 1, 1, h5, w5)
    conv("model.10.cv2", 2 * c, d.c5, 1, 1, h5, w5)
    c3k2(13, *blocks[13], h4, w4)
    c3k2(16, *blocks[16], h3, w3)
    conv("model.17", d.c3, d.c3, 3, 2, h3, w3)
    c3k2(19, *blocks[19], h4, w4)
    conv("model.20", d.c4, d.c4, 3, 2, h4, w4)
    c3k2(22, *blocks[22], h5, w5)
    c2, c3, c4, nk = head_dims(d, nc, kpt_shape)
    for l, (ch, hh, ww) in enumerate(((d.c3, h3, w3), (d.c4, h4, w4), (d.c5, h5, w5))):
        conv(f"model.23.cv2.{l}.0", ch, c2, 3, 1, hh, ww)
        conv(f"model.23.cv2.{l}.1", c2, c2, 3, 1, hh, ww)
        conv(f"model.23.cv2.{l}.2", c2, 4 * REG_MAX, 1, 1, hh, ww)
        conv(f"model.23.cv3.{l}.0.0", ch, ch, 3, 1, hh, ww, groups=ch)
        conv(f"model.23.cv3.{l}.0.1", ch, c3, 1, 1, hh, ww)
        conv(f"model.23.cv3.{l}.1.0", c3, c3, 3, 1, hh, ww, groups=c3)
        conv(f"model.23.cv3.{l}.1.1", c3, c3, 1, 1, hh, ww)
        conv(f"model.23.cv3.{l}.2", c3, nc, 1, 1, hh, ww)
        if kpt_shape is not None:
            conv(f"model.23.cv4.{l}.0", ch, c4, 3, 1, hh, ww)
            conv(f"model.23.cv4.{l}.1", c4, c4, 3, 1, hh, ww)
            conv(f"model.23.cv4.{l}.2", c4, nk, 1, 1, hh, ww)
    anchors = h3 * w3 + h4 * w4 + h5 * w5
    out.append(("model.23.dfl", REG_MAX, 1, 1, 1, 4, anchors, 1))          # Conv2d(16, 1, 1) over the (16, 4, anchors) view
    return out


def conv_flops11(inv) -> float:
    """2 * MACs over a ``conv_inventory11`` list (grouped convolutions count cin / groups inputs per output)."""
    return float(sum(2 * (cin // g) * cout * k * k * ho * wo for (_, cin, cout, k, _, ho, wo, g) in inv))


def synth_state_dict11(scale: str, nc: int, kpt_shape: Optional[tuple] = None, seed: int = 0, cls_bias: float = -4.0,
                       gain: Optional[float] = None) -> "OrderedDict[str, np.ndarray]":
    """``synth_state_dict``'s recipe over the YOLO11 specification (fan-in of a depthwise conv: its 9 taps)."""
    rng = np.random.default_rng(seed)
    gain = SYNTH_GAIN[scale] if gain is None else gain
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    r16 = lambda a: a.astype(np.float16).astype(np.float32)
    for name, shp in yolo11_state_spec(scale, nc, kpt_shape).items():
        if name.endswith("num_batches_tracked"):
            sd[name] = np.array(0, dtype=np.int64)
        elif name.endswith("dfl.conv.weight"):
            sd[name] = np.arange(REG_MAX, dtype=np.float32).reshape(shp)
        elif name.endswith("conv.weight") or name.endswith(".2.weight"):
            fan_in = shp[1] * shp[2] * shp[3]
            sd[name] = r16(rng.normal(0.0, math.sqrt(gain / fan_in), size=shp).astype(np.float32))
        elif name.endswith("bn.weight"):
            sd[name] = r16(rng.uniform(0.8, 1.6, size=shp).astype(np.float32))
        elif name.endswith("bn.bias"):
            sd[name] = r16(rng.uniform(-0.3, 0.3, size=shp).astype(np.float32))
        elif name.endswith("running_mean"):
            sd[name] = r16(rng.uniform(-0.2, 0.2, size=shp).astype(np.float32))
        elif name.endswith("running_var"):
            sd[name] = r16(rng.uniform(0.5, 1.5, size=shp).astype(np.float32))
        elif name.endswith(".2.bias"):
            if ".cv3." in name:
                sd[name] = r16(np.full(shp, cls_bias, dtype=np.float32) + rng.uniform(-0.5, 0.5, size=shp).astype(np.float32))
            elif ".cv2." in name:
                sd[name] = r16(rng.uniform(0.5, 1.5, size=shp).astype(np.float32))
            else:
                sd[name] = r16(rng.uniform(-0.5, 0.5, size=shp).astype(np.float32))
        else:
            raise AssertionError(name)
    return sd
