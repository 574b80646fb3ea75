"""GPU tests of what runs BETWEEN the convolutions, stated directly and at the edges (csrc/kernels_misc.hip, csrc/act_fast.h).

A. The helper kernels per storage type (fp32, fp16, h2 pairs), exact.  Every case is a ``TASK_TRACKNET`` op list run through
   ``Model.tracknet_infer``: the caller's array lands in buffer 0 (h2: encoded on the device) and the head buffer comes back raw.
   * SPPF (``pool5_kernel<f32x4|f16x8>``, ``pool5_h2_kernel``, ``sppf_h2_kernel<256|512|1024>``, ``sppf_f16_kernel<256|1024>``) runs in
     place on buffer 0, which is also the head: the test supplies the source slice AND the sentinel content of every other channel in
     one array.  Map sizes from 1 x 1 to the LDS limits of the fused kernels (48 x 50 / 60 x 80) and one pixel row beyond them
     (49 x 49 / 69 x 70: three launches), channel offsets, batches for which the workgroup-id mapping of ``sppf_h2_kernel`` has idle
     slots; every ``fuse_sppf`` value, the fused results bitwise those of the three launches.
   * MaxPool2d(2, 2) and Upsample(2) between slices of buffers with different pixel strides; the untouched channels of the output
     buffers hold a sentinel written by a zero-weight 1 x 1 conv (``tests/test_gpu_conv.py::slice_sentinel``).
   * Contents: strictly negative maps (a zero-padding pool would show), heavy ties with both zeros, ramps whose answer has a
     closed form (asserted literally: the message names level and pixel), magnitudes from 1e-7 to 6e4.
   Reference: ``max_pool2d`` / ``interpolate(mode="nearest")`` in fp64 on the values the input buffer holds.  ``np.array_equal``, no
   tolerance; channels outside the written slice are compared as bit patterns.
   * ``h2_encode_kernel`` against its Python twin ``graph.h2_split`` bit for bit on fp16 subnormals, round-to-even halfway cases,
     the values next to +-65504, and the overflow flag around them.
   * fp16 graphs: ``pa_model_create`` refuses a pool / upsample on a buffer whose width is not a multiple of 8 halves (the 16-byte
     accesses of the fp16 helper kernels would be misaligned on every second pixel).
B. The activation epilogues over their whole argument range: an identity 1 x 1 conv with each activation on each arithmetic path
   (h2 three- and two-product, fp16, bf16x3, strict fp32), ~2.2 M arguments in [-80, 80] plus tails up to +-6e4, against the
   function in fp64, in ulps of the fp32 result.  The bound is not a constant of this file: it is the error of the plain fp32
   formula in numpy on the same arguments (max x 2 for the two hardware approximations v_exp_f32 / v_rcp_f32, mean x 1.5).  The
   figures are printed and, where the environment names a directory in ``PADEL_REPORT_DIR``, appended to ``act_ulp_sweep.txt`` there
   (profiles/act_ulp_sweep.txt is a copy of one such run).

The stem kernels (``stem_mfma_kernel``, ``stem_l1_h2``) have their own file, tests/test_gpu_stem.py: their output is read back
through a level-3 head that changes nothing (one-hot unshuffle convs, tests/stem_probe.py), at every width from 16 to 80."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import engine as E, graph as G
from tests.test_gpu_conv import slice_sentinel

pytestmark = pytest.mark.gpu

VEC = {"f32": 4, "f16": 8, "h2": 16}                       # channel granularity of a helper op's slices (graph_plan.cpp: validate_desc)
DTYPE = {"f32": G.DTYPE_F32, "f16": G.DTYPE_F16, "h2": G.DTYPE_H2}
CONTENTS = ("negative", "ties", "ramp", "wide")


# ---- storage types: what a buffer holds for a given fp32 array, as bits and as values ---------------------------------------
def to_input(t, x):
    """The array handed to tracknet_infer (fp16 graphs take halves; h2 graphs take fp32 and encode on the device)."""
    return x.astype(np.float16) if t == "f16" else x.astype(np.float32)


def stored_bits(t, x):
    """Raw content of a buffer that holds ``x`` (..., C): uint32 (fp32; h2: the group layout) or uint16 (fp16)."""
    if t == "f16":
        return x.astype(np.float16).view(np.uint16)
    if t == "h2":
        return G.h2_encode_nhwc(x.astype(np.float32)).view(np.uint32)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def stored_values(t, x):
    """The numbers those bits stand for, fp64."""
    if t == "f16":
        return x.astype(np.float16).astype(np.float64)
    if t == "h2":
        return G.h2_value(*G.h2_split(x.astype(np.float32))).astype(np.float64)
    return x.astype(np.float32).astype(np.float64)


def raw_bits(t, out):
    """The head buffer as returned by tracknet_infer (fp32-sized) -> the bits of its storage type.  fp16: the buffer is sized for
    fp32, the halves are the first half of the returned bytes."""
    if t == "f16":
        return out.reshape(-1).view(np.uint16)[:out.size].reshape(out.shape)
    return out.view(np.uint32)


def values_of(t, bits):
    if t == "f16":
        return bits.view(np.float16).astype(np.float64)
    if t == "h2":
        return G.h2_decode_nhwc(bits.view(np.float32)).astype(np.float64)
    return bits.view(np.float32).astype(np.float64)


# ---- contents ---------------------------------------------------------------------------------------------------------------
def ramp_bases(t, H, W):
    """Three maps that do not decrease in y nor in x, exact in storage type ``t``: y W + x (fp16 above 2048: y + x), y, x."""
    yy, xx = np.mgrid[0:H, 0:W]
    full = yy * W + xx if (t != "f16" or H * W <= 2048) else yy + xx
    return [full.astype(np.float64), yy.astype(np.float64), xx.astype(np.float64)]


def make_content(kind, t, rng, B, H, W, c):
    shape = (B, H, W, c)
    if kind == "negative":
        return rng.uniform(-9.0, -1.0, shape).astype(np.float32)
    if kind == "ties":        # five distinct numbers, the zero with both signs; zeros are the maximum of many windows
        return rng.choice(np.array([-2.5, -1.0, -0.0, 0.0, 0.75, 1.5], np.float32), shape, p=[0.3, 0.3, 0.15, 0.15, 0.05, 0.05])
    if kind == "ramp":        # channel j: base j % 3, negated for j % 6 >= 3
        bases = ramp_bases(t, H, W)
        x = np.stack([bases[j % 3] * (1.0 if j % 6 < 3 else -1.0) for j in range(c)], -1)
        return np.broadcast_to(x, shape).astype(np.float32)
    mag = np.exp(rng.uniform(np.log(1e-7), np.log(6e4), shape))
    x = (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 8:        # the ends of the fp16 range and of its subnormals
        flat[rng.choice(flat.size, 8, replace=False)] = [65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, -2.0 ** -14, 1e-7, -1e-7]
    return x


def first_diff(got, want):
    idx = np.argwhere(got != want)
    return "" if idx.size == 0 else f"{len(idx)} differ, first at (n, y, x, channel) = {tuple(int(i) for i in idx[0])}: got {got[tuple(idx[0])]!r}, want {want[tuple(idx[0])]!r}"


# ---- A.1 SPPF ---------------------------------------------------------------------------------------------------------------
# (type, H, W, c, off, B).  h2: B x ceil(c / 16) = 1, 3, 15, 18 among others; maps above 1024 pixels take the 1024-thread
# instantiations; 48 x 50 / 60 x 80 are the largest maps the fused h2 / fp16 kernels accept, 49 x 49 / 69 x 70 fall through
SPPF_CASES = [
    ("h2", 1, 1, 16, 0, 1), ("h2", 1, 7, 48, 16, 1), ("h2", 7, 1, 16, 48, 3), ("h2", 2, 3, 48, 0, 5), ("h2", 4, 4, 32, 16, 9),
    ("h2", 5, 9, 48, 48, 6), ("h2", 13, 13, 32, 0, 2), ("h2", 12, 20, 16, 16, 15), ("h2", 33, 31, 48, 0, 1), ("h2", 23, 40, 32, 48, 1),
    ("h2", 48, 50, 48, 16, 1), ("h2", 49, 49, 32, 0, 1),
    ("f32", 1, 1, 4, 0, 1), ("f32", 1, 7, 20, 4, 3), ("f32", 7, 1, 4, 36, 2), ("f32", 2, 3, 64, 0, 1), ("f32", 4, 4, 20, 36, 3),
    ("f32", 5, 9, 4, 4, 15), ("f32", 13, 13, 64, 4, 1), ("f32", 12, 20, 20, 0, 2), ("f32", 33, 31, 4, 36, 1), ("f32", 23, 40, 20, 4, 1),
    ("f32", 49, 49, 4, 0, 1),
    ("f16", 1, 1, 8, 0, 1), ("f16", 1, 7, 24, 8, 3), ("f16", 7, 1, 8, 40, 5), ("f16", 2, 3, 64, 0, 1), ("f16", 4, 4, 24, 40, 6),
    ("f16", 5, 9, 8, 8, 18), ("f16", 13, 13, 24, 0, 2), ("f16", 12, 20, 64, 8, 1), ("f16", 33, 31, 8, 40, 1), ("f16", 23, 40, 24, 8, 1),
    ("f16", 48, 50, 8, 0, 1), ("f16", 60, 80, 8, 8, 1), ("f16", 69, 70, 8, 0, 1),
]
FUSE_MODES = {"h2": (0, 1, 2, 3, 4), "f32": (0, 1), "f16": (0, 1)}


def sppf_reference(src):
    """(B, H, W, c) fp64 -> (B, H, W, 3 c): three chained MaxPool2d(5, 1, 2)."""
    t = torch.from_numpy(src).permute(0, 3, 1, 2)
    ys = []
    for _ in range(3):
        t = F.max_pool2d(t, 5, 1, 2)
        ys.append(t)
    return torch.cat(ys, 1).permute(0, 2, 3, 1).numpy()


def check_ramp_sppf(t, got, H, W, c, name):
    """Level k of a map v that does not decrease in y, x is v(min(y + 2k, H - 1), min(x + 2k, W - 1)); of -v it is
    -v(max(y - 2k, 0), max(x - 2k, 0)).  ``got``: (B, H, W, 3 c) values."""
    bases = ramp_bases(t, H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in (1, 2, 3):
        up = [b[np.minimum(yy + 2 * k, H - 1), np.minimum(xx + 2 * k, W - 1)] for b in bases]
        dn = [-b[np.maximum(yy - 2 * k, 0), np.maximum(xx - 2 * k, 0)] for b in bases]
        want = np.stack([(up if j % 6 < 3 else dn)[j % 3] for j in range(c)], -1)
        lev = got[..., (k - 1) * c:k * c]
        assert np.array_equal(lev, np.broadcast_to(want, lev.shape)), f"{name}: ramp, level {k}: {first_diff(lev, np.broadcast_to(want, lev.shape))}"


@pytest.mark.parametrize("case", SPPF_CASES, ids=["{}-{}x{}-c{}@{}-B{}".format(*c) for c in SPPF_CASES])
def test_sppf(gpu_engine, case):
    t, H, W, c, off, B = case
    width = off + 4 * c + VEC[t]                                   # wider than the concat: channels right of it must survive
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPE[t])
    b0 = g.buf(0, width)
    g.sppf_pool(b0, c, off)
    g.head_buf = (b0, -1, -1)
    m = E.Model(gpu_engine, g)
    m.set_max_batch(B)
    rng = np.random.default_rng(H * 1009 + W * 31 + c + off + B)
    lo, hi = off + c, off + 4 * c
    try:
        for kind in CONTENTS:
            x = np.broadcast_to(slice_sentinel(width), (B, H, W, width)).copy()
            x[..., off:off + c] = make_content(kind, t, rng, B, H, W, c)
            want = sppf_reference(stored_values(t, x[..., off:off + c]))
            keep = stored_bits(t, x)
            outs = {}
            for mode in FUSE_MODES[t]:
                gpu_engine.set_tuning(fuse_sppf=mode)
                outs[mode] = raw_bits(t, m.tracknet_infer(to_input(t, x))).copy()
                if t == "h2":
                    assert not m.take_overflow()
            for mode, bits in outs.items():
                name = f"{case} {kind} fuse_sppf={mode}"
                got = values_of(t, bits)[..., lo:hi]
                if kind == "ramp":
                    check_ramp_sppf(t, got, H, W, c, name)
                assert np.array_equal(got, want), f"{name}: {first_diff(got, want)}"
                # every channel outside [off + c, off + 4c) still holds the bits that were put there (h2: whole 16-channel groups)
                assert np.array_equal(bits[..., :lo], keep[..., :lo]), f"{name}: channels left of the written slice changed"
                assert np.array_equal(bits[..., hi:], keep[..., hi:]), f"{name}: channels right of the written slice changed"
                assert np.array_equal(bits, outs[0]), f"{name}: differs bitwise from the three launches"
    finally:
        gpu_engine.set_tuning(fuse_sppf=1)
        m.close()


# ---- A.2 MaxPool2d(2, 2) and Upsample(2) ------------------------------------------------------------------------------------
W_IN, W_SMALL, W_BIG = 112, 128, 160                     # three pixel strides (multiples of 32: fp16 convs read whole k-steps)
# (type, H, W, c, offset in the input buffer, in the pooled buffer, in the upsampled buffer, B)
POOL_CASES = [
    ("h2", 2, 2, 16, 0, 16, 48, 1), ("h2", 2, 6, 32, 16, 48, 0, 3), ("h2", 6, 2, 48, 48, 0, 16, 1), ("h2", 10, 14, 32, 0, 16, 48, 3),
    ("h2", 24, 40, 48, 16, 48, 0, 1),
    ("f32", 2, 2, 4, 0, 4, 36, 1), ("f32", 2, 6, 20, 4, 36, 0, 3), ("f32", 6, 2, 64, 36, 0, 4, 1), ("f32", 10, 14, 20, 0, 36, 4, 3),
    ("f32", 24, 40, 64, 4, 0, 36, 1),
    ("f16", 2, 2, 8, 0, 8, 40, 1), ("f16", 2, 6, 24, 8, 40, 0, 3), ("f16", 6, 2, 64, 40, 0, 8, 1), ("f16", 10, 14, 24, 0, 40, 8, 3),
    ("f16", 24, 40, 64, 8, 0, 40, 1),
]


def pool_graph(t, c, in_off, off1, off0, upsample):
    """buffer 0 [in_off : in_off + c) -MaxPool2d(2, 2)-> S1 [off1 : off1 + c) (-Upsample(2)-> S0 [off0 : off0 + c)); S1 and S0 are
    filled with a sentinel first (zero-weight 1 x 1 conv, bias = sentinel).  The last buffer comes back: raw as the head of fp32 and
    h2 graphs (h2: the conv writes fp32 into a head buffer, the helper writes pairs into its slice — both are compared as bits);
    fp16 graphs through an identity 1 x 1 (their head is an fp32 buffer).  Nothing reads the upsampled slice but a pool-free
    read-back, so the upsample is never absorbed into a conv."""
    z = lambda *shape: np.zeros(shape, np.float32)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPE[t])
    b0 = g.buf(0, W_IN)
    s1 = g.buf(1, W_SMALL)
    g.conv((b0, 0, 32), (s1, 0), z(W_SMALL, 32, 1, 1), slice_sentinel(W_SMALL), 1, 2, G.ACT_NONE)
    g.maxpool2((b0, in_off, c), (s1, off1))
    last, lvl, width = s1, 1, W_SMALL
    if upsample:
        s0 = g.buf(0, W_BIG)
        g.conv((b0, 0, 32), (s0, 0), z(W_BIG, 32, 1, 1), slice_sentinel(W_BIG), 1, 1, G.ACT_NONE)
        g.upsample2x((s1, off1, c), (s0, off0))
        last, lvl, width = s0, 0, W_BIG
    if t == "f16":
        hd = g.buf(lvl, width)
        g.conv((last, 0, width), (hd, 0), np.eye(width, dtype=np.float32)[:, :, None, None], z(width), 1, 1, G.ACT_NONE)
        last = hd
    g.head_buf = (last, -1, -1)
    return g


@pytest.mark.parametrize("case", POOL_CASES, ids=["{}-{}x{}-c{}-at{}-{}-{}-B{}".format(*c) for c in POOL_CASES])
def test_maxpool2_and_upsample(gpu_engine, case):
    t, H, W, c, in_off, off1, off0, B = case
    rng = np.random.default_rng(H * 1009 + W * 31 + c + in_off + B)
    yy, xx = np.mgrid[0:H // 2, 0:W // 2]
    for upsample, off, width in ((False, off1, W_SMALL), (True, off0, W_BIG)):
        m = E.Model(gpu_engine, pool_graph(t, c, in_off, off1, off0, upsample))
        m.set_max_batch(B)
        try:
            for kind in CONTENTS:
                x = np.full((B, H, W, W_IN), 3.0e4, np.float32)      # the neighbours of the input slice: a pool that strays into them shows
                x[..., in_off:in_off + c] = make_content(kind, t, rng, B, H, W, c)
                src = torch.from_numpy(stored_values(t, x[..., in_off:in_off + c])).permute(0, 3, 1, 2)
                ref = F.max_pool2d(src, 2, 2)
                if upsample:
                    ref = F.interpolate(ref, scale_factor=2.0, mode="nearest")
                want = ref.permute(0, 2, 3, 1).numpy()
                out = m.tracknet_infer(to_input(t, x))
                if t == "h2":
                    assert not m.take_overflow()
                name = f"{case} {kind} {'maxpool + upsample' if upsample else 'maxpool'}"
                assert out.shape[-1] == width
                # fp16: the identity conv delivered fp32 values of the halves; fp32 / h2: raw bits of the head buffer
                got = out[..., off:off + c].astype(np.float64) if t != "h2" else G.h2_decode_nhwc(out)[..., off:off + c].astype(np.float64)
                if kind == "ramp":       # MaxPool2d(2, 2) of v: v(2y + 1, 2x + 1), of -v: -v(2y, 2x); the upsample repeats it
                    bases = ramp_bases(t, H, W)
                    hi_, lo_ = [b[2 * yy + 1, 2 * xx + 1] for b in bases], [-b[2 * yy, 2 * xx] for b in bases]
                    lit = np.stack([(hi_ if j % 6 < 3 else lo_)[j % 3] for j in range(c)], -1)
                    if upsample:
                        lit = lit.repeat(2, 0).repeat(2, 1)
                    assert np.array_equal(got, np.broadcast_to(lit, got.shape)), f"{name}: ramp: {first_diff(got, np.broadcast_to(lit, got.shape))}"
                assert np.array_equal(got, want), f"{name}: {first_diff(got, want)}"
                sent = np.broadcast_to(slice_sentinel(width), out.shape)
                for side, sl in (("left", slice(0, off)), ("right", slice(off + c, width))):
                    assert np.array_equal(out[..., sl].view(np.uint32), np.ascontiguousarray(sent[..., sl]).view(np.uint32)), \
                        f"{name}: channels {side} of the written slice lost the sentinel"
        finally:
            m.close()


# ---- A.4 h2_encode_kernel ---------------------------------------------------------------------------------------------------
ENC_SHAPE = (1, 80, 80, 80)          # SPPF on [0, 16) -> [16, 64): channels [0, 16) and [64, 80) are read back as the encoder wrote them
ENC_KEEP = np.r_[0:16, 64:80]


def encoder_specials():
    f32 = np.float32
    v = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -24, -1.5 * 2.0 ** -24, 65488.0, 65503.996, 65504.0, -65504.0]
    b = f32(2.0 ** -14)                                   # 6.1035e-5: the smallest normal fp16 number, and its fp32 neighbours
    v += [b, np.nextafter(b, f32(0)), np.nextafter(b, f32(1)), -b, -np.nextafter(b, f32(0)), -np.nextafter(b, f32(1))]
    for e in (-24, -20, -15, -14, -13, -5, 0, 1, 7, 10, 14, 15):      # halfway between adjacent fp16 numbers: (k + 1/2) ulp, k even and odd
        ulp = 2.0 ** (max(e, -14) - 10)
        base = 2.0 ** e
        for k in (0, 1, 2, 3, 510, 511):
            h = base + (k + 0.5) * ulp
            if h < 65504.0:
                v += [h, -h, float(np.nextafter(f32(h), f32(0))), float(np.nextafter(f32(h), f32(1e9)))]
    return np.array(v, np.float32)


def encoder_run(gpu_engine, x):
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_H2)
    b0 = g.buf(0, ENC_SHAPE[-1])
    g.sppf_pool(b0, 16)
    g.head_buf = (b0, -1, -1)
    m = E.Model(gpu_engine, g)
    m.set_max_batch(1)
    try:
        out = m.tracknet_infer(x)
        return out.view(np.uint16).reshape(out.shape[:-1] + (out.shape[-1] // 16, 32)), m.take_overflow()
    finally:
        m.close()


def _enc_input():
    rng = np.random.default_rng(11)
    sp = encoder_specials()
    mag = np.exp(rng.uniform(np.log(1e-9), np.log(65504.0), 100000)).astype(np.float32)
    mag = np.minimum(mag, np.float32(65504.0))
    vals = np.concatenate([sp, mag, -mag[:50000]]).astype(np.float32)
    x = np.zeros(ENC_SHAPE, np.float32)
    kept = x[..., ENC_KEEP].reshape(-1)
    assert vals.size <= kept.size
    kept[:vals.size] = vals
    x[..., ENC_KEEP] = kept.reshape(ENC_SHAPE[:-1] + (32,))
    return x


def _groups(bits):                       # the two kept 16-channel groups (0 and 4) of the (…, group, 32 halves) view
    return bits[..., (0, 4), :]


def test_h2_encode_matches_python_twin_bit_for_bit(gpu_engine):
    x = _enc_input()
    want = G.h2_encode_nhwc(x).view(np.uint16).reshape(ENC_SHAPE[:-1] + (5, 32))
    got, flag = encoder_run(gpu_engine, x)
    assert not flag, "overflow flag raised by values inside [-65504, 65504]"
    bad = np.argwhere(_groups(got) != _groups(want))
    assert bad.size == 0, f"{len(bad)} halves differ from graph.h2_split; first at {tuple(bad[0])}"


@pytest.mark.parametrize("value", [float(np.nextafter(np.float32(65504.0), np.float32(1e9))), -1e9, float("inf"), float("nan")],
                         ids=["65504-next", "-1e9", "inf", "nan"])
def test_h2_encode_flags_one_element_and_keeps_the_others(gpu_engine, value):
    x = _enc_input()
    pos = (0, 37, 41, 70)                                  # group 4, channel 6 of the group
    x[pos] = value
    want = G.h2_encode_nhwc(np.where(np.isfinite(x), x, np.float32(0))).view(np.uint16).reshape(ENC_SHAPE[:-1] + (5, 32)).copy()
    got, flag = encoder_run(gpu_engine, x)
    assert flag, f"{value}: the overflow flag stayed down"
    gi = (0, 37, 41, 4)
    if np.isfinite(value):                                 # clamped: the pair of +-65504
        big = np.array([np.sign(value) * 65504.0], np.float16).view(np.uint16)[0]
        assert got[gi][6] == big and got[gi][22] in (0x0000, 0x8000), (hex(got[gi][6]), hex(got[gi][22]))
        assert want[gi][6] == big
    want[gi][[6, 22]] = got[gi][[6, 22]]                   # every OTHER half keeps its bits
    bad = np.argwhere(_groups(got) != _groups(want))
    assert bad.size == 0, f"{value}: {len(bad)} other halves changed; first at {tuple(bad[0])}"


# ---- fp16 graphs: buffer widths of helper ops -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sppf", "maxpool", "upsample"])
def test_fp16_helper_on_a_buffer_that_is_not_a_multiple_of_8_wide_is_refused(gpu_engine, kind):
    """pool5_kernel<f16x8>, maxpool2_kernel<f16x8> and upsample2x_kernel<f16x8> move 16-byte vectors at pixel x width halves: with
    width % 8 == 4 every second pixel is misaligned.  Model creation fails with a message; nothing is launched."""
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F16)
    if kind == "sppf":
        b0 = g.buf(0, 36)
        g.sppf_pool(b0, 8)
        g.head_buf = (b0, -1, -1)
    elif kind == "maxpool":
        b0, b1 = g.buf(0, 32), g.buf(1, 36)
        g.maxpool2((b0, 0, 8), (b1, 8))
        g.head_buf = (b1, -1, -1)
    else:
        b0, b1, b2 = g.buf(0, 32), g.buf(1, 32), g.buf(0, 44)
        g.maxpool2((b0, 0, 8), (b1, 8))
        g.upsample2x((b1, 8, 8), (b2, 16))
        g.head_buf = (b2, -1, -1)
    with pytest.raises(E.EngineError, match="multiple of 8"):
        E.Model(gpu_engine, g)


# ---- B. activation epilogues ------------------------------------------------------------------------------------------------
# path -> (graph dtype, tuning while it runs, storage type of the input buffer)
ACT_PATHS = {
    "h2-three-product": (G.DTYPE_H2, dict(w_single=0), "h2"),
    "h2-two-product": (G.DTYPE_H2, dict(w_single=1), "h2"),       # the identity is an fp16 matrix: PA_CONV_W_SINGLE
    "fp16": (G.DTYPE_F16, dict(), "f16"),
    "bf16x3": (G.DTYPE_F32, dict(impl=2), "f32"),
    "strict-fp32": (G.DTYPE_F32, dict(impl=0), "f32"),
}
ACT_DEFAULTS = dict(impl=2, w_single=1, variant=-1)
ACT_SHAPE = (2, 132, 131, 64)
TAILS = np.array([s * v for v in (100.0, 200.0, 1e3, 1e4, 6e4) for s in (1.0, -1.0)], np.float32)
MAX_FACTOR, MEAN_FACTOR = 2.0, 1.5        # x the plain fp32 formula's own max / mean ulp error, measured beside the kernel's


def act_arguments():
    rng = np.random.default_rng(2024)
    sweep = np.concatenate([rng.uniform(-80.0, 80.0, 1000000), np.clip(rng.normal(0.0, 4.0, 1000000), -80.0, 80.0),
                            np.linspace(-80.0, 80.0, 200001)]).astype(np.float32) + np.float32(0.0)       # (+ 0: no negative zero)
    x = np.zeros(int(np.prod(ACT_SHAPE)), np.float32)
    assert sweep.size + TAILS.size <= x.size
    x[:sweep.size] = sweep
    x[sweep.size:sweep.size + TAILS.size] = TAILS
    return x.reshape(ACT_SHAPE), sweep.size


def act_run(eng, dtype, act, x, pairs=False):
    """Identity 1 x 1 (np.eye, zero bias) with ``act`` writing the fp32 head; ``pairs`` (h2): writing PAIRS, read back through a second
    identity without activation."""
    eye = np.eye(64, dtype=np.float32)[:, :, None, None]
    g = G.Graph(task=G.TASK_TRACKNET, dtype=dtype)
    b0 = g.buf(0, 64)
    if pairs:
        mid = g.buf(0, 64)
        g.conv((b0, 0, 64), (mid, 0), eye, np.zeros(64, np.float32), 1, 1, act)
        b0 = mid
        act = G.ACT_NONE
    hd = g.buf(0, 64)
    g.conv((b0, 0, 64), (hd, 0), eye, np.zeros(64, np.float32), 1, 1, act)
    g.head_buf = (hd, -1, -1)
    m = E.Model(eng, g)
    m.set_max_batch(ACT_SHAPE[0])
    try:
        y = m.tracknet_infer(x)
        if dtype == G.DTYPE_H2:
            assert not m.take_overflow()
    finally:
        m.close()
    return y


def ulp_error(got, truth):
    """|got - truth| in ulps of the fp32 result, the ulp taken at max(|truth|, 2^-126)."""
    _, e = np.frexp(np.maximum(np.abs(truth), 2.0 ** -126))
    return np.abs(got.astype(np.float64) - truth) / np.ldexp(1.0, e - 24)


ACT_TRUTH = {G.ACT_SILU: lambda v: v / (1.0 + np.exp(-v)), G.ACT_SIGMOID: lambda v: 1.0 / (1.0 + np.exp(-v))}
ACT_FP32 = {G.ACT_SILU: lambda v: v / (np.float32(1.0) + np.exp(-v)), G.ACT_SIGMOID: lambda v: np.float32(1.0) / (np.float32(1.0) + np.exp(-v))}
ACT_NAME = {G.ACT_SILU: "silu", G.ACT_SIGMOID: "sigmoid"}


def _report(line):
    print(line)
    out = os.environ.get("PADEL_REPORT_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "act_ulp_sweep.txt"), "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("path", list(ACT_PATHS))
def test_activation_epilogue_sweep(gpu_engine, path):
    dtype, tuning, st = ACT_PATHS[path]
    x32, n_sweep = act_arguments()
    xin = to_input(st, x32)
    held = stored_values(st, x32).astype(np.float32)                # what the input buffer holds: the exact argument of the activation
    try:
        gpu_engine.set_tuning(**{**ACT_DEFAULTS, **tuning})
        # premise: the identity conv delivers the stored value itself, bit for bit (the sign of a zero excepted: a stored -0, which
        # only an argument that underflowed can be, comes out of the accumulator as +0)
        y = act_run(gpu_engine, dtype, G.ACT_NONE, xin)
        assert np.array_equal((y + np.float32(0)).view(np.uint32), (held + np.float32(0)).view(np.uint32)), \
            f"{path}: the identity conv does not return its input bit for bit ({first_diff(y, held)}): no ulp statement for this path"
        arg = held.reshape(-1)[:n_sweep]
        tail = held.reshape(-1)[n_sweep:n_sweep + TAILS.size]
        a64 = arg.astype(np.float64)
        heads = {}
        for act in (G.ACT_SILU, G.ACT_SIGMOID):
            y = act_run(gpu_engine, dtype, act, xin)
            heads[act] = y
            assert np.isfinite(y).all(), f"{path} {ACT_NAME[act]}: non-finite results"
            truth = ACT_TRUTH[act](a64)
            with np.errstate(over="ignore"):
                floor = ulp_error(ACT_FP32[act](arg), truth)
            err = ulp_error(y.reshape(-1)[:n_sweep], truth)
            worst = int(err.argmax())
            _report(f"{path:17s} {ACT_NAME[act]:7s} arguments as {st:3s}: fp32 formula max {floor.max():.3f} mean {floor.mean():.4f} ulp | "
                    f"kernel max {err.max():.3f} (at x = {float(arg[worst])!r}) mean {err.mean():.4f} ulp")
            assert err.max() <= MAX_FACTOR * floor.max(), f"{path} {ACT_NAME[act]}: max {err.max():.3f} ulp at x = {float(arg[worst])!r}; the fp32 formula has {floor.max():.3f}"
            assert err.mean() <= MEAN_FACTOR * floor.mean(), f"{path} {ACT_NAME[act]}: mean {err.mean():.4f} ulp; the fp32 formula has {floor.mean():.4f}"
            # tails: a condition on the size of the result (the truth is below fp32's normal range for x <= -100)
            yt = y.reshape(-1)[n_sweep:n_sweep + TAILS.size].astype(np.float64)
            pos, neg = tail >= 100.0, tail <= -100.0
            assert pos.sum() == 5 and neg.sum() == 5
            lim = tail[pos].astype(np.float64) if act == G.ACT_SILU else np.ones(5)
            assert (np.abs(yt[pos] - lim) <= np.spacing(lim.astype(np.float32)).astype(np.float64)).all(), f"{path} {ACT_NAME[act]}: x >= 100 -> {yt[pos]}"
            assert (np.abs(yt[neg]) <= 1e-30).all(), f"{path} {ACT_NAME[act]}: x <= -100 -> {yt[neg]}"
            assert (yt[neg] <= 0).all() if act == G.ACT_SILU else (yt[neg] >= 0).all(), f"{path} {ACT_NAME[act]}: sign for x <= -100: {yt[neg]}"
        flat = held.reshape(-1)
        y = act_run(gpu_engine, dtype, G.ACT_RELU, xin).reshape(-1)
        assert np.array_equal(y, np.maximum(flat, np.float32(0))), f"{path} relu: {first_diff(y, np.maximum(flat, np.float32(0)))}"
        y = act_run(gpu_engine, dtype, G.ACT_LEAKY, xin).reshape(-1)
        want = np.where(flat >= 0, flat, np.float32(0.01) * flat).astype(np.float32)
        assert np.array_equal(y, want), f"{path} leaky: {first_diff(y, want)}"
        if st == "h2":      # the encoder of the epilogue: the pairs a conv stores are h2_split of the fp32 value its head store writes
            for act in (G.ACT_SILU, G.ACT_SIGMOID):
                yp = act_run(gpu_engine, dtype, act, xin, pairs=True)
                want = G.h2_value(*G.h2_split(heads[act]))
                assert np.array_equal(yp, want), f"{path} {ACT_NAME[act]}: pair store vs head store: {first_diff(yp, want)}"
    finally:
        gpu_engine.set_tuning(**ACT_DEFAULTS)
