"""GPU tests of the two kernels that turn the u8 network input into the first activations, read back directly:
``stem_mfma_kernel<NF, OM>`` (csrc/kernels_misc.hip) and the stem phase and layer 1 of ``stem_l1_h2_kernel<NF, WS, WR>``
(csrc/stem_l1_h2.hip).

The instrument (tests/stem_probe.py; checked on the CPU by tests/test_stem_probe_host.py): a ``TASK_DETECT`` graph with one class
whose head is a pixel-unshuffle of the stem's level-1 map — stride-2 3x3 convs with one-hot weights, every product but one an
exact zero — so that ``Model.read_head(0, n)`` returns the stored values themselves: the fp32 word, the half, or h + m / 2048 of a
pair.  Every head byte is written by the graph (``counts == 0``), fp32 and h2 graphs run over an arena filled with NaN patterns,
frames have the network's own size (letterbox = copy) and the reference is computed from ``read_netin``, the bytes the kernel saw.
``test_unshuffle_premise`` states the premise per storage type on a random array: the unshuffle chain is a bit-exact permutation
(the sign of a zero excepted); a stem test whose premise fails says "no statement for this path".

Reference: fp64 on the exact bytes, x = u8 / 255, t = sum_k w_k x_k + b over the 27 taps with zero outside the image,
v = t / (1 + exp(-t)), and S = sum_k |w_k| x_k + |b|, the scale of the rounding error.  With u = 2^-24 a result passes when

    |got - v| <= 1.1 K u S + A ulp32(v) + store(v)

1.1: the largest |silu'| (1.0998).  K = 30 for the stand-alone kernel: one rounding of u8 / 255 in its table, one per product, 28
additions including the bias.  K = 36 for the fused kernel's stem phase: the same plus the fp16-pair representation of w / 255
(<= 2^-22 relative = 4 u) plus the two fmaf of its scale-and-bias step.  K is derived, not fitted: numpy fp32 emulations of both
orders stay below a third of it (tests/test_stem_probe_host.py), a dropped or misplaced tap is an error of order 0.04 S.
A = 2 x 3.402 ulp, the admission bound of the SiLU epilogues (tests/test_gpu_helpers.py, profiles/act_ulp_sweep.txt).  store(v):
0 for fp32, 2^-11 |v| + 2^-25 for fp16, 2^-22 |v| for pairs — and the value must be one the storage can hold.

A. stand-alone stem (``fuse_stem = 0``): every width 16 .. 80 (NF 1 .. 5; 64 and 80, yolov8 l / x, run nowhere else) in fp32 and
   pairs, 32 and 64 in fp16; maps of 16 x 16, 16 x 48 (a non-trivial fast division) and 48 x 32 with batches 1 .. 3; a write into a
   slice of a wider buffer; 327 680 stem pixels, which take the grid-stride loop into its second pass (the grid is capped at
   4096 workgroups of 4 x 16 pixels); the overflow flag.
B. fused stem + layer 1 (h2, widths 16 / 32 / 48): layer 1 has exactly 2 c outputs, so the readout of the stem phase is layer 1
   itself with one-hot weights — each row selects one (tap, channel), five passes cover the 9 c pairs.  Per pass: the fused kernel
   ran (one conv row fewer in the profile); where the tap lies in layer 1's padding the value is exactly 0.0 (a kernel that
   evaluated the stem there would leave silu(bias), |bias| >= 0.25); everywhere else the bound with K = 36; every stem element
   seen twice — odd rows and columns: tap 0 of one output and tap 2 of its neighbour, often in another workgroup's tile or in the
   tail planes versus the chunk planes — is seen with the same bits.  Register weights, the weight ring (tune = 8) and three
   products (w_single = 0).  Then layer 1's own arithmetic with random weights and SiLU against an fp64 conv over the stem map
   reassembled from the readout, under the h2 conv criterion of tests/test_gpu_h2.py (3e-6 relative).

Every test prints its worst |got - v| / (u S); where ``PADEL_REPORT_DIR`` names a directory the line is appended to
``stem_direct.txt`` there (profiles/stem_direct.txt is a copy of one such run)."""
import os

import numpy as np
import pytest

from padel_analytics_amd import engine as E, graph as G
from tests import stem_probe as P
from tests.test_gpu_helpers import stored_values, to_input

pytestmark = pytest.mark.gpu

DEFAULTS = dict(fuse_stem=1, w_single=1, tune=1, impl=2, variant=-1)
SHAPES_A = [(1, 32, 32), (3, 32, 96), (2, 96, 64)]
BIG_SHAPE = (5, 512, 512)                            # 5 x 256 x 256 = 327 680 stem pixels
KW = dict(conf=0.25, iou=0.7)


def _report(line):
    print(line)
    out = os.environ.get("PADEL_REPORT_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "stem_direct.txt"), "a") as f:
            f.write(line + "\n")


# ---- premise: the unshuffle convs return their input bit for bit ---------------------------------------------------------------
# path -> (storage, tuning, input channels, unshuffle levels): the chains the probe graphs put behind the stem
PREMISES = {
    "f32-bf16x3": ("f32", dict(impl=2), 16, 2),
    "f32-strict": ("f32", dict(impl=0), 16, 2),
    "h2": ("h2", dict(), 16, 2),
    "h2-three-product": ("h2", dict(w_single=0), 16, 2),
    "h2-behind-layer1": ("h2", dict(), 32, 1),
    "f16": ("f16", dict(), 32, 2),
}
_premise_result = {}


def premise(eng, path):
    """None, or why the unshuffle chain of ``path`` is not a bit-exact permutation (computed once per path)."""
    if path not in _premise_result:
        t, tuning, cin, levels = PREMISES[path]
        rng = np.random.default_rng(len(path) + cin)
        shape = (2, 24, 40, cin)
        mag = np.exp(rng.uniform(np.log(1e-7), np.log(6e4), shape))
        x = np.where(rng.random(shape) < 0.5, rng.normal(0, 1, shape), mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
        x.reshape(-1)[:8] = [6.0e4, -6.0e4, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 0.0, 1e-7, -1e-7]      # (a pair store flags h = 65504 itself: the clamp's value)
        held = stored_values(t, x).astype(np.float32)
        m = E.Model(eng, P.premise_graph(t, cin, levels))
        m.set_max_batch(shape[0])
        try:
            eng.set_tuning(**{**DEFAULTS, **tuning})
            got = P.unshuffle_decode(m.tracknet_infer(to_input(t, x)), levels)
            flag = t == "h2" and m.take_overflow()
        finally:
            eng.set_tuning(**DEFAULTS)
            m.close()
        bad = np.argwhere((got + np.float32(0)).view(np.uint32) != (held + np.float32(0)).view(np.uint32))
        _premise_result[path] = (f"{len(bad)} of {got.size} values differ, first at {tuple(int(i) for i in bad[0])}: got {got[tuple(bad[0])]!r}, "
                                 f"stored {held[tuple(bad[0])]!r}" if len(bad) else "the overflow flag was raised" if flag else None)
    return _premise_result[path]


def require_premise(eng, path):
    why = premise(eng, path)
    assert why is None, f"{path}: the unshuffle convs do not return their input bit for bit ({why}): no statement for this path"


@pytest.mark.parametrize("path", list(PREMISES))
def test_unshuffle_premise(gpu_engine, path):
    require_premise(gpu_engine, path)


# ---- running a probe graph ----------------------------------------------------------------------------------------------------
def infer(m, frames, fill):
    """One inference of a probe model on frames of the network's own size -> (level-3 head map, the u8 network input).  ``fill``:
    over an arena of NaN patterns (fp32 / h2 graphs; the first call makes the plan that is filled)."""
    B, h, w, _ = frames.shape
    assert h % 32 == 0 and w % 32 == 0
    m.set_max_batch(B)
    kw = dict(imgsz=max(h, w), **KW)
    if fill:
        m.yolo_infer(frames, B, h, w, **kw)
        m.fill_arena(0xFF)
    _, _, counts = m.yolo_infer(frames, B, h, w, **kw)
    assert (counts == 0).all(), "a probe graph has no detections: decode keeps nothing"
    netin = m.read_netin(B)
    assert netin.shape == (B, h, w, 4) and np.array_equal(netin[..., :3], frames), "letterbox of a frame of the network's size is a copy"
    return m.read_head(0, B), netin


def n_conv_rows(m):
    return sum(1 for r in m.profile_rows() if r["kind"] == G.OP_CONV)


# ---- A. stand-alone stem ------------------------------------------------------------------------------------------------------
# (storage, width, tuning of the readout convs, premise)
CASES_A = [("f32", c, dict(impl=2), "f32-bf16x3") for c in (16, 32, 48, 64, 80)] + [("f32", 48, dict(impl=0), "f32-strict")] + \
          [("h2", c, dict(), "h2") for c in (16, 32, 48, 64, 80)] + [("f16", c, dict(), "f16") for c in (32, 64)]


def run_standalone(eng, t, c, tuning, shapes, buf_width=0, choff=0, name=None):
    name = name or f"stem_mfma_kernel<{c // 16}, {('f32', 'f16', 'h2').index(t)}> {t} c{c}"
    w, b = P.stem_weights(c)
    m = E.Model(eng, P.standalone_graph(t, c, w, b, buf_width, choff))
    worst = 0.0
    try:
        eng.set_tuning(**{**DEFAULTS, **tuning, "fuse_stem": 0})
        for shape in shapes:
            head, netin = infer(m, P.probe_frames(*shape), fill=t != "f16")
            assert not np.isnan(head).any(), f"{name} {shape}: a head byte the graph did not write"
            v, S = P.stem_truth(netin, w, b)
            worst = max(worst, P.check(f"{name} {shape}", t, P.K_STANDALONE, P.decode_level1(head), v, S))
            if t == "h2":
                assert not m.take_overflow(), f"{name} {shape}: overflow flag with ordinary weights"
    finally:
        eng.set_tuning(**DEFAULTS)
        m.close()
    _report(f"{name}{''.join(f' {k}={v}' for k, v in tuning.items())}: worst |got - v| / (u S) = {worst:.3f} (K = {P.K_STANDALONE}) over {shapes}")


@pytest.mark.parametrize("t,c,tuning,path", CASES_A, ids=[f"{t}-c{c}" + "".join(f"-{k}{v}" for k, v in tu.items()) for t, c, tu, _ in CASES_A])
def test_standalone_stem(gpu_engine, t, c, tuning, path):
    require_premise(gpu_engine, path)
    run_standalone(gpu_engine, t, c, tuning, SHAPES_A)


@pytest.mark.parametrize("t,path", [("f32", "f32-bf16x3"), ("h2", "h2"), ("f16", "f16")])
def test_standalone_stem_writes_a_slice(gpu_engine, t, path):
    """16 channels at channel 16 of a 48-channel level-1 buffer: ``out_choff`` and a pixel stride that is not the width."""
    require_premise(gpu_engine, path)
    run_standalone(gpu_engine, t, 16, {}, SHAPES_A[1:], buf_width=48, choff=16, name=f"stem_mfma_kernel {t} c16 at 16 of 48")


@pytest.mark.parametrize("t,path", [("f32", "f32-bf16x3"), ("h2", "h2")])
def test_standalone_stem_grid_stride_second_pass(gpu_engine, t, path):
    """``launch_stem`` caps the grid at 256 x 16 workgroups of 4 waves x 16 pixels: beyond 262 144 pixels a wave takes a second tile."""
    B, h, w = BIG_SHAPE
    assert B * (h // 2) * (w // 2) > 4096 * 4 * 16
    require_premise(gpu_engine, path)
    run_standalone(gpu_engine, t, 16, {}, [BIG_SHAPE], name=f"stem_mfma_kernel {t} c16 second pass")


def test_standalone_stem_raises_the_overflow_flag(gpu_engine):
    w, b = P.stem_weights(16)
    b[5] = P.BIG_BIAS
    m = E.Model(gpu_engine, P.standalone_graph("h2", 16, w, b))
    try:
        gpu_engine.set_tuning(**{**DEFAULTS, "fuse_stem": 0})
        infer(m, P.probe_frames(*SHAPES_A[1]), fill=True)
        assert m.take_overflow(), "silu(7e4) does not fit a pair and the flag stayed down"
        assert not m.take_overflow(), "taking the flag clears it"
    finally:
        gpu_engine.set_tuning(**DEFAULTS)
        m.close()


# ---- B. fused stem + layer 1 --------------------------------------------------------------------------------------------------
VARIANTS = {"register-weights": dict(), "weight-ring": dict(tune=8), "three-product": dict(w_single=0)}
SHAPES_B = [(1, 32, 32), (3, 32, 96), (2, 64, 160), (9, 32, 64)]
CASES_B = [(c, SHAPES_B[1], v) for c in (16, 32, 48) for v in VARIANTS] + [(c, s, "register-weights") for c in (16, 32, 48) for s in (SHAPES_B[0], SHAPES_B[2], SHAPES_B[3])]
_stem_maps = {}                                      # (c, shape) -> (stem map reassembled from the readout, network input)


def run_fused(eng, g, frames, tuning, name):
    """The graph under ``fuse_stem = 0`` (profile: its conv rows) and under ``fuse_stem = 1`` with ``tuning``; asserts that the
    fused kernel ran -> (layer-1 map of the fused run, network input, overflow flag of the fused run)."""
    m = E.Model(eng, g)
    eng.set_profiling(True)
    try:
        eng.set_tuning(**{**DEFAULTS, **tuning, "fuse_stem": 0})
        infer(m, frames, fill=True)
        rows0 = n_conv_rows(m)
        m.take_overflow()
        eng.set_tuning(fuse_stem=1)
        head, netin = infer(m, frames, fill=True)
        rows1 = n_conv_rows(m)
        flag = m.take_overflow()
    finally:
        eng.set_tuning(**DEFAULTS)
        eng.set_profiling(False)
        m.close()
    assert rows1 == rows0 - 1, f"{name}: the fused kernel did not run (layer 1 was launched on its own: {rows1} conv rows, {rows0} unfused)"
    assert not np.isnan(head).any(), f"{name}: a head byte the graph did not write"
    return P.decode_layer1(head), netin, flag


def read_stem_phase(eng, c, shape, variant):
    """The five readout passes -> (Observations, network input); B.1 is asserted per pass."""
    w, b = P.stem_weights(c)
    frames = P.probe_frames(*shape)
    obs = P.Observations(c)
    for p in range(P.N_PASSES):
        name = f"stem_l1_h2_kernel<{c // 16}> {variant} c{c} {shape} pass {p}"
        l1, netin, flag = run_fused(eng, P.fused_readout_graph(c, w, b, p), frames, VARIANTS[variant], name)
        assert not flag, f"{name}: overflow flag with ordinary weights"
        obs.add_pass(p, l1)
    return obs, netin


def check_stem_phase(c, shape, variant, obs, netin):
    name = f"stem_l1_h2_kernel<{c // 16}> {variant} c{c} {shape}"
    w, b = P.stem_weights(c)
    # B.2: layer 1's padding is exactly zero
    for tap, z in obs.padding():
        bad = np.argwhere(z != 0.0)
        assert bad.size == 0, (f"{name}: tap {divmod(tap, 3)} in layer 1's padding reads {float(z[tuple(bad[0])])!r} at (image, position, "
                               f"channel) = {tuple(int(i) for i in bad[0])}; silu(bias) of that channel is {float(b[bad[0][-1]] / (1 + np.exp(-b[bad[0][-1]]))):.4f}")
    # B.4: one stem element, one value — whichever tile, plane set or pass computed it
    stem, differ, twice = obs.reassemble()
    assert twice > 0
    assert differ == 0 and obs.repeat_mismatch == 0, \
        f"{name}: {differ} of {twice} second observations of a stem element differ bitwise from the first ({obs.repeat_mismatch} among the repeats of the last pass)"
    # B.3: the bound
    v, S = P.stem_truth(netin, w, b)
    worst = P.check(name, "h2", P.K_FUSED, stem, v, S)
    _report(f"{name}: worst |got - v| / (u S) = {worst:.3f} (K = {P.K_FUSED}); {twice} elements seen twice, all bit-identical")
    return stem


@pytest.mark.parametrize("c,shape,variant", CASES_B, ids=[f"c{c}-{'x'.join(map(str, s))}-{v}" for c, s, v in CASES_B])
def test_fused_stem_phase(gpu_engine, c, shape, variant):
    require_premise(gpu_engine, "h2-behind-layer1" if variant != "three-product" else "h2-three-product")
    obs, netin = read_stem_phase(gpu_engine, c, shape, variant)
    stem = check_stem_phase(c, shape, variant, obs, netin)
    if variant == "register-weights":
        _stem_maps[(c, shape)] = (stem, netin)


def stem_map(eng, c, shape):
    """The fused kernel's stem map of (weights, frames) of this width and shape, read once and left unchanged."""
    if (c, shape) not in _stem_maps:
        obs, netin = read_stem_phase(eng, c, shape, "register-weights")
        _stem_maps[(c, shape)] = (check_stem_phase(c, shape, "register-weights", obs, netin), netin)
    return _stem_maps[(c, shape)]


@pytest.mark.parametrize("shape", [SHAPES_B[1], SHAPES_B[2]], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", [16, 32, 48])
def test_fused_layer1_arithmetic(gpu_engine, c, shape):
    """Random layer-1 weights and bias with SiLU, read through one unshuffle: fp32-random weights (three products), the same rounded
    to fp16 (two products: register weights, and the weight ring).  Truth: an fp64 conv over the very pairs the kernel's LDS held."""
    require_premise(gpu_engine, "h2-behind-layer1")
    stem, netin0 = stem_map(gpu_engine, c, shape)
    w, b = P.stem_weights(c)
    w1, b1 = P.layer1_weights(c)
    w1h = w1.astype(np.float16).astype(np.float32)
    frames = P.probe_frames(*shape)
    for wname, wts, tuning in (("fp32 weights, three products", w1, {}), ("fp16 weights, register weights", w1h, {}), ("fp16 weights, weight ring", w1h, dict(tune=8))):
        name = f"stem_l1_h2_kernel<{c // 16}> layer 1 c{c} {shape} {wname}"
        g = P.fused_graph(c, w, b, wts, b1, G.ACT_SILU)
        assert bool(g.ops[1]["flags"] & G.FLAG_W_SINGLE) == (wts is w1h)
        got, netin, flag = run_fused(gpu_engine, g, frames, tuning, name)
        assert not flag and np.array_equal(netin, netin0)
        want = P.layer1_truth(stem, wts, b1)
        assert np.isfinite(got).all() and P.storable("h2", got), name
        err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
        print(f"{name}: rel err {err:.2e} vs fp64 conv2d over the stem map")
        assert err < 3e-6, f"{name}: rel err {err:.2e} vs fp64 conv2d"


@pytest.mark.parametrize("c", [16, 32, 48])
def test_fused_stem_raises_the_overflow_flag(gpu_engine, c):
    w, b = P.stem_weights(c)
    b[5] = P.BIG_BIAS
    w1, b1 = P.layer1_weights(c)
    _, _, flag = run_fused(gpu_engine, P.fused_graph(c, w, b, w1.astype(np.float16).astype(np.float32), b1, G.ACT_SILU), P.probe_frames(*SHAPES_B[1]), {},
                           f"stem_l1_h2_kernel<{c // 16}> c{c} stem bias 7e4")
    assert flag, "silu(7e4) does not fit a pair and the flag stayed down"
