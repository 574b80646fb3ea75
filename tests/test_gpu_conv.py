"""GPU unit test of the fp32-storage conv kernels through the C-ABI (the h2 kernels — the default arithmetic since round 3
— have their own file, tests/test_gpu_h2.py): every tile variant of the fp32-input MFMA generations (tap-unrolled LDS-DMA
kernels conv_tap.hip; the register-staged LDS kernel of round 1 that used to cross-check them is retired: tools/legacy_conv/conv_lds.hip) and of the bf16x3 kernels
(conv_tap_bx3.hip / conv_patch_bx3.hip: the full-range fallback of h2) against torch.nn.functional.conv2d (fp64 CPU), on
shapes that exercise stride 2, 1x1, the 16-channel K tail (cin % 32 == 16) including the full-chunk -> tail wrap of the tap
kernel's request ring, partial channel tiles (cout = 80 -> 5 fragments), the M tail, the fused residual and every
activation; each family BITWISE equal across its own tiles (same K order + same accumulation blocks)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import engine as E, graph as G
from tests import tile_support as TS

pytestmark = pytest.mark.gpu

# (B, H, W, cin, cout, k, stride, act, residual)
CASES = [
    (2, 24, 40, 32, 64, 3, 1, G.ACT_SILU, False),
    (3, 20, 36, 48, 80, 3, 1, G.ACT_SILU, True),      # full chunk -> K-tail wrap + partial N tile + residual
    (2, 32, 48, 16, 16, 3, 2, G.ACT_RELU, False),     # stride 2, smallest channels (tail block only)
    (1, 16, 24, 96, 96, 1, 1, G.ACT_NONE, False),     # 1x1, no activation
    (2, 12, 20, 64, 144, 3, 1, G.ACT_SIGMOID, False),
    (1, 36, 28, 288, 48, 1, 1, G.ACT_SILU, True),
    (1, 8, 12, 576, 192, 3, 1, G.ACT_SILU, False),    # long K: exercises several accumulation blocks
    (2, 32, 48, 64, 96, 3, 2, G.ACT_SILU, True),      # stride 2 with cin % 32 == 0, residual at the output resolution
    (3, 17, 23, 96, 96, 3, 1, G.ACT_SILU, True),      # odd spatial size: M tail + borders in every tile, residual
    (2, 16, 20, 80, 48, 3, 1, G.ACT_SILU, False),     # two full chunks + tail (cin 80), 48 outputs (128x48 tile)
    (2, 18, 26, 16, 32, 3, 1, G.ACT_SILU, False),     # stride 1 with the tail block only (n-scale's 16 channels), partial patches
    (2, 20, 24, 64, 192, 3, 1, G.ACT_SILU, True),     # two full 96-channel tiles (quad patch kernel: both channel halves), partial patches in y and x
    (1, 20, 27, 688, 96, 1, 1, G.ACT_SILU, False),    # 1x1 with long K: 21 full chunks + a 16-channel tail = three accumulation blocks (9 + 9 + 4), M tail
    (3, 18, 22, 96, 208, 3, 2, G.ACT_SILU, True),     # stride 2 to an odd map (9 x 11 outputs: M tail, every border), 13 fragments = two 192-channel tiles, residual
    # added with tests/tile_support.py (tests/test_tile_coverage.py says which (tile, class) cells each of these fills)
    (2, 16, 16, 64, 80, 3, 1, G.ACT_LEAKY, False),    # LeakyReLU (InpaintNet's activation); 512 pixels x 80 channels: whole 64 x 80 tiles (25 / 225), partial 96- and 64-channel tiles
    (1, 16, 32, 32, 384, 3, 1, G.ACT_RELU, False),    # whole tiles for every tile shape but 64 x 80 (384 = 3 x 128 = 4 x 96 = 8 x 48), whole 8 x 16 and 16 x 16 patches
    (1, 18, 20, 64, 39, 3, 1, G.ACT_NONE, True),      # cout % 16 != 0: a partial channel FRAGMENT (element-wise stores), residual, no activation
]
ACT_FN = {G.ACT_SILU: F.silu, G.ACT_RELU: F.relu, G.ACT_SIGMOID: torch.sigmoid, G.ACT_NONE: lambda t: t, G.ACT_LEAKY: lambda t: F.leaky_relu(t, 0.01)}

TAP_VARIANTS = (6, 7, 9, 10, 11, 12, 13, 14, 15, 20)
BX3_VARIANTS = (6, 7, 9, 11, 12, 13, 14, 20, 25, 206, 207, 209, 211, 220, 225, 213, 303, 304, 306)      # bf16x3 kernels (conv_tap_bx3.hip): fp32 accuracy, own rounding


def _launched(m, which=-1):
    """(family, tile) the engine reports for a conv of the op list (default: the last one, the conv under test), from the profile rows."""
    r = [r for r in m.profile_rows() if r["kind"] == G.OP_CONV][which]
    return r["family"], r["tile"]


def _check_launched(path, case, requested, got, w_single=False):
    """The forced runs of one case against tests/tile_support.py, both directions; prints the (requested -> launched) table."""
    print(f"case {case}{' two-product' if w_single else ''}: " + "  ".join(f"{t} -> {f}/{v}" for t, (f, v) in got.items()))
    for t, fv in got.items():
        want = TS.expected(path, t, case, w_single)
        assert fv == want, f"requested {t}, launched {fv[0]}/{fv[1]}; tests/tile_support.py says {want[0]}/{want[1]}"
    assert set(got) == {t for t, _ in requested}

def _run(eng, case, x, w, b, wr, ran=None):
    """Graph: [op0: 1x1 conv (stride s, no act) x -> residual buffer]  op1: the conv under test (+ residual).
    ``ran``: a dict -> profiling on for this run, ``ran["launched"]`` = (family, tile) of the conv under test."""
    B, H, W, cin, cout, k, s, act, use_res = case
    g = G.Graph(task=G.TASK_TRACKNET)
    b0 = g.buf(0, cin)
    lvl = 1 if s == 2 else 0
    b1 = g.buf(lvl, G.pad16(cout))
    res = None
    if use_res:
        b2 = g.buf(lvl, G.pad16(cout))
        g.conv((b0, 0, cin), (b2, 0), wr, np.zeros(cout, np.float32), 1, s, G.ACT_NONE)
        res = (b2, 0)
    g.conv((b0, 0, cin), (b1, 0), w, b, k, s, act, res=res)
    g.head_buf = (b1, -1, -1)
    m = E.Model(eng, g)
    m.set_max_batch(B)
    if ran is not None:
        eng.set_profiling(True)
    try:
        y = m.tracknet_infer(x)[..., :cout]
        if ran is not None:
            ran["launched"] = _launched(m)
    finally:
        if ran is not None:
            eng.set_profiling(False)
    m.close()
    return y


@pytest.mark.parametrize("case", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_conv_variants(gpu_engine, case):
    B, H, W, cin, cout, k, s, act, use_res = case
    rng = np.random.default_rng(cin * 131 + cout)
    x = rng.normal(0, 1, (B, H, W, cin)).astype(np.float32)
    w = rng.normal(0, (2.0 / (cin * k * k)) ** 0.5, (cout, cin, k, k)).astype(np.float32)
    b = rng.normal(0, 0.5, cout).astype(np.float32)
    wr = rng.normal(0, (1.0 / cin) ** 0.5, (cout, cin, 1, 1)).astype(np.float32)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    want = F.conv2d(xt.double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=s, padding=k // 2)
    want = ACT_FN[act](want)
    if use_res:
        want = want + F.conv2d(xt.double(), torch.from_numpy(wr).double(), stride=s)
    want = want.permute(0, 2, 3, 1).numpy()
    scale = max(1.0, float(np.abs(want).max()))
    outs = {}
    runs, got = TS.plan("tap", TAP_VARIANTS, case), {}
    try:
        for v, _ in runs:                                 # LDS-DMA ring: twice, a DMA / barrier race is not deterministic
            gpu_engine.set_tuning(impl=0, variant=v)
            for rep in range(2):
                ran = {}
                outs[f"T{v}.{rep}"] = _run(gpu_engine, case, x, w, b, wr, ran=ran)
                got[v] = ran["launched"]
        gpu_engine.set_tuning(impl=0, variant=7, tap_pd=3)   # 1x1 tap kernel with prefetch distance 3
        outs["T7.pd3"] = _run(gpu_engine, case, x, w, b, wr)
        gpu_engine.set_tuning(impl=0, variant=-1, tap_pd=2)
        outs["auto"] = _run(gpu_engine, case, x, w, b, wr)
        gpu_engine.set_tuning(graph=1)
        outs["auto.graph"] = _run(gpu_engine, case, x, w, b, wr)
        gpu_engine.set_tuning(graph=0, alias=0)
        outs["auto.noalias"] = _run(gpu_engine, case, x, w, b, wr)
    finally:
        gpu_engine.set_tuning(impl=2, variant=-1, tap_pd=2, graph=0, alias=1)
    _check_launched("tap", case, runs, got)
    ref_name, ref = next(iter(outs.items()))
    for name, y in outs.items():
        assert y.shape == want.shape
        err = float(np.abs(y - want).max()) / scale
        assert err < 3e-6, f"{name}: rel err {err:.2e} vs fp64 conv2d"
        assert np.array_equal(y, ref), f"{name} differs bitwise from {ref_name} (max {np.abs(y - ref).max():.3e})"
    # ---- bf16x3: same accuracy bar against fp64, bitwise equal among its own tiles, and its RMS error not worse
    # than the fp32 MFMA kernels' (the admission criterion for making it the default)
    outs3 = {}
    runs3, got3 = TS.plan("bx3", BX3_VARIANTS, case), {}      # (the 30x ids on a conv the patch kernel does not take are duplicates of 220 / 209 / 206)
    try:
        for v, _ in runs3:
            gpu_engine.set_tuning(impl=2, variant=v)
            for rep in range(2):
                ran = {}
                outs3[f"B{v}.{rep}"] = _run(gpu_engine, case, x, w, b, wr, ran=ran)
                got3[v] = ran["launched"]
        gpu_engine.set_tuning(impl=2, variant=-1)
        outs3["B.auto"] = _run(gpu_engine, case, x, w, b, wr)
    finally:
        gpu_engine.set_tuning(impl=2, variant=-1)
    _check_launched("bx3", case, runs3, got3)
    n3, r3 = next(iter(outs3.items()))
    for name, y in outs3.items():
        err = float(np.abs(y - want).max()) / scale
        assert err < 3e-6, f"{name}: rel err {err:.2e} vs fp64 conv2d"
        assert np.array_equal(y, r3), f"{name} differs bitwise from {n3} (max {np.abs(y - r3).max():.3e})"
    rms32 = float(np.sqrt(np.mean((ref - want) ** 2)))
    rms3 = float(np.sqrt(np.mean((r3 - want) ** 2)))
    print(f"case {case}: RMS error vs fp64  fp32-MFMA {rms32:.3e}  bf16x3 {rms3:.3e}")
    assert rms3 <= 1.25 * rms32 + 1e-9, (rms3, rms32)


# ---- channel slices (real graphs read C2f halves at a channel offset and write into slices of concat buffers; the sweeps above
# only ever use offset 0).  Shared with the fp16 path (tests/test_gpu_fp16.py); the h2 path has its own, tests/test_gpu_h2_epilogue.py.
SLICE_BASES = [(1, 16, 16, 64, 3, 1), (1, 16, 16, 64, 1, 1), (1, 32, 32, 64, 3, 2)]      # (B, H, W, cin, k, stride)
SLICE_WIDTH = 160
BIG = 3.0e4                                                                              # what the neighbours of an input / residual slice hold


def slice_sentinel(n):
    return (-100.0 - 0.25 * np.arange(n)).astype(np.float32)          # fp16 numbers


def slice_graph(dtype, base, cout, d, use_res, out_choff=0, in_choff=None, res_choff=0):
    """[1x1 -> residual slice], sentinel fill of the SLICE_WIDTH-wide buffer S (1x1, zero weights, bias = sentinel), the conv under
    test -> S[out_choff : out_choff + cout]; fp32 graphs read S back as the head, fp16 graphs through an identity 1x1.  ``in_choff``
    (not None): the input through an identity copy into channel ``in_choff`` of a wider buffer whose other channels hold BIG;
    ``res_choff``: the residual at that channel of a wider buffer.  Returns (graph, index of the conv under test among the convs)."""
    B, H, W, cin, k, s = base
    z = lambda *shape: np.zeros(shape, np.float32)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=dtype)
    b0 = g.buf(0, cin)
    lvl = 1 if s == 2 else 0
    src = (b0, 0, cin)
    if in_choff is not None:
        bi = g.buf(0, in_choff + cin + (16 if in_choff else 0))
        if in_choff:
            g.conv((b0, 0, cin), (bi, 0), z(in_choff, cin, 1, 1), np.full(in_choff, BIG, np.float32), 1, 1, G.ACT_NONE)
            g.conv((b0, 0, cin), (bi, in_choff + cin), z(16, cin, 1, 1), np.full(16, BIG, np.float32), 1, 1, G.ACT_NONE)
        g.conv((b0, 0, cin), (bi, in_choff), np.eye(cin, dtype=np.float32)[:, :, None, None], z(cin), 1, 1, G.ACT_NONE)
        src = (bi, in_choff, cin)
    res = None
    if use_res:
        rw = (res_choff + cout + 15) // 16 * 16
        rb = g.buf(lvl, rw)
        if res_choff:
            g.conv((b0, 0, cin), (rb, 0), z(res_choff, cin, 1, 1), np.full(res_choff, BIG, np.float32), 1, s, G.ACT_NONE)
        g.conv((b0, 0, cin), (rb, res_choff), d["wr"], z(cout), 1, s, G.ACT_NONE)
        res = (rb, res_choff)
    S = g.buf(lvl, SLICE_WIDTH)
    g.conv((b0, 0, cin), (S, 0), z(SLICE_WIDTH, cin, 1, 1), slice_sentinel(SLICE_WIDTH), 1, s, G.ACT_NONE)
    g.conv(src, (S, out_choff), d["w"], d["b"], k, s, G.ACT_SILU, res=res)
    if dtype == G.DTYPE_F16:
        hd = g.buf(lvl, SLICE_WIDTH)
        g.conv((S, 0, SLICE_WIDTH), (hd, 0), np.eye(SLICE_WIDTH, dtype=np.float32)[:, :, None, None], z(SLICE_WIDTH), 1, 1, G.ACT_NONE)
        g.head_buf = (hd, -1, -1)
        return g, -2
    g.head_buf = (S, -1, -1)
    return g, -1


def slice_data(base, cout, f16=False):
    B, H, W, cin, k, s = base
    rng = np.random.default_rng(cin * 7 + cout * 5 + k + s)
    r = (lambda a: a.astype(np.float16).astype(np.float32)) if f16 else (lambda a: a.astype(np.float32))
    x = rng.normal(0, 1, (B, H, W, cin))
    return dict(x=x.astype(np.float16) if f16 else x.astype(np.float32), w=r(rng.normal(0, (2.0 / (cin * k * k)) ** 0.5, (cout, cin, k, k))),
                b=rng.normal(0, 0.5, cout).astype(np.float32), wr=r(rng.normal(0, (1.0 / cin) ** 0.5, (cout, cin, 1, 1))))


def slice_run(eng, path, dtype, base, cout, d, use_res, tile, **kw):
    """One forced run of a slice graph; what launched is checked against tests/tile_support.py.  Returns S as fp32 (B, Ho, Wo, SLICE_WIDTH)."""
    g, which = slice_graph(dtype, base, cout, d, use_res, **kw)
    B, H, W, cin, k, s = base
    case = (B, H, W, cin, cout, k, s, G.ACT_SILU, use_res)
    eng.set_tuning(variant=tile)
    eng.set_profiling(True)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(B)
        y = m.tracknet_infer(d["x"])
        got = _launched(m, which)
    finally:
        eng.set_profiling(False)
        m.close()
    want = TS.expected(path, tile, case)
    assert got == want, f"requested {tile}, launched {got[0]}/{got[1]}; tests/tile_support.py says {want[0]}/{want[1]}"
    return y


def check_slices(eng, path, dtype, tiles, base, out_slices, res_offsets):
    """The three slice statements on every native tile of ``tiles``: (1) cout channels written at out_choff are the bits of the
    offset-0 run and every other channel of S keeps its sentinel — also under a 96- / 128-channel tile that overhangs the slice;
    (2) an input slice at channel 32 between channels that hold BIG, (3) a residual at ``res_offsets``: bitwise the offset-0 runs.
    The offsets include one that misses the vector alignment the fast epilogues test (4 floats / 8 halves): element-wise path."""
    B, H, W, cin, k, s = base
    f16 = dtype == G.DTYPE_F16
    sent = slice_sentinel(SLICE_WIDTH)
    nat = lambda cout, res: [t for t in tiles if TS.native(path, t, (B, H, W, cin, cout, k, s, G.ACT_SILU, res))]
    for choff, cout, res in out_slices:
        d = slice_data(base, cout, f16)
        for t in nat(cout, res):
            ref = slice_run(eng, path, dtype, base, cout, d, res, t)
            y = slice_run(eng, path, dtype, base, cout, d, res, t, out_choff=choff)
            name = f"{path} tile {t}, {cout} channels at {choff}"
            assert np.array_equal(y[..., choff:choff + cout], ref[..., :cout]), f"{name}: differs from the offset-0 run"
            rest = np.concatenate([y[..., :choff], y[..., choff + cout:]], -1)
            bad = rest != np.broadcast_to(np.concatenate([sent[:choff], sent[choff + cout:]]), rest.shape)
            assert not bad.any(), f"{name}: {int(bad.sum())} values outside the slice changed"
            assert np.array_equal(ref[..., cout:], np.broadcast_to(sent[cout:], ref[..., cout:].shape)), f"{name}: the offset-0 run wrote beyond its channels"
    for cout in (96, 40):
        d = slice_data(base, cout, f16)
        for t in nat(cout, True):
            ref = slice_run(eng, path, dtype, base, cout, d, True, t, in_choff=0)
            y = slice_run(eng, path, dtype, base, cout, d, True, t, in_choff=32)
            assert np.array_equal(y, ref), f"{path} tile {t}, cout {cout}: input slice at channel 32 differs from offset 0 (max {np.abs(y - ref).max():.3e})"
            ref = slice_run(eng, path, dtype, base, cout, d, True, t)
            for rc in res_offsets:
                y = slice_run(eng, path, dtype, base, cout, d, True, t, res_choff=rc)
                assert np.array_equal(y, ref), f"{path} tile {t}, cout {cout}: residual at channel {rc} differs from offset 0 (max {np.abs(y - ref).max():.3e})"


@pytest.mark.parametrize("base", SLICE_BASES, ids=["3x3", "1x1", "s2"])
@pytest.mark.parametrize("path", ["tap", "bx3"])
def test_conv_slices(gpu_engine, path, base):
    """fp32 storage (tap_epilogue / bx3_common.h): the vector path needs choff % 4 == 0 and cs % 4 == 0; 6 is the offset that misses it."""
    try:
        gpu_engine.set_tuning(impl=0 if path == "tap" else 2)
        check_slices(gpu_engine, path, G.DTYPE_F32, TAP_VARIANTS if path == "tap" else BX3_VARIANTS, base,
                     [(16, 32, False), (48, 80, True), (16, 96, True), (6, 26, True)], (16, 6))
    finally:
        gpu_engine.set_tuning(impl=2, variant=-1)


@pytest.mark.parametrize("shape", [(2, 24, 40, 64, 32, 80, 1), (1, 18, 28, 32, 48, 96, 1), (3, 16, 16, 96, 16, 48, 1),
                                   (2, 24, 48, 64, 32, 80, 3), (1, 16, 32, 32, 96, 48, 3), (2, 40, 16, 96, 32, 64, 3)],
                         ids=["up64+32", "up32+48", "up96+16", "3x3-up64+32", "3x3-up32+96", "3x3-up96+32"])
def test_upsample_absorbed(gpu_engine, shape):
    """Upsample(2) + cat in front of a stride-1 conv is never materialised — the bf16x3 1x1 kernel (YOLOv8's
    FPN joins) and the 3x3 patch kernel (TrackNet's decoder blocks) read the first channels at [y >> 1][x >> 1] of the
    coarse map (csrc/graph_plan.cpp:find_upsample_folds).  Same arithmetic on the same values: bitwise equal to running the
    upsample kernel, for every tile that has the absorbing instantiation; tiles without it keep the upsample kernel."""
    B, H, W, c_up, c_skip, cout, k = shape
    rng = np.random.default_rng(c_up * 7 + c_skip + k)
    cin0 = 32
    x = rng.normal(0, 1, (B, H, W, cin0)).astype(np.float32)
    w_dn = rng.normal(0, (2.0 / (cin0 * 9)) ** 0.5, (c_up, cin0, 3, 3)).astype(np.float32)
    w_sk = rng.normal(0, (2.0 / cin0) ** 0.5, (c_skip, cin0, 1, 1)).astype(np.float32)
    w = rng.normal(0, (2.0 / ((c_up + c_skip) * k * k)) ** 0.5, (cout, c_up + c_skip, k, k)).astype(np.float32)
    b = rng.normal(0, 0.5, cout).astype(np.float32)

    def run(**tuning):
        g = G.Graph(task=G.TASK_TRACKNET)
        b0 = g.buf(0, cin0)
        coarse = g.buf(1, c_up)
        cat = g.buf(0, c_up + c_skip)
        out = g.buf(0, G.pad16(cout))
        g.conv((b0, 0, cin0), (coarse, 0), w_dn, np.zeros(c_up, np.float32), 3, 2, G.ACT_SILU)
        g.upsample2x((coarse, 0, c_up), (cat, 0))
        g.conv((b0, 0, cin0), (cat, c_up), w_sk, np.zeros(c_skip, np.float32), 1, 1, G.ACT_NONE)
        g.conv((cat, 0, c_up + c_skip), (out, 0), w, b, k, 1, G.ACT_SILU)
        g.head_buf = (out, -1, -1)
        gpu_engine.set_tuning(**tuning)
        gpu_engine.set_profiling(True)
        m = E.Model(gpu_engine, g)
        m.set_max_batch(B)
        y = m.tracknet_infer(x)[..., :cout]
        n_up = sum(1 for r in m.profile_rows() if r["kind"] == G.OP_UPSAMPLE2X)
        m.close()
        gpu_engine.set_profiling(False)
        return y, n_up

    # tile ids with an absorbing instantiation: every 1x1 id maps to one; 3x3: the patch kernel (30x) only
    absorbing = (-1, 220, 209, 213, 7) if k == 1 else (-1, 303, 304, 306)
    keeping = () if k == 1 else (220, 213)
    try:
        ref, n_up = run(impl=2, variant=-1, fold_up=0)
        assert n_up == 1
        for v in absorbing + keeping:
            y, n_up = run(impl=2, variant=v, fold_up=1)
            if v == -1 and k == 3:
                assert n_up in (0, 1)                   # the per-layer heuristic may prefer a tap tile on a tiny map
            else:
                assert n_up == (0 if v in absorbing else 1), f"variant {v}: {n_up} upsample launches"
            assert np.array_equal(y, ref), f"variant {v}: absorbed upsample differs (max {np.abs(y - ref).max():.3e})"
        y, n_up = run(impl=0, variant=-1, fold_up=1)        # the fp32-MFMA kernels keep the upsample kernel
        assert n_up == 1
    finally:
        gpu_engine.set_tuning(impl=2, variant=-1, fold_up=1)
