"""The ops the ResNet-50 graph adds, each on its own through a unit op list (the style of tests/test_gpu_helpers.py):
MaxPool2d(3, 2, 1), the 7x7 stem, the pooled linear head, the pre-activation residual (PA_CONV_RES_PREACT) per native h2 tile
and on bf16x3, and the 1x1 stride-2 conv no graph had used before."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import engine as E, graph as G
from tests import tile_support as TS
from tests.test_gpu_conv import BX3_VARIANTS, _launched
from tests.test_gpu_h2 import H2_TILES
from tests.test_gpu_h2_epilogue import native_runs, sentinel
from tests.test_gpu_helpers import ACT_FP32, ACT_TRUTH, MAX_FACTOR, MEAN_FACTOR, ulp_error

DTYPES = {"f32": G.DTYPE_F32, "h2": G.DTYPE_H2}
z = lambda *shape: np.zeros(shape, np.float32)
eye = lambda n: np.eye(n, dtype=np.float32)[:, :, None, None]


def held(dtype, x):
    """What a buffer of this storage type holds after x was written to it."""
    return G.h2_value(*G.h2_split(x)) if dtype == "h2" else np.asarray(x, np.float32)


# ---------------------------------------------------------------------------------------- MaxPool2d(3, 2, 1)
def pool_content(kind, rng, shape):
    if kind == "negative":            # every value below zero: a zero-padded pool would return 0 at the borders
        return -rng.uniform(0.5, 900.0, shape).astype(np.float32)
    if kind == "ties":                # +0 / -0 and few distinct values: ties everywhere
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 0.5], np.float32), shape)
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(6e4), shape))
    return (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)      # wide magnitudes


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "h2"])
@pytest.mark.parametrize("out_hw", [(112, 112), (7, 7), (1, 1), (5, 9)])
def test_maxpool3s2_equals_fp64_max_pool2d(gpu_engine, dtype, out_hw):
    Ho, Wo = out_hw
    H, W, B = 2 * Ho, 2 * Wo, 2
    cin_w, in_off, c, out_off, out_w = (48, 16, 16, 4, 32) if dtype == "h2" else (24, 4, 8, 12, 24)
    for kind in ("negative", "ties", "wide"):
        rng = np.random.default_rng(Ho * 31 + Wo + len(kind))
        x = pool_content(kind, rng, (B, H, W, cin_w))
        g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPES[dtype])
        b0 = g.buf(0, cin_w)
        S = g.buf(1, out_w)
        fill = G.pad16(out_w)
        g.conv((b0, 0, cin_w if dtype == "h2" else 16), (S, 0), z(out_w, cin_w if dtype == "h2" else 16, 1, 1), sentinel(fill)[:out_w], 1, 2, G.ACT_NONE)
        g.maxpool3s2((b0, in_off, c), (S, out_off))
        if dtype == "h2":             # pairs -> fp32 through an identity 1x1 (exact)
            hd = g.buf(1, out_w)
            g.conv((S, 0, out_w), (hd, 0), eye(out_w), z(out_w), 1, 1, G.ACT_NONE)
            g.head_buf = (hd, -1, -1)
        else:
            g.head_buf = (S, -1, -1)
        m = E.Model(gpu_engine, g)
        try:
            m.set_max_batch(B)
            y = m.tracknet_infer(x)
            assert not m.take_overflow()
        finally:
            m.close()
        xin = held(dtype, x)[..., in_off:in_off + c]
        want = F.max_pool2d(torch.from_numpy(xin).double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
        assert want.shape == (B, Ho, Wo, c)
        got = y[..., out_off:out_off + c]
        assert np.array_equal(got.astype(np.float64), want), (kind, int((got != want).sum()))
        keep = np.ones(out_w, bool)
        keep[out_off:out_off + c] = False
        assert np.array_equal(y[..., keep], np.broadcast_to(sentinel(fill)[:out_w][keep], y[..., keep].shape)), f"{kind}: neighbouring channels touched"


# ---------------------------------------------------------------------------------------- 7x7 stem
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "h2-pairs", "h2-head"])
def test_stem7_against_fp64_conv2d(gpu_engine, mode):
    rng = np.random.default_rng(7)
    B = 2
    frames = rng.integers(0, 256, (B, 224, 224, 3), dtype=np.uint8)          # 224 x 224: no resize, the network input is the frame (RGB)
    frames[0, :8] = 255; frames[0, -8:] = 0; frames[1, :, :8] = 0; frames[1, :, -8:] = 255      # strong borders: padding must be zero in NORMALISED space
    w = rng.normal(0, (2.0 / 147) ** 0.5, (64, 3, 7, 7)).astype(np.float32)
    b = rng.normal(0, 0.5, 64).astype(np.float32)
    dtype = "f32" if mode == "f32" else "h2"
    g = G.Graph(task=G.TASK_RESNET, dtype=DTYPES[dtype])
    st = g.buf(1, 64)
    g.stem7(w, b, (st, 0))
    if mode == "h2-pairs":
        hd = g.buf(1, 64)
        g.conv((st, 0, 64), (hd, 0), eye(64), z(64), 1, 1, G.ACT_NONE)
        g.head_buf = (hd, -1, -1)
    else:
        g.head_buf = (st, -1, -1)
    m = E.Model(gpu_engine, g)
    try:
        m.set_max_batch(2)
        xy, logits = m.resnet_infer(frames[:2], 2, 224, 224)
        assert xy is None and logits is None
        y = m.resnet_read_head(2)
        netin = m.resnet_read_netin(2)
        assert not m.take_overflow()
    finally:
        m.close()
    assert np.array_equal(netin[..., :3], frames[:2, ..., ::-1]) and not netin[..., 3].any()
    lut = G.resnet_norm_table().astype(np.float64)
    rgb = frames[:2, ..., ::-1]
    xn = np.stack([lut[c][rgb[..., c]] for c in range(3)], axis=1)            # (n, 3, 224, 224)
    want = F.relu(F.conv2d(torch.from_numpy(xn), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2, padding=3))
    want = want.permute(0, 2, 3, 1).numpy()
    assert y.shape == want.shape == (2, 112, 112, 64)
    rel = np.abs(y - want).max() / max(1.0, np.abs(want).max())
    border = np.zeros((112, 112), bool)
    border[:2] = border[-2:] = border[:, :2] = border[:, -2:] = True
    print(f"stem7 {mode}: rel err {rel:.2e} (borders {np.abs(y - want)[:, border].max() / max(1.0, np.abs(want).max()):.2e})")
    assert rel < 3e-6, rel
    assert (want[:, border] > 0).any()


# ---------------------------------------------------------------------------------------- pooled linear head
def _gap_fc(eng, dtype, x, w, b):
    B, H, W, C = x.shape
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPES[dtype])
    b0 = g.buf(0, C)
    g.gap_fc((b0, 0, C), w, b)
    g.head_buf = (b0, -1, -1)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(B)
        m.tracknet_infer(x)
        return m.read_fc(B)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "h2"])
def test_gap_fc_logits_within_twice_the_fp32_formula(gpu_engine, dtype):
    rng = np.random.default_rng(5)
    B, H, W, C, N = 5, 7, 7, 2048, 24
    x = np.maximum(rng.normal(0.3, 1.0, (B, H, W, C)), 0).astype(np.float32)      # behind a ReLU, like layer4's output
    w = rng.normal(0, 0.05, (N, C)).astype(np.float32)
    b = rng.normal(0, 0.5, N).astype(np.float32)
    xy, logits = _gap_fc(gpu_engine, dtype, x, w, b)
    xh = held(dtype, x)
    z64 = xh.astype(np.float64).mean(axis=(1, 2)) @ w.astype(np.float64).T + b.astype(np.float64)
    mean32 = (xh.reshape(B, H * W, C).sum(axis=1, dtype=np.float32) / np.float32(H * W)).astype(np.float32)
    z32 = (mean32 @ w.T + b).astype(np.float32)                              # the formula in float32, as numpy evaluates it
    floor, err = np.abs(z32 - z64).max(), np.abs(logits - z64).max()
    print(f"gap_fc {dtype}: logits L-inf {err:.3e}; fp32 numpy formula {floor:.3e}")
    assert err <= 2 * floor, (err, floor)
    assert ((xy > 0) & (xy < 1)).all()           # (the sigmoid's own bound: the sweep below)


@pytest.mark.gpu
def test_gap_fc_sigmoid_meets_the_activation_sweep_bound(gpu_engine):
    """32 768 logits spread like the sweep's arguments: kernel max <= 2 x, mean <= 1.5 x the float32 formula's own ulp error."""
    rng = np.random.default_rng(9)
    B, C, N = 512, 16, 64
    x = rng.normal(0, 1, (B, 2, 2, C)).astype(np.float32)
    w = rng.normal(0, 2.0, (N, C)).astype(np.float32)
    b = rng.normal(0, 2.0, N).astype(np.float32)
    xy, logits = _gap_fc(gpu_engine, "f32", x, w, b)
    assert np.abs(logits).max() < 80 and logits.std() > 2
    truth = ACT_TRUTH[G.ACT_SIGMOID](logits.astype(np.float64).reshape(-1))
    floor = ulp_error(ACT_FP32[G.ACT_SIGMOID](logits.reshape(-1)), truth)
    err = ulp_error(xy.reshape(-1), truth)
    print(f"gap_fc sigmoid: fp32 formula max {floor.max():.3f} mean {floor.mean():.4f} ulp | kernel max {err.max():.3f} mean {err.mean():.4f} ulp")
    assert err.max() <= MAX_FACTOR * floor.max() and err.mean() <= MEAN_FACTOR * floor.mean()


# ---------------------------------------------------------------------------------------- pre-activation residual
# (B, H, W, cin, cout, k, stride, act, residual): per kernel group whole and partial tiles, all with ReLU and a residual
PRE_CASES = [
    (1, 8, 16, 64, 192, 3, 1, G.ACT_RELU, True),
    (3, 17, 23, 96, 96, 3, 1, G.ACT_RELU, True),
    (1, 8, 16, 64, 80, 3, 1, G.ACT_RELU, True),
    (1, 16, 16, 16, 96, 3, 1, G.ACT_RELU, True),
    (1, 16, 24, 128, 192, 1, 1, G.ACT_RELU, True),
    (1, 20, 27, 704, 96, 1, 1, G.ACT_RELU, True),
    (1, 8, 16, 64, 80, 1, 1, G.ACT_RELU, True),
    (2, 32, 32, 64, 192, 3, 2, G.ACT_RELU, True),
    (1, 18, 22, 128, 80, 3, 2, G.ACT_RELU, True),
]


def test_preact_cases_reach_every_h2_tile_natively():
    reached = {t for case in PRE_CASES for t, _ in native_runs(case)}
    assert reached == set(H2_TILES), sorted(set(H2_TILES) - reached)


def _pre_data(case):
    B, H, W, cin, cout, k, s, act, _ = case
    rng = np.random.default_rng(cin * 17 + cout + k + s)
    return dict(x=rng.normal(0, 1, (B, H, W, cin)).astype(np.float32),
                w=rng.normal(0, (2.0 / (cin * k * k)) ** 0.5, (cout, cin, k, k)).astype(np.float16).astype(np.float32),
                scale=rng.uniform(0.5, 2.0, cout).astype(np.float32), b=rng.normal(0, 0.5, cout).astype(np.float32),
                wr=rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin, 1, 1)).astype(np.float32))


def _pre_want(case, d):
    """(relu(conv + r), relu(conv) + r, conv + bias, r) in fp64, NHWC."""
    B, H, W, cin, cout, k, s, act, _ = case
    xt = torch.from_numpy(d["x"]).permute(0, 3, 1, 2).double()
    w = torch.from_numpy(d["w"]).double() * torch.from_numpy(d["scale"]).double()[:, None, None, None]
    conv = F.conv2d(xt, w, torch.from_numpy(d["b"]).double(), stride=s, padding=k // 2)
    r = F.conv2d(xt, torch.from_numpy(d["wr"]).double(), stride=s)
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    return nhwc(F.relu(conv + r)), nhwc(F.relu(conv) + r), nhwc(conv), nhwc(r)


def _pre_graph(case, d, dtype, head, flagged=True):
    B, H, W, cin, cout, k, s, act, _ = case
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPES[dtype])
    b0 = g.buf(0, cin)
    lvl = 1 if s == 2 else 0
    rb = g.buf(lvl, G.pad16(cout))
    g.conv((b0, 0, cin), (rb, 0), d["wr"], z(cout), 1, s, G.ACT_NONE)
    wd = G.pad16(cout)
    scale = d["scale"] if dtype == "h2" else None
    wgt = d["w"] if dtype == "h2" else (d["w"] * d["scale"][:, None, None, None]).astype(np.float32)
    if head == "direct":
        b1 = g.buf(lvl, wd)
        g.conv((b0, 0, cin), (b1, 0), wgt, d["b"], k, s, act, res=(rb, 0), out_scale=scale, res_preact=flagged)
        g.head_buf = (b1, -1, -1)
        return g, -1
    S = g.buf(lvl, wd)
    g.conv((b0, 0, cin), (S, 0), z(wd, cin, 1, 1), sentinel(wd), 1, s, G.ACT_NONE)
    g.conv((b0, 0, cin), (S, 0), wgt, d["b"], k, s, act, res=(rb, 0), out_scale=scale, res_preact=flagged)
    hd = g.buf(lvl, wd)
    g.conv((S, 0, wd), (hd, 0), eye(wd), z(wd), 1, 1, G.ACT_NONE)
    g.head_buf = (hd, -1, -1)
    return g, -2


def _pre_run(eng, case, d, dtype, head, tile, ws=True, flagged=True, path="h2"):
    g, which = _pre_graph(case, d, dtype, head, flagged)
    eng.set_tuning(variant=tile, w_single=1 if ws else 0)
    eng.set_profiling(True)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(case[0])
        y = m.tracknet_infer(d["x"])
        got = _launched(m, which)
        assert not m.take_overflow()
    finally:
        eng.set_profiling(False)
        m.close()
    if tile >= 0:
        want = TS.expected(path, tile, case, ws)
        assert got == want, f"requested {tile}, launched {got}; tests/tile_support.py says {want}"
    return y[..., :case[4]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PRE_CASES, ids=[f"p{i}" for i in range(len(PRE_CASES))])
def test_preact_residual_per_h2_tile(gpu_engine, case):
    d = _pre_data(case)
    pre, post, conv, r = _pre_want(case, d)
    sc = max(1.0, float(np.abs(pre).max()))
    flips = np.mean((conv > 0) != (conv + r > 0))
    assert flips > 0.1 and np.abs(pre - post).max() > 0.5, "the residual must move the sum across zero"
    try:
        first = True
        for tile, ws in native_runs(case):
            y32 = _pre_run(gpu_engine, case, d, "h2", "direct", tile, ws)        # fp32 head: element-wise path
            err = float(np.abs(y32 - pre).max()) / sc
            assert err < 3e-6, f"tile {tile}: fp32 head rel err {err:.2e} vs fp64 relu(conv + r)"
            y = _pre_run(gpu_engine, case, d, "h2", "pairs", tile, ws)           # pairs: 16-byte path (+ residual load) / element-wise
            stored = G.h2_value(*G.h2_split(y32))
            assert np.array_equal(y, stored), f"tile {tile}: pair store differs from h2_split of its own fp32 output ({int((y != stored).sum())} values)"
            assert float(np.abs(y - pre).max()) / sc < 3e-6
            if first:                                                            # the same case unflagged: the other order
                first = False
                for head in ("direct", "pairs"):
                    yu = _pre_run(gpu_engine, case, d, "h2", head, tile, ws, flagged=False)
                    assert float(np.abs(yu - post).max()) / sc < 3e-6
                    assert np.abs(yu - (y32 if head == "direct" else y)).max() > 0.5, "flagged and unflagged runs agree: the flag is ignored"
    finally:
        gpu_engine.set_tuning(variant=-1, w_single=1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [PRE_CASES[i] for i in (0, 1, 4, 5, 7, 8)], ids=lambda c: f"{c[3]}-{c[4]}-k{c[5]}s{c[6]}")
def test_preact_residual_bf16x3(gpu_engine, case):
    d = _pre_data(case)
    pre, post, _, _ = _pre_want(case, d)
    sc = max(1.0, float(np.abs(pre).max()))
    try:
        gpu_engine.set_tuning(impl=2)
        tiles = [t for t in BX3_VARIANTS if TS.native("bx3", t, case)]
        assert tiles
        for i, tile in enumerate(tiles):
            y = _pre_run(gpu_engine, case, d, "f32", "direct", tile, path="bx3")
            err = float(np.abs(y - pre).max()) / sc
            assert err < 3e-6, f"bf16x3 tile {tile}: rel err {err:.2e}"
            if i == 0:
                yu = _pre_run(gpu_engine, case, d, "f32", "direct", tile, flagged=False, path="bx3")
                assert float(np.abs(yu - post).max()) / sc < 3e-6 and np.abs(yu - y).max() > 0.5
    finally:
        gpu_engine.set_tuning(variant=-1, impl=2)


@pytest.mark.gpu
def test_preact_is_refused_where_it_is_not_implemented(gpu_engine):
    case = PRE_CASES[4]
    d = _pre_data(case)
    g, _ = _pre_graph(case, d, "f32", "direct")
    try:
        gpu_engine.set_tuning(impl=0)                                            # fp32-MFMA tap kernels
        m = E.Model(gpu_engine, g)
        try:
            m.set_max_batch(case[0])
            with pytest.raises(E.EngineError, match="PA_CONV_RES_PREACT"):
                m.tracknet_infer(d["x"])
        finally:
            m.close()
    finally:
        gpu_engine.set_tuning(impl=2)
    g16 = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F16)                        # fp16 storage: refused at model creation
    b0, rb, b1 = g16.buf(0, 128), g16.buf(0, 192), g16.buf(0, 192)
    g16.conv((b0, 0, 128), (rb, 0), d["wr"], z(192), 1, 1, G.ACT_NONE)
    g16.conv((b0, 0, 128), (b1, 0), d["w"], d["b"], 1, 1, G.ACT_RELU, res=(rb, 0))
    g16.ops[-1]["flags"] |= G.FLAG_RES_PREACT
    g16.head_buf = (b1, -1, -1)
    with pytest.raises(E.EngineError, match="PA_CONV_RES_PREACT"):
        E.Model(gpu_engine, g16)
    g2, _ = _pre_graph(case, d, "h2", "direct")                                   # the flag without a residual slice
    g2.ops[-1]["res_buf"] = -1
    with pytest.raises(E.EngineError, match="PA_CONV_RES_PREACT"):
        E.Model(gpu_engine, g2)


# ---------------------------------------------------------------------------------------- 1x1 stride 2
S2_CASES = [(2, 56, 56, 256, 512), (2, 14, 14, 1024, 2048), (1, 10, 18, 64, 80), (3, 6, 10, 48, 40)]      # 56 -> 28, 14 -> 7, 5 x 9, 3 x 5 outputs
H2_TAP_TILES = (207, 209, 211, 213, 220, 225, 239, 243)


def _s2_run(eng, dtype, shape, x, w, b, tile, path):
    B, H, W, cin, cout = shape
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPES[dtype])
    b0, b1 = g.buf(0, cin), g.buf(1, G.pad16(cout))
    g.conv((b0, 0, cin), (b1, 0), w, b, 1, 2, G.ACT_NONE)
    g.head_buf = (b1, -1, -1)
    eng.set_tuning(variant=tile)
    eng.set_profiling(True)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(B)
        y = m.tracknet_infer(x)
        got = _launched(m)
        assert not m.take_overflow()
    finally:
        eng.set_profiling(False)
        m.close()
    if tile >= 0:
        case = (B, H, W, cin, cout, 1, 2, G.ACT_NONE, False)
        assert got == TS.expected(path, tile, case, False), (tile, got)
    return y[..., :cout], got


@pytest.mark.gpu
@pytest.mark.parametrize("shape", S2_CASES, ids=lambda s: "x".join(map(str, s)))
def test_conv_1x1_stride_2(gpu_engine, shape):
    """ResNet's downsample branch: out[y][x] = W in[2y][2x] + b.  Every h2 tap tile agrees bit for bit (one accumulation scheme);
    h2 and bf16x3 each stay inside the conv bound against fp64 (they round differently: no bitwise promise between them)."""
    B, H, W, cin, cout = shape
    rng = np.random.default_rng(cin + cout)
    x = rng.normal(0, 1, (B, H, W, cin)).astype(np.float32)
    w = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin, 1, 1)).astype(np.float32)
    b = rng.normal(0, 0.5, cout).astype(np.float32)
    want = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2)
    want = want.permute(0, 2, 3, 1).numpy()
    assert np.allclose(want, x[:, ::2, ::2].astype(np.float64) @ w[:, :, 0, 0].astype(np.float64).T + b.astype(np.float64), rtol=0, atol=1e-12)
    sc = max(1.0, float(np.abs(want).max()))
    case = (B, H, W, cin, cout, 1, 2, G.ACT_NONE, False)
    try:
        ref_y = None
        for tile in (-1,) + tuple(t for t in H2_TAP_TILES if TS.native("h2", t, case)):
            y, got = _s2_run(gpu_engine, "h2", shape, x, w, b, tile, "h2")
            err = float(np.abs(y - want).max()) / sc
            assert err < 3e-6, f"h2 tile {tile} ({got}): rel err {err:.2e}"
            if ref_y is None:
                ref_y = y
            assert np.array_equal(y, ref_y), f"h2 tile {tile} ({got}) differs from the first h2 run"
        gpu_engine.set_tuning(impl=2)
        for tile in (-1,) + tuple(t for t in (9, 13, 20, 207, 209, 220, 213) if TS.native("bx3", t, case)):
            y, got = _s2_run(gpu_engine, "f32", shape, x, w, b, tile, "bx3")
            err = float(np.abs(y - want).max()) / sc
            assert err < 3e-6, f"bf16x3 tile {tile} ({got}): rel err {err:.2e}"
    finally:
        gpu_engine.set_tuning(variant=-1)
