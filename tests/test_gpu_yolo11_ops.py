"""The two ops YOLO11 adds, each on its own through a unit op list (the style of tests/test_gpu_resnet_ops.py): the depthwise 3x3
against fp64 ``conv2d(groups=C)`` at every border, the PSA attention against the fp64 formula with the fp32 torch evaluation of the
same formula on the same inputs as the yardstick."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import engine as E, graph as G
from tests.test_gpu_h2_epilogue import sentinel
from tests.yolo11_ref import psa_attention
from tests.yolo11_report import record

pytestmark = pytest.mark.gpu

DTYPES = {"f32": G.DTYPE_F32, "h2": G.DTYPE_H2}
z = lambda *shape: np.zeros(shape, np.float32)
eye = lambda n: np.eye(n, dtype=np.float32)[:, :, None, None]


def held(dtype, x):
    """What a buffer of this storage type holds after x was written to it."""
    return G.h2_value(*G.h2_split(x)) if dtype == "h2" else np.asarray(x, np.float32)


def _run(eng, g, x, replay_after_fill=False):
    m = E.Model(eng, g)
    try:
        m.set_max_batch(x.shape[0])
        y = m.tracknet_infer(x)
        ovf = m.take_overflow()
        if replay_after_fill:
            m.fill_arena(0xFF)
            y2 = m.tracknet_infer(x)
            assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), "a replay over NaN-filled arena bytes changed the result"
        return y, ovf
    finally:
        m.close()


def _to_head(g, dtype, S, out_w):
    """Pairs -> fp32 through an identity 1x1 (exact); fp32 buffers are read directly."""
    if dtype == "h2":
        hd = g.buf(0, out_w)
        g.conv((S, 0, out_w), (hd, 0), eye(out_w), z(out_w), 1, 1, G.ACT_NONE)
        g.head_buf = (hd, -1, -1)
    else:
        g.head_buf = (S, -1, -1)


# ---------------------------------------------------------------------------------------- depthwise 3x3
IN_OFF, OUT_OFF = 16, 20          # the slices sit at channel offsets of wider buffers


def _dw_graph(dtype, C, act, res):
    """b0 = [16 pad | C input | C residual | 16 pad]; S = sentinel-filled, the op writes S[OUT_OFF : OUT_OFF + C]."""
    in_w, out_w = 32 + 2 * C, G.pad16(OUT_OFF + C + 12)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPES[dtype])
    b0, S = g.buf(0, in_w), g.buf(0, out_w)
    g.conv((b0, 0, in_w), (S, 0), z(out_w, in_w, 1, 1), sentinel(out_w), 1, 1, G.ACT_NONE)
    return g, b0, S, in_w, out_w


def _dw_case(eng, dtype, B, H, W, C, act, res, content, replay=False):
    rng = np.random.default_rng(H * 131 + W * 17 + C + act + 2 * res)
    g, b0, S, in_w, out_w = _dw_graph(dtype, C, act, res)
    w = rng.normal(0, 0.4, (C, 1, 3, 3)).astype(np.float32)
    b = rng.normal(0, 0.5, C).astype(np.float32)
    x = rng.normal(0, 1.5, (B, H, W, in_w)).astype(np.float32)
    if content == "negative":          # every input below zero, every weight above: each tap that exists lowers the sum
        x, w = -np.abs(x) - 0.25, np.abs(w) + 0.05
    g.dwconv3((b0, IN_OFF, C), (S, OUT_OFF), w, b, act, res=(b0, IN_OFF + C) if res else None)
    _to_head(g, dtype, S, out_w)
    y, ovf = _run(eng, g, x, replay_after_fill=replay)
    assert not ovf
    xh = torch.from_numpy(held(dtype, x)).double().permute(0, 3, 1, 2)
    want = F.conv2d(xh[:, IN_OFF:IN_OFF + C], torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1, groups=C)
    if act == G.ACT_SILU:
        want = F.silu(want)
    if res:
        want = want + xh[:, IN_OFF + C:IN_OFF + 2 * C]
    want = want.permute(0, 2, 3, 1).numpy()
    got = y[..., OUT_OFF:OUT_OFF + C]
    rel = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    assert rel < 3e-6, f"{dtype} {H}x{W} C={C} act={act} res={res} {content}: rel err {rel:.2e} vs fp64 conv2d(groups=C)"
    if content == "negative" and act == G.ACT_NONE and not res:
        assert (got - b < 0).all()
    keep = np.ones(out_w, bool)
    keep[OUT_OFF:OUT_OFF + C] = False
    assert np.array_equal(y[..., keep], np.broadcast_to(sentinel(out_w)[keep], y[..., keep].shape)), "neighbouring channels touched"
    return rel


@pytest.mark.parametrize("dtype", ["f32", "h2"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (3, 5), (20, 20), (33, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_depthwise_equals_fp64_grouped_conv2d(gpu_engine, dtype, hw):
    worst = 0.0
    for C in (16, 80, 384):
        for act in (G.ACT_NONE, G.ACT_SILU):
            for res in (False, True):
                worst = max(worst, _dw_case(gpu_engine, dtype, 2, hw[0], hw[1], C, act, res, "normal"))
        worst = max(worst, _dw_case(gpu_engine, dtype, 2, hw[0], hw[1], C, G.ACT_NONE, False, "negative"))
    print(f"depthwise {dtype} {hw}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("dtype", ["f32", "h2"])
def test_depthwise_replay_over_nan_filled_arena(gpu_engine, dtype):
    for hw in ((1, 1), (3, 5), (33, 17)):
        _dw_case(gpu_engine, dtype, 2, hw[0], hw[1], 80, G.ACT_SILU, True, "normal", replay=True)


def test_depthwise_h2_output_beyond_fp16_raises_the_overflow_flag(gpu_engine):
    C = 16
    g, b0, S, in_w, out_w = _dw_graph("h2", C, G.ACT_NONE, False)
    g.dwconv3((b0, IN_OFF, C), (S, OUT_OFF), np.ones((C, 1, 3, 3), np.float32), z(C), G.ACT_NONE)
    _to_head(g, "h2", S, out_w)
    x = np.full((2, 5, 5, in_w), 100.0, np.float32)
    x[..., IN_OFF:IN_OFF + C] = 3.0e4                      # nine taps: 2.7e5 > 65504 in the interior, 1.2e5 in the corners
    _, ovf = _run(gpu_engine, g, x)
    assert ovf
    x[..., IN_OFF:IN_OFF + C] = 3.0e3                      # 2.7e4: fits
    y, ovf = _run(gpu_engine, g, x)
    assert not ovf and y[0, 2, 2, OUT_OFF] == 2.7e4 and y[0, 0, 0, OUT_OFF] == 1.2e4


def test_new_ops_are_validated(gpu_engine):
    g, b0, S, in_w, out_w = _dw_graph("f32", 16, G.ACT_NONE, False)
    g.dwconv3((b0, IN_OFF, 16), (b0, IN_OFF + 8), z(16, 1, 3, 3), z(16), G.ACT_NONE)          # writes the slice it reads
    g.head_buf = (S, -1, -1)
    with pytest.raises(E.EngineError, match="cannot write the slice it reads"):
        E.Model(gpu_engine, g)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F32)
    b0, b1 = g.buf(0, 2 * (2 * 16 + 64)), g.buf(0, 128)
    g.psa_attn((b0, 0), (b1, 0), heads=2, kd=16, hd=64)
    g.head_buf = (b1, -1, -1)
    with pytest.raises(E.EngineError, match="key dim 32 and head dim 64 only"):
        E.Model(gpu_engine, g)


# ---------------------------------------------------------------------------------------- PSA attention
TOKENS = {1: (1, 1), 15: (3, 5), 64: (8, 8), 65: (5, 13), 240: (12, 20), 400: (20, 20), 1600: (40, 40)}
A_IN_OFF, A_OUT_OFF = 16, 4


def _attn_graph(dtype, heads):
    in_w, out_w = 32 + heads * 128, G.pad16(A_OUT_OFF + heads * 64 + 12)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPES[dtype])
    b0, S = g.buf(0, in_w), g.buf(0, out_w)
    g.conv((b0, 0, in_w), (S, 0), z(out_w, in_w, 1, 1), sentinel(out_w), 1, 1, G.ACT_NONE)
    g.psa_attn((b0, A_IN_OFF), (S, A_OUT_OFF), heads)
    _to_head(g, dtype, S, out_w)
    return g, in_w, out_w


def _attn_input(heads, B, N, kind, seed):
    """(B, H, W, in_w) buffer content: [16 pad | q of all heads | k of all heads | v of all heads | 16 pad]."""
    H, W = TOKENS[N]
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1.0, (B, H, W, 32 + heads * 128)).astype(np.float32)
    x[..., :16] = 3.0e4
    x[..., -16:] = -3.0e4
    qk = x[..., A_IN_OFF:A_IN_OFF + heads * 64]
    if kind == "pm80":                  # logits = q . k * 32^-1/2 spread over +-80: e^80 overflows fp32 without the running maximum
        qk *= np.float32(np.sqrt(80.0 / 3.0))            # per-logit std 80 / 3
    elif kind == "equal":               # q = 0: every logit 0, every softmax row uniform
        x[..., A_IN_OFF:A_IN_OFF + heads * 32] = 0.0
    x[..., A_IN_OFF + heads * 64:A_IN_OFF + heads * 128] *= np.float32(4.0)
    return x


def _attn_want(xh, heads, dt):
    B, H, W, _ = xh.shape
    t = torch.from_numpy(xh[..., A_IN_OFF:A_IN_OFF + heads * 128]).to(dt).reshape(B, H * W, heads * 128).permute(0, 2, 1)
    q = t[:, :heads * 32].reshape(B, heads, 32, H * W)
    k = t[:, heads * 32:heads * 64].reshape(B, heads, 32, H * W)
    v = t[:, heads * 64:].reshape(B, heads, 64, H * W)
    if dt == torch.float64 and q.abs().max() > 0:
        logits = (q.transpose(-2, -1) @ k) * 32 ** -0.5
        _attn_want.logit_range = float(logits.abs().max())
    y = psa_attention(q, k, v, 32 ** -0.5)                     # (B, heads, 64, N)
    return y.reshape(B, heads * 64, H * W).permute(0, 2, 1).reshape(B, H, W, heads * 64).numpy()


def _attn_case(eng, dtype, heads, N, kind="normal"):
    B = 2
    x = _attn_input(heads, B, N, kind, seed=N * 7 + heads)
    g, in_w, out_w = _attn_graph(dtype, heads)
    y, ovf = _run(eng, g, x, replay_after_fill=True)
    assert not ovf
    xh = held(dtype, x)
    want = _attn_want(xh, heads, torch.float64)
    w32 = _attn_want(xh, heads, torch.float32).astype(np.float64)
    got = y[..., A_OUT_OFF:A_OUT_OFF + heads * 64].astype(np.float64)
    assert np.isfinite(got).all()
    err, floor = float(np.abs(got - want).max()), float(np.abs(w32 - want).max())
    tag = f"attention {dtype} heads={heads} N={N} {kind}"
    record(tag, {"linf_engine_vs_fp64": err, "linf_fp32_torch_vs_fp64": floor})
    print(f"{tag}: engine {err:.3e}, fp32 torch {floor:.3e}")
    assert err <= 4 * floor, f"{tag}: L-inf {err:.3e} > 4 x {floor:.3e} (the fp32 torch evaluation of the same formula)"
    keep = np.ones(out_w, bool)
    keep[A_OUT_OFF:A_OUT_OFF + heads * 64] = False
    assert np.array_equal(y[..., keep], np.broadcast_to(sentinel(out_w)[keep], y[..., keep].shape)), "neighbouring channels touched"
    # the same image alone and as the second of a batch of two: the same bits
    y1, _ = _run(eng, g, x[1:2])
    assert np.array_equal(y1[0].view(np.uint32), y[1].view(np.uint32)), f"{tag}: batch 1 and batch 2 differ"
    return y


@pytest.mark.parametrize("dtype", ["f32", "h2"])
@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("N", list(TOKENS))
def test_attention_within_4x_the_fp32_formula(gpu_engine, dtype, heads, N):
    _attn_case(gpu_engine, dtype, heads, N)


@pytest.mark.parametrize("dtype", ["f32", "h2"])
def test_attention_logits_of_plus_minus_80(gpu_engine, dtype):
    _attn_case(gpu_engine, dtype, 2, 240, "pm80")
    assert _attn_want.logit_range > 80.0, _attn_want.logit_range


@pytest.mark.parametrize("dtype", ["f32", "h2"])
def test_attention_all_logits_equal(gpu_engine, dtype):
    for N in (65, 240):
        _attn_case(gpu_engine, dtype, 2, N, "equal")
