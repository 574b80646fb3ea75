"""TEST INFRASTRUCTURE: graphs that read a level-1 map (the stem's output) back exactly, and the fp64 statement of the stem.

The stem output cannot be read through the C-ABI directly: ``pa_yolo_read_head`` returns the level-3 head maps only.  So a probe
graph puts a head behind the stem that changes nothing: stride-2 3x3 convs with ONE-HOT weights (``ACT_NONE``, zero bias).  Output
channel ``q cin + ch`` of such a conv selects tap (ky, kx) = ``TAPS[q]`` of input channel ``ch`` — input pixel (2 oy + q // 2,
2 ox + q % 2): a pixel-unshuffle.  Two of them carry a level-1 map of c channels into 16 c channels of the level-3 head buffer
(one, behind a layer 1 of 2 c channels, into 8 c), at channel offset ``READOUT``.  Every product but one is an exact zero, so the
head holds the stored value itself: the fp32 word, the half, or h + m / 2048 of a pair.  Channels [0, READOUT) of level 3 and the
whole level-4 / level-5 head maps come from zero-weight convs with bias -30 in the class channel (no detection survives), fed by
16-channel scratch buffers (an h2 conv may not read an fp32 head map): every head byte is written by the graph.

``tests/test_stem_probe_host.py`` runs every probe graph through ``tests/graph_interp`` on the CPU; ``tests/test_gpu_stem.py``
runs them on the engine.  Never imported by the product package."""
from __future__ import annotations

import numpy as np

from padel_analytics_amd import graph as G

TAPS = ((1, 1), (1, 2), (2, 1), (2, 2))      # unshuffle quadrant q = 2 dy + dx <- tap (ky, kx) of a stride-2 3x3 with padding 1
READOUT = 80                                 # head channel where the readout starts (64 box + 1 class channels, rounded up to 16)
DTYPE = {"f32": G.DTYPE_F32, "f16": G.DTYPE_F16, "h2": G.DTYPE_H2}
U = 2.0 ** -24
K_STANDALONE, K_FUSED = 30, 36               # roundings of the two arithmetic orders (derivation: tests/test_gpu_stem.py)
SILU_ULPS = 2.0 * 3.402                      # MAX_FACTOR of tests/test_gpu_helpers.py x the fp32 formula's max (profiles/act_ulp_sweep.txt)
BIG_BIAS = 7.0e4                             # silu(7e4) = 7e4 > 65504: raises the overflow flag of an h2 graph


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def stem_weights(c: int, seed: int = 0):
    """(w (c, 3, 3, 3) as [cout][ky][kx][colour], b (c,)) fp32: N(0, 0.5) not fp16-exact; channel 1 all zero (output = silu(bias);
    the fused kernel's row scale takes its ex == 0 branch), channel 2 scaled by 1e-4, one weight of channel 3 set to 40; bias
    N(0, 1) pushed away from zero to |b| >= 0.25, so that silu(b) is visibly not 0."""
    rng = np.random.default_rng(7919 * c + seed)
    w = rng.normal(0.0, 0.5, (c, 3, 3, 3)).astype(np.float32)
    w[1] = 0.0
    w[2] *= np.float32(1e-4)
    w[3, 1, 2, 0] = 40.0
    b = rng.normal(0.0, 1.0, c).astype(np.float32)
    b = np.where(np.abs(b) < 0.25, np.copysign(np.float32(0.25), b), b).astype(np.float32)
    return w, b


def probe_frames(B: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """(B, h, w, 3) random bytes; image 0 carries a band of 255 along its top and left edges and a band of 0 along its bottom and
    right edges: the border outputs then carry the largest / the missing terms."""
    rng = np.random.default_rng(104729 * B + 31 * h + w + seed)
    f = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    f[0, :3], f[0, :, :3] = 255, 255
    f[0, -3:], f[0, :, -3:] = 0, 0
    return f


# ---- graph pieces -----------------------------------------------------------------------------------------------------------
def unshuffle_weight(cin: int) -> np.ndarray:
    w = np.zeros((4 * cin, cin, 3, 3), np.float32)
    for q, (ky, kx) in enumerate(TAPS):
        w[q * cin + np.arange(cin), np.arange(cin), ky, kx] = 1.0
    return w


def append_stem(g: G.Graph, w: np.ndarray, b: np.ndarray, dst) -> None:
    """The OP_STEM op exactly as ``graph.build_yolov8`` appends it: weights [cout][27] in (ky, kx, colour) order, bias, SiLU.
    ``w`` is [cout][ky][kx][colour] already; ``Graph.stem`` takes the checkpoint's [cout][colour][ky][kx]."""
    g.stem(np.asarray(w).transpose(0, 3, 1, 2), b, dst)


def _finish_heads(g: G.Graph, src, head3: int, width: int) -> None:
    """Everything of the three head maps that the readout does not write: zero-weight convs, bias -30 in the class channel."""
    z = lambda *s: np.zeros(s, np.float32)
    sw = g.padk(16)                                  # (fp16 graphs: a k-step is 32 channels, the scratch is written at that width)

    def bias(n):
        b = z(n)
        b[64] = -30.0
        return b
    prev = src
    for lvl in (3, 4, 5):
        s = g.buf(lvl, sw)
        g.conv(prev, (s, 0), z(sw, prev[2], 3, 3), z(sw), 3, 2, G.ACT_NONE)
        if lvl == 3:
            g.conv((s, 0, sw), (head3, 0), z(READOUT, sw, 1, 1), bias(READOUT), 1, 1, G.ACT_NONE)
            heads = [head3]
        else:
            hd = g.buf(lvl, width)
            g.conv((s, 0, sw), (hd, 0), z(width, sw, 1, 1), bias(width), 1, 1, G.ACT_NONE)
            heads.append(hd)
        prev = (s, 0, sw)
    g.head_buf = tuple(heads)


def standalone_graph(t: str, c: int, w, b, buf_width: int = 0, choff: int = 0) -> G.Graph:
    """stem -> level-1 buffer [choff, choff + c) (``buf_width`` channels wide, default c) -> two unshuffles -> head channels
    [READOUT, READOUT + 16 c).  The first unshuffle has 4 c outputs, never the 2 c of a layer 1 the fused kernel accepts."""
    g = G.Graph(task=G.TASK_DETECT, nc=1, dtype=DTYPE[t])
    l1 = g.buf(1, buf_width or c)
    if t == "f16" and (buf_width or c) > choff + c:
        # an fp16 conv reads whole 32-channel k-steps: the channels right of a 16-channel slice are read under zero weights, and no
        # fill of the arena makes them finite on fp16 graphs — a stem with zero weights and zero bias writes silu(0) = 0 there
        n = (buf_width or c) - (choff + c)
        append_stem(g, np.zeros((n, 3, 3, 3), np.float32), np.zeros(n, np.float32), (l1, choff + c))
    append_stem(g, w, b, (l1, choff))
    u1 = g.buf(2, 4 * c)
    g.conv((l1, choff, c), (u1, 0), unshuffle_weight(c), np.zeros(4 * c, np.float32), 3, 2, G.ACT_NONE)
    width = READOUT + 16 * c
    head3 = g.buf(3, width)
    g.conv((u1, 0, 4 * c), (head3, READOUT), unshuffle_weight(4 * c), np.zeros(16 * c, np.float32), 3, 2, G.ACT_NONE)
    _finish_heads(g, (u1, 0, 4 * c), head3, width)
    return g


def fused_graph(c: int, w, b, w1, b1, act1: int) -> G.Graph:
    """h2: stem -> c channels -> layer 1 (3x3 stride 2, exactly 2 c outputs: the shape ``stem_l1_h2`` takes) -> one unshuffle ->
    head channels [READOUT, READOUT + 8 c)."""
    g = G.Graph(task=G.TASK_DETECT, nc=1, dtype=G.DTYPE_H2)
    l1 = g.buf(1, c)
    append_stem(g, w, b, (l1, 0))
    y = g.buf(2, 2 * c)
    g.conv((l1, 0, c), (y, 0), w1, b1, 3, 2, act1)
    width = READOUT + 8 * c
    head3 = g.buf(3, width)
    g.conv((y, 0, 2 * c), (head3, READOUT), unshuffle_weight(2 * c), np.zeros(8 * c, np.float32), 3, 2, G.ACT_NONE)
    _finish_heads(g, (y, 0, 2 * c), head3, width)
    return g


N_PASSES = 5


def pass_pairs(c: int, p: int) -> np.ndarray:
    """The 2 c (tap, channel) pairs that pass ``p`` reads, as indices tap * c + channel into the 9 c pairs; the last pass is padded
    with repeats of the first pairs."""
    return (p * 2 * c + np.arange(2 * c)) % (9 * c)


def readout_weight(c: int, p: int) -> np.ndarray:
    """Layer-1 weights of readout pass ``p``: row r is one-hot at tap (ky, kx) = divmod(pair // c, 3), channel pair % c."""
    pairs = pass_pairs(c, p)
    w1 = np.zeros((2 * c, c, 3, 3), np.float32)
    w1[np.arange(2 * c), pairs % c, (pairs // c) // 3, (pairs // c) % 3] = 1.0
    return w1


def fused_readout_graph(c: int, w, b, p: int) -> G.Graph:
    g = fused_graph(c, w, b, readout_weight(c, p), np.zeros(2 * c, np.float32), G.ACT_NONE)
    assert g.ops[1]["flags"] & G.FLAG_W_SINGLE, "one-hot weights are fp16 numbers"
    return g


def premise_graph(t: str, cin: int, levels: int) -> G.Graph:
    """The unshuffle convs alone, as a TASK_TRACKNET graph over a caller-supplied level-0 array."""
    g = G.Graph(task=G.TASK_TRACKNET, dtype=DTYPE[t])
    cur = g.buf(0, cin)
    for lvl in range(1, levels + 1):
        nxt = g.buf(lvl, 4 * cin)
        g.conv((cur, 0, cin), (nxt, 0), unshuffle_weight(cin), np.zeros(4 * cin, np.float32), 3, 2, G.ACT_NONE)
        cur, cin = nxt, 4 * cin
    g.head_buf = (cur, -1, -1)
    return g


# ---- decode -----------------------------------------------------------------------------------------------------------------
def unshuffle_decode(y: np.ndarray, levels: int) -> np.ndarray:
    """(B, H, W, 4^levels c) NHWC, the output of ``levels`` chained unshuffle convs -> the (B, 2^levels H, 2^levels W, c) map
    they read."""
    for _ in range(levels):
        B, H, W, C = y.shape
        y = y.reshape(B, H, W, 2, 2, C // 4).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, C // 4)
    return y


def decode_level1(head: np.ndarray) -> np.ndarray:
    """Level-3 head map of a ``standalone_graph`` -> the level-1 map (B, H / 2, W / 2, c)."""
    return unshuffle_decode(head[..., READOUT:], 2)


def decode_layer1(head: np.ndarray) -> np.ndarray:
    """Level-3 head map of a ``fused_graph`` -> layer 1's output (B, H / 4, W / 4, 2 c)."""
    return unshuffle_decode(head[..., READOUT:], 1)


class Observations:
    """What the readout passes of one (weights, frames) saw of the fused kernel's stem planes: ``obs[tap]`` (B, Ho, Wo, c) is the
    value layer 1's tap (ky, kx) = divmod(tap, 3) read at every output pixel — stem element (2 oy - 1 + ky, 2 ox - 1 + kx), or
    layer 1's zero padding where that lies at row / column -1."""

    def __init__(self, c: int):
        self.c = c
        self.obs = None
        self.repeat_mismatch = 0

    def add_pass(self, p: int, l1: np.ndarray) -> None:
        c = self.c
        if self.obs is None:
            self.obs = np.full((9,) + l1.shape[:3] + (c,), np.nan, np.float32)
            self.have = np.zeros((9, c), bool)
        for r, pair in enumerate(pass_pairs(c, p)):
            t, ch = divmod(int(pair), c)
            if self.have[t, ch]:              # a repeat of the padded last pass: the same element read again
                self.repeat_mismatch += int((self.obs[t, ..., ch].view(np.uint32) != np.ascontiguousarray(l1[..., r]).view(np.uint32)).sum())
            else:
                self.obs[t, ..., ch] = l1[..., r]
                self.have[t, ch] = True

    def padding(self):
        """[(tap, values that must be exactly zero)]: the observations of stem row -1 and stem column -1."""
        assert self.have.all()
        out = []
        for t in range(9):
            ky, kx = divmod(t, 3)
            if ky == 0:
                out.append((t, self.obs[t][:, 0]))
            if kx == 0:
                out.append((t, self.obs[t][:, :, 0]))
        return out

    def reassemble(self):
        """-> (stem map (B, 2 Ho, 2 Wo, c) fp32, number of observations of an element that differ BITWISE from its first one,
        number of elements seen more than once).  Padding observations are left out."""
        assert self.have.all()
        _, B, Ho, Wo, c = self.obs.shape
        stem = np.full((B, 2 * Ho, 2 * Wo, c), np.nan, np.float32)
        seen = np.zeros((2 * Ho, 2 * Wo), np.int32)
        differ = 0
        for t in range(9):
            ky, kx = divmod(t, 3)
            oy = np.arange(1 if ky == 0 else 0, Ho)
            ox = np.arange(1 if kx == 0 else 0, Wo)
            sy, sx = 2 * oy - 1 + ky, 2 * ox - 1 + kx
            val = np.ascontiguousarray(self.obs[t][:, oy][:, :, ox])
            cur = stem[:, sy[:, None], sx[None, :]]
            first = (seen[np.ix_(sy, sx)] == 0)[None, :, :, None]
            differ += int(((cur.view(np.uint32) != val.view(np.uint32)) & ~first).sum())
            stem[:, sy[:, None], sx[None, :]] = np.where(first, val, cur)
            seen[np.ix_(sy, sx)] += 1
        assert (seen >= 1).all()
        return stem, differ, int((seen > 1).sum()) * B * c


# ---- truth and bound --------------------------------------------------------------------------------------------------------
def _patches(x: np.ndarray):
    """x (B, H, W, 3) -> [(ky, kx, the (B, H / 2, W / 2, 3) inputs under that tap, zero outside the image)]."""
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return [(ky, kx, xp[:, ky:ky + H:2, kx:kx + W:2]) for ky in range(3) for kx in range(3)]


def stem_truth(netin: np.ndarray, w: np.ndarray, b: np.ndarray):
    """fp64 on the exact bytes ``netin`` (B, H, W, >= 3) u8: x = u8 / 255, t = sum_k w_k x_k + b over the 27 taps (zero outside the
    image), v = t / (1 + exp(-t)); S = sum_k |w_k| x_k + |b|, the scale of the rounding error.  -> (v, S), (B, H / 2, W / 2, c)."""
    x = netin[..., :3].astype(np.float64) / 255.0
    w64 = w.astype(np.float64)
    t = np.zeros(x.shape[:1] + (x.shape[1] // 2, x.shape[2] // 2, w.shape[0]))
    S = np.zeros_like(t)
    for ky, kx, px in _patches(x):
        t += px @ w64[:, ky, kx].T
        S += px @ np.abs(w64[:, ky, kx]).T
    t += b.astype(np.float64)
    S += np.abs(b.astype(np.float64))
    with np.errstate(over="ignore"):
        v = t / (1.0 + np.exp(-t))
    return v, S


def ulp32(v: np.ndarray) -> np.ndarray:
    """One unit in the last place of the fp32 result, taken at max(|v|, 2^-126) as ``test_gpu_helpers.ulp_error`` does."""
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


def store_term(t: str, v: np.ndarray) -> np.ndarray:
    if t == "f16":
        return 2.0 ** -11 * np.abs(v) + 2.0 ** -25
    if t == "h2":
        return 2.0 ** -22 * np.abs(v)
    return np.zeros_like(v)


def bound(t: str, K: int, v: np.ndarray, S: np.ndarray) -> np.ndarray:
    """|got - v| <= 1.1 K u S + SILU_ULPS ulp32(v) + store(v); 1.1: the largest |silu'| is 1.0998."""
    return 1.1 * K * U * S + SILU_ULPS * ulp32(v) + store_term(t, v)


# ---- the fp16 conv kernels (tests/test_gpu_f16_epilogue.py): one fp32 accumulation over K exact products, bias, activation -----
ACT_ULPS = {G.ACT_NONE: 0.0, G.ACT_RELU: 0.0, G.ACT_LEAKY: 1.0, G.ACT_SILU: SILU_ULPS, G.ACT_SIGMOID: SILU_ULPS}
F16_MAX = 65504.0


def ulp16(v: np.ndarray) -> np.ndarray:
    """Spacing of the fp16 numbers at |v|: 2^(e - 11) for 2^(e - 1) <= |v| < 2^e, 2^-24 below 2^-14 (gradual underflow)."""
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -14))
    return np.ldexp(1.0, e - 11)


def conv16_bound(K: int, act: int, v: np.ndarray, S: np.ndarray) -> np.ndarray:
    """fp32-head output of an fp16 conv: |y32 - v| <= 1.1 K u S + ACT_ULPS ulp32(v).  Products of two halves are exact in fp32, so
    the K = cin k k + 1 roundings are those of the additions (bias included); 1.1 bounds the slope of every activation."""
    return 1.1 * K * U * S + ACT_ULPS[act] * ulp32(v)


def conv16_bound_f16(K: int, act: int, v: np.ndarray, S: np.ndarray, res=None) -> np.ndarray:
    """The same result stored as a half: ``v`` already includes the residual ``res`` (the stored halves, exact), whose fp32
    addition costs one more ulp32; then half a unit of the fp16 spacing at the largest value the store may have seen."""
    b = conv16_bound(K, act, v if res is None else v - res, S)
    if res is not None:
        b = b + ulp32(v)
    return b + 0.5 * ulp16(np.abs(v) + b)


def storable(t: str, got: np.ndarray) -> bool:
    """``got`` holds only values the storage type can hold."""
    if t == "f16":
        return bool(np.array_equal(got, got.astype(np.float16).astype(np.float32)))
    if t == "h2":
        return bool(np.array_equal(G.h2_value(*G.h2_split(got)), got))
    return True


def check(name: str, t: str, K: int, got: np.ndarray, v: np.ndarray, S: np.ndarray) -> float:
    """Asserts the bound element-wise; the message names image, channel, (y, x) and the ratio to the bound.  -> worst
    |got - v| / (u S)."""
    assert got.shape == v.shape, (got.shape, v.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    err = np.abs(got.astype(np.float64) - v)
    ratio = err / bound(t, K, v, S)
    n, y, x, ch = (int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape))
    assert ratio[n, y, x, ch] <= 1.0, (f"{name}: image {n} channel {ch} (y, x) = ({y}, {x}): got {float(got[n, y, x, ch])!r}, fp64 "
                                       f"{float(v[n, y, x, ch])!r}, error {ratio[n, y, x, ch]:.3g} x the bound ({int((ratio > 1).sum())} elements beyond it)")
    assert storable(t, got), f"{name}: a value the {t} storage cannot hold"
    return float((err / (U * S)).max())


# ---- fp32 emulations of the two arithmetic orders (numpy; the order within a matrix instruction is not modelled) ----------------
def _silu32(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (x / (np.float32(1.0) + np.exp(-x))).astype(np.float32)


def _stored(t: str, v: np.ndarray) -> np.ndarray:
    if t == "f16":
        return v.astype(np.float16).astype(np.float32)
    if t == "h2":
        return G.h2_value(*G.h2_split(v))
    return v


def emulate_standalone(netin: np.ndarray, w: np.ndarray, b: np.ndarray, t: str = "f32") -> np.ndarray:
    """``stem_mfma_kernel``'s order: sum_k w_k fl(u8 / 255) accumulated in fp32 over k = (ky, kx, colour), + bias, SiLU, store."""
    x = (netin[..., :3].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    acc = None
    for ky, kx, px in _patches(x):
        for col in range(3):
            prod = (px[..., col:col + 1] * w[None, None, None, :, ky, kx, col]).astype(np.float32)
            acc = prod if acc is None else (acc + prod).astype(np.float32)
    return _stored(t, _silu32((acc + b).astype(np.float32)))


def emulate_fused(netin: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The stem phase of ``stem_l1_h2_kernel``: w / 255 scaled per row by a power of two into [2^12, 2^13), split into an fp16 pair;
    main and correction sums over the exact bytes in fp32; fmaf(fmaf(cross, 1 / 2048, main), 1 / scale, bias); SiLU; pair store."""
    c = w.shape[0]
    wv = (w.reshape(c, 27) / np.float32(255.0)).astype(np.float32)
    mx = np.abs(wv).max(axis=1)
    ex = (mx.view(np.uint32) >> 23) & 255
    e = np.where(ex == 0, 0, np.clip(139 - ex.astype(np.int64), -100, 100))
    sc, isc = np.ldexp(np.float32(1.0), e).astype(np.float32), np.ldexp(np.float32(1.0), -e).astype(np.float32)
    xs = (wv * sc[:, None]).astype(np.float32)
    hh = xs.astype(np.float16)
    mm = ((xs - hh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    hh, mm = hh.astype(np.float32).reshape(c, 3, 3, 3), mm.astype(np.float32).reshape(c, 3, 3, 3)
    main = cross = None
    for ky, kx, px in _patches(netin[..., :3].astype(np.float32)):
        for col in range(3):
            pm = (px[..., col:col + 1] * hh[None, None, None, :, ky, kx, col]).astype(np.float32)
            pc = (px[..., col:col + 1] * mm[None, None, None, :, ky, kx, col]).astype(np.float32)
            main = pm if main is None else (main + pm).astype(np.float32)
            cross = pc if cross is None else (cross + pc).astype(np.float32)
    inner = (cross.astype(np.float64) / 2048.0 + main.astype(np.float64)).astype(np.float32)        # fmaf: one rounding
    x = (inner.astype(np.float64) * isc.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    return _stored("h2", _silu32(x))


def layer1_weights(c: int, seed: int = 0):
    """Random layer-1 weights (2 c, c, 3, 3) and bias, fp32 (not fp16-exact)."""
    rng = np.random.default_rng(15485863 + 613 * c + seed)
    w1 = rng.normal(0.0, (2.0 / (9 * c)) ** 0.5, (2 * c, c, 3, 3)).astype(np.float32)
    b1 = rng.normal(0.0, 0.5, 2 * c).astype(np.float32)
    return w1, b1


def layer1_truth(stem: np.ndarray, w1: np.ndarray, b1: np.ndarray) -> np.ndarray:
    """fp64 Conv(c, 2 c, 3, 2, padding 1) + SiLU over ``stem`` (B, H, W, c) -> (B, H / 2, W / 2, 2 c)."""
    B, H, W, c = stem.shape
    xp = np.pad(stem.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    t = np.zeros((B, H // 2, W // 2, w1.shape[0]))
    for ky in range(3):
        for kx in range(3):
            t += xp[:, ky:ky + H:2, kx:kx + W:2] @ w1[:, :, ky, kx].astype(np.float64).T
    t += b1.astype(np.float64)
    with np.errstate(over="ignore"):
        return t / (1.0 + np.exp(-t))
