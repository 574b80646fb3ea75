"""Per-tile tests of the fp16 conv stores (csrc/f16_epilogue.h, shared by conv_tap16.hip and conv_patch16.hip): exact halves, the
clamp, the fp32 head.

The sweep of tests/test_gpu_fp16.py holds every tile to ONE tolerance, 1.5e-3 of the largest output: a store that rounds the wrong
way, flushes small results or drops the low bits of a dword passes it, and the fp32-head instantiation only ever ran as an identity
1x1.  Here the conv under test runs twice per native (tile, case) on the same fp16-rounded operands:

  head="f32"  it writes the fp32 head buffer itself (``f16_epilogue_fast<.., F32OUT>`` on whole tiles, the element-wise path with
              ``out_f32`` elsewhere): ``y32``;
  head="f16"  [1x1 -> residual buffer], a per-channel sentinel fill of a non-head buffer, the conv under test into it, an identity
              1x1 into the fp32 head: ``y16``.  The readback is exact for every finite half (``test_identity_readback...``).

What launched is checked against tests/tile_support.py in every run; ``TS.f16_store_paths`` names the store path, and
tests/test_tile_coverage.py proves from that table that every tile id meets every path its fragment count allows.

A. exact store: both instantiations compute act(acc + bias) with the same operations, so y16 == RN16(clip(y32, +-65504)) with
   numpy's ``astype(float16)`` (round to nearest even, gradual underflow), as bits after + 0.0 — no tolerance.  With a residual
   the kernel adds the stored half r16 (read back in a run of its own) in fp32: t = fl32(y32 + r16).  hipcc contracts by default,
   so the activation's last multiply and that add may be ONE fma, whose result is t or a neighbour of t: y16 must be RN16(clip(t'))
   for a t' in {t - ulp32(t), t, t + ulp32(t)}, and where y16 != RN16(clip(t)) the three candidates must differ (the set is
   computed on the host and is below 1 % of the elements: tests/test_f16_epilogue_host.py).  Channels a partial fragment masks out
   keep the sentinel; zero rows up to ``out_width`` hold RN16(act(0)).
B. element-wise against fp64 (tests/stem_probe.py::conv16_bound): |y32 - v| <= 1.1 K u S + ACT_ULPS ulp32(v) with K = cin k k + 1,
   u = 2^-24, S = sum |x||w| + |b|; for halves + 0.5 ulp16(|v| + bound) and, with a residual, ulp32 of the sum.
C. y32 bitwise equal across the tiles of an accumulation family (tap16 / tap16d; p16 / p16q) — before any fp16 rounding.
D. the clamp: planted outputs of +1e5 and -1e5 are stored as +-65504 exactly, nothing is infinite, nothing else changes; the
   fp32 head holds the unclamped value; +-65504 is a legal operand of the next conv.
E. small magnitudes: subnormal halves as results and as operands, A and B unchanged.

Every figure is printed; where ``PADEL_REPORT_DIR`` names a directory the lines are appended to ``f16_epilogue.txt`` there
(profiles/f16_epilogue.txt is a copy of one such run)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import engine as E, graph as G
from tests import stem_probe as P, tile_support as TS
from tests.test_gpu_conv import ACT_FN, _launched
from tests.test_gpu_fp16 import PATCH_VARIANTS, VARIANTS

pytestmark = pytest.mark.gpu

TILES = VARIANTS + PATCH_VARIANTS
FAMILIES = ("tap16", "tap16d", "p16", "p16q")

# (B, H, W, cin, cout, k, stride, act, residual).  cout 384 = 3 x 128 = 4 x 96 = 6 x 64 = 8 x 48 = 12 x 32 = 24 x 16 and M = 512 on
# 16 x 32 maps: whole channel tiles, whole pixel tiles and whole 8 x 16 / 16 x 16 patches on every id (the 16-byte paths); 39 and 80
# channels and odd maps: partial tiles, partial fragments (element-wise).
CASES = [
    (1, 16, 32, 32, 384, 3, 1, G.ACT_RELU, False),          # 0  stride-1 3x3 (all four families)
    (1, 16, 32, 64, 384, 3, 1, G.ACT_SILU, True),           # 1
    (1, 18, 20, 64, 39, 3, 1, G.ACT_NONE, True),            # 2
    (3, 17, 23, 96, 80, 3, 1, G.ACT_LEAKY, False),          # 3
    (1, 16, 32, 64, 384, 1, 1, G.ACT_SILU, False),          # 4  1x1 (tap16 / tap16d)
    (1, 16, 32, 96, 384, 1, 1, G.ACT_NONE, True),           # 5
    (1, 9, 13, 96, 39, 1, 1, G.ACT_SIGMOID, True),          # 6
    (2, 32, 32, 32, 384, 3, 2, G.ACT_RELU, False),          # 7  stride-2 3x3
    (2, 32, 32, 64, 384, 3, 2, G.ACT_SILU, True),           # 8
    (1, 18, 22, 64, 39, 3, 2, G.ACT_SILU, False),           # 9
    (1, 8, 16, 768, 256, 3, 1, G.ACT_RELU, False),          # 10 TrackNet layers at 8 x 16: up_block_1.conv_1 (K = 6912)
    (1, 8, 16, 384, 128, 3, 1, G.ACT_RELU, False),          # 11 up_block_2.conv_1
    (1, 8, 16, 32, 64, 3, 1, G.ACT_RELU, False),            # 12 down_block_1.conv_1
    (1, 8, 16, 64, 8, 1, 1, G.ACT_SIGMOID, False),          # 13 the predictor: an fp32 head of 8 channels at pixel stride 8
    (1, 9, 13, 64, 80, 1, 1, G.ACT_LEAKY, False),           # 14 a partial-tile 1x1 without sigmoid (the clamp's element-wise path)
]
# the clamp: per kernel group one case of whole tiles (16-byte stores) and one of partial tiles (element-wise); no sigmoid.  A
# negative value of 1e5 exists behind ACT_NONE only (cases 2 and 5): the others plant the positive one.
CLAMP_CASES = (0, 2, 5, 14, 7, 9)
# small magnitudes: per family one tile on a whole-tile case and one on a partial-tile case — (case, tiles)
SMALL_RUNS = ((1, (20, 60, 303, 323)), (3, (7, 47, 306, 326)))
# operand scales (x, w): the three of tests/test_gpu_h2.py::test_h2_dynamic_range — x subnormal as a half at 3e-6, w at 1e-5 — and,
# because 3e-6 x 1e-3 puts every result below 2^-25 (all stored halves are zero) and 200 x 1e-5 every result in the normal range,
# the same subnormal operands against a partner that puts the RESULTS into the subnormal range (2^-24, 2^-14).  ``sub``: at least a
# quarter of the fp64 results lie there (asserted on the reference, tests/test_f16_epilogue_host.py).
SMALL_SCALES = [(1e-4, 1.0, True), (3e-6, 1e-3, False), (200.0, 1e-5, False), (3e-6, 8.0, True), (1.0, 1e-5, True)]


def _report(line):
    print(line)
    out = os.environ.get("PADEL_REPORT_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "f16_epilogue.txt"), "a") as f:
            f.write(line + "\n")


def native_tiles(case, group=None):
    """Tile ids that run ``case`` under their own id; ``group``: "tap" (tap16 + tap16d: one accumulation order) or "patch"."""
    ts = [t for t in TILES if TS.native("f16", t, case)]
    if group is not None:
        ts = [t for t in ts if (t >= 300) == (group == "patch")]
    return ts


def groups(case):
    return ("tap", "patch") if case[5] == 3 and case[6] == 1 else ("tap",)


def nores(case):
    return case[:8] + (False,)


def head_runs(case):
    """The two runs of a (tile, case): [(head, case as run)] — the fp32-head run never carries the residual."""
    return [("f32", nores(case)), ("f16", case)]


# ---- operands and the fp64 reference ------------------------------------------------------------------------------------------
def data(case, xs=1.0, ws=1.0):
    """fp16-rounded x, w, wr (w and wr as fp32 arrays holding halves), fp32 bias."""
    B, H, W, cin, cout, k, s, act, use_res = case
    rng = np.random.default_rng(cin * 131 + cout * 7 + k * 3 + s)
    h = lambda a: a.astype(np.float16)
    return dict(x=h(rng.normal(0, 1, (B, H, W, cin)) * xs),
                w=h(rng.normal(0, (2.0 / (cin * k * k)) ** 0.5, (cout, cin, k, k)) * ws).astype(np.float32),
                b=(rng.normal(0, 0.5, cout) * xs * ws).astype(np.float32),
                wr=h(rng.normal(0, (1.0 / cin) ** 0.5, (cout, cin, 1, 1)) * ws).astype(np.float32))


def reference(case, d):
    """fp64 on the fp16 operands -> dict(v = act(conv + b), S = conv(|x|, |w|) + |b|, r = the residual conv (fp64, unrounded) or
    None), each (B, Ho, Wo, cout)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    xt = torch.from_numpy(d["x"].astype(np.float64)).permute(0, 3, 1, 2)
    w, b = torch.from_numpy(d["w"]).double(), torch.from_numpy(d["b"]).double()
    nhwc = lambda t: np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())
    v = nhwc(ACT_FN[act](F.conv2d(xt, w, b, stride=s, padding=k // 2)))
    S = nhwc(F.conv2d(xt.abs(), w.abs(), b.abs(), stride=s, padding=k // 2))
    r = nhwc(F.conv2d(xt, torch.from_numpy(d["wr"]).double(), stride=s)) if use_res else None
    return dict(v=v, S=S, r=r)


@functools.lru_cache(maxsize=None)
def case_data(i, xs=1.0, ws=1.0):
    d = data(CASES[i], xs, ws)
    return d, reference(CASES[i], d)


def K_of(case):
    return case[3] * case[5] * case[5] + 1


def rn16(a):
    """What a correct store leaves, as the fp32 the identity readback returns: clamp, round to nearest even with gradual underflow
    (numpy's conversion), and + 0.0 (a stored -0 comes out of the accumulator as +0)."""
    a = np.clip(np.asarray(a, np.float32), np.float32(-P.F16_MAX), np.float32(P.F16_MAX))
    return a.astype(np.float16).astype(np.float32) + np.float32(0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def residual_candidates(y32, r16):
    """-> (RN16(clip(t)), the mask of elements whose three candidates RN16(clip(t - ulp)), RN16(clip(t)), RN16(clip(t + ulp))
    differ, [the three candidates]); t = fl32(y32 + r16)."""
    t = (np.asarray(y32, np.float32) + np.asarray(r16, np.float32)).astype(np.float32)
    u = P.ulp32(t)
    cands = [rn16((t.astype(np.float64) + sgn * u).astype(np.float32)) for sgn in (0.0, -1.0, 1.0)]
    adjacent = (bits(cands[1]) != bits(cands[0])) | (bits(cands[2]) != bits(cands[0]))
    return cands[0], adjacent, cands


def sentinel(n):
    return (-100.0 - 0.25 * np.arange(n)).astype(np.float32)          # fp16 numbers


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def build_graph(case, d, head="f16", out_width=None):
    """head="f16": [1x1 -> residual buffer], sentinel fill of the non-head buffer S (1x1, zero weights, bias = sentinel), the conv
    under test -> S, identity 1x1 S -> fp32 head.  head="f32": the conv under test writes the head buffer itself (cout channels wide
    where that is a multiple of 4, as TrackNet's 8-channel head; else padded to 16).  head="res": the residual buffer alone behind
    the identity.  Returns (graph, index of the conv under test among the conv ops)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    z = lambda *shape: np.zeros(shape, np.float32)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F16)
    b0 = g.buf(0, cin)
    lvl = 1 if s == 2 else 0
    wd = g.padk(cout)
    eye = np.eye(wd, dtype=np.float32)[:, :, None, None]
    res = None
    if use_res or head == "res":
        rb = g.buf(lvl, wd)
        g.conv((b0, 0, cin), (rb, 0), d["wr"], z(cout), 1, s, G.ACT_NONE, out_width=wd)
        res = (rb, 0)
    if head == "res":
        hd = g.buf(lvl, wd)
        g.conv((rb, 0, wd), (hd, 0), eye, z(wd), 1, 1, G.ACT_NONE)
        g.head_buf = (hd, -1, -1)
        return g, -2
    if head == "f32":
        assert out_width is None
        b1 = g.buf(lvl, cout if cout % 4 == 0 else G.pad16(cout))
        g.conv((b0, 0, cin), (b1, 0), d["w"], d["b"], k, s, act, res=res)
        g.head_buf = (b1, -1, -1)
        return g, -1
    assert head == "f16", head
    S = g.buf(lvl, wd)
    g.conv((b0, 0, cin), (S, 0), z(wd, cin, 1, 1), sentinel(wd), 1, s, G.ACT_NONE)
    g.conv((b0, 0, cin), (S, 0), d["w"], d["b"], k, s, act, res=res, out_width=out_width)
    hd = g.buf(lvl, wd)
    g.conv((S, 0, wd), (hd, 0), eye, z(wd), 1, 1, G.ACT_NONE)
    g.head_buf = (hd, -1, -1)
    return g, -2


def run(eng, case, d, tile, head="f16", x=None, out_width=None):
    """One forced run (``tile`` = -1: the engine's own choice); what launched must be what tests/tile_support.py says."""
    g, which = build_graph(case, d, head, out_width)
    eng.set_tuning(variant=tile)
    eng.set_profiling(True)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(case[0])
        y = m.tracknet_infer(d["x"] if x is None else x)
        got = _launched(m, which)
    finally:
        eng.set_profiling(False)
        m.close()
    if tile >= 0 and head != "res":
        want = TS.expected("f16", tile, case)
        assert got == want, f"requested {tile}, launched {got[0]}/{got[1]}; tests/tile_support.py says {want[0]}/{want[1]}"
    else:
        assert got[0] in FAMILIES, got
    return y


def first_bad(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def check_bound(name, got, v, bound, S):
    """|got - v| <= bound element-wise -> worst |got - v| / (u S)."""
    assert got.shape == v.shape, (got.shape, v.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    err = np.abs(got.astype(np.float64) - v)
    ratio = err / bound
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"{name}: worst error {float(ratio[at]):.3f} x the bound")
    assert ratio[at] <= 1.0, (f"{name}: (n, y, x, c) = {tuple(int(i) for i in at)}: got {float(got[at])!r}, fp64 {float(v[at])!r}, error "
                              f"{ratio[at]:.3g} x the bound ({int((ratio > 1).sum())} elements beyond it)")
    return float((err / (P.U * S)).max())


def check_exact_and_bound(eng, case, d, ref, tile, stats, r16=None, check_width=True):
    """Statements A and B on one native (tile, case).  -> y32 (B, Ho, Wo, cout)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    K = K_of(case)
    fam = TS.expected("f16", tile, case)[0]
    name = f"{fam} tile {tile} {case}"
    y32 = run(eng, nores(case), d, tile, head="f32")[..., :cout]
    stats["f32", fam] = max(stats.get(("f32", fam), 0.0), check_bound(name + " fp32 head", y32, ref["v"], P.conv16_bound(K, act, ref["v"], ref["S"]), ref["S"]))
    y = run(eng, case, d, tile)
    wd = y.shape[-1]
    keep = y[..., cout:] == np.broadcast_to(sentinel(wd)[cout:], y[..., cout:].shape)
    assert keep.all(), f"{name}: wrote beyond its {cout} channels (channels {sorted(set(int(c) + cout for c in np.argwhere(~keep)[:, -1]))[:8]})"
    y16 = y[..., :cout]
    assert np.isfinite(y16).all(), f"{name}: non-finite halves"
    if use_res:
        want, adjacent, cands = residual_candidates(y32, r16)
        ok = (bits(y16) == bits(cands[0])) | (bits(y16) == bits(cands[1])) | (bits(y16) == bits(cands[2]))
        assert ok.all(), (f"{name}: {int((~ok).sum())} halves are none of RN16(t - ulp), RN16(t), RN16(t + ulp), first at (n, y, x, c) = {first_bad(~ok)}: "
                          f"stored {y16[first_bad(~ok)]!r}, y32 {y32[first_bad(~ok)]!r}, residual {r16[first_bad(~ok)]!r}")
        mism = bits(y16) != bits(want)
        stray = mism & ~adjacent
        assert not stray.any(), f"{name}: {int(stray.sum())} halves differ from RN16(y32 + r16) where one ulp32 cannot change the half, first at {first_bad(stray)}"
        stats["ties"] = stats.get("ties", 0) + int(mism.sum())
        stats["adjacent"] = stats.get("adjacent", 0) + int(adjacent.sum())
        stats["elements"] = stats.get("elements", 0) + mism.size
        v16 = ref["v"] + r16.astype(np.float64)
        bound16 = P.conv16_bound_f16(K, act, v16, ref["S"], res=r16.astype(np.float64))
    else:
        want = rn16(y32)
        bad = bits(y16) != bits(want)
        assert not bad.any(), (f"{name}: {int(bad.sum())} stored halves differ from RN16(clip(y32)) of the same tile's fp32 output, first at (n, y, x, c) = "
                               f"{first_bad(bad)}: stored {y16[first_bad(bad)]!r}, y32 {y32[first_bad(bad)]!r}, RN16 {want[first_bad(bad)]!r}")
        v16, bound16 = ref["v"], P.conv16_bound_f16(K, act, ref["v"], ref["S"])
    stats["f16", fam] = max(stats.get(("f16", fam), 0.0), check_bound(name + " fp16 store", y16, v16, bound16, ref["S"]))
    if check_width and cout % 16:
        # zero rows up to out_width: the kernel writes act(0 + 0) [+ the residual buffer's own zero rows] there, the sentinel beyond
        ow = G.pad16(cout)
        yw = run(eng, case, d, tile, out_width=ow)
        assert np.array_equal(bits(yw[..., :cout]), bits(y16)), f"{name}: out_width {ow} changes the {cout} real channels"
        a0 = rn16(np.float32(ACT_FN[act](torch.zeros(1, dtype=torch.float64)).item()))
        assert (yw[..., cout:ow] == a0).all(), f"{name}: zero rows hold {np.unique(yw[..., cout:ow])[:4]}, RN16(act(0)) = {a0}"
        assert np.array_equal(yw[..., ow:], np.broadcast_to(sentinel(wd)[ow:], yw[..., ow:].shape)), f"{name}: wrote beyond out_width {ow}"
    return y32


def summary(stats):
    s = "; ".join(f"{fam} {head} head {stats[head, fam]:.3f}" for head in ("f32", "f16") for fam in FAMILIES if (head, fam) in stats)
    if "elements" in stats:
        s += f"; residual: {stats['ties']} halves of {stats['elements']} are RN16 of a neighbour of fl32(y32 + r16) ({stats['adjacent']} tie-adjacent)"
    return "worst |got - v| / (u S): " + s


# ---- premise --------------------------------------------------------------------------------------------------------------------
def all_finite_halves():
    """(1, 32, 64, 32) fp16 holding every bit pattern once, inf and NaN (exponent 31) replaced by zero."""
    p = np.arange(65536, dtype=np.uint16)
    p[(p & 0x7C00) == 0x7C00] = 0
    return p.view(np.float16).reshape(1, 32, 64, 32)


def test_identity_readback_is_exact_for_every_finite_half(gpu_engine):
    """The instrument of every statement below: an identity 1x1 (``np.eye``, no activation, zero bias) into the fp32 head returns
    each half as the same number — normal, subnormal, +-65504 — with -0 as +0 (the accumulator starts at +0)."""
    x = all_finite_halves()
    want = x.astype(np.float32) + np.float32(0.0)
    sub = (np.abs(want) < 2.0 ** -14) & (want != 0)
    assert int(sub.sum()) == 2 * 1023
    case = (1, 32, 64, 32, 32, 1, 1, G.ACT_NONE, False)
    d = dict(x=x, w=np.eye(32, dtype=np.float32)[:, :, None, None], b=np.zeros(32, np.float32))
    try:
        for tile in (-1, 11, 51, 12, 9, 49):
            y = run(gpu_engine, case, d, tile, head="f32")
            bad = bits(y) != bits(want)
            assert not (bad & ~sub).any(), f"tile {tile}: {int((bad & ~sub).sum())} normal halves or zeros come back changed, first at {first_bad(bad & ~sub)}"
            assert not bad.any(), (f"tile {tile}: {int(bad.sum())} of 2046 subnormal halves come back changed ({int((y[sub] == 0).sum())} as zero): the matrix "
                                   "instruction does not read subnormal operands exactly")
    finally:
        gpu_engine.set_tuning(variant=-1)
    _report("identity 1x1 readback (auto, 11, 51, 12, 9, 49): all 63488 finite halves exact, the 2046 subnormal ones included")


# ---- A, B, C --------------------------------------------------------------------------------------------------------------------
STORE_PARAMS = [(i, grp) for i, c in enumerate(CASES) for grp in groups(c)]


@pytest.mark.parametrize("i,group", STORE_PARAMS, ids=[f"s{i}-{grp}" for i, grp in STORE_PARAMS])
def test_f16_store_per_tile(gpu_engine, i, group):
    case = CASES[i]
    d, ref = case_data(i)
    stats, heads = {}, {}
    try:
        r16 = run(gpu_engine, case, d, -1, head="res")[..., :case[4]] if case[8] else None
        if r16 is not None:
            assert np.array_equal(rn16(r16), r16 + np.float32(0.0)), "the residual buffer holds halves"
        for tile in native_tiles(case, group):
            heads[tile] = check_exact_and_bound(gpu_engine, case, d, ref, tile, stats, r16)
    finally:
        gpu_engine.set_tuning(variant=-1)
    assert heads
    paths = sorted({p for t in heads for head, c in head_runs(case) for p in TS.f16_store_paths(TS.expected("f16", t, c)[0], t, c, head)})
    _report(f"case {i} {case} {group} tiles {list(heads)} paths {paths}: " + summary(stats))
    t0 = next(iter(heads))
    for t, y in heads.items():      # C: one accumulation order per group, before any fp16 rounding
        assert np.array_equal(bits(y), bits(heads[t0])), f"fp32 head of tile {t} differs bitwise from tile {t0} (max {np.abs(y - heads[t0]).max():.3e})"


# ---- D: the clamp ---------------------------------------------------------------------------------------------------------------
def clamp_inputs(case, corner):
    """Operands with ONE output of +1e5 and, behind ACT_NONE, one of -1e5 at the same pixel (n, oy, ox): channel ``cp``'s centre-tap
    weights u are scaled by 8, channel ``cm``'s are -8 beta u, and the input pixel under the centre tap gets a u added — a and
    beta solved on the fp64 reference (the conv is linear in both), everything rounded to halves and the reference recomputed
    from the rounded operands.  ``corner``: the last pixel and channels (a partial tile's element-wise stores), else mid-map,
    channels 5 and 6.  -> (operands, reference, {(n, oy, ox, c): +-1}, mask of the outputs whose operands are unchanged)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    d = {key: val.copy() for key, val in data(case).items()}
    Ho, Wo = TS.out_hw(case)
    n, oy, ox, cp, cm = (B - 1, Ho - 1, Wo - 1, cout - 1, cout - 2) if corner else (0, Ho // 2, Wo // 2, 5, 6)
    lin = case[:7] + (G.ACT_NONE, use_res)
    total = lambda dd: (lambda r: r["v"] + (r["r"].astype(np.float16).astype(np.float64) if use_res else 0.0))(reference(lin, dd))[n, oy, ox]
    c = k // 2
    u = d["w"][cp, :, c, c].copy()
    d["w"][cp, :, c, c] = 8.0 * u
    spike = np.zeros(d["x"].shape, np.float64)
    spike[n, oy * s, ox * s, :] = u
    x0 = d["x"].astype(np.float64)
    base = total(d)[cp]
    slope = total(dict(d, x=(x0 + spike)))[cp] - base
    assert slope > 0
    d["x"] = (x0 + (1.0e5 - base) / slope * spike).astype(np.float16)
    assert np.isfinite(d["x"]).all() and float(np.abs(d["x"].astype(np.float32)).max()) < 3.0e4, "the planted input itself stays well inside fp16"
    planted = {(n, oy, ox, cp): 1}
    if act == G.ACT_NONE:
        w0 = d["w"].copy()
        w0[cm, :, c, c] = 0.0
        w1 = w0.copy()
        w1[cm, :, c, c] = -8.0 * u
        v0, v1 = total(dict(d, w=w0))[cm], total(dict(d, w=w1))[cm]
        assert v1 < v0
        d["w"][cm, :, c, c] = (np.float64((-1.0e5 - v0) / (v1 - v0)) * (-8.0 * u.astype(np.float64))).astype(np.float16).astype(np.float32)
        planted[(n, oy, ox, cm)] = -1
    ref = reference(case, d)
    same = np.ones(ref["v"].shape, bool)
    same[n, max(oy - 1, 0):oy + 2, max(ox - 1, 0):ox + 2, :] = False      # outputs that read the changed input pixel (a superset at stride 2)
    same[..., [cp, cm]] = False                                           # (and the residual conv reads it at this pixel only)
    return d, ref, planted, same


def clamp_premises(case, corner):
    """On the fp64 reference: exactly the planted outputs leave the fp16 range, at 1e5 (clear of the rounding boundary 65520), and
    every other one stays below 6e4 less its bound.  -> what ``clamp_inputs`` returned."""
    d, ref, planted, same = clamp_inputs(case, corner)
    r16 = ref["r"].astype(np.float16).astype(np.float64) if case[8] else None
    v = ref["v"] + (r16 if case[8] else 0.0)
    b = P.conv16_bound_f16(K_of(case), case[7], v, ref["S"], res=r16)
    over = np.abs(v) > P.F16_MAX
    assert int(over.sum()) == len(planted) and all(over[at] for at in planted), f"{int(over.sum())} outputs out of range, planted {planted}"
    for at, sgn in planted.items():
        assert 9.9e4 < sgn * v[at] < 1.01e5, (at, v[at])
    assert (np.abs(v)[~over] + b[~over] < 6.0e4).all(), float(np.abs(v)[~over].max())
    assert len(planted) == (2 if case[7] == G.ACT_NONE else 1)
    return d, ref, planted, same


CLAMP_PARAMS = [(i, grp) for i in CLAMP_CASES for grp in groups(CASES[i])]


@pytest.mark.parametrize("i,group", CLAMP_PARAMS, ids=[f"d{i}-{grp}" for i, grp in CLAMP_PARAMS])
def test_f16_store_clamps_per_tile(gpu_engine, i, group):
    """The clamp of ``f16e_pack4`` (16-byte paths) and of the element-wise path is all that stands between a large activation and
    an infinity in HBM (fp16 graphs have no range flag)."""
    case = CASES[i]
    K, act, cout = K_of(case), case[7], case[4]
    d0, _ = case_data(i)
    plant = {corner: clamp_premises(case, corner) for corner in (False, True)}
    try:
        r16 = {}
        for tile in native_tiles(case, group):
            name = f"{TS.expected('f16', tile, case)[0]} tile {tile} {case}"
            base = run(gpu_engine, case, d0, tile)[..., :cout]
            for corner in (False, True):
                d, ref, planted, same = plant[corner]
                if case[8] and corner not in r16:
                    r16[corner] = run(gpu_engine, case, d, -1, head="res")[..., :cout].astype(np.float64)
                y = run(gpu_engine, case, d, tile)[..., :cout]
                assert np.isfinite(y).all(), f"{name}: {int((~np.isfinite(y)).sum())} non-finite halves behind a planted 1e5"
                for at, sgn in planted.items():
                    assert y[at] == np.float32(sgn * P.F16_MAX), f"{name}: a planted {sgn * 1e5:.0e} at {at} is stored as {y[at]!r}"
                changed = (bits(y) != bits(base)) & same
                assert not changed.any(), f"{name}: {int(changed.sum())} halves whose operands did not change differ from the unplanted run, first at {first_bad(changed)}"
                y32 = run(gpu_engine, nores(case), d, tile, head="f32")[..., :cout]
                check_bound(name + " fp32 head, planted", y32, ref["v"], P.conv16_bound(K, act, ref["v"], ref["S"]), ref["S"])
                v = ref["v"] + (r16[corner] if case[8] else 0.0)
                inside = np.abs(v) <= 6.0e4
                b16 = P.conv16_bound_f16(K, act, v, ref["S"], res=r16[corner] if case[8] else None)
                assert (np.abs(y - v)[inside] <= b16[inside]).all(), f"{name}: in-range halves beyond the bound"
    finally:
        gpu_engine.set_tuning(variant=-1)


def test_clamped_values_are_legal_operands(gpu_engine):
    """A buffer holding +-65504 (what the clamp leaves) feeds a 3x3 fp16 conv with an fp32 head: finite, inside bound B."""
    case = (1, 16, 16, 32, 48, 3, 1, G.ACT_NONE, False)
    d = data(case)
    d["x"] = d["x"].copy()
    d["x"][0, 5, 7, :8] = np.float16(65504.0) * np.where(np.arange(8) % 2, -1, 1).astype(np.float16)
    d["x"][0, 0, 0, 3], d["x"][0, 15, 15, 31] = np.float16(-65504.0), np.float16(65504.0)
    ref = reference(case, d)
    assert float(np.abs(ref["v"]).max()) > 5.0e3
    try:
        for tile in (-1, 20, 60, 303, 323):
            y = run(gpu_engine, case, d, tile, head="f32")
            check_bound(f"tile {tile}: +-65504 as operands", y, ref["v"], P.conv16_bound(K_of(case), case[7], ref["v"], ref["S"]), ref["S"])
    finally:
        gpu_engine.set_tuning(variant=-1)


# ---- E: small magnitudes ----------------------------------------------------------------------------------------------------------
def subnormal_share(v):
    a = np.abs(v)
    return float(((a > 2.0 ** -24) & (a < 2.0 ** -14)).mean())


@pytest.mark.parametrize("xs,ws,sub", SMALL_SCALES, ids=[f"x{xs:g}-w{ws:g}" for xs, ws, _ in SMALL_SCALES])
def test_f16_store_small_magnitudes(gpu_engine, xs, ws, sub):
    """Both conversions (packed on the 16-byte paths, scalar on the element-wise path) round to nearest even with gradual
    underflow, and subnormal operands take part in the sums: A and B as at unit scale.  A conversion that flushes fails A where
    ``sub`` (a quarter of the results and more are subnormal halves); dropped subnormal operands fail B on the fp32 head."""
    stats = {}
    try:
        for i, tiles in SMALL_RUNS:
            case = CASES[i]
            d, ref = case_data(i, xs, ws)
            share = subnormal_share(ref["v"] + (ref["r"] if case[8] else 0.0))
            assert share >= 0.25 or not sub, share
            r16 = run(gpu_engine, case, d, -1, head="res")[..., :case[4]] if case[8] else None
            for tile in tiles:
                assert TS.native("f16", tile, case)
                check_exact_and_bound(gpu_engine, case, d, ref, tile, stats, r16, check_width=False)
            print(f"case {i}: {share:.3f} of the fp64 results are subnormal halves")
    finally:
        gpu_engine.set_tuning(variant=-1)
    _report(f"operand scales x {xs:g} w {ws:g}: " + summary(stats))
