"""Per-tile tests of the h2 PAIR stores and of channel slices (csrc/h2_common.h: h2_epilogue).

The sweeps of tests/test_gpu_h2.py let the conv under test write the fp32 head buffer, which reaches two of the five store
paths of ``h2_epilogue``.  Every layer of a real graph but the last writes fp16 PAIRS: the 16-byte path (clamp, cvt_pk,
permlane16_swap, one store per fragment), the same with a 16-byte residual load through the inverse swaps, and the
element-wise path of partial tiles and unaligned slices.  Here the conv under test writes a non-head buffer and an identity
1x1 (``np.eye``, no activation, zero bias) copies it to the fp32 head — the pattern of tests/test_gpu_fp16.py::_run.  The copy
is exact (tests/test_tile_coverage.py::test_identity_readback_of_pairs_is_exact), so the head holds ``h2_value`` of the pairs the
tile stored, whatever tile the identity conv itself lands on.

Per (tile, case) that tests/tile_support.py marks native, with what launched checked against that table:
  1. exact: head == h2_value(h2_split(y32)), y32 = the same tile's fp32-head output on the same operands.  Both paths compute
     act(fma(fma(cross, 1/2048, main), scale, bias)) [+ decoded residual] with the same operations in the same order and
     ``h2_split`` is the encoder's arithmetic (RN16, exact difference, x 2048, RN16): no tolerance;
  2. against fp64 conv2d: the 3e-6 relative bound of the fp32-head sweeps, unchanged;
  3. bitwise across tiles (all h2 tiles share one accumulation scheme);
  4. the overflow flag stays down; one planted output of 1e5 raises it on every tile's pair path, fast and slow.
The buffer is filled with a per-channel sentinel first: channels a partial fragment masks out must still hold it.

Slices: the conv writes ``cout`` channels at ``out_choff`` of a 160-wide buffer (a 96- / 192-channel tile overhangs the slice by
channels that belong to a neighbour: they keep the sentinel exactly); reads its input at channel 32 of a wider buffer whose other
channels hold 3e4; adds a residual from channel 16 of a wider buffer — each bitwise the offset-0 run.  ``out_choff = 8`` with 24
channels (4-aligned, not 16-aligned: accepted by the engine, element-wise path) is part of the set."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import engine as E, graph as G
from tests import tile_support as TS
from tests.test_gpu_conv import ACT_FN, _launched
from tests.test_gpu_h2 import H2_TILES

pytestmark = pytest.mark.gpu

# (B, H, W, cin, cout, k, stride, act, residual) — per kernel group (stride-1 3x3 with whole chunks / with 16, 32, 48 input channels,
# 1x1, stride-2 3x3): whole tiles without and with residual (16-byte stores / + 16-byte residual loads) and partial tiles
# (element-wise).  tests/test_tile_coverage.py checks that every tile id meets all three natively.
EPI_CASES = [
    (1, 16, 16, 64, 192, 3, 1, G.ACT_SILU, False),
    (1, 8, 16, 64, 192, 3, 1, G.ACT_RELU, True),
    (3, 17, 23, 96, 96, 3, 1, G.ACT_SILU, True),
    (1, 18, 20, 64, 39, 3, 1, G.ACT_NONE, True),
    (2, 16, 16, 64, 80, 3, 1, G.ACT_LEAKY, False),       # the 64 x 80 tile's whole tiles
    (1, 8, 16, 64, 80, 3, 1, G.ACT_SILU, True),
    (1, 16, 32, 32, 384, 3, 1, G.ACT_RELU, False),
    (1, 16, 16, 16, 96, 3, 1, G.ACT_LEAKY, True),
    (1, 18, 20, 48, 39, 3, 1, G.ACT_SILU, False),
    (1, 16, 24, 128, 192, 1, 1, G.ACT_SILU, False),
    (1, 16, 24, 128, 192, 1, 1, G.ACT_RELU, True),
    (1, 20, 27, 704, 96, 1, 1, G.ACT_SILU, True),
    (1, 8, 16, 64, 80, 1, 1, G.ACT_NONE, False),
    (1, 8, 16, 64, 80, 1, 1, G.ACT_SILU, True),
    (2, 32, 32, 32, 192, 3, 2, G.ACT_RELU, False),
    (2, 32, 32, 64, 192, 3, 2, G.ACT_SILU, True),
    (1, 18, 22, 128, 80, 3, 2, G.ACT_SILU, True),
    (1, 16, 32, 64, 80, 3, 2, G.ACT_NONE, False),
    (1, 16, 32, 64, 80, 3, 2, G.ACT_SILU, True),
]
# the overflow-flag cases: per kernel group one with whole tiles (16-byte path) and one with partial tiles (element-wise path)
OVF_CASES = [EPI_CASES[i] for i in (0, 3, 4, 6, 8, 9, 11, 14, 16)]


def native_runs(case):
    """(tile, w_single) of every native run: the two-product mode reaches every tile id; the three-product mode is added where it
    runs another kernel family under the same id (343: h2w instead of h2v)."""
    runs = []
    for t in H2_TILES:
        f2 = TS.expected("h2", t, case, True)
        if f2[1] == t:
            runs.append((t, True))
        f3 = TS.expected("h2", t, case, False)
        if f3[1] == t and f3 != f2:
            runs.append((t, False))
    return runs


def _data(case):
    B, H, W, cin, cout, k, s, act, use_res = case
    rng = np.random.default_rng(cin * 29 + cout * 3 + k + s)
    d = dict(x=rng.normal(0, 1, (B, H, W, cin)).astype(np.float32),
             w=rng.normal(0, (2.0 / (cin * k * k)) ** 0.5, (cout, cin, k, k)).astype(np.float16).astype(np.float32),       # fp16 numbers: PA_CONV_W_SINGLE
             scale=rng.uniform(0.5, 2.0, cout).astype(np.float32), b=rng.normal(0, 0.5, cout).astype(np.float32),
             wr=rng.normal(0, (1.0 / cin) ** 0.5, (cout, cin, 1, 1)).astype(np.float32))
    return d


def _want(case, d):
    B, H, W, cin, cout, k, s, act, use_res = case
    xt = torch.from_numpy(d["x"]).permute(0, 3, 1, 2).double()
    w = torch.from_numpy(d["w"]).double() * torch.from_numpy(d["scale"]).double()[:, None, None, None]
    want = ACT_FN[act](F.conv2d(xt, w, torch.from_numpy(d["b"]).double(), stride=s, padding=k // 2))
    if use_res:
        want = want + F.conv2d(xt, torch.from_numpy(d["wr"]).double(), stride=s)
    return want.permute(0, 2, 3, 1).numpy()


def sentinel(n):
    return (-100.0 - 0.25 * np.arange(n)).astype(np.float32)          # fp16 numbers: exact as pairs


BIG = 3.0e4                                                            # what the neighbours of an input / residual slice hold


def _graph(case, d, head="pair", out_choff=0, width=None, in_choff=None, res_choff=0):
    """[1x1 -> residual buffer], [sentinel fill], the conv under test -> a slice of the non-head buffer S, identity 1x1 S -> fp32 head.
    head="f32": the conv writes the head buffer itself (the graph of tests/test_gpu_h2.py).  Returns (graph, index of the conv
    under test among the conv ops)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    z = lambda *shape: np.zeros(shape, np.float32)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_H2)
    b0 = g.buf(0, cin)
    lvl = 1 if s == 2 else 0
    src = (b0, 0, cin)
    if in_choff is not None:             # the input through an identity copy into a slice of a (wider) buffer: the same pairs at every offset
        bi = g.buf(0, in_choff + cin + (16 if in_choff else 0))
        if in_choff:
            g.conv((b0, 0, cin), (bi, 0), z(in_choff, cin, 1, 1), np.full(in_choff, BIG, np.float32), 1, 1, G.ACT_NONE)
            g.conv((b0, 0, cin), (bi, in_choff + cin), z(16, cin, 1, 1), np.full(16, BIG, np.float32), 1, 1, G.ACT_NONE)
        g.conv((b0, 0, cin), (bi, in_choff), np.eye(cin, dtype=np.float32)[:, :, None, None], z(cin), 1, 1, G.ACT_NONE)
        src = (bi, in_choff, cin)
    res = None
    if use_res:
        rb = g.buf(lvl, res_choff + G.pad16(cout))
        if res_choff:
            g.conv((b0, 0, cin), (rb, 0), z(res_choff, cin, 1, 1), np.full(res_choff, BIG, np.float32), 1, s, G.ACT_NONE)
        g.conv((b0, 0, cin), (rb, res_choff), d["wr"], z(cout), 1, s, G.ACT_NONE)
        res = (rb, res_choff)
    if head == "f32":
        assert out_choff == 0 and width is None
        b1 = g.buf(lvl, G.pad16(cout))
        g.conv(src, (b1, 0), d["w"], d["b"], k, s, act, res=res, out_scale=d["scale"])
        g.head_buf = (b1, -1, -1)
        which = -1
    else:
        wd = G.pad16(cout) if width is None else width
        assert wd % 16 == 0 and out_choff + cout <= wd
        S = g.buf(lvl, wd)
        g.conv((b0, 0, cin), (S, 0), z(wd, cin, 1, 1), sentinel(wd), 1, s, G.ACT_NONE)
        g.conv(src, (S, out_choff), d["w"], d["b"], k, s, act, res=res, out_scale=d["scale"])
        hd = g.buf(lvl, wd)
        g.conv((S, 0, wd), (hd, 0), np.eye(wd, dtype=np.float32)[:, :, None, None], z(wd), 1, 1, G.ACT_NONE)
        g.head_buf = (hd, -1, -1)
        which = -2
    assert g.ops[which]["flags"] & G.FLAG_W_SINGLE
    return g, which


def _run(eng, case, d, tile, ws, x=None, **kw):
    """One forced run; what launched must be what tests/tile_support.py says.  Returns (head array, overflow flag)."""
    g, which = _graph(case, d, **kw)
    eng.set_tuning(variant=tile, w_single=1 if ws else 0)
    eng.set_profiling(True)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(case[0])
        y = m.tracknet_infer(d["x"] if x is None else x)
        got = _launched(m, which)
        flag = m.take_overflow()
    finally:
        eng.set_profiling(False)
        m.close()
    want = TS.expected("h2", tile, case, ws)
    assert got == want, f"requested {tile}, launched {got[0]}/{got[1]}; tests/tile_support.py says {want[0]}/{want[1]}"
    return y, flag


def _reset(eng):
    eng.set_tuning(variant=-1, w_single=1)


@pytest.mark.parametrize("case", EPI_CASES, ids=[f"e{i}" for i in range(len(EPI_CASES))])
def test_h2_pair_store_per_tile(gpu_engine, case):
    cout = case[4]
    d = _data(case)
    want = _want(case, d)
    sc = max(1.0, float(np.abs(want).max()))
    heads = {}
    try:
        for tile, ws in native_runs(case):
            y32, _ = _run(gpu_engine, case, d, tile, ws, head="f32")
            stored = G.h2_value(*G.h2_split(y32[..., :cout]))
            for rep in range(2):                       # twice: a DMA / barrier race is not deterministic
                name = f"{tile}{'' if ws else ' three-product'}.{rep}"
                y, flag = _run(gpu_engine, case, d, tile, ws)
                assert not flag, f"{name}: overflow flag"
                assert np.array_equal(y[..., cout:], np.broadcast_to(sentinel(y.shape[-1])[cout:], y[..., cout:].shape)), f"{name}: wrote beyond its {cout} channels"
                y = y[..., :cout]
                bad = y != stored
                assert not bad.any(), (f"{name}: pair store differs from h2_split of its own fp32 output: {int(bad.sum())} values, max "
                                       f"{np.abs(y - stored).max():.3e}, first at (n, y, x, c) = {tuple(int(i) for i in np.argwhere(bad)[0])}")
                err = float(np.abs(y - want).max()) / sc
                assert err < 3e-6, f"{name}: rel err {err:.2e} vs fp64 conv2d"
                heads[name] = y
    finally:
        _reset(gpu_engine)
    print(f"case {case}: pair path(s) " + ", ".join(sorted({p for t, ws in native_runs(case) for p in TS.h2_store_paths(TS.expected('h2', t, case, ws)[0], t, case)}))
          + f" on tiles {[t for t, _ in native_runs(case)]}")
    ref_name, ref = next(iter(heads.items()))
    for name, y in heads.items():
        assert np.array_equal(y, ref), f"{name} differs bitwise from {ref_name} (max {np.abs(y - ref).max():.3e})"


def overflow_inputs(case, corner):
    """Operands with exactly ONE output outside the fp16 range: 1e5 — clear of the band (65488, 65504] where the two store paths
    are documented to differ — planted through one input pixel (x along the centre-tap weights of one channel, whose BatchNorm
    scale is 8 so that the planted input itself stays a pair); every other output stays below 6e4.  All of it is checked on
    the fp64 reference (here and, without a GPU, in tests/test_tile_coverage.py).  ``corner``: in the last pixel and channel — where
    a tile that does not divide the case has its partial pixel tile / channel tile / fragment (element-wise path); otherwise mid-map,
    channel 5 (a tile that divides the case stores everything through the 16-byte path: the range check on the packed halves)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    d = _data(case)
    Ho, Wo = TS.out_hw(case)
    n, oy, ox, co = (B - 1, Ho - 1, Wo - 1, cout - 1) if corner else (0, Ho // 2, Wo // 2, 5)
    d["scale"][co] = 8.0
    spike = np.zeros_like(d["x"])
    spike[n, oy * s, ox * s, :] = d["w"][co, :, k // 2, k // 2]
    case_lin = case[:7] + (G.ACT_NONE, use_res)
    slope = _want(case_lin, dict(d, x=spike, b=np.zeros(cout, np.float32)))[n, oy, ox, co]      # output per unit of the spike (conv and residual are linear)
    base = _want(case_lin, d)[n, oy, ox, co]
    assert slope > 0
    x = (d["x"] + np.float32((1.0e5 - base) / slope) * spike).astype(np.float32)
    assert float(np.abs(x).max()) < 6.0e4, "the planted input itself must be a pair"
    want = _want(case, dict(d, x=x))
    over = np.abs(want) > 6.0e4
    assert int(over.sum()) == 1 and over[n, oy, ox, co] and 9.0e4 < want[n, oy, ox, co] < 1.1e5, "exactly one output out of range"
    return d, x, (n, oy, ox, co)


@pytest.mark.parametrize("case", OVF_CASES, ids=[f"o{i}" for i in range(len(OVF_CASES))])
def test_h2_pair_store_raises_the_overflow_flag_per_tile(gpu_engine, case):
    """``overflow_inputs``: one output of 1e5 must raise the model's flag on every native tile's pair path and is stored clamped;
    the same graph on the unplanted input leaves the flag down."""
    planted = {corner: overflow_inputs(case, corner) for corner in (False, True)}
    try:
        for tile, ws in native_runs(case):
            whole = "full" in TS.classes("h2", TS.expected("h2", tile, case, ws)[0], tile, case)
            d, x, at = planted[not whole]
            y, flag = _run(gpu_engine, case, d, tile, ws, x=x)
            assert flag, f"tile {tile}: an output of 1e5 did not raise the overflow flag ({'16-byte' if whole else 'element-wise'} path)"
            assert y[at] == np.float32(G.H2_MAX), f"tile {tile}: stored {y[at]} for a clamped value"
            _, flag = _run(gpu_engine, case, d, tile, ws)
            assert not flag, f"tile {tile}: flag up on in-range outputs"
    finally:
        _reset(gpu_engine)


# ---- slices ------------------------------------------------------------------------------------------------------------
# one base shape per kernel group, small maps; (out_choff, cout, residual) inside a 160-wide buffer
SLICE_BASES = [(1, 16, 16, 64, 3, 1), (1, 16, 16, 32, 3, 1), (1, 16, 16, 64, 1, 1), (1, 32, 32, 64, 3, 2)]
OUT_SLICES = [(16, 32, False), (48, 80, True), (16, 96, True), (48, 96, False), (8, 24, False)]
SLICE_WIDTH = 160


def _slice_case(base, cout, res, act=G.ACT_SILU):
    B, H, W, cin, k, s = base
    return (B, H, W, cin, cout, k, s, act, res)


@pytest.mark.parametrize("base", SLICE_BASES, ids=["3x3", "3x3-cin32", "1x1", "s2"])
def test_h2_output_slice_leaves_the_neighbours_alone(gpu_engine, base):
    sent = sentinel(SLICE_WIDTH)
    try:
        for choff, cout, res in OUT_SLICES:
            case = _slice_case(base, cout, res)
            d = _data(case)
            for tile, ws in native_runs(case):
                ref, _ = _run(gpu_engine, case, d, tile, ws, width=SLICE_WIDTH)
                y, flag = _run(gpu_engine, case, d, tile, ws, width=SLICE_WIDTH, out_choff=choff)
                name = f"tile {tile}, {cout} channels at {choff}"
                assert not flag
                assert np.array_equal(y[..., choff:choff + cout], ref[..., :cout]), f"{name}: differs from the offset-0 run"
                out = np.concatenate([y[..., :choff], y[..., choff + cout:]], -1)
                exp = np.concatenate([sent[:choff], sent[choff + cout:]])
                bad = out != np.broadcast_to(exp, out.shape)
                assert not bad.any(), f"{name}: {int(bad.sum())} values outside the slice changed (channels {sorted(set(int(c) for c in np.argwhere(bad)[:, -1]))[:8]} of the remainder)"
                assert np.array_equal(ref[..., cout:], np.broadcast_to(sent[cout:], ref[..., cout:].shape)), f"{name}: offset-0 run wrote beyond its channels"
    finally:
        _reset(gpu_engine)


@pytest.mark.parametrize("base", SLICE_BASES, ids=["3x3", "3x3-cin32", "1x1", "s2"])
def test_h2_input_slice_reads_its_own_channels(gpu_engine, base):
    """src = (buf, 32, cin) of a buffer 32 + cin + 16 wide whose other channels hold 3e4: bitwise the in_choff = 0 run."""
    try:
        for cout, res in ((96, False), (40, True)):
            case = _slice_case(base, cout, res)
            d = _data(case)
            for tile, ws in native_runs(case):
                ref, _ = _run(gpu_engine, case, d, tile, ws, in_choff=0)
                y, flag = _run(gpu_engine, case, d, tile, ws, in_choff=32)
                assert not flag
                assert np.array_equal(y, ref), f"tile {tile}, cout {cout}: input slice at channel 32 differs from offset 0 (max {np.abs(y - ref).max():.3e})"
    finally:
        _reset(gpu_engine)


@pytest.mark.parametrize("base", SLICE_BASES, ids=["3x3", "3x3-cin32", "1x1", "s2"])
def test_h2_residual_slice_reads_its_own_group(gpu_engine, base):
    """The residual at res_choff = 16 of a wider buffer (channels 0 .. 15 hold 3e4): bitwise the res_choff = 0 run — 192 channels
    on whole tiles (16-byte residual loads), 40 channels (element-wise path)."""
    try:
        for cout in (192, 40):
            case = _slice_case(base, cout, True)
            d = _data(case)
            for tile, ws in native_runs(case):
                ref, _ = _run(gpu_engine, case, d, tile, ws)
                y, flag = _run(gpu_engine, case, d, tile, ws, res_choff=16)
                assert not flag
                assert np.array_equal(y, ref), f"tile {tile}, cout {cout}: residual at channel 16 differs from offset 0 (max {np.abs(y - ref).max():.3e})"
    finally:
        _reset(gpu_engine)
