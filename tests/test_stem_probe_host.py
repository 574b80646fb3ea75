"""CPU checks of tests/stem_probe.py, the instrument of tests/test_gpu_stem.py.

* every probe graph passes ``validate_desc`` (the stand-alone harness of tests/test_graph_plan_host.py), and run through
  tests/graph_interp with NaN in every byte the graph does not write, its decoded head equals the interpreter's stem buffer bit
  for bit and no head value is NaN; the five readout passes behind a fused-shape layer 1 reassemble the map, the padding
  positions decode to 0 and every element seen twice is seen with the same bits;
* the numpy reference equals ``F.silu(F.conv2d(x.double(), ...))`` to 1e-14;
* numpy fp32 emulations of both arithmetic orders (stand-alone: sum w fl(u8 / 255); fused: sum (w / 255 as a row-scaled fp16 pair)
  u8) stay inside the bound on the weights and frames of the GPU cases: the reference alone does not use the bound up."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from padel_analytics_amd import graph as G
from tests import graph_interp, stem_probe as P
from tests.test_graph_plan_host import ask, build_harness, describe_graph

# (storage, width, level-1 buffer width, channel offset): every stand-alone graph of tests/test_gpu_stem.py
STANDALONE = [("f32", c, 0, 0) for c in (16, 32, 48, 64, 80)] + [("h2", c, 0, 0) for c in (16, 32, 48, 64, 80)] + \
             [("f16", 32, 0, 0), ("f16", 64, 0, 0)] + [(t, 16, 48, 16) for t in ("f32", "h2", "f16")]
SHAPES = [(1, 32, 32), (3, 32, 96), (2, 96, 64)]


def _net_in(frames):
    return torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("stem_probe") / "graph_plan_main")


def _validate(harness, g, fusable):
    v, s = ask(harness, describe_graph(g) + "validate\nstem\n")
    assert v == "ok", v
    stem_op = [i for i, o in enumerate(g.ops) if o["kind"] == G.OP_STEM][-1]          # (the stem under test is the last one)
    assert (stem_op in [int(x) for x in s.split()[1:]]) == fusable, s


@pytest.mark.parametrize("t,c,width,choff", STANDALONE, ids=[f"{t}-c{c}" + (f"@{o}of{w}" if w else "") for t, c, w, o in STANDALONE])
def test_standalone_graph_decodes_the_stem_buffer_bit_for_bit(harness, t, c, width, choff):
    w, b = P.stem_weights(c)
    g = P.standalone_graph(t, c, w, b, width, choff)
    _validate(harness, g, not (t == "f16" and width))          # (the fp16 slice is read at k-step width: 32 channels, not the stem's 16)
    if t == "h2":
        assert all(o["flags"] & G.FLAG_W_SINGLE for o in g.ops if o["kind"] == G.OP_CONV)
    frames = P.probe_frames(2, 32, 64)
    bufs = graph_interp.run(g, net_in=_net_in(frames), stale=float("nan"))
    heads = [_nhwc(bufs[i]) for i in g.head_buf]
    assert not any(np.isnan(h).any() for h in heads), "a head byte the graph does not write"
    assert all((h[..., :P.READOUT] == np.where(np.arange(P.READOUT) == 64, -30.0, 0.0)).all() for h in heads)
    stem_op = [o for o in g.ops if o["kind"] == G.OP_STEM][-1]
    stem = _nhwc(bufs[stem_op["out_buf"]])[..., choff:choff + c]
    got = P.decode_level1(heads[0])
    assert got.shape == (2, 16, 32, c)
    assert np.array_equal(_bits(got), _bits(stem))
    assert P.storable(t, got)
    # and the interpreter's fp32 stem is the reference to fp32 rounding
    v, S = P.stem_truth(np.concatenate([frames, np.zeros_like(frames[..., :1])], -1), w, b)
    P.check(f"interpreter {t} c{c}", t, P.K_STANDALONE, got, v, S)


@pytest.mark.parametrize("c", [16, 32, 48])
def test_fused_readout_passes_reassemble_the_stem_map(harness, c):
    w, b = P.stem_weights(c)
    frames = P.probe_frames(2, 32, 64)
    obs = P.Observations(c)
    stem = None
    for p in range(P.N_PASSES):
        g = P.fused_readout_graph(c, w, b, p)
        _validate(harness, g, True)
        bufs = graph_interp.run(g, net_in=_net_in(frames), stale=float("nan"))
        heads = [_nhwc(bufs[i]) for i in g.head_buf]
        assert not any(np.isnan(h).any() for h in heads)
        obs.add_pass(p, P.decode_layer1(heads[0]))
        stem = _nhwc(bufs[g.ops[0]["out_buf"]])
    assert set(np.concatenate([P.pass_pairs(c, p) for p in range(P.N_PASSES)]).tolist()) == set(range(9 * c))
    assert obs.repeat_mismatch == 0
    pads = obs.padding()
    assert len(pads) == 6
    for tap, z in pads:
        assert z.size and (z == 0.0).all(), tap
    got, differ, twice = obs.reassemble()
    assert differ == 0
    assert twice == 2 * c * (16 * 32 - 9 * 17), twice          # all but the 9 rows x 17 columns seen once (the test below)
    assert np.array_equal(_bits(got), _bits(stem))
    assert P.storable("h2", got)


def test_elements_seen_twice_are_the_odd_rows_and_columns():
    """An element is seen once per tap that reaches it: rows 2 oy - 1 + ky.  Even rows: ky = 1 only.  Odd rows but the last: ky = 2 of
    one output row and ky = 0 of the next.  The same for columns; the counts multiply."""
    c = 16
    obs = P.Observations(c)
    rng = np.random.default_rng(0)
    stem = rng.normal(0, 1, (1, 8, 12, c)).astype(np.float32)
    xp = np.pad(stem, ((0, 0), (1, 1), (1, 1), (0, 0)))
    full = np.stack([xp[:, ky:ky + 8:2, kx:kx + 12:2] for ky in range(3) for kx in range(3)])      # (9, 1, 4, 6, c)
    for p in range(P.N_PASSES):
        pairs = P.pass_pairs(c, p)
        obs.add_pass(p, np.stack([full[q // c][..., q % c] for q in pairs], -1))
    got, differ, twice = obs.reassemble()
    assert np.array_equal(got, stem) and differ == 0 and obs.repeat_mismatch == 0
    rows = np.array([1 if (y % 2 == 0 or y == 7) else 2 for y in range(8)])
    cols = np.array([1 if (x % 2 == 0 or x == 11) else 2 for x in range(12)])
    assert twice == int((np.outer(rows, cols) > 1).sum()) * c
    # a halo that was recomputed differently shows
    full[8, 0, 1, 2, 5] = np.nextafter(full[8, 0, 1, 2, 5], np.float32(9))      # element (3, 5) as the last of its four taps sees it
    obs = P.Observations(c)
    for p in range(P.N_PASSES):
        obs.add_pass(p, np.stack([full[q // c][..., q % c] for q in P.pass_pairs(c, p)], -1))
    assert obs.reassemble()[1] == 1


def test_unshuffle_decode_inverts_the_one_hot_convs():
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.normal(0, 1, (2, 16, 16, 24)).astype(np.float32))
    y = x.permute(0, 3, 1, 2)
    for cin in (24, 96):
        y = F.conv2d(y, torch.from_numpy(P.unshuffle_weight(cin)), stride=2, padding=1)
    assert np.array_equal(P.unshuffle_decode(_nhwc(y), 2), x.numpy())


@pytest.mark.parametrize("c", [16, 80])
def test_reference_matches_torch_in_fp64(c):
    w, b = P.stem_weights(c)
    frames = P.probe_frames(2, 32, 64)
    v, S = P.stem_truth(frames, w, b)
    x = torch.from_numpy(frames.astype(np.float64) / 255.0).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
    want = F.silu(F.conv2d(x, wt, torch.from_numpy(b.astype(np.float64)), stride=2, padding=1)).permute(0, 2, 3, 1).numpy()
    assert float(np.abs(v - want).max()) <= 1e-14 * max(1.0, float(np.abs(want).max()))
    s_want = F.conv2d(x, wt.abs(), torch.from_numpy(np.abs(b).astype(np.float64)), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    assert float(np.abs(S - s_want).max()) <= 1e-13 and float(S.min()) >= 0.25
    assert float(np.abs(v[..., 1] - b[1] / (1 + np.exp(-np.float64(b[1])))).max()) <= 1e-15       # channel 1: bias only


@pytest.mark.parametrize("c", [16, 32, 48, 64, 80])
def test_fp32_emulations_of_both_orders_stay_inside_the_bound(c):
    w, b = P.stem_weights(c)
    for B, h, ww in SHAPES:
        frames = P.probe_frames(B, h, ww)
        v, S = P.stem_truth(frames, w, b)
        for t in ("f32", "h2") + (("f16",) if c in (32, 64) else ()):
            worst = P.check(f"emulation stand-alone {t} c{c} {(B, h, ww)}", t, P.K_STANDALONE, P.emulate_standalone(frames, w, b, t), v, S)
            assert t != "f32" or worst <= P.K_STANDALONE / 3.0, worst          # (the reference uses a third of K at the most)
        if c <= 48:
            P.check(f"emulation fused c{c} {(B, h, ww)}", "h2", P.K_FUSED, P.emulate_fused(frames, w, b), v, S)


def test_the_bound_notices_a_dropped_tap_and_an_unpadded_border():
    """The two planted errors of the issue, in the emulation: a stem without its last tap, and silu(bias) where zero padding is due."""
    c = 16
    w, b = P.stem_weights(c)
    frames = P.probe_frames(1, 32, 32)
    v, S = P.stem_truth(frames, w, b)
    w_bad = w.copy()
    w_bad[:, 2, 2, 2] = 0.0
    with pytest.raises(AssertionError, match="x the bound"):
        P.check("dropped tap", "f32", P.K_STANDALONE, P.emulate_standalone(frames, w_bad, b), v, S)
    silu_b = (b.astype(np.float64) / (1 + np.exp(-b.astype(np.float64)))).astype(np.float32)
    assert (np.abs(silu_b) >= 0.1).all()          # what a kernel that evaluated the stem in layer 1's padding would leave there
