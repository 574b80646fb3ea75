"""The two ways ``stem_l1_h2_kernel`` gets the operands of its stem phase must give the same bits.

The register-weights instantiations (``<NF, true, true>``, what the benchmark runs) read the stem's weight rows from an operand
block built once per weight blob (``stem_l1_operands_kernel``) and gather the input bytes from a patch staged in LDS; the
weight-ring instantiations (``tune = 8``) split the weights in their prologue and gather every K slot from HBM with its own
clamp and border predicate.  Same arithmetic, same K order, same MFMA sequence: every stored bit is the same.

With the instrument of tests/test_gpu_stem.py (tests/stem_probe.py), for c = 16, 32, 48 and network inputs (1, 32, 32) — one
partial tile column, two tile rows —, (2, 64, 160) — an interior tile, a partial last column, a frame boundary — and (3, 32, 96),
each with three more frames appended (all 0, all 255, columns alternating 0 / 255):
* the nine tap observations of the five readout passes, and the stem map reassembled from them, match bit for bit;
* layer 1 with random fp16-number weights and SiLU matches bit for bit.
For c = 16 and 32 a model created ``empty=True`` runs once (its operand block is built from zero weights), receives the weights
of a loaded model through ``bcast_weights_from`` and must then give the loaded model's head bit for bit: a block that was not
rebuilt shows (tests/test_gpu_baseline_configs.py does the same for the benchmark's c = 48 graphs)."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, graph as G
from tests import stem_probe as P
from tests.test_gpu_stem import DEFAULTS, KW, VARIANTS, n_conv_rows, require_premise, run_fused

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 32), (2, 64, 160), (3, 32, 96)]
CASES = [(c, s) for c in (16, 32, 48) for s in SHAPES]
IDS = [f"c{c}-{'x'.join(map(str, s))}" for c, s in CASES]


def frames_of(shape):
    B, h, w = shape
    extra = np.zeros((3, h, w, 3), np.uint8)
    extra[1] = 255
    extra[2, :, 0::2] = 255
    return np.concatenate([P.probe_frames(B, h, w), extra])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def n_differ(a, b):
    return int((bits(a) != bits(b)).sum())


@pytest.mark.parametrize("c,shape", CASES, ids=IDS)
def test_stem_phase_register_weights_equals_weight_ring(gpu_engine, c, shape):
    require_premise(gpu_engine, "h2-behind-layer1")
    w, b = P.stem_weights(c)
    frames = frames_of(shape)
    obs = {v: P.Observations(c) for v in ("register-weights", "weight-ring")}
    for p in range(P.N_PASSES):
        for v, o in obs.items():
            name = f"stem_l1_h2_kernel<{c // 16}> {v} c{c} {shape} + 3 frames, pass {p}"
            l1, _, flag = run_fused(gpu_engine, P.fused_readout_graph(c, w, b, p), frames, VARIANTS[v], name)
            assert not flag, f"{name}: overflow flag with ordinary weights"
            o.add_pass(p, l1)
    a, r = obs["register-weights"], obs["weight-ring"]
    for t in range(9):
        d = n_differ(a.obs[t], r.obs[t])
        assert d == 0, f"c{c} {shape}: {d} of {a.obs[t].size} observations of tap {divmod(t, 3)} differ bitwise between the two operand paths"
    sa, da, _ = a.reassemble()
    sr, dr, _ = r.reassemble()
    assert da == 0 and dr == 0 and a.repeat_mismatch == 0 and r.repeat_mismatch == 0
    assert not np.isnan(sa).any() and n_differ(sa, sr) == 0
    assert sa[-3:].any() and not np.array_equal(sa[-3], sa[-2]), "the appended frames reached the kernel"


@pytest.mark.parametrize("c,shape", CASES, ids=IDS)
def test_layer1_register_weights_equals_weight_ring(gpu_engine, c, shape):
    require_premise(gpu_engine, "h2-behind-layer1")
    w, b = P.stem_weights(c)
    w1, b1 = P.layer1_weights(c)
    w1h = w1.astype(np.float16).astype(np.float32)
    frames = frames_of(shape)
    got = {}
    for v in ("register-weights", "weight-ring"):
        g = P.fused_graph(c, w, b, w1h, b1, G.ACT_SILU)
        assert g.ops[1]["flags"] & G.FLAG_W_SINGLE
        got[v], _, flag = run_fused(gpu_engine, g, frames, VARIANTS[v], f"stem_l1_h2_kernel<{c // 16}> layer 1 {v} c{c} {shape}")
        assert not flag and np.isfinite(got[v]).all()
    d = n_differ(got["register-weights"], got["weight-ring"])
    assert d == 0, f"c{c} {shape}: {d} of {got['weight-ring'].size} layer-1 values differ bitwise between the two operand paths"
    assert np.abs(got["weight-ring"]).max() > 0.1


@pytest.mark.parametrize("c", [16, 32])
def test_operand_block_is_rebuilt_after_a_weight_broadcast(gpu_engine, c):
    eng = gpu_engine
    if getattr(eng, "nranks", None) is None:
        eng.comm_init(E.comm_unique_id(), 1, 0)
    w, b = P.stem_weights(c)
    w1, b1 = P.layer1_weights(c)
    g = P.fused_graph(c, w, b, w1.astype(np.float16).astype(np.float32), b1, G.ACT_SILU)
    frames = frames_of(SHAPES[1])
    B, h, wd, _ = frames.shape

    def head(m):
        m.set_max_batch(B)
        m.yolo_infer(frames, B, h, wd, imgsz=max(h, wd), **KW)
        return m.read_head(0, B)

    loaded, empty = E.Model(eng, g), E.Model(eng, g, empty=True)
    eng.set_profiling(True)
    try:
        eng.set_tuning(**DEFAULTS)
        want = head(loaded)
        assert n_conv_rows(loaded) == sum(1 for o in g.ops if o["kind"] == G.OP_CONV) - 1, "the fused kernel did not run"
        zero = head(empty)                           # builds the empty model's operand block from zero weights
        assert not np.array_equal(zero, want)
        eng.bcast_weights_from(loaded, empty, root=0)
        got = head(empty)
        assert n_conv_rows(empty) == n_conv_rows(loaded)
    finally:
        eng.set_tuning(**DEFAULTS)
        eng.set_profiling(False)
        loaded.close()
        empty.close()
    d = n_differ(got, want)
    assert d == 0, f"c{c}: {d} of {want.size} head values differ between the loaded and the broadcast weights (a stale stem operand block?)"
