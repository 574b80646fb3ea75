"""The third phase of ``stem_l1_h2_kernel`` (csrc/stem_l1_h2.hip, tuning ``fuse_stem_cv1``): the 1x1 conv behind layer 1 — model.2.cv1
of a YOLOv8 graph — computed inside the fused stem + layer-1 kernel, layer 1's map never written.  Same products in the same order
per accumulator as the launch it replaces, the same epilogue: every stored bit is the same.

Probe graphs (tests/stem_probe.py): stem (c) -> layer 1 (3x3 stride 2, 2c, SiLU) -> 1x1 (2c -> 2c, SiLU) into channels
[choff, choff + 2c) of a buffer ``choff + 2c`` wide, whose other channels a second 1x1 fills from the first one's output -> one
unshuffle (one-hot 3x3 stride 2: every value of the buffer, returned bit for bit) -> head channels.  Every run is made over an
arena filled with NaN patterns: on the fused path layer 1's buffer keeps them, so a head without NaN also says nobody read it.

* c = 48, 32, 16; batch 2; network inputs (32, 64) — layer-1 map 8 x 16: whole 4 x 16 tiles, two tile rows —, (64, 160) — 16 x 40:
  a partial last tile column, four tile rows —, (32, 32) — 8 x 8: narrower than one tile; the 1x1 at channel offset 0 of a buffer of
  its own width and at offset 16 of a wider one.  (A partial last tile ROW cannot be made: the network input of pa_yolo_infer is a
  multiple of 32 in both directions, so a layer-1 map has a multiple of 8 rows.  The kernel's pixel mask treats rows and columns
  alike; the columns are what a graph can reach.)
* ``Model.last_stem_path()`` says the fused path ran on each of them — and did not with profiling on, with a second reader of layer
  1's map (a hand-made graph), with a three-product 1x1 (weights that are no fp16 numbers), with ``fuse_stem_cv1 = 0``.
* real YOLOv8 n / s / m graphs at a 192 x 288 network input: heads, boxes and counts bit for bit.
* range: model.1's BatchNorm scaled by 2^18 (model.2.cv1's scaled back) overflows the pairs: the flag goes up on both paths, ``yolo.YOLO`` repeats
  the batch on bf16x3 on both, and the results are the bf16x3 model's."""
import numpy as np
import pytest

from padel_analytics_amd import checkpoint, engine as E, graph as G, yolo, yolo_arch
from tests import stem_probe as P
from tests import synth
from tests.test_gpu_stem import DEFAULTS, KW, infer, n_conv_rows, require_premise

pytestmark = pytest.mark.gpu

SHAPES = {"whole-tiles": (2, 32, 64), "partial-column": (2, 64, 160), "narrow": (2, 32, 32)}
CASES = [(c, s, off) for c in (48, 32, 16) for s in SHAPES for off in (0, 16)]
IDS = [f"c{c}-{s}-choff{off}" for c, s, off in CASES]
ON = {**DEFAULTS, "fuse_stem_cv1": 1}


def fp16_numbers(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def cv1_weights(c, seed=1):
    rng = np.random.default_rng(seed)
    return fp16_numbers(rng.normal(0.0, 1.0 / np.sqrt(2 * c), (2 * c, 2 * c, 1, 1))), rng.normal(0.0, 0.2, 2 * c).astype(np.float32)


def probe_graph(c, choff=0, *, w2=None, second_reader=False, b1_add=0.0):
    w, b = P.stem_weights(c)
    w1, b1 = P.layer1_weights(c)
    g = G.Graph(task=G.TASK_DETECT, nc=1, dtype=G.DTYPE_H2)
    l1 = g.buf(1, c)
    P.append_stem(g, w, b, (l1, 0))
    y = g.buf(2, 2 * c)
    g.conv((l1, 0, c), (y, 0), fp16_numbers(w1), b1 + np.float32(b1_add), 3, 2, G.ACT_SILU)
    wide = choff + 2 * c
    z = g.buf(2, wide)
    w2d, b2 = cv1_weights(c)
    g.conv((y, 0, 2 * c), (z, choff), w2d if w2 is None else w2, b2, 1, 1, G.ACT_SILU)
    if choff:            # the channels in front of the slice, from the slice itself
        rng = np.random.default_rng(2)
        g.conv((z, choff, 2 * c), (z, 0), fp16_numbers(rng.normal(0.0, 0.1, (choff, 2 * c, 1, 1))), np.zeros(choff, np.float32), 1, 1, G.ACT_NONE)
    width = P.READOUT + 4 * wide
    head3 = g.buf(3, width)
    g.conv((z, 0, wide), (head3, P.READOUT), P.unshuffle_weight(wide), np.zeros(4 * wide, np.float32), 3, 2, G.ACT_NONE)
    if second_reader:    # layer 1's map read once more: into a scratch buffer nobody reads
        g.conv((y, 0, 2 * c), (g.buf(2, 16), 0), np.zeros((16, 2 * c, 1, 1), np.float32), np.zeros(16, np.float32), 1, 1, G.ACT_NONE)
    P._finish_heads(g, (z, 0, wide), head3, width)
    return g


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(eng, m, frames, tuning, fill=True):
    """-> (level-3 head, last_stem_path, overflow flag) of one inference under ``tuning``."""
    eng.set_tuning(**tuning)
    m.take_overflow()
    head, _ = infer(m, frames, fill=fill)
    return head, m.last_stem_path(), m.take_overflow()


def both(eng, g, frames):
    m = E.Model(eng, g)
    try:
        off = run(eng, m, frames, {**ON, "fuse_stem_cv1": 0})
        on = run(eng, m, frames, ON)
    finally:
        eng.set_tuning(**ON)
        m.close()
    return off, on


@pytest.mark.parametrize("c,shape,choff", CASES, ids=IDS)
def test_fused_cv1_equals_its_own_launch(gpu_engine, c, shape, choff):
    require_premise(gpu_engine, "h2-behind-layer1")
    g = probe_graph(c, choff)
    assert g.ops[1]["flags"] & G.FLAG_W_SINGLE and g.ops[2]["flags"] & G.FLAG_W_SINGLE and g.ops[2]["out_choff"] == choff
    frames = P.probe_frames(*SHAPES[shape])
    (h0, p0, f0), (h1, p1, f1) = both(gpu_engine, g, frames)
    assert p0 == 0, "fuse_stem_cv1 = 0 and the fused path ran"
    assert p1 == 1, "the fused path did not run"
    assert not f0 and not f1, "overflow flag with ordinary weights"
    assert not np.isnan(h0).any() and not np.isnan(h1).any(), "a head byte that was not written, or a read of the NaN-filled arena"
    d = int((bits(h0) != bits(h1)).sum())
    print(f"c{c} {shape} choff {choff}: {d} of {h0.size} head values differ, largest |value| {np.abs(h0[..., P.READOUT:]).max():.3f}")
    assert d == 0, f"{d} of {h0.size} values of the 1x1's buffer differ bitwise between the fused kernel and the separate launch"
    assert np.abs(h0[..., P.READOUT:]).max() > 0.05, "the readout carries the 1x1's values"


def test_fused_path_stays_off(gpu_engine):
    c, frames = 32, P.probe_frames(*SHAPES["whole-tiles"])
    eng = gpu_engine
    # profiling: the conv keeps its row
    g = probe_graph(c)
    m = E.Model(eng, g)
    try:
        want, p, _ = run(eng, m, frames, ON)
        assert p == 1
        eng.set_profiling(True)
        got, p, _ = run(eng, m, frames, ON)
        rows = n_conv_rows(m)
        eng.set_profiling(False)
        assert p == 0, "the fused path ran under profiling"
        assert rows == sum(1 for o in g.ops if o["kind"] == G.OP_CONV) - 1, "profile rows: every conv but layer 1 (inside the stem's row)"
        assert np.array_equal(bits(got), bits(want))
        again, p, _ = run(eng, m, frames, ON)
        assert p == 1 and np.array_equal(bits(again), bits(want)), "profiling off again: the fused path is back"
    finally:
        eng.set_profiling(False)
        eng.set_tuning(**ON)
        m.close()
    # a second reader of layer 1's map; a 1x1 whose weights are no fp16 numbers (three products)
    w2 = cv1_weights(c)[0] * np.float32(1.0 + 2.0 ** -14)
    for name, g in (("second reader", probe_graph(c, second_reader=True)), ("three-product 1x1", probe_graph(c, w2=w2))):
        if name == "three-product 1x1":
            assert not g.ops[2]["flags"] & G.FLAG_W_SINGLE
        (h0, p0, _), (h1, p1, _) = both(eng, g, frames)
        assert p0 == 0 and p1 == 0, f"{name}: the fused path ran"
        assert not np.isnan(h1).any() and np.array_equal(bits(h0), bits(h1))


@pytest.mark.parametrize("scale", ["m", "s", "n"])
def test_yolov8_detections_bitwise(gpu_engine, scale):
    eng = gpu_engine
    h, w = 180, 320
    frames = synth.synthetic_frames(2, h, w, seed=9)
    sd = yolo_arch.synth_state_dict(scale, 80, None, seed=3, cls_bias=-1.0)
    m = E.Model(eng, G.build_yolov8(sd, 80, None, dtype="h2"))
    m.set_max_batch(2)
    kw = dict(imgsz=288, conf=0.25, iou=0.7)
    got = {}
    try:
        for v in (0, 1):
            eng.set_tuning(**{**ON, "fuse_stem_cv1": v})
            b, _, cnt = m.yolo_infer(frames, 2, h, w, **kw)
            got[v] = (np.array(b), np.array(cnt), m.last_stem_path(), [m.read_head(l, 2) for l in range(3)], m.take_overflow())
    finally:
        eng.set_tuning(**ON)
        m.close()
    (b0, c0, p0, h0, f0), (b1, c1, p1, h1, f1) = got[0], got[1]
    assert (p0, p1) == (0, 1), "which path ran"
    assert not f0 and not f1
    assert int(c0.sum()) > 0, "no detections to compare"
    assert np.array_equal(c0, c1) and np.array_equal(bits(b0), bits(b1)), "detections differ"
    for l in range(3):
        assert np.isfinite(h1[l]).all() and np.array_equal(bits(h0[l]), bits(h1[l])), f"head {l} differs"


def test_probe_overflow_raises_the_flag_on_both_paths(gpu_engine):
    """Layer 1's bias + 7e4 in one channel: silu(7e4) does not fit a pair — the phase-2 epilogue's own range check."""
    c = 32
    add = np.zeros(2 * c, np.float32)
    add[5] = P.BIG_BIAS
    (_, p0, f0), (_, p1, f1) = both(gpu_engine, probe_graph(c, b1_add=add), P.probe_frames(*SHAPES["partial-column"]))
    assert (p0, p1) == (0, 1)
    assert f0 and f1, f"the flag stayed down (separate launch: {f0}, fused: {f1})"


def test_overflowing_checkpoint_repeats_on_bx3_like_unfused(gpu_engine, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(E, "fp32_mode", lambda: "h2")
    eng = gpu_engine
    sd = yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5)
    f = np.float32(2.0 ** 18)                        # in the BatchNorms: the conv weights stay the fp16 numbers they are (two-product layers)
    sd["model.1.bn.weight"] = sd["model.1.bn.weight"] * f
    sd["model.1.bn.bias"] = sd["model.1.bn.bias"] * f
    sd["model.2.cv1.bn.weight"] = sd["model.2.cv1.bn.weight"] / f          # (brings the rest of the network back to ordinary magnitudes)
    path = str(tmp_path / "hot.pt")
    checkpoint.save_checkpoint(path, sd, "detect", 80, None, "n", {0: "person"})
    frames = synth.synthetic_frames(2, 90, 160, seed=5)
    args = (frames, 0.25, 0.7, 160)

    def copy_result(r):
        return tuple(None if a is None else np.array(a) for a in r[:3]) + tuple(r[3:])

    got = {}
    try:
        for v in (0, 1):
            eng.set_tuning(**{**ON, "fuse_stem_cv1": v})
            y = yolo.YOLO(path, engine=eng, fp32_mode="h2")
            y.set_max_batch(2)
            assert y.graph.ops[1]["flags"] & G.FLAG_W_SINGLE and y.graph.ops[2]["flags"] & G.FLAG_W_SINGLE
            m = E.Model(eng, y.graph)                # the h2 model itself: which path, and its flag
            m.set_max_batch(2)
            m.yolo_infer(frames, 2, 90, 160, imgsz=160, conf=0.25, iou=0.7, letterbox_auto=True)
            assert m.last_stem_path() == v
            assert m.take_overflow(), f"fuse_stem_cv1 = {v}: layer 1's output leaves the fp16 range and the flag stayed down"
            m.close()
            got[v] = copy_result(y.infer_frames(*args, channel_reverse=False))
            assert y.fell_back and y.fp32_mode == "bx3", f"fuse_stem_cv1 = {v}: the call was not repeated on bf16x3"
            y.close()
        assert capsys.readouterr().out.count("beyond the fp16 range") == 2
        ref = yolo.YOLO(path, engine=eng, fp32_mode="bx3")
        ref.set_max_batch(2)
        want = copy_result(ref.infer_frames(*args, channel_reverse=False))
        ref.close()
    finally:
        eng.set_tuning(**ON)
    for v in (0, 1):
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got[v][:3], want[:3])), f"fuse_stem_cv1 = {v}: not the bf16x3 results"
