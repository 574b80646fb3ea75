"""The fused head tail (csrc/head_tail_h2.hip, tuning ``fuse_head``, on by default): the heads' last 1x1 convs and the decode as one
kernel — bitwise the detections of the convs followed by ``decode_kernel``.

Graphs (h2, synthetic weights): yolov8n detect nc 80 (class conv 80 -> 80: K = 2 chunks + a 16-channel tail, five class fragments),
yolov8m detect nc 80 (192 -> 80), yolov8m pose (13, 3) (64 -> 64, 192 -> 1, 48 -> 39: 32 + 16 tail) and yolov8n pose (17, 3)
(64 -> 51).  The m graphs carry fp16-number weights (two products per operand pair, PA_CONV_W_SINGLE), the n graphs weights that are
no fp16 numbers (three products, a non-zero m plane): asserted on the tail ops' flags.

Shapes, batch 3: imgsz 64 (64 + 16 + 4 anchors per image: partial fragments on P4 and P5, a fragment that spans images), imgsz 96 with
a square source (P3 = 144 anchors) and with a 160 x 96 source (a 64 x 96 net: rows of 12, 6 and 3 anchors).  The arena is filled with
0xA5 before every run, so a read of something nobody wrote shows as a difference."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, graph as G, yolo_arch
from tests import synth

pytestmark = pytest.mark.gpu

B = 3
MODELS = {                      # name -> (scale, nc, kpt, fp16-number weights)
    "n-detect80-3p": ("n", 80, None, False),
    "m-detect80-2p": ("m", 80, None, True),
    "m-pose13-2p": ("m", 1, (13, 3), True),
    "n-pose17-3p": ("n", 1, (17, 3), False),
}
SHAPES = {"64sq": (64, 64, 64), "96sq": (96, 96, 96), "96x160": (96, 160, 96)}      # name -> (h, w, imgsz)
DEFAULT_CONF = 0.25
_graphs = {}


def graph_of(name):
    if name not in _graphs:
        scale, nc, kpt, half = MODELS[name]
        sd = yolo_arch.synth_state_dict(scale, nc, kpt, seed=7, cls_bias=-1.0)
        conv_w = lambda k, v: k.endswith(".weight") and np.asarray(v).ndim == 4
        if half:        # fp16 numbers, like a checkpoint's: the packed m plane is zero
            sd = {k: (np.asarray(v).astype(np.float16).astype(np.float32) if conv_w(k, v) else v) for k, v in sd.items()}
        else:           # no fp16 numbers: 1.0003 moves every weight off the fp16 grid, the m plane carries the rest
            sd = {k: ((np.asarray(v, np.float32) * np.float32(1.0003)).astype(np.float32) if conv_w(k, v) else v) for k, v in sd.items()}
        g = G.build_yolov8(sd, nc, kpt, dtype="h2")
        tail = [o for o in g.ops if o["out_buf"] in g.head_buf]
        assert len(tail) == (9 if kpt else 6)
        assert all(bool(o.get("flags", 0) & G.FLAG_W_SINGLE) == half for o in tail), "the weights did not give the product form this case is about"
        _graphs[name] = g
    return _graphs[name]


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same(r0, r1):
    (b0, k0, c0), (b1, k1, c1) = r0, r1
    ok = np.array_equal(c0, c1) and np.array_equal(u32(b0), u32(b1))
    if k0 is not None:
        ok = ok and np.array_equal(u32(k0), u32(k1))
    return ok


def model_for(eng, name, frames, h, w, imgsz):
    """A model of graph ``name`` with its plan made (one call): ``fill_arena`` needs one."""
    m = E.Model(eng, graph_of(name))
    m.set_max_batch(B)
    m.yolo_infer(frames, B, h, w, imgsz=imgsz, conf=DEFAULT_CONF, iou=0.7)
    return m


def run(eng, m, frames, h, w, fuse, **kw):
    eng.set_tuning(fuse_head=fuse)
    m.fill_arena(0xA5)
    b, k, c = m.yolo_infer(frames, B, h, w, iou=0.7, **kw)
    return (b.copy(), None if k is None else k.copy(), c.copy()), m.last_post_path()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("model", sorted(MODELS))
def test_fused_head_tail_matches_convs_and_decode(gpu_engine, model, shape):
    h, w, imgsz = SHAPES[shape]
    g = graph_of(model)
    frames = synth.synthetic_frames(B, h, w, seed=21)
    m = model_for(gpu_engine, model, frames, h, w, imgsz)
    cases = [dict(conf=1e-4), dict(conf=DEFAULT_CONF), dict(conf=1.0), dict(conf=1e-4, max_det=1), dict(conf=DEFAULT_CONF, max_det=1)]
    if g.nc == 80:
        cases += [dict(conf=1e-4, classes=[0, 3, 79]), dict(conf=DEFAULT_CONF, classes=[5])]
    A = sum((s[0] * s[1]) for s in m.head_shapes(h, w, imgsz))
    try:
        for kw in cases:
            r1, p1 = run(gpu_engine, m, frames, h, w, 1, imgsz=imgsz, **kw)
            heads1 = [m.read_head(l, B) for l in range(3)] if kw == cases[0] else None
            again = [m.read_head(l, B) for l in range(3)] if kw == cases[0] else None
            r0, p0 = run(gpu_engine, m, frames, h, w, 0, imgsz=imgsz, **kw)
            assert (p1, p0) == (E.POST_PATH_FUSED, E.POST_PATH_DECODE), (model, shape, kw)
            assert not m.take_overflow()
            print(f"{model} {shape} {kw}: counts fused {r1[2].tolist()} unfused {r0[2].tolist()} of {A} anchors")
            assert same(r0, r1), (model, shape, kw)
            if kw["conf"] >= 1.0:          # sigmoid <= 1: nothing passes
                assert int(r0[2].sum()) == 0
            if kw["conf"] < 0.01 and "classes" not in kw:
                assert int(r0[2].min()) >= 1
            if heads1 is not None:
                heads0 = [m.read_head(l, B) for l in range(3)]
                for l in range(3):
                    assert np.array_equal(u32(heads0[l]), u32(heads1[l])), f"{model} {shape}: head {l} read after a fused call differs"
                    assert np.array_equal(u32(again[l]), u32(heads1[l])), f"{model} {shape}: second read of head {l} differs"
                    assert np.isfinite(heads1[l][..., :64 + g.nc + g.nk]).all()
    finally:
        gpu_engine.set_tuning(fuse_head=1)           # the default
        m.close()


def test_nearly_every_anchor_passes_at_the_low_conf(gpu_engine):
    """The low-conf case is about a full candidate list: checked on the head map (every class-0 logit above the threshold's) for the
    pose graph, whose only class every anchor scores."""
    h, w, imgsz = SHAPES["96sq"]
    frames = synth.synthetic_frames(B, h, w, seed=21)
    m = model_for(gpu_engine, "m-pose13-2p", frames, h, w, imgsz)
    try:
        run(gpu_engine, m, frames, h, w, 1, imgsz=imgsz, conf=1e-4)
        heads = [m.read_head(l, B) for l in range(3)]
    finally:
        gpu_engine.set_tuning(fuse_head=1)
        m.close()
    logits = np.concatenate([x[..., 64].reshape(B, -1) for x in heads], 1)
    assert logits.shape[1] == 144 + 36 + 9
    assert float((1 / (1 + np.exp(-logits.astype(np.float64))) > 1e-4).mean()) > 0.95


def test_submit_wait_with_conf_changing_between_tickets(gpu_engine):
    """conf is a plain kernel argument outside the captured graph: tickets A, B, A on one model, queued back to back."""
    h, w, imgsz = SHAPES["96x160"]
    frames = synth.synthetic_frames(B, h, w, seed=22)
    m = model_for(gpu_engine, "m-pose13-2p", frames, h, w, imgsz)
    buf = gpu_engine.alloc(frames.nbytes).upload(frames)
    confs = (DEFAULT_CONF, 1e-4, DEFAULT_CONF)
    out = {}
    try:
        for graph in (0, 1):
            for fuse in (1, 0):
                gpu_engine.set_tuning(fuse_head=fuse, graph=graph)
                m.fill_arena(0xA5)
                ts = [m.yolo_submit(buf, B, h, w, imgsz=imgsz, conf=c, iou=0.7, pre_mode=E.PRE_LETTERBOX) for c in confs]
                path = m.last_post_path()
                res = []
                for t in ts:
                    b, k, c, ovf = m.yolo_wait(t)
                    assert not ovf
                    res.append((b.copy(), k.copy(), c.copy()))
                assert path == (E.POST_PATH_FUSED if fuse else E.POST_PATH_DECODE)
                out[graph, fuse] = res
    finally:
        gpu_engine.set_tuning(fuse_head=1, graph=0)
        m.close()
        buf.free()
    ref = out[0, 0]
    assert int(ref[1][2].sum()) > int(ref[0][2].sum()), "the two thresholds select the same candidates: the case says nothing"
    assert same(ref[0], ref[2])
    for key, res in out.items():
        for i in range(3):
            assert same(ref[i], res[i]), (key, i)


def test_path_export(gpu_engine):
    """1 on fused calls; 0 with fuse_head = 0, while profiling, on an fp16 model and after pa_yolo_postprocess."""
    h, w, imgsz = SHAPES["64sq"]
    frames = synth.synthetic_frames(B, h, w, seed=23)
    kw = dict(imgsz=imgsz, conf=DEFAULT_CONF, iou=0.7)
    g = graph_of("n-detect80-3p")
    m = E.Model(gpu_engine, g)
    m.set_max_batch(B)
    scale, nc, kpt, _ = MODELS["n-detect80-3p"]
    m16 = E.Model(gpu_engine, G.build_yolov8(yolo_arch.synth_state_dict(scale, nc, kpt, seed=7, cls_bias=-1.0), nc, kpt, dtype="f16"))
    m16.set_max_batch(B)
    try:
        gpu_engine.set_tuning(fuse_head=1)
        assert m.last_post_path() == E.POST_PATH_DECODE          # nothing has run
        r1 = m.yolo_infer(frames, B, h, w, **kw)
        assert m.last_post_path() == E.POST_PATH_FUSED
        gpu_engine.set_profiling(True)
        rp = m.yolo_infer(frames, B, h, w, **kw)
        assert m.last_post_path() == E.POST_PATH_DECODE
        rows = [(r["kind"], r["ksize"], r["M"], r["cout"], r["cin"]) for r in m.profile_rows()]
        gpu_engine.set_tuning(fuse_head=0)
        m.yolo_infer(frames, B, h, w, **kw)
        assert rows == [(r["kind"], r["ksize"], r["M"], r["cout"], r["cin"]) for r in m.profile_rows()]       # the profile keeps its rows
        assert sum(1 for r in rows if r[0] == G.OP_CONV and r[1] == 1 and r[3] in (64, 80)) >= 6 and rows[-2][0] == E.PROF_DECODE
        gpu_engine.set_tuning(fuse_head=1)
        gpu_engine.set_profiling(False)
        m.yolo_infer(frames, B, h, w, **kw)
        assert m.last_post_path() == E.POST_PATH_FUSED
        heads = [m.read_head(l, B) for l in range(3)]
        rpp = m.yolo_postprocess(heads, h, w, **kw)
        assert m.last_post_path() == E.POST_PATH_DECODE
        gpu_engine.set_tuning(fuse_head=0)
        r0 = m.yolo_infer(frames, B, h, w, **kw)
        assert m.last_post_path() == E.POST_PATH_DECODE
        gpu_engine.set_tuning(fuse_head=1)
        m16.yolo_infer(frames, B, h, w, **kw)
        assert m16.last_post_path() == E.POST_PATH_DECODE
    finally:
        gpu_engine.set_profiling(False)
        gpu_engine.set_tuning(fuse_head=1)
        m.close()
        m16.close()
    assert same(r0, r1) and same(r0, rp) and same(r0, rpp)
