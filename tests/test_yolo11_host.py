"""YOLO11 on the host, no GPU: the architecture table against the published known answers, family / scale inference, the op list
of ``graph.build_yolo11`` interpreted on the CPU against the torch restatement (tests/yolo11_ref.py), the checkpoint plumbing
(family field, Ultralytics-shaped pickle) and the synthetic checkpoint's attention statistics."""
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import yolov8_ref as ref
from padel_analytics_amd import checkpoint, graph as G, yolo_arch as ya
from padel_analytics_amd.yolo import YOLO
from tests import synth, yolo11_interp, yolo11_synth
from tests.yolo11_ref import Yolo11Ref

# published model table (ultralytics docs, YOLO11 detect at 640^2, nc = 80): exact parameter counts and GFLOPs to two decimals as
# the restated structure gives them; the table prints 2.6 / 9.4 / 20.1 / 25.3 / 56.9 M and 6.5 / 21.5 / 68.0 / 86.9 / 194.9
KNOWN = {"n": (2_624_080, 6.48), "s": (9_458_752, 21.47), "m": (20_114_688, 67.98), "l": (25_372_160, 86.91), "x": (56_966_176, 194.90)}
KNOWN_POSE = {"n": 2_874_462, "m": 20_912_364}          # 17 x 3 keypoints, nc = 1: published 2.9 M and 20.9 M


@pytest.mark.parametrize("scale", list(KNOWN))
def test_published_parameter_counts_and_gflops(scale):
    params, gflops = KNOWN[scale]
    assert ya.count_parameters(ya.yolo11_state_spec(scale, 80)) == params
    assert round(ya.conv_flops11(ya.conv_inventory11(scale, 80, None, 640, 640)) / 1e9, 2) == gflops


@pytest.mark.parametrize("scale", list(KNOWN_POSE))
def test_published_pose_parameter_counts(scale):
    assert ya.count_parameters(ya.yolo11_state_spec(scale, 1, (17, 3))) == KNOWN_POSE[scale]


def _shapes_only(spec):
    return {k: np.zeros(shp, np.float32) for k, shp in spec.items()}


@pytest.mark.parametrize("kpt", [None, (13, 3)])
@pytest.mark.parametrize("scale", list(KNOWN))
def test_family_and_scale_are_inferred(scale, kpt):
    nc = 1 if kpt else 80
    sd = _shapes_only(ya.yolo11_state_spec(scale, nc, kpt))
    assert ya.infer_family(sd) == "yolo11"
    assert ya.infer_model(sd) == {"family": "yolo11", "scale": scale, "nc": nc, "nk": 39 if kpt else 0}
    v8 = _shapes_only(ya.yolov8_state_spec(scale, nc, kpt))
    assert ya.infer_model(v8) == {"family": "yolov8", "scale": scale, "nc": nc, "nk": 39 if kpt else 0}


def _head_maps(model, x):
    with torch.no_grad():
        det, kp = model.head_raw(model.features(x))
    return [d if not kp else torch.cat([d, kp[l]], 1) for l, d in enumerate(det)]


# n: c3k False in the shallow blocks, a padded 8-channel bottleneck at model.2; m: c3k True everywhere, 4 heads; l: two PSABlocks
@pytest.mark.parametrize("dtype", ["f32", "h2"])
@pytest.mark.parametrize("scale,nc,kpt", [("n", 80, None), ("n", 1, (13, 3)), ("m", 2, None), ("l", 1, None)])
def test_op_list_equals_the_oracle(scale, nc, kpt, dtype):
    sd = ya.synth_state_dict11(scale, nc, kpt, seed=1, gain=1.0)
    g = G.build_yolo11(sd, nc, kpt, dtype=dtype)
    d = ya.arch11_dims(scale)
    assert sum(o["kind"] == G.OP_PSA_ATTN for o in g.ops) == d.n and sum(o["kind"] == G.OP_DWCONV3 for o in g.ops) == d.n + 6
    x = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(4))
    bufs = yolo11_interp.run(g, x)
    dirty = yolo11_interp.run(g, x, stale=1000.0)
    want = _head_maps(Yolo11Ref(sd, nc, kpt), x)
    for l in range(3):
        got = bufs[g.head_buf[l]][:, :want[l].shape[1]]
        assert float((got - want[l]).abs().max()) <= 2e-5 * max(1.0, float(want[l].abs().max())), l
        assert torch.equal(dirty[g.head_buf[l]][:, :want[l].shape[1]], got), "stale pad channels leaked into the head"
    for o in g.ops:
        lvl, ch = g.bufs[o["in_buf"]]
        if o["kind"] in (G.OP_CONV, G.OP_DWCONV3, G.OP_PSA_ATTN):
            assert o["cin"] % 16 == 0 and o["in_choff"] % 16 == 0 and o["in_choff"] + o["cin"] <= ch
            assert o["out_choff"] % 4 == 0 or o["out_buf"] in g.head_buf          # (fp32 head maps take any channel offset)
    if dtype == "h2":           # fp16-number weights stay unfolded: every conv of the graph runs two products per operand pair
        assert all(o["flags"] & G.FLAG_W_SINGLE for o in g.ops if o["kind"] == G.OP_CONV)


def test_class_branch_width_that_is_no_multiple_of_16():
    """nc = 90 at the n scale: c3 = max(64, min(90, 100)) = 90 channels through the depthwise conv, padded to 96."""
    sd = ya.synth_state_dict11("n", 90, None, seed=2, gain=1.0)
    assert sd["model.23.cv3.0.1.0.conv.weight"].shape == (90, 1, 3, 3)
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(5))
    want = _head_maps(Yolo11Ref(sd, 90, None), x)
    for dtype in ("f32", "h2"):
        g = G.build_yolo11(sd, 90, None, dtype=dtype)
        assert {o["cin"] for o in g.ops if o["kind"] == G.OP_DWCONV3} >= {96}
        bufs = yolo11_interp.run(g, x, stale=777.0)
        for l in range(3):
            got = bufs[g.head_buf[l]][:, :154]
            assert float((got - want[l]).abs().max()) <= 2e-5 * max(1.0, float(want[l].abs().max())), (dtype, l)


def test_qkv_rows_are_permuted_to_q_k_v_planes():
    sd = ya.synth_state_dict11("n", 1, None, seed=3)
    g = G.build_yolo11(sd, 1, None)
    att = next(o for o in g.ops if o["kind"] == G.OP_PSA_ATTN)
    assert (att["stride"], att["ksize"], att["npad"], att["cin"], att["cout"]) == (2, 32, 64, 256, 128)
    pe = g.ops[g.ops.index(att) + 1]
    assert pe["kind"] == G.OP_DWCONV3 and pe["in_buf"] == att["in_buf"] and pe["in_choff"] == 128 and pe["res_buf"] == att["out_buf"]


# ---------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_carries_the_family(tmp_path):
    p11, p8 = tmp_path / "y11.pt", tmp_path / "y8.pt"
    checkpoint.make_synthetic_yolo(p11, "n", 1, None, seed=0, family="yolo11")
    checkpoint.make_synthetic_yolo(p8, "n", 1, None, seed=0)
    assert checkpoint.load_checkpoint(p11).family == "yolo11" and checkpoint.load_checkpoint(p8).family == "yolov8"
    obj = torch.load(str(p8), weights_only=True)
    del obj["family"]                                  # a file written before the field existed
    torch.save(obj, str(p8))
    assert checkpoint.load_checkpoint(p8).family == "yolov8"
    y = YOLO(p11)                                      # builds the op list; no device is touched before the first inference
    assert y.family == "yolo11" and any(o["kind"] == G.OP_PSA_ATTN for o in y.graph.ops)
    assert not any(o["kind"] == G.OP_PSA_ATTN for o in YOLO(p8).graph.ops)


def test_half_is_refused_with_the_reason(tmp_path):
    p = tmp_path / "y11.pt"
    checkpoint.make_synthetic_yolo(p, "n", 1, None, seed=0, family="yolo11")
    with pytest.raises(ValueError, match="fp16 storage is not implemented"):
        YOLO(p, half=True)
    y = YOLO(p)
    with pytest.raises(ValueError, match="fp16 storage is not implemented"):
        y.set_half(True)
    assert y.half is False and y.graph.dtype != G.DTYPE_F16


def _ultralytics_tree(sd, pose):
    """A fake ``ultralytics`` package and an nn.Module tree of its classes that reproduces ``sd`` in fp16, with the class names a
    YOLO11 pickle carries: C3k2, C3k, C2PSA, PSABlock, Attention, DWConv, Bottleneck, Conv, SPPF, Detect / Pose."""
    pkg, nnm = types.ModuleType("ultralytics"), types.ModuleType("ultralytics.nn")
    tasks, mods = types.ModuleType("ultralytics.nn.tasks"), types.ModuleType("ultralytics.nn.modules")
    klass = {}
    for n in ("Conv", "DWConv", "C3k2", "C3k", "C2PSA", "PSABlock", "Attention", "Bottleneck", "SPPF", "Detect", "Pose", "DFL", "Sequential"):
        klass[n] = type(n, (nn.Module,), {"__module__": mods.__name__})
        setattr(mods, n, klass[n])
    for n in ("DetectionModel", "PoseModel"):
        klass[n] = type(n, (nn.Module,), {"__module__": tasks.__name__})
        setattr(tasks, n, klass[n])
    sys.modules.update({"ultralytics": pkg, "ultralytics.nn": nnm, "ultralytics.nn.tasks": tasks, "ultralytics.nn.modules": mods})
    d_c3k2 = {"2", "4", "6", "8", "13", "16", "19", "22"}

    def kind(path):
        """Class of the module at ``path`` (names below the root), as upstream nests them."""
        name, i, rest = path[-1], path[1] if len(path) > 1 else "", path[2:]
        if len(path) == 2:                       # model.{i}
            return "C3k2" if i in d_c3k2 else "C2PSA" if i == "10" else "SPPF" if i == "9" else ("Pose" if pose else "Detect") if i == "23" else "Conv"
        if i in d_c3k2 and len(rest) == 2 and rest[0] == "m":
            return "C3k" if f"model.{i}.m.0.cv3.conv.weight" in sd else "Bottleneck"
        if i in d_c3k2 and len(rest) == 4 and rest[2] == "m":
            return "Bottleneck"
        if i == "10" and len(rest) == 2 and rest[0] == "m":
            return "PSABlock"
        if name == "attn":
            return "Attention"
        if name == "dfl":
            return "DFL"
        if f"{'.'.join(path)}.conv.weight" in sd:          # conv + bn pairs: DWConv in the head's class branch, Conv elsewhere
            return "DWConv" if i == "23" and rest[0] == "cv3" and len(rest) == 4 and rest[3] == "0" else "Conv"
        return "Sequential"                      # model, m, ffn, cv2 / cv3 / cv4 of the head and their numbered children

    root = klass["PoseModel" if pose else "DetectionModel"]()

    def child(parent, path):
        name = path[-1]
        if name not in parent._modules:
            parent.add_module(name, nn.Module() if name in ("conv", "bn") else klass[kind(path)]())
        return parent._modules[name]

    for key, val in sd.items():
        parts = key.split(".")
        node = root
        for i in range(len(parts) - 1):
            node = child(node, tuple(parts[:i + 1]))
        t = torch.from_numpy(np.asarray(val))
        t = t.half() if t.is_floating_point() else t
        if parts[-1] in ("weight", "bias"):
            node.register_parameter(parts[-1], nn.Parameter(t, requires_grad=False))
        else:
            node.register_buffer(parts[-1], t)
    return root


@pytest.mark.parametrize("scale,nc,kpt", [("n", 80, None), ("m", 1, (13, 3))])
def test_ultralytics_shaped_yolo11_pickle_loads(tmp_path, scale, nc, kpt):
    sd = ya.synth_state_dict11(scale, nc, kpt, seed=3)
    try:
        model = _ultralytics_tree(sd, pose=kpt is not None)
        names = {type(m).__name__ for m in model.modules()}
        assert {"C3k2", "C3k", "C2PSA", "PSABlock", "Attention", "DWConv"} <= names
        model.yaml = {"nc": nc, "scale": scale, **({"kpt_shape": list(kpt)} if kpt else {})}
        model.names = {i: f"c{i}" for i in range(nc)}
        path = tmp_path / "yolo11_fake.pt"
        torch.save({"epoch": -1, "model": model, "ema": None, "train_args": {"imgsz": 640}, "version": "8.3.0"}, str(path))
    finally:
        for k in [k for k in sys.modules if k == "ultralytics" or k.startswith("ultralytics.")]:
            del sys.modules[k]
    with pytest.raises(Exception):
        torch.load(str(path), map_location="cpu", weights_only=True)
    got = checkpoint.load_checkpoint(path)
    assert (got.family, got.scale, got.nc, got.task) == ("yolo11", scale, nc, "pose" if kpt else "detect")
    assert got.kpt_shape == (tuple(kpt) if kpt else None) and set(got.state_dict) == set(sd)
    for k, v in sd.items():
        assert np.array_equal(got.state_dict[k], np.asarray(v)), k          # (the synthetic values are fp16 numbers already)
    y = YOLO(path)
    assert y.family == "yolo11" and y.graph.nc == nc and len(y.graph.ops) > 80


# ---------------------------------------------------------------------------------------- the synthetic checkpoint
def test_attention_rows_of_the_synthetic_checkpoint_are_neither_uniform_nor_one_hot():
    """On the test clip (2 synthetic 720p frames letterboxed to 384 x 640: 240 tokens) the per-row standard deviation of the scaled
    attention logits, median over rows and heads, lies in [0.5, 8]: a uniform softmax (std -> 0) or a one-hot one (std >> 8) would
    let a wrong attention kernel pass the end-to-end tests.  Arithmetic: 32 products of unit-variance q and k x 32^-1/2 x gamma^2,
    gamma ~ U(.8, 1.6), gives 1-2."""
    frames = synth.synthetic_frames(2, 720, 1280, seed=3)
    x = ref.preprocess([f[..., ::-1] for f in frames], 640)
    sd = yolo11_synth.calibrated_state_dict("n", 80, None, x, 0.5, seed=5)
    m = Yolo11Ref(sd, 80, None)
    m.attn_logits = []
    with torch.no_grad():
        det, _ = m.head_raw(m.features(x))
    assert len(m.attn_logits) == 1 and m.attn_logits[0].shape == (2, 2, 240, 240)
    med = float(m.attn_logits[0].std(dim=-1).median())
    print(f"attention logits: median per-row std {med:.3f}")
    assert 0.5 <= med <= 8.0, med
    # and the class bias leaves about 1 % of the anchors above the threshold
    frac = float(np.mean([float((d[:, 64:].sigmoid().amax(1) > 0.5).float().mean()) for d in det]))
    assert 0.002 <= frac <= 0.05, frac
