"""Court-keypoint ResNet-50, everything that needs no GPU: the oracle pinned by known answers, the preprocessing tables pinned
to Pillow byte for byte, the graph builder against the oracle's structure, the tracker's host logic over a stub model, and
the two conditions the synthetic checkpoint must meet for the GPU parity test to mean anything."""
import json

import numpy as np
import pytest
import torch

from padel_analytics_amd import engine as E, graph as G
from tests import resnet_ref as R


# ---------------------------------------------------------------------------------------- oracle: known answers
def test_oracle_parameter_counts_are_the_published_ones():
    assert R.count_params(1000) == 25_557_032                       # torchvision's resnet50
    assert R.count_params(24) == 23_557_208 == 25_557_032 - 2_049_000 + 49_176


def test_oracle_macs_round_to_the_published_figure():
    assert round(R.macs(1000, 224) / 1e9, 2) == 4.09


def test_oracle_state_dict_keys_and_shapes():
    sh = R.state_dict_shapes(24)
    assert sh["conv1.weight"] == (64, 3, 7, 7) and sh["fc.weight"] == (24, 2048) and sh["fc.bias"] == (24,)
    assert sh["layer1.0.downsample.0.weight"] == (256, 64, 1, 1) and sh["layer4.0.downsample.0.weight"] == (2048, 1024, 1, 1)
    assert sh["layer3.5.conv2.weight"] == (256, 256, 3, 3) and sh["layer4.2.bn3.running_var"] == (2048,)
    assert "layer1.1.downsample.0.weight" not in sh and "layer3.6.conv1.weight" not in sh
    convs = [k for k in sh if k.endswith(".weight") and len(sh[k]) == 4]
    assert len(convs) == 53 and len(sh) == 53 * 5 + 2
    assert sh == G.resnet50_shapes(24)                              # the builder's own table: the same set


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_runs_in_both_precisions(dtype):
    rng = np.random.default_rng(3)
    sd = {k: (np.abs(rng.normal(1, 0.1, s)) if k.endswith("running_var") else rng.normal(0, 0.05, s)).astype(np.float32)
          for k, s in R.state_dict_shapes(24).items()}
    frames = rng.integers(0, 256, (1, 64, 80, 3), dtype=np.uint8)
    xy, z = R.predict(sd, frames, dtype)
    assert xy.shape == z.shape == (1, 24) and xy.dtype == {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    assert np.isfinite(z).all() and ((xy > 0) & (xy < 1)).all()


# ---------------------------------------------------------------------------------------- preprocessing: Pillow itself
def _replay_pass(img, out_size, axis):
    """One resample pass in numpy over the tables the device kernels use (22-bit fixed point, accumulator from 1 << 21)."""
    bounds, coefs = E.pil_coeffs(img.shape[axis], out_size, E.PIL_BILINEAR)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for o in range(out_size):
        lo, n = bounds[o]
        acc = (1 << 21) + np.tensordot(coefs[o, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


@pytest.mark.parametrize("wh", [(1280, 720), (1920, 1080), (854, 480), (333, 517)])
def test_bilinear_tables_equal_pillow_byte_for_byte(wh):
    from PIL import Image
    w, h = wh
    rng = np.random.default_rng(w + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: h // 3, : w // 3] = (img[: h // 3, : w // 3] // 128) * 255          # hard edges as well as noise
    got = _replay_pass(_replay_pass(img, 224, 1), 224, 0)                    # Pillow: horizontal pass first, then vertical
    want = np.asarray(Image.fromarray(img).resize((224, 224), Image.BILINEAR))
    assert np.array_equal(got, want), int((got != want).sum())


def test_bilinear_tap_counts():
    assert E.pil_coeffs(1920, 224, E.PIL_BILINEAR)[1].shape == (224, 19)
    assert E.pil_coeffs(1920, 224, E.PIL_BICUBIC)[1].shape[1] > 19           # the bicubic tables are untouched (support 2)


def test_normalisation_table_is_the_fp32_expression():
    t = G.resnet_norm_table()
    assert t.shape == (3, 256) and t.dtype == np.float32
    mean, std = (0.485, 0.465, 0.406), (0.229, 0.224, 0.225)                 # 0.465: the reference's value
    for c in range(3):
        for b in range(256):
            want = (np.float32(b) / np.float32(255) - np.float32(mean[c])) / np.float32(std[c])
            assert t[c, b] == want, (c, b)
    assert np.array_equal(t, R.norm_table())
    x = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    for c in range(3):
        assert np.array_equal(x.clone().sub_(torch.tensor(mean[c])).div_(torch.tensor(std[c])).numpy(), t[c])


# ---------------------------------------------------------------------------------------- graph builder
def _random_sd(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return {k: (np.abs(rng.normal(1, 0.1, s)) if k.endswith("running_var") else rng.normal(0, 0.05, s)).astype(np.float32)
            for k, s in shapes.items()}


@pytest.mark.parametrize("dtype", ["f32", "h2"])
def test_builder_structure_follows_the_oracle(dtype):
    sd = _random_sd(R.state_dict_shapes(24))
    g = G.build_resnet50(sd, dtype)
    assert g.task == G.TASK_RESNET
    kinds = [o["kind"] for o in g.ops]
    assert kinds[0] == G.OP_STEM7 and kinds[1] == G.OP_MAXPOOL3S2 and kinds[-1] == G.OP_GAP_FC
    assert kinds.count(G.OP_CONV) == 52 and len(kinds) == 55                 # 53 convs: conv1 is the stem op
    level = lambda b: g.bufs[b][0]
    assert level(g.ops[0]["out_buf"]) == 1 and level(g.ops[1]["out_buf"]) == 2
    ops = iter(g.ops[2:-1])
    flagged = 0
    for p, cin, planes, stride, down in R.blocks():
        c1, c2 = next(ops), next(ops)
        ds = next(ops) if down else None
        c3 = next(ops)
        assert (c1["ksize"], c1["stride"], c1["cin"], c1["cout"], c1["act"]) == (1, 1, cin, planes, G.ACT_RELU), p
        assert (c2["ksize"], c2["stride"], c2["cin"], c2["cout"], c2["act"]) == (3, stride, planes, planes, G.ACT_RELU), p
        assert (c3["ksize"], c3["stride"], c3["cin"], c3["cout"], c3["act"]) == (1, 1, planes, 4 * planes, G.ACT_RELU), p
        assert level(c2["out_buf"]) == level(c1["out_buf"]) + (stride == 2) == level(c3["out_buf"])
        assert not (c1["flags"] | c2["flags"]) & G.FLAG_RES_PREACT and c1["res_buf"] < 0 and c2["res_buf"] < 0
        assert c3["flags"] & G.FLAG_RES_PREACT and c3["res_buf"] >= 0, p
        flagged += 1
        if down:
            assert (ds["ksize"], ds["stride"], ds["cin"], ds["cout"], ds["act"]) == (1, stride, cin, 4 * planes, G.ACT_NONE), p
            assert not ds["flags"] & G.FLAG_RES_PREACT and c3["res_buf"] == ds["out_buf"]
        else:
            assert c3["res_buf"] == c1["in_buf"], p                           # the identity is the block's own input
    assert flagged == 16 and next(ops, None) is None
    assert [level(o["out_buf"]) for o in g.ops if o["kind"] == G.OP_CONV][-1] == 5
    fc = g.ops[-1]
    assert (fc["cin"], fc["cout"], fc["act"]) == (2048, 24, G.ACT_SIGMOID)
    blob = g.blob()
    assert np.array_equal(blob[fc["w_off"]:fc["w_off"] + 24 * 2048].reshape(24, 2048), sd["fc.weight"])
    st = g.ops[0]
    assert np.array_equal(blob[st["reserved"]:st["reserved"] + 768].reshape(3, 256), G.resnet_norm_table())
    w0, b0 = G.fold_bn({"x.conv.weight": sd["conv1.weight"], **{f"x.bn.{k}": sd[f"bn1.{k}"] for k in R.BN_KEYS}}, "x", 1e-5)
    wl = blob[st["w_off"]:st["w_off"] + 148 * 64].reshape(148, 64)
    assert np.array_equal(wl[(2 * 7 + 5) * 3 + 1], w0[:, 1, 2, 5]) and not wl[147].any()
    assert round(g.conv_flops(224, 224) / 2e9, 2) == round((R.macs(24) - 24 * 2048) / 1e9, 2)


def test_builder_refuses_other_networks():
    good = R.state_dict_shapes(24)
    resnet18 = {"conv1.weight": (64, 3, 7, 7), "fc.weight": (24, 512), "fc.bias": (24,)}
    for n, planes in enumerate((64, 128, 256, 512), 1):
        for i in range(2):
            resnet18[f"layer{n}.{i}.conv1.weight"] = (planes, planes, 3, 3)
            resnet18[f"layer{n}.{i}.conv2.weight"] = (planes, planes, 3, 3)
    with pytest.raises(ValueError, match="ResNet-50"):
        G.build_resnet50(_random_sd(resnet18))
    with pytest.raises(ValueError, match="ResNet-50"):
        G.build_resnet50(_random_sd(R.state_dict_shapes(1000)))              # the ImageNet head
    deeper = dict(good)
    deeper.update({k.replace("layer3.5", "layer3.6"): s for k, s in good.items() if k.startswith("layer3.5.")})   # towards resnet101
    with pytest.raises(ValueError, match="ResNet-50"):
        G.build_resnet50(_random_sd(deeper))
    sd = _random_sd(good)
    sd["bn1.num_batches_tracked"] = np.array(7)                              # what a real state_dict also carries
    assert len(G.build_resnet50(sd).ops) == 55


# ---------------------------------------------------------------------------------------- tracker host logic
class _StubModel:
    """Stands in for resnet.CourtResNet: output k of a frame is (frame[0, 0, 0] + k) / 512."""
    instances = []

    def __init__(self, path):
        self.path, self.batches, self.max_batch = path, [], None
        _StubModel.instances.append(self)

    def set_max_batch(self, n): self.max_batch = n

    def to(self, device): return self

    def infer(self, frames, n=None, h=None, w=None):
        frames = np.asarray(frames)
        self.batches.append(len(frames))
        return ((frames[:, 0, 0, 0].astype(np.float32)[:, None] + np.arange(24, dtype=np.float32)) / np.float32(512)).astype(np.float32)


@pytest.fixture
def stub_model(monkeypatch):
    from padel_analytics_amd import resnet
    _StubModel.instances = []
    monkeypatch.setattr(resnet, "CourtResNet", _StubModel)
    return _StubModel


def test_tracker_batches_ids_and_scaling(stub_model):
    from padel_analytics_amd.trackers import KeypointsTracker
    t = KeypointsTracker("court.pt", 4)                                       # the defaults: model_type="resnet"
    assert t.model_type == "resnet" and not stub_model.instances              # construction is lazy
    frames = [np.full((36, 50, 3), v, np.uint8) for v in range(10)]
    out = t.predict_frames(iter(frames))
    m = stub_model.instances[0]
    assert m.path == "court.pt" and m.max_batch == 4 and m.batches == [4, 4, 2]       # a last short batch
    assert len(out) == 10
    for v, kps in enumerate(out):
        assert [k.id for k in kps] == list(range(12))                         # ids 0..11: POINTS_MAPPER is the YOLO model's
        for i, k in enumerate(kps):
            x = np.float32(v + 2 * i) / np.float32(512) * 50                  # float32 x int, as numpy computes it
            y = np.float32(v + 2 * i + 1) / np.float32(512) * 36
            assert k.xy == (float(np.float32(x)), float(np.float32(y)))
    json.dumps([k.serialize() for k in out[0]])                               # the JSON cache takes them
    assert t.predict_frames(iter([])) == [] and m.batches == [4, 4, 2]        # no frames: no batch
    assert t.streams is True


def test_tracker_predict_sample_raises_no_predict_sample(stub_model):
    from padel_analytics_amd.trackers import KeypointsTracker, NoPredictSample
    with pytest.raises(NoPredictSample):
        KeypointsTracker("court.pt", 4).predict_sample([np.zeros((4, 4, 3), np.uint8)])
    assert not stub_model.instances


def test_tracker_missing_file_is_not_implemented_with_its_cause(tmp_path):
    from padel_analytics_amd.trackers import KeypointsTracker
    t = KeypointsTracker(str(tmp_path / "missing.pt"), 4)
    touched = []

    def gen():
        touched.append(1)
        yield np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="no court model this engine can run") as ei:
        t.predict_frames(gen())
    assert isinstance(ei.value.__cause__, FileNotFoundError) and not touched   # resolved before the generator is touched
    bad = tmp_path / "garbage.pt"
    bad.write_bytes(b"not a checkpoint")
    with pytest.raises(NotImplementedError, match="no court model this engine can run") as ei:
        KeypointsTracker(str(bad), 4).predict_frames(iter([]))
    assert isinstance(ei.value.__cause__, ValueError)


def test_tracker_wrong_network_is_not_implemented(tmp_path):
    from padel_analytics_amd.trackers import KeypointsTracker
    from tests import resnet_synth as S
    p = tmp_path / "imagenet_head.pt"
    S.save_plain(p, {k: np.zeros(s, np.float32) for k, s in R.state_dict_shapes(1000).items()})
    with pytest.raises(NotImplementedError, match="no court model this engine can run") as ei:
        KeypointsTracker(str(p), 4).predict_frames(iter([]))
    assert isinstance(ei.value.__cause__, ValueError)


def test_tracker_valid_checkpoint_and_no_frames(tmp_path):
    from padel_analytics_amd.trackers import KeypointsTracker
    from tests import resnet_synth as S
    p = tmp_path / "court.pt"
    S.save_plain(p, _random_sd(R.state_dict_shapes(24)))
    t = KeypointsTracker(str(p), 8)
    assert t.predict_frames(iter([])) == []                                   # a loadable checkpoint never raises; no device needed for no frames
    assert set(t.model.state_dict) == set(R.state_dict_shapes(24))


def test_model_class_switches_arithmetic_like_the_yolo_class():
    """``Tracker.use_full_range`` (a sharded run puts every rank on bx3 at once) needs ``set_fp32_mode`` on the model."""
    from padel_analytics_amd.resnet import CourtResNet
    from padel_analytics_amd.trackers import KeypointsTracker
    net = CourtResNet(state_dict=_random_sd(R.state_dict_shapes(24)), fp32_mode="h2")
    t = KeypointsTracker("unused.pt", 4)
    t._model = net
    assert not t.full_range
    t.use_full_range()
    assert net.fp32_mode == "bx3" and t.full_range and net._model is None
    with pytest.raises(ValueError):
        net.set_fp32_mode("fp8")


# ---------------------------------------------------------------------------------------- synthetic checkpoint
def test_synthetic_checkpoint_keeps_the_sigmoid_sensitive():
    from tests import resnet_synth as S
    frames, sd = S.clip_and_state_dict()
    G.check_resnet50_state_dict(sd)
    _, z = R.predict(sd, frames, torch.float64)
    assert z.shape == (S.N_FRAMES, 24)
    print(f"logits: min {z.min():.3f} max {z.max():.3f} std {z.std():.3f}; across frames (mean per-output std) {z.std(axis=0).mean():.3f}")
    assert z.min() >= -4.0 and z.max() <= 4.0
    assert z.std() >= 0.3
    frames2, sd2 = S.test_frames(), S.synthetic_state_dict(S.test_frames(), 0)      # seeded: the same checkpoint again
    assert np.array_equal(frames, frames2) and all(np.array_equal(sd[k], sd2[k]) for k in sd)
