"""The court-keypoint ResNet-50 on the engine: network input against Pillow, the whole graph against the fp64 oracle with the
criterion ``smoke()`` uses (the engine gets the margin the float32 reference arithmetic itself needs, and no more), batch
invariance, stale arena, the bf16x3 mode, hipGraph replay, and ``KeypointsTracker`` in its default configuration through
``TrackingRunner`` and its JSON cache."""
import json
import os

import numpy as np
import pytest
import torch

from padel_analytics_amd import engine as E, graph as G, video
from padel_analytics_amd.resnet import CourtResNet
from tests import resnet_ref as R, resnet_synth as S
from tests import synth  # noqa: F401  (registers the synthetic:// frame source)

pytestmark = pytest.mark.gpu

H, W = S.FRAME_HW


@pytest.fixture(scope="module")
def clip():
    frames, sd = S.clip_and_state_dict()
    xy32, z32 = R.predict(sd, frames, torch.float32)
    xy64, z64 = R.predict(sd, frames, torch.float64)
    return dict(frames=frames, sd=sd, xy32=xy32, z32=z32, xy64=xy64, z64=z64)


def _px(xy):
    return R.keypoints_px(xy, W, H)


@pytest.mark.parametrize("hw", [(720, 1280), (1080, 1920), (480, 854), (517, 333), (224, 224), (224, 640), (300, 224)])
def test_network_input_is_pillow_bilinear_rgb(gpu_engine, hw):
    h, w = hw
    frames = np.ascontiguousarray(synth.synthetic_frames(2, h, w, seed=h + w))
    frames[1] = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    g = G.Graph(task=G.TASK_RESNET)                      # any PA_TASK_RESNET graph builds the network input: the stem alone is enough
    st = g.buf(1, 64)
    g.stem7(np.zeros((64, 3, 7, 7), np.float32), np.zeros(64, np.float32), (st, 0))
    g.head_buf = (st, -1, -1)
    m = E.Model(gpu_engine, g)
    try:
        m.set_max_batch(2)
        m.resnet_infer(frames, 2, h, w)
        netin = m.resnet_read_netin(2)
    finally:
        m.close()
    for i in range(2):
        want = R.resize_rgb_u8(frames[i])
        assert np.array_equal(netin[i, ..., :3], want), (hw, i, int((netin[i, ..., :3] != want).sum()))
    assert not netin[..., 3].any()


def test_whole_graph_against_the_fp64_oracle(gpu_engine, clip):
    net = CourtResNet(state_dict=clip["sd"], engine=gpu_engine)
    try:
        net.set_max_batch(5)
        xy, z = net.infer(clip["frames"], want_logits=True)
        assert not net.fell_back and net.fp32_mode == E.fp32_mode()
        m = net._model
        assert not m.take_overflow()
        d64 = np.abs(_px(xy) - _px(clip["xy64"]))
        f64 = np.abs(_px(clip["xy32"]) - _px(clip["xy64"]))
        rec = dict(frames=5, frame_hw=[H, W], mode=net.fp32_mode,
                   engine_vs_fp64_px=dict(linf=float(d64.max()), rms=float(np.sqrt((d64 ** 2).mean()))),
                   fp32_oracle_vs_fp64_px=dict(linf=float(f64.max()), rms=float(np.sqrt((f64 ** 2).mean()))),
                   logits_linf=dict(engine_vs_fp64=float(np.abs(z - clip["z64"]).max()), fp32_oracle_vs_fp64=float(np.abs(clip["z32"] - clip["z64"]).max())),
                   logits_range=[float(clip["z64"].min()), float(clip["z64"].max())], logits_std=float(clip["z64"].std()))
        print("resnet parity:", json.dumps(rec))
        out = os.environ.get("PADEL_REPORT_DIR")
        if out:
            with open(os.path.join(out, "resnet_parity.json"), "w") as f:
                json.dump(rec, f, indent=1)
        bound = max(1e-3, 4 * f64.max())
        assert d64.max() <= bound, (d64.max(), bound)
        assert np.abs(xy - 1.0 / (1.0 + np.exp(-z.astype(np.float64)))).max() < 3e-7       # xy is the sigmoid of the logits read beside it

        # batch invariance: frame k alone gives the bits it gives inside the batch of 5
        for k in (0, 3):
            xy1, z1 = net.infer(clip["frames"][k:k + 1], want_logits=True)
            assert np.array_equal(z1[0], z[k]) and np.array_equal(xy1[0], xy[k]), k
        # a stale arena (NaN patterns in every activation byte) changes nothing: no kernel reads what nobody wrote
        m.fill_arena(0xFF)
        xy2, z2 = net.infer(clip["frames"], want_logits=True)
        assert np.array_equal(z2, z) and np.array_equal(xy2, xy) and not m.take_overflow()
        # hipGraph replay of the op list: the same bits
        try:
            gpu_engine.set_tuning(graph=1)
            for _ in range(2):                           # capture, then replay
                xy3, z3 = net.infer(clip["frames"], want_logits=True)
                assert np.array_equal(z3, z)
        finally:
            gpu_engine.set_tuning(graph=0)
        # profile rows: the three new ops and 52 convs that all name the kernel family that ran
        gpu_engine.set_profiling(True)
        try:
            net.infer(clip["frames"])
            rows = m.profile_rows()
        finally:
            gpu_engine.set_profiling(False)
        kinds = [r["kind"] for r in rows]
        assert kinds.count(G.OP_STEM7) == 1 and kinds.count(G.OP_MAXPOOL3S2) == 1 and kinds.count(G.OP_GAP_FC) == 1
        convs = [r for r in rows if r["kind"] == G.OP_CONV]
        assert len(convs) == 52 and all(r["family"] and r["tile"] > 0 for r in convs)
        assert sum(r["res"] for r in convs) == 16
    finally:
        net.close()


def test_bx3_mode_gives_the_same_keypoints(gpu_engine, clip):
    net = CourtResNet(state_dict=clip["sd"], engine=gpu_engine, fp32_mode="bx3")
    try:
        net.set_max_batch(5)
        xy, z = net.infer(clip["frames"], want_logits=True)
    finally:
        net.close()
    f64 = np.abs(_px(clip["xy32"]) - _px(clip["xy64"])).max()
    d64 = np.abs(_px(xy) - _px(clip["xy64"])).max()
    print(f"bx3: engine vs fp64 {d64:.3e} px, fp32 oracle vs fp64 {f64:.3e} px")
    assert d64 <= max(1e-3, 4 * f64)


def test_overflow_repeats_on_bx3(gpu_engine, clip):
    """A checkpoint whose activations leave the fp16 range raises the h2 model's flag; CourtResNet repeats the call on bf16x3."""
    sd = dict(clip["sd"])
    sd["bn1.weight"] = (sd["bn1.weight"] * np.float32(1e5)).astype(np.float32)            # conv1's output x 1e5
    sd["layer1.0.bn1.weight"] = np.zeros_like(sd["layer1.0.bn1.weight"])                 # ... and nothing downstream sees it:
    sd["layer1.0.downsample.1.weight"] = np.zeros_like(sd["layer1.0.downsample.1.weight"])   # the logits stay finite
    net = CourtResNet(state_dict=sd, engine=gpu_engine, fp32_mode="h2")
    try:
        net.set_max_batch(2)
        xy = net.infer(clip["frames"][:2])
        assert net.fell_back and net.fp32_mode == "bx3"
        want, _ = R.predict(sd, clip["frames"][:2], torch.float64)
        assert np.abs(_px(xy) - _px(want)).max() < 0.05
    finally:
        net.close()


def test_tracker_default_configuration_through_the_runner(gpu_engine, clip, tmp_path):
    from padel_analytics_amd.trackers import Keypoints, KeypointsTracker, TrackingRunner
    path = tmp_path / "court_resnet50.pt"
    S.save_plain(path, clip["sd"])                       # torch.save(state_dict): the reference's file format
    src = video.ArrayClip(np.concatenate([clip["frames"], clip["frames"][:2]]))           # 7 frames: batches of 4 + 3
    t = KeypointsTracker(str(path), 4, save_path=tmp_path / "court.json")
    assert t.model_type == "resnet"
    runner = TrackingRunner([t], src, tmp_path / "out.mp4")
    runner.run()
    assert len(t) == 7
    want = _px(clip["xy64"])
    bound = max(1e-3, 4 * np.abs(_px(clip["xy32"]) - want).max())
    for i, kps in enumerate(t.results.predictions):
        assert isinstance(kps, Keypoints) and [k.id for k in kps] == list(range(12))
        got = np.array([k.xy for k in kps])
        assert np.abs(got - want[i % 5]).max() <= bound, (i, np.abs(got - want[i % 5]).max())
    data = json.loads((tmp_path / "court.json").read_text())
    assert len(data) == 7 and len(data[0]) == 12
    t2 = KeypointsTracker(str(path), 4, load_path=tmp_path / "court.json")
    assert len(t2) == 7
    for a, b in zip(t2.results.predictions, t.results.predictions):
        assert [(k.id, tuple(k.xy)) for k in a] == [(k.id, tuple(k.xy)) for k in b]
