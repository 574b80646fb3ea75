"""GPU: the range guard of the fp16 family (``half=True``).  Every kernel that turns an fp32 value x into a stored half of an
activation buffer — ``f16_epilogue_fast`` (16-byte pair stores, the 8-byte leftover of an odd fragment count, both with a
residual), ``f16_epilogue_slow``, ``stem_mfma_kernel<NF, 1>`` — raises the model's sticky flag iff ``!(|x| <= 65504)``, tested on
the value the clamp sees (behind the residual add): NaN raises, exactly +-65504 does not, and the fp32 head paths never do.  The
stored bits are those of the clamp alone.  Then the consumers: ``yolo.YOLO`` and ``BallTracker`` leave ``half`` when the flag is
up, one ladder f16 -> the default fp32-equivalent path -> bf16x3.

1. per native tile of every fp16 conv family one case per store path (tests/tile_support.py names the path; what launched is
   asserted from the profile rows).  Zero weights and no activation: the output is the bias, plus the residual where there is one,
   so each value is planted exactly.  Expected halves: ``rn16`` of tests/test_gpu_f16_epilogue.py on fl32(bias + residual).
2. a raise in the last workgroup only: one output pixel (15, 15), last channel.
3. the fp16 stem.
4. a YOLOv8n detect checkpoint whose stem output leaves the range: both steps of the ladder, results of a bx3 model, bit for bit;
   the same through the trackers' pipelined batch loop.
5. ``BallTracker(half=True)`` on a TrackNet whose first block leaves the range.
6. no false alarms on the ordinary synthetic checkpoints."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ball_ref as br
from padel_analytics_amd import checkpoint, detections as D, engine as E, graph as G, video, yolo, yolo_arch
from padel_analytics_amd.trackers import BallTracker, PlayerTracker, TrackingRunner
from tests import stem_probe as P, synth, tile_support as TS
from tests.test_gpu_ball import _calibrated_tracknet, _clip
from tests.test_gpu_conv import _launched
from tests.test_gpu_f16_epilogue import TILES, bits, rn16
from tests.test_gpu_stem import DEFAULTS as STEM_DEFAULTS, SHAPES_A, infer as stem_infer

pytestmark = pytest.mark.gpu

F16_MAX = np.float32(65504.0)
FIRST_BEYOND = np.float32(65520.0)          # the first fp32 value that rounds past 65504: RN16 alone would make it inf
FAST_PATHS = ("pair16", "tail8", "pair16_res", "tail8_res")


def conv_case(cout, res, hw=16):
    return (1, hw, hw, 32, cout, 3, 1, G.ACT_NONE, res)


def family(tile):
    return TS.expected("f16", tile, conv_case(32, False))[0]


def store_params():
    """[(tile, path, case)]: per tile every fast path its fragment count allows — on cout 32, 48 or, for the wider tiles, the tile's
    own channel count, whichever is the first to take the path on a 16 x 16 map — and the element-wise path twice: a partial
    fragment (cout 20) without a residual, partial pixel tiles (a 15 x 15 map) with one."""
    out = []
    for tile in TILES:
        fam, bn = family(tile), TS.SHAPES["f16"][tile][-1]
        for path in FAST_PATHS:
            if path not in TS.f16_paths_of_tile(tile):
                continue
            res = path.endswith("_res")
            hit = [c for c in (conv_case(co, res) for co in (32, 48, bn)) if path in TS.f16_store_paths(fam, tile, c, "f16")]
            assert hit, (tile, path)
            out.append((tile, path, hit[0]))
        for name, case in (("slow", conv_case(20, False)), ("slow_res", conv_case(32, True, hw=15))):
            assert TS.f16_store_paths(fam, tile, case, "f16") == {"slow"}, (tile, case)
            out.append((tile, name, case))
    assert all(TS.native("f16", t, c) for t, _, c in out)
    return out


STORE_PARAMS = store_params()


def planted_channel(tile, path, cout):
    """A channel whose value goes through ``path``: a wave's fragments are NF consecutive ones, stored in pairs from the first, an
    odd last one alone.  Element-wise path: the last real channel (a partial fragment's, where there is one)."""
    nf = TS.F16_NF[tile]
    if path.startswith("tail8"):
        return (nf - 1) * 16 + 5
    if path.startswith("pair16"):
        return 21 if nf >= 2 and cout >= 32 else 5           # fragment 1: the half of a pair that permlane16_swap moves
    return cout - 1


def build(case, bias, rvec=None, head="f16", w=None):
    """[zero-weight 1x1 with bias ``rvec`` -> residual buffer], zero fill of the buffer S, the conv under test (weights ``w``, default
    zero) -> S, identity 1x1 S -> fp32 head; head="f32": the conv under test writes the fp32 head itself.  -> (graph, its index)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    z = lambda *shape: np.zeros(shape, np.float32)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F16)
    b0 = g.buf(0, cin)
    wd = g.padk(cout)
    w = z(cout, cin, k, k) if w is None else w
    res = None
    if use_res:
        rb = g.buf(0, wd)
        g.conv((b0, 0, cin), (rb, 0), z(cout, cin, 1, 1), rvec, 1, 1, G.ACT_NONE, out_width=wd)
        res = (rb, 0)
    if head == "f32":
        b1 = g.buf(0, cout if cout % 4 == 0 else G.pad16(cout))
        g.conv((b0, 0, cin), (b1, 0), w, bias, k, s, act, res=res)
        g.head_buf = (b1, -1, -1)
        return g, -1
    S = g.buf(0, wd)
    g.conv((b0, 0, cin), (S, 0), z(wd, cin, 1, 1), z(wd), 1, 1, G.ACT_NONE)
    g.conv((b0, 0, cin), (S, 0), w, bias, k, s, act, res=res)
    hd = g.buf(0, wd)
    g.conv((S, 0, wd), (hd, 0), np.eye(wd, dtype=np.float32)[:, :, None, None], z(wd), 1, 1, G.ACT_NONE)
    g.head_buf = (hd, -1, -1)
    return g, -2


def run(eng, case, tile, bias, rvec=None, head="f16", w=None, x=None):
    """One forced run -> (the cout output channels, the flag, the flag read once more).  What launched is what tile_support says."""
    g, which = build(case, bias, rvec, head, w)
    eng.set_tuning(variant=tile)
    eng.set_profiling(True)
    m = E.Model(eng, g)
    try:
        m.set_max_batch(case[0])
        y = m.tracknet_infer(np.zeros(case[:4], np.float16) if x is None else x)
        got = _launched(m, which)
        flag, again = m.take_overflow(), m.take_overflow()
    finally:
        eng.set_profiling(False)
        eng.set_tuning(variant=-1)
        m.close()
    want = TS.expected("f16", tile, case)
    assert got == want, f"requested {tile}, launched {got[0]}/{got[1]}; tests/tile_support.py says {want[0]}/{want[1]}"
    return y[..., :case[4]], flag, again


def ordinary(cout, seed):
    """fp16 numbers well inside the range, none zero."""
    return (0.25 * (1 + (np.arange(cout) * 7 + seed) % 9) * np.where(np.arange(cout) % 2, -1, 1)).astype(np.float32)


def expect(case, bias, rvec):
    """The halves a correct store leaves, as the identity readback returns them: RN16(clip(fl32(bias + residual)))."""
    t = bias if rvec is None else (bias + rvec).astype(np.float32)
    Ho, Wo = TS.out_hw(case)
    return np.broadcast_to(rn16(t), (case[0], Ho, Wo, case[4]))


@pytest.mark.parametrize("tile,path,case", STORE_PARAMS, ids=[f"{family(t)}-{t}-{p}" for t, p, _ in STORE_PARAMS])
def test_flag_per_store_path(gpu_engine, tile, path, case):
    cout, use_res = case[4], case[8]
    c = planted_channel(tile, path, cout)
    assert 0 <= c < cout - 1 or path.startswith("slow")
    c2 = c - 1 if c == cout - 1 else c + 1
    name = f"{family(tile)} tile {tile} {path} {case}, channel {c}"
    rvec = ordinary(cout, 3) if use_res else None
    if use_res:
        rvec[[c, c2]] = 0.0                    # (the planted sums are then the bias itself; (c) below plants through the add)
    base = ordinary(cout, 0)

    def one(bias, rv=rvec, nan=False):
        y, flag, again = run(gpu_engine, case, tile, bias, rv)
        if not nan:
            want = expect(case, bias, rv)
            bad = bits(y) != bits(want)
            assert not bad.any(), f"{name}: {int(bad.sum())} stored halves differ from RN16(clip(bias + residual)), first at {tuple(np.argwhere(bad)[0])}"
        return flag, again

    # (a) in range, +65504 and -65504 exactly among the values: no flag
    b = base.copy()
    b[c], b[c2] = F16_MAX, -F16_MAX
    assert one(b) == (False, False), f"{name}: flag raised with every value in range (+-65504 exactly is in range)"
    # (b) one value beyond: the flag, once; the stored halves are the clamp's
    for v in (FIRST_BEYOND, np.float32(-1.0e5), np.float32(np.nan)):
        b = base.copy()
        b[c] = v
        assert one(b, nan=bool(np.isnan(v))) == (True, False), f"{name}: bias {v!r}: the flag must be up exactly once"
    # (c) the test is behind the residual add
    if use_res:
        b, r = base.copy(), rvec.copy()
        b[c], r[c] = 40000.0, 40000.0
        assert one(b, r) == (True, False), f"{name}: 40000 + 40000 did not raise"
        r0 = rvec.copy()
        assert one(b, r0) == (False, False), f"{name}: bias 40000 alone raised"
        b0 = base.copy()
        b0[c] = 0.0
        assert one(b0, r) == (False, False), f"{name}: residual 40000 alone raised"
    else:
        # (d) the same conv writing the fp32 head: nothing is clamped, nothing is flagged
        b = base.copy()
        b[c] = 1.0e5
        y, flag, again = run(gpu_engine, case, tile, b, head="f32")
        assert (flag, again) == (False, False), f"{name}: an fp32 head raised the flag"
        assert (y[..., c] == np.float32(1.0e5)).all() and np.array_equal(y, np.broadcast_to(b, y.shape)), f"{name}: fp32 head"


# (family, tile): two workgroups and more on a 16 x 16 map with 96 channels (pixel tiles of 128 / patches of 8 x 16; the quad tile
# covers the map with one patch and splits the channels)
LAST_WG = (("tap16", 20), ("tap16d", 60), ("p16", 303), ("p16q", 323))


@pytest.mark.parametrize("fam,tile", LAST_WG, ids=[f for f, _ in LAST_WG])
def test_flag_from_the_last_workgroup_only(gpu_engine, fam, tile):
    """One value beyond the range, at pixel (15, 15) of the last channel: one lane of one wave of the last workgroup sees it — the
    ballot, then the atomicOr by the wave's first lane.  The centre tap of a 3x3 over an input that is zero but for one pixel."""
    case = conv_case(96, False)
    assert family(tile) == fam and TS.f16_store_paths(fam, tile, case, "f16") <= {"pair16", "tail8"}
    w = np.zeros((96, 32, 3, 3), np.float32)
    w[95, 0, 1, 1] = 512.0
    bias = np.zeros(96, np.float32)
    want = np.zeros((1, 16, 16, 96), np.float32)
    for xv, flag_want, stored in ((256.0, True, F16_MAX), (64.0, False, np.float32(32768.0))):        # 131072 and 32768
        x = np.zeros((1, 16, 16, 32), np.float16)
        x[0, 15, 15, 0] = xv
        y, flag, again = run(gpu_engine, case, tile, bias, w=w, x=x)
        want[0, 15, 15, 95] = stored
        assert np.array_equal(bits(y), bits(want)), f"{fam} tile {tile}: stored halves"
        assert (flag, again) == (flag_want, False), f"{fam} tile {tile}: input {xv}: flag {flag}, then {again}"


# ---- 3. the fp16 stem -------------------------------------------------------------------------------------------------------------
def stem_model(eng, c, b5=None):
    """The stand-alone stem probe with the stem writing halves; 16- and 48-channel stems sit in a buffer of whole 32-channel k-steps
    (the probe graph writes zeros into the rest)."""
    w, b = P.stem_weights(c)
    if b5 is not None:
        b[5] = b5
    return E.Model(eng, P.standalone_graph("f16", c, w, b, buf_width=G.Graph(task=G.TASK_DETECT, dtype=G.DTYPE_F16).padk(c)))


def test_fp16_stem_raises_and_clears(gpu_engine):
    m = stem_model(gpu_engine, 16, P.BIG_BIAS)
    try:
        gpu_engine.set_tuning(**{**STEM_DEFAULTS, "fuse_stem": 0})
        head, _ = stem_infer(m, P.probe_frames(*SHAPES_A[1]), fill=False)
        assert m.take_overflow(), "silu(7e4) was clamped to 65504 and the flag stayed down"
        assert not m.take_overflow(), "taking the flag clears it"
        got = P.decode_level1(head)[..., 5]
        assert (got == F16_MAX).all(), "the stored half is the clamp's"
    finally:
        gpu_engine.set_tuning(**STEM_DEFAULTS)
        m.close()


@pytest.mark.parametrize("c", [16, 48])
def test_fp16_stem_ordinary_weights_no_flag(gpu_engine, c):
    m = stem_model(gpu_engine, c)
    try:
        gpu_engine.set_tuning(**{**STEM_DEFAULTS, "fuse_stem": 0})
        for shape in SHAPES_A:
            stem_infer(m, P.probe_frames(*shape), fill=False)
            assert not m.take_overflow(), f"c{c} {shape}: overflow flag with ordinary weights"
    finally:
        gpu_engine.set_tuning(**STEM_DEFAULTS)
        m.close()


# ---- 4. YOLO ----------------------------------------------------------------------------------------------------------------------
STEM_FACTOR = 3.0e5          # SiLU(x) ~ x beyond 65504 behind the stem; model.1 scaled back: its packed halves are tiny, not infinite


def hot_detect_sd():
    sd = yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5)
    sd["model.0.conv.weight"] = sd["model.0.conv.weight"] * STEM_FACTOR
    sd["model.1.conv.weight"] = sd["model.1.conv.weight"] / STEM_FACTOR
    return sd


def save_detect(path, sd):
    checkpoint.save_checkpoint(path, sd, "detect", 80, None, "n", {0: "person"})
    return str(path)


def copy_result(r):
    return tuple(None if a is None else np.array(a) for a in r[:3]) + tuple(r[3:])


def same_result(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def test_yolo_half_takes_both_steps(gpu_engine, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(E, "fp32_mode", lambda: "h2")          # the ladder's middle step, whatever the environment's default
    ck = save_detect(tmp_path / "hot.pt", hot_detect_sd())
    frames = synth.synthetic_frames(2, 90, 160, seed=5)          # letterboxed to a 96 x 160 network input
    args = (frames, 0.25, 0.7, 160)
    y = yolo.YOLO(ck, engine=gpu_engine, half=True)
    assert y.half and y.graph.dtype == G.DTYPE_F16 and y.graph.f16_weight_overflow is False and not y.fell_back
    y.set_max_batch(2)
    got = copy_result(y.infer_frames(*args, channel_reverse=False))
    out = capsys.readouterr().out
    assert y.half is False and y.fell_back and y.fp32_mode == "bx3", (y.half, y.fell_back, y.fp32_mode)
    assert out.count("beyond the fp16 range") == 2, out              # f16 -> h2, h2 -> bx3
    again = copy_result(y.infer_frames(*args, channel_reverse=False))
    y.close()
    ref = yolo.YOLO(ck, engine=gpu_engine, fp32_mode="bx3")
    ref.set_max_batch(2)
    want = copy_result(ref.infer_frames(*args, channel_reverse=False))
    ref.close()
    assert not ref.fell_back
    print(f"detections per frame: {want[2].tolist()}")
    assert same_result(got, want) and same_result(again, want), "the repeated batch is not the bx3 model's, bit for bit"


def _player_tracker(ck, **kw):
    zone = D.PolygonZone(np.array([[40, 40], [600, 40], [600, 340], [40, 340]]), frame_resolution_wh=(640, 360))
    t = PlayerTracker(ck, zone, batch_size=6, **kw)
    t.video_info_post_init(video.VideoInfo(width=640, height=360, fps=30, total_frames=20))
    return t


def _track(tracker, clip):
    tracker.restart()
    tracker.predict_and_update(clip.frames())
    return [o.serialize() for o in tracker.results]


def test_yolo_half_overflow_in_a_pipelined_clip(gpu_engine, tmp_path, monkeypatch):
    """20 frames in batches of 6 through the trackers' two-call loop: the first collected ticket reports the flag, the batch queued
    behind it dies with the model, every batch ends on the bx3 model."""
    monkeypatch.setattr(E, "fp32_mode", lambda: "h2")          # the ladder's middle step, whatever the environment's default
    ck = save_detect(tmp_path / "hot.pt", hot_detect_sd())
    clip = video.DeviceClip(gpu_engine, synth.synthetic_frames(20, 360, 640, seed=9))
    t = _player_tracker(ck, half=True)
    assert t.arithmetic == "f16" and t.full_range
    piped = _track(t, clip)
    assert t.model.half is False and t.model.fell_back and t.model.fp32_mode == "bx3" and t.arithmetic == "bx3"
    t.to("cpu")
    ref = _player_tracker(ck)
    ref.model.set_fp32_mode("bx3")
    want = _track(ref, clip)
    ref.to("cpu")
    clip.free()
    assert piped == want and len(piped) == 20


# ---- 5. BallTracker ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ball_case(hot):
    """16 frames and a calibrated synthetic TrackNet.  ``hot``: the first block's BatchNorm scale and shift are multiplied by a
    factor that takes its largest folded weight to 6e4 — still an fp16 number — and the second block's weights divided by it (ReLU
    commutes with a positive factor: the rest of the network sees ordinary values).  Premise, on the host: the first block's
    largest output over the first window is beyond 7e4."""
    T = 16
    frames = _clip(T, 360, 640, seed=33)
    sd = dict(_calibrated_tracknet(frames))
    if hot:
        p = "down_block_1.conv_1"
        w, b = G.fold_bn(sd, p, G.TRACKNET_BN_EPS)
        f = np.float32(6.0e4 / np.abs(w).max())
        x = torch.from_numpy(br.window_input(br.median_background(frames), [br.resize_frame(fr) for fr in frames[:8]]))[None]
        top = float(F.conv2d(x, torch.from_numpy(w), torch.from_numpy(b), padding=1).max()) * float(f)
        print(f"hot TrackNet: factor {float(f):.4g}, largest output of {p} over the first window {top:.4g}")
        assert top > 7.0e4, top
        sd[f"{p}.bn.weight"] = np.asarray(sd[f"{p}.bn.weight"], np.float32) * f
        sd[f"{p}.bn.bias"] = np.asarray(sd[f"{p}.bn.bias"], np.float32) * f
        sd["down_block_1.conv_2.conv.weight"] = np.asarray(sd["down_block_1.conv_2.conv.weight"], np.float32) / f
        assert not G.build_tracknet(sd, dtype="f16").f16_weight_overflow
    return frames, sd


def _ball_tracker(tmp_path, sd, name, **kw):
    ck = tmp_path / f"{name}.pt"
    if not ck.exists():
        checkpoint.save_checkpoint(ck, sd, "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    return BallTracker(str(ck), None, batch_size=8, median_max_sample_num=16, **kw)


def _ball_run(tracker, frames, name):
    T = len(frames)
    video.register_source(name, lambda p: video.VideoInfo(640, 360, 30, T),
                          lambda p, start, end, stride: iter(frames[start:T if end is None else min(end, T):stride]))
    TrackingRunner([tracker], f"{name}://clip", "unused.mp4").run()
    return [(b.frame, tuple(b.xy), b.visibility) for b in tracker.results.predictions]


def test_ball_tracker_half_leaves_half(gpu_engine, tmp_path):
    frames, sd = ball_case(True)
    t = _ball_tracker(tmp_path, sd, "hot", half=True)
    assert t.half and t.arithmetic == "f16"
    got = _ball_run(t, frames, "hotball")
    assert t.half is False and t.arithmetic in ("h2", "bx3") and len(got) == 16
    end = t.arithmetic
    t.to("cpu")
    ref = _ball_tracker(tmp_path, sd, "hot")
    for _ in range(2):
        if ref.arithmetic != end:
            ref.use_full_range()
    assert ref.arithmetic == end
    want = _ball_run(ref, frames, "hotball")
    assert ref.arithmetic == end, "the reference run stayed on the arithmetic the half tracker ended on"
    ref.to("cpu")
    print(f"BallTracker(half=True) on the hot checkpoint ends on {end}")
    assert got == want


# ---- 6. no false alarms -----------------------------------------------------------------------------------------------------------
def test_no_false_alarm_ball_tracker(gpu_engine, tmp_path):
    frames, sd = ball_case(False)
    t = _ball_tracker(tmp_path, sd, "plain", half=True)
    got = _ball_run(t, frames, "plainball")
    assert len(got) == 16 and t.half and t.arithmetic == "f16" and t.graph.dtype == G.DTYPE_F16      # (it reads the flag after every stream)
    t.to("cpu")


def test_no_false_alarm_yolo(gpu_engine, tmp_path):
    clip = video.DeviceClip(gpu_engine, synth.synthetic_frames(20, 360, 640, seed=8))
    ck = save_detect(tmp_path / "plain.pt", yolo_arch.synth_state_dict("n", 80, None, seed=3, cls_bias=0.5))
    t = _player_tracker(ck, half=True)
    out = _track(t, clip)
    assert len(out) == 20 and t.model.half and not t.model.fell_back and t.arithmetic == "f16"
    assert not t.model._model.take_overflow()
    t.to("cpu")
    clip.free()
    kpt = (13, 3)
    pk = tmp_path / "pose.pt"
    checkpoint.save_checkpoint(pk, yolo_arch.synth_state_dict("n", 1, kpt, seed=4, cls_bias=0.5), "pose", 1, kpt, "n", {0: "person"})
    y = yolo.YOLO(str(pk), engine=gpu_engine, half=True)
    y.set_max_batch(2)
    y.infer_frames(synth.synthetic_frames(2, 90, 160, seed=5), 0.25, 0.7, 160, channel_reverse=False)
    assert y.half and not y.fell_back and y.arithmetic == "f16" and not y._model.take_overflow()
    y.close()
