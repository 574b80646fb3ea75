"""GPU: the ball tracker's TrackNet stage on the fp16 kernels (``BallTracker(half=True)``, ``graph.build_tracknet(sd, "f16")``,
the fp16 mode of ``ball_assemble_kernel``) — the clip and the calibration of tests/test_gpu_ball.py.

* assembly: what the session feeds the network equals the host's window assembly cast to fp16, and the five pad channels are
  written on every launch (the session's heat maps equal ``oracle.ball_ref.ensemble`` of ``Model.tracknet_infer`` over host-made
  windows to 1e-6 — sums of at most 8 fp32 terms in [0, 1], each rounding at most 2^-24 — and are the same bits after the arena
  was filled with 0xFF);
* parity, per case (T, feed): the reference is the fp32 oracle ``br.track(frames, TrackNetRef.forward)``, the yardstick e_emu is
  the L-inf distance from it of the CPU emulation of the SAME op list with fp16 storage (tests/graph_interp.py); the engine's
  heat maps must be within 3 x e_emu of the oracle (the emulation and the kernels add their fp32 products in different orders;
  single fp16 rounding flips then compound through 18 layers), and the masks must equal ``heat_ref > 0.5`` outside the band
  |heat_ref - 0.5| < 3 x e_emu, which may hold at most 1 % of the pixels.  Both figures are printed, and written as JSON where
  PADEL_HALF_PARITY_OUT names a file (profiles/tracknet_half_parity.json is such a record);
* shards: ``predict_partial`` over two shards with 7 frames of context equals the unsharded run exactly;
* plugin: ``BallTracker(half=True)`` with an InpaintNet through ``TrackingRunner``, and the fp16 kernel families on every conv."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import ball_ref as br, tracknet_ref as tr
from padel_analytics_amd import checkpoint, engine as E, graph as G, video
from padel_analytics_amd.trackers import Ball, BallTracker, TrackingRunner
from tests import graph_interp
from tests.test_gpu_ball import _calibrated_tracknet, _clip

pytestmark = pytest.mark.gpu

F16_FAMILIES = ("tap16", "p16")


@functools.lru_cache(maxsize=None)
def _case(T):
    """Clip, calibrated weights, resized background / frames and the host-made network windows of a T-frame clip: made once."""
    frames = _clip(T, 360, 640, seed=21)
    sd = _calibrated_tracknet(frames)
    med = br.median_background(frames)
    small = [br.resize_frame(f) for f in frames]
    x = np.zeros((T - 7, 32, 288, 512), np.float32)
    for g in range(T - 7):
        x[g, :27] = br.window_input(med, small[g:g + 8])
    return frames, sd, x


def _median_rgb(frames):
    return np.median(np.array([f[..., ::-1] for f in frames]), 0).astype("uint8")


def _session_run(m, frames, feed):
    """Feeds of ``feed`` frames, then the flush -> (masks, heat, rects) of every frame."""
    sess = E.BallSession(m, 360, 640)
    sess.set_background(_median_rgb(frames))
    out = [sess.feed(frames[i:i + feed], want_heat=True, want_rects=True) for i in range(0, len(frames), feed)]
    out.append(sess.feed(None, flush=True, want_heat=True, want_rects=True))
    sess.close()
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def test_fp16_window_assembly(gpu_engine):
    T = 12
    frames, sd, x = _case(T)
    m = E.Model(gpu_engine, G.build_tracknet(sd, dtype="f16"))
    m.set_max_batch(8)
    # feeds of 8 and 4 frames complete 1 and 4 windows: the host-made windows go through the network in the same two batches,
    # so that every conv runs the same kernel on the same shape both times
    x16 = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float16)
    y = np.concatenate([m.tracknet_infer(x16[:1]), m.tracknet_infer(x16[1:])])
    want = br.ensemble(np.ascontiguousarray(y.transpose(0, 3, 1, 2)))
    masks, heat, rects = _session_run(m, frames, 8)
    assert heat.shape == want.shape == (T, 288, 512)
    err = float(np.abs(heat - want).max())
    print(f"fp16 assembly: session heat vs ensemble of tracknet_infer over host-assembled windows: {err:.2e}")
    assert err <= 1e-6
    assert np.isfinite(heat).all() and float(heat.max()) > 0.5 > float(heat.min())
    # the pad channels 27..31 of the input buffer are written by every launch: NaN patterns left in the arena change nothing
    m.fill_arena(0xFF)
    masks2, heat2, rects2 = _session_run(m, frames, 8)
    assert np.array_equal(heat2.view(np.uint32), heat.view(np.uint32)) and np.array_equal(masks2, masks) and np.array_equal(rects2, rects)
    m.close()


@pytest.mark.parametrize("T,feed", [(12, 8), (19, 4)])
def test_fp16_ball_session_parity(gpu_engine, T, feed):
    frames, sd, x = _case(T)
    g16 = G.build_tracknet(sd, dtype="f16")
    head = g16.head_buf[0]

    def emulation(xb):                     # (N, 27, 288, 512) fp32 -> (N, 8, 288, 512): the op list with fp16 storage on the CPU
        x32 = torch.zeros(xb.shape[0], 32, 288, 512)
        x32[:, :27] = xb
        return graph_interp.run(g16, buf0=x32.half().float())[head][:, :8]

    _, _, _, heat_ref = br.track(frames, tr.TrackNetRef(sd).forward, batch=4)
    _, _, _, heat_emu = br.track(frames, emulation, batch=4)
    m = E.Model(gpu_engine, g16)
    m.set_max_batch(feed)
    masks, heat, rects = _session_run(m, frames, feed)
    m.close()
    assert heat.shape == heat_ref.shape == (T, 288, 512)
    e_emu = float(np.abs(heat_emu - heat_ref).max())
    e_eng = float(np.abs(heat - heat_ref).max())
    band = np.abs(heat_ref - 0.5) < 3 * e_emu
    want_mask = heat_ref > 0.5
    flips = int(((masks > 0) != want_mask)[~band].sum())
    emu_flips = int(((heat_emu > 0.5) != want_mask)[~band].sum())
    rec = {"T": T, "feed": feed, "e_emu": e_emu, "e_engine": e_eng, "e_engine_vs_emulation": float(np.abs(heat - heat_emu).max()),
           "band_fraction": float(band.mean()), "mask_flips_outside_band": flips, "emulation_flips_outside_band": emu_flips,
           "foreground_outside_band": int(want_mask[~band].sum())}
    print("fp16 ball parity: " + json.dumps(rec))
    if os.environ.get("PADEL_HALF_PARITY_OUT"):
        with open(os.environ["PADEL_HALF_PARITY_OUT"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert e_eng <= 3 * e_emu, f"engine heat {e_eng:.2e} from the fp32 oracle, emulation {e_emu:.2e}"
    assert band.mean() <= 0.01, f"the band holds {band.mean():.2%} of the pixels"
    assert want_mask[~band].any(), "calibration produced empty masks"
    assert flips == 0
    for i in range(T):                     # device predict_location == the oracle's, on the masks the device produced
        assert tuple(rects[i]) == tuple(br.predict_location(masks[i])), i


def _half_tracker(tmp_path, sd, T, inpaint=None, **kw):
    ck = tmp_path / "TrackNet_synth.pt"
    if not ck.exists():
        checkpoint.save_checkpoint(ck, sd, "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    return BallTracker(str(ck), inpaint, batch_size=8, median_max_sample_num=T, **kw)


def test_fp16_shards_equal_the_unsharded_run(gpu_engine, tmp_path):
    T = 19
    frames, sd, _ = _case(T)
    t = _half_tracker(tmp_path, sd, T, half=True)
    t.median = _median_rgb(frames)
    whole = t.predict_partial(iter(frames))
    a = t.predict_partial(iter(frames[0:17]), first_frame=0, head_context=0, tail_context=7)
    b = t.predict_partial(iter(frames[3:19]), first_frame=10, head_context=7, tail_context=0)
    assert t.graph.dtype == G.DTYPE_F16 and len(whole) == T and len(a) == 10 and len(b) == 9
    assert a + b == whole
    assert sum(v for _, _, v in whole) > 0
    t.to("cpu")


def test_fp16_ball_tracker_plugin(gpu_engine, tmp_path):
    T = 16
    frames = _clip(T, 360, 640, seed=33)
    sd = _calibrated_tracknet(frames)
    ick = tmp_path / "InpaintNet_synth.pt"
    checkpoint.save_checkpoint(ick, tr.synth_inpaintnet_state_dict(8), "inpaintnet", param_dict={"seq_len": 16})
    video.register_source("ballclip", lambda p: video.VideoInfo(640, 360, 30, T),
                          lambda p, start, end, stride: iter(frames[start:T if end is None else min(end, T):stride]))
    got = {}
    for half in (True, False):
        t = _half_tracker(tmp_path, sd, T, str(ick), half=half, save_path=tmp_path / f"ball_{int(half)}.json")
        TrackingRunner([t], "ballclip://clip", tmp_path / "out.mp4").run()
        assert len(t) == T and t.graph.dtype == (G.DTYPE_F16 if half else G.build_tracknet(sd, E.graph_dtype()).dtype)
        data = json.loads((tmp_path / f"ball_{int(half)}.json").read_text())
        assert len(data) == T
        back = [Ball.from_json(d) for d in data]
        assert [(b.frame, tuple(b.xy), b.visibility) for b in back] == [(b.frame, tuple(b.xy), b.visibility) for b in t.results.predictions]
        t2 = _half_tracker(tmp_path, sd, T, str(ick), half=half, load_path=tmp_path / f"ball_{int(half)}.json")
        assert len(t2) == T
        got[half] = [(b.xy[0], b.xy[1], b.visibility) for b in t.results.predictions]
        if half:                           # which kernels ran the network: one profiled pass of the tracker's own model
            t.to("cuda")
            sess = E.BallSession(t._model, 360, 640)
            sess.set_background(_median_rgb(frames))
            gpu_engine.set_profiling(True)
            try:
                sess.feed(frames[:8])      # (the rows are those of the last feed; a flush runs no network)
                convs = [r for r in t._model.profile_rows() if r["kind"] == G.OP_CONV]
            finally:
                gpu_engine.set_profiling(False)
                sess.close()
            assert len(convs) == 18 and all(r["family"].startswith(F16_FAMILIES) for r in convs), [(r["family"], r["tile"]) for r in convs]
        t.to("cpu")
    assert [v for _, _, v in got[True]] == [v for _, _, v in got[False]] and sum(v for _, _, v in got[True]) > 0
    dist = max(float(np.hypot(a[0] - b[0], a[1] - b[1])) for a, b in zip(got[True], got[False]))
    print(f"fp16 ball plugin: largest centre distance half=True vs half=False over {T} frames: {dist:.2f} px")
    if os.environ.get("PADEL_HALF_PARITY_OUT"):
        with open(os.environ["PADEL_HALF_PARITY_OUT"], "a") as f:
            f.write(json.dumps({"plugin_frames": T, "largest_centre_distance_px": dist}) + "\n")
