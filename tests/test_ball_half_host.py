"""CPU: the fp16 TrackNet graph (``graph.build_tracknet(sd, "f16")``) and ``BallTracker(half=True)`` without a GPU.

* the f16 graph is the f32 graph with another storage type: same op kinds, buffers and slices, every conv input a whole number of
  32-channel k-steps; its description passes the engine's host-only checks (csrc/graph_plan.cpp through tests/graph_plan_main.cpp,
  called the way tests/test_graph_plan_host.py calls it) and its activation plan is sound;
* interpreted on the CPU with fp16 storage rounding (tests/graph_interp.py) it agrees with the fp32 oracle (oracle/tracknet_ref.py).
  The bound: every stored activation is rounded to fp16 (relative 2^-11 = 4.9e-4) in each of the 17 conv layers in front of the
  predictor and the weights once; the roundings are independent, so the pre-sigmoid logit carries about sqrt(18) x 4.9e-4 = 2.1e-3
  of its scale (a few units for the calibrated weights: the largest activation of the graph is about 5), and the sigmoid's slope
  is at most 1/4: about 1e-3 to 2e-3 on the heat value.  On a 288 x 512 window of the clip of tests/test_gpu_ball_half.py this
  emulation is 9.9e-4 from the oracle (the fp32 interpretation 9.8e-7); the assertion allows three times that figure, 3e-3, the
  width of the band in which the GPU parity test lets a mask pixel differ;
* the tracker: ``half=True`` builds the F16 graph, ``use_full_range()`` goes back to the default fp32-equivalent path, and with
  ``half=False`` the weight blob is byte-equal to ``build_tracknet(sd, E.graph_dtype())``."""
import numpy as np
import pytest
import torch

from oracle import tracknet_ref as tr
from padel_analytics_amd import checkpoint, engine as E, graph as G
from padel_analytics_amd.trackers import BallTracker
from tests import graph_interp
from tests.test_graph_plan_host import BATCH, SLACK, Desc, answers, build_harness, live_ranges

E_EMU_WINDOW = 9.9e-4          # CPU fp16-storage emulation against the fp32 oracle, one 288 x 512 window (module docstring)
SLICE_FIELDS = ("kind", "in_buf", "in_choff", "cin", "out_buf", "out_choff", "cout", "ksize", "stride", "act", "res_buf", "res_choff", "npad")


@pytest.fixture(scope="module")
def sd():
    return tr.synth_tracknet_state_dict(5)


def test_f16_tracknet_graph(sd, tmp_path):
    g32, g16 = G.build_tracknet(sd, "f32"), G.build_tracknet(sd, "f16")
    assert g16.dtype == G.DTYPE_F16 and g32.dtype == G.DTYPE_F32
    assert g16.bufs == g32.bufs and g16.bufs[0] == (0, 32) and g16.in_channels == 32
    assert g16.head_buf == g32.head_buf and g16.out_channels == g32.out_channels == 8
    assert [[o[f] for f in SLICE_FIELDS] for o in g16.ops] == [[o[f] for f in SLICE_FIELDS] for o in g32.ops]
    convs = [o for o in g16.ops if o["kind"] == G.OP_CONV]
    assert len(convs) == 18 and all(o["cin"] % 32 == 0 and o["in_choff"] % 8 == 0 and o["out_choff"] % 8 == 0 for o in convs)
    assert all(o["cin"] % 8 == 0 and o["in_choff"] % 8 == 0 and o["out_choff"] % 8 == 0 for o in g16.ops if o["kind"] != G.OP_CONV)
    assert G.build_tracknet(sd, "h2").bufs == g32.bufs            # the two existing storage types keep their input width

    # the engine's host-only checks and memory plan
    d = Desc(g16)
    got = answers(build_harness(tmp_path / "graph_plan_main"), {"tracknet-f16": d})["tracknet-f16"]
    assert got["validate"] == "ok" and got["folds"] == [] and got["stem"] == []       # the fp16 kernels absorb no upsample
    nh, nw = d.net
    live = live_ranges(d, got["folds"])
    assert all(r is not None for r in live)
    for alias in (1, 0):
        arena, logical, rows, _ = got["plan"][alias]
        assert len(rows) == len(d.bufs) and sum(n for _, n in rows) == logical and arena <= logical
        for b, ((off, nbytes), (level, ch)) in enumerate(zip(rows, d.bufs)):
            es = 4 if b in d.head_buf else 2
            assert off % 16 == 0 and nbytes % 256 == 0 and nbytes >= BATCH * (nh >> level) * (nw >> level) * ch * es + SLACK, (alias, b)
            assert off + nbytes <= arena, (alias, b)
        for a in range(len(rows)):
            for b in range(a + 1, len(rows)):
                if not alias or (live[a][0] <= live[b][1] and live[b][0] <= live[a][1]):
                    (oa, na), (ob, nb_) = rows[a], rows[b]
                    assert oa + na <= ob or ob + nb_ <= oa, (alias, a, b)

    # the op list interpreted with fp16 storage against the fp32 oracle, input values as the window assembly makes them (u8 / 255)
    rng = np.random.default_rng(11)
    x = torch.from_numpy((rng.integers(0, 256, (2, 27, 32, 64)).astype(np.float64) / 255.0).astype(np.float32))
    want = tr.TrackNetRef(sd).forward(x)
    x32 = torch.zeros(2, 32, 32, 64)
    x32[:, :27] = x
    y32 = graph_interp.run(g32, buf0=x32)[g32.head_buf[0]][:, :8]
    y16 = graph_interp.run(g16, buf0=x32.half().float())[g16.head_buf[0]][:, :8]
    dirty = graph_interp.run(g16, buf0=x32.half().float(), stale=1000.0)[g16.head_buf[0]][:, :8]
    e32, e16 = float((y32 - want).abs().max()), float((y16 - want).abs().max())
    print(f"tracknet 32x64: fp32 interpretation vs oracle {e32:.2e}, fp16-storage emulation vs oracle {e16:.2e}, "
          f"heat range [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert float(want.max()) - float(want.min()) > 0.05, "a constant heat map would agree with anything"
    assert e32 <= 2e-5
    assert e16 <= 3 * E_EMU_WINDOW, f"fp16-storage emulation {e16:.2e} from the oracle"
    assert torch.equal(dirty, y16), "stale buffer contents leaked into the head"


def test_ball_tracker_half_option(sd, tmp_path):
    ck = tmp_path / "TrackNet_synth.pt"
    checkpoint.save_checkpoint(ck, sd, "tracknet", param_dict={"seq_len": 8, "bg_mode": "concat"})
    t = BallTracker(str(ck), None, 8, half=True)
    assert t.half and t.graph.dtype == G.DTYPE_F16 and t.full_range
    assert t.graph.blob().tobytes() == G.build_tracknet(sd, "f16").blob().tobytes()
    default = G.build_tracknet(sd, E.graph_dtype())
    t.use_full_range()                                              # the way back
    assert not t.half and t.fp32_mode == E.fp32_mode() and t.graph.dtype == default.dtype
    assert t.graph.blob().tobytes() == default.blob().tobytes()
    t0 = BallTracker(str(ck), None, 8)
    assert not t0.half and t0.graph.dtype == default.dtype and t0.graph.ops == default.ops and t0.graph.bufs == default.bufs
    assert t0.graph.blob().tobytes() == default.blob().tobytes()
    assert BallTracker(str(ck), None, 8, half=False).graph.blob().tobytes() == default.blob().tobytes()
