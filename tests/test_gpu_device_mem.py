"""``engine.device_bytes_live()`` (``pa_device_bytes_live``): the device bytes the library's own buffers hold, counted where they are
allocated and released (csrc/device_mem.h).  Every device buffer of the engine is released by the destructor of the struct that owns
it; that no struct keeps a buffer the type does not own is asserted here, as numbers that must return exactly:

* a model: the count rises with the weights, with the plan and with the second lane, and closing the model brings it back to what
  it was before the model; planning another source size and coming back, three times, gives the same count at every visit of a
  plan with the same number of lanes; so does ``set_max_batch`` 4 -> 2 -> 4;
* a ball session created and destroyed, unused and used (the median of host frames goes through a temporary);
* the scratch users ``yuv420_to_bgr`` (host source), ``render``, ``jpeg_encode`` and ``jpeg_decode``: a call at 32 x 48, one at 64 x 96
  that makes their buffers grow (the render call by its 2 000 marks: its staging holds marks, not pixels), one at 32 x 48 again:
  the count does not move between the second and the third, and the third gives the first's bytes.  (The encoder's gathered
  output has a floor of 1 MiB that frames of this size do not outgrow: its slots and tables are what grows.)
* closing the engine brings the count back to what it was before the engine.

Shapes as tests/test_gpu_lanes.py: YOLOv8n graphs of synthetic weights, 180 x 320 frames, imgsz 320, max_batch 4; TrackNet at
max_batch 2.  Every test has an engine of its own, so that its close can be observed.  The count is the library's, not the
card's: other tenants do not move it, and all equalities are exact."""
import gc

import numpy as np
import pytest

from oracle import tracknet_ref as tr
from padel_analytics_amd import engine as E, graph as G, render as R, video
from tests import synth, yuv_ref
from tests.test_gpu_lanes import B, H, S, W, collect, kwargs, make_model

pytestmark = pytest.mark.gpu

H2, W2 = 144, 256                    # the second source size (test_plan_changes_with_both_lanes_allocated)
live = E.device_bytes_live


@pytest.fixture
def own_engine():
    """An engine that is closed here, and the count from before it was created."""
    gc.collect()                     # models that earlier tests dropped without closing are released now, not in the middle
    before = live()
    eng = E.Engine(0)
    assert live() > before           # (the page of zeros the padded conv taps read)
    yield eng, before
    eng.close()
    assert live() == before


def both_lanes(m, clip, n, hw):
    """Two tickets in flight on n frames of clip, both collected: afterwards the model has its second lane."""
    view = clip.buffer.view(0, n * clip.frame_bytes)
    ts = [m.yolo_submit(view, n, *hw, **kwargs()) for _ in range(2)]
    out = [collect(m, t) for t in ts]
    assert m.lanes_allocated() == 2
    return out


def test_model_lifecycle_replan_and_max_batch(own_engine):
    eng, _ = own_engine
    clip = video.DeviceClip(eng, synth.synthetic_frames(B, H, W, seed=77))            # (pa_device_malloc: the caller's, not counted)
    small = video.DeviceClip(eng, synth.synthetic_frames(B, H2, W2, seed=78))
    with_engine = live()
    m = make_model(eng, "pose")
    with_weights = live()
    assert with_weights > with_engine and m.lanes_allocated() == 0
    first = m.yolo_infer(clip.buffer, B, H, W, **kwargs())
    with_plan = live()
    assert with_plan > with_weights and m.lanes_allocated() == 1
    got = both_lanes(m, clip, B, (H, W))
    at_first_size = live()
    assert at_first_size > with_plan
    for g in got:                                                                      # (and the lanes still compute)
        assert np.array_equal(g[0], first[0]) and np.array_equal(g[2], first[2])
    # another plan and back, three times
    at_second_size = None
    for _ in range(3):
        both_lanes(m, small, B, (H2, W2))
        print("second size:", live())
        assert at_second_size in (None, live())
        at_second_size = live()
        both_lanes(m, clip, B, (H, W))
        print("first size:", live(), "at the first visit:", at_first_size)
        assert live() == at_first_size
    # max_batch 4 -> 2 -> 4
    m.set_max_batch(2)
    assert m.lanes_allocated() == 0 and live() < at_first_size
    both_lanes(m, clip, 2, (H, W))
    assert live() < at_first_size
    m.set_max_batch(B)
    both_lanes(m, clip, B, (H, W))
    assert live() == at_first_size
    m.close()
    assert live() == with_engine
    clip.free()
    small.free()


def test_ball_session(own_engine):
    eng, _ = own_engine
    m = E.Model(eng, G.build_tracknet(tr.synth_tracknet_state_dict(1), dtype=E.graph_dtype()))
    m.set_max_batch(2)
    frames = synth.synthetic_frames(9, 90, 160, seed=4)
    before = live()
    sess = E.BallSession(m, 90, 160)
    assert live() > before
    sess.close()
    assert live() == before
    used = None
    for _ in range(2):                   # the first session's feed plans the model: that memory is the model's and stays
        sess = E.BallSession(m, 90, 160)
        sess.background_from_frames(frames)                                            # host frames: through a temporary
        masks = [sess.feed(frames[i:i + 2])[0] for i in range(0, 8, 2)] + [sess.feed(None, flush=True)[0]]
        assert sum(len(k) for k in masks) == 8
        sess.close()
        print("after a used session:", live())
        assert used in (None, live())
        used = live()
    assert used > before
    m.close()


def scratch_round(eng, h, w, n_marks):
    """One call of each scratch user on one frame of h x w -> (their outputs, the count after each call)."""
    frame = synth.synthetic_frames(1, h, w, seed=11)
    raw, _ = yuv_ref.bgr_to_yuv420(frame, "nv12")
    raw = np.ascontiguousarray(raw, np.uint8).ravel()
    geom = video.yuv_desc(w, h, "i420", range="full")
    bgr, yuv, back = eng.alloc(h * w * 3), eng.alloc(video.yuv_span(1, h, w, geom)), eng.alloc(h * w * 3)
    counts, outs = [], []
    try:
        eng.yuv420_to_bgr(raw, 1, h, w, video.yuv_desc(w, h, "nv12"), bgr)
        counts.append(live())
        outs.append(bgr.download(np.empty(h * w * 3, np.uint8)))
        marks, first = R.pack([[R.disc(3 + k % (w - 6), 3 + k // (w - 6) % (h - 6), 2, (k % 256, 255 - k % 256, 90)) for k in range(n_marks)]])
        eng.render(bgr, 1, h, w, marks, first, yuv, out=E.RENDER_YUV420, geom=geom, enc=video.YUV_ENC_COEFFS["bt601_full"])
        counts.append(live())
        outs.append(yuv.download(np.empty(yuv.nbytes, np.uint8)))
        data, offsets = eng.jpeg_encode(yuv, 1, h, w, geom, 90)
        counts.append(live())
        outs += [data.copy(), offsets.copy()]
        status = eng.jpeg_decode(data, offsets, back, h, w)
        counts.append(live())
        assert status.tolist() == [0]
        outs.append(back.download(np.empty(h * w * 3, np.uint8)))
    finally:
        for b in (bgr, yuv, back):
            b.free()
    return outs, counts


def test_scratch_users_grow_and_do_not_shrink(own_engine):
    eng, _ = own_engine
    start = live()
    first, c1 = scratch_round(eng, 32, 48, 5)
    _, c2 = scratch_round(eng, 64, 96, 2000)
    third, c3 = scratch_round(eng, 32, 48, 5)
    print("after yuv, render, encode, decode:", c1, c2, c3)
    assert start < c1[0] < c1[1] < c1[2] < c1[3]                                        # every user has scratch of its own
    assert c1[3] < c2[0] < c2[1] < c2[2] < c2[3]                                        # ... which the larger call outgrows
    assert c3 == [c2[3]] * 4                                                            # ... and the smaller one leaves alone
    assert len(first) == len(third) == 5
    for a, b in zip(first, third):
        assert a.dtype == b.dtype and np.array_equal(a, b)
