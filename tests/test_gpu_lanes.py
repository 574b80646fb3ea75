"""Lanes (include/padel_hip.h, pa_yolo_submit): alternate in-flight YOLO tickets run on two streams, each with its own network
input, activation arena and post-processing buffers.  Every ticket must give, bitwise, what the synchronous call gives on the
same frames — boxes, keypoints, counts, overflow flag — and the engine's stream must still order everything as one stream did.

Shapes as tests/test_gpu_pipeline.py: YOLOv8n graphs of synthetic weights, 180 x 320 frames, imgsz 320, max_batch 4; every
batch has its own frame content, so a lane that read its neighbour's memory or a stale byte gives another batch's boxes.
The PIL-stretch cases run on 144 x 256 frames: BOTH axes change on the way to 320 x 320, so the resample is two passes through a
temporary, of which every lane has its own (180 x 320 would be a vertical pass alone); ``resample_passes() == 2`` says so."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, graph as G, video, yolo_arch
from tests import synth, yuv_ref

pytestmark = pytest.mark.gpu

H, W, S, B = 180, 320, 320, 4
HS, WS = 144, 256                   # the stretch cases' frames: neither side is S
KPT = (13, 3)
MODELS = {"det1": (1, None), "det80": (80, None), "pose": (1, KPT)}
NBATCH = 6


def make_model(eng, kind, dtype=None, max_batch=B):
    nc, kpt = MODELS[kind]
    sd = yolo_arch.synth_state_dict("n", nc, kpt, seed=2, cls_bias=1.0)
    m = E.Model(eng, G.build_yolov8(sd, nc, kpt, dtype=dtype or E.graph_dtype()))
    m.set_max_batch(max_batch)
    return m


def kwargs(pre="letterbox"):
    return dict(imgsz=S, conf=0.25, iou=0.7, classes=[0], pre_mode=E.PRE_PIL_STRETCH if pre == "stretch" else E.PRE_LETTERBOX)


@pytest.fixture(scope="module")
def clip(gpu_engine):
    c = video.DeviceClip(gpu_engine, synth.synthetic_frames(NBATCH * B, H, W, seed=77))
    yield c
    c.free()


@pytest.fixture(scope="module")
def stretch_clip(gpu_engine):
    c = video.DeviceClip(gpu_engine, synth.synthetic_frames(NBATCH * B, HS, WS, seed=79))
    yield c
    c.free()


def clip_for(pre, clip, stretch_clip):
    """(clip, (h, w)) of a preprocessing mode."""
    return (stretch_clip, (HS, WS)) if pre == "stretch" else (clip, (H, W))


def views_of(clip, per=B, n=NBATCH):
    return [clip.buffer.view(i * B * clip.frame_bytes, per * clip.frame_bytes) for i in range(n)]


def keep(res):
    return tuple(None if a is None else np.array(a) for a in res[:3])


def same(got, want):
    assert got[3] is False
    for a, b in zip(got[:3], want):
        assert (a is None and b is None) or np.array_equal(a, b)


def collect(m, ticket):
    r = m.yolo_wait(ticket)
    return keep(r) + (r[3],)


def sync_results(m, views, n, kw, hw=(H, W)):
    return [keep(m.yolo_infer(v, n, *hw, **kw)) for v in views]


def two_in_flight(m, views, n, kw, lanes=None, hw=(H, W)):
    """The trackers' loop: submit k + 1, then wait k.  lanes (a list): the lane of every submit is appended."""
    out, prev = [], None
    for v in views:
        t = m.yolo_submit(v, n, *hw, **kw)
        if lanes is not None:
            lanes.append(m.last_lane())
        if prev is not None:
            out.append(collect(m, prev))
        prev = t
    out.append(collect(m, prev))
    return out


CASES = [("det1", "letterbox", None), ("det80", "stretch", None), ("pose", "letterbox", None), ("pose", "stretch", "f32")]


@pytest.mark.parametrize("kind,pre,dtype", CASES, ids=[f"{k}-{p}-{d or 'default'}" for k, p, d in CASES])
def test_two_lanes_equal_the_synchronous_call_bitwise(gpu_engine, clip, stretch_clip, kind, pre, dtype):
    m = make_model(gpu_engine, kind, dtype)
    kw = kwargs(pre)
    src, hw = clip_for(pre, clip, stretch_clip)
    views = views_of(src)
    assert m.lanes_allocated() == 0
    want = sync_results(m, views, B, kw, hw)
    short = keep(m.yolo_infer(views[5], 3, *hw, **kw))                  # one ticket with n < max_batch
    assert m.resample_passes() == (2 if pre == "stretch" else 0)        # stretch: through the temporary, not one pass alone
    assert sum(int(w[2].sum()) for w in want) > 0 and len({w[0].tobytes() for w in want}) == NBATCH, "the batches must differ"
    # two in flight: the lanes alternate
    lanes = []
    got = two_in_flight(m, views, B, kw, lanes, hw)
    assert lanes == [0, 1, 0, 1, 0, 1] and m.lanes_allocated() == 2
    for g, w in zip(got, want):
        same(g, w)
    # four in flight, one of them short, collected out of submission order
    ts = [m.yolo_submit(views[i], B, *hw, **kw) for i in range(3)] + [m.yolo_submit(views[5], 3, *hw, **kw)]
    for i in (3, 1, 0, 2):
        same(m.yolo_wait(ts[i]), short if i == 3 else want[i])
    assert not m.take_overflow()
    m.close()


def test_lazy_allocation(gpu_engine, clip, stretch_clip):
    """A model that is only ever called synchronously has one lane; so has one whose submits are each waited for before the next."""
    for pre in ("letterbox", "stretch"):
        m = make_model(gpu_engine, "pose")
        kw = kwargs(pre)
        src, hw = clip_for(pre, clip, stretch_clip)
        views = views_of(src, n=3)
        assert m.lanes_allocated() == 0
        want = sync_results(m, views, B, kw, hw)
        assert m.lanes_allocated() == 1 and m.last_lane() == 0
        arena = m.plan_bytes()
        for v, w in zip(views, want):
            same(m.yolo_wait(m.yolo_submit(v, B, *hw, **kw)), w)
            assert m.lanes_allocated() == 1 and m.last_lane() == 0
        two_in_flight(m, views[:2], B, kw, hw=hw)
        assert m.lanes_allocated() == 2 and m.plan_bytes() == arena      # plan_bytes keeps reporting one lane's plan
        m.close()


def test_lanes_1_never_uses_the_second_lane(gpu_engine, clip):
    m = make_model(gpu_engine, "pose")
    kw = kwargs()
    views = views_of(clip, n=4)
    want = sync_results(m, views, B, kw)
    gpu_engine.set_tuning(lanes=1)
    try:
        lanes = []
        got = two_in_flight(m, views, B, kw, lanes)
        assert lanes == [0, 0, 0, 0] and m.lanes_allocated() == 1
    finally:
        gpu_engine.set_tuning(lanes=2)
    for g, w in zip(got, want):
        same(g, w)
    m.close()


def test_isolation_after_fill_arena(gpu_engine, stretch_clip):
    """NaN patterns in both lanes' arenas and network inputs, then two tickets in flight through the two-pass stretch: each lane's
    vertical pass must read the temporary its own horizontal pass wrote."""
    hw = (HS, WS)
    m = make_model(gpu_engine, "pose")
    kw = kwargs("stretch")
    views = views_of(stretch_clip, n=6)
    want = sync_results(m, views, B, kw, hw)
    assert m.resample_passes() == 2
    two_in_flight(m, views[:2], B, kw, hw=hw)                           # both lanes exist
    assert m.lanes_allocated() == 2
    m.fill_arena(0xFF)
    lanes = []
    got = two_in_flight(m, views[2:4], B, kw, lanes, hw)
    assert lanes == [0, 1]
    for g, w in zip(got, want[2:4]):
        same(g, w)
    m.fill_arena(0xFF)
    ts = [m.yolo_submit(v, B, *hw, **kw) for v in views[2:6]]           # four in flight
    for i in (1, 3, 0, 2):
        same(m.yolo_wait(ts[i]), want[2 + i])
    m.close()


def _yuv_clips(n):
    """Two different clips of n frames as tightly packed NV12 bytes."""
    raws = []
    for seed in (5, 6):
        raw, _ = yuv_ref.bgr_to_yuv420(synth.synthetic_frames(n, H, W, seed=seed), "nv12")
        raws.append(np.ascontiguousarray(raw, np.uint8).ravel())
    return raws


def test_ordering_against_the_engine_stream_conversion(gpu_engine):
    """ONE frame buffer: convert clip X into it, submit, convert clip Y into the same buffer, submit.  The first ticket must have
    read X (the second conversion waits for it: join), the second Y (its lane waits for the conversion: fork)."""
    eng = gpu_engine
    m = make_model(eng, "pose")
    kw = kwargs()
    x, y = _yuv_clips(B)
    desc = video.yuv_desc(W, H, "nv12")
    buf = E.DeviceBuffer(eng, B * H * W * 3)
    want = []
    for raw in (x, y):
        eng.yuv420_to_bgr(raw, B, H, W, desc, buf)
        want.append(keep(m.yolo_infer(buf, B, H, W, **kw)))
    assert not np.array_equal(want[0][0], want[1][0]) and int(want[0][2].sum()) > 0
    for rep in range(2):                                                # the second round starts with both lanes allocated
        eng.yuv420_to_bgr(x, B, H, W, desc, buf)
        t0 = m.yolo_submit(buf, B, H, W, **kw)
        l0 = m.last_lane()
        eng.yuv420_to_bgr(y, B, H, W, desc, buf)
        t1 = m.yolo_submit(buf, B, H, W, **kw)
        assert (l0, m.last_lane()) == (0, 1)
        same(m.yolo_wait(t1), want[1])
        same(m.yolo_wait(t0), want[0])
    buf.free()
    m.close()


@pytest.mark.parametrize("copy_stream", [False, True], ids=["memcpy_h2d", "pa_upload"])
def test_ordering_against_the_engine_stream_upload(gpu_engine, copy_stream):
    """The same with an upload in place of the conversion.  pa_memcpy_h2d runs on the engine's stream: it waits for the ticket
    that still reads the buffer.  pa_upload runs on the copy stream, which nothing orders (padel_hip.h: pa_engine_synchronize
    first) — and that synchronize must wait for the ticket, on whichever lane it runs."""
    eng = gpu_engine
    m = make_model(eng, "det1")
    kw = kwargs()
    x = synth.synthetic_frames(B, H, W, seed=5)
    y = synth.synthetic_frames(B, H, W, seed=6)
    buf = E.DeviceBuffer(eng, B * H * W * 3)
    want = []
    for fr in (x, y):
        buf.upload(fr)
        want.append(keep(m.yolo_infer(buf, B, H, W, **kw)))
    assert not np.array_equal(want[0][0], want[1][0]) and int(want[0][2].sum()) > 0
    for rep in range(2):
        buf.upload(x, copy_stream=copy_stream)
        t0 = m.yolo_submit(buf, B, H, W, **kw)
        if copy_stream:
            eng.synchronize()
        buf.upload(y, copy_stream=copy_stream)
        t1 = m.yolo_submit(buf, B, H, W, **kw)
        assert m.last_lane() == 1
        same(m.yolo_wait(t0), want[0])
        same(m.yolo_wait(t1), want[1])
    buf.free()
    m.close()


def test_read_head_after_a_ticket_on_lane_1(gpu_engine, clip):
    if E.fp32_mode() != "h2":
        pytest.skip("the fused head tail is an h2 kernel")
    m = make_model(gpu_engine, "pose")
    kw = kwargs()
    views = views_of(clip, n=2)
    m.yolo_infer(views[1], B, H, W, **kw)
    assert m.last_post_path() == E.POST_PATH_FUSED
    want = [m.read_head(l, B) for l in range(3)]
    t0 = m.yolo_submit(views[0], B, H, W, **kw)
    t1 = m.yolo_submit(views[1], B, H, W, **kw)
    m.yolo_wait(t0)
    m.yolo_wait(t1)
    assert m.last_lane() == 1 and m.last_post_path() == E.POST_PATH_FUSED
    for l in range(3):
        assert np.array_equal(m.read_head(l, B), want[l])
    net = m.read_netin(B)
    m.yolo_infer(views[1], B, H, W, **kw)
    assert m.last_lane() == 0 and np.array_equal(m.read_netin(B), net)
    m.close()


def test_plan_changes_with_both_lanes_allocated(gpu_engine, clip):
    kw = kwargs()
    m = make_model(gpu_engine, "pose")
    views = views_of(clip, n=2)
    two_in_flight(m, views, B, kw)
    assert m.lanes_allocated() == 2
    # a smaller batch
    fresh = make_model(gpu_engine, "pose", max_batch=2)
    halves = views_of(clip, per=2, n=3)
    want = sync_results(fresh, halves, 2, kw)
    m.set_max_batch(2)
    assert m.lanes_allocated() == 0
    lanes = []
    got = two_in_flight(m, halves, 2, kw, lanes)
    assert lanes == [0, 1, 0] and m.lanes_allocated() == 2
    for g, w in zip(got, want):
        same(g, w)
    # another source size
    h2, w2 = 144, 256
    small = video.DeviceClip(gpu_engine, synth.synthetic_frames(4, h2, w2, seed=78))
    sv = [small.buffer.view(i * 2 * small.frame_bytes, 2 * small.frame_bytes) for i in range(2)]
    want = [keep(fresh.yolo_infer(v, 2, h2, w2, **kw)) for v in sv]
    ts = [m.yolo_submit(v, 2, h2, w2, **kw) for v in sv]
    assert m.lanes_allocated() == 2 and m.last_lane() == 1
    for t, w in zip(ts, want):
        same(m.yolo_wait(t), w)
    fresh.close()
    # close with a ticket in flight on each lane, then the pages and the memory are reused
    m.yolo_submit(sv[0], 2, h2, w2, **kw)
    m.yolo_submit(sv[1], 2, h2, w2, **kw)
    assert m.last_lane() == 1
    m.close()
    again = make_model(gpu_engine, "pose", max_batch=2)
    for v, w in zip(sv, want):
        for a, b in zip(keep(again.yolo_infer(v, 2, h2, w2, **kw)), w):
            assert np.array_equal(a, b)
    again.close()
    small.free()


def test_captured_replay_on_two_lanes(gpu_engine, clip):
    m = make_model(gpu_engine, "det80")
    kw = kwargs()
    views = views_of(clip, n=4)
    want = sync_results(m, views, B, kw)
    gpu_engine.set_tuning(graph=1)
    try:
        lanes = []
        got = two_in_flight(m, views, B, kw, lanes)
        assert lanes == [0, 1, 0, 1]
        again = sync_results(m, views[:1], B, kw)
    finally:
        gpu_engine.set_tuning(graph=0)
    for g, w in zip(got + [again[0] + (False,)], want + want[:1]):
        same(g, w)
    m.close()
