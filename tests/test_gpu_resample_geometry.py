"""resample_pass_kernel / resample_vpass4_kernel and the enqueue logic around them (csrc/engine_pre.cpp) at the geometries of
tests/resample_rows.py, byte for byte against Pillow: a horizontal pass that is the last pass, single vertical passes through vpass4 and
— from a source pointer that is not 4-byte aligned — through the generic kernel's 3 -> 4-byte path, a source of the target size, odd
sizes, frames of an odd byte count in batches, one axis up and the other down, both channel orders, the clip on both sides, 49 and 29
taps; the ball session's resize (3 -> 3 bytes, the one-tap identity pass, the ring wrapping inside one feed) through
``BallSession.read_resized``.  What each row is meant to reach, and that its frames overshoot, is checked on the CPU in
tests/test_resample_geometry_host.py.  Equality is exact: there is no tolerance.

Every network input is built over stale bytes (``Model.fill_arena`` overwrites it with 0xA5 between the run that makes the plan and the
run that is read back), so a byte that no launch writes cannot pass by luck.  The same-size YOLO row passes because ``yolo_enqueue``
hands a source of the network's size to the letterbox kernel in copy mode, as the ResNet path does; a library built without that
branch runs no launch at all and fails the row with all 76 800 fourth bytes (and every other byte) still 0xA5."""
import numpy as np
import pytest

from oracle import tracknet_ref as tr
from padel_analytics_amd import engine as E, graph as G, yolo_arch
from tests import resample_rows as RR

pytestmark = pytest.mark.gpu

KW = dict(imgsz=RR.YOLO_S, conf=0.5, iou=0.7, pre_mode=E.PRE_PIL_STRETCH)


def check_bytes(got, want, tag):
    assert got.shape == want.shape, f"{tag}: {got.shape}, Pillow's {want.shape}"
    diff = got != want
    if diff.any():
        f, y, x, c = (int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} bytes differ; first at (frame {f}, y {y}, x {x}, c {c}): "
                             f"{int(got[f, y, x, c])} != {int(want[f, y, x, c])}")


def check_netin(got, want, tag):
    assert got.shape == want.shape[:3] + (4,), f"{tag}: network input {got.shape}, Pillow's {want.shape}"
    assert not got[..., 3].any(), f"{tag}: the fourth byte must be zero ({int((got[..., 3] != 0).sum())} are not)"
    check_bytes(got[..., :3], want, tag)


# ---------------------------------------------------------------------------------------- YOLO stretch
@pytest.fixture(scope="module")
def yolo_model(gpu_engine):
    m = E.Model(gpu_engine, G.build_yolov8(yolo_arch.synth_state_dict("n", 2, None, seed=0), 2, None, dtype=E.graph_dtype()))
    m.set_max_batch(3)
    yield m
    m.close()


STALE = 0xA5                # what the network input holds before the run that is read back (Model.fill_arena)


def yolo_netin(m, row, frames, reverse):
    """The network input of ``frames``, built over a network input of STALE bytes: a first run makes the plan, fill_arena overwrites
    what it left, the second run is read back.  A byte the preprocessing does not write — the fourth of a pixel, every byte when
    nothing is launched — shows as 0xA5."""
    n, (h, w) = len(frames), row["hw"]
    buf = view = None
    if row["src_offset"]:
        buf = m.engine.alloc(frames.nbytes + row["src_offset"])
        view = buf.view(row["src_offset"], frames.nbytes).upload(frames)
        assert view.ptr % 4 == row["src_offset"] % 4
    try:
        for stale in (False, True):
            if stale:
                m.fill_arena(STALE)
                assert (m.read_netin(n) == STALE).all()
            if view is None:
                m.yolo_infer(frames, n, h, w, channel_reverse=reverse, **KW)
            else:
                m.yolo_wait(m.yolo_submit(view, n, h, w, channel_reverse=reverse, **KW))
        return m.read_netin(n)
    finally:
        if buf is not None:
            buf.free()


@pytest.mark.parametrize("reverse", [False, True], ids=["as given", "reversed"])
@pytest.mark.parametrize("row", RR.YOLO_ROWS, ids=[r["name"] for r in RR.YOLO_ROWS])
def test_yolo_stretch_equals_pillow(yolo_model, row, reverse):
    name, tag = row["name"], f"{row['name']} reverse {reverse}"
    if (RR.COPY,) == row["reach"]:
        # another frame set of the same geometry first: a launch that never happened would leave ITS bytes or STALE ones, and a lucky
        # zero-filled allocation cannot pass
        other = RR.frames_of(name, 1)
        assert other.tobytes() != RR.frames_of(name).tobytes()
        check_netin(yolo_netin(yolo_model, row, other, reverse), RR.pillow_of(name, 1)[..., ::-1] if reverse else RR.pillow_of(name, 1),
                    tag + " (the frames before)")
    got = yolo_netin(yolo_model, row, RR.frames_of(name), reverse)
    want = RR.pillow_of(name)
    check_netin(got, want[..., ::-1] if reverse else want, tag)


@pytest.mark.parametrize("reverse", [False, True], ids=["as given", "reversed"])
def test_misaligned_source_gives_the_bytes_of_the_aligned_one(yolo_model, reverse):
    """vpass4 and the generic kernel's vertical 3 -> 4-byte path (the launcher's choice for a source pointer at byte offset 1)."""
    rows = {r["name"]: r for r in RR.YOLO_ROWS}
    got = [yolo_netin(yolo_model, rows[n], RR.frames_of(n), reverse).tobytes() for n in ("yolo 117x160", "yolo 117x160 +1")]
    assert got[0] == got[1]


# ---------------------------------------------------------------------------------------- ResNet stretch
@pytest.fixture(scope="module")
def resnet_model(gpu_engine):
    g = G.Graph(task=G.TASK_RESNET)                      # any PA_TASK_RESNET graph builds the network input: the stem alone is enough
    st = g.buf(1, 64)
    g.stem7(np.zeros((64, 3, 7, 7), np.float32), np.zeros(64, np.float32), (st, 0))
    g.head_buf = (st, -1, -1)
    m = E.Model(gpu_engine, g)
    m.set_max_batch(3)
    yield m
    m.close()


@pytest.mark.parametrize("row", RR.RESNET_ROWS, ids=[r["name"] for r in RR.RESNET_ROWS])
def test_resnet_stretch_equals_pillow(resnet_model, row):
    frames = RR.frames_of(row["name"])                    # BGR as the tracker hands them over; the network sees RGB
    resnet_model.resnet_infer(frames, len(frames), *row["hw"])
    resnet_model.fill_arena(STALE)                        # the run that is read back writes over stale bytes, the fourth included
    assert (resnet_model.resnet_read_netin(len(frames)) == STALE).all()
    resnet_model.resnet_infer(frames, len(frames), *row["hw"])
    check_netin(resnet_model.resnet_read_netin(len(frames)), RR.pillow_of(row["name"])[..., ::-1], row["name"])


# ---------------------------------------------------------------------------------------- ball stretch
@pytest.fixture(scope="module")
def ball_model(gpu_engine):
    m = E.Model(gpu_engine, G.build_tracknet(tr.synth_tracknet_state_dict(1), dtype=E.graph_dtype()))
    m.set_max_batch(2)
    yield m
    m.close()


@pytest.mark.parametrize("row", RR.BALL_ROWS, ids=[r["name"] for r in RR.BALL_ROWS])
def test_ball_resize_equals_pillow(ball_model, row):
    """The background arrives RGB and is stored RGB (reverse = 0); frames arrive BGR and are stored RGB (reverse = 1).  Eleven frames,
    two per feed, into the ring of 2 + 7 slots: frames 0 .. 7 are read back before the ring wraps, the fifth feed puts frame 8 into
    slot 8 and frame 9 into slot 0 (the second resize call of a feed, from the second frame of the upload), the ring then holds frames
    2 .. 10.  The TrackNet graph runs on synthetic weights; its outputs are not asserted here."""
    name = row["name"]
    frames, want = RR.frames_of(name), RR.pillow_of(name)[..., ::-1]
    assert len(frames) == RR.BALL_FRAMES == 11 and ball_model.max_batch == 2
    sess = E.BallSession(ball_model, *row["hw"])
    try:
        bg = RR.frames_of(name, 1)[0]
        sess.set_background(bg)
        check_bytes(sess.read_resized()[None], RR.pillow_of(name, 1)[:1], f"{name} background")
        with pytest.raises(E.EngineError, match="not among the last"):
            sess.read_resized(0)
        for i in range(0, 8, 2):
            sess.feed(frames[i:i + 2])
        check_bytes(np.stack([sess.read_resized(i) for i in range(8)]), want[:8], f"{name} frames 0 .. 7")
        sess.feed(frames[8:10])
        sess.feed(frames[10:11])
        check_bytes(np.stack([sess.read_resized(i) for i in range(2, 11)]), want[2:11], f"{name} frames 2 .. 10 (the whole ring)")
        for gone in (1, 11):
            with pytest.raises(E.EngineError, match="not among the last"):
                sess.read_resized(gone)
        check_bytes(sess.read_resized()[None], RR.pillow_of(name, 1)[:1], f"{name} background after the feeds")
    finally:
        sess.close()
