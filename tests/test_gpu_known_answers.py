"""The hand-derived known answers of tests/known_answers.py through the HIP decode / NMS kernels (postproc.hip) via
``pa_yolo_postprocess``: the product's Detect / Pose inference branch, NMS and scale_boxes / scale_coords on
caller-supplied head maps, against numbers worked out from the published formulas (no oracle in between)."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, graph as G, yolo_arch
from tests import known_answers as KA

pytestmark = pytest.mark.gpu


def _model(eng, nc, kpt, n):
    m = E.Model(eng, G.build_yolov8(yolo_arch.synth_state_dict("n", nc, kpt, seed=0), nc, kpt, dtype=E.graph_dtype()))
    m.set_max_batch(n)
    return m


def _check_rows(boxes, count, want, tag):
    assert count == len(want), f"{tag}: {count} rows, expected {len(want)}"
    for i, w in enumerate(want):
        g = boxes[i]
        assert np.array_equal(g[:4], np.asarray(w[:4], np.float32)), f"{tag} row {i}: box {g[:4]} != {w[:4]}"
        assert abs(float(g[4]) - w[4]) < 3e-7 and int(g[5]) == w[5], f"{tag} row {i}: score / class {g[4:6]} != {w[4:6]}"
    assert (boxes[count:] == 0).all(), f"{tag}: rows beyond the count must be zero"


@pytest.mark.parametrize("builder,classes", [(KA.detect_cases, None), (KA.detect_cases_class_filter, [1])], ids=["all", "classes=[1]"])
def test_detect_known_answers(gpu_engine, builder, classes):
    nc, heads, exp = builder()
    m = _model(gpu_engine, nc, None, len(heads[0]))
    assert [h.shape[1:] for h in heads] == [tuple(s) for s in m.head_shapes(KA.H0, KA.W0, KA.IMGSZ)]
    boxes, _, counts = m.yolo_postprocess(heads, KA.H0, KA.W0, imgsz=KA.IMGSZ, conf=0.5, iou=0.7, classes=classes)
    m.close()
    for i in range(len(counts)):
        _check_rows(boxes[i], int(counts[i]), exp[i], f"image {i}")


def test_detect_max_det_truncates_after_nms(gpu_engine):
    nc, heads, exp = KA.detect_cases()
    m = _model(gpu_engine, nc, None, len(heads[0]))
    boxes, _, counts = m.yolo_postprocess(heads, KA.H0, KA.W0, imgsz=KA.IMGSZ, conf=0.5, iou=0.7, max_det=2)
    m.close()
    for i in range(len(counts)):
        _check_rows(boxes[i], int(counts[i]), exp[i][:2], f"image {i} (max_det 2)")


def test_pose_known_answers(gpu_engine):
    nc, kshape, heads, rows, ek = KA.pose_cases()
    m = _model(gpu_engine, nc, kshape, 1)
    boxes, kpts, counts = m.yolo_postprocess(heads, KA.H0, KA.W0, imgsz=KA.IMGSZ, conf=0.25, iou=0.7, classes=[0])
    m.close()
    _check_rows(boxes[0], int(counts[0]), rows, "pose")
    k = kpts[0, 0].reshape(13, 3)
    assert np.array_equal(k[:, :2], ek[:, :2].astype(np.float32)), k[:3]
    assert np.allclose(k[:, 2], ek[:, 2], atol=3e-7)


def test_class_filter_of_postprocess_does_not_leak_into_infer(gpu_engine):
    """One class list on the device, one host copy of it: ``yolo_postprocess(classes=[1])`` between two
    ``yolo_infer(classes=[0])`` calls must not leave filter [1] behind for the second (the engine compares the caller's list
    with the host copy to skip the upload; a path that replaced the device list alone made the third call filter by class 1).
    64 x 64 frames at imgsz 64: the smallest size at which the calibrated synthetic YOLOv8n returns a class-0 detection."""
    from tests import synth
    from tests.helpers import calibrated_state_dict
    S = 64
    frames = synth.synthetic_frames(2, S, S, seed=3)
    sd = calibrated_state_dict("n", 80, None, [f[..., ::-1] for f in frames], S, 0.5, seed=5)
    m = E.Model(gpu_engine, G.build_yolov8(sd, 80, None, dtype=E.graph_dtype()))
    m.set_max_batch(2)
    kw = dict(imgsz=S, conf=0.5, iou=0.7)
    boxes0, _, counts0 = m.yolo_infer(frames, 2, S, S, classes=[0], **kw)
    assert int(counts0.sum()) >= 1 and (boxes0[0, :counts0[0], 5] == 0).all() and (boxes0[1, :counts0[1], 5] == 0).all(), counts0
    heads = [m.read_head(l, 2) for l in range(3)]
    _, _, counts_other = m.yolo_postprocess(heads, S, S, classes=[1], **kw)
    boxes1, _, counts1 = m.yolo_infer(frames, 2, S, S, classes=[0], **kw)
    m.close()
    assert not np.array_equal(counts_other, counts0), "the class-1 filter keeps other rows than the class-0 one"
    assert np.array_equal(counts1, counts0) and boxes1.tobytes() == boxes0.tobytes(), (counts0, counts1)
