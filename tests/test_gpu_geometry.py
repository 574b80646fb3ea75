"""letterbox_kernel and the rescale of decode_kernel / nms_kernel at odd source geometries (tests/known_answers.py: GEOMETRY_ODD — a
left pad, top != bottom, a rounded pad that differs from the unrounded one, upscales, portrait head maps, frame edges other than
1280 x 720), which the four sources of the other GPU tests never produce.

a. the network input byte for byte against the oracle's LetterBox (``ref.letterbox_u8``), on a synthetic frame and two frames of
   uniform random bytes (a weight that is off by one unit only shows on noise), both channel orders, auto on and off;
b. replanning one model through five geometries: tables and mode of an earlier plan must not survive;
c. hand-derived rescale known answers through ``yolo_postprocess``;
d. random head maps at every row against the oracle's decode + NMS + scale_boxes / scale_coords;
e. end to end (letterbox -> network -> decode -> NMS) with the bars of tests/test_gpu_yolo_parity.py.

The head maps of d. and the conditions they must meet (enough detections, coordinates clamped at 0 and at the frame edge) are checked
on the CPU in tests/test_letterbox_geometry_host.py."""
import numpy as np
import pytest
import torch

from oracle import yolov8_ref as ref
from padel_analytics_amd import engine as E, graph as G, yolo_arch
from tests import known_answers as KA
from tests import synth

pytestmark = pytest.mark.gpu

ROWS = KA.GEOMETRY_ODD
NETIN_ROWS = KA.GEOMETRY_ODD + KA.GEOMETRY_ODD_NO_AUTO
KW = dict(conf=0.5, iou=0.7)


def _new_model(eng, nc, kpt, batch):
    m = E.Model(eng, G.build_yolov8(yolo_arch.synth_state_dict("n", nc, kpt, seed=0), nc, kpt, dtype=E.graph_dtype()))
    m.set_max_batch(batch)
    return m


@pytest.fixture(scope="module")
def detect_model(gpu_engine):
    m = _new_model(gpu_engine, 2, None, 3)
    yield m
    m.close()


@pytest.fixture(scope="module")
def pose_model(gpu_engine):
    m = _new_model(gpu_engine, 1, (13, 3), 2)
    yield m
    m.close()


# ---------------------------------------------------------------------------------------- a. the network input
def frames_of(g, seed=0):
    """One synthetic frame and two frames of uniform random bytes at the row's source size."""
    h, w = g["hw"]
    rng = np.random.default_rng(1000 + seed)
    return np.concatenate([synth.synthetic_frames(1, h, w, seed=seed), rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)])


def oracle_netin(g, frames, reverse):
    want = np.stack([ref.letterbox_u8(f, g["imgsz"], auto=g["auto"]) for f in frames])
    return want[..., ::-1] if reverse else want


def check_netin(got, want, tag):
    assert got.shape == want.shape[:3] + (4,), f"{tag}: network input {got.shape}, the oracle's {want.shape}"
    assert not got[..., 3].any(), f"{tag}: the fourth byte must be zero"
    diff = got[..., :3] != want
    if diff.any():
        f, y, x, c = (int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{tag}: {int(diff.sum())} of {diff.size} bytes differ; first at (frame {f}, y {y}, x {x}, c {c}): "
                             f"{int(got[f, y, x, c])} != {int(want[f, y, x, c])}")


def check_pads(got, g, tag):
    """114 on all four sides, by the hand-derived pads alone (no oracle)."""
    top, bottom, left, right = g["pads"]
    nh, nw = g["net"]
    assert got.shape[1:3] == (nh, nw), (tag, got.shape)
    for name, band in (("top", got[:, :top]), ("bottom", got[:, nh - bottom:]), ("left", got[:, :, :left]), ("right", got[:, :, nw - right:])):
        assert (band[..., :3] == 114).all(), f"{tag}: {name} pad"


@pytest.mark.parametrize("reverse", [False, True], ids=["bgr", "reversed"])
@pytest.mark.parametrize("g", NETIN_ROWS, ids=[g["name"] for g in NETIN_ROWS])
def test_network_input_equals_the_oracle(detect_model, g, reverse):
    m, (h, w), S = detect_model, g["hw"], g["imgsz"]
    frames = frames_of(g)
    assert len({f.tobytes() for f in frames}) == 3
    m.yolo_infer(frames, 3, h, w, imgsz=S, channel_reverse=reverse, letterbox_auto=g["auto"], **KW)
    got = m.read_netin(3)
    tag = f"{g['name']} reverse {reverse}"
    check_pads(got, g, tag)
    check_netin(got, oracle_netin(g, frames, reverse), tag)
    shapes = [m.read_head(l, 3).shape[1:] for l in range(3)]
    assert shapes == [tuple(s) for s in m.head_shapes(h, w, S, letterbox_auto=g["auto"])], shapes
    assert [s[:2] for s in shapes] == [(hh, ww) for hh, ww, _ in KA.levels_of(g["net"])]


# ---------------------------------------------------------------------------------------- b. replanning
def test_replanning_one_model_leaves_nothing_behind(gpu_engine):
    """bilinear (vertical tables) -> copy -> bilinear (horizontal tables, portrait) -> 2 x 2 area -> the first again."""
    m = _new_model(gpu_engine, 2, None, 3)
    seen = []
    for row in (3, 0, 4, 2, 3):
        g = ROWS[row]
        frames = frames_of(g, seed=row)
        m.yolo_infer(frames, 3, *g["hw"], imgsz=g["imgsz"], **KW)
        got = m.read_netin(3)
        check_netin(got, oracle_netin(g, frames, False), f"plan {len(seen)} ({g['name']})")
        seen.append(got)
    m.close()
    assert seen[-1].tobytes() == seen[0].tobytes()


# ---------------------------------------------------------------------------------------- c. rescale known answers
def _check_rows(boxes, count, want, tag):
    assert count == len(want), f"{tag}: {count} rows, expected {len(want)}"
    for i, w in enumerate(want):
        g = boxes[i]
        assert np.array_equal(g[:4], np.asarray(w[:4], np.float32)), f"{tag} row {i}: box {g[:4]} != {w[:4]}"
        assert abs(float(g[4]) - w[4]) < 3e-7 and int(g[5]) == w[5], f"{tag} row {i}: score / class {g[4:6]} != {w[4:6]}"
    assert (boxes[count:] == 0).all(), f"{tag}: rows beyond the count must be zero"


def test_detect_rescale_known_answers(detect_model):
    nc, cases = KA.odd_detect_cases()
    for row, heads, want in cases:
        g = ROWS[row]
        boxes, _, counts = detect_model.yolo_postprocess(heads, *g["hw"], imgsz=g["imgsz"], **KW)
        _check_rows(boxes[0], int(counts[0]), want, g["name"])


@pytest.mark.parametrize("kpt_shape", [(13, 3), (12, 2)], ids=["13x3", "12x2"])
def test_pose_rescale_known_answers(gpu_engine, pose_model, kpt_shape):
    """13 x 3 at rows 1, 2, 9 and 8; 12 x 2 (no visibility channel) at row 8."""
    nc, cases = KA.odd_pose_cases(kpt_shape)
    m = pose_model if kpt_shape == (13, 3) else _new_model(gpu_engine, nc, kpt_shape, 1)
    for row, heads, want, ek in cases:
        if kpt_shape == (12, 2) and row != 7:
            continue
        g = ROWS[row]
        boxes, kpts, counts = m.yolo_postprocess(heads, *g["hw"], imgsz=g["imgsz"], conf=0.25, iou=0.7, classes=[0])
        _check_rows(boxes[0], int(counts[0]), want, g["name"])
        k = kpts[0, 0].reshape(kpt_shape)
        assert np.array_equal(k[:, :2], ek[:, :2].astype(np.float32)), (g["name"], k[:5], ek[:5])
        if kpt_shape[1] == 3:
            assert np.allclose(k[:, 2], ek[:, 2], atol=3e-7), g["name"]
    if m is not pose_model:
        m.close()


# ---------------------------------------------------------------------------------------- d. random heads at every row
WANTED = 40                 # anchors above the threshold per image (of 315 .. 5 040)
SEEDS = {"detect": 0, "pose": 0}


def random_heads(g, kind, seed):
    """Head maps the way tests/test_gpu_nms_stress.py makes them: normal DFL logits (spread 3: distances over the whole 0 .. 15 cells, so
    boxes leave the frame on every side), class logits above the threshold on a fraction of the anchors chosen so that about WANTED pass
    per image; pose: raw keypoint offsets N(0, 3) cells (x, y), N(0, 2) visibility logits.  -> (nc, kpt_shape, conf, heads)."""
    nc, kpt, conf = (2, None, 0.5) if kind == "detect" else (1, (13, 3), 0.25)
    nk = kpt[0] * kpt[1] if kpt else 0
    rng = np.random.default_rng(seed * 1000 + ROWS.index(g) * 10 + (kind == "pose"))
    heads = KA.blank_heads_net(g["net"], 2, nc, nk)
    frac = WANTED / sum(hh * ww for hh, ww, _ in KA.levels_of(g["net"]))
    for hd in heads:
        hd[..., :64] = rng.normal(0, 3.0, hd[..., :64].shape)
        logit = rng.normal(0, 2, hd.shape[:3])
        hot = logit > np.quantile(logit, 1 - frac)
        which = rng.integers(0, nc, hd.shape[:3])
        for c in range(nc):
            hd[..., 64 + c] = np.where(hot & (which == c), np.abs(logit) * 0.3 + 0.1, -20.0)
        if nk:
            k = rng.normal(0, 3.0, hd.shape[:3] + kpt)
            k[..., 2] = rng.normal(0, 2.0, hd.shape[:3] + (kpt[0],))
            hd[..., 64 + nc:64 + nc + nk] = k.reshape(hd.shape[:3] + (nk,))
    return nc, kpt, conf, heads


def oracle_post(g, nc, kpt, conf, heads):
    """-> per image (boxes (n, 6), kpts (n, K, dim) | None) in the source frame."""
    nk = kpt[0] * kpt[1] if kpt else 0
    mo = ref.YoloV8Ref({}, nc, kpt)
    det = [torch.from_numpy(h[..., :64 + nc]).permute(0, 3, 1, 2).contiguous() for h in heads]
    kp = [torch.from_numpy(h[..., 64 + nc:64 + nc + nk]).permute(0, 3, 1, 2).contiguous() for h in heads] if kpt else []
    out = ref.non_max_suppression(mo.decode(det, kp), conf, 0.7, None, 300, nc=nc)
    res = []
    for d in out:
        d = d.clone()
        d[:, :4] = ref.scale_boxes(g["net"], d[:, :4], g["hw"])
        k = ref.scale_coords(g["net"], d[:, 6:].view(len(d), *kpt), g["hw"]).numpy() if kpt else None
        res.append((d[:, :6].numpy(), k))
    return res


def check_oracle_is_not_empty(g, res):
    """The conditions of the issue on the ORACLE's output: every image keeps at least 5 detections; across the row some coordinate is
    clamped at 0 and some at w0 or h0."""
    h0, w0 = g["hw"]
    assert all(len(b) >= 5 for b, _ in res), [len(b) for b, _ in res]
    xs = np.concatenate([b[:, [0, 2]].ravel() for b, _ in res] + [k[..., 0].ravel() for _, k in res if k is not None])
    ys = np.concatenate([b[:, [1, 3]].ravel() for b, _ in res] + [k[..., 1].ravel() for _, k in res if k is not None])
    assert (xs == 0).any() or (ys == 0).any(), "nothing clamped at 0"
    assert (xs == w0).any() or (ys == h0).any(), "nothing clamped at the frame edge"
    assert ((xs > 0) & (xs < w0)).any() and ((ys > 0) & (ys < h0)).any()


@pytest.mark.parametrize("kind", ["detect", "pose"])
@pytest.mark.parametrize("g", ROWS, ids=[g["name"] for g in ROWS])
def test_postprocess_matches_oracle_on_random_heads(detect_model, pose_model, g, kind):
    nc, kpt, conf, heads = random_heads(g, kind, SEEDS[kind])
    m = detect_model if kind == "detect" else pose_model
    boxes, kpts, counts = m.yolo_postprocess(heads, *g["hw"], imgsz=g["imgsz"], conf=conf, iou=0.7)
    res = oracle_post(g, nc, kpt, conf, heads)
    check_oracle_is_not_empty(g, res)
    for i, (want, wk) in enumerate(res):
        got = boxes[i, :counts[i]]
        assert len(want) == len(got), f"image {i}: oracle kept {len(want)}, engine kept {counts[i]}"
        assert np.allclose(want, got, atol=2e-3), f"image {i}: first differing rank {int(np.argmax(~np.isclose(want, got, atol=2e-3).all(1)))}"
        assert (boxes[i, counts[i]:] == 0).all()
        if kpt:
            gk = kpts[i, :counts[i]].reshape(counts[i], *kpt)
            assert np.allclose(wk[..., :2], gk[..., :2], atol=2e-3), f"image {i}: keypoints, worst {np.abs(wk[..., :2] - gk[..., :2]).max():.3e} px"
            assert np.allclose(wk[..., 2], gk[..., 2], rtol=0, atol=3e-7), f"image {i}: visibilities, worst {np.abs(wk[..., 2] - gk[..., 2]).max():.3e}"


# ---------------------------------------------------------------------------------------- e. end to end
E2E = [(3, 80, None, 0.5), (4, 80, None, 0.5), (5, 80, None, 0.5), (8, 1, (13, 3), 0.25)]


def e2e_inputs(row, nc, kpt, conf):
    """-> (row dict, frames as the engine gets them, sources as upstream gets them, calibrated weights)."""
    from tests.test_gpu_yolo_parity import _calib
    g = ROWS[row]
    frames = synth.synthetic_frames(2, *g["hw"], seed=3)
    srcs = [f[..., ::-1] for f in frames]
    return g, frames, srcs, _calib("n", nc, kpt, srcs, g["imgsz"], conf, seed=5)


@pytest.mark.parametrize("row,nc,kpt,conf", E2E, ids=[("pose-n " if c[2] else "detect-n ") + ROWS[c[0]]["name"] for c in E2E])
def test_end_to_end_parity(gpu_engine, row, nc, kpt, conf):
    from tests.test_gpu_yolo_parity import _check, _engine_predict
    g, frames, srcs, sd = e2e_inputs(row, nc, kpt, conf)
    m, got = _engine_predict(gpu_engine, sd, nc, kpt, frames, imgsz=g["imgsz"], conf=conf, iou=0.7, classes=[0], channel_reverse=False)
    check_netin(m.read_netin(2), oracle_netin(g, frames, False), g["name"])       # upstream flips its (reversed) sources back
    m.close()
    _check(f"geometry {'pose' if kpt else 'detect'}-n {g['name']}", sd, nc, kpt, srcs, got, conf, 0.7, g["imgsz"])
