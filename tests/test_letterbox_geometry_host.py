"""Letterbox geometry and cv2 bilinear tables at odd source sizes, on the CPU: the engine's host code (csrc/graph_plan.cpp through the
stand-alone harness tests/graph_plan_main.cpp) against the oracle (oracle/yolov8_ref.py) and both against numbers worked out by hand
(tests/known_answers.py: GEOMETRY_ODD, odd_detect_cases, odd_pose_cases).

* ``cv2_linear_table`` (C++) equals ``cv2_linear_coeffs`` (numpy) number for number: the resizes of every hand-derived row, of every
  source the suite used before, and a sweep of every source length 2 .. 2200 against seven output lengths.  Both are single precision
  after the cast, like OpenCV's ``float fx``; a hand-worked output where single and double precision give different weights pins
  which one it is.  (Read from OpenCV's source — not checked against a run of cv2, which is not installed where this runs.)
* ``yolo_geometry`` (C++) equals ``letterbox_geometry`` (Python) on resized size, top, left, network size and mode: the rows and a sweep
  over both orientations, imgsz 160 / 320 / 640, auto on and off.
* the hand-derived rows and rescale cases through the oracle, so that the GPU tests (tests/test_gpu_geometry.py) and the oracle are
  pinned to the same numbers."""
import numpy as np
import pytest
import torch

from oracle import yolov8_ref as ref
from tests import known_answers as KA
from tests.test_graph_plan_host import ask, build_harness

ROWS = KA.GEOMETRY_ODD + KA.GEOMETRY_ODD_NO_AUTO
USED_BEFORE = ((1280, 640), (854, 640), (1920, 640), (720, 360), (1080, 360), (480, 360))      # (source, output) lengths of the suite's sources
SWEEP_DST = (160, 193, 237, 320, 360, 362, 640)
SWEEP_SRC = range(2, 2201)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("letterbox_geometry") / "graph_plan_main")


def resizes_of(rows):
    """(source, output) length of every axis the rows resize with the tables."""
    out = []
    for g in rows:
        if g["mode"] == 2:
            out += [(g["hw"][1], g["resized"][0]), (g["hw"][0], g["resized"][1])]
    return sorted(set(p for p in out if p[0] != p[1]))


def tables(exe, pairs):
    lines = ask(exe, "".join(f"cv2 {s} {d}\n" for s, d in pairs))
    assert len(lines) == len(pairs)
    return [np.array(ln.split()[1:], dtype=np.int64) for ln in lines]


def oracle_table(src, dst):
    return np.stack(ref.cv2_linear_coeffs(src, dst), 1).reshape(-1)


def assert_tables_equal(exe, pairs):
    bad = []
    for (s, d), got in zip(pairs, tables(exe, pairs)):
        want = oracle_table(s, d)
        assert got.shape == want.shape == (3 * d,), (s, d)
        n = int((got != want).sum())
        if n:
            bad.append(f"{s}->{d}: {n} of {3 * d}")
    assert not bad, f"{len(bad)} of {len(pairs)} tables differ from the oracle's coefficients: " + ", ".join(bad[:12])


# ---------------------------------------------------------------------------------------- the tables
def test_rows_resize_what_they_are_meant_to():
    pairs = resizes_of(ROWS)
    for p in ((201, 193), (97, 237), (363, 182), (768, 360), (64, 160), (48, 120), (97, 118)):
        assert p in pairs, p


def test_table_equals_oracle_coefficients_on_the_rows(harness):
    assert_tables_equal(harness, resizes_of(ROWS) + [(725, 362)] + list(USED_BEFORE))


def test_table_equals_oracle_coefficients_sweep(harness):
    assert_tables_equal(harness, [(s, d) for d in SWEEP_DST for s in SWEEP_SRC])


def test_oracle_coefficients_are_well_formed():
    for s, d in resizes_of(ROWS) + list(USED_BEFORE):
        idx, c0, c1 = ref.cv2_linear_coeffs(s, d)
        assert idx.dtype == c0.dtype == c1.dtype == np.int64 and len(idx) == d
        assert (c0 + c1 == 2048).all() and (c0 >= 0).all() and (c1 >= 0).all(), (s, d)
        assert idx.min() >= 0 and idx.max() <= s - 1 and (np.diff(idx) >= 0).all(), (s, d)
        assert (c1[idx == s - 1] == 0).all(), (s, d)           # the clamp at the last source sample


def test_hand_worked_coefficient_where_the_precisions_differ(harness):
    """725 -> 362, output 71: (71 + 0.5) * 725 / 362 - 0.5 = 51837.5 / 362 - 0.5 = 142.697513812...; index 142.  A float32 in [128, 256)
    has 16 fraction bits: 0.697513812 * 65536 = 45712.27 -> the float32 nearest to the coordinate has the fraction f = 45712 / 65536
    (= 0.697509765625), and 142 is subtracted exactly.  f * 2048 = 45712 / 32 = 1428.5 exactly: half to even -> 1428;
    (1 - f) * 2048 = 19824 / 32 = 619.5 -> 620.  In double precision the fraction stays 0.697513812: 1428.508 -> 1429 and
    619.49 -> 619.  OpenCV's ``float fx`` gives the first."""
    (got,) = tables(harness, [(725, 362)])
    assert got[3 * 71:3 * 71 + 3].tolist() == [142, 620, 1428]
    idx, c0, c1 = ref.cv2_linear_coeffs(725, 362)
    assert (int(idx[71]), int(c0[71]), int(c1[71])) == (142, 620, 1428)
    # the two ends: output 0: 0.5 * 725 / 362 - 0.5 = 0.50138...: index 0, fraction 0.50138 -> round(1026.83) = 1027, 2048 - 1027 = 1021;
    # output 361: 361.5 * 725 / 362 - 0.5 = 723.4986...: index 723, fraction 0.4986 -> round(1021.17) = 1021, and 1027
    assert got[:3].tolist() == [0, 1021, 1027] and got[-3:].tolist() == [723, 1027, 1021]


def test_upscale_table_clamps_at_both_ends(harness):
    """64 -> 160 (scale 0.4): output 0: 0.5 * 0.4 - 0.5 = -0.3 -> floor -1 < 0: index 0, fraction 0 -> (0, 2048, 0); output 1: 0.1 ->
    (0, round(0.9 * 2048 = 1843.2) = 1843, round(204.8) = 205); output 159: 159.5 * 0.4 - 0.5 = 63.3 -> index 63 = the last sample: fraction 0
    -> (63, 2048, 0); output 158: 62.9 -> (62, round(0.1 * 2048) = 205, 1843)."""
    (got,) = tables(harness, [(64, 160)])
    assert got[:6].tolist() == [0, 2048, 0, 0, 1843, 205]
    assert got[-6:].tolist() == [62, 205, 1843, 63, 2048, 0]
    assert oracle_table(64, 160).tolist() == got.tolist()


# ---------------------------------------------------------------------------------------- the geometry
def geometry(exe, cases):
    """cases: (h, w, imgsz, auto) -> (rw, rh, top, left, net_h, net_w, mode, [(H, W)] * 3) each."""
    lines = ask(exe, "".join(f"geometry {h} {w} {S} 0 {int(au)}\n" for h, w, S, au in cases))
    assert len(lines) == len(cases)
    out = []
    for ln in lines:
        v = ln.split()
        assert v[0] == "geometry", ln
        v = [int(x) for x in v[1:]]
        out.append(tuple(v[:7]) + ([(v[7 + 2 * l], v[8 + 2 * l]) for l in range(3)],))
    return out


def oracle_geometry(h, w, S, auto):
    nw, nh, top, bottom, left, right = ref.letterbox_geometry(h, w, S, auto=bool(auto))
    mode = 0 if (w, h) == (nw, nh) else 1 if (w, h) == (2 * nw, 2 * nh) else 2       # the branches of cv2_resize_linear_u8
    return nw, nh, top, left, nh + top + bottom, nw + left + right, mode


@pytest.mark.parametrize("g", ROWS, ids=[g["name"] for g in ROWS])
def test_rows_by_hand_oracle_and_engine_agree(harness, g):
    (h, w), S = g["hw"], g["imgsz"]
    nw, nh, top, bottom, left, right = ref.letterbox_geometry(h, w, S, auto=g["auto"])
    assert (nw, nh) == g["resized"] and (top, bottom, left, right) == g["pads"] and (nh + top + bottom, nw + left + right) == g["net"]
    (got,) = geometry(harness, [(h, w, S, g["auto"])])
    assert got[:7] == (*g["resized"], g["pads"][0], g["pads"][2], *g["net"], g["mode"])
    assert got[7] == [(hh, ww) for hh, ww, _ in KA.levels_of(g["net"])]
    assert oracle_geometry(h, w, S, g["auto"])[6] == g["mode"]
    # scale_boxes / scale_coords: what they subtract and divide by, seen through a box / a point placed at the pad
    gain, (bx, by), (kx, ky) = g["gain"], g["box_pad"], g["kpt_pad"]
    assert abs(min(g["net"][0] / h, g["net"][1] / w) - gain) < 1e-12
    b = ref.scale_boxes(g["net"], torch.tensor([[bx, by, bx + 32.0, by + 64.0]]), (h, w))[0].numpy()
    assert b.tolist() == [0.0, 0.0, KA._q(32, gain), KA._q(64, gain)], b
    k = ref.scale_coords(g["net"], torch.tensor([[[kx + 32.0, ky + 64.0, 1.0]]]), (h, w))[0, 0].numpy()
    assert np.allclose(k[:2], [32 / gain, 64 / gain], rtol=0, atol=1e-4) and k[2] == 1.0, k
    assert (round(kx - 0.1), round(ky - 0.1)) == (bx, by)


def test_rows_cover_what_they_are_for():
    by = {g["name"].split(":")[0]: g for g in KA.GEOMETRY_ODD}
    assert len(by) == 10
    assert by["1"]["pads"][0] != by["1"]["pads"][1] and by["1"]["mode"] == 0                  # copy, top != bottom
    assert by["2"]["pads"][2] > 0 and by["2"]["net"][0] > by["2"]["net"][1]                   # left pad, portrait
    assert by["3"]["mode"] == 1 and by["3"]["pads"][0] != by["3"]["pads"][1]
    assert by["7"]["mode"] == 2 and by["7"]["gain"] == 0.5
    assert by["5"]["pads"][2] != by["5"]["pads"][3]
    for n in ("6", "8"):                                                                      # upscales
        assert by[n]["resized"][0] > by[n]["hw"][1] and by[n]["resized"][1] > by[n]["hw"][0]
    assert by["9"]["box_pad"][0] > by["9"]["kpt_pad"][0] and by["1"]["box_pad"][1] < by["1"]["kpt_pad"][1]


def test_geometry_sweep(harness):
    rng = np.random.default_rng(0)
    sizes = set()
    for S in (160, 320, 640):
        for a in list(range(S // 4, S + 3, 7)) + [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S]:
            for b in (S // 3 + 1, S // 2, S - 33, S - 1, S, S + 1, 2 * S - 2, 2 * S, 2 * S + 2):
                sizes.add((a, b, S))
                sizes.add((b, a, S))
        for _ in range(300):
            a, b = (int(x) for x in rng.integers(17, 4 * S, 2))
            sizes.add((a, b, S))
            sizes.add((b, a, S))
    cases = [(h, w, S, au) for h, w, S in sorted(sizes) for au in (0, 1)]
    got = geometry(harness, cases)
    modes = set()
    for c, g in zip(cases, got):
        want = oracle_geometry(*c)
        assert g[:7] == want, (c, g[:7], want)
        assert g[7] == [(want[4] >> (3 + l), want[5] >> (3 + l)) for l in range(3)], c
        modes.add((g[6], g[2] > 0, g[3] > 0))
    assert {m[0] for m in modes} == {0, 1, 2} and len(modes) >= 7, modes
    assert len(cases) > 4000


# ---------------------------------------------------------------------------------------- the rescale cases through the oracle
def _oracle_post(g, nc, kpt_shape, heads, conf):
    m = ref.YoloV8Ref({}, nc, kpt_shape)
    nk = kpt_shape[0] * kpt_shape[1] if kpt_shape else 0
    det = [torch.from_numpy(h[..., :64 + nc]).permute(0, 3, 1, 2).contiguous() for h in heads]
    kpt = [torch.from_numpy(h[..., 64 + nc:64 + nc + nk]).permute(0, 3, 1, 2).contiguous() for h in heads] if kpt_shape else []
    (d,) = ref.non_max_suppression(m.decode(det, kpt), conf, 0.7, None, 300, nc=nc)
    d = d.clone()
    d[:, :4] = ref.scale_boxes(g["net"], d[:, :4], g["hw"])
    k = ref.scale_coords(g["net"], d[:, 6:].view(len(d), *kpt_shape), g["hw"]).numpy() if kpt_shape else None
    return d[:, :6].numpy(), k


def _check_rows(got, want, tag):
    assert len(got) == len(want), f"{tag}: {len(got)} rows, expected {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[:4], np.asarray(w[:4], np.float32)), f"{tag} row {i}: box {g[:4]} != {w[:4]}"
        assert abs(float(g[4]) - w[4]) < 2e-7 and int(g[5]) == w[5], f"{tag} row {i}: score / class {g[4:6]} != {w[4:6]}"


def test_odd_detect_cases_through_the_oracle():
    nc, cases = KA.odd_detect_cases()
    assert [c[0] for c in cases] == [0, 1, 8, 7]
    for row, heads, want in cases:
        g = KA.GEOMETRY_ODD[row]
        boxes, _ = _oracle_post(g, nc, None, heads, 0.5)
        _check_rows(boxes, want, g["name"])


@pytest.mark.parametrize("kpt_shape", [(13, 3), (12, 2)], ids=["13x3", "12x2"])
def test_odd_pose_cases_through_the_oracle(kpt_shape):
    nc, cases = KA.odd_pose_cases(kpt_shape)
    for row, heads, want, ek in cases:
        g = KA.GEOMETRY_ODD[row]
        boxes, kpts = _oracle_post(g, nc, kpt_shape, heads, 0.25)
        _check_rows(boxes, want, g["name"])
        assert np.array_equal(kpts[0][:, :2], ek[:, :2].astype(np.float32)), (g["name"], kpts[0][:5], ek[:5])
        if kpt_shape[1] == 3:
            assert np.allclose(kpts[0][:, 2], ek[:, 2], atol=2e-7)


# ---------------------------------------------------------------------------------------- the random heads of the GPU test
@pytest.mark.parametrize("kind", ["detect", "pose"])
def test_random_heads_of_the_gpu_test_meet_their_conditions(kind):
    """tests/test_gpu_geometry.py::test_postprocess_matches_oracle_on_random_heads cannot pass empty: on the oracle's own output every
    image keeps at least 5 detections and every row has a coordinate clamped at 0 and one clamped at the frame edge (seeds chosen here)."""
    from tests import test_gpu_geometry as T
    for g in T.ROWS:
        nc, kpt, conf, heads = T.random_heads(g, kind, T.SEEDS[kind])
        assert [h.shape[1:3] for h in heads] == [(hh, ww) for hh, ww, _ in KA.levels_of(g["net"])]
        T.check_oracle_is_not_empty(g, T.oracle_post(g, nc, kpt, conf, heads))
