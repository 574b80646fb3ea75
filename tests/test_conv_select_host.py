"""csrc/conv_select.cpp on the CPU: the tile table, the resolver and the four choosers, through the stand-alone harness
tests/conv_select_main.cpp (g++ and the ROCm headers; no GPU, no engine library).

* resolver: for every (path, tile, case, w_single) of the forced-tile sweeps (tests/test_tile_coverage.py: SWEEPS) the resolved
  (family, tile) equals the hand-written table tests/tile_support.py — the comparison the GPU sweeps make per launch, here over
  the whole grid;
* shapes: ``conv_tile_shape`` equals ``tile_support.SHAPES`` for every id of every path, and knows no other id;
* auto choice: the chooser's tile for every conv of the shipped graphs equals tests/golden/conv_tile_choices.json, which was
  recorded from the choosers of the commit named in it (the harness linked against that commit's own conv objects).  A deliberate
  change of a chooser regenerates the file:  python -m tests.test_conv_select_host --record HARNESS --commit SHA
* the absorbed-upsample rule of the engine (attach in2, resolve, detach where nothing reads it) on the shapes of
  tests/test_gpu_h2.py::test_h2_upsample_absorbed."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import graph as G, yolo_arch
from tests import tile_support as TS

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "conv_tile_choices.json"
PATHS = ("h2", "bx3", "f16", "tap")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("conv_select") / "conv_select_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
                    str(ROOT / "tests" / "conv_select_main.cpp"), str(CSRC / "conv_select.cpp"), str(CSRC / "launch_plan.cpp"), "-o", str(exe)], check=True)
    return exe


def line(path, B, H, W, Ho, Wo, cin, cout, npad, k, s, ws, in_cs, up_c=0, requested=-1, copies=1):
    return f"{path} {B} {H} {W} {Ho} {Wo} {cin} {cout} {npad} {k} {s} {int(ws)} {copies} {in_cs} {up_c} {requested}"


def run(exe, lines):
    """-> [(chosen, resolved, family, bm, bn, copy, absorbed)] per input line ("-" columns of a parent-commit harness: None)."""
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[None if c == "-" else c for c in ln.split()] for ln in out if ln]
    assert len(rows) == len(lines)
    num = lambda c: None if c is None else int(c)
    return [(int(r[0]), num(r[1]), r[2], num(r[3]), num(r[4]), int(r[5]), num(r[6])) for r in rows]


def case_line(path, case, ws, tile, copies=1):
    B, H, W, cin, cout, k, s, act, res = case
    Ho, Wo = TS.out_hw(case)
    return line(path, B, H, W, Ho, Wo, cin, cout, G.pad16(cout), k, s, ws, cin, requested=tile, copies=copies)


# ---------------------------------------------------------------------------------------- resolver == tile_support.expected
@pytest.mark.parametrize("path", PATHS)
def test_resolver_matches_the_hand_written_table(harness, path):
    from tests.test_tile_coverage import SWEEPS
    tiles, runs = SWEEPS[path]
    grid = [(t, case, ws) for case, ws in runs for t in tiles]
    got = run(harness, [case_line(path, case, ws, t) for t, case, ws in grid])
    wrong = [(t, case, ws, (g[2], g[1]), TS.expected(path, t, case, ws)) for (t, case, ws), g in zip(grid, got)
             if (g[2], g[1]) != TS.expected(path, t, case, ws)]
    assert not wrong, f"{len(wrong)} of {len(grid)} cells; first (tile, case, w_single, resolver, table): {wrong[:5]}"
    # ... and before the engine has built its operand copies (ConvArgs::wr still null) no register-weights family is named
    got = run(harness, [case_line(path, case, ws, t, copies=0) for t, case, ws in grid])
    assert not [g for g in got if g[2] in ("h2r", "h2v", "h2s", "h2s3")]
    assert all(g[1] in TS.SHAPES[path] for g in got)


# ---------------------------------------------------------------------------------------- conv_tile_shape == tile_support.SHAPES
@pytest.mark.parametrize("path", PATHS)
def test_tile_shapes_match_the_hand_written_table(harness, path):
    ids = list(range(0, 1200))
    got = run(harness, [line(path, 1, 32, 32, 32, 32, 64, 96, 96, 3, 1, 1, 64, requested=i) for i in ids])
    for i, g in zip(ids, got):
        shape = TS.SHAPES[path].get(i)
        want = (0, 0) if shape is None else (shape[1], shape[2]) if shape[0] == "lin" else (shape[1] * shape[2], shape[3])
        assert (g[3], g[4]) == want, (path, i, g, shape)
        assert shape is not None or g[1] == -1, f"{path}: id {i} resolves to {g[1:3]} but is no tile of tile_support.SHAPES"


# ---------------------------------------------------------------------------------------- the engine's upsample-absorption rule
def test_absorbed_upsample_follows_the_resolved_kernel(harness):
    """Upsample(2) + cat in front of a stride-1 conv (tests/test_gpu_h2.py: test_h2_upsample_absorbed's shapes): the upsample is
    absorbed exactly where the kernel the tile resolves to reads the coarse map — the 1x1 tap tiles, the 3x3 patch kernel."""
    def ask(path, k, tile, ws=1, cin=96, up_c=64, H=24, W=40):
        return run(harness, [line(path, 2, H, W, H, W, cin, 48, 48, k, 1, ws, cin, up_c=up_c, requested=tile)])[0]
    for tile, want in ((303, (303, "h2p", 1)), (304, (304, "h2p", 1)), (313, (313, "h2p", 1)), (220, (220, "h2t", 0)),
                       (324, (303, "h2p", 1)), (325, (304, "h2p", 1)), (323, (303, "h2p", 1)), (246, (213, "h2t", 0))):
        g = ask("h2", 3, tile)
        assert (g[1], g[2], g[6]) == want, (tile, g)
    g = ask("h2", 3, -1)                       # the auto choice of this two-product layer is a quad tile: it lands on the patch kernel
    assert g[0] in (323, 324, 325) and (g[2], g[6]) == ("h2p", 1), g
    for tile, want in ((220, (220, "h2t")), (213, (213, "h2t")), (243, (243, "h2d")), (239, (239, "h2d")), (245, (243, "h2d")),
                       (247, (243, "h2d")), (303, (220, "h2t")), (343, (220, "h2t"))):
        g = ask("h2", 1, tile)
        assert (g[1], g[2], g[6]) == want + (1,), (tile, g)
    assert ask("h2", 3, 303, up_c=48)[6] == 0 and ask("h2", 3, 303, up_c=48)[2] == "h2p"       # not whole 32-channel chunks: the upsample runs
    assert ask("h2", 3, 303, H=25)[6] == 0 and ask("h2", 1, 220, H=25)[6] == 0               # odd map
    for tile, want in ((303, (303, "bx3p", 1)), (306, (306, "bx3p", 1)), (220, (220, "bx3t", 0)), (7, (7, "bx3t", 0))):
        g = ask("bx3", 3, tile)
        assert (g[1], g[2], g[6]) == want, (tile, g)
    for tile, want in ((209, 209), (9, 209), (304, 209), (213, 213), (13, 213), (14, 213), (306, 213), (206, 213), (6, 213),
                       (220, 220), (7, 220), (303, 220), (211, 220), (25, 220)):
        g = ask("bx3", 1, tile)
        assert (g[1], g[2], g[6]) == (want, "bx3t", 1), (tile, g)


# ---------------------------------------------------------------------------------------- auto choice == the recorded table
def _conv_layers(g):
    """[H, W, Ho, Wo, cin, cout, npad, k, stride, w_single, in_cs] of every conv op at network size 1 x 1 << level units."""
    return [(g.bufs[o["in_buf"]][0], g.bufs[o["out_buf"]][0], o["cin"], o["cout"], o["npad"], o["ksize"], o["stride"],
             1 if o.get("flags", 0) & G.FLAG_W_SINGLE else 0, g.bufs[o["in_buf"]][1]) for o in g.ops if o["kind"] == G.OP_CONV]


@functools.lru_cache(maxsize=None)
def shipped_models():
    """name -> (net_h, net_w, layers): the h2 graphs the package ships, over synthetic weights, at the network sizes of the
    benchmark's c2 / c3 workloads (1280 x 720 frames: letterbox to 384 x 640, the pose model's 1280 x 1280) and of the trackers."""
    from oracle import tracknet_ref as tr
    from tests import resnet_ref as R
    rng = np.random.default_rng(0)
    resnet_sd = {k: (np.abs(rng.normal(1, 0.1, s)) if k.endswith("running_var") else rng.normal(0, 0.05, s)).astype(np.float32)
                 for k, s in R.state_dict_shapes(G.RESNET_OUT).items()}
    graphs = {
        "yolov8n-detect": (384, 640, G.build_yolov8(yolo_arch.synth_state_dict("n", 1, None, seed=0), 1, None, dtype="h2")),
        "yolov8m-detect": (384, 640, G.build_yolov8(yolo_arch.synth_state_dict("m", 80, None, seed=0), 80, None, dtype="h2")),
        "yolov8m-pose13": (1280, 1280, G.build_yolov8(yolo_arch.synth_state_dict("m", 1, (13, 3), seed=0), 1, (13, 3), dtype="h2")),
        "yolo11n-detect": (384, 640, G.build_yolo11(yolo_arch.synth_state_dict11("n", 80, None, seed=0), 80, None, dtype="h2")),
        "yolo11n-pose13": (1280, 1280, G.build_yolo11(yolo_arch.synth_state_dict11("n", 1, (13, 3), seed=0), 1, (13, 3), dtype="h2")),
        "tracknet": (288, 512, G.build_tracknet(tr.synth_tracknet_state_dict(0), dtype="h2")),
        "resnet50": (G.RESNET_INPUT, G.RESNET_INPUT, G.build_resnet50(resnet_sd, dtype="h2")),
        "inpaintnet": (1, 16, G.build_inpaintnet(tr.synth_inpaintnet_state_dict(0), dtype="h2")),
    }
    return {name: (nh, nw, [[nh >> li, nw >> li, nh >> lo, nw >> lo] + list(rest) for li, lo, *rest in _conv_layers(g)])
            for name, (nh, nw, g) in graphs.items()}


def choices(exe, layers, batch):
    """[[h2, bx3, f16, tap, copy]] per layer: the four choosers over the same layers (the h2 one with each op's own w_single flag)."""
    rows = {p: run(exe, [line(p, batch, *ly[:9], ly[9] if p == "h2" else 0, ly[10]) for ly in layers]) for p in PATHS}
    return [[rows[p][i][0] for p in PATHS] + [rows["h2"][i][5]] for i in range(len(layers))]


def test_auto_choice_matches_the_recorded_table(harness):
    gold = json.loads(GOLDEN.read_text())
    assert gold["columns"] == list(PATHS) + ["copy"] and len(gold["recorded_from"]) >= 7
    models = shipped_models()
    assert sorted(gold["models"]) == sorted(models)
    n = 0
    for name, (nh, nw, layers) in models.items():
        rec = gold["models"][name]
        assert rec["net"] == [nh, nw] and rec["layers"] == layers, f"{name}: the graph's conv list changed — regenerate the golden file"
        for batch in (1, 64):
            got = choices(harness, layers, batch)
            want = rec[f"b{batch}"]
            diff = [(i, layers[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert len(got) == len(want) and not diff, f"{name} batch {batch}: (op, layer, got, recorded) {diff[:5]}"
            n += len(got)
    assert n > 700          # (every model contributes)
    flat = [c for rec in gold["models"].values() for b in ("b1", "b64") for c in rec[b]]
    assert {324, 325, 247, 248, 303, 213}.issubset({c[0] for c in flat}) and {0, 1} == {c[4] for c in flat}


def record(exe, commit):
    models = shipped_models()
    out = {"recorded_from": commit,
           "note": "auto tile choice of every conv of the shipped h2 graphs (synthetic weights), batch 1 and 64, from the four choosers "
                   "of the commit above: tests/conv_select_main.cpp linked against that commit's conv objects",
           "layer_columns": ["H", "W", "Ho", "Wo", "cin", "cout", "npad", "ksize", "stride", "w_single", "in_cs"],
           "columns": list(PATHS) + ["copy"], "models": {}}
    for name, (nh, nw, layers) in models.items():
        out["models"][name] = {"net": [nh, nw], "layers": layers, "b1": choices(exe, layers, 1), "b64": choices(exe, layers, 64)}
    body = ",\n".join(f'  {json.dumps(k)}: {{"net": {json.dumps(v["net"])},\n   "layers": {json.dumps(v["layers"])},\n   "b1": {json.dumps(v["b1"])},\n'
                      f'   "b64": {json.dumps(v["b64"])}}}' for k, v in out["models"].items())
    head = ",\n".join(f" {json.dumps(k)}: {json.dumps(out[k])}" for k in ("recorded_from", "note", "layer_columns", "columns"))
    GOLDEN.write_text("{" + head[1:] + ",\n \"models\": {\n" + body + "\n }}\n")
    json.loads(GOLDEN.read_text())


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="HARNESS", help="a built tests/conv_select_main.cpp")
    ap.add_argument("--commit", required=True, help="the commit whose choosers HARNESS was linked against")
    a = ap.parse_args()
    record(Path(a.record), a.commit)
    print(f"wrote {GOLDEN}", file=sys.stderr)
