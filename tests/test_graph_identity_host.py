"""What every graph builder emits, pinned byte for byte: buffer table, op list (every ``pa_op_desc`` field), scalars and
the packed weight blob of each builder x storage type, as SHA-256 digests in ``tests/golden/graph_digests.json``.

The device only ever sees these bytes, so a change to graph.py that keeps the digests leaves results and speed where they
were.  The state dicts take names and shapes from the specs / synthesizers and their VALUES from an integer counter formula
(no RNG stream, no torch, no threads): multiples of 1/4096 in [-1/4, 1/4), which are fp16 numbers (``grid``: h2 graphs keep
them unfolded, PA_CONV_W_SINGLE), or the same times 1 + 2^-20 in fp32 (``offgrid``: folded).  Between the formula and the
blob lie only correctly rounded elementwise fp32 operations, so the digests do not depend on the host.

``PADEL_RECORD_GRAPH_DIGESTS=1 pytest tests/test_graph_identity_host.py`` rewrites the fixture instead of comparing — to be
run on the commit whose output is the reference, never to make a failing comparison pass."""
import hashlib
import json
import os
import zlib
from pathlib import Path

import numpy as np
import pytest

from oracle import tracknet_ref
from padel_analytics_amd import graph as G, yolo_arch

FIXTURE = Path(__file__).parent / "golden" / "graph_digests.json"
RECORD = os.environ.get("PADEL_RECORD_GRAPH_DIGESTS") == "1"

# the integer fields of pa_op_desc (include/padel_hip.h) in declaration order; `pad_` is the struct's padding
OP_FIELDS = ("kind", "in_buf", "in_choff", "cin", "out_buf", "out_choff", "cout", "ksize", "stride", "act", "res_buf",
             "res_choff", "npad", "reserved", "w_off", "b_off", "flags")


def fill(shapes: dict, offgrid: bool) -> dict:
    """name -> fp32 array of that shape from the counter formula (``num_batches_tracked``: int64 zero)."""
    sd = {}
    for name, shp in shapes.items():
        if name.endswith("num_batches_tracked"):
            sd[name] = np.array(0, np.int64)
            continue
        i = np.arange(int(np.prod(shp, dtype=np.int64)), dtype=np.int64)
        v = (((i * 2654435761 + zlib.crc32(name.encode())) % 2048 - 1024).astype(np.float32) / np.float32(4096)).reshape(shp)
        if offgrid:
            v = v * np.float32(1 + 2.0 ** -20)
        if name.endswith("running_var"):
            v = np.float32(0.5) + np.abs(v)           # strictly positive
        elif name.endswith(".weight") and len(shp) == 1:      # BatchNorm's gamma (every other weight has 2 - 4 axes)
            v = np.float32(1) + v
        sd[name] = v.astype(np.float32)
    return sd


def shapes_of(sd) -> dict:
    return {k: tuple(np.shape(v)) for k, v in sd.items()}


def _yolov8(scale, nc, kpt, dtype, offgrid):
    return G.build_yolov8(fill(yolo_arch.yolov8_state_spec(scale, nc, kpt), offgrid), nc, kpt, dtype)


def _yolo11(scale, nc, kpt, dtype, offgrid):
    return G.build_yolo11(fill(yolo_arch.yolo11_state_spec(scale, nc, kpt), offgrid), nc, kpt, dtype)


def _tracknet(dtype):
    return G.build_tracknet(fill(shapes_of(tracknet_ref.synth_tracknet_state_dict()), True), dtype)


def _inpaintnet(dtype):
    return G.build_inpaintnet(fill(shapes_of(tracknet_ref.synth_inpaintnet_state_dict()), True), dtype)


def _resnet50(dtype):
    return G.build_resnet50(fill(G.resnet50_shapes(), True), dtype)


POSE = (13, 3)
# case name -> (builder, arguments, {graph module attribute: forced value})
CASES = {}
for _dt in ("f32", "f16", "h2"):
    CASES[f"yolov8-n-detect-{_dt}-grid"] = (_yolov8, ("n", 80, None, _dt, False), {})
    CASES[f"yolov8-s-pose-{_dt}-grid"] = (_yolov8, ("s", 1, POSE, _dt, False), {})
    CASES[f"tracknet-{_dt}-offgrid"] = (_tracknet, (_dt,), {})
CASES["yolov8-n-detect-h2-offgrid"] = (_yolov8, ("n", 80, None, "h2", True), {})
CASES["yolov8-n-detect-h2-grid-folded"] = (_yolov8, ("n", 80, None, "h2", False), {"UNFOLDED_BN": False})
CASES["yolov8-m-pose-h2-grid"] = (_yolov8, ("m", 1, POSE, "h2", False), {})
CASES["yolov8-m-pose-h2-grid-merged"] = (_yolov8, ("m", 1, POSE, "h2", False), {"HEAD_SPLIT": False})
CASES["yolov8-m-pose-h2-grid-split"] = (_yolov8, ("m", 1, POSE, "h2", False), {"HEAD_SPLIT": True})
for _name, _args in (("n-detect", ("n", 80, None)), ("s-pose", ("s", 1, POSE))):
    CASES[f"yolo11-{_name}-f32-grid"] = (_yolo11, _args + ("f32", False), {})
    CASES[f"yolo11-{_name}-h2-grid"] = (_yolo11, _args + ("h2", False), {})
    CASES[f"yolo11-{_name}-h2-offgrid"] = (_yolo11, _args + ("h2", True), {})
for _dt in ("f32", "h2"):
    CASES[f"inpaintnet-{_dt}-offgrid"] = (_inpaintnet, (_dt,), {})
    CASES[f"resnet50-{_dt}-offgrid"] = (_resnet50, (_dt,), {})


def digests(g: G.Graph) -> dict:
    for o in g.ops:
        assert set(o) <= set(OP_FIELDS) | {"pad_"}, sorted(set(o) - set(OP_FIELDS))
    head = (int(g.task), int(g.nc), int(g.nk), int(g.kpt_dim), [(int(l), int(c)) for l, c in g.bufs],
            tuple(int(b) for b in g.head_buf), int(g.in_channels), int(g.out_channels), int(g.dtype), int(g.n_floats))
    layout = hashlib.sha256(repr(head).encode())
    for o in g.ops:
        layout.update(repr(tuple(int(o.get(k, 0)) for k in OP_FIELDS)).encode())
    blob = g.blob()
    assert blob.dtype == np.float32 and blob.size == g.n_floats
    return {"layout": layout.hexdigest(), "blob": hashlib.sha256(blob.tobytes()).hexdigest()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_graph_bytes_are_the_recorded_ones(case, monkeypatch):
    build, args, forced = CASES[case]
    for attr, value in forced.items():
        monkeypatch.setattr(G, attr, value)
    have = digests(build(*args))
    if RECORD:
        recorded = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {}
        recorded[case] = have
        FIXTURE.write_text(json.dumps(recorded, indent=1, sort_keys=True) + "\n")
        return
    want = json.loads(FIXTURE.read_text())[case]
    wrong = [k for k in ("layout", "blob") if have[k] != want[k]]
    assert not wrong, f"{case}: {' and '.join(wrong)} differ from the recorded graph"


def test_fills_take_the_paths_they_are_meant_to():
    """``grid`` conv weights are fp16 numbers (the h2 graph keeps them unfolded: every BN'd conv is PA_CONV_W_SINGLE with
    its own output scale), ``offgrid`` ones are not (folded, no conv is single); BatchNorm's variance is positive."""
    spec = yolo_arch.yolov8_state_spec("n", 80, None)
    grid, off = fill(spec, False), fill(spec, True)
    convs = [k for k in spec if k.endswith("conv.weight") and "dfl" not in k]
    assert all(G.fp16_exact(grid[k]) for k in convs) and not any(G.fp16_exact(off[k]) for k in convs)
    assert all(float(v.min()) > 0 for k, v in grid.items() if k.endswith("running_var"))
    single = lambda g: [bool(o["flags"] & G.FLAG_W_SINGLE) for o in g.ops if o["kind"] == G.OP_CONV]
    assert all(single(G.build_yolov8(grid, 80, None, "h2"))) and not any(single(G.build_yolov8(off, 80, None, "h2")))
