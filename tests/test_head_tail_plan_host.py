"""find_head_tail and the tail's liveness rule (csrc/graph_plan.cpp) on the CPU, through tests/head_tail_plan_main.cpp.

* the matcher finds the tail of every h2 YOLOv8 / YOLO11 detect and pose graph (nc 1 / 80, keypoints (13, 3) / (17, 3)), with the
  ops an independent reading of the op list names: per level the box, class and keypoint 1x1 conv into the head buffer;
* it refuses: another dtype, TrackNet / InpaintNet / ResNet graphs, a one-conv graph that writes a head buffer, a tail conv with
  an activation, with a residual, with a wrong cout or out_choff, a 3x3 tail conv, a missing or doubled branch, a reader of a head
  map, an input that a later op overwrites;
* with the tail passed to plan_activations its inputs live to the end: they share no byte with a buffer that is touched at or after
  their first use (the head maps included), the arena does not grow on the bench's three models at the bench's shapes, and without
  the tail the plan is the old one (tests/test_graph_plan_host.py pins that one against its recorded answers)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import graph as G, yolo_arch
from tests.test_graph_plan_host import CSRC, ROOT, OP_FIELDS, ask, describe, describe_graph, live_ranges, Desc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    import os
    exe = tmp_path_factory.mktemp("head_tail_plan") / "head_tail_plan_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
                    str(ROOT / "tests" / "head_tail_plan_main.cpp"), str(CSRC / "graph_plan.cpp"), str(CSRC / "conv_select.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def tail_of(exe, text):
    w = ask(exe, text + "tail\n")[-1].split()
    assert w[0] == "tail"
    return None if w[1] == "0" else [[int(x) for x in w[2 + 3 * l:5 + 3 * l]] for l in range(3)]


def plan_of(exe, text, nh, nw, batch, alias, with_tail):
    w = ask(exe, text + f"plan {nh} {nw} {batch} {alias} {int(with_tail)}\n")[-1].split()
    assert w[0] == "plan", w
    return int(w[1]), int(w[2]), [tuple(int(x) for x in r.split(":")) for r in w[3:]]


YOLO = [("v8", "n", 1, None), ("v8", "n", 80, None), ("v8", "m", 1, None), ("v8", "m", 80, None), ("v8", "n", 1, (13, 3)), ("v8", "m", 1, (13, 3)),
        ("v8", "n", 1, (17, 3)), ("v8", "m", 1, (17, 3)), ("11", "n", 80, None), ("11", "m", 80, None), ("11", "n", 1, (13, 3)), ("11", "m", 1, (17, 3))]


def build(fam, scale, nc, kpt, dtype="h2"):
    if fam == "v8":
        return G.build_yolov8(yolo_arch.synth_state_dict(scale, nc, kpt, seed=0), nc, kpt, dtype=dtype)
    return G.build_yolo11(yolo_arch.synth_state_dict11(scale, nc, kpt, seed=0), nc, kpt, dtype=dtype)


def expected_tail(g):
    """The tail by an independent reading: per level the ops that write the head buffer, keyed by their channel offset."""
    nk = g.nk
    out = []
    for hb in g.head_buf:
        by_off = {int(o["out_choff"]): i for i, o in enumerate(g.ops) if o["out_buf"] == hb}
        out.append([by_off[0], by_off[64], by_off[64 + g.nc] if nk else -1])
    return out


@pytest.fixture(scope="module")
def graphs():
    return {case: build(*case) for case in YOLO}


@pytest.mark.parametrize("case", YOLO, ids=lambda c: f"yolo{c[0]}{c[1]}-nc{c[2]}-{'x'.join(map(str, c[3])) if c[3] else 'detect'}")
def test_tail_found_and_inputs_live_to_the_end(harness, graphs, case):
    g = graphs[case]
    text = describe_graph(g)
    tail = tail_of(harness, text)
    assert tail == expected_tail(g)
    for l in range(3):
        for c, i in enumerate(tail[l]):
            if i < 0:
                assert c == 2 and g.nk == 0
                continue
            o = g.ops[i]
            assert (o["kind"], o["ksize"], o["stride"], o["act"], o["res_buf"]) == (G.OP_CONV, 1, 1, G.ACT_NONE, -1)
            assert o["cout"] == (64, g.nc, g.nk)[c] and o["in_buf"] not in g.head_buf
    d = Desc(g)
    folds = []
    live = live_ranges(d, folds)            # (the folds only lengthen the life of an upsample's source: not a tail input)
    nops = len(g.ops)
    for alias in (1, 0):
        arena, logical, rows = plan_of(harness, text, 64, 64, 3, alias, True)
        arena0, logical0, rows0 = plan_of(harness, text, 64, 64, 3, alias, False)
        assert logical == logical0 and arena >= arena0 and [n for _, n in rows] == [n for _, n in rows0]
        if not alias:
            assert rows == rows0
        for l in range(3):
            for i in tail[l]:
                if i < 0:
                    continue
                b = g.ops[i]["in_buf"]
                ob, nb = rows[b]
                assert ob + nb <= arena
                for x in range(len(rows)):
                    if x == b or live[x] is None or live[x][1] < live[b][0]:
                        continue                     # dead before the input is first written
                    ox, nx = rows[x]
                    assert ob + nb <= ox or ox + nx <= ob, f"tail input {b} (op {i}, of {nops}) shares bytes with buffer {x} {live[x]}"


def test_arena_does_not_grow_on_the_bench_models(harness, graphs, capsys):
    """players (yolov8m, nc 80, 384 x 640 net), ball (yolov8n, nc 1, 384 x 640), pose (yolov8m 13 x 3, 1280 x 1280), batch 64."""
    for case, (nh, nw) in ((("v8", "m", 80, None), (384, 640)), (("v8", "n", 1, None), (384, 640)), (("v8", "m", 1, (13, 3)), (1280, 1280))):
        text = describe_graph(graphs[case])
        with_tail = plan_of(harness, text, nh, nw, 64, 1, True)[0]
        without = plan_of(harness, text, nh, nw, 64, 1, False)[0]
        with capsys.disabled():
            print(f"\narena bytes {case}: {without} without the tail rule, {with_tail} with it")
        assert with_tail == without


def test_other_graphs_have_no_tail(harness):
    from oracle import tracknet_ref as tr
    from tests.test_graph_plan_host import _resnet_sd
    for dt in ("f32", "f16"):
        assert tail_of(harness, describe_graph(build("v8", "n", 80, None, dt))) is None
    assert tail_of(harness, describe_graph(build("11", "n", 80, None, "f32"))) is None
    for g in (G.build_tracknet(tr.synth_tracknet_state_dict(0), dtype="h2"), G.build_inpaintnet(tr.synth_inpaintnet_state_dict(0), dtype="h2"),
              G.build_resnet50(_resnet_sd(), dtype="h2"), G.build_resnet50(_resnet_sd(), dtype="f32")):
        assert tail_of(harness, describe_graph(g)) is None


# ---------------------------------------------------------------------------------------- hand-made graphs: one field off
NF = 1 << 20


def conv(in_buf, out_buf, out_choff, cout, k=1, act=G.ACT_NONE, res_buf=-1, cin=32):
    return dict(kind=G.OP_CONV, in_buf=in_buf, in_choff=0, cin=cin, out_buf=out_buf, out_choff=out_choff, cout=cout, ksize=k, stride=1, act=act,
                res_buf=res_buf, res_choff=0, npad=(cout + 15) // 16 * 16, reserved=1 << 17, w_off=0, b_off=1 << 16, flags=0, pad_=0)


def small(nc=3, nk=6, dtype=G.DTYPE_H2):
    """Per level: a feature buffer (written by a 3x3 conv from buffer 0..2), one input buffer per branch, the head buffer."""
    cs = (64 + nc + nk + 3) // 4 * 4
    bufs, ops, heads = [], [], []
    for l in range(3):
        feat = len(bufs); bufs.append((3 + l, 32))
        ins = []
        for _ in range(3 if nk else 2):
            ins.append(len(bufs)); bufs.append((3 + l, 32))
            ops.append(conv(feat, ins[-1], 0, 32, k=3, act=G.ACT_SILU))
        hd = len(bufs); bufs.append((3 + l, cs))
        heads.append(hd)
        for b, (off, co) in zip(ins, ((0, 64), (64, nc), (64 + nc, nk))):
            ops.append(conv(b, hd, off, co))
    return dict(task=G.TASK_POSE if nk else G.TASK_DETECT, dtype=dtype, bufs=bufs, ops=ops, head_buf=heads, nc=nc, nk=nk, kpt_dim=3 if nk else 0,
                in_channels=0, n_floats=NF)


def text_of(g):
    return describe(g["task"], g["dtype"], g["bufs"], g["ops"], g["head_buf"], g["nc"], g["nk"], g["kpt_dim"], g["in_channels"], g["n_floats"])


def tail_ops(g, l=0):
    return [i for i, o in enumerate(g["ops"]) if o["out_buf"] == g["head_buf"][l]]


def test_small_graph_matches(harness):
    for nk in (6, 0):
        g = small(nk=nk)
        t = tail_of(harness, text_of(g))
        assert t == [tail_ops(g, l) + ([-1] if not nk else []) for l in range(3)]


REFUSALS = {
    "activation": lambda g: g["ops"][tail_ops(g)[1]].update(act=G.ACT_SILU),
    "residual": lambda g: g["ops"][tail_ops(g)[0]].update(res_buf=0),
    "3x3": lambda g: g["ops"][tail_ops(g)[2]].update(ksize=3),
    "box cout": lambda g: g["ops"][tail_ops(g)[0]].update(cout=48, npad=48),
    "class cout": lambda g: g["ops"][tail_ops(g)[1]].update(cout=2),
    "class out_choff": lambda g: g["ops"][tail_ops(g)[1]].update(out_choff=60),
    "keypoint out_choff": lambda g: g["ops"][tail_ops(g)[2]].update(out_choff=64 + g["nc"] + 1, cout=g["nk"] - 1),
    "keypoint cout": lambda g: g["ops"][tail_ops(g, 2)[2]].update(cout=g["nk"] - 3),
    "missing branch": lambda g: g["ops"].pop(tail_ops(g, 1)[2]),
    "doubled branch": lambda g: g["ops"].append(dict(g["ops"][tail_ops(g)[0]])),
    "extra writer": lambda g: g["ops"].append(dict(kind=G.OP_UPSAMPLE2X, in_buf=g["head_buf"][1] - 1, in_choff=0, cin=32, out_buf=g["head_buf"][0], out_choff=0,
                                                   cout=32, ksize=0, stride=0, act=0, res_buf=-1, res_choff=0, npad=0, reserved=0, w_off=0, b_off=0, flags=0, pad_=0)),
    "head map is read": lambda g: g["ops"].append(conv(g["head_buf"][0], 1, 0, 32, cin=32)),
    "head map as residual": lambda g: g["ops"].append(conv(0, 1, 0, 32, res_buf=g["head_buf"][2])),
    "input overwritten later": lambda g: g["ops"].append(conv(0, g["ops"][tail_ops(g)[0]]["in_buf"], 0, 32, k=3, act=G.ACT_SILU)),
    "reads a head buffer": lambda g: g["ops"][tail_ops(g, 1)[0]].update(in_buf=g["head_buf"][1]),
    "fp32 model": lambda g: g.update(dtype=G.DTYPE_F32),
    "fp16 model": lambda g: g.update(dtype=G.DTYPE_F16),
    "tracknet task": lambda g: g.update(task=G.TASK_TRACKNET),
    "one head buffer for two levels": lambda g: g["head_buf"].__setitem__(1, g["head_buf"][0]),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_small_graph_one_field_off_is_refused(harness, name):
    g = small()
    REFUSALS[name](g)
    assert tail_of(harness, text_of(g)) is None, name


def test_one_conv_into_a_head_buffer_is_refused(harness):
    """The conv unit tests' graphs: a detect-task h2 graph whose only op writes head buffer 0."""
    for cout, off in ((64, 0), (16, 0), (80, 64)):
        g = dict(task=G.TASK_DETECT, dtype=G.DTYPE_H2, bufs=[(3, 32), (3, 144), (4, 144), (5, 144)], ops=[conv(0, 1, off, cout)], head_buf=[1, 2, 3],
                 nc=80, nk=0, kpt_dim=0, in_channels=0, n_floats=NF)
        assert tail_of(harness, text_of(g)) is None
