"""stem_cv1_fusable (csrc/graph_plan.cpp) and what build_steps makes of it (csrc/launch_plan.cpp), on the CPU through
tests/stem_cv1_plan_main.cpp.

* the recogniser accepts model.0 + model.1 + model.2.cv1 of every h2 YOLOv8 detect / pose graph (n, s, m) and of hand-made graphs
  of the same form, and names nothing in fp32 / fp16 graphs, TrackNet and ResNet graphs;
* it refuses, one field off: a 3x3 or stride-2 conv behind layer 1, another activation on either conv, a residual, a three-product
  layer 1 or 1x1 (no PA_CONV_W_SINGLE), a 1x1 that reads a slice of layer 1's output or at another offset, a second reader of
  layer 1's buffer (as input, as residual), a second writer, layer 1 into a head buffer, the 1x1 writing back into layer 1's buffer;
* build_steps gives the stem's step both convs (has_cv1) and KEEPS the 1x1's own step, marked stem_cv1; with tuning
  fuse_stem_cv1 = 0, or with the weight-ring instantiations forced (tune bit 3), neither mark appears and the list is the same;
* the 1x1 behind the stem gets an operand-order weight copy at every width, cin = 32 included."""
import os
import subprocess

import pytest

from padel_analytics_amd import graph as G, yolo_arch
from tests.test_graph_plan_host import CSRC, ROOT, ask, describe, describe_graph

NF = 1 << 22


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stem_cv1_plan") / "stem_cv1_plan_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
                    str(ROOT / "tests" / "stem_cv1_plan_main.cpp"), str(CSRC / "graph_plan.cpp"), str(CSRC / "launch_plan.cpp"),
                    str(CSRC / "conv_select.cpp"), "-o", str(exe)], check=True)
    return exe


def fusable(exe, text):
    w = ask(exe, text + "fusable\n")[-1].split()
    assert w[0] == "fusable"
    return {int(w[i]): int(w[i + 1]) for i in range(1, len(w), 2)}


def steps(exe, text, nh, nw, n, cv1=1, tune=1):
    w = ask(exe, text + f"steps {nh} {nw} {n} {cv1} {tune}\n")[-1].split()
    assert w[0] == "steps", w
    return [tuple(int(x) for x in s.split(":")) for s in w[1:]]


def copies(exe, text):
    w = ask(exe, text + "copies\n")[-1].split()
    return {int(s.split(":")[0]): int(s.split(":")[1]) for s in w[1:]}


YOLO = [("n", 80, None), ("s", 80, None), ("m", 80, None), ("n", 1, (13, 3)), ("m", 1, (13, 3))]


@pytest.mark.parametrize("case", YOLO, ids=lambda c: f"yolov8{c[0]}-nc{c[1]}-{'pose' if c[2] else 'detect'}")
def test_yolov8_h2_graphs_are_recognised_and_planned(harness, case):
    scale, nc, kpt = case
    sd = yolo_arch.synth_state_dict(scale, nc, kpt, seed=0)
    g = G.build_yolov8(sd, nc, kpt, dtype="h2")
    o0, o1, o2 = g.ops[0], g.ops[1], g.ops[2]
    assert o0["kind"] == G.OP_STEM and (o1["ksize"], o1["stride"]) == (3, 2) and (o2["ksize"], o2["stride"], o2["cin"]) == (1, 1, o1["cout"])
    text = describe_graph(g)
    assert fusable(harness, text) == {0: 2}
    on = steps(harness, text, 64, 64, 2)
    assert on[0] == (0, 2, 1, 0), "the stem's step covers model.0 + model.1 and carries model.2.cv1"
    assert on[1] == (2, 1, 0, 1), "model.2.cv1 keeps its own step, marked"
    assert all(s[2:] == (0, 0) for s in on[2:])
    for kw in (dict(cv1=0), dict(tune=9)):
        off = steps(harness, text, 64, 64, 2, **kw)
        assert [s[:2] for s in off] == [s[:2] for s in on] and all(s[2:] == (0, 0) for s in off), kw
    cp = copies(harness, text)
    assert cp[2] >= (o2["npad"] // 16) * (o2["cin"] // 32) * 2048, "the 1x1 behind the stem has an operand-order copy"
    for dt in ("f32", "f16"):
        assert fusable(harness, describe_graph(G.build_yolov8(sd, nc, kpt, dtype=dt)))[0] < 2


def test_other_graphs_name_nothing(harness):
    from oracle import tracknet_ref as tr
    from tests.test_graph_plan_host import _resnet_sd
    for g in (G.build_tracknet(tr.synth_tracknet_state_dict(0), dtype="h2"), G.build_resnet50(_resnet_sd(), dtype="h2")):
        assert 2 not in fusable(harness, describe_graph(g)).values()


# ---------------------------------------------------------------------------------------- hand-made graphs: one field off
def op(kind, in_buf, cin, out_buf, cout, k, s, act=G.ACT_SILU, flags=G.FLAG_W_SINGLE, **kw):
    o = dict(kind=kind, in_buf=in_buf, in_choff=0, cin=cin, out_buf=out_buf, out_choff=0, cout=cout, ksize=k, stride=s, act=act, res_buf=-1,
             res_choff=0, npad=(cout + 15) // 16 * 16, reserved=1 << 17, w_off=0, b_off=1 << 16, flags=flags, pad_=0)
    o.update(kw)
    return o


def small(c=32, dtype=G.DTYPE_H2):
    """buffers: 0 stem map, 1 layer-1 map, 2 the 1x1's output (wider: a concatenation buffer), 3 a level-3 feature map, 4..6 heads."""
    bufs = [(1, c), (2, 2 * c), (2, 3 * c), (3, 64), (3, 80), (4, 80), (5, 80)]
    ops = [op(G.OP_STEM, 0, 3, 0, c, 3, 2, flags=0, w_off=1 << 10, b_off=1 << 11, reserved=0),
           op(G.OP_CONV, 0, c, 1, 2 * c, 3, 2),
           op(G.OP_CONV, 1, 2 * c, 2, 2 * c, 1, 1, out_choff=16),
           op(G.OP_CONV, 2, 3 * c, 3, 64, 3, 2)]
    return dict(task=G.TASK_DETECT, dtype=dtype, bufs=bufs, ops=ops, head_buf=[4, 5, 6], nc=16, nk=0, kpt_dim=0, in_channels=0, n_floats=NF)


def text_of(g):
    return describe(g["task"], g["dtype"], g["bufs"], g["ops"], g["head_buf"], g["nc"], g["nk"], g["kpt_dim"], g["in_channels"], g["n_floats"])


@pytest.mark.parametrize("c", [16, 32, 48])
def test_small_graph_is_recognised(harness, c):
    g = small(c)
    assert fusable(harness, text_of(g)) == {0: 2}
    st = steps(harness, text_of(g), 64, 96, 2)
    assert st[:2] == [(0, 2, 1, 0), (2, 1, 0, 1)]
    assert 2 in copies(harness, text_of(g))


REFUSALS = {
    "3x3 behind layer 1": lambda g: g["ops"][2].update(ksize=3),
    "stride 2 behind layer 1": lambda g: g["ops"][2].update(stride=2),
    "1x1 without SiLU": lambda g: g["ops"][2].update(act=G.ACT_NONE),
    "1x1 with ReLU": lambda g: g["ops"][2].update(act=G.ACT_RELU),
    "layer 1 without SiLU": lambda g: g["ops"][1].update(act=G.ACT_NONE),
    "1x1 with a residual": lambda g: g["ops"][2].update(res_buf=3),
    "three-product 1x1": lambda g: g["ops"][2].update(flags=0),
    "three-product layer 1": lambda g: g["ops"][1].update(flags=0),
    "1x1 reads half of layer 1": lambda g: g["ops"][2].update(cin=g["ops"][1]["cout"] // 2),
    "1x1 reads at an offset": lambda g: (g["bufs"].__setitem__(1, (2, 2 * g["ops"][1]["cout"])), g["ops"][2].update(in_choff=16)),
    "1x1 reads another buffer": lambda g: g["ops"][2].update(in_buf=2, out_buf=1),
    "second reader of layer 1": lambda g: g["ops"].append(op(G.OP_CONV, 1, g["ops"][1]["cout"], 3, 64, 3, 2)),
    "layer 1 as a residual": lambda g: g["ops"].append(op(G.OP_CONV, 2, 32, 2, g["ops"][1]["cout"], 1, 1, res_buf=1)),
    "second writer of layer 1": lambda g: g["ops"].append(op(G.OP_CONV, 2, 32, 1, 32, 1, 1)),
    "an upsample reads layer 1": lambda g: g["ops"].append(dict(op(G.OP_UPSAMPLE2X, 1, 32, 0, 32, 0, 0, act=0, flags=0), npad=0, reserved=0, b_off=0)),
    "layer 1 into a head buffer": lambda g: (g["bufs"].__setitem__(4, (2, g["ops"][1]["cout"])), g["ops"][1].update(out_buf=4), g["ops"][2].update(in_buf=4)),
    "1x1 writes layer 1's buffer": lambda g: g["ops"][2].update(out_buf=1, out_choff=0),
    "stem read twice": lambda g: g["ops"].append(op(G.OP_CONV, 0, g["ops"][0]["cout"], 3, 64, 3, 2)),
    "fp32 graph": lambda g: g.update(dtype=G.DTYPE_F32),
    "fp16 graph": lambda g: g.update(dtype=G.DTYPE_F16),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_small_graph_one_field_off_is_refused(harness, name):
    g = small()
    REFUSALS[name](g)
    assert fusable(harness, text_of(g))[0] < 2, name
