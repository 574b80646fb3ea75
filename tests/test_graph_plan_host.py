"""csrc/graph_plan.cpp on the CPU: what the engine decides about a graph before anything runs, through the stand-alone harness
tests/graph_plan_main.cpp (g++ against graph_plan.cpp and conv_select.cpp; no GPU, no engine library).

* same answers as the commit the file was split out of: validation, upsample folds, ``stem_fusable``, the activation plan
  (arena / logical bytes and a SHA-256 of the ``offset:bytes`` row, batch 2 at a 64 x 64 network input — 32 x 64 for TrackNet-task
  graphs — with alias 1 and 0), the letterbox geometry and the ``cv2_linear_table`` rows equal tests/golden/graph_plan.json, which
  was recorded from the code of the commit named in it: the harness compiled with -DGRAPH_PLAN_PARENT at the end of a scratch
  translation unit that includes that commit's csrc/engine.cpp, stubs hipMalloc / hipFree / hipMemsetAsync / hipMemcpyAsync /
  hipStreamSynchronize with malloc / free / memset / memcpy / nothing, and adapts that commit's static functions to graph_plan.h's
  signatures (offsets read back as ``bptr[i] - arena``, bytes as the distance between neighbours of its alias-0 plan); built with
  the ROCm clang++ (-D__HIP_PLATFORM_AMD__, the ROCm include directory, that commit's conv_select.cpp,
  -Wl,--unresolved-symbols=ignore-all).  A deliberate change of one of these decisions regenerates the file:
      python -m tests.test_graph_plan_host --record HARNESS --commit SHA
* the plan is sound: a second implementation of the liveness rules, here in Python from the op list alone, and the assertion that
  no two buffers that are live together share a byte;
* every refusal of ``validate_desc`` is reachable and fires first: a valid small graph, one field changed, the message;
* ``pil_coeffs`` equals ``pa_pil_coeffs`` of the built library (which needs no GPU).

The graphs: build_yolov8 for the scales n, s, m, l, x, detect (nc 80) and pose (nc 1, 13 x 3 keypoints), f32 / f16 / h2;
build_yolo11 the same in f32 and h2 (its depthwise conv and attention have no fp16 form: the builder refuses);
build_tracknet, build_inpaintnet and build_resnet50 in f32 and h2 — over the synthetic state dicts of the other host tests."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import graph as G, yolo_arch

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "graph_plan.json"
OP_FIELDS = ("kind", "in_buf", "in_choff", "cin", "out_buf", "out_choff", "cout", "ksize", "stride", "act", "res_buf", "res_choff", "npad",
             "reserved", "w_off", "b_off", "flags", "pad_")          # pa_op_desc in struct order
DTYPES = {"f32": G.DTYPE_F32, "f16": G.DTYPE_F16, "h2": G.DTYPE_H2}
SLACK = 512                                                          # kConvReadSlack (csrc/kernels.h)
BATCH = 2
SOURCES = ((720, 1280), (1080, 1920), (480, 854), (640, 640))
CV2_TABLES = ((1280, 640), (854, 640))
PIL_SIZES = ((1280, 640), (720, 640), (1920, 224), (1080, 224), (1280, 512), (720, 288), (100, 224))


def build_harness(exe, extra=()):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", *extra, "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
                    str(ROOT / "tests" / "graph_plan_main.cpp"), str(CSRC / "graph_plan.cpp"), str(CSRC / "conv_select.cpp"), "-o", str(exe)],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("graph_plan") / "graph_plan_main")


def ask(exe, text):
    """-> the answer lines of the commands in ``text``."""
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return [ln for ln in out if ln]


# ---------------------------------------------------------------------------------------- descriptions
def describe(task, dtype, bufs, ops, head_buf=(-1, -1, -1), nc=0, nk=0, kpt_dim=0, in_channels=0, n_floats=0):
    hb = list(head_buf) + [-1] * (3 - len(head_buf))
    lines = [f"graph {len(bufs)} {len(ops)}", f"{task} {dtype} {nc} {nk} {kpt_dim} {hb[0]} {hb[1]} {hb[2]} {in_channels} {n_floats}"]
    lines += [f"{l} {c}" for l, c in bufs]
    lines += [" ".join(str(int(o.get(f, 0))) for f in OP_FIELDS) for o in ops]
    return "\n".join(lines) + "\n"


def describe_graph(g):
    return describe(g.task, g.dtype, g.bufs, g.ops, g.head_buf, g.nc, g.nk, g.kpt_dim, g.in_channels, g.n_floats)


def net_size(g):
    return (32, 64) if g.task == G.TASK_TRACKNET else (64, 64)


def _resnet_sd():
    from tests import resnet_ref as R
    rng = np.random.default_rng(0)
    return {k: (np.abs(rng.normal(1, 0.1, s)) if k.endswith("running_var") else rng.normal(0, 0.05, s)).astype(np.float32)
            for k, s in R.state_dict_shapes(G.RESNET_OUT).items()}


class Desc:
    """What the tests need of a built graph (the weights are dropped: 66 graphs, the largest of 70 M parameters)."""
    def __init__(self, g):
        self.task, self.dtype, self.bufs, self.head_buf = g.task, g.dtype, list(g.bufs), tuple(g.head_buf)
        self.ops = [{f: int(o.get(f, 0)) for f in OP_FIELDS} for o in g.ops]
        self.text = describe_graph(g)
        self.net = net_size(g)


def build_descs():
    """name -> Desc of every graph of the module docstring (a state dict is made once, shared by its dtypes, then dropped)."""
    from oracle import tracknet_ref as tr
    out = {}
    fams = (("yolov8", G.build_yolov8, yolo_arch.synth_state_dict, yolo_arch.SCALES, ("f32", "f16", "h2")),
            ("yolo11", G.build_yolo11, yolo_arch.synth_state_dict11, yolo_arch.SCALES11, ("f32", "h2")))
    for fam, build, synth, scales, dts in fams:
        for scale in scales:
            for head, nc, kpt in (("detect", 80, None), ("pose", 1, (13, 3))):
                sd = synth(scale, nc, kpt, seed=0)
                for dt in dts:
                    out[f"{fam}{scale}-{head}-{dt}"] = Desc(build(sd, nc, kpt, dtype=dt))
    for name, build, sd in (("tracknet", G.build_tracknet, tr.synth_tracknet_state_dict(0)),
                            ("inpaintnet", G.build_inpaintnet, tr.synth_inpaintnet_state_dict(0)), ("resnet50", G.build_resnet50, _resnet_sd())):
        for dt in ("f32", "h2"):
            out[f"{name}-{dt}"] = Desc(build(sd, dtype=dt))
    return out


def answers(exe, descs):
    """name -> {"validate", "folds", "stem", "plan": {alias: (arena, logical, [(off, bytes)])}} from ONE run of the harness."""
    text = ""
    for d in descs.values():
        nh, nw = d.net
        text += d.text + f"validate\nfolds\nstem\nplan {nh} {nw} {BATCH} 1\nplan {nh} {nw} {BATCH} 0\n"
    lines = ask(exe, text)
    assert len(lines) == 5 * len(descs), lines[:3]
    out = {}
    for i, name in enumerate(descs):
        v, f, s, p1, p0 = lines[5 * i:5 * i + 5]
        assert f.split()[0] == "folds" and s.split()[0] == "stem", (f, s)
        plans = {}
        for alias, p in ((1, p1), (0, p0)):
            w = p.split()
            assert w[0] == "plan", p
            plans[alias] = (int(w[1]), int(w[2]), [tuple(int(x) for x in r.split(":")) for r in w[3:]], " ".join(w[3:]))
        out[name] = {"validate": v, "folds": [[int(x) for x in r.split(":")] for r in f.split()[1:]], "stem": [int(x) for x in s.split()[1:]],
                     "plan": plans}
    return out


def general_answers(exe):
    """Letterbox geometry + head levels, cv2 tables: what does not depend on a graph."""
    cmds = [f"geometry {h} {w} 640 0 {au}" for h, w in SOURCES for au in (0, 1)] + [f"cv2 {s} {d}" for s, d in CV2_TABLES]
    lines = ask(exe, "\n".join(cmds) + "\n")
    assert len(lines) == len(cmds)
    return {c: [int(x) for x in ln.split()[1:]] for c, ln in zip(cmds, lines)}


@pytest.fixture(scope="module")
def descs():
    return build_descs()


@pytest.fixture(scope="module")
def got(harness, descs):
    return answers(harness, descs)


def golden_record(ans):
    return {"validate": ans["validate"], "folds": ans["folds"], "stem": ans["stem"],
            "plan": {f"alias{a}": {"arena": p[0], "logical": p[1], "sha256": hashlib.sha256(p[3].encode()).hexdigest()} for a, p in ans["plan"].items()}}


# ---------------------------------------------------------------------------------------- a. the parent commit's answers
def test_same_answers_as_the_recorded_commit(harness, descs, got):
    gold = json.loads(GOLDEN.read_text())
    assert len(gold["recorded_from"]) >= 7
    assert sorted(gold["graphs"]) == sorted(descs)
    for name in descs:
        assert golden_record(got[name]) == gold["graphs"][name], name
    assert all(g["validate"] == "ok" for g in gold["graphs"].values())
    assert any(g["folds"] for g in gold["graphs"].values()) and any(g["stem"] for g in gold["graphs"].values())
    assert general_answers(harness) == gold["general"]


# ---------------------------------------------------------------------------------------- b. the plan, checked independently
def live_ranges(d, folds):
    """(first, last) op index per buffer by the rules above plan_activations (csrc/graph_plan.cpp), from the op list alone: live
    from the first op that touches a buffer to the last; the source of an absorbed upsample until the absorbing conv; buffer 0 of
    a TrackNet-task graph from before op 0; head buffers past the end; fp16 head buffers throughout.  None: never touched."""
    nb, nops = len(d.bufs), len(d.ops)
    rng = [None] * nb

    def touch(b, i):
        if 0 <= b < nb:
            rng[b] = (i, i) if rng[b] is None else (min(rng[b][0], i), max(rng[b][1], i))
    absorbs = {conv: up for up, conv in folds}
    for i, o in enumerate(d.ops):
        if o["kind"] not in (G.OP_STEM, G.OP_STEM7):
            touch(o["in_buf"], i)
        touch(o["out_buf"], i)
        if o["kind"] in (G.OP_CONV, G.OP_DWCONV3) and o["res_buf"] >= 0:
            touch(o["res_buf"], i)
        if i in absorbs:
            touch(d.ops[absorbs[i]]["in_buf"], i)
    if d.task == G.TASK_TRACKNET:
        touch(0, -1)
    for hb in d.head_buf:
        touch(hb, nops + 1)
        if d.dtype == G.DTYPE_F16:
            touch(hb, -1)
    return rng


def test_plan_is_sound(descs, got):
    checked = 0
    for name, d in descs.items():
        nh, nw = d.net
        live = live_ranges(d, got[name]["folds"])
        for alias in (1, 0):
            arena, logical, rows, _ = got[name]["plan"][alias]
            assert len(rows) == len(d.bufs)
            for b, ((off, nbytes), (level, ch)) in enumerate(zip(rows, d.bufs)):
                es = 2 if d.dtype == G.DTYPE_F16 and b not in d.head_buf else 4
                assert nbytes % 256 == 0 and nbytes >= BATCH * (nh >> level) * (nw >> level) * ch * es + SLACK, (name, alias, b)
                if live[b] is not None or not alias:
                    assert off + nbytes <= arena, (name, alias, b)
            assert sum(n for _, n in rows) == logical, (name, alias)
            if alias:
                assert arena <= logical, name
            else:
                assert arena == logical and all(rows[i][0] + rows[i][1] == rows[i + 1][0] for i in range(len(rows) - 1)) and rows[0][0] == 0, name
            used = [b for b in range(len(rows)) if live[b] is not None]
            for i, a in enumerate(used):
                for b in used[i + 1:]:
                    together = live[a][0] <= live[b][1] and live[b][0] <= live[a][1]
                    if together or not alias:
                        (oa, na), (ob, nb_) = rows[a], rows[b]
                        assert oa + na <= ob or ob + nb_ <= oa, f"{name} alias {alias}: buffers {a} {live[a]} and {b} {live[b]} share bytes"
                        checked += together
        assert got[name]["plan"][1][0] < got[name]["plan"][1][1] or len(d.bufs) < 4, f"{name}: aliasing saves nothing"
    assert checked > 10000


# ---------------------------------------------------------------------------------------- c. every refusal
NF = 1 << 20                         # floats of the pretend weight blob
W_OFF, B_OFF, R_OFF = 0, 1 << 16, 1 << 17


def op(kind, in_buf=0, in_choff=0, cin=32, out_buf=1, out_choff=0, cout=32, ksize=0, stride=0, act=0, res_buf=-1, res_choff=0, npad=0,
       reserved=0, w_off=W_OFF, b_off=B_OFF, flags=0):
    return dict(kind=kind, in_buf=in_buf, in_choff=in_choff, cin=cin, out_buf=out_buf, out_choff=out_choff, cout=cout, ksize=ksize, stride=stride,
                act=act, res_buf=res_buf, res_choff=res_choff, npad=npad, reserved=reserved, w_off=w_off, b_off=b_off, flags=flags, pad_=0)


def conv(in_buf, out_buf, k=3, s=1):
    return op(G.OP_CONV, in_buf=in_buf, out_buf=out_buf, ksize=k, stride=s, act=G.ACT_SILU, npad=32, reserved=R_OFF)


def small(dtype="f32", extra_bufs=(), extra_ops=(), **desc):
    """Two 3x3 convs (stride 1, stride 2) over 32-channel buffers at levels 0, 0, 1, then the ops of the case."""
    g = dict(task=G.TASK_TRACKNET, dtype=DTYPES[dtype], bufs=[(0, 32), (0, 32), (1, 32)] + list(extra_bufs),
             ops=[conv(0, 1), conv(1, 2, s=2)] + [dict(o) for o in extra_ops], head_buf=[-1, -1, -1], nc=0, nk=0, kpt_dim=0, in_channels=32, n_floats=NF)
    g.update(desc)
    return g


def set_op(i, **fields):
    return lambda g: g["ops"][i].update(fields)


def set_buf(i, level, channels):
    return lambda g: g["bufs"].__setitem__(i, (level, channels))


def set_desc(**fields):
    return lambda g: g.update({k: (DTYPES[v] if k == "dtype" else v) for k, v in fields.items()})


def both(*fs):
    return lambda g: [f(g) for f in fs]


STEM = op(G.OP_STEM, out_buf=2, cin=3, ksize=3, stride=2, act=G.ACT_SILU)
SPPF = op(G.OP_SPPF_POOL, in_buf=3, out_buf=3, out_choff=32, ksize=5, stride=1)
UPSAMPLE = op(G.OP_UPSAMPLE2X, in_buf=2, out_buf=1)
MAXPOOL = op(G.OP_MAXPOOL2, in_buf=1, out_buf=2)
MAXPOOL3 = op(G.OP_MAXPOOL3S2, in_buf=1, out_buf=2, ksize=3, stride=2)
STEM7 = op(G.OP_STEM7, out_buf=3, cin=3, cout=64, ksize=7, stride=2, act=G.ACT_RELU, npad=64, reserved=R_OFF)
GAP_FC = op(G.OP_GAP_FC, in_buf=2, out_buf=2, cout=8, act=G.ACT_SIGMOID)
DWCONV = op(G.OP_DWCONV3, in_buf=1, out_buf=0, ksize=3, stride=1, npad=32)
PSA = op(G.OP_PSA_ATTN, in_buf=3, out_buf=4, cin=128, cout=64, ksize=32, stride=1, npad=64)
PSA_BUFS = ((1, 128), (1, 64))
HEADS = dict(extra_bufs=((3, 104), (4, 104), (5, 104)), head_buf=[3, 4, 5])

# (id, the valid graph, the one change, a distinctive part of the message): one per refusal of validate_desc, in its order
REFUSALS = [
    ("empty", small(), lambda g: g.update(ops=[]), "model desc: empty graph"),
    ("dtype", small(), lambda g: g.update(dtype=7), "model desc: dtype 7"),
    ("buffer", small(), set_buf(2, 7, 32), "model desc: buffer 2 (level 7, channels 32)"),
    ("h2-buffer", small("h2"), set_buf(0, 0, 40), "model desc: h2 buffer 0 has 40 channels"),
    ("output-slice", small(), set_op(0, out_choff=16), "op 0: bad output slice"),
    ("f16-pool-width", small("f16", extra_ops=[MAXPOOL]), set_buf(2, 1, 36), "op 2: fp16 pool / upsample buffers must be a multiple of 8 channels wide"),
    ("h2-group", small("h2"), set_op(0, in_choff=8), "op 0: h2 slices must start on a 16-channel group"),
    ("input-slice", small(), set_op(0, in_choff=16), "op 0: bad input slice"),
    ("conv-shape", small(), set_op(0, ksize=5), "op 0: unsupported conv (cin 32 choff 0 k 5 s 1)"),
    ("npad", small(), set_op(0, npad=16), "op 0: npad 16 for cout 32"),
    ("conv-weights", small(), set_op(0, w_off=NF), "op 0: weights outside the blob"),
    ("conv-residual", small(), set_op(0, res_buf=1, res_choff=16), "op 0: bad residual slice"),
    ("preact-no-residual", small(), set_op(0, flags=G.FLAG_RES_PREACT), "op 0: PA_CONV_RES_PREACT without a residual slice"),
    ("preact-f16", small("f16", extra_ops=[dict(conv(0, 1), res_buf=0)]), set_op(2, flags=G.FLAG_RES_PREACT),
     "op 2: PA_CONV_RES_PREACT is not implemented for fp16 storage"),
    ("h2-scales", small("h2"), set_op(0, reserved=0), "op 0: h2 row scales outside the blob"),
    ("h2-residual", small("h2", extra_ops=[dict(conv(0, 1), res_buf=3, res_choff=4)], extra_bufs=((0, 48),)), set_op(2, res_choff=2),
     "op 2: h2 residual slice alignment"),
    ("bx3-weights", small(), set_op(0, reserved=NF - 4), "op 0: bf16x3 weights outside the blob"),
    ("level", small(), set_op(1, stride=1), "op 1: level mismatch"),
    ("stem", small(extra_ops=[STEM]), set_op(2, cout=24), "op 2: bad stem"),
    ("stem-level", small(extra_ops=[STEM]), set_op(2, out_buf=1), "op 2: stem output must be level 1"),
    ("sppf", small(extra_ops=[SPPF], extra_bufs=((1, 128),)), set_op(2, in_choff=32), "op 2: bad sppf slices"),
    ("upsample", small(extra_ops=[UPSAMPLE]), set_op(2, cout=16), "op 2: bad upsample"),
    ("maxpool", small(extra_ops=[MAXPOOL]), set_op(2, cout=16), "op 2: bad maxpool"),
    ("maxpool3-f16", small(extra_ops=[MAXPOOL3]), set_desc(dtype="f16"), "op 2: MaxPool2d(3, 2, 1) is not implemented for fp16 storage"),
    ("maxpool3", small(extra_ops=[MAXPOOL3]), set_op(2, cout=16), "op 2: bad 3x3 stride-2 maxpool"),
    ("stem7-f16", small(extra_ops=[STEM7], extra_bufs=((1, 64),)), set_desc(dtype="f16"), "op 2: the 7x7 stem is not implemented for fp16 storage"),
    ("stem7", small(extra_ops=[STEM7], extra_bufs=((1, 64),)), set_op(2, act=G.ACT_SILU), "op 2: bad 7x7 stem"),
    ("stem7-level", small(extra_ops=[STEM7], extra_bufs=((1, 64),)), set_buf(3, 2, 64), "op 2: stem output must be level 1"),
    ("gap-fc-f16", small(extra_ops=[GAP_FC]), set_desc(dtype="f16"), "op 2: the pooled linear head is not implemented for fp16 storage"),
    ("gap-fc", small(extra_ops=[GAP_FC]), set_op(2, act=G.ACT_NONE), "op 2: bad pooled linear head"),
    ("gap-fc-twice", small(extra_ops=[GAP_FC]), lambda g: g["ops"].append(dict(GAP_FC)), "op 3: a graph has one pooled linear head"),
    ("dwconv-f16", small(extra_ops=[DWCONV]), set_desc(dtype="f16"), "op 2: the depthwise conv is not implemented for fp16 storage"),
    ("dwconv", small(extra_ops=[DWCONV]), set_op(2, stride=2), "op 2: bad depthwise conv (3x3, stride 1, cin = cout, act none | SiLU)"),
    ("dwconv-weights", small(extra_ops=[DWCONV]), set_op(2, w_off=NF), "op 2: weights outside the blob"),
    ("dwconv-head", small("h2", extra_ops=[DWCONV]), set_desc(head_buf=[1, -1, -1]), "op 2: a depthwise conv cannot read an fp32 head map of an h2 model"),
    ("dwconv-in-place", small(extra_ops=[DWCONV]), set_op(2, out_buf=1), "op 2: a depthwise conv cannot write the slice it reads"),
    ("dwconv-residual", small(extra_ops=[DWCONV]), set_op(2, res_buf=2), "op 2: bad residual slice"),
    ("psa-f16", small(extra_ops=[PSA], extra_bufs=PSA_BUFS), set_desc(dtype="f16"), "op 2: PSA attention is not implemented for fp16 storage"),
    ("psa-dims", small(extra_ops=[PSA], extra_bufs=PSA_BUFS), set_op(2, ksize=16), "op 2: PSA attention is implemented for key dim 32 and head dim 64 only (got kd 16, hd 64)"),
    ("psa", small(extra_ops=[PSA], extra_bufs=PSA_BUFS), set_op(2, cout=32), "op 2: bad PSA attention (heads 1, cin 128, cout 32)"),
    ("psa-head", small("h2", extra_ops=[PSA], extra_bufs=PSA_BUFS), set_desc(head_buf=[3, -1, -1]), "op 2: PSA attention cannot read an fp32 head map of an h2 model"),
    ("psa-in-place", small(extra_ops=[PSA], extra_bufs=PSA_BUFS), set_op(2, out_buf=3), "op 2: PSA attention cannot write the slice it reads"),
    ("kind", small(), set_op(1, kind=99), "op 1: unknown kind 99"),
    ("head-buffer", small(task=G.TASK_DETECT, nc=4, **HEADS), set_buf(4, 5, 104), "model desc: head buffer 1"),
    ("kpt-shape", small(task=G.TASK_POSE, nc=1, nk=39, kpt_dim=3, **HEADS), set_desc(kpt_dim=4), "model desc: kpt shape"),
]


def _copy(g):
    return dict(g, bufs=list(g["bufs"]), ops=[dict(o) for o in g["ops"]], head_buf=list(g["head_buf"]))


def _text(g):
    return describe(g["task"], g["dtype"], g["bufs"], g["ops"], g["head_buf"], g["nc"], g["nk"], g["kpt_dim"], g["in_channels"], g["n_floats"])


@pytest.fixture(scope="module")
def refusal_answers(harness):
    text = ""
    for _, g, change, _ in REFUSALS:
        broken = _copy(g)
        change(broken)
        text += _text(g) + "validate\n" + _text(broken) + "validate\n"
    lines = ask(harness, text)
    assert len(lines) == 2 * len(REFUSALS)
    return {case[0]: (lines[2 * i], lines[2 * i + 1]) for i, case in enumerate(REFUSALS)}


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_each_refusal_is_reachable_and_fires_first(refusal_answers, case):
    name, _, _, message = case
    untouched, broken = refusal_answers[name]
    assert untouched == "ok", f"{name}: the graph before the change: {untouched}"
    assert broken.startswith("refused: ") and message in broken, f"{name}: {broken}"


def test_every_refusal_of_validate_desc_has_a_case():
    """The parametrised list above has one case per FAIL of validate_desc, in the function's own order."""
    src = (CSRC / "graph_plan.cpp").read_text()
    body = src[src.index("int validate_desc("):src.index("\n}\n", src.index("int validate_desc("))]
    assert body.count("FAIL(") == len(REFUSALS) == 45


def test_refusals_of_the_yolo11_ops_through_the_builder(harness):
    """The two graphs of tests/test_gpu_yolo11_ops.py::test_new_ops_are_validated, made with the graph builder."""
    z = lambda *shape: np.zeros(shape, np.float32)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F32)
    b0, S = g.buf(0, 64), g.buf(0, 48)
    g.conv((b0, 0, 64), (S, 0), z(48, 64, 1, 1), z(48), 1, 1, G.ACT_NONE)
    ok = ask(harness, describe_graph(g) + "validate\n")
    g.dwconv3((b0, 16, 16), (b0, 24), z(16, 1, 3, 3), z(16), G.ACT_NONE)          # writes the slice it reads
    g.head_buf = (S, -1, -1)
    bad = ask(harness, describe_graph(g) + "validate\n")
    assert ok == ["ok"] and "cannot write the slice it reads" in bad[0], (ok, bad)
    g = G.Graph(task=G.TASK_TRACKNET, dtype=G.DTYPE_F32)
    b0, b1 = g.buf(0, 2 * (2 * 16 + 64)), g.buf(0, 128)
    g.psa_attn((b0, 0), (b1, 0), heads=2, kd=16, hd=64)
    g.head_buf = (b1, -1, -1)
    assert "key dim 32 and head dim 64 only" in ask(harness, describe_graph(g) + "validate\n")[0]


def test_plan_time_refusals(harness):
    g = small()
    lines = ask(harness, _text(g) + "validate\nplan 32 64 2 1\nplan 32 63 2 1\nplan 31 64 2 0\n" +
                "geometry 1760 1760 1760 0 0\ngeometry 1792 1792 1792 0 0\ngeometry 640 640 600 0 0\ngeometry 640 640 640 7 0\n")
    assert lines[0] == "ok" and lines[1].startswith("plan ")
    assert lines[2] == "refused: network input 32x63 is not a multiple of 2" and lines[3] == "refused: network input 31x64 is not a multiple of 2"
    assert lines[4].startswith("geometry ") and lines[4].split()[-2] == str(220 ** 2 + 110 ** 2 + 55 ** 2)        # 63525 anchors: the last imgsz that fits
    assert lines[5] == f"refused: {224 ** 2 + 112 ** 2 + 56 ** 2} anchors per image exceed the 16-bit sort key"      # 65856
    assert lines[6] == "refused: imgsz 600 must be a positive multiple of 32" and lines[7] == "refused: unknown pre_mode 7"


# ---------------------------------------------------------------------------------------- d. pil_coeffs
@pytest.mark.parametrize("filt", [0, 1], ids=["bicubic", "bilinear"])
def test_pil_coeffs_equal_the_library(harness, filt):
    from padel_analytics_amd import engine as E
    lib = ctypes.CDLL(str(E.lib_path()))
    lines = ask(harness, "".join(f"pil {s} {d} {filt}\n" for s, d in PIL_SIZES))
    for (s, d), ln in zip(PIL_SIZES, lines):
        left, right = ln.split("|")
        ks, bounds, coefs = int(left.split()[1]), [int(x) for x in left.split()[2:]], [int(x) for x in right.split()]
        k = ctypes.c_int(0)
        assert lib.pa_pil_coeffs(s, d, filt, None, None, 0, ctypes.byref(k)) == 0 and k.value == ks, (s, d)
        b, c = (ctypes.c_int32 * (2 * d))(), (ctypes.c_int32 * (ks * d))()
        assert lib.pa_pil_coeffs(s, d, filt, b, c, ks * d, ctypes.byref(k)) == 0
        assert list(b) == bounds and list(c) == coefs, (s, d)


# ---------------------------------------------------------------------------------------- recording
def record(exe, commit):
    descs = build_descs()
    ans = answers(exe, descs)
    out = {"recorded_from": commit,
           "note": "decisions of the engine's host-side planning code for every shipped graph family (synthetic weights): tests/graph_plan_main.cpp "
                   "compiled against the engine source of the commit above (tests/test_graph_plan_host.py says how)",
           "plan": f"batch {BATCH}, network input 64 x 64 (TrackNet-task graphs: 32 x 64); sha256 of the harness's offset:bytes row",
           "general": general_answers(exe),
           "graphs": {name: golden_record(a) for name, a in ans.items()}}
    body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in out["graphs"].items())
    gen = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in out["general"].items())
    head = ",\n".join(f" {json.dumps(k)}: {json.dumps(out[k])}" for k in ("recorded_from", "note", "plan"))
    GOLDEN.write_text("{" + head[1:] + ",\n \"general\": {\n" + gen + "\n },\n \"graphs\": {\n" + body + "\n }}\n")
    json.loads(GOLDEN.read_text())


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="HARNESS", help="tests/graph_plan_main.cpp built against the commit to record from")
    ap.add_argument("--commit", required=True, help="that commit")
    a = ap.parse_args()
    record(Path(a.record), a.commit)
    print(f"wrote {GOLDEN}", file=sys.stderr)
