"""csrc/launch_plan.cpp on the CPU: what one replay of an op list launches and with which arguments, through the stand-alone harness
tests/launch_plan_main.cpp (g++ against launch_plan.cpp, graph_plan.cpp and conv_select.cpp; no GPU, no engine library).

* same launches as the commit the file was split out of: per (graph, tuning) the number of steps and a SHA-256 of the harness's text
  (one line per launch: launcher, op and ops covered, requested / resolved tile and family, every field of the argument struct, each
  pointer as owner+byte offset) equal tests/golden/launch_plan.json; the two smallest graphs are recorded in full, so a mismatch is
  readable.  The file was recorded from the commit named in it: a scratch translation unit that includes that commit's csrc/engine.cpp,
  stubs the HIP runtime calls it makes (hipMalloc hands out distinct made-up addresses, nothing is dereferenced), defines every
  padel::launch_* as a printer over tests/launch_plan_print.h (the op index: the next op of that kind whose slices match the
  arguments) and drives that commit's own pa_model_create -> plan_buffers -> run_graph (ensure_operand_copies, run_ops) per `steps`
  command; built with the ROCm clang++ (-D__HIP_PLATFORM_AMD__, the ROCm include directory, that commit's conv_select.cpp and
  graph_plan.cpp, -Wl,--unresolved-symbols=ignore-all).  A refusal there comes after the launches in front of it, here before any:
  a refused case records the message alone.  A deliberate change of one of these decisions regenerates the file:
      python -m tests.test_launch_plan_host --record RECORDER --commit SHA
* the rules on graphs of a few ops, with the expected steps written out: an absorbed upsample with and without fold_up and under
  a forced tile whose kernel does not read the coarse map, the fused stem, the PA_CONV_RES_PREACT refusal, the tail marks;
* the harness once more under -fsanitize=address,undefined.

The graphs: the 66 of tests/test_graph_plan_host.py at its network sizes, batch 2; the three the benchmark runs (YOLOv8 n / m detect
at 384 x 640, m pose at 1280 x 1280, h2) at batch 1 and 64.  Tunings: default, fold_up=0, fuse_stem=0, w_single=0, tune=9, impl=0
(f32 graphs), variant=220 and variant=303 (h2 and f32 graphs)."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from padel_analytics_amd import graph as G, yolo_arch
from tests import tile_support as TS
from tests.test_graph_plan_host import BATCH, DTYPES, R_OFF, Desc, build_descs, conv, describe, op

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "launch_plan.json"
TUNINGS = {"default": (), "fold_up0": (("fold_up", 0),), "fuse_stem0": (("fuse_stem", 0),), "w_single0": (("w_single", 0),), "tune9": (("tune", 9),),
           "impl0": (("impl", 0),), "variant220": (("variant", 220),), "variant303": (("variant", 303),)}
BENCH = (("yolov8n-detect", "n", 1, None, 384, 640), ("yolov8m-detect", "m", 80, None, 384, 640), ("yolov8m-pose13", "m", 1, (13, 3), 1280, 1280))
FULL_TEXT = 2                  # graphs recorded in full: the smallest by op count


def build_harness(exe, extra=()):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", *extra, "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
                    str(ROOT / "tests" / "launch_plan_main.cpp"), str(CSRC / "launch_plan.cpp"), str(CSRC / "graph_plan.cpp"),
                    str(CSRC / "conv_select.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("launch_plan") / "launch_plan_main")


def tuning_text(settings):
    return "tuning reset\n" + "".join(f"tuning {k} {v}\n" for k, v in settings)


def blocks(exe, text):
    """-> [(step lines, refusal or None)] per `steps` command of ``text``."""
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    res, lines, refused = [], [], None
    for ln in out:
        if ln.startswith("refused: "):
            refused = ln[len("refused: "):]
        elif ln.startswith("end "):
            assert refused is not None or int(ln.split()[1]) == len(lines), ln
            res.append((lines, refused))
            lines, refused = [], None
        elif ln:
            lines.append(ln)
    return res


def applies(tuning, dtype):
    if tuning == "impl0":
        return dtype == G.DTYPE_F32
    return dtype != G.DTYPE_F16 if tuning.startswith("variant") else True


def cases():
    """[(case name, graph text, dtype, n_ops, net_h, net_w, batch)]: every graph once per batch it is recorded at."""
    out = [(name, d.text, d.dtype, len(d.ops), d.net[0], d.net[1], BATCH) for name, d in build_descs().items()]
    for name, scale, nc, kpt, nh, nw in BENCH:
        d = Desc(G.build_yolov8(yolo_arch.synth_state_dict(scale, nc, kpt, seed=0), nc, kpt, dtype="h2"))
        out += [(f"bench-{name}-b{b}", d.text, d.dtype, len(d.ops), nh, nw, b) for b in (1, 64)]
    return out


def answers(exe, cs):
    """"<case>|<tuning>" -> {"steps", "sha256"} | {"refused"}, plus "text" for the FULL_TEXT smallest graphs."""
    keys, text = [], ""
    full = {c[0] for c in sorted(cs, key=lambda c: c[3])[:FULL_TEXT]}
    for name, gtext, dtype, _, nh, nw, b in cs:
        text += gtext
        for tn, settings in TUNINGS.items():
            if applies(tn, dtype):
                keys.append((name, tn))
                text += tuning_text(settings) + f"steps {nh} {nw} {b} {b}\n"
    got = blocks(exe, text)
    assert len(got) == len(keys)
    out = {}
    for (name, tn), (lines, refused) in zip(keys, got):
        rec = {"refused": refused} if refused is not None else {"steps": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}
        if name in full and refused is None:
            rec["text"] = lines
        out[f"{name}|{tn}"] = rec
    return out


# ---------------------------------------------------------------------------------------- a. the parent commit's launches
def test_same_launches_as_the_recorded_commit(harness):
    gold = json.loads(GOLDEN.read_text())
    assert len(gold["recorded_from"]) >= 7
    got = answers(harness, cases())
    assert sorted(got) == sorted(gold["cases"])
    for key, want in gold["cases"].items():
        if "text" in want and got[key].get("text") != want["text"]:
            diff = [(a, b) for a, b in zip(got[key].get("text", []), want["text"]) if a != b]
            assert False, f"{key}: first differing step (got, recorded): {diff[:1]}"
        assert got[key] == want, key
    recs = gold["cases"].values()
    assert len(gold["cases"]) > 400 and sum("text" in r for r in recs) >= FULL_TEXT and any("refused" in r for r in recs)
    assert gold["cases"]["yolov8n-detect-h2|default"]["steps"] < gold["cases"]["yolov8n-detect-h2|fold_up0"]["steps"]
    assert gold["cases"]["yolov8n-detect-h2|default"]["steps"] < gold["cases"]["yolov8n-detect-h2|fuse_stem0"]["steps"]


# ---------------------------------------------------------------------------------------- b. the rules, by hand
def fields(line):
    """a step line -> (launcher, {field: value}) (a fused stem's second group, the conv's, under "conv.")"""
    groups = line.split(" | ")
    words = groups[0].split() + groups[1].split() + [("conv." + w) for g in groups[2:] for w in g.split()]
    return words[0], dict(w.split("=", 1) for w in words[1:])


def steps_of(exe, g, nh, nw, n=2, tuning=()):
    (lines, refused), = blocks(exe, describe(g["task"], DTYPES[g["dtype"]], g["bufs"], g["ops"], g.get("head_buf", (-1, -1, -1)), g.get("nc", 0),
                                            g.get("nk", 0), g.get("kpt_dim", 0), 32, 1 << 20) + tuning_text(tuning) + f"steps {nh} {nw} {n} {n}\n")
    return [fields(ln) for ln in lines], refused


def up_graph(k):
    """nn.Upsample(2) of 64 channels into the first 64 of a 96-channel map whose only reader is a k x k conv (h2)."""
    return dict(task=G.TASK_TRACKNET, dtype="h2", bufs=[(1, 64), (0, 96), (0, 48)],
                ops=[op(G.OP_UPSAMPLE2X, in_buf=0, cin=64, out_buf=1, cout=64),
                     op(G.OP_CONV, in_buf=1, cin=96, out_buf=2, cout=48, ksize=k, stride=1, act=G.ACT_SILU, npad=48, reserved=R_OFF)])


def test_absorbed_upsample_is_no_step(harness):
    st, refused = steps_of(harness, up_graph(1), 48, 80)
    assert refused is None and [(s[0], s[1]["op"]) for s in st] == [("conv", "1")]
    f = st[0][1]
    assert (f["in2"], f["in2_cs"], f["in2_choff"], f["up_c"], f["in"], f["out"]) == ("buf0+0", "64", "0", "64", "buf1+0", "buf2+0")
    assert (f["H"], f["W"], f["M"], f["oscale"], f["ovf_flag"]) == ("48", "80", str(2 * 48 * 80), f"blob+{4 * R_OFF}", "flag+0")
    st, refused = steps_of(harness, up_graph(1), 48, 80, tuning=(("fold_up", 0),))
    assert refused is None and [(s[0], s[1]["op"]) for s in st] == [("upsample2x", "0"), ("conv", "1")]
    assert (st[1][1]["in2"], st[1][1]["in2_cs"], st[1][1]["up_c"]) == ("null", "0", "0")
    u = st[0][1]
    assert (u["in"], u["out"], u["c"], u["B"], u["H"], u["W"], u["f16"]) == ("buf0+0", "buf1+0", "64", "2", "24", "40", str(G.DTYPE_H2))


def test_forced_tile_whose_kernel_does_not_read_the_coarse_map(harness):
    """Every h2 tile of a 1x1 conv resolves to a kernel that reads in2 (tests/test_conv_select_host.py's table), so the consumer here
    is the 3x3 one: tile 303 is the patch kernel, which reads it; tile 220 is the tap ring (tile_support), which does not."""
    case = (2, 48, 80, 96, 48, 3, 1, G.ACT_SILU, False)
    assert TS.expected("h2", 220, case, 1) == ("h2t", 220) and TS.expected("h2", 303, case, 1) == ("h2p", 303)
    st, _ = steps_of(harness, up_graph(3), 48, 80, tuning=(("variant", 303),))
    assert [s[0] for s in st] == ["conv"] and (st[0][1]["fam"], st[0][1]["in2"]) == ("h2p", "buf0+0")
    st, _ = steps_of(harness, up_graph(3), 48, 80, tuning=(("variant", 220),))
    assert [(s[0], s[1]["op"]) for s in st] == [("upsample2x", "0"), ("conv", "1")]
    assert (st[1][1]["req"], st[1][1]["ran"], st[1][1]["fam"], st[1][1]["in2"], st[1][1]["up_c"]) == ("220", "220", "h2t", "null", "0")


def test_fused_stem_is_one_step_over_two_ops(harness):
    g = dict(task=G.TASK_DETECT, dtype="h2", bufs=[(1, 16), (2, 32)],
             ops=[op(G.OP_STEM, out_buf=0, cin=3, cout=16, ksize=3, stride=2, act=G.ACT_SILU),
                  op(G.OP_CONV, in_buf=0, cin=16, out_buf=1, cout=32, ksize=3, stride=2, act=G.ACT_SILU, npad=32, reserved=R_OFF)])
    st, refused = steps_of(harness, g, 64, 64)
    assert refused is None and [(s[0], s[1]["op"], s[1]["n"]) for s in st] == [("stem_l1_h2", "0", "2")]
    f = st[0][1]
    assert (f["in"], f["out"], f["Ho"], f["cout"], f["out_f16"], f["opw"]) == ("netin+0", "buf0+0", "32", "16", "2", "wr+0")
    assert (f["conv.in"], f["conv.out"], f["conv.H"], f["conv.Ho"], f["conv.cin"], f["conv.cout"], f["conv.stride"]) == ("buf0+0", "buf1+0", "32", "16", "16", "32", "2")
    st, refused = steps_of(harness, g, 64, 64, tuning=(("fuse_stem", 0),))
    assert refused is None and [(s[0], s[1]["op"], s[1]["n"]) for s in st] == [("stem", "0", "1"), ("conv", "1", "1")]
    assert st[1][1]["in"] == "buf0+0" and st[0][1]["out"] == "buf0+0"


def test_preact_residual_is_refused_on_the_tap_family_with_nothing_planned(harness):
    g = dict(task=G.TASK_TRACKNET, dtype="f32", bufs=[(0, 32), (0, 32), (0, 32)],
             ops=[conv(0, 1), dict(conv(1, 2), res_buf=0, flags=G.FLAG_RES_PREACT)])
    st, refused = steps_of(harness, g, 32, 64)
    assert refused is None and [s[0] for s in st] == ["conv", "conv"] and st[1][1]["res_pre"] == "1" and st[1][1]["fam"].startswith("bx3")
    st, refused = steps_of(harness, g, 32, 64, tuning=(("impl", 0),))
    assert st == [] and refused == ("op 1: PA_CONV_RES_PREACT needs the h2 or the bf16x3 kernels (tuning impl = 2, bf16x3 weights in the blob), "
                                    "not the fp32-MFMA tap family")


def test_tail_marks_are_the_ops_of_find_head_tail(harness):
    g = G.build_yolov8(yolo_arch.synth_state_dict("n", 1, (13, 3), seed=0), 1, (13, 3), dtype="h2")
    text = Desc(g).text
    out = subprocess.run([str(harness)], input=text + "tail 64 64 2 2\n", capture_output=True, text=True, check=True).stdout.split()
    marked = [int(x) for x in out[1:]]
    hb = set(g.head_buf)
    want = [i for i, o in enumerate(g.ops) if o["out_buf"] in hb]          # a pose graph: exactly the nine last 1x1 convs write the head maps
    assert out[0] == "tail" and len(marked) == 9 and marked == want
    assert all(g.ops[i]["kind"] == G.OP_CONV and g.ops[i]["ksize"] == 1 for i in marked)


# ---------------------------------------------------------------------------------------- c. sanitizers
def test_harness_under_address_and_undefined_sanitizers(tmp_path):
    exe = build_harness(tmp_path / "launch_plan_main_san", extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    d = Desc(G.build_yolov8(yolo_arch.synth_state_dict("n", 1, (13, 3), seed=0), 1, (13, 3), dtype="h2"))
    text = "".join(d.text + tuning_text(s) + "steps 64 64 2 2\ntail 64 64 2 2\n" for s in TUNINGS.values())
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.count("\nend ") == len(TUNINGS)


# ---------------------------------------------------------------------------------------- recording
def record(exe, commit):
    out = answers(exe, cases())
    head = {"recorded_from": commit,
            "note": "launches of one op-list replay per (graph, tuning): tests/launch_plan_print.h's lines as printed by stand-ins for every "
                    "padel::launch_* under the engine source of the commit above (tests/test_launch_plan_host.py says how)",
            "command": "python -m tests.test_launch_plan_host --record RECORDER --commit SHA"}
    body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in out.items())
    GOLDEN.write_text("{" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in head.items())[1:] + ",\n \"cases\": {\n" + body + "\n }}\n")
    json.loads(GOLDEN.read_text())


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="RECORDER", help="the scratch recorder built over the commit to record from")
    ap.add_argument("--commit", required=True, help="that commit")
    a = ap.parse_args()
    record(Path(a.record), a.commit)
    print(f"wrote {GOLDEN}", file=sys.stderr)
