"""csrc/lane_plan.h on the CPU, through tests/lane_plan_main.cpp (plain g++, no GPU, no engine library): which lane the next
pa_yolo_submit runs on, and whether a model may have a second lane.

* ``pick_lane`` over every combination of busy flags and ticket ages, with and without a second lane, against the rule written
  out here: an idle lane if there is one (lane 0 first), else the lane whose last ticket is older; lane 0 when there is no second;
* replayed over the trackers' loop (submit k + 1 before wait k) and over four tickets in flight, the rule alternates the lanes;
* ``second_lane_wanted``: the knob, and the FLOP gate at and around its threshold (the threshold itself still gets the lane);
* ``second_lane_fits``: the lane must fit and leave one more arena free, at and around both bounds."""
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lane_plan") / "lane_plan_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "lane_plan_main.cpp"), "-o", str(exe)], check=True)
    return exe


def ask(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    out = [ln for ln in out if ln]
    assert len(out) == len(lines), out[-1:]
    return [ln.split()[1] for ln in out]


def rule(second_ok, busy0, last0, busy1, last1):
    if not second_ok or not busy0:
        return 0
    if not busy1:
        return 1
    return 1 if last1 < last0 else 0


def test_pick_lane_every_combination(harness):
    ages = (-1, 0, 1, 2, 7)
    cases = [c for c in itertools.product((0, 1), (0, 1), ages, (0, 1), ages) if c[2] != c[4] or c[2] == -1]
    got = ask(harness, ["pick " + " ".join(str(x) for x in c) for c in cases])
    assert [int(g) for g in got] == [rule(*c) for c in cases]
    assert len(cases) > 150 and {int(g) for g in got} == {0, 1}


def _replay(harness, second_ok, script):
    """script: 's' submit, ('w', k) wait for ticket k -> the lane of every submit, by the harness's answers."""
    busy, last, lane_of, lanes, nxt = [0, 0], [-1, -1], {}, [], 0
    for step in script:
        if step == "s":
            li = int(ask(harness, [f"pick {second_ok} {busy[0]} {last[0]} {busy[1]} {last[1]}"])[0])
            busy[li], last[li], lane_of[nxt] = 1, nxt, li
            lanes.append(li)
            nxt += 1
        else:
            li = lane_of[step[1]]
            if last[li] == step[1]:
                busy[li] = 0
    return lanes


def test_the_batch_loops_alternate(harness):
    loop = ["s"] + [x for k in range(6) for x in ("s", ("w", k))] + [("w", 6)]          # submit k + 1 before wait k
    assert _replay(harness, 1, loop) == [0, 1, 0, 1, 0, 1, 0]
    assert _replay(harness, 0, loop) == [0] * 7
    four = ["s"] * 4 + [("w", 0), ("w", 1), "s", "s"]                                   # four in flight, two collected, two more
    assert _replay(harness, 1, four) == [0, 1, 0, 1, 0, 1]
    sync_like = [x for k in range(4) for x in ("s", ("w", k))]                          # never two in flight: lane 1 is never wanted
    assert _replay(harness, 1, sync_like) == [0] * 4


def test_second_lane_wanted_knob_and_gate(harness):
    t = 3.0e12
    cases = [(1, 1e9, 0, 0), (2, 1e9, 0, 1), (2, 1e15, 0, 1), (2, 1e15, -1, 1), (0, 1e9, 0, 0), (3, 1e9, 0, 1),
             (2, t, t, 1), (2, t * (1 - 1e-12), t, 1), (2, t * (1 + 1e-12), t, 0), (2, 2 * t, t, 0), (2, 0.5 * t, t, 1), (1, 0.5 * t, t, 0)]
    got = ask(harness, [f"wanted {l} {f!r} {g!r}" for l, f, g, _ in cases])
    assert [int(x) for x in got] == [c[3] for c in cases]


def test_second_lane_fits_bounds(harness):
    lane, arena = 12_000_000_000, 11_300_000_000
    cases = [(lane + arena, 1), (lane + arena - 1, 0), (lane + arena + 1, 1), (lane, 0), (lane - 1, 0), (0, 0), (1 << 40, 1)]
    got = ask(harness, [f"fits {f} {lane} {arena}" for f, _ in cases])
    assert [int(x) for x in got] == [c[1] for c in cases]
    assert ask(harness, ["fits 10 10 0", "fits 9 10 0"]) == ["1", "0"]


def test_the_engines_gate_is_a_number(harness):
    assert float(ask(harness, ["gate"])[0]) >= 0
