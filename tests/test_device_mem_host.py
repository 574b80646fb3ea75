"""csrc/device_mem.h on the CPU, through tests/device_mem_main.cpp (plain g++, no HIP, no engine library): ``DevMem<T>``, the owner
of every device allocation of the engine, over hooks that are ``malloc`` / ``free`` with counters and a switch that makes a chosen
allocation fail.  Asserted from the counters:

* ``alloc`` then destruction balances; ``reset`` twice frees once;
* ``fit`` at or below the capacity allocates nothing; above it, the old buffer is freed once, first, and exactly ``alloc_bytes`` are
  allocated;
* a failing ``alloc`` or ``fit`` leaves a null pointer with zero bytes, and destruction afterwards frees nothing more (the engine's
  frame and input staging used to keep the freed pointer and the new capacity);
* keep-prefix growth keeps the first ``keep`` bytes and frees the old buffer once; when its copy fails the old buffer stays, contents
  and all, and the new one is freed (the JPEG encoder's ``grow`` used to leak it); likewise when its allocation fails;
* move construction and move assignment transfer ownership; assignment over a full target frees the target's buffer once; a struct
  of several owners assigned from ``T{}`` (``L = Lane{}``) frees each once;
* page-locked buffers go through their own pair of hooks;
* no scenario frees anything twice, and every one ends with zero live bytes.

The program is built once more with the address and undefined-behaviour sanitizers and run on its own: same answers, exit status 0,
nothing on stderr."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
SCENARIOS = ("alloc_then_destroy", "reset_twice", "fit_below_capacity", "fit_above_capacity", "fit_from_empty", "alloc_fails", "fit_fails",
             "keep_prefix", "keep_prefix_from_empty", "keep_prefix_copy_fails", "keep_prefix_alloc_fails", "move_construct",
             "move_assign_into_empty", "move_assign_over_full", "struct_assigned_from_empty", "pinned")


def build(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "device_mem_main.cpp"), "-o", str(out)],
                   check=True)
    return out


def run_program(exe: Path) -> dict:
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr[-4000:]
    out = {}
    for line in done.stdout.splitlines():
        name, *fields = line.split()
        out[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return out


@pytest.fixture(scope="module")
def got(tmp_path_factory) -> dict:
    return run_program(build(tmp_path_factory.mktemp("device_mem") / "device_mem_main"))


def counts(a: dict, allocs: int, frees: int, failed: int = 0):
    assert (a["allocs"], a["frees"], a["failed"]) == (allocs, frees, failed), a


def test_every_scenario_ran_balanced_and_freed_nothing_twice(got):
    assert tuple(got) == SCENARIOS
    for name, a in got.items():
        assert a["live"] == 0 and a["pin_live"] == 0 and a["bad_free"] == 0, (name, a)
        assert a["allocs"] == a["frees"] and a["pin_allocs"] == a["pin_frees"], (name, a)


def test_alloc_then_destruction_balances(got):
    a = got["alloc_then_destroy"]
    assert a["empty_null"] == 1 and a["r"] == 0 and a["bytes"] == 100 and a["nonnull"] == 1
    assert a["live_inside"] == 100 and a["frees_inside"] == 0
    counts(a, 1, 1)
    b = got["reset_twice"]
    assert b["null"] == 1 and b["bytes"] == 0
    counts(b, 1, 1)


def test_fit_below_capacity_allocates_nothing(got):
    a = got["fit_below_capacity"]
    assert a["r"] == 0 and a["r_equal"] == 0 and a["same_ptr"] == 1 and a["bytes"] == 100
    assert a["allocs_inside"] == 1 and a["frees_inside"] == 0
    counts(a, 1, 1)


def test_fit_above_capacity_frees_once_and_allocates_alloc_bytes(got):
    a = got["fit_above_capacity"]
    assert a["r"] == 0 and a["bytes"] == 250 and a["last_alloc_bytes"] == 250 and a["nonnull"] == 1 and a["live_inside"] == 250
    assert a["allocs_inside"] == 2 and a["frees_inside"] == 1 and a["old_freed"] == 1 and a["freed_before_alloc"] == 1
    counts(a, 2, 2)
    b = got["fit_from_empty"]
    assert b["r0"] == 0 and b["allocs_after_fit0"] == 0 and b["r"] == 0 and b["bytes"] == 64
    counts(b, 1, 1)


def test_a_failing_alloc_leaves_the_object_empty(got):
    a = got["alloc_fails"]
    assert a["r"] != 0 and a["null"] == 1 and a["bytes"] == 0
    assert a["r_again"] == 0 and a["bytes_again"] == 30
    counts(a, 1, 1, failed=1)                 # the one allocation that stood, freed once: the failed one left nothing to free


def test_a_failing_fit_leaves_no_pointer_and_no_capacity(got):
    a = got["fit_fails"]
    assert a["r"] != 0 and a["null"] == 1 and a["bytes"] == 0 and a["live_inside"] == 0
    assert a["old_freed"] == 1 and a["frees_inside"] == 1
    counts(a, 1, 1, failed=1)                 # destruction afterwards freed nothing: no second free of the old buffer


def test_keep_prefix_growth(got):
    a = got["keep_prefix"]
    assert a["r_below"] == 0 and a["allocs_below"] == 1
    assert a["r"] == 0 and a["bytes"] == 256 and a["last_alloc_bytes"] == 256 and a["prefix_same"] == 1 and a["live_inside"] == 256
    assert a["old_freed"] == 1 and a["frees_inside"] == 1 and a["allocs_inside"] == 2
    counts(a, 2, 2)
    b = got["keep_prefix_from_empty"]
    assert b["r"] == 0 and b["bytes"] == 32
    counts(b, 1, 1)


def test_keep_prefix_growth_whose_copy_fails_keeps_the_old_buffer_and_frees_the_new(got):
    a = got["keep_prefix_copy_fails"]
    assert a["r"] == 7 and a["same_ptr"] == 1 and a["bytes"] == 64 and a["contents_same"] == 1 and a["live_inside"] == 64
    assert a["old_freed"] == 0 and a["new_freed"] == 1 and a["allocs_inside"] == 2 and a["frees_inside"] == 1
    counts(a, 2, 2)
    b = got["keep_prefix_alloc_fails"]
    assert b["r"] != 0 and b["same_ptr"] == 1 and b["bytes"] == 64 and b["contents_same"] == 1 and b["frees_inside"] == 0
    counts(b, 1, 1, failed=1)


def test_moves_transfer_ownership(got):
    a = got["move_construct"]
    assert a["source_empty"] == 1 and a["target_has"] == 1 and a["frees_inside"] == 0 and a["allocs_inside"] == 1
    counts(a, 1, 1)
    b = got["move_assign_into_empty"]
    assert b["source_empty"] == 1 and b["target_has"] == 1 and b["frees_inside"] == 0
    counts(b, 1, 1)


def test_assignment_over_a_full_target_frees_its_buffer_once(got):
    a = got["move_assign_over_full"]
    assert a["source_empty"] == 1 and a["target_has"] == 1 and a["old_freed"] == 1 and a["frees_inside"] == 1 and a["live_inside"] == 100
    counts(a, 2, 2)


def test_a_struct_assigned_from_an_empty_one_frees_each_member_once(got):
    a = got["struct_assigned_from_empty"]
    assert a["each_freed_once"] == 1 and a["frees_inside"] == 3 and a["members_empty"] == 1 and a["live_inside"] == 0
    assert a["moved_whole"] == 1
    counts(a, 4, 4)


def test_page_locked_buffers_use_their_own_hooks(got):
    a = got["pinned"]
    assert a["r"] == 0 and a["bytes"] == 256 and a["pin_live_inside"] == 256 and a["r_fail"] != 0 and a["fail_null"] == 1
    assert (a["allocs"], a["frees"], a["pin_allocs"], a["pin_frees"]) == (0, 0, 1, 1)


def test_the_sanitizers_stay_silent(got, tmp_path):
    san = run_program(build(tmp_path / "device_mem_main_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert san == got                          # exit status 0 and nothing on stderr: no report from either sanitizer
