"""The perspective warp without a GPU (include/padel_hip.h, ``pa_warp_perspective``): the numpy twin ``topdown.warp_host`` against an
independent statement of the rule and against answers known beforehand, the shared header csrc/warp_math.h through the stand-alone
program tests/warp_main.cpp (g++ -ffp-contract=off; once more under the address and undefined-behaviour sanitizers) bit for bit
against the twin, and one case per refusal of ``pa_warp_check`` with the twin raising the same words."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from padel_analytics_amd import engine as E, topdown as T
from tests import warp_cases as W

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "padel_analytics_amd" / "csrc"
NAMED = W.named_cases()


def twin(c: W.Case) -> np.ndarray:
    return T.warp_host(c.frames, c.matrices, c.valid, c.oh, c.ow, c.fill)


@pytest.fixture(scope="module")
def seeded():
    """The seeded cases and the twin's answers, computed once."""
    cases = W.seeded_cases()
    return cases, [twin(c) for c in cases]


# ---------------------------------------------------------------------------------------------- the twin
def test_the_twin_is_float64_bilinear_at_quantised_coordinates_rounded_half_up(seeded):
    cases, answers = seeded
    assert len(cases) >= 300
    filled = 0
    for c, got in list(zip(cases, answers))[:60] + [(c, twin(c)) for c in NAMED.values()]:
        want = W.reference(c)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), c.name
        filled += int((want == np.array(c.fill, np.uint8)).all(axis=-1).sum())
    assert filled > 500                                   # the fill rules were exercised, and so was the picture:
    assert sum(int((a != np.array(c.fill, np.uint8)).any(axis=-1).sum()) for c, a in zip(cases, answers)) > 10000


def test_identity_copies_the_frame():
    c = NAMED["identity"]
    assert np.array_equal(twin(c), c.frames)


def test_an_integer_translation_copies_the_shifted_frame_with_fill_outside():
    c = NAMED["translation by (3, -2)"]                      # canvas (u, v) reads source (u + 3, v - 2)
    want = np.empty_like(c.frames)
    want[:] = np.array(c.fill, np.uint8)
    want[0, 2:, :10] = c.frames[0, :7, 3:]
    assert np.array_equal(twin(c), want)


def test_half_a_pixel_averages_the_neighbours():
    """2 x 2 source, fill 0, every canvas pixel half a pixel right and down.  (0, 0) is the mean of all four: (10 + 20 + 30 + 41) / 4 =
    25.25 -> 25.  (1, 0) has the right-hand taps outside: (20 + 41) / 4 = 15.25 -> 15.  (0, 1): (30 + 41) / 4 = 17.75 -> 18.
    (1, 1): 41 / 4 = 10.25 -> 10.  G and R likewise: 50.25, 30.25, 35.25, 20.25 and 75.25, 45.25, 52.75, 30.25."""
    assert twin(NAMED["half a pixel"])[0].tolist() == [[[25, 50, 75], [15, 30, 45]], [[18, 35, 53], [10, 20, 30]]]


def test_a_hair_below_zero_is_cell_minus_one_with_weight_31():
    """sx = u - 1e-20 is u for u >= 1 (the sum rounds) and -1e-20 for u = 0: floor(32 sx) = -1, cell -1, weight 31 — so column 0 is
    (fill + 31 P(0, y)) / 32 across, not an index error and not P(1, y)."""
    c = NAMED["a hair below zero"]
    got = twin(c)
    f, fill = c.frames[0].astype(np.int64), np.array(c.fill, np.int64)
    assert np.array_equal(got[0, 1:, 1:], c.frames[0, 1:, 1:])
    # (0, 0): row -1 is fill throughout (top = 32 fill, weight 1), row 0 is the mix across (weight 31)
    assert np.array_equal(got[0, 0, 0], (fill * 32 * 1 + (fill + f[0, 0] * 31) * 31 + 512) >> 10)
    # (0, 3): sy = 3 exactly, weight 0 down: the mix across alone
    assert np.array_equal(got[0, 3, 0], ((fill + f[3, 0] * 31) * 32 + 512) >> 10)
    assert np.array_equal(got, W.reference(c))


def test_what_is_fill():
    fill = lambda c: np.array(c.fill, np.uint8)
    c = NAMED["behind the horizon"]                          # Z = 4 - v
    got = twin(c)
    assert (got[0, 4:] == fill(c)).all() and not (got[0, :4] == fill(c)).all(axis=-1).all()
    for name in ("zero over zero", "not valid"):
        c = NAMED[name]
        assert (twin(c) == fill(c)).all(), name
    c = NAMED["infinity minus infinity"]                     # X = 1e308 u - 1e308 v: NaN where both products overflow
    got = twin(c)
    assert (got[0, 2:, 2:] == fill(c)).all()
    assert np.array_equal(got[0, 0, 0], c.frames[0, 0, 0])   # (0, 0) is the source's corner


# ---------------------------------------------------------------------------------------------- the shared header
def build_program(out: Path, *flags) -> Path:
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", str(ROOT / "tests" / "warp_main.cpp"),
                    str(CSRC / "warp_check.cpp"), "-o", str(out)], check=True)
    return out


def check_program(exe: Path, tmp_path, seeded) -> None:
    cases, answers = seeded
    cases = list(cases) + list(NAMED.values())
    answers = list(answers) + [twin(c) for c in NAMED.values()]
    W.write_cases(tmp_path / "cases.bin", cases)
    done = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True)
    assert done.returncode == 0 and done.stderr == b"", done.stderr.decode()
    got = W.read_answers(done.stdout, [(c.frames.shape[0], c.oh, c.ow) for c in cases])
    for c, g, a in zip(cases, got, answers):
        assert isinstance(g, np.ndarray), (c.name, g)
        assert np.array_equal(g, a), c.name


def test_the_shared_header_equals_the_twin_bit_for_bit(tmp_path, seeded):
    check_program(build_program(tmp_path / "warp_main"), tmp_path, seeded)


def test_the_program_runs_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path, seeded):
    exe = build_program(tmp_path / "warp_asan", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer")
    check_program(exe, tmp_path, seeded)


# ---------------------------------------------------------------------------------------------- the refusals
OK = dict(n=1, h=4, w=5, oh=3, ow=6, matrices=np.eye(3)[None], valid=[1])
NAN_M, INF_M = np.eye(3)[None].copy(), np.tile(np.eye(3), (2, 1, 1))
NAN_M[0, 1, 2], INF_M[1, 2, 0] = np.nan, np.inf
REFUSALS = {
    "no frame": (dict(n=0, matrices=np.zeros((0, 3, 3)), valid=[]), "n = 0, at least one frame is needed"),
    "h": (dict(h=0), "h = 0 outside [1, 4096]"),
    "w": (dict(w=4097), "w = 4097 outside [1, 4096]"),
    "oh": (dict(oh=4097), "oh = 4097 outside [1, 4096]"),
    "ow": (dict(ow=0), "ow = 0 outside [1, 4096]"),
    "no matrices": (dict(matrices=None), "is NULL"),
    "no valid": (dict(valid=None), "is NULL"),
    "nan": (dict(matrices=NAN_M), "entry 5 of frame 0's matrix is not finite"),
    "infinity in the second frame": (dict(n=2, matrices=INF_M, valid=[1, 1]), "entry 6 of frame 1's matrix is not finite"),
    "overlap": (dict(overlap=True), "dst overlaps src"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_one_refusal_per_reason_in_the_check_and_in_the_twin(name):
    r, said = REFUSALS[name]
    a = dict(OK, **{k: v for k, v in r.items() if k != "overlap"})
    n, h, w, oh, ow = a["n"], a["h"], a["w"], a["oh"], a["ow"]
    frames, out = np.zeros((n, h, w, 3), np.uint8), None
    if r.get("overlap"):                                      # frames and canvas out of one block: the canvas begins at the source's last byte
        block = np.zeros(256, np.uint8)
        frames, out = block[:n * h * w * 3].reshape(n, h, w, 3), block[n * h * w * 3 - 1:][:n * oh * ow * 3]
    why = E.warp_check(n, h, w, oh, ow, a["matrices"], a["valid"], src=frames.ctypes.data or 1,
                       **({"dst": out.ctypes.data} if out is not None else {}))
    assert why is not None and why.startswith("pa_warp_perspective: ") and said in why, why
    with pytest.raises(ValueError) as twin_said:
        T.warp_host(frames, a["matrices"], a["valid"], oh, ow, out=out)
    assert str(twin_said.value) == why                        # the same words


def test_null_frames_and_canvases_are_refused():
    for kw in (dict(src=None), dict(dst=None)):
        why = E.warp_check(1, 4, 5, 3, 6, np.eye(3), [1], **kw)
        assert why is not None and "is NULL" in why


def test_an_invalid_frame_may_carry_any_matrix_and_touching_buffers_are_accepted():
    m = np.full((2, 3, 3), np.nan)
    m[1] = np.eye(3)
    assert E.warp_check(2, 4, 5, 3, 6, m, [0, 1]) is None
    got = T.warp_host(np.full((2, 4, 5, 3), 9, np.uint8), m, [0, 1], 3, 6, fill=(1, 2, 3))
    assert (got[0] == (1, 2, 3)).all() and (got[1, :, :5] == 9).all() and (got[1, :, 5] == (1, 2, 3)).all()
    src_bytes = 2 * 4 * 5 * 3
    assert E.warp_check(2, 4, 5, 3, 6, m, [0, 1], src=4096, dst=4096 + src_bytes) is None      # dst begins where src ends
    assert E.warp_check(2, 4, 5, 3, 6, m, [0, 1], src=4096, dst=4096 + src_bytes - 1) is not None
    assert E.warp_check(2, 4, 5, 3, 6, m, [0, 1], src=4096 + 2 * 3 * 6 * 3, dst=4096) is None
    assert E.warp_check(1, 4096, 4096, 4096, 4096, np.eye(3), [1]) is None


def test_the_symbols_are_part_of_the_abi():
    assert {"pa_warp_perspective", "pa_warp_check", "pa_warp_last_path"} <= set(E.ABI_SYMBOLS)
    assert E.WARP_MAX_DIM == 4096
