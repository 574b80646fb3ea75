"""The table of tests/resample_rows.py, checked on the CPU (needs the built library for ``E.pil_coeffs``, no GPU): for every row

a. the device tables replayed in numpy, horizontal pass then vertical pass, equal ``Image.resize`` byte for byte — the bilinear pin of
   tests/test_resnet_host.py extended to the bicubic filter and to odd sizes;
b. Pillow's one-step resize equals its own two-step resize, width first (a condition on the inputs: Pillow 12 resamples a source
   262 or more rows high and 2 to 4 pixels wide vertically first, and the one-step result is then not the horizontal-first one;
   every source width here is at least 90);
c. every bicubic pass that runs (other than the one-tap identity pass and the passes of the 49 / 29-tap row) has a sample below 0 and
   a sample above 255 before the clip, so a kernel without the clip gives other bytes;
d. the tables are as wide as the row claims;
e. the row reaches the launches it names, through the engine's choice restated in ``resample_rows.launches``.
"""
import numpy as np
import pytest

from padel_analytics_amd import engine as E
from tests import resample_rows as RR

IDS = [r["name"] for r in RR.ROWS]


def replay_row(row, frames):
    """-> (result, [(pass, least, greatest value before the clip, table width)])"""
    (sh, sw), (dh, dw) = row["hw"], row["target"]
    cur, seen = frames, []
    if sw != dw:
        cur, lo, hi, ks = RR.replay_pass(cur, dw, 2, row["filter"])
        seen.append(("horizontal", lo, hi, ks))
    if sh != dh:
        cur, lo, hi, ks = RR.replay_pass(cur, dh, 1, row["filter"])
        seen.append(("vertical", lo, hi, ks))
    return cur, seen


@pytest.mark.parametrize("row", RR.ROWS, ids=IDS)
def test_row(row):
    frames = RR.frames_of(row["name"])[:row["batch"]]
    assert frames.shape == (row["batch"],) + row["hw"] + (3,) and len({f.tobytes() for f in frames}) == len(frames)
    got, seen = replay_row(row, frames)
    want = RR.pillow_of(row["name"])[:row["batch"]]
    # a. the replay is Pillow
    assert got.shape == want.shape == (row["batch"],) + row["target"] + (3,)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} bytes differ"
    # b. Pillow itself went width first
    for f, w in zip(frames, want):
        assert np.array_equal(RR.pillow_two_step(f, row["target"], row["filter"]), w)
    # c. the clip is exercised on both sides
    for which, lo, hi, _ in seen:
        print(f"{row['name']}: {which} pass before the clip: {lo} .. {hi}")
        if row["filter"] == E.PIL_BICUBIC and row["name"] != RR.NO_OVERSHOOT:
            assert lo < 0 and hi > 255, (which, lo, hi)
    # d. tap counts
    widths = {which: ks for which, _, _, ks in seen}
    identity = RR.launches(row) == (RR.V_IDENTITY,)
    assert (widths.get("horizontal", 0), 1 if identity else widths.get("vertical", 0)) == row["taps"]
    # e. the launches
    assert RR.launches(row) == row["reach"]


def test_same_size_is_a_copy_in_pillow():
    for name in ("yolo 160x160", "ball 288x512"):
        assert np.array_equal(RR.pillow_of(name), RR.frames_of(name))


def test_the_table_covers_what_it_is_for():
    reach = [r["reach"] for r in RR.ROWS]
    for kind in (RR.COPY, RR.H_LAST, RR.H_TMP, RR.VPASS4, RR.V_GENERIC, RR.V_IDENTITY):
        assert any(kind in r for r in reach), kind
    yolo = {r["name"]: r for r in RR.YOLO_ROWS}
    # the generic vertical 3 -> 4-byte launch: only the misaligned source reaches it, with the frames of the aligned row
    assert [n for n, r in yolo.items() if RR.V_GENERIC in r["reach"]] == ["yolo 117x160 +1"]
    assert RR.frames_of("yolo 117x160 +1").tobytes() == RR.frames_of("yolo 117x160").tobytes()
    assert yolo["yolo 1080x1917"]["taps"] == (49, 29)
    # frames after the first start at an odd byte offset in some row of every family; sources with an odd width and an odd height
    for rows in (RR.YOLO_ROWS, RR.RESNET_ROWS, RR.BALL_ROWS):
        assert any((r["hw"][0] * r["hw"][1] * 3) % 2 for r in rows)
        assert any(r["hw"][0] % 2 and r["hw"][1] % 2 for r in rows)
    # one axis up, the other down
    assert any(r["hw"][0] < RR.YOLO_S < r["hw"][1] for r in RR.YOLO_ROWS) and any(r["hw"][1] < RR.YOLO_S < r["hw"][0] for r in RR.YOLO_ROWS)
    # the ball ring wraps inside one feed of two frames
    assert RR.BALL_FRAMES > 2 + 7 and (2 + 7) % 2 == 1
