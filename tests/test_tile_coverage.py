"""CPU tests that keep the forced-tile sweeps honest (no GPU, no engine library).

* From tests/tile_support.py alone: every tile id of the parametrised sweeps (tests/test_gpu_h2.py, test_gpu_conv.py,
  test_gpu_fp16.py) runs NATIVELY — launched id == requested id — on at least one case of every class its kernel supports
  (whole tiles, partial pixel tile / partial patch in y and in x, partial channel tile, partial channel fragment, with and
  without residual, a wrapped K loop) and every kernel family sees every activation.  No cell is excused: a class a kernel does
  not have (the K loop of the wide patch kernels) is absent from the table's ``required_classes``.
* The pair-store test (tests/test_gpu_h2_epilogue.py) reaches the three pair paths of h2_epilogue on every tile id.
* The premise of that test: an identity 1x1 reads a pair back exactly, on the CPU twin of the arithmetic.
* The fp16 store test (tests/test_gpu_f16_epilogue.py) reaches, on every fp16 tile id, every store path of f16_epilogue its
  fragment count allows, through both heads; its clamp cases reach a 16-byte and an element-wise path on every id.
* ``parse_profile_text`` reads 10-, 11-, 12- and 13-column lines."""
import numpy as np
import pytest

from padel_analytics_amd import engine as E, graph as G
from tests import tile_support as TS
from tests import test_gpu_conv as TC, test_gpu_fp16 as TF, test_gpu_h2 as TH, test_gpu_h2_epilogue as TE, test_gpu_f16_epilogue as T16

SWEEPS = {
    "h2": (TH.H2_TILES, [(c, False) for c in TH.H2_CASES] + [(c, ws) for c in TH.W_SINGLE_CASES for ws in (True, False)]),
    "tap": (TC.TAP_VARIANTS, [(c, False) for c in TC.CASES]),
    "bx3": (TC.BX3_VARIANTS, [(c, False) for c in TC.CASES]),
    "f16": (TF.VARIANTS + TF.PATCH_VARIANTS, [(c, False) for c in TF.CASES]),
}


@pytest.mark.parametrize("path", sorted(SWEEPS))
def test_every_tile_runs_natively_on_every_class_its_kernel_supports(path):
    tiles, runs = SWEEPS[path]
    gaps = TS.coverage_gaps(path, tiles, runs)
    assert not gaps, f"{path} sweep: unfilled (tile, family, class) cells: {gaps}"


@pytest.mark.parametrize("path", sorted(SWEEPS))
def test_only_duplicate_runs_are_dropped(path):
    """``plan`` keeps every native run; a dropped id resolves to a (family, tile) that the same case's plan runs under its own id."""
    tiles, runs = SWEEPS[path]
    for case, ws in runs:
        kept = dict(TS.plan(path, tiles, case, ws))
        for t in tiles:
            want = TS.expected(path, t, case, ws)
            if want[1] == t:
                assert kept.get(t) == want
            elif t not in kept:
                assert kept.get(want[1]) == want, (path, t, case, want)
        assert all(TS.expected(path, t, case, ws)[1] in TS.SHAPES[path] for t in tiles)


def test_table_spot_checks():
    """A few rows a reader can check against csrc/kernels.h by eye."""
    c = lambda cin, cout, k, s: (1, 16, 16, cin, cout, k, s, G.ACT_SILU, False)
    assert TS.expected("h2", 324, c(64, 96, 3, 1), True) == ("h2r", 324)
    assert TS.expected("h2", 324, c(64, 96, 3, 1), False) == ("h2q", 323)           # 96-channel register-weight tiles: two-product layers only
    assert TS.expected("h2", 324, c(48, 96, 3, 1), True) == ("h2p", 303)            # a 16-channel tail: neither quad kernel
    assert TS.expected("h2", 324, c(64, 96, 1, 1), True) == ("h2t", 220)
    assert TS.expected("h2", 245, c(688, 96, 1, 1), True) == ("h2d", 243)           # 21 chunks + a tail: not the register-weights 1x1
    assert TS.expected("h2", 245, c(704, 96, 1, 1), True) == ("h2s", 245)
    assert TS.expected("h2", 246, c(64, 96, 3, 2), False) == ("h2t", 213)
    assert TS.expected("h2", 343, c(32, 48, 3, 1), False) == ("h2w", 343)
    assert TS.expected("bx3", 306, c(64, 96, 1, 1)) == ("bx3t", 206)
    assert TS.expected("f16", 326, c(64, 96, 3, 2)) == ("tap16", 31)
    assert TS.expected("f16", 326, c(64, 96, 3, 1)) == ("p16q", 326)
    assert TS.ACTS == (G.ACT_NONE, G.ACT_SILU, G.ACT_RELU, G.ACT_SIGMOID, G.ACT_LEAKY)


def test_pair_store_cases_reach_every_path_on_every_tile():
    """h2_epilogue's pair paths: 16-byte stores, the same with 16-byte residual loads, element-wise — each on every tile id."""
    seen = {}
    for case in TE.EPI_CASES:
        for t, ws in TE.native_runs(case):
            fam = TS.expected("h2", t, case, ws)[0]
            seen.setdefault((t, fam), set()).update(TS.h2_store_paths(fam, t, case))
    assert {t for t, _ in seen} == set(TH.H2_TILES)
    assert ("h2w", 343) in {(f, t) for t, f in seen}
    missing = {k: {"fast", "fast_res", "slow"} - v for k, v in seen.items() if {"fast", "fast_res", "slow"} - v}
    assert not missing, missing
    for case in TE.OVF_CASES:
        assert case[7] != G.ACT_SIGMOID
    paths = {}
    for case in TE.OVF_CASES:
        for t, ws in TE.native_runs(case):
            paths.setdefault(t, set()).update(p[:4] for p in TS.h2_store_paths(TS.expected("h2", t, case, ws)[0], t, case))
    assert all(paths.get(t) == {"fast", "slow"} for t in TH.H2_TILES), paths


def test_f16_store_paths_by_hand():
    """Rows a reader can check against csrc/f16_epilogue.h and the launcher tables by eye."""
    full, part = T16.CASES[0], T16.CASES[3]
    res = T16.CASES[1]
    assert TS.f16_store_paths("tap16", 6, full, "f16") == {"pair16"}                       # NF 4: two pairs
    assert TS.f16_store_paths("tap16", 7, full, "f16") == {"pair16", "tail8"}              # NF 3: a pair and the 8-byte leftover
    assert TS.f16_store_paths("tap16", 12, full, "f16") == {"tail8"}                       # NF 1: the leftover alone
    assert TS.f16_store_paths("p16q", 323, res, "f16") == {"pair16_res", "tail8_res"}
    assert TS.f16_store_paths("p16", 306, res, "f16") == {"pair16_res"}                    # NF 6
    assert TS.f16_store_paths("tap16d", 47, full, "f32") == {"f32"}
    assert TS.f16_store_paths("tap16d", 47, res, "f32") == {"slow_f32"}                    # an fp32 head with a residual is never ``wide``
    assert TS.f16_store_paths("tap16", 7, part, "f16") == {"slow"} and TS.f16_store_paths("tap16", 7, part, "f32") == {"slow_f32"}
    assert {t for t, nf in TS.F16_NF.items() if nf & 1} == {7, 12, 20, 31, 47, 60, 71, 303, 323}


def _f16_paths(cases, tiles_of=T16.native_tiles):
    seen = {}
    for case in cases:
        for t in tiles_of(case):
            for head, c in T16.head_runs(case):
                fam = TS.expected("f16", t, c)[0]
                seen.setdefault(t, set()).update(TS.f16_store_paths(fam, t, c, head))
    return seen


def test_f16_store_cases_reach_every_path_on_every_tile():
    """f16_epilogue: 16-byte pair stores, the 8-byte leftover of an odd NF, both with the residual loads, 16-byte fp32 stores and the
    two element-wise forms — each on every tile id whose NF has it, natively, over the cases of tests/test_gpu_f16_epilogue.py."""
    assert set(T16.TILES) == set(TS.SHAPES["f16"]) == set(TS.F16_NF)
    seen = _f16_paths(T16.CASES)
    missing = {t: TS.f16_paths_of_tile(t) - seen.get(t, set()) for t in T16.TILES if TS.f16_paths_of_tile(t) - seen.get(t, set())}
    assert not missing, missing
    assert all(seen[t] == TS.f16_paths_of_tile(t) for t in T16.TILES), "a path the tile's NF does not have"
    assert "pair16" not in seen[12] and all("tail8" not in seen[t] for t in T16.TILES if TS.F16_NF[t] % 2 == 0)
    # each kernel group (stride-1 3x3 with the patch kernels, 1x1, stride-2 3x3) has whole and partial tiles, a partial fragment, and
    # every fp16 family sees every activation but through the epilogue they share
    for k, s in ((3, 1), (1, 1), (3, 2)):
        grp = [c for c in T16.CASES if (c[5], c[6]) == (k, s)]
        for t in T16.TILES:
            if not any(TS.native("f16", t, c) for c in grp):
                assert t >= 300 and (k, s) != (3, 1)
                continue
            cls = set().union(*(TS.classes("f16", TS.expected("f16", t, c)[0], t, c) for c in grp if TS.native("f16", t, c)))
            assert {"full", "n_tail16", "res", "nores"} <= cls and cls & {"m_tail", "patch_y"}, (k, s, t, cls)
    assert {c[7] for c in T16.CASES} == set(TS.ACTS)
    # the clamp: no sigmoid; a 16-byte and an element-wise path on every id; the negative value behind ACT_NONE on both
    clamp = [T16.CASES[i] for i in T16.CLAMP_CASES]
    assert all(c[7] != G.ACT_SIGMOID for c in clamp)
    for cases in (clamp, [c for c in clamp if c[7] == G.ACT_NONE]):
        got = {}
        for case in cases:
            for t in T16.native_tiles(case):
                got.setdefault(t, set()).update("slow" if p == "slow" else "fast" for p in TS.f16_store_paths(TS.expected("f16", t, case)[0], t, case, "f16"))
        if cases is clamp:
            assert all(got.get(t) == {"fast", "slow"} for t in T16.TILES), got
        else:
            assert {"fast", "slow"} <= set().union(*got.values())
    # small magnitudes: per family one whole-tile and one partial-tile run, each with a packed and a scalar conversion
    fams = {}
    for i, tiles in T16.SMALL_RUNS:
        for t in tiles:
            assert TS.native("f16", t, T16.CASES[i])
            fam = TS.expected("f16", t, T16.CASES[i])[0]
            fams.setdefault(fam, set()).update(TS.f16_store_paths(fam, t, T16.CASES[i], "f16"))
    assert set(fams) == set(T16.FAMILIES) and all(v & {"slow"} and v - {"slow"} for v in fams.values()), fams


@pytest.mark.parametrize("corner", [False, True], ids=["mid", "corner"])
@pytest.mark.parametrize("i", range(len(TE.OVF_CASES)))
def test_overflow_cases_plant_exactly_one_value(i, corner):
    TE.overflow_inputs(TE.OVF_CASES[i], corner)           # asserts its own premises on the fp64 reference


def test_identity_readback_of_pairs_is_exact():
    """An identity 1x1 of an h2 graph packs as wh = 4096 (row scale 2^12), wm = 0, output scale 2^-12; the three products of the
    kernels give main = 4096 h, cross = 4096 m, and the epilogue fma(cross, 1 / 2048, main) * 2^-12 + 0 is the pair's value bit
    for bit: the fp32 head behind an identity conv holds ``h2_value`` of what the producer stored."""
    planes, inv = G.pack_conv_weight_h2(np.eye(16, dtype=np.float32)[:, :, None, None])
    h = planes[:, 0, 0, :16].view(np.float16).astype(np.float32)
    assert np.array_equal(h, 4096.0 * np.eye(16, dtype=np.float32)) and G.h2_weights_single(planes)
    assert np.array_equal(inv, np.full(16, 2.0 ** -12, np.float32))
    rng = np.random.default_rng(0)
    x = (rng.choice([-1.0, 1.0], 320000) * np.exp(rng.uniform(np.log(1e-7), np.log(1e3), 320000))).astype(np.float32)
    x = np.concatenate([x, np.float32([0.0, -0.0, 65504.0, -65504.0, 1e5, 6.1e-5, 5.96e-8, 2047.5, 2048.5])])
    hh, mm = G.h2_split(x)
    v = G.h2_value(hh, mm)
    main = np.float32(4096.0) * hh.astype(np.float32)                  # one non-zero product per sum: exact
    cross = np.float32(4096.0) * mm.astype(np.float32)
    fma = (cross.astype(np.float64) * (1.0 / 2048.0) + main.astype(np.float64)).astype(np.float32)      # exact in fp64, rounded once: an fma
    got = fma * np.float32(2.0 ** -12) + np.float32(0.0)
    assert np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, v.view(np.uint32) & 0x7FFFFFFF) and np.array_equal(got, v)
    assert np.array_equal(v.astype(np.float64), hh.astype(np.float64) + mm.astype(np.float64) / 2048.0), "a pair's value is exact in fp32"
    # ... and re-encoding the value the head holds gives the value again (what the exactness assertion compares)
    assert np.array_equal(G.h2_value(*G.h2_split(v)), v)


def test_profile_rows_parse_old_and_new_lines():
    rows = E.parse_profile_text("2,3,1920,64,32,1,128,96,0.01234,70778880\n"
                                "2,3,1920,64,32,1,128,96,0.01234,70778880,1\n"
                                "2,3,1920,64,32,1,128,96,0.01234,70778880,1,323\n"
                                "2,3,1920,64,32,1,128,96,0.01234,70778880,0,323,h2q\n"
                                "5,0,0,0,0,0,0,0,0.00100,0,0,-1,\n")
    assert [r["res"] for r in rows] == [0, 1, 1, 0, 0]
    assert [r["tile"] for r in rows] == [-1, -1, 323, 323, -1]
    assert [r["family"] for r in rows] == ["", "", "", "h2q", ""]
    for r in rows[:4]:
        assert (r["kind"], r["ksize"], r["M"], r["cout"], r["cin"], r["stride"], r["mf"], r["nf"]) == (2, 3, 1920, 64, 32, 1, 128, 96)
        assert r["ms"] == pytest.approx(0.01234) and r["flops"] == 70778880.0
