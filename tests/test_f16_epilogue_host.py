"""CPU checks of the premises of tests/test_gpu_f16_epilogue.py (no GPU, no engine library), on the fp64 reference and on numpy
emulations alone:

* the three graph forms of that file (fp32 head, sentinel + identity readback, residual readback) run through tests/graph_interp on a
  partial-fragment case with residual and on the 8-channel head: the interpreter's halves satisfy statements A and B themselves;
* D: exactly the planted outputs leave the fp16 range, at +-1e5, every other one stays below 6e4 less its bound, the planted input
  stays a half, and the mask of unchanged operands is right (``clamp_premises`` asserts the first three);
* E: the share of results that are subnormal halves, per scale;
* bound B is satisfiable: numpy fp32 emulations of the two accumulation orders — (64-channel chunk, tap, half) of the tap kernels,
  (32-channel chunk, tap) of the patch kernels — stay below a third of it on every case;
* the subset rule of A is not vacuous: the tie-adjacent set is below 1 % of the elements;
* ``rn16`` is round-to-nearest-even with gradual underflow and the clamp, on hand-made values."""
import numpy as np
import pytest
import torch

from tests import stem_probe as P, tile_support as TS
from tests import test_gpu_f16_epilogue as T
from tests.test_gpu_conv import ACT_FN


def _act64(act, t):
    return ACT_FN[act](torch.from_numpy(np.ascontiguousarray(t, np.float64))).numpy()


def emulate(case, d, chunk):
    """fp32 accumulation of the conv over 32-channel k-steps in the order (``chunk``-channel chunk, tap, 32-channel part of the
    chunk), each k-step's 32 exact products summed by an fp32 matrix product (the order inside a matrix instruction is not
    modelled); + bias in fp32.  -> pre-activation fp32 (B, Ho, Wo, cout)."""
    B, H, W, cin, cout, k, s, act, use_res = case
    Ho, Wo = TS.out_hw(case)
    p = k // 2
    x = np.pad(d["x"].astype(np.float32), ((0, 0), (p, p), (p, p), (0, 0)))
    acc = np.zeros((B, Ho, Wo, cout), np.float32)
    for c0 in range(0, cin, chunk):
        for ky in range(k):
            for kx in range(k):
                for c1 in range(c0, min(c0 + chunk, cin), 32):
                    px = x[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, c1:c1 + 32]
                    acc = (acc + (px @ d["w"][:, c1:c1 + 32, ky, kx].T).astype(np.float32)).astype(np.float32)
    return (acc + d["b"]).astype(np.float32)


@pytest.mark.parametrize("i", range(len(T.CASES)))
def test_bound_b_is_satisfiable_in_both_accumulation_orders(i):
    case = T.CASES[i]
    d, ref = T.case_data(i)
    K, act = T.K_of(case), case[7]
    bound = P.conv16_bound(K, act, ref["v"], ref["S"])
    assert (ref["S"] >= np.abs(ref["v"]) * 0).all() and float(ref["S"].min()) > 0
    for chunk in (64, 32):
        t32 = emulate(case, d, chunk)
        err = np.abs(_act64(act, t32) - ref["v"])
        worst = float((err / bound).max())
        assert worst <= 1.0 / 3.0, f"case {i}, {chunk}-channel chunks: the emulation uses {worst:.3f} of the bound"
        # ... and a store of that value as a half stays inside the fp16 bound
        if not case[8]:
            y16 = T.rn16(_act64(act, t32).astype(np.float32))
            assert (np.abs(y16 - ref["v"]) <= P.conv16_bound_f16(K, act, ref["v"], ref["S"])).all()


def test_bound_b_notices_a_dropped_k_step_and_a_flushed_operand():
    i = 12
    case = T.CASES[i]
    d, ref = T.case_data(i)
    bound = P.conv16_bound(T.K_of(case), case[7], ref["v"], ref["S"])
    w_bad = d["w"].copy()
    w_bad[:, :, 2, 2] = 0.0
    assert (np.abs(_act64(case[7], emulate(case, dict(d, w=w_bad), 32)) - ref["v"]) > bound).mean() > 0.3
    d, ref = T.case_data(3, 3e-6, 8.0)              # subnormal x: flushed operands leave act(bias)
    case = T.CASES[3]
    bound = P.conv16_bound(T.K_of(case), case[7], ref["v"], ref["S"])
    flushed = dict(d, x=np.where(np.abs(d["x"]) < np.float16(2.0 ** -14), np.float16(0), d["x"]))
    assert (np.abs(_act64(case[7], emulate(case, flushed, 32)) - ref["v"]) > bound).mean() > 0.9


@pytest.mark.parametrize("corner", [False, True], ids=["mid", "corner"])
@pytest.mark.parametrize("i", T.CLAMP_CASES)
def test_clamp_cases_plant_exactly_the_values_they_claim(i, corner):
    case = T.CASES[i]
    d, ref, planted, same = T.clamp_premises(case, corner)           # asserts its own premises on the fp64 reference
    d0, ref0 = T.case_data(i)
    assert d["x"].dtype == np.float16 and np.array_equal(d["w"], d["w"].astype(np.float16).astype(np.float32))
    # where ``same`` holds, the reference is the unplanted one to the last bit (same operands), and it excludes the planted
    assert np.array_equal(ref["v"][same], ref0["v"][same]) and not any(same[at] for at in planted)
    if case[8]:
        assert np.array_equal(ref["r"][same], ref0["r"][same])
    assert same.mean() > 0.8
    # without the clamp the planted halves would be infinite
    with np.errstate(over="ignore"):
        for at, sgn in planted.items():
            assert np.isinf(np.float32(ref["v"][at]).astype(np.float16)) and T.rn16(np.float32(ref["v"][at])) == np.float32(sgn * 65504.0)


@pytest.mark.parametrize("xs,ws,sub", T.SMALL_SCALES, ids=[f"x{xs:g}-w{ws:g}" for xs, ws, _ in T.SMALL_SCALES])
def test_small_scales_put_results_and_operands_into_the_subnormal_range(xs, ws, sub):
    tiny = lambda a: float(((np.abs(a) < 2.0 ** -14) & (a != 0)).mean())
    for i, _ in T.SMALL_RUNS:
        case = T.CASES[i]
        d, ref = T.case_data(i, xs, ws)
        v = ref["v"] + (ref["r"] if case[8] else 0.0)
        share = T.subnormal_share(v)
        if sub:
            assert share >= 0.25, f"case {i}: {share:.3f} of the results are subnormal halves"
        elif xs * ws < 1e-6:
            assert float(np.abs(v).max()) < 2.0 ** -25, "every stored half is zero: the fp32 head carries the statement"
        else:
            assert float(np.median(np.abs(v[v != 0]))) > 2.0 ** -14
        assert (d["x"] != 0).mean() > 0.9 and (d["w"] != 0).mean() > 0.9, "operands survive their own rounding to halves"
        if xs < 1e-5:
            assert tiny(d["x"].astype(np.float32)) > 0.9
        if ws < 1e-4:
            assert tiny(d["w"]) > 0.9


def test_tie_adjacent_set_is_small():
    """Statement A with a residual admits RN16 of a neighbour of t only where the neighbours round differently: that set must be a
    small minority, or the rule would admit a store that is wrong everywhere."""
    for i in (1, 2, 5, 6, 8):
        case = T.CASES[i]
        d, ref = T.case_data(i)
        y32 = ref["v"].astype(np.float32)
        r16 = ref["r"].astype(np.float16).astype(np.float32)
        want, adjacent, cands = T.residual_candidates(y32, r16)
        assert adjacent.mean() < 0.01, f"case {i}: {adjacent.mean():.4f} of the elements are tie-adjacent"
        assert np.array_equal(want, T.rn16(y32 + r16))
    d, ref = T.case_data(1, 1e-4, 1.0)
    _, adjacent, _ = T.residual_candidates(ref["v"].astype(np.float32), ref["r"].astype(np.float16).astype(np.float32))
    assert adjacent.mean() < 0.01


def test_rn16_is_nearest_even_with_gradual_underflow_and_the_clamp():
    f = lambda *a: np.float32(a)
    assert np.array_equal(T.rn16(f(1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20)), f(1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10))      # ties to even
    assert np.array_equal(T.rn16(f(2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25)), f(2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -23, 2.0 ** -14))
    assert np.array_equal(T.bits(T.rn16(f(-0.0, -2.0 ** -26))), T.bits(f(0.0, 0.0)))
    assert np.array_equal(T.rn16(f(65504.0, 65519.0, 65520.0, 1e5, -1e5, np.inf)), f(65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0))
    assert np.array_equal(P.ulp16(np.float64([1.0, 1.5, 2.0, 2.0 ** -14, 2.0 ** -15, 0.0, 65504.0])), [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0])
    x = T.all_finite_halves()
    assert np.isfinite(x.astype(np.float32)).all() and len(np.unique(x.view(np.uint16))) == 65536 - 2 * 1024


def test_interpreter_halves_satisfy_a_and_b():
    """The graphs of the GPU file through tests/graph_interp (fp16 storage rounding on the CPU): the instrument returns the stored
    halves and the sentinel, and numpy's own halves pass the exact statement and the bound."""
    from tests import graph_interp
    nhwc = lambda t: np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())
    for i in (2, 13):
        case = T.CASES[i]
        cout, act = case[4], case[7]
        d, ref = T.case_data(i)
        x = torch.from_numpy(d["x"].astype(np.float32)).permute(0, 3, 1, 2).contiguous()
        g32, _ = T.build_graph(T.nores(case), d, head="f32")
        y32 = nhwc(graph_interp.run(g32, buf0=x)[g32.head_buf[0]])[..., :cout]
        T.check_bound(f"interpreter case {i}", y32, ref["v"], P.conv16_bound(T.K_of(case), act, ref["v"], ref["S"]), ref["S"])
        g16, _ = T.build_graph(case, d)
        y = nhwc(graph_interp.run(g16, buf0=x)[g16.head_buf[0]])
        assert np.array_equal(y[..., cout:], np.broadcast_to(T.sentinel(y.shape[-1])[cout:], y[..., cout:].shape))
        if case[8]:
            gr, _ = T.build_graph(case, d, head="res")
            r16 = nhwc(graph_interp.run(gr, buf0=x)[gr.head_buf[0]])[..., :cout]
            _, _, cands = T.residual_candidates(y32, r16)
            assert ((y[..., :cout] == cands[0]) | (y[..., :cout] == cands[1]) | (y[..., :cout] == cands[2])).all()
        else:
            assert np.array_equal(T.bits(y[..., :cout]), T.bits(T.rn16(y32)))
