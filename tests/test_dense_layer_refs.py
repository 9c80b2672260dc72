"""CPU checks of the dense-layer references (tests/dense_layer_refs.py):
the prologue against torch, and that the exact and interval cases of
tests/test_dense_layer_rounding_gpu.py can tell a wrong rounding chain
from the documented one. Each wrong chain a kernel could plausibly run is
emulated here and must change a stated share of an exact case's bits."""

import functools

import numpy as np
import pytest
import torch

import conv_refs as cr
import dense_layer_refs as dr
import kernel_refs as kr

FLOOR = 0.01       # share of elements a wrong chain must change
SHARE_CAP = 0.10   # ambiguous share of an interval case, the project's cap


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def test_prologue_matches_torch_fp32():
    """prologue_bits against torch's fp32 addcmul, relu and cast. torch
    may or may not fuse the multiply-add; its result must be the fma
    chain's or the two-rounding chain's, and the fma chain's wherever the
    two agree (all but a handful of elements, counted)."""
    rng = np.random.default_rng(7)
    shape = (4, 64, 24, 24)
    mag = np.exp2(rng.uniform(-4, 3, shape))
    x_bits = cr.rne_bf16(mag * rng.choice([-1.0, 1.0], shape))
    scale = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    shift = (np.exp2(rng.uniform(-6, 2, 64))
             * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
    got = dr.prologue_bits(x_bits, scale, shift)      # asserts exactness
    two = dr.prologue_two_roundings_bits(x_bits, scale, shift)
    x = torch.from_numpy(cr.bf16_f32(x_bits))
    ref = torch.addcmul(torch.from_numpy(shift).view(1, -1, 1, 1), x,
                        torch.from_numpy(scale).view(1, -1, 1, 1))
    assert ref.dtype == torch.float32
    ref = _bits(torch.relu(ref).to(torch.bfloat16))
    differ = got != two
    print(f"fma and mul-then-add differ on {int(differ.sum())} of "
          f"{differ.size} elements; torch sides with the fma on "
          f"{int((ref[differ] == got[differ]).sum())} of them")
    assert np.array_equal(ref[~differ], got[~differ])
    assert np.all((ref == got) | (ref == two))
    assert differ.sum() < 0.001 * differ.size
    a = cr.bf16_f32(got)
    assert 0.2 < np.mean(a == 0) < 0.8 and not (a < 0).any()


def test_prologue_special_values():
    """NaN stays NaN, -Inf and negatives clip to +0, +Inf stays, -0.0
    passes the ReLU (`f < 0 ? 0 : f`) when the fma gives one (-0 * 1 + -0;
    with shift +0 it gives +0), ties go to even."""
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    x = np.array([0x7FC0, 0x7F80, 0xFF80, 0xBF80, 0x8000, 0x0000, 0x3F80],
                 np.uint16).reshape(1, 1, -1)
    assert dr.prologue_bits(x, one, zero)[0, 0].tolist() == [
        0x7FC0, 0x7F80, 0x0000, 0x0000, 0x0000, 0x0000, 0x3F80]
    assert dr.prologue_bits(x, one, -zero)[0, 0].tolist() == [
        0x7FC0, 0x7F80, 0x0000, 0x0000, 0x8000, 0x0000, 0x3F80]
    # 1 * (1 + 2^-8) + 0 and 1 * (1 + 3 * 2^-8): ties, down and up to even
    for scale, want in ((1.00390625, 0x3F80), (1.01171875, 0x3F82)):
        got = dr.prologue_bits(x[:, :, 6:], np.float32([scale]), zero)
        assert got.tolist() == [[[want]]]
    # the exactness assertion fires when float64 cannot hold the sum
    with pytest.raises(AssertionError):
        dr.prologue_bits(x[:, :, 6:], np.float32([1 + 2.0 ** -23]),
                         np.float32([2.0 ** 40]))


@functools.lru_cache(maxsize=None)
def _a_stats(shape):
    """Per (bias, relu): the share of output elements each wrong chain
    changes, and the numbers that show the case is what it claims."""
    case = dr.a_exact_case(shape)
    k = shape[2]
    f, w_bits, sums = case["f"], case["w_bits"], case["sums"]
    s32 = sums.astype(np.float32)
    relu_f = np.where(f < 0, np.float32(0), f)
    d = tuple(case["directed"].T)
    a_two = dr.prologue_two_roundings_bits(case["x_bits"], case["scale"],
                                           case["shift"])
    wrong_a = {
        "trunc_prologue": cr.trunc_bf16(relu_f),
        "two_roundings": a_two,
        "no_relu": cr.rne_bf16(f),
    }
    wrong_t = {name: cr.rne_bf16(cr.conv_ref64(a, w_bits, 1, 0)[0])
               for name, a in wrong_a.items()}
    wrong_t["trunc_middle"] = cr.trunc_bf16(s32)
    stats = {
        "outputs": sums.size,
        "exact_in_fp32": bool(np.array_equal(s32.astype(np.float64), sums)),
        "clipped": float(np.mean(f < 0)),
        "prologue_inexact": float(np.mean(
            cr.bf16_f32(case["a_bits"]).astype(np.float32) != relu_f)),
        "sums_over_8_bits": float(np.mean(
            kr.bf16_bits_to_f64(case["t_bits"]) != sums)),
        "directed": len(case["directed"]),
        "directed_differ": int((a_two[d] != case["a_bits"][d]).sum()),
        "directed_x": bool(np.all(
            kr.bf16_bits_to_f64(case["x_bits"][d]) == dr.A_X_STAR)),
        "directed_channels": len(set(case["directed"][:, 1].tolist())),
        "x_non_integer": float(np.mean(
            kr.bf16_bits_to_f64(case["x_bits"]) % 1 != 0)),
        "scale_full_mantissa": float(np.mean(
            case["scale"].view(np.uint32) & np.uint32(0xFFFF) != 0)),
        "shift_signs": (bool((case["shift"] > 0).any()),
                        bool((case["shift"] < 0).any())),
        "bias_signs": (bool((case["bias"] > 0).any()),
                       bool((case["bias"] < 0).any())),
        "share": {},
    }
    for hb, relu in dr.a_combos(shape):
        want = case["expected"][hb, relu]
        bias = case["bias"] if hb else None
        share = {name: float(np.mean(dr._a_tail(t, bias, relu, k) != want))
                 for name, t in wrong_t.items()}
        if hb:
            with np.errstate(over="ignore"):
                g = s32 + case["bias"].reshape(1, -1, 1, 1)
                h = cr.bf16_f32(case["t_bits"]) + case["bias"].reshape(
                    1, -1, 1, 1)
            if relu:
                g = np.where(g < 0, np.float32(0), g)
                h = np.where(h < 0, np.float32(0), h)
            share["no_middle_rounding"] = float(np.mean(cr.rne_bf16(g) != want))
            share["trunc_output"] = float(np.mean(cr.trunc_bf16(h) != want))
        stats["share"][hb, relu] = share
        before = cr.bf16_f32(case["expected"][hb, False])
        stats["finite"] = bool(np.isfinite(before).all())
    return stats


@pytest.mark.parametrize("shape", dr.A_SHAPES, ids=dr.case_id)
def test_a_exact_case_is_exact_and_not_vacuous(shape):
    st = _a_stats(shape)
    print(f"A {dr.case_id(shape)}: {st}")
    n, c, k, h, w = shape[:5]
    assert st["outputs"] == n * k * h * w
    assert st["exact_in_fp32"] and st["finite"]
    assert 0.3 < st["clipped"] < 0.7
    assert st["prologue_inexact"] > 0.45      # nearly every kept element
    assert st["sums_over_8_bits"] > 0.5
    assert st["x_non_integer"] > 0.9 and st["scale_full_mantissa"] > 0.9
    assert st["shift_signs"] == (True, True)
    assert st["bias_signs"] == (True, True)
    assert st["directed_channels"] == 4 and st["directed_x"]
    assert st["directed"] == 4 * min(32, n * h * w)
    # (ii): a multiply and an add give another `a` on every directed
    # element, and that reaches the output
    assert st["directed_differ"] == st["directed"]
    for combo, share in st["share"].items():
        assert share.pop("two_roundings") > 0, combo
        # (i), (iii), (iv), (v) and a truncated middle rounding
        assert set(share) == {"trunc_prologue", "no_relu", "trunc_middle"} | (
            {"no_middle_rounding", "trunc_output"} if combo[0] else set())
        for name, value in share.items():
            assert value >= FLOOR, (combo, name, value)


def test_a_exact_case_does_not_depend_on_the_stride():
    a = dr.a_exact_case((31, 32, 2048, 8, 8, 64 * 64))
    b = dr.a_exact_case((31, 32, 2048, 8, 8, 64 * 64 + 1))
    for key in ("x_bits", "scale", "shift", "w_bits", "bias"):
        assert np.array_equal(a[key], b[key])
    for combo in dr.COMBOS:
        assert np.array_equal(a["expected"][combo], b["expected"][combo])


def test_a_expected_without_bias_keeps_signed_zero():
    """No bias is + -0.0: a -0.0 sum stays -0.0 (and passes the ReLU)."""
    t = np.array([0x8000, 0x0000, 0xBF80, 0x3F80], np.uint16).reshape(1, 4, 1, 1)
    assert dr._a_tail(t, None, False, 4).ravel().tolist() == [
        0x8000, 0x0000, 0xBF80, 0x3F80]
    assert dr._a_tail(t, None, True, 4).ravel().tolist() == [
        0x8000, 0x0000, 0x0000, 0x3F80]


@functools.lru_cache(maxsize=None)
def _b_stats(shape):
    case = dr.b_exact_case(shape)
    sums, round1 = case["sums"], case["round1"]
    s32 = sums.astype(np.float32)
    dropped = sums != round1
    lost = cr.rne_bf16(round1) != case["expected"]
    x = kr.bf16_bits_to_f64(case["x_bits"])
    return {
        "outputs": sums.size,
        "product": np.abs(x).max() * np.abs(case["w_int"]).max() * 9 * shape[1],
        "exact_in_fp32": bool(np.array_equal(s32.astype(np.float64), sums)),
        "round1_exact": bool(np.array_equal(
            round1.astype(np.float32).astype(np.float64), round1)),
        "sums_over_8_bits": float(np.mean(
            kr.bf16_bits_to_f64(case["expected"]) != sums)),
        "trunc": float(np.mean(cr.trunc_bf16(s32) != case["expected"])),
        "dropped": float(np.mean(dropped)),
        "dropped_and_same_bits": int((dropped & ~lost).sum()),
        "both_signs": bool((sums > 0).any() and (sums < 0).any()),
    }


@pytest.mark.parametrize("shape", dr.B_SHAPES, ids=dr.case_id)
def test_b_exact_case_is_exact_and_not_vacuous(shape):
    st = _b_stats(shape)
    print(f"B {dr.case_id(shape)}: {st}")
    n, c, h, w = shape[:4]
    assert st["outputs"] == n * dr.B_K * h * w
    assert st["product"] < 2 ** 24
    assert st["exact_in_fp32"] and st["round1_exact"]
    assert st["trunc"] >= FLOOR                                # (vi)
    assert st["sums_over_8_bits"] >= 2 * FLOOR
    if c > dr.B_ROUND:                                         # (vii)
        assert st["dropped"] > 0.99
        assert st["dropped_and_same_bits"] == 0
    else:
        assert st["dropped"] == 0 and st["both_signs"]


@pytest.mark.parametrize("shape", dr.A_INTERVAL_SHAPES, ids=dr.case_id)
def test_a_interval_case_is_mostly_a_single_point(shape):
    case = dr.a_interval_case(shape)
    print(f"A {dr.case_id(shape)}: ambiguous share " + ", ".join(
        f"bias={hb} relu={relu} {case['share'][hb, relu]:.4f}"
        for hb, relu in dr.COMBOS))
    k = shape[2]
    for combo in dr.COMBOS:
        lo, hi = case["lo"][combo], case["hi"][combo]
        assert case["share"][combo] <= SHARE_CAP
        assert np.isfinite(cr.bf16_f32(lo)).all()
        assert cr.inside(lo, lo, hi).all() and cr.inside(hi, lo, hi).all()
    # the prologue does clip, and wrong prologues leave the interval
    assert 0.2 < np.mean(cr.bf16_f32(case["a_bits"]) == 0) < 0.8
    if case["r"].size >= 1000:
        f = dr._fma_f32(case["x_bits"], case["scale"], case["shift"])
        for a in (cr.trunc_bf16(np.where(f < 0, np.float32(0), f)),
                  cr.rne_bf16(f)):
            r = cr.conv_ref64(a, case["w_bits"], 1, 0)[0]
            wrong = dr._a_tail(cr.rne_bf16(r), case["bias"], True, k)
            assert np.mean(~cr.inside(wrong, case["lo"][True, True],
                                      case["hi"][True, True])) > FLOOR


@pytest.mark.parametrize("shape", dr.B_INTERVAL_SHAPES, ids=dr.case_id)
def test_b_interval_case_is_mostly_a_single_point(shape):
    case = dr.b_interval_case(shape)
    print(f"B {dr.case_id(shape)}: ambiguous share {case['share']:.4f}")
    assert case["share"] <= SHARE_CAP
    lo, hi = case["lo"], case["hi"]
    assert np.isfinite(cr.bf16_f32(lo)).all()
    assert cr.inside(lo, lo, hi).all() and cr.inside(hi, lo, hi).all()
    x = cr.bf16_f32(case["x_bits"])
    assert 0.3 < np.mean(x == 0) < 0.7 and not (x < 0).any()
    if case["r"].size >= 1000:
        t = cr.trunc_bf16(case["r"].astype(np.float32))
        assert np.mean(~cr.inside(t, lo, hi)) > FLOOR


@pytest.mark.parametrize("shape", dr.A_NONFINITE_SHAPES, ids=dr.case_id)
def test_a_nonfinite_case_holds_nan_and_inf(shape):
    case = dr.a_interval_case(shape, specials=True)
    n, c, k, h, w = shape[:5]
    a = cr.bf16_f32(case["a_bits"])
    assert np.isnan(a[0, 1, 0, 0]) and a[0, 5, h - 1, w - 1] == np.inf
    assert a[n - 1, 7, h // 2, w // 2] == 0           # -Inf, clipped
    assert a[n - 1, 9, 0, w - 1] == np.inf
    assert (~np.isfinite(a)).sum() == 3
    r = case["r"]
    assert np.isnan(r[0, :, 0, 0]).all()
    assert np.isinf(r[0, :, h - 1, w - 1]).all()
    assert np.isfinite(r[n - 1, :, h // 2, w // 2]).all()
    zero = r[n - 1, :, 0, w - 1]
    assert np.isnan(zero[2]) and np.isinf(np.delete(zero, 2)).all()
    assert np.isnan(r).sum() == k + 1 and np.isinf(r).sum() == 2 * k - 1
    for combo in dr.COMBOS:
        lo = cr.bf16_f32(case["lo"][combo])
        assert np.array_equal(np.isnan(lo), np.isnan(r))
        assert (lo == np.inf).any()
        assert (lo == -np.inf).any() == (not combo[1])
        assert case["share"][combo] <= SHARE_CAP
