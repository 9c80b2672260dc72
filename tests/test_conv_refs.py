"""CPU checks of the conv references (tests/conv_refs.py): the epilogue
chain against the torch reference of the epilogue kernels, and that the
exact and interval cases of tests/test_conv_rounding_gpu.py can tell a
wrong rounding chain from the documented one."""

import functools

import numpy as np
import pytest
import torch

import conv_refs as cr
import epilogue_refs as er
import kernel_refs as kr

EXACT = ([(s, m) for s in cr.CONV1X1_SHAPES for m in ("act", "res")]
         + [(s, "act") for s in cr.CONV3X3_SHAPES])
INTERVAL = ([(s, "res", 0.10) for s in cr.CONV1X1_INTERVAL_SHAPES]
            + [(s, "act", 0.30) for s in cr.CONV3X3_INTERVAL_SHAPES])


def _ids(params):
    return [f"{cr.case_id(p[0])}-{p[1]}" for p in params]


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def test_rne_and_truncation():
    tie = np.float32(1.00390625)  # 1 + 2^-8: half a bf16 ulp above 1
    f = np.array([1.0, tie, 1.01171875, np.nextafter(tie, np.float32(0)),
                  np.nextafter(tie, np.float32(2)), -tie, 3.4e38, np.inf,
                  -np.inf, 0.0, -0.0], dtype=np.float32)
    # ties go to the even neighbour; past bf16 max rounds to Inf
    want = [0x3F80, 0x3F80, 0x3F82, 0x3F80, 0x3F81, 0xBF80, 0x7F80, 0x7F80,
            0xFF80, 0x0000, 0x8000]
    assert cr.rne_bf16(f).tolist() == want
    assert cr.trunc_bf16(f[:6]).tolist() == [0x3F80, 0x3F80, 0x3F81, 0x3F80,
                                             0x3F80, 0xBF80]
    # torch's cast is the same rounding
    g = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(cr.rne_bf16(g),
                          _bits(torch.from_numpy(g).to(torch.bfloat16)))
    # a float64 goes through fp32; NaN stays a quiet NaN of its sign
    assert cr.rne_bf16(np.array([1.0 + 2.0 ** -8 + 2.0 ** -20,
                                 1.0 + 2.0 ** -8 + 2.0 ** -40])).tolist() == [
        0x3F81, 0x3F80]
    nan = np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001],
                   dtype=np.uint32).view(np.float32)
    assert cr.rne_bf16(nan).tolist() == [0x7FC0, 0xFFFF, 0x7FC0]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_epilogue_chain_matches_the_epilogue_reference(with_res, relu):
    """Bit for bit with epilogue_refs.epilogue_ref (CPU torch) on the
    special values and on random data; where the reference is NaN the
    chain is NaN too (which NaN is not pinned)."""
    torch.manual_seed(3)
    rand = (torch.randn(2, 16, 9, 7).to(torch.bfloat16),
            torch.randn(2, 16, 9, 7).to(torch.bfloat16), torch.randn(16))
    for x, res, bias in (er.special_case((1, 16, 12, 12)), rand):
        if not with_res:
            res = None
        ref = er.epilogue_ref(x, res, bias, relu)
        got = cr.epilogue_chain(_bits(x), None if res is None else _bits(res),
                                bias.numpy(), relu)
        nan = torch.isnan(ref).numpy()
        assert np.array_equal(np.isnan(cr.bf16_f32(got)), nan)
        assert (~nan).sum() > nan.sum() > 0 or x is rand[0]
        assert np.array_equal(got[~nan], _bits(ref)[~nan])


def test_conv_ref64_small_cases_by_hand():
    rng = np.random.default_rng(1)
    x = cr.rne_bf16(rng.standard_normal((2, 3, 4, 5)))
    w1 = cr.rne_bf16(rng.standard_normal((4, 3, 1, 1)))
    w3 = cr.rne_bf16(rng.standard_normal((4, 3, 3, 3)))
    xf, w1f, w3f = (kr.bf16_bits_to_f64(a) for a in (x, w1, w3))
    r, s = cr.conv_ref64(x, w1, 1, 0)
    assert np.allclose(r, np.einsum("kc,nchw->nkhw", w1f[:, :, 0, 0], xf),
                       rtol=1e-13, atol=0)
    assert np.allclose(s, np.einsum("kc,nchw->nkhw", np.abs(w1f[:, :, 0, 0]),
                                    np.abs(xf)), rtol=1e-13, atol=0)
    for stride in (1, 2):
        r, s = cr.conv_ref64(x, w3, stride, 1)
        xp = np.pad(xf, ((0, 0), (0, 0), (1, 1), (1, 1)))
        assert r.shape == cr.out_shape((2, 3, 4, 4, 5, stride))
        for (n, k, oh, ow), v in np.ndenumerate(r):
            win = xp[n, :, oh * stride:oh * stride + 3,
                     ow * stride:ow * stride + 3]
            assert abs(v - (win * w3f[k]).sum()) <= 1e-13 * s[n, k, oh, ow]
    # non-finite inputs reach exactly their own pixel, 0 * Inf included
    x[0, 1, 2, 3] = 0x7F80
    w1[2, 1, 0, 0] = 0
    r, s = cr.conv_ref64(x, w1, 1, 0)
    assert np.isfinite(s).all()
    bad = ~np.isfinite(r)
    assert bad.sum() == 4 and bad[0, :, 2, 3].all()
    assert np.isnan(r[0, 2, 2, 3]) and np.isinf(r[0, 0, 2, 3])


@functools.lru_cache(maxsize=None)
def _exact_stats(shape, mode):
    """What the exact-case tests need, reduced to a few numbers (the
    cases themselves are large)."""
    case = cr.exact_case(shape, mode)
    sums = case["sums"]
    s32 = sums.astype(np.float32)
    u = s32.view(np.uint32)
    tie = (u & np.uint32(0xFFFF)) == np.uint32(0x8000)
    odd = ((u >> np.uint32(16)) & np.uint32(1)) == 1
    x = kr.bf16_bits_to_f64(case["x_bits"])
    res = case["res_bits"]
    before = cr.bf16_f32(case["expected"][False])
    after = cr.bf16_f32(case["expected"][True])
    return {
        "outputs": sums.size,
        "product": np.abs(x).max() * np.abs(case["w_int"]).max()
        * cr.n_terms(shape),
        "exact_in_fp32": bool(np.array_equal(s32.astype(np.float64), sums)),
        "t_is_rne": bool(np.array_equal(case["t_bits"], cr.rne_bf16(s32))),
        "rne_not_trunc": float(np.mean(case["t_bits"] != cr.trunc_bf16(s32))),
        "ties_up": int((tie & odd).sum()),
        "ties_down": int((tie & ~odd).sum()),
        "res_non_integer": None if res is None else float(np.mean(
            kr.bf16_bits_to_f64(res) % 1 != 0)),
        "bias_signs": (bool((case["bias"] > 0).any()),
                       bool((case["bias"] < 0).any())),
        "clamped": float(np.mean((before < 0) & (after == 0))),
        "kept": float(np.mean((before > 0) & (after == before))),
        "negative_after_relu": bool((after < 0).any()),
        "non_finite": bool(~np.isfinite(before).all()),
        "channel_scales": bool(np.array_equal(
            kr.bf16_bits_to_f64(case["w_bits"]),
            case["w_int"] * np.ldexp(1.0, np.arange(shape[2]) % 5 - 2)
            .reshape(-1, 1, 1, 1))),
    }


@pytest.mark.parametrize("shape,mode", EXACT, ids=_ids(EXACT))
def test_exact_case_is_exact_and_not_vacuous(shape, mode):
    st = _exact_stats(shape, mode)
    print(f"{cr.case_id(shape)} {mode}: {st}")
    assert st["outputs"] == np.prod(cr.out_shape(shape))
    assert st["product"] < 2 ** 24
    assert st["exact_in_fp32"] and st["t_is_rne"]
    if st["outputs"] >= 1000:
        assert st["rne_not_trunc"] >= 0.01
    assert st["channel_scales"]
    assert st["bias_signs"] == (True, True)
    if mode == "res":
        assert st["res_non_integer"] > 0.05
    assert st["clamped"] > 0.1 and st["kept"] > 0.1
    assert not st["negative_after_relu"] and not st["non_finite"]


def test_exact_cases_hold_ties_in_both_directions():
    up = sum(_exact_stats(s, m)["ties_up"] for s, m in EXACT)
    down = sum(_exact_stats(s, m)["ties_down"] for s, m in EXACT)
    print(f"ties rounding up {up}, down {down}")
    assert up > 0 and down > 0


def test_exact_case_tells_the_mutations_apart():
    """The three wrong chains the GPU test is there to catch, emulated on
    the CPU: each changes output bits of an exact case."""
    case = cr.exact_case((2, 64, 128, 14, 14), "res")
    s32 = case["sums"].astype(np.float32)
    for relu in (False, True):
        want = case["expected"][relu]
        trunc = cr.epilogue_chain(cr.trunc_bf16(s32), case["res_bits"],
                                  case["bias"], relu)
        f = s32 + cr.bf16_f32(case["res_bits"])
        f = f + case["bias"].reshape(1, -1, 1, 1)
        if relu:
            f = np.where(f < 0, np.float32(0), f)
        skipped = cr.rne_bf16(f)
        assert np.mean(trunc != want) > 0.005
        assert np.mean(skipped != want) > 0.005


@pytest.mark.parametrize("shape,mode,cap", INTERVAL, ids=_ids(INTERVAL))
def test_interval_case_is_mostly_a_single_point(shape, mode, cap):
    """The share of elements with lo != hi, from the reference alone, is
    capped: a condition on the inputs, not a tolerance on the kernel."""
    case = cr.interval_case(shape, mode)
    print(f"{cr.case_id(shape)} {mode}: ambiguous share "
          f"{case['share'][False]:.4f} without ReLU, "
          f"{case['share'][True]:.4f} with")
    for relu in (False, True):
        assert case["share"][relu] <= cap
        lo, hi = case["lo"][relu], case["hi"][relu]
        assert np.isfinite(cr.bf16_f32(lo)).all()
        assert cr.inside(lo, lo, hi).all() and cr.inside(hi, lo, hi).all()
    # a truncated first rounding leaves the interval
    t = cr.trunc_bf16(case["r"].astype(np.float32))
    wrong = cr.epilogue_chain(t, case["res_bits"], case["bias"], True)
    if case["r"].size >= 1000:
        assert np.mean(~cr.inside(wrong, case["lo"][True],
                                  case["hi"][True])) > 0.01


@pytest.mark.parametrize("shape", cr.CONV1X1_NONFINITE_SHAPES,
                         ids=cr.case_id)
def test_nonfinite_case_holds_nan_and_both_kinds_of_inf(shape):
    case = cr.interval_case(shape, "res", specials=True)
    n, c, k, h, w = shape
    r = case["r"]
    # the NaN and the first +Inf reach every channel of their own pixel
    assert np.isnan(r[0, :, 0, 0]).all()
    assert np.isinf(r[0, :, h - 1, w - 1]).all()
    # +Inf and -Inf in one pixel: NaN where their weights' signs agree
    pair = r[n - 1, :, h // 2, w // 2]
    assert np.isnan(pair).any() and np.isinf(pair).any()
    assert (~np.isfinite(r)).sum() == 3 * k
    for relu in (False, True):
        lo = cr.bf16_f32(case["lo"][relu])
        nan = np.isnan(lo)
        assert np.array_equal(nan, np.isnan(r))
        assert (lo == np.inf).any()
        assert (lo[n // 2, 3, h // 2, 0] == np.inf)  # from the residual
        assert ((lo == -np.inf).any()) == (not relu)
        assert case["share"][relu] <= 0.10
