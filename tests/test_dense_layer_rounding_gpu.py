"""The rounding chains of the two DenseNet dense-layer kernels
(dense_layer.hip) on an MI355X against the CPU references of
dense_layer_refs.py:

  A  a = RNE_bf16(relu(fma32(x, scale, shift))), fp32 sum, t =
     RNE_bf16(acc), out = RNE_bf16(relu?(f32(t) + bias))
  B  out = RNE_bf16(fp32 sum), the reduction split over four waves and,
     above 128 input channels, over rounds

Every input is uploaded from CPU bit patterns and every expected value
derives from those bits (tests/test_dense_layer_refs.py checks the
references and that each case tells wrong chains apart;
tests/test_dense_layer_index.py walks the same shapes' addressing and
pins the kernel variant each one reaches). Kernel A reads a flat buffer
with image stride xs that is NaN everywhere outside the channel prefix
it may read; its `out` carries a sentinel tail and a fill no result can
equal. Kernel B writes into a patterned buffer of which every element
outside the slot is compared afterwards. The inputs are compared with
what was uploaded after every call."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import conv_refs as cr  # noqa: E402
import dense_layer_refs as dr  # noqa: E402
import kernel_refs as kr  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 128           # sentinel elements behind out and behind x
OUT_FILL = 0xF1A5   # bf16 -1.6e30: finite, negative, far from any result
X_NAN = 0x7FC0      # x outside the read prefix


@pytest.fixture(scope="module")
def hr():
    from client_amd.ops import gpu_available, hip_runtime

    if not gpu_available():
        pytest.skip("no HIP device")
    return hip_runtime


# the references are computed once and shared; no test changes them
a_exact = functools.lru_cache(maxsize=None)(dr.a_exact_case)
b_exact = functools.lru_cache(maxsize=None)(dr.b_exact_case)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_u16(bits):
    return torch.from_numpy(
        np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda()


def _host_u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _same_f32(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))


def _run_a(hr, case, has_bias, relu, xs=None):
    """One call of kernel A through the launcher, x laid out with image
    stride xs (the shape's own by default). Checks the sentinel tail,
    that every output was overwritten and that no input changed. Returns
    the output bits [N, K, H, W]."""
    from client_amd.models.resnet import pack_conv1x1_weight

    n, c, k, h, w = case["shape"][:5]
    xs = case["shape"][5] if xs is None else xs
    hw = h * w
    assert xs >= c * hw
    flat = np.full(n * xs + PAD, X_NAN, np.uint16)
    for i in range(n):
        flat[i * xs:i * xs + c * hw] = case["x_bits"][i].ravel()
    w_cpu = torch.from_numpy(case["w_bits"].view(np.int16))
    wp_bits = pack_conv1x1_weight(w_cpu).numpy().view(np.uint16)
    x, wp = _dev_u16(flat), _dev_u16(wp_bits)
    scale, shift = _dev_f32(case["scale"]), _dev_f32(case["shift"])
    bias = _dev_f32(case["bias"])
    count = n * k * hw
    out = _dev_u16(np.full(count + PAD, OUT_FILL, np.uint16))
    hr.dense_conv1x1_bf16(x.data_ptr(), xs, scale.data_ptr(),
                          shift.data_ptr(), wp.data_ptr(),
                          bias.data_ptr() if has_bias else 0, out.data_ptr(),
                          n, c, k, h, w, relu, _stream())
    torch.cuda.synchronize()
    got = _host_u16(out)
    assert np.all(got[count:] == OUT_FILL), "wrote past out"
    left = np.flatnonzero(got[:count] == OUT_FILL)
    assert left.size == 0, (
        f"{left.size} outputs not written, first at "
        f"{np.unravel_index(left[0], (n, k, h, w))}")
    assert np.array_equal(_host_u16(x), flat), "x changed"
    assert np.array_equal(_host_u16(wp), wp_bits), "weights changed"
    assert _same_f32(scale, case["scale"]), "scale changed"
    assert _same_f32(shift, case["shift"]), "shift changed"
    assert _same_f32(bias, case["bias"]), "bias changed"
    return got[:count].reshape(n, k, h, w)


def _run_b(hr, case, k0=None, os=None):
    """One call of kernel B into channels [k0, k0 + 32) of a buffer with
    image stride os (the shape's own slot by default). The buffer holds
    a pattern, and OUT_FILL in the slot: checks that every slot element
    was overwritten, that every other element, a tail included, kept its
    bits, and that no input changed. Returns the slot's bits
    [N, 32, H, W]."""
    from client_amd.models.resnet import pack_conv3x3_weight

    n, c, h, w = case["shape"][:4]
    hw = h * w
    k0 = case["shape"][4] if k0 is None else k0
    os = case["shape"][5] * hw if os is None else os
    assert (k0 + dr.B_K) * hw <= os
    before = (np.arange(n * os + PAD) % 251 + 16000).astype(np.uint16)
    slot = np.zeros(before.size, bool)
    for i in range(n):
        slot[i * os + k0 * hw:i * os + (k0 + dr.B_K) * hw] = True
    before[slot] = OUT_FILL
    w_cpu = torch.from_numpy(case["w_bits"].view(np.int16))
    wp_bits = pack_conv3x3_weight(w_cpu).numpy().view(np.uint16)
    x, wp, buf = _dev_u16(case["x_bits"]), _dev_u16(wp_bits), _dev_u16(before)
    hr.dense_conv3x3_k32_bf16(x.data_ptr(), wp.data_ptr(), buf.data_ptr(), n,
                              c, h, w, k0, os, _stream())
    torch.cuda.synchronize()
    got = _host_u16(buf)
    outside = np.flatnonzero((got != before) & ~slot)
    assert outside.size == 0, (
        f"{outside.size} elements outside the slot changed, first at flat "
        f"offset {outside[0]} (image stride {os})")
    got = got[slot].reshape(n, dr.B_K, h, w)
    left = np.argwhere(got == OUT_FILL)
    assert len(left) == 0, (
        f"{len(left)} slot elements not written, first at {tuple(left[0])}")
    assert np.array_equal(_host_u16(x), case["x_bits"]), "x changed"
    assert np.array_equal(_host_u16(wp), wp_bits), "weights changed"
    return got


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def _assert_bits(case, got, want, what):
    assert not np.any(want == OUT_FILL)
    bad = got != want
    if bad.any():
        i = _first(bad)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} elements "
            f"({bad.mean():.4%}) differ; first at (n, k, h, w) = {i}: exact "
            f"sum {case['sums'][i]!r}, got 0x{got[i]:04X}, expected "
            f"0x{want[i]:04X}")


def _assert_inside(case, got, lo, hi, what):
    bad = ~cr.inside(got, lo, hi)
    if bad.any():
        i = _first(bad)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} elements "
            f"({bad.mean():.4%}) outside [lo, hi]; first at (n, k, h, w) = "
            f"{i}: r {case['r'][i]!r}, got 0x{got[i]:04X}, lo 0x{lo[i]:04X}, "
            f"hi 0x{hi[i]:04X}")


@pytest.mark.parametrize("shape", dr.A_SHAPES, ids=dr.case_id)
def test_a_exact_rounding_chain(hr, shape):
    """A prologue that rounds on nearly every kept element and clips half
    of them, directed elements on which fmaf and a multiply-then-add
    part, and an accumulator that is exact in any summation order: the
    output is one bit pattern per element, and it differs from the
    documented chain's wherever the prologue truncated, rounded twice or
    did not clip, the middle rounding was skipped or truncated on either
    store path, or the output was truncated."""
    case = a_exact(shape)
    for has_bias, relu in dr.a_combos(shape):
        got = _run_a(hr, case, has_bias, relu)
        _assert_bits(case, got, case["expected"][has_bias, relu],
                     f"A {dr.case_id(shape)} bias={has_bias} relu={relu}")


@pytest.mark.parametrize("shape", dr.B_SHAPES, ids=dr.case_id)
def test_b_exact(hr, shape):
    """Integer data whose four partial tiles and their sum are exact: one
    bit pattern per element, other bits wherever the sum was truncated or
    a wave's second-round chunk did not reach it."""
    case = b_exact(shape)
    _assert_bits(case, _run_b(hr, case), case["expected"],
                 f"B {dr.case_id(shape)}")


@pytest.mark.parametrize("shape", dr.A_INTERVAL_SHAPES, ids=dr.case_id)
def test_a_inside_interval(hr, shape):
    """Random data: lo <= got <= hi, the chains of the float64 sum over
    the exact prologue values less and plus the worst-case fp32
    accumulation error; bit equality wherever the two agree."""
    case = dr.a_interval_case(shape)
    combos = [(True, True)] + ([(False, False)] if shape[2] <= 128 else [])
    for combo in combos:
        print(f"A {dr.case_id(shape)} bias={combo[0]} relu={combo[1]}: "
              f"ambiguous share {case['share'][combo]:.4%}")
        got = _run_a(hr, case, *combo)
        _assert_inside(case, got, case["lo"][combo], case["hi"][combo],
                       f"A {dr.case_id(shape)} bias={combo[0]} "
                       f"relu={combo[1]}")


@pytest.mark.parametrize("shape", dr.B_INTERVAL_SHAPES, ids=dr.case_id)
def test_b_inside_interval(hr, shape):
    case = dr.b_interval_case(shape)
    print(f"B {dr.case_id(shape)}: ambiguous share {case['share']:.4%}")
    _assert_inside(case, _run_b(hr, case), case["lo"], case["hi"],
                   f"B {dr.case_id(shape)}")


@pytest.mark.parametrize("shape", dr.A_NONFINITE_SHAPES, ids=dr.case_id)
def test_a_nan_inf(hr, shape):
    """A NaN, a +Inf, a -Inf (clipped by the prologue's ReLU) and a +Inf
    under a zero weight in x: NaN exactly where the float64 reference
    over the prologue's values has it, everything else (the infinities
    included) inside the interval. One shape with 2-byte stores, one with
    16-byte stores."""
    case = dr.a_interval_case(shape, specials=True)
    want_nan = np.isnan(case["r"])
    for combo in dr.COMBOS:
        assert np.array_equal(want_nan,
                              np.isnan(cr.bf16_f32(case["lo"][combo])))
        got = _run_a(hr, case, *combo)
        wrong = np.isnan(kr.bf16_bits_to_f64(got)) != want_nan
        assert not wrong.any(), (
            f"bias={combo[0]} relu={combo[1]}: NaN positions differ at "
            f"{int(wrong.sum())} elements, first at (n, k, h, w) = "
            f"{_first(wrong)}")
        _assert_inside(case, got, case["lo"][combo], case["hi"][combo],
                       f"A {dr.case_id(shape)} non-finite bias={combo[0]} "
                       f"relu={combo[1]}")


@pytest.mark.parametrize("shape", [dr.A_SHAPES[0], dr.A_SHAPES[1],
                                   dr.A_SHAPES[2], dr.B_SHAPES[0],
                                   dr.B_SHAPES[2], dr.B_SHAPES[4]],
                         ids=dr.case_id)
def test_stride_and_slot_invariance(hr, shape):
    """The exact case's bits at other layouts. A: x dense (xs = C*HW), an
    even wider stride and an odd one, which takes the 2-byte loads and
    stores whatever HW is. B: another slot of a wider buffer whose image
    stride is no multiple of the plane."""
    if shape in dr.A_SHAPES:
        n, c, k, h, w, _ = shape
        case = a_exact(shape)
        chw = c * h * w
        for xs in (chw, chw + 2 * h * w + 2, chw + 3):
            _assert_bits(case, _run_a(hr, case, True, True, xs=xs),
                         case["expected"][True, True],
                         f"A {dr.case_id(shape)} xs={xs}")
    else:
        n, c, h, w, k0, cb = shape
        case = b_exact(shape)
        for slot, os in ((k0, cb * h * w), (cb, (cb + 32) * h * w + 1)):
            _assert_bits(case, _run_b(hr, case, k0=slot, os=os),
                         case["expected"], f"B {dr.case_id(shape)} k0={slot} "
                         f"os={os}")
