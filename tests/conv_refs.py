"""References for the fused conv kernels (conv1x1.hip, conv3x3.hip),
computed on the CPU from the input bits (numpy; CPU torch in double for
the 3x3 convolution).

Both kernels document one rounding chain: fp32 accumulator -> RNE to
bf16 -> ((t + residual) + bias) in fp32 -> ReLU -> RNE to bf16. Two kinds
of case pin it down:

  exact_case     small integers, so that the accumulator is an exact fp32
                 value in any summation order and the expected output is
                 one bit pattern per element;
  interval_case  random data, where the accumulator lies within
                 delta = n_terms * 2^-24 * S of the float64 sum r and,
                 the chain being monotone, the output lies between the
                 chains of r - delta and r + delta.

Used by tests/test_conv_rounding_gpu.py; checked on the CPU by
tests/test_conv_refs.py. Nothing here touches a GPU.
"""

import numpy as np

import kernel_refs as kr
import weight_fp8_refs as wr

# (N, C, K, H, W) of the 1x1 cases. Exact cases: every shape.
CONV1X1_SHAPES = [
    (3, 96, 64, 7, 7),        # n64s; three chunks; tiles spanning images
    (2, 64, 128, 14, 14),     # n64d; two channel rows
    (2, 96, 64, 4, 6),        # n64v; tiles spanning images; three chunks
    (1, 32, 64, 1, 1),        # one pixel, one chunk
    (2, 2048, 64, 7, 7),      # the longest reduction; exact only
    (40, 32, 2048, 7, 7),     # n128s; 16 tiles x 32 rows = 512 workgroups
    (10, 32, 2048, 14, 14),   # n128d
    (31, 32, 2048, 8, 8),     # n128v; last tile half empty
]
# the interval's ambiguous share grows with C, so the long reduction is
# left to the exact cases, where the interval is a single point
CONV1X1_INTERVAL_SHAPES = [s for s in CONV1X1_SHAPES if s[1] <= 96]
# (N, C, K, H, W, stride) of the 3x3 cases
CONV3X3_SHAPES = [
    (3, 32, 64, 7, 7, 1),      # tiles spanning images
    (2, 32, 128, 9, 5, 1),     # non-square
    (2, 64, 64, 7, 7, 2),      # odd extent, stride 2
    (2, 32, 64, 8, 8, 2),      # even extent, stride 2
    (2, 512, 64, 7, 7, 1),     # the longest reduction (4608); exact only
    (127, 32, 512, 8, 8, 1),   # the smallest shape on the 128-column kernel
]
# C = 32 only: C = 64 already leaves 40 % of the elements ambiguous
CONV3X3_INTERVAL_SHAPES = [s for s in CONV3X3_SHAPES if s[1] == 32]
# (N, C, K, H, W) of the 1x1 NaN/Inf cases: 2-byte and 16-byte stores
CONV1X1_NONFINITE_SHAPES = [(3, 96, 64, 7, 7), (2, 96, 64, 4, 6)]


def case_id(shape):
    return "x".join(map(str, shape))


def n_terms(shape):
    """Reduction length: C for a 1x1 shape, 9 C for a 3x3 one."""
    return shape[1] * (9 if len(shape) == 6 else 1)


def out_shape(shape):
    n, _, k, h, w = shape[:5]
    stride = shape[5] if len(shape) == 6 else 1
    return n, k, (h - 1) // stride + 1, (w - 1) // stride + 1


# ---------------------------------------------------------------------------
# bf16 roundings
# ---------------------------------------------------------------------------


def rne_bf16(v):
    """float32 or float64 values -> bf16 bits, round to nearest even (a
    float64 is first rounded to fp32: the composition is monotone, and
    the identity on the first step for any fp32 value). NaN gives the
    quiet NaN of its sign, as f32_to_bf16_rne in kernels.hip."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.ascontiguousarray(v).astype(np.float32)
    u = f.view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    bits = wr.bf16_rne_bits(np.where(nan, np.float32(0), f))
    quiet = ((u >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16)
    return np.where(nan, quiet, bits).astype(np.uint16)


def trunc_bf16(v):
    """fp32 values -> bf16 bits by truncation: what a kernel that dropped
    the accumulator's low half would give."""
    return kr.bf16_wire_encode(v).reshape(np.shape(v))


def bf16_f32(bits):
    """bf16 bits -> the same values as np.float32, any shape."""
    bits = np.asarray(bits, dtype=np.uint16)
    return kr.bf16_wire_decode(bits).reshape(bits.shape)


# ---------------------------------------------------------------------------
# the operation
# ---------------------------------------------------------------------------


def _conv_f64(x, w, stride, pad):
    """x [N, C, H, W], w [K, C, kh, kw] float64 -> [N, K, OH, OW]."""
    n, c, h, wd = x.shape
    k = w.shape[0]
    if w.shape[2:] == (1, 1):
        assert stride == 1 and pad == 0
        xm = x.reshape(n, c, h * wd)
        wm = w.reshape(k, c)
        # non-finite inputs are taken out of the matrix product (a BLAS
        # may skip a zero operand, and 0 * Inf has to stay NaN) and their
        # columns summed term by term
        bad = ~np.isfinite(xm)
        r = np.matmul(wm[None], np.where(bad, 0.0, xm))
        with np.errstate(invalid="ignore"):
            for i, p in np.argwhere(bad.any(axis=1)):
                r[i, :, p] = (wm * xm[i, None, :, p]).sum(axis=1)
        return r.reshape(n, k, h, wd)
    import torch
    import torch.nn.functional as F

    assert w.shape[2:] == (3, 3)
    return F.conv2d(torch.from_numpy(x), torch.from_numpy(w), stride=stride,
                    padding=pad).numpy()


def conv_ref64(x_bits, w_bits, stride, pad):
    """x_bits [N, C, H, W], w_bits [K, C, kh, kw] bf16 bit patterns, kh =
    kw = 1 (a matrix product over the channels) or 3 (a direct
    convolution in double) -> (r, S) float64 [N, K, OH, OW]: the
    convolution and S = conv(|x|, |w|). S takes non-finite inputs as
    zero, so that it stays a bound for the finite terms."""
    x = kr.bf16_bits_to_f64(x_bits)
    w = kr.bf16_bits_to_f64(w_bits)
    r = _conv_f64(x, w, stride, pad)
    xa = np.where(np.isfinite(x), np.abs(x), 0.0)
    return r, _conv_f64(xa, np.abs(w), stride, pad)


def epilogue_chain(t_bits, res_bits, bias_f32, relu):
    """The kernels' tail after the first rounding, operation by operation
    in fp32: f = f32(t); f += f32(res) when there is a residual; f +=
    bias[k]; ReLU as `if f < 0: f = 0` (so -0.0 and NaN pass, as in
    epilogue_finish); RNE to bf16 bits. t_bits and res_bits [N, K, H, W]
    bf16 bits (res_bits may be None), bias_f32 [K]."""
    bias = np.asarray(bias_f32)
    assert bias.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        f = bf16_f32(t_bits)
        if res_bits is not None:
            f = f + bf16_f32(res_bits)
        f = f + bias.reshape(1, -1, 1, 1)
        assert f.dtype == np.float32
        if relu:
            f = np.where(f < 0, np.float32(0), f)
    return rne_bf16(f)


# ---------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------

EXACT_X_MAX = 8


def exact_w_max(shape):
    """+/-8 integer weights; +/-16 for the one-chunk 1x1 reductions, whose
    sums would otherwise seldom need more than 8 bits."""
    return 16 if n_terms(shape) <= 32 else 8


def _channel_scale(values):
    """Per-channel magnitude of [N, K, H, W] values (never zero)."""
    return np.sqrt((values ** 2).mean(axis=(0, 2, 3))) + 2.0 ** -10


def exact_case(shape, mode, seed=0):
    """A case whose output is determined bit for bit.

    x holds integers in [-8, 8] and w integers in [-w_max, w_max] times
    2^(k % 5 - 2) for output channel k, with max|x| * max|w_int| *
    n_terms < 2^24: every product and every partial sum of a channel is
    an integer multiple of its power of two below 2^24 of them, so the
    fp32 accumulator holds the float64 sum exactly in any summation
    order. Many sums need more than 8 significant bits, so the rounding
    to bf16 in the middle of the chain does real work. The bias is random
    fp32 of both signs at the magnitude of its channel's sums; the
    residual (mode "res") random non-integer bf16 of that magnitude.

    Returns a dict: shape, mode, x_bits, w_bits, w_int, bias, res_bits
    (None in mode "act"), sums (float64, exact), t_bits = RNE(sums), and
    expected = {relu: epilogue_chain(t_bits, ...)}."""
    assert mode in ("act", "res")
    conv3 = len(shape) == 6
    n, c, k, h, w = shape[:5]
    stride, pad, kh = (shape[5], 1, 3) if conv3 else (1, 0, 1)
    rng = np.random.default_rng([seed, int(conv3), int(mode == "res"), *shape])
    wmax = exact_w_max(shape)
    assert EXACT_X_MAX * wmax * n_terms(shape) < 2 ** 24
    xv = rng.integers(-EXACT_X_MAX, EXACT_X_MAX + 1, (n, c, h, w))
    w_int = rng.integers(-wmax, wmax + 1, (k, c, kh, kh))
    wv = w_int * np.ldexp(1.0, np.arange(k) % 5 - 2).reshape(k, 1, 1, 1)
    x_bits = trunc_bf16(xv.astype(np.float32))
    w_bits = trunc_bf16(wv.astype(np.float32))
    # the operands are bf16 values: truncation lost nothing
    assert np.array_equal(kr.bf16_bits_to_f64(x_bits), xv)
    assert np.array_equal(kr.bf16_bits_to_f64(w_bits), wv)
    sums, _ = conv_ref64(x_bits, w_bits, stride, pad)
    sigma = _channel_scale(sums)
    bias = (rng.standard_normal(k) * sigma).astype(np.float32)
    res_bits = None
    if mode == "res":
        res = rng.standard_normal(sums.shape) * sigma.reshape(1, k, 1, 1)
        res_bits = rne_bf16(res)
    t_bits = rne_bf16(sums)
    return {
        "shape": shape, "mode": mode, "stride": stride, "x_bits": x_bits,
        "w_bits": w_bits, "w_int": w_int, "bias": bias,
        "res_bits": res_bits, "sums": sums, "t_bits": t_bits,
        "expected": {relu: epilogue_chain(t_bits, res_bits, bias, relu)
                     for relu in (False, True)},
    }


# ---------------------------------------------------------------------------
# interval cases
# ---------------------------------------------------------------------------


def _le(a_bits, b_bits):
    """a <= b elementwise as floats (bf16 bits in; false on NaN)."""
    with np.errstate(invalid="ignore"):
        return bf16_f32(a_bits) <= bf16_f32(b_bits)


def interval(r, s, terms, res_bits, bias_f32, relu):
    """(lo_bits, hi_bits, share). The kernel's fp32 accumulator a has
    |a - r| <= delta = terms * 2^-24 * S: bf16 x bf16 products are exact
    in fp32, and any summation order of `terms` of them makes at most
    that many roundings, each at most 2^-24 of a partial sum that S
    bounds (the project's worst-case accumulation term). Every step of
    the chain (RNE, adding a constant in fp32, ReLU, RNE) is monotone
    non-decreasing in a, so lo = chain(RNE(r - delta)) <= got <=
    chain(RNE(r + delta)) = hi as floats. share is the fraction of
    elements with lo != hi as floats; elsewhere the check is equality.
    Where the reference is NaN, lo and hi are both NaN."""
    with np.errstate(invalid="ignore"):
        delta = terms * 2.0 ** -24 * s
        lo = epilogue_chain(rne_bf16(r - delta), res_bits, bias_f32, relu)
        hi = epilogue_chain(rne_bf16(r + delta), res_bits, bias_f32, relu)
        lo_f, hi_f = bf16_f32(lo), bf16_f32(hi)
        nan = np.isnan(lo_f)
        assert np.array_equal(nan, np.isnan(hi_f))
        assert np.all(lo_f[~nan] <= hi_f[~nan])
        share = float(np.mean(lo_f[~nan] != hi_f[~nan])) if (~nan).any() else 0.0
    return lo, hi, share


def interval_case(shape, mode, seed=0, specials=False):
    """Random data as the older tests use: x = randn, w = 0.05 randn as
    bf16, bias = randn fp32, residual (mode "res") = randn bf16. With
    `specials` (1x1 shapes) x also holds a NaN, a +Inf, and a +Inf and a
    -Inf that meet in one pixel, and the residual one +Inf. Returns a
    dict: shape, mode, x_bits, w_bits, bias, res_bits, r, s, and lo / hi
    / share = {relu: ...} from `interval`."""
    assert mode in ("act", "res")
    conv3 = len(shape) == 6
    n, c, k, h, w = shape[:5]
    stride, pad, kh = (shape[5], 1, 3) if conv3 else (1, 0, 1)
    rng = np.random.default_rng([seed, int(conv3), int(mode == "res"),
                                 int(specials), *shape])
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    wt = (0.05 * rng.standard_normal((k, c, kh, kh))).astype(np.float32)
    x_bits, w_bits = rne_bf16(x), rne_bf16(wt)
    bias = rng.standard_normal(k).astype(np.float32)
    res_bits = None
    if mode == "res":
        res_bits = rne_bf16(rng.standard_normal(out_shape(shape)))
    if specials:
        assert not conv3 and mode == "res" and c >= 10
        x_bits[0, 1, 0, 0] = 0x7FC0                    # NaN
        x_bits[0, 5, h - 1, w - 1] = 0x7F80            # +Inf
        x_bits[n - 1, 7, h // 2, w // 2] = 0xFF80      # -Inf ...
        x_bits[n - 1, 9, h // 2, w // 2] = 0x7F80      # ... meets +Inf
        res_bits[n // 2, 3, h // 2, 0] = 0x7F80
    r, s = conv_ref64(x_bits, w_bits, stride, pad)
    case = {"shape": shape, "mode": mode, "stride": stride,
            "x_bits": x_bits, "w_bits": w_bits, "bias": bias,
            "res_bits": res_bits, "r": r, "s": s, "lo": {}, "hi": {},
            "share": {}}
    for relu in (False, True):
        case["lo"][relu], case["hi"][relu], case["share"][relu] = interval(
            r, s, n_terms(shape), res_bits, bias, relu)
    return case


def inside(got_bits, lo_bits, hi_bits):
    """Elementwise: lo <= got <= hi as floats, or all three NaN."""
    nan = np.isnan(bf16_f32(lo_bits))
    ok = _le(lo_bits, got_bits) & _le(got_bits, hi_bits)
    return np.where(nan, np.isnan(bf16_f32(got_bits)), ok)
