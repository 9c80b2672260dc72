"""References for the two DenseNet dense-layer kernels (dense_layer.hip),
computed on the CPU from the input bits with conv_refs' roundings.

Kernel A documents the chain
  a = RNE_bf16(relu(fma32(x, scale, shift)))      (prologue)
  acc = fp32 sum of w * a                          (MFMA)
  t = RNE_bf16(acc)
  out = RNE_bf16(relu?(f32(t) + bias))             (no bias: + -0.0)
and kernel B  out = RNE_bf16(fp32 sum of w * x), the four waves' partial
tiles added in wave order. As in conv_refs there are two kinds of case:
exact ones, whose accumulator is an exact fp32 value in any summation
order, and interval ones on random data.

Used by tests/test_dense_layer_rounding_gpu.py; checked on the CPU by
tests/test_dense_layer_refs.py; the same shapes' addressing is walked by
tests/test_dense_layer_index.py. Nothing here touches a GPU.
"""

import numpy as np

import conv_refs as cr
import kernel_refs as kr

# (N, C, K, H, W, xs) of the kernel A cases: xs is the image stride of x
A_SHAPES = [
    (3, 96, 64, 7, 7, 128 * 49),        # n64s; tiles spanning images
    (2, 64, 128, 14, 14, 96 * 196),     # n64d; two channel rows
    (2, 96, 64, 4, 6, 160 * 24),        # n64v
    (2, 64, 64, 4, 4, 64 * 16 + 1),     # even HW, odd stride: n64s
    (1, 32, 64, 1, 1, 32),              # one pixel, one chunk
    (2, 1024, 64, 7, 7, 1024 * 49),     # the longest reduction; exact only
    (40, 32, 2048, 7, 7, 64 * 49),      # n128s
    (10, 32, 2048, 14, 14, 64 * 196),   # n128d
    (31, 32, 2048, 8, 8, 64 * 64),      # n128v; last tile half empty
    (31, 32, 2048, 8, 8, 64 * 64 + 1),  # odd stride: n128s
]
A_INTERVAL_SHAPES = [s for s in A_SHAPES if s[1] <= 96]
# 2-byte and 16-byte stores
A_NONFINITE_SHAPES = [(3, 96, 64, 7, 7, 128 * 49), (2, 96, 64, 4, 6, 160 * 24)]
# (N, C, H, W, k0, C_buf) of the kernel B cases: the 32 output channels go
# to channels [k0, k0 + 32) of a buffer with C_buf channels, that is with
# image stride C_buf * H * W
B_SHAPES = [
    (3, 160, 7, 7, 32, 96),     # two rounds, waves 1-3 idle in the second
    (2, 256, 9, 5, 0, 32),      # two full rounds
    (96, 32, 8, 20, 0, 32),     # NT=2, R=3: tiles spanning images
    (128, 32, 4, 32, 0, 32),    # NT=2, R=2
    (2, 160, 3, 33, 32, 96),    # NT=2, R=1: 31 padding columns, two rounds
    (1, 64, 3, 64, 0, 32),      # W = 64: the largest LDS footprint
    (80, 32, 7, 7, 0, 32),      # NT=1, R=2
    (1, 32, 1, 1, 0, 32),       # one pixel, all halo
]
B_INTERVAL_SHAPES = [s for s in B_SHAPES if s[1] == 32]
B_K = 32          # output channels of kernel B
B_ROUND = 128     # input channels the four waves take per round

COMBOS = [(b, r) for b in (False, True) for r in (False, True)]


def case_id(shape):
    return "x".join(map(str, shape))


def a_combos(shape):
    """(bias, relu) combinations run on a kernel A shape: all four up to
    K = 128, the served (bias, relu) on the large-K ones."""
    return COMBOS if shape[2] <= 128 else [(True, True)]


# ---------------------------------------------------------------------------
# kernel A's prologue
# ---------------------------------------------------------------------------


def _fma_f32(x_bits, scale_f32, shift_f32):
    """fl32(x * scale + shift) per channel, one rounding, as fmaf. numpy
    has no fma: x * scale is exact in float64 (8 x 24 significant bits);
    the sum is a float64 addition whose TwoSum error term is asserted to
    be zero on every finite element, so it is exact too and the cast to
    fp32 is the only rounding. (The inputs' exponent ranges are bounded
    so that this holds; it is a condition on the case, checked here.)"""
    scale = np.asarray(scale_f32)
    shift = np.asarray(shift_f32)
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    x = kr.bf16_bits_to_f64(x_bits)
    view = (1, -1) + (1,) * (x.ndim - 2)
    with np.errstate(invalid="ignore", over="ignore"):
        p = x * scale.astype(np.float64).reshape(view)
        h = np.broadcast_to(shift.astype(np.float64).reshape(view), p.shape)
        s = p + h
        bb = s - p
        err = (p - (s - bb)) + (h - bb)
        fin = np.isfinite(s)
        assert np.all(err[fin] == 0), "x*scale + shift is not exact in float64"
        return s.astype(np.float32)


def _relu_rne(f):
    """dl_bn_relu's ReLU (`f < 0 ? 0 : f`: NaN and -0.0 pass), then RNE."""
    with np.errstate(invalid="ignore"):
        return cr.rne_bf16(np.where(f < 0, np.float32(0), f))


def prologue_bits(x_bits, scale_f32, shift_f32):
    """a = RNE_bf16(relu(fma32(x, scale, shift))) as bf16 bits; x_bits
    [N, C, ...] bf16 bits, scale and shift [C] float32."""
    return _relu_rne(_fma_f32(x_bits, scale_f32, shift_f32))


def prologue_two_roundings_bits(x_bits, scale_f32, shift_f32, relu=True):
    """The prologue as a separate fp32 multiply and add: what the kernel
    would compute without the fused multiply-add."""
    x = cr.bf16_f32(x_bits)
    view = (1, -1) + (1,) * (x.ndim - 2)
    with np.errstate(invalid="ignore", over="ignore"):
        f = x * np.asarray(scale_f32).reshape(view)
        f = f + np.asarray(shift_f32).reshape(view)
    assert f.dtype == np.float32
    return _relu_rne(f) if relu else cr.rne_bf16(f)


def _a_tail(t_bits, bias, relu, k):
    """After the middle rounding: + bias (or -0.0), ReLU, RNE."""
    b = bias if bias is not None else np.full(k, -0.0, np.float32)
    return cr.epilogue_chain(t_bits, None, b, relu)


# ---------------------------------------------------------------------------
# kernel A, exact
# ---------------------------------------------------------------------------

A_F_MIN, A_F_MAX = 1.0, 8.0     # every f the ReLU keeps: [2^0, 2^3)
A_QUANTUM = 2.0 ** -7           # so every a is a multiple of one bf16 ulp of 1
A_X_STAR = 3.484375             # the directed x, 223 / 64
A_DIRECTED_PIXELS = 32


def _directed_scale_shift(rng):
    """One (scale, shift) for which A_X_STAR tells fmaf from a multiply
    and an add. p = x* scale lies in [4, 8), where fp32 spacing is 2^-21;
    T is a bf16 midpoint in [3.5, 4), where it is 2^-22. With shift = T -
    fl32(p), exact in fp32, the two-step sum is T itself, a tie that goes
    to the even neighbour, while p + shift = T + e with 2^-23 < |e| <=
    2^-22 rounds in fp32 to T +/- 2^-22 and from there to the neighbour
    on e's side. Candidates are drawn until the two are different
    neighbours, and both chains are then evaluated."""
    xb = cr.rne_bf16(np.array([A_X_STAR], np.float32))
    while True:
        scale = np.float32(rng.uniform(1.16, 1.25))
        p = float(A_X_STAR) * float(scale)
        p32 = float(np.float32(p))
        e = p - p32
        if abs(e) <= 2.0 ** -23:
            continue
        k = int(rng.integers(224, 256))       # T = (k + 1/2) 2^-6 in [3.5, 4)
        if (k % 2 == 0) != (e > 0):           # even neighbour opposite to e
            k ^= 1
        shift = np.float32((k + 0.5) * 2.0 ** -6 - p32)
        assert float(shift) == (k + 0.5) * 2.0 ** -6 - p32
        one = prologue_bits(xb.reshape(1, 1), scale.reshape(1),
                            shift.reshape(1))
        two = prologue_two_roundings_bits(xb.reshape(1, 1), scale.reshape(1),
                                          shift.reshape(1))
        if one[0, 0] != two[0, 0]:
            return scale, shift


def a_exact_case(shape, seed=0):
    """A kernel A case whose output is determined bit for bit, with a
    prologue that rounds.

    |x| is non-integer bf16 in [2, 3.5) of either sign, scale full-
    mantissa fp32 in [1, 1.25) and shift fp32 in (-0.9, 0.9): f = fma(x,
    scale, shift) lies in (1.1, 5.3) for a positive x and below -1.1 for
    a negative one, which the ReLU clips (about half the elements). Every
    surviving f is in [1, 8), so every a is a multiple of q = 2^-7 with
    a / q <= 1024, and with conv_refs.exact_case's weights (integers in
    +/-w_max times 2^(k % 5 - 2)) 1024 * w_max * C < 2^24: the fp32
    accumulator holds the exact sum in any order.

    Four channels are directed (_directed_scale_shift): A_X_STAR stands in
    min(32, N*H*W) of their pixels, listed in `directed` as (n, c, h, w)
    rows, and a multiply followed by an add gives another `a` there.

    The data do not depend on xs (shape[5]); the runner lays x out with
    that stride. Returns a dict: shape, x_bits [N,C,H,W], scale, shift,
    w_bits [K,C,1,1], w_int, bias, a_bits, directed, sums (exact), t_bits,
    expected = {(bias, relu): bits}."""
    n, c, k, h, w = shape[:5]
    rng = np.random.default_rng([seed, 11, n, c, k, h, w])
    mag = rng.integers(128, 224, (n, c, h, w)) / 64.0       # [2, 3.5)
    x = mag * rng.choice([-1.0, 1.0], (n, c, h, w))
    scale = rng.uniform(1.0, 1.25, c).astype(np.float32)
    shift = rng.uniform(-0.9, 0.9, c).astype(np.float32)
    pixels = min(A_DIRECTED_PIXELS, n * h * w)
    directed = []
    for ch in rng.choice(c, 4, replace=False):
        scale[ch], shift[ch] = _directed_scale_shift(rng)
        for j in rng.choice(n * h * w, pixels, replace=False):
            i = (j // (h * w), ch, j % (h * w) // w, j % w)
            x[i] = A_X_STAR
            directed.append(i)
    directed = np.array(directed)
    x_bits = cr.trunc_bf16(x.astype(np.float32))
    assert np.array_equal(kr.bf16_bits_to_f64(x_bits), x)
    f = _fma_f32(x_bits, scale, shift)
    kept = f[f >= 0]
    assert kept.min() >= A_F_MIN and kept.max() < A_F_MAX
    a_bits = _relu_rne(f)
    a = kr.bf16_bits_to_f64(a_bits)
    assert np.array_equal(a / A_QUANTUM, np.round(a / A_QUANTUM))
    wmax = cr.exact_w_max(shape[:5])
    assert (a / A_QUANTUM).max() * wmax * c < 2 ** 24
    w_int = rng.integers(-wmax, wmax + 1, (k, c, 1, 1))
    wv = w_int * np.ldexp(1.0, np.arange(k) % 5 - 2).reshape(k, 1, 1, 1)
    w_bits = cr.trunc_bf16(wv.astype(np.float32))
    assert np.array_equal(kr.bf16_bits_to_f64(w_bits), wv)
    sums, _ = cr.conv_ref64(a_bits, w_bits, 1, 0)
    sigma = np.sqrt((sums ** 2).mean(axis=(0, 2, 3))) + 2.0 ** -10
    bias = (rng.standard_normal(k) * sigma).astype(np.float32)
    t_bits = cr.rne_bf16(sums)
    return {
        "shape": shape, "x_bits": x_bits, "scale": scale, "shift": shift,
        "w_bits": w_bits, "w_int": w_int, "bias": bias, "a_bits": a_bits,
        "f": f, "directed": directed, "sums": sums, "t_bits": t_bits,
        "expected": {(hb, relu): _a_tail(t_bits, bias if hb else None, relu,
                                         k) for hb, relu in COMBOS},
    }


# ---------------------------------------------------------------------------
# kernel A, interval
# ---------------------------------------------------------------------------


def a_interval_case(shape, seed=5, specials=False):
    """The random data of tests/test_dense_layer_gpu.py (_a_inputs: x =
    randn bf16, scale in [0.5, 1.5), shift in [-0.5, 0.5), w = 0.05 randn
    bf16, bias = randn). a_bits is the exact prologue, and the interval is
    conv_refs.interval on conv_ref64(a_bits, w_bits) with terms = C.

    With `specials` x also holds a NaN, a +Inf, a -Inf (which the ReLU
    clips to 0: scale is positive) and a +Inf whose channel has a zero
    weight in output channel 2, so that 0 * Inf gives a NaN there and
    +/-Inf in the pixel's other channels.

    Returns a dict: shape, x_bits, scale, shift, w_bits, bias, a_bits, r,
    s, and lo / hi / share = {(bias, relu): ...}."""
    import test_dense_layer_gpu as dg

    n, c, k, h, w = shape[:5]
    buf, scale, shift, wt, bias = dg._a_inputs((n, c, c, k, h, w, True),
                                               seed + int(specials), False)

    def bits(t):
        import torch

        return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()

    x_bits, w_bits = bits(buf), bits(wt)
    scale, shift, bias = scale.numpy(), shift.numpy(), bias.numpy()
    if specials:
        assert c >= 10 and k >= 3 and n * h * w >= 4
        x_bits[0, 1, 0, 0] = 0x7FC0                    # NaN
        x_bits[0, 5, h - 1, w - 1] = 0x7F80            # +Inf
        x_bits[n - 1, 7, h // 2, w // 2] = 0xFF80      # -Inf: clipped
        x_bits[n - 1, 9, 0, w - 1] = 0x7F80            # +Inf ...
        w_bits[2, 9, 0, 0] = 0                         # ... times zero
    a_bits = prologue_bits(x_bits, scale, shift)
    r, s = cr.conv_ref64(a_bits, w_bits, 1, 0)
    case = {"shape": shape, "x_bits": x_bits, "scale": scale, "shift": shift,
            "w_bits": w_bits, "bias": bias, "a_bits": a_bits, "r": r, "s": s,
            "lo": {}, "hi": {}, "share": {}}
    for hb, relu in COMBOS:
        b = bias if hb else np.full(k, -0.0, np.float32)
        case["lo"][hb, relu], case["hi"][hb, relu], case["share"][hb, relu] \
            = cr.interval(r, s, c, None, b, relu)
    return case


# ---------------------------------------------------------------------------
# kernel B
# ---------------------------------------------------------------------------


def _b_w_max(shape):
    """+/-8 integer weights; +/-16 where a pixel has at most 32 terms (a
    1x1 plane sees only the centre tap), whose sums would otherwise
    seldom need more than 8 bits."""
    n, c, h, w = shape[:4]
    return 16 if c * min(h, 3) * min(w, 3) <= 32 else 8


def b_exact_case(shape, seed=0):
    """A kernel B case whose output is one bit pattern per element:
    conv_refs.exact_case's magnitudes (x integers in +/-8, w integers in
    +/-w_max times 2^(k % 5 - 2), 8 * w_max * 9C < 2^24), so the four
    waves' partial tiles and their sum are exact and most sums need more
    than 8 bits. Input channels >= 128, the ones a wave takes in its
    second round, hold |x| and |w|: their partial sum is then far above
    the rounding step of the whole wherever it is not zero, and an
    output that lost it has other bits.

    Returns a dict: shape, x_bits [N,C,H,W], w_bits [32,C,3,3], w_int,
    sums (exact), round1 (the exact sum over channels < 128), expected."""
    n, c, h, w = shape[:4]
    rng = np.random.default_rng([seed, 12, *shape[:4]])
    wmax = _b_w_max(shape)
    assert cr.EXACT_X_MAX * wmax * 9 * c < 2 ** 24
    xv = rng.integers(-cr.EXACT_X_MAX, cr.EXACT_X_MAX + 1, (n, c, h, w))
    w_int = rng.integers(-wmax, wmax + 1, (B_K, c, 3, 3))
    xv[:, B_ROUND:] = np.abs(xv[:, B_ROUND:])
    w_int[:, B_ROUND:] = np.abs(w_int[:, B_ROUND:])
    wv = w_int * np.ldexp(1.0, np.arange(B_K) % 5 - 2).reshape(B_K, 1, 1, 1)
    x_bits = cr.trunc_bf16(xv.astype(np.float32))
    w_bits = cr.trunc_bf16(wv.astype(np.float32))
    assert np.array_equal(kr.bf16_bits_to_f64(x_bits), xv)
    assert np.array_equal(kr.bf16_bits_to_f64(w_bits), wv)
    sums, _ = cr.conv_ref64(x_bits, w_bits, 1, 1)
    round1, _ = cr.conv_ref64(x_bits[:, :B_ROUND], w_bits[:, :B_ROUND], 1, 1)
    return {"shape": shape, "x_bits": x_bits, "w_bits": w_bits,
            "w_int": w_int, "sums": sums, "round1": round1,
            "expected": cr.rne_bf16(sums)}


def b_interval_case(shape, seed=0):
    """Random data shaped like the kernel's own: x = relu(randn) as bf16
    (kernel B reads kernel A's ReLU output) and w = 0.05 (randn + 1). The
    sums then do not cancel to a small multiple of S, which with centred
    data leaves a fifth of the elements ambiguous at C = 32; the cap on
    that share is a condition on the inputs (test_dense_layer_refs.py).
    The accumulation error has terms = 9C + 3: 9C products in a wave's
    MFMA chain, in any order, and the three additions of the partial
    tiles. There is no epilogue: adding -0.0 is the identity.
    Returns a dict: shape, x_bits, w_bits, r, s, lo, hi, share."""
    n, c, h, w = shape[:4]
    rng = np.random.default_rng([seed, 13, *shape[:4]])
    x_bits = cr.rne_bf16(np.maximum(rng.standard_normal((n, c, h, w)), 0.0))
    w_bits = cr.rne_bf16(
        0.05 * (rng.standard_normal((B_K, c, 3, 3)) + 1.0))
    r, s = cr.conv_ref64(x_bits, w_bits, 1, 1)
    lo, hi, share = cr.interval(r, s, 9 * c + 3, None,
                                np.full(B_K, -0.0, np.float32), False)
    return {"shape": shape, "x_bits": x_bits, "w_bits": w_bits, "r": r,
            "s": s, "lo": lo, "hi": hi, "share": share}
