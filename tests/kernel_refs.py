"""Plain high-precision references for the HIP kernels (numpy only).

Used by tests/test_kernel_edges_gpu.py; checked on the CPU by
tests/test_kernel_refs.py. Nothing here touches a GPU.
"""

import numpy as np

# ---------------------------------------------------------------------------
# bf16 wire codec (truncation)
# ---------------------------------------------------------------------------


def bf16_wire_encode(x):
    """fp32 -> bf16 wire bytes: keep the high 16 bits of every word."""
    bits = np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)
    return (bits >> np.uint32(16)).astype(np.uint16)


def bf16_wire_decode(u16):
    """bf16 wire words -> fp32: zero-extend the low 16 bits."""
    u16 = np.ascontiguousarray(u16, dtype=np.uint16).reshape(-1)
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_bits_to_f64(u16):
    """Exact float64 value of bf16 bit patterns (any shape)."""
    u16 = np.asarray(u16, dtype=np.uint16)
    return bf16_wire_decode(u16).astype(np.float64).reshape(u16.shape)


# ---------------------------------------------------------------------------
# fp8 e4m3 (OCP "fn": no Inf, NaN = 0x7F / 0xFF, max finite 448)
# ---------------------------------------------------------------------------

FP8_MAX = 448.0
# largest magnitude torch.float8_e4m3fn still rounds to 448 (the midpoint
# between 448 and the absent 480, a tie that goes to the even code 0x7E)
FP8_TORCH_FINITE_LIMIT = 464.0


def fp8_e4m3_decode_table():
    """256 float64 values: normals (-1)^s 2^(e-7) (1+m/8), subnormals
    (-1)^s (m/8) 2^-6 at e = 0, NaN at 0x7F and 0xFF."""
    tab = np.empty(256, dtype=np.float64)
    for code in range(256):
        s = -1.0 if code & 0x80 else 1.0
        e = (code >> 3) & 0xF
        m = code & 0x7
        if (code & 0x7F) == 0x7F:
            tab[code] = np.nan
        elif e == 0:
            tab[code] = s * (m / 8.0) * 2.0 ** -6
        else:
            tab[code] = s * 2.0 ** (e - 7) * (1.0 + m / 8.0)
    return tab


def fp8_e4m3_encode(x):
    """fp32 -> e4m3 codes by the contract the cast kernel is written to:
    round to nearest, ties to the even code; finite results above 448
    saturate to +-448 (0x7E / 0xFE); NaN and +-Inf give the NaN code
    0x7F with the input's sign bit; the sign of zero is preserved."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    sign = ((x.view(np.uint32) >> np.uint32(31)).astype(np.uint8)) << 7
    with np.errstate(invalid="ignore"):  # signalling-NaN inputs
        a = np.abs(x.astype(np.float64))
    nonfinite = ~np.isfinite(a)
    a = np.where(nonfinite, 0.0, np.minimum(a, FP8_MAX))
    _, ex = np.frexp(a)  # a = m * 2^ex, m in [0.5, 1)
    e = np.where(a < 2.0 ** -6, -6, ex - 1)  # subnormals share e = -6
    q = np.rint(np.ldexp(a, 3 - e))  # exact scaling; rint is ties-to-even
    # q in [0, 8] for subnormals, [8, 16] for normals; q = 16 carries into
    # the next exponent, q = 8 at e = -6 is the smallest normal
    code = (q + (e + 6) * 8).astype(np.int64)
    code = np.where(nonfinite, 0x7F, code).astype(np.uint8)
    return code | sign


def fp8_finite_values():
    """The 127 non-negative finite e4m3 values, ascending (codes 0..0x7E)."""
    return fp8_e4m3_decode_table()[:0x7F].copy()


def fp8_edge_inputs():
    """fp32 inputs at every place the encoder can go wrong: all decoded
    values, all midpoints between neighbours and each midpoint +-1 fp32
    ulp, 2^-10 (half the smallest subnormal) and its neighbours, fp32
    subnormals, +-0, the saturation edge and non-finite values. Both
    signs. Returns (finite_le_464, beyond) as fp32 arrays: `beyond`
    holds everything above 464 plus Inf/NaN."""
    vals = fp8_finite_values()
    mids = (vals[:-1] + vals[1:]) / 2.0  # exact in fp32 (<= 6 mantissa bits)
    f32 = np.float32
    inf = f32(np.inf)
    mids32 = mids.astype(f32)
    pts = [vals.astype(f32), mids32,
           np.nextafter(mids32, inf), np.nextafter(mids32, -inf)]
    tiny = f32(2.0 ** -10)
    pts.append(np.array([tiny, np.nextafter(tiny, inf),
                         np.nextafter(tiny, f32(0))], dtype=f32))
    # fp32 subnormals (smallest, a middle one, largest) and the smallest
    # normal
    pts.append(np.array([1, 0x1234, 0x7FFFFF, 0x800000],
                        dtype=np.uint32).view(f32))
    pts.append(np.array([0.0, 448.0, 464.0,
                         np.nextafter(f32(448.0), inf),
                         np.nextafter(f32(464.0), -inf)], dtype=f32))
    pos = np.concatenate(pts)
    finite = np.concatenate([pos, -pos])
    big = np.array([np.nextafter(f32(464.0), inf), 465.0, 480.0, 1e30,
                    np.finfo(f32).max], dtype=f32)
    beyond = np.concatenate([big, -big,
                             np.array([np.inf, -np.inf, np.nan], dtype=f32),
                             np.array([0x7FC00001, 0xFFC00000, 0x7F800001],
                                      dtype=np.uint32).view(f32)])
    return finite, beyond


# ---------------------------------------------------------------------------
# bf16-output kernels with fp32 math: |got - r| <= ulp_bf16(r)/2 + delta
# ---------------------------------------------------------------------------


def ulp_bf16(r):
    """2^(floor(log2|r|) - 7) for r != 0 in the bf16 normal range; 0 at 0."""
    r = np.abs(np.asarray(r, dtype=np.float64))
    _, ex = np.frexp(r)  # |r| = m 2^ex with m in [0.5, 1): floor(log2) = ex-1
    return np.where(r == 0, 0.0, np.ldexp(1.0, ex - 1 - 7))


def bf16_bound(r, delta):
    """Largest accepted |got - r|: the final round-to-nearest-even to
    bf16 (half an ulp of r) plus `delta` for the fp32 arithmetic before
    it."""
    return 0.5 * ulp_bf16(r) + np.asarray(delta, dtype=np.float64)


def rmsnorm_ref(x_bits, w_bits, eps):
    """x_bits [rows, dim], w_bits [dim] bf16 bit patterns -> (r, delta)
    in float64. eps is taken at fp32 precision, as the kernel receives
    it. delta = 2^-18 |r|: a tree sum of <= 4104 positive terms, one
    division, rsqrtf and two multiplies, each <= 2^-24 relative except
    the ~1-ulp rsqrtf; under 2^-20 in total."""
    x = bf16_bits_to_f64(x_bits)
    w = bf16_bits_to_f64(w_bits)
    ms = (x * x).mean(axis=-1, keepdims=True)
    r = x / np.sqrt(ms + np.float64(np.float32(eps))) * w
    return r, 2.0 ** -18 * np.abs(r)


def rope_ref(x_bits, cos, sin, pos, q_scale=1.0):
    """x_bits [b, h, d] bf16 bits; cos/sin [max_seq, d/2] fp32 tables
    (taken as exact); pos [b]. Interleaved pairs (2j, 2j+1). Returns
    (r, delta) float64 [b, h, d]; delta = 2^-21 (|x1|+|x2|) q_scale
    covers two products, one add and one scale in fp32."""
    x = bf16_bits_to_f64(x_bits)
    c = np.asarray(cos, dtype=np.float64)[pos][:, None, :]
    s = np.asarray(sin, dtype=np.float64)[pos][:, None, :]
    qs = np.float64(np.float32(q_scale))
    x1, x2 = x[..., 0::2], x[..., 1::2]
    r = np.empty_like(x)
    r[..., 0::2] = (x1 * c - x2 * s) * qs
    r[..., 1::2] = (x1 * s + x2 * c) * qs
    d = 2.0 ** -21 * (np.abs(x1) + np.abs(x2)) * abs(qs)
    delta = np.empty_like(x)
    delta[..., 0::2] = d
    delta[..., 1::2] = d
    return r, delta


def decode_gemm_ref(x_bits, w_bits):
    """x_bits [8, K], w_bits [N, K] bf16 bits -> (r, delta) float64
    [8, N]; delta = 2^-17 S with S = sum_k |x_k w_k|: the kernel's
    accumulation depth is K/512 + 8 + 6 <= 48 fp32 roundings of 2^-24."""
    x = bf16_bits_to_f64(x_bits)
    w = bf16_bits_to_f64(w_bits)
    r = x @ w.T
    s = np.abs(x) @ np.abs(w).T
    return r, 2.0 ** -17 * s


def assert_within_bf16_bound(got_bits, r, delta, what=""):
    """Per-element check of bf16 output bits against the float64
    reference; reports the worst element."""
    got = bf16_bits_to_f64(got_bits)
    assert got.shape == r.shape, (got.shape, r.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    err = np.abs(got - r)
    bound = bf16_bound(r, delta)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} elements outside the "
            f"bound; worst at {i}: got {got[i]!r}, ref {r[i]!r}, "
            f"err {err[i]:.3e} > bound {bound[i]:.3e}")


# ---------------------------------------------------------------------------
# image preprocess
# ---------------------------------------------------------------------------

PIXEL_ATOL = 0.02  # on the 0..255 pixel scale (fp32 coordinate math)


def preprocess_ref(img, oh, ow, mode, mean, std):
    """float64 pixel-center bilinear resize + normalize, (ih, iw, 3) u8
    -> (3, oh, ow). Modes: 0 (v - mean_c) * std_c, 1 v / 127.5 - 1,
    2 v - mean_c."""
    ih, iw, _ = img.shape
    out = np.empty((3, oh, ow), dtype=np.float64)
    sy, sx = ih / oh, iw / ow
    fy = (np.arange(oh) + 0.5) * sy - 0.5
    fx = (np.arange(ow) + 0.5) * sx - 0.5
    y0 = np.minimum(np.maximum(0, np.floor(fy).astype(int)), ih - 1)
    x0 = np.minimum(np.maximum(0, np.floor(fx).astype(int)), iw - 1)
    y1 = np.minimum(ih - 1, y0 + 1)
    x1 = np.minimum(iw - 1, x0 + 1)
    wy = np.where(fy < 0, 0.0, fy - np.floor(fy))[:, None]
    wx = np.where(fx < 0, 0.0, fx - np.floor(fx))[None, :]
    for c in range(3):
        p = img[:, :, c].astype(np.float64)
        v = ((1 - wy) * ((1 - wx) * p[y0][:, x0] + wx * p[y0][:, x1])
             + wy * ((1 - wx) * p[y1][:, x0] + wx * p[y1][:, x1]))
        if mode == 1:
            v = v / 127.5 - 1.0
        elif mode == 2:
            v = v - mean[c]
        else:
            v = (v - mean[c]) * std[c]
        out[c] = v
    return out


def preprocess_atol(mode, std):
    """Per-channel absolute tolerance [3, 1, 1]: the pixel-scale figure
    times the mode's output scale."""
    if mode == 1:
        scale = np.full(3, 1.0 / 127.5)
    elif mode == 2:
        scale = np.ones(3)
    else:
        scale = np.abs(np.asarray(std, dtype=np.float64))
    return (PIXEL_ATOL * scale).reshape(3, 1, 1)


def preprocess_identity_fp32(img, mode, mean, std):
    """Same-size 'resize': all weights are exactly 0, so the output is
    the fp32 normalize formula on the source pixel, bit for bit."""
    f32 = np.float32
    out = np.empty((3,) + img.shape[:2], dtype=f32)
    for c in range(3):
        v = img[:, :, c].astype(f32)
        if mode == 1:
            v = v / f32(127.5) - f32(1.0)
        elif mode == 2:
            v = v - f32(mean[c])
        else:
            v = (v - f32(mean[c])) * f32(std[c])
        out[c] = v
    return out
