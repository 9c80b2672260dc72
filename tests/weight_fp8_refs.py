"""float64 references for the fp8 (e4m3) weight-only linear kernels
(numpy only; nothing here touches a GPU or torch).

A weight is row-major e4m3 ``codes`` [N, K] and int8 ``scale_exp`` [N];
W_eff[n, k] = decode(codes[n, k]) * 2^scale_exp[n]. The tiled storage
layout is the business of client_amd.models.weight_fp8.pack_codes; the
references work on row-major codes.
"""

import numpy as np

import kernel_refs as kr

_TABLE = kr.fp8_e4m3_decode_table()


def decode_codes(codes):
    return _TABLE[np.asarray(codes, dtype=np.uint8)]


def w_eff(codes, scale_exp):
    """float64 W_eff [N, K]."""
    s = np.ldexp(1.0, np.asarray(scale_exp, dtype=np.int64))
    return decode_codes(codes) * s[:, None]


def bf16_rne_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (u >> np.uint32(16)).astype(np.uint16).reshape(np.shape(x))


def fp8w_gemm_ref(x_bits, codes, scale_exp):
    """x_bits [M, K] bf16 bits, codes [N, K], scale_exp [N] -> (r, delta)
    float64 [M, N].

    r = 2^e_n sum_k x decode(w). delta = (K + 8) 2^-24 2^e_n sum_k
    |x decode(w)|: a bf16 x bf16 product is exact in fp32 (16
    significant bits), and any summation order of K terms has at most
    K - 1 roundings, each at most 2^-24 of a running sum that the sum
    of magnitudes bounds (the depth x 2^-24 form prefill_attention_refs
    uses for its MFMA dot products); the + 8 covers a cross-wave combine
    and the second-order terms. The power-of-two scale is exact. The
    final rounding to bf16 is the ulp/2 of kr.bf16_bound."""
    x = kr.bf16_bits_to_f64(x_bits)
    w = decode_codes(codes)
    s = np.ldexp(1.0, np.asarray(scale_exp, dtype=np.int64))[None, :]
    k = x.shape[1]
    r = (x @ w.T) * s
    delta = (k + 8) * 2.0 ** -24 * s * (np.abs(x) @ np.abs(w).T)
    return r, delta


def emulate_fp32(x_bits, codes, scale_exp, rng):
    """The GEMM in fp32 with the k terms added one by one in a shuffled
    order, scaled and rounded to bf16: bits [M, N]. An independent
    statement of what any fp32-accumulating kernel may produce."""
    x = kr.bf16_bits_to_f64(x_bits).astype(np.float32)
    w = decode_codes(codes).astype(np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for k in rng.permutation(x.shape[1]):
        acc = (acc + x[:, k, None] * w[None, :, k]).astype(np.float32)
    s = np.ldexp(np.float32(1.0), np.asarray(scale_exp, dtype=np.int32))
    return bf16_rne_bits(acc * s[None, :].astype(np.float32))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------


def random_codes(rng, n, k):
    """Random finite e4m3 codes (both zeros, subnormals and +-448 occur)."""
    c = rng.integers(0, 256, (n, k), dtype=np.uint8)
    nan = (c & 0x7F) == 0x7F
    c[nan] = (c[nan] & 0x80) | 0x7E
    return c


def random_case(m, n, k, seed=0):
    """(x_bits [m, k], codes [n, k], scale_exp [n]): x standard normal
    as bf16 (no subnormals: |x| is never that small), scale_exp in
    [-8, 4]."""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + seed)
    x = rng.standard_normal((m, k)).astype(np.float32)
    x_bits = kr.bf16_wire_encode(x).reshape(m, k)
    assert np.all((x_bits & 0x7F80) != 0)
    se = rng.integers(-8, 5, n).astype(np.int8)
    return x_bits, random_codes(rng, n, k), se


# M, N, K: every value of every axis of the issue's product, then the
# shapes at which the kernel takes its other paths: K = 4096 runs one
# unrolled step per wave, 4416 an unrolled step and a single-chunk step
# on some waves; N = 8192 and 16384 select the 8- and 4-wave workgroups,
# with K long enough for their unrolled steps
RANDOM_SHAPES = [
    (1, 1, 64), (7, 15, 128), (8, 16, 576), (9, 17, 1024), (16, 33, 64),
    (1, 100, 1024), (16, 100, 576), (8, 33, 128),
    (8, 48, 4096), (16, 17, 4416), (8, 8192, 2048), (3, 16400, 1024),
]

EXACT_M = (1, 8, 16)
EXACT_N = (16, 48)
EXACT_K = (64, 128)


def exact_integer_case(m, n, k):
    """x in {-1, 0, 1}, decoded weights in {-2, ..., 2}, scale_exp in
    {-3, ..., 2}: every product and partial sum is a small integer, so
    any summation order gives the same fp32 value and the bf16 output is
    determined bit for bit. x is asymmetric in (m, k) and the weights in
    (n, k), so a transposed operand or output map cannot pass. Returns
    (x_bits, codes, scale_exp, expected_bits [m, n], max |sum|)."""
    mi, ki = np.meshgrid(np.arange(m), np.arange(k), indexing="ij")
    xv = ((2 * mi + 3 * ki + (mi * ki) % 5) % 3 - 1).astype(np.float32)
    ni, kj = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    wv = ((3 * ni + 5 * kj + (ni * kj) % 7) % 5 - 2).astype(np.float32)
    se = ((np.arange(n) * 5) % 6 - 3).astype(np.int8)
    x_bits = kr.bf16_wire_encode(xv).reshape(m, k)
    codes = kr.fp8_e4m3_encode(wv).reshape(n, k)
    assert np.array_equal(decode_codes(codes), wv.astype(np.float64))
    sums = xv.astype(np.float64) @ wv.astype(np.float64).T
    r = sums * np.ldexp(1.0, se.astype(np.int64))[None, :]
    r32 = r.astype(np.float32)
    expected = kr.bf16_wire_encode(r32).reshape(m, n)
    # exactly representable: truncation lost nothing
    assert np.array_equal(kr.bf16_bits_to_f64(expected), r)
    return x_bits, codes, se, expected, float(np.abs(sums).max())
