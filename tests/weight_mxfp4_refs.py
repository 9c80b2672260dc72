"""float64 references and inputs for the MXFP4 weight kernels (numpy
only). A weight is ``codes`` [N, K], one e2m1 code (0..15) per element,
and uint8 ``scales`` [N, K/32]; packing is weight_mxfp4.py's business."""

import numpy as np

import kernel_refs as kr
from weight_fp8_refs import bf16_rne_bits

MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
TABLE = np.concatenate([MAGS, -MAGS])


def w_eff(codes, scales):
    """float64 W_eff [N, K]."""
    s = np.ldexp(1.0, np.asarray(scales, np.int64) - 127)
    return TABLE[codes] * np.repeat(s, 32, axis=1)


def w_eff_bits(codes, scales):
    w = w_eff(codes, scales)
    bits = kr.bf16_wire_encode(w.astype(np.float32)).reshape(w.shape)
    assert np.array_equal(kr.bf16_bits_to_f64(bits), w)  # exactly bf16
    return bits


def gemm_ref(x_bits, codes, scales):
    """(r, delta) [M, N]: delta = (K + 8) 2^-24 sum_k |x W_eff|, the bound
    weight_fp8_refs.fp8w_gemm_ref derives (exact products, K - 1 roundings)."""
    x = kr.bf16_bits_to_f64(x_bits)
    w = w_eff(codes, scales)
    return x @ w.T, (x.shape[1] + 8) * 2.0 ** -24 * (np.abs(x) @ np.abs(w).T)


def random_case(m, n, k, seed=0):
    """x ~ N(0, 1) as bf16, random codes, block exponents in [-8, 4]."""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + seed)
    x_bits = kr.bf16_wire_encode(
        rng.standard_normal((m, k)).astype(np.float32)).reshape(m, k)
    codes = rng.integers(0, 16, (n, k), dtype=np.uint8)
    scales = (127 + rng.integers(-8, 5, (n, k // 32))).astype(np.uint8)
    return x_bits, codes, scales


def exact_case(m, n, k):
    """x in {-1, 0, 1}, integer e2m1 weights, block exponents in {-3..2}:
    every partial sum is a multiple of 2^-3 below 2^13, exact in fp32 in
    any order. Both operands are asymmetric in their indices."""
    mi, ki = np.meshgrid(np.arange(m), np.arange(k), indexing="ij")
    xv = ((2 * mi + 3 * ki + (mi * ki) % 5) % 3 - 1).astype(np.float32)
    ni, kj = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    # magnitude indices 0 and 2, 4..7 are the integers 0, 1, 2, 3, 4, 6
    mag = np.array([0, 2, 4, 5, 6, 7])[(3 * ni + 5 * kj + (ni * kj) % 7) % 6]
    codes = (mag | (((ni + 2 * kj) % 3 == 0) << 3)).astype(np.uint8)
    nb, kb = np.meshgrid(np.arange(n), np.arange(k // 32), indexing="ij")
    scales = (127 + (5 * nb + 7 * kb) % 6 - 3).astype(np.uint8)
    x_bits = kr.bf16_wire_encode(xv).reshape(m, k)
    r = xv.astype(np.float64) @ w_eff(codes, scales).T
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r)
    return x_bits, codes, scales, bf16_rne_bits(r.astype(np.float32))
