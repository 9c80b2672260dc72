"""float64 reference, error bound, fp32 emulation and shared inputs for
the fused GQA decode-attention kernel (numpy only).

Used by tests/test_decode_attention_gpu.py; the bound is checked on the
CPU by tests/test_kv_fp8.py against the fp32 emulation of the kernel's
algorithm. Nothing here touches a GPU.
"""

import numpy as np

import kernel_refs as kr

NAN_BF16 = 0x7FC1  # poison behind every row's own keys
NAN_FP8 = 0x7F

# the shapes the GPU tests run: (b, hq, hk, d)
SHAPES = [(3, 4, 2, 16), (2, 8, 8, 64), (3, 8, 2, 128), (1, 8, 1, 128)]


def cache_len_for(split):
    return 2 * split + 9


def positions_for(split):
    """Row positions the tests draw from: both ends, and each side of
    the first and second split boundary."""
    return [0, 1, split - 1, split, split + 1, 2 * split - 1,
            cache_len_for(split) - 1]


def max_lens_for(split):
    return [split, 2 * split, 2 * split + 8]


def launches_for(b, split):
    """(pos [b], max_len) for seven launches: every position appears in
    every row slot, every max_len is used, and launch 6 pairs the row at
    cache_len - 1 with max_len = split (the inactive-row case: its
    length is clamped to max_len)."""
    p = positions_for(split)
    ml = max_lens_for(split)
    out = []
    for k in range(7):
        pos = np.array([p[(k + 2 * i) % 7] for i in range(b)], dtype=np.int64)
        out.append((pos, ml[k % 3]))
    assert out[6][0][0] == cache_len_for(split) - 1 and out[6][1] == split
    return out


def row_lengths(pos, max_len):
    return np.minimum(np.asarray(pos, dtype=np.int64) + 1, max_len)


def decode_stored(store, kv_fp8):
    """Exact float64 values of stored K/V: bf16 bit patterns (uint16) or
    e4m3 codes (uint8)."""
    if kv_fp8:
        return kr.fp8_e4m3_decode_table()[np.asarray(store, dtype=np.uint8)]
    return kr.bf16_bits_to_f64(store)


def _bf16_bits(values):
    a = np.asarray(values, dtype=np.float32)
    return kr.bf16_wire_encode(a).reshape(a.shape)


def encode_store(values, kv_fp8):
    """float values -> the stored representation (bf16 by truncation,
    e4m3 by the cast contract); the tests' inputs are whatever these
    bits say."""
    a = np.asarray(values, dtype=np.float32)
    if kv_fp8:
        return kr.fp8_e4m3_encode(a).reshape(a.shape)
    return _bf16_bits(a)


def poison(store, pos, max_len, kv_fp8):
    """Copy of store [b, hk, L, d] with a NaN pattern at every key
    position j >= n_i of every row."""
    out = store.copy()
    for i, n in enumerate(row_lengths(pos, max_len)):
        out[i, :, int(n):] = NAN_FP8 if kv_fp8 else NAN_BF16
    return out


def random_case(shape, split, kv_fp8, seed=0):
    """q bits [b, hq, d], K and V stores [b, hk, cache_len, d] without
    poison. q ~ N(0, 1) d^-1/4 and K ~ N(0, 1) d^-1/4 give scores of
    order one."""
    b, hq, hk, d = shape
    rng = np.random.default_rng(seed + 1000 * d + 10 * b + int(kv_fp8))
    L = cache_len_for(split)
    q = _bf16_bits(rng.standard_normal((b, hq, d)) * d ** -0.25)
    k = encode_store(rng.standard_normal((b, hk, L, d)) * d ** -0.25, kv_fp8)
    v = encode_store(rng.standard_normal((b, hk, L, d)), kv_fp8)
    return q, k, v


def decode_attention_ref(q_bits, k_store, v_store, pos, max_len, scale,
                         kv_fp8):
    """float64 reference from the exact stored inputs, and the bound on
    the fp32 arithmetic of the kernel. Returns (r, delta), [b, hq, d].

    Row i, head h (kv head g = h // rep) attends to j < n = n_i:
    s_j = scale * q . k_j, p_j = softmax(s)_j, r = sum_j p_j v_j.

    delta, with x_j = s_j - max_j s_j <= 0 and A = sum_j p_j |v_j|:

      e_s = (d + 2) 2^-24 max_j sum_t |q_t k_jt| scale
          a d-term fp32 dot product in any order and the multiply by
          scale: an absolute error of every score, so at most 2 e_s
          relative on every p_j (numerator and denominator);
      (n + 16) 2^-23 A
          n-term fp32 sums of the numerator and the denominator in any
          order (n 2^-24 each), and a constant for the exp evaluations
          (two per key: within its split and the rescale of the split
          in the combine, ~1 ulp each), the division and the products;
      2^-23 (sum_j p_j |x_j| |v_j| + (sum_j p_j |x_j|) A)
          exp(x) is evaluated as exp2(x log2 e) with the argument
          rounded to fp32: a relative error |x| 2^-24 of exp(x), in the
          numerator and the denominator. The two exponents of a key
          (s_j - m_split and m_split - m) have the same sign and add up
          to x_j, so splitting does not increase it; 2^-23 instead of
          2^-24 covers the rounding of the two subtractions.

    The first two lines are the starting form; the third was missing
    from it and matters for the keys far below the maximum."""
    q = kr.bf16_bits_to_f64(q_bits)
    k = decode_stored(k_store, kv_fp8)
    v = decode_stored(v_store, kv_fp8)
    b, hq, d = q.shape
    hk = k.shape[1]
    rep = hq // hk
    sc = np.float64(np.float32(scale))
    r = np.zeros((b, hq, d))
    delta = np.zeros((b, hq, d))
    for i, n in enumerate(row_lengths(pos, max_len)):
        n = int(n)
        for h in range(hq):
            g = h // rep
            kk = k[i, g, :n]
            vv = v[i, g, :n]
            s = (kk @ q[i, h]) * sc
            x = s - s.max()
            p = np.exp(x)
            p /= p.sum()
            r[i, h] = p @ vv
            e_s = ((d + 2) * 2.0 ** -24
                   * (np.abs(kk) @ np.abs(q[i, h])).max() * abs(sc))
            a = p @ np.abs(vv)
            px = p * np.abs(x)
            delta[i, h] = ((2 * e_s + (n + 16) * 2.0 ** -23) * a
                           + 2.0 ** -23 * (px @ np.abs(vv) + px.sum() * a))
    return r, delta


def _bf16_rne_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (u >> np.uint32(16)).astype(np.uint16)


def emulate_fp32(q_bits, k_store, v_store, pos, max_len, scale, kv_fp8,
                 split):
    """The kernel's algorithm in numpy fp32: per split of `split` keys
    the scores, their max m, p = exp(s - m), l = sum p and acc = p V;
    then the online-softmax merge of the partials in ascending split
    order and one RNE rounding to bf16. Returns bf16 bits [b, hq, d].
    (Summation order inside a split is numpy's, not the kernel's: the
    bound holds for any order.)"""
    f32 = np.float32
    q = kr.bf16_bits_to_f64(q_bits).astype(f32)
    k = decode_stored(k_store, kv_fp8)
    v = decode_stored(v_store, kv_fp8)
    b, hq, d = q.shape
    rep = hq // k.shape[1]
    out = np.zeros((b, hq, d), dtype=f32)
    for i, n in enumerate(row_lengths(pos, max_len)):
        n = int(n)
        for h in range(hq):
            g = h // rep
            m, l, o = f32(-np.inf), f32(0), np.zeros(d, dtype=f32)
            for first in range(0, n, split):
                kk = k[i, g, first:min(n, first + split)].astype(f32)
                vv = v[i, g, first:min(n, first + split)].astype(f32)
                s = (kk @ q[i, h]).astype(f32) * f32(scale)
                ms = s.max()
                p = np.exp(s - ms, dtype=f32)
                ls = p.sum(dtype=f32)
                acc = (p @ vv).astype(f32)
                m_new = max(m, ms)
                c_old = np.exp(f32(m - m_new), dtype=f32)
                c_new = np.exp(f32(ms - m_new), dtype=f32)
                l = f32(l * c_old + ls * c_new)
                o = (o * c_old + acc * c_new).astype(f32)
                m = m_new
            out[i, h] = o / l
    return _bf16_rne_bits(out).reshape(b, hq, d)


def fp8_half_ulp(x):
    """Half the e4m3 spacing at |x| <= 448 (float64): 2^(e - 3) / 2 for
    normals, 2^-10 below 2^-6."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    _, ex = np.frexp(a)
    e = np.where(a < 2.0 ** -6, -6, ex - 1)
    return np.ldexp(0.5, e - 3)


def softmax_edge_cases(split, kv_fp8, shape=(1, 4, 2, 64)):
    """(name, q bits, K store, V store, pos, max_len) for one launch
    each, scale 1:
      equal     q = 0: all scores equal over n = 2 split + 8 keys;
      dominant  scores -198 everywhere but +198 at the last key, which
                lies in the last split (n = 2 split + 5);
      single    n = 1."""
    b, hq, hk, d = shape
    L = cache_len_for(split)
    rng = np.random.default_rng(77 + int(kv_fp8))
    v = encode_store(rng.standard_normal((b, hk, L, d)), kv_fp8)
    k = encode_store(rng.standard_normal((b, hk, L, d)) * d ** -0.25, kv_fp8)
    q = _bf16_bits(rng.standard_normal((b, hq, d)) * d ** -0.25)
    cases = []
    n = 2 * split + 8
    cases.append(("equal", np.zeros_like(q), k, v,
                  np.full(b, n - 1, dtype=np.int64), n))
    n = 2 * split + 5
    qd = np.zeros((b, hq, d), dtype=np.float32)
    qd[..., 0] = 16.5
    kd = np.zeros((b, hk, L, d), dtype=np.float32)
    kd[..., 0] = -12.0
    kd[:, :, n - 1, 0] = 12.0
    cases.append(("dominant", _bf16_bits(qd), encode_store(kd, kv_fp8), v,
                  np.full(b, n - 1, dtype=np.int64), 2 * split + 8))
    cases.append(("single", q, k, v, np.zeros(b, dtype=np.int64), split))
    return cases
