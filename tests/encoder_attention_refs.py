"""float64 reference, error bound, fp32 emulation and shared inputs for
the BERT encoder attention kernel (numpy only).

Used by tests/test_encoder_attention_gpu.py; the bound is checked on the
CPU by tests/test_encoder_attention.py against the emulation of the
kernel's algorithm. Nothing here touches a GPU.

Layouts: qkv [B, S, 3, heads, d] bf16 bits (q, k, v of a token side by
side, as the packed in-projection writes them); key_mask [B, S] uint8;
kv_len [B] int32; out [B, S, heads, d]. Query c of row i is real when
c < kv_len[i] and sees the keys j < kv_len[i] with key_mask[i, j] != 0.
"""

import functools

import numpy as np

import attention_refs as ar
import kernel_refs as kr
from prefill_attention_refs import _bf16_round_f32

SHAPES = [(3, 2, 16), (2, 4, 64), (2, 2, 128)]  # (B, heads, d)
PATTERNS = ("ones", "first", "third", "tile")
MASKED_K_FACTOR = 64.0  # a missed mask dominates the softmax


def seq_lens_for(qt, kt, ks):
    """S: one token, one past a query tile, two key tiles and a query
    tile and five, and (keys staged in blocks of ks > kt) one past a
    staged block and a tile."""
    out = [1, qt + 1, 2 * kt + qt + 5]
    if ks > kt:
        out.append(ks + kt + 3)
    return out


def kv_lens_for(s, kt):
    """Keys per row: none, one, each side of the first key tile's end and
    the whole sequence, clipped to S."""
    return [min(v, s) for v in (0, 1, kt - 1, kt, kt + 1, s)]


def launches_for(b, s, kt):
    """kv_len [b] for six launches: every value in every row slot."""
    vals = kv_lens_for(s, kt)
    return [np.array([vals[(k + i) % 6] for i in range(b)], dtype=np.int32)
            for k in range(6)]


def mask_row(pattern, s, n, kt):
    """key_mask row [s] uint8 for a row of n = kv_len keys: zeros from n
    on; inside, the pattern, which always leaves key n - 1 visible (the
    definition of kv_len).
      ones   nothing masked
      first  key 0 masked (left padding)
      third  keys 1, 4, 7, ... masked
      tile   the whole key tile [kt, 2 kt) masked: a softmax tile with
             no visible key after a visible one"""
    m = np.zeros(s, dtype=np.uint8)
    m[:n] = 1
    if pattern == "first":
        m[:1] = 0
    elif pattern == "third":
        m[1:n:3] = 0
    elif pattern == "tile":
        m[kt:min(2 * kt, n)] = 0
    elif pattern != "ones":
        raise ValueError(pattern)
    if n > 0:
        m[n - 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def random_case(shape, s, seed=0):
    """qkv bits [B, s, 3, heads, d] without poison: q and K ~ N(0, 1)
    d^-1/4 (scores of order one, attention_refs.random_case), V ~ N(0, 1).
    Cached: the CPU and GPU tests share the array and leave it unchanged."""
    b, heads, d = shape
    rng = np.random.default_rng(seed + 1000 * d + 10 * b + 7 * s)
    x = rng.standard_normal((b, s, 3, heads, d))
    x[:, :, :2] *= d ** -0.25
    qkv = ar._bf16_bits(x)
    qkv.setflags(write=False)
    return qkv


def poison(qkv, key_mask, kv_len):
    """Copy of qkv with a NaN pattern in every entry of a position
    >= kv_len, and the K entries of masked keys inside kv_len multiplied
    by 64 (exact in bf16, finite)."""
    out = qkv.copy()
    for i, n in enumerate(np.asarray(kv_len)):
        n = int(n)
        out[i, n:] = ar.NAN_BF16
        hidden = np.nonzero(key_mask[i, :n] == 0)[0]
        if hidden.size:
            k = kr.bf16_bits_to_f64(qkv[i, hidden, 1]) * MASKED_K_FACTOR
            out[i, hidden, 1] = ar._bf16_bits(k)
    return out


def masks_for(kv_len, s, kt, first_pattern):
    """key_mask [B, s]: row i takes pattern (first_pattern + i) mod 4."""
    return np.stack([
        mask_row(PATTERNS[(first_pattern + i) % 4], s, int(n), kt)
        for i, n in enumerate(kv_len)])


def cases(shape, qt, kt, ks):
    """The launches of the kernel tests, CPU and GPU alike: yields
    (poisoned qkv, key_mask, kv_len, scale). For every S, every kv_len in
    every row slot with every mask pattern."""
    b, _, d = shape
    for s in seq_lens_for(qt, kt, ks):
        qkv = random_case(shape, s)
        for n_launch, kv_len in enumerate(launches_for(b, s, kt)):
            for p in range(4):
                mask = masks_for(kv_len, s, kt, p)
                yield (poison(qkv, mask, kv_len), mask, kv_len,
                       0.75 if (n_launch + p) % 2 else d ** -0.5)


def encoder_attention_ref(qkv_bits, key_mask, kv_len, scale):
    """float64 reference from the exact bf16 inputs and the bound on the
    kernel's arithmetic. Returns (r, delta, real): r and delta
    [B, S, heads, d] (zero where the query is not real or sees no key),
    real [B, S] bool.

    The bound is the formula of
    prefill_attention_refs.prefill_attention_ref, whose arithmetic the
    kernel keeps (fp32 scores from bf16 products, fp32 m, l and O, tiles
    of KTILE keys from key 0, P rounded RNE to bf16 for the P V product, l
    from the unrounded probabilities): the sums run over the visible
    keys; the operation-count term (n + 16) 2^-23 A uses n = kv_len, the
    keys walked, because a masked key inside kv_len still adds an exact
    zero to both sums and its tile still rescales the accumulators."""
    x = kr.bf16_bits_to_f64(qkv_bits)
    b, s, _, heads, d = x.shape
    sc = np.float64(np.float32(scale))
    r = np.zeros((b, s, heads, d))
    delta = np.zeros((b, s, heads, d))
    real = np.zeros((b, s), dtype=bool)
    for i in range(b):
        n = int(min(max(kv_len[i], 0), s))
        if n == 0:
            continue
        real[i, :n] = True
        vis = key_mask[i, :n] != 0
        if not vis.any():
            continue
        for h in range(heads):
            qq = x[i, :n, 0, h]                              # [n, d]
            kk = x[i, :n, 1, h][vis]
            vv = x[i, :n, 2, h][vis]
            sco = (qq @ kk.T) * sc
            xs = sco - sco.max(axis=1, keepdims=True)
            p = np.exp(xs)
            p /= p.sum(axis=1, keepdims=True)
            r[i, :n, h] = p @ vv
            dots = np.abs(qq) @ np.abs(kk).T
            e_s = (d + 2) * 2.0 ** -24 * dots.max(axis=1) * abs(sc)
            a = p @ np.abs(vv)                               # [n, d]
            px = p * np.abs(xs)
            delta[i, :n, h] = (
                (2 * e_s + (n + 16) * 2.0 ** -23)[:, None] * a
                + 2.0 ** -23 * (px @ np.abs(vv)
                                + px.sum(axis=1, keepdims=True) * a)
                + 2.0 ** -8 * a)
    return r, delta, real


def emulate_encoder(qkv_bits, key_mask, kv_len, scale, ktile):
    """The kernel's algorithm in numpy: fp32 scores, key tiles of `ktile`
    keys from key 0 up to kv_len, masked keys at -inf, online rescale of
    m, l and O, l summed from the unrounded probabilities, P rounded RNE
    to bf16 before P V, one RNE rounding to bf16 at the end. Keys and
    queries at or past kv_len are never read. Returns bf16 bits
    [B, S, heads, d], zeros where the query is not real or sees no key.
    (Summation order inside a tile is numpy's: the bound holds for any
    order.)"""
    f32 = np.float32
    b, s, _, heads, d = qkv_bits.shape
    out = np.zeros((b, s, heads, d), dtype=f32)
    for i in range(b):
        n = int(min(max(kv_len[i], 0), s))
        if n == 0:
            continue
        x = kr.bf16_bits_to_f64(qkv_bits[i, :n]).astype(f32)
        vis = key_mask[i, :n] != 0
        for h in range(heads):
            q, kk, vv = x[:, 0, h], x[:, 1, h], x[:, 2, h]
            m = np.full(n, -np.inf, dtype=f32)
            l = np.zeros(n, dtype=f32)
            o = np.zeros((n, d), dtype=f32)
            for first in range(0, n, ktile):
                j = np.arange(first, min(n, first + ktile))
                sco = (q @ kk[j].T).astype(f32) * f32(scale)
                sco = np.where(vis[j][None, :], sco,
                               f32(-np.inf)).astype(f32)
                m_new = np.maximum(m, sco.max(axis=1))
                m_use = np.where(np.isinf(m_new), f32(0), m_new).astype(f32)
                alpha = np.exp(m - m_use, dtype=f32)
                p = np.exp(sco - m_use[:, None], dtype=f32)
                l = (l * alpha + p.sum(axis=1, dtype=f32)).astype(f32)
                o = (o * alpha[:, None]
                     + (_bf16_round_f32(p) @ vv[j]).astype(f32)).astype(f32)
                m = m_new
            seen = l > 0
            out[i, :n, h][seen] = o[seen] / l[seen, None]
    return ar._bf16_rne_bits(out).reshape(b, s, heads, d)


def softmax_edge_cases(kt, shape=(1, 2, 64)):
    """(name, qkv bits, key_mask, kv_len) for one launch each, scale 1,
    S = 2 kt + 3, nothing masked:
      equal     q = 0: all scores equal;
      dominant  scores -198 everywhere but +198 at key kt, the first key
                of the second tile;
      large     scores 198 and 181.5 alternating: exp of either
                overflows fp32 without the running max."""
    b, heads, d = shape
    s = 2 * kt + 3
    base = random_case(shape, s, seed=77)
    mask = np.ones((b, s), dtype=np.uint8)
    kv_len = np.full(b, s, dtype=np.int32)
    out = []
    eq = base.copy()
    eq[:, :, 0] = 0
    out.append(("equal", eq, mask, kv_len))
    q = np.zeros((b, s, heads, d), dtype=np.float32)
    q[..., 0] = 16.5
    k = np.zeros((b, s, heads, d), dtype=np.float32)
    k[..., 0] = -12.0
    k[:, kt, :, 0] = 12.0
    dom = base.copy()
    dom[:, :, 0] = ar._bf16_bits(q)
    dom[:, :, 1] = ar._bf16_bits(k)
    out.append(("dominant", dom, mask, kv_len))
    k = np.zeros((b, s, heads, d), dtype=np.float32)
    k[:, 0::2, :, 0] = 12.0
    k[:, 1::2, :, 0] = 11.0
    big = base.copy()
    big[:, :, 0] = ar._bf16_bits(q)
    big[:, :, 1] = ar._bf16_bits(k)
    out.append(("large", big, mask, kv_len))
    return out
