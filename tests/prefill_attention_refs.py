"""float64 reference, error bound, fp32 emulation and shared inputs for
the fused prefill-chunk attention kernel (numpy only).

Used by tests/test_prefill_attention_gpu.py; the bound is checked on the
CPU by tests/test_prefill_attention.py against the emulation of the
kernel's algorithm. Nothing here touches a GPU.

Layouts: q/out [B, C, hq, d] bf16 bits; K/V stores [rows, hk, L, d] bf16
bits or e4m3 codes; pos/lens/row_map [B]. Query c of row i is real when
c < lens[i] and sees the keys j <= min(pos[i] + c, max_len - 1) of
cache row row_map[i].
"""

import functools

import numpy as np

import attention_refs as ar
import kernel_refs as kr

SHAPES = ar.SHAPES  # (B, hq, hk, d)


def cache_len_for(qt, kt):
    return 2 * kt + qt + 12


def chunk_for(qt):
    return qt + 3


def positions_for(qt, kt):
    """Row start positions: the first key tile's start, each side of its
    end, and the start that puts the chunk's last query just past the
    second tile boundary."""
    return [0, 1, kt - 1, kt, kt + 1, 2 * kt - qt - 1]


def lens_for(qt):
    """Real tokens per row: none, one, each side of the query tile and
    the whole chunk."""
    return [0, 1, qt - 1, qt, qt + 1, chunk_for(qt)]


def launches_for(b, qt, kt):
    """(pos [b], lens [b], max_len) for twelve launches: every position
    and every length appears in every row slot, once with the smallest
    multiple of kt that covers the launch and once with 2 kt + qt + 8.
    Every launch has pos + lens <= max_len <= cache_len - 1."""
    p = positions_for(qt, kt)
    ln = lens_for(qt)
    out = []
    for k in range(6):
        pos = np.array([p[(k + i) % 6] for i in range(b)], dtype=np.int64)
        lens = np.array([ln[(k + 2 * i + 1) % 6] for i in range(b)],
                        dtype=np.int64)
        need = int(max((pos + lens).max(), 1))
        for max_len in (-(-need // kt) * kt, 2 * kt + qt + 8):
            assert need <= max_len <= cache_len_for(qt, kt) - 1
            out.append((pos, lens, max_len))
    return out


def row_maps_for(b):
    """(row_map, cache rows): the identity, and a permutation into a
    cache with two rows more than b (rows 0 and b + 1 stay unmapped)."""
    ident = np.arange(b, dtype=np.int64)
    perm = np.array([(b - i) for i in range(b)], dtype=np.int64)
    return [(ident, b), (perm, b + 2)]


def extents(pos, lens, max_len):
    return np.minimum(np.asarray(pos) + np.asarray(lens), max_len)


def poison(store, pos, lens, row_map, max_len, kv_fp8):
    """Copy of store [rows, hk, L, d] with a NaN pattern at every key
    j >= pos[i] + lens[i] of the mapped rows and in every row that is
    not mapped."""
    nan = ar.NAN_FP8 if kv_fp8 else ar.NAN_BF16
    out = np.full_like(store, nan)
    for i, n in enumerate(extents(pos, lens, max_len)):
        out[row_map[i], :, :int(n)] = store[row_map[i], :, :int(n)]
    return out


@functools.lru_cache(maxsize=None)
def random_case(shape, c, cache_len, rows, kv_fp8, seed=0):
    """q bits [B, c, hq, d], K and V stores [rows, hk, cache_len, d]
    without poison; scores of order one (attention_refs.random_case).
    Cached: the CPU and GPU tests share the arrays and leave them
    unchanged."""
    b, hq, hk, d = shape
    rng = np.random.default_rng(seed + 1000 * d + 10 * b + int(kv_fp8)
                                + 7 * rows)
    q = ar._bf16_bits(rng.standard_normal((b, c, hq, d)) * d ** -0.25)
    k = ar.encode_store(
        rng.standard_normal((rows, hk, cache_len, d)) * d ** -0.25, kv_fp8)
    v = ar.encode_store(rng.standard_normal((rows, hk, cache_len, d)),
                        kv_fp8)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def mixed_row_cases(shape, qt, kt, kv_fp8):
    """The launches of the mixed-rows test, CPU and GPU alike: yields
    (q, poisoned K, poisoned V, pos, lens, row_map, max_len, scale).
    All twelve launches through the identity map (scale 0.75), three of
    them again through the permuted map into a larger cache (scale 1)."""
    b = shape[0]
    c, L = chunk_for(qt), cache_len_for(qt, kt)
    for n_map, (row_map, rows) in enumerate(row_maps_for(b)):
        q, k, v = random_case(shape, c, L, rows, kv_fp8)
        for n, (pos, lens, max_len) in enumerate(launches_for(b, qt, kt)):
            if n_map == 1 and n % 4 != 1:
                continue
            yield (q, poison(k, pos, lens, row_map, max_len, kv_fp8),
                   poison(v, pos, lens, row_map, max_len, kv_fp8), pos, lens,
                   row_map, max_len, 0.75 if n_map == 0 else 1.0)


def prefill_attention_ref(q_bits, k_store, v_store, pos, lens, row_map,
                          max_len, scale, kv_fp8):
    """float64 reference from the exact stored inputs and the bound on
    the kernel's arithmetic. Returns (r, delta, real): r and delta
    [B, C, hq, d] (zero where the query is not real), real [B, C] bool.

    For one query with n visible keys the bound is that of
    attention_refs.decode_attention_ref (its three lines, with this n)
    plus 2^-8 A, A = sum_j p_j |v_j|:

      the probabilities are rounded once (RNE) to bf16 as the operand of
      the P V product, a relative error of at most 2^-9 on every term of
      the numerator. The kernel sums the denominator l from the
      UNROUNDED fp32 probabilities, so the denominator takes no such
      error and 2^-9 A of the term is not used by the rounding.

    Unlike the decode kernel (two exp evaluations per key, whatever n),
    the online softmax rescales the accumulators once per later key
    tile: ceil(n / KTILE) - 1 further exp evaluations and multiplies per
    key, each about 2^-22 relative on numerator and denominator alike.
    They are not in decode's constant 16; the unused 2^-9 A above covers
    them for any n below 2^12 KTILE."""
    q = kr.bf16_bits_to_f64(q_bits)
    b, c_len, hq, d = q.shape
    hk = k_store.shape[1]
    rep = hq // hk
    sc = np.float64(np.float32(scale))
    r = np.zeros((b, c_len, hq, d))
    delta = np.zeros((b, c_len, hq, d))
    real = np.zeros((b, c_len), dtype=bool)
    for i in range(b):
        ln = int(min(lens[i], c_len))
        if ln <= 0:
            continue
        real[i, :ln] = True
        p_abs = int(pos[i]) + np.arange(ln)
        n_vis = np.minimum(p_abs, max_len - 1) + 1          # [ln]
        n_max = int(n_vis.max())
        vis = np.arange(n_max)[None, :] < n_vis[:, None]    # [ln, n_max]
        for g in range(hk):
            kk = ar.decode_stored(k_store[row_map[i], g, :n_max], kv_fp8)
            vv = ar.decode_stored(v_store[row_map[i], g, :n_max], kv_fp8)
            for h in range(g * rep, (g + 1) * rep):
                qq = q[i, :ln, h]                           # [ln, d]
                s = np.where(vis, (qq @ kk.T) * sc, -np.inf)
                x = s - s.max(axis=1, keepdims=True)
                p = np.exp(x)
                p /= p.sum(axis=1, keepdims=True)
                r[i, :ln, h] = p @ vv
                dots = np.where(vis, np.abs(qq) @ np.abs(kk).T, 0.0)
                e_s = (d + 2) * 2.0 ** -24 * dots.max(axis=1) * abs(sc)
                a = p @ np.abs(vv)                          # [ln, d]
                px = p * np.where(vis, np.abs(x), 0.0)
                delta[i, :ln, h] = (
                    (2 * e_s + (n_vis + 16) * 2.0 ** -23)[:, None] * a
                    + 2.0 ** -23 * (px @ np.abs(vv)
                                    + px.sum(axis=1, keepdims=True) * a)
                    + 2.0 ** -8 * a)
    return r, delta, real


def _bf16_round_f32(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32."""
    bits = ar._bf16_rne_bits(x).astype(np.uint32) << np.uint32(16)
    return bits.view(np.float32).reshape(np.shape(x))


def emulate_prefill(q_bits, k_store, v_store, pos, lens, row_map, max_len,
                    scale, kv_fp8, ktile):
    """The kernel's algorithm in numpy: fp32 scores, key tiles of
    `ktile` keys from key 0, online rescale of m, l and O, l summed from
    the unrounded probabilities, P rounded RNE to bf16 before P V, one
    RNE rounding to bf16 at the end. Returns bf16 bits [B, C, hq, d],
    zeros where the query is not real. (Summation order inside a tile
    is numpy's: the bound holds for any order.)"""
    f32 = np.float32
    q = kr.bf16_bits_to_f64(q_bits).astype(f32)
    b, c_len, hq, d = q.shape
    hk = k_store.shape[1]
    rep = hq // hk
    out = np.zeros((b, c_len, hq, d), dtype=f32)
    for i in range(b):
        ln = int(min(lens[i], c_len))
        if ln <= 0:
            continue
        last = np.minimum(int(pos[i]) + np.arange(ln), max_len - 1)  # [ln]
        n_max = int(last.max()) + 1
        for g in range(hk):
            kk = ar.decode_stored(k_store[row_map[i], g, :n_max],
                                  kv_fp8).astype(f32)
            vv = ar.decode_stored(v_store[row_map[i], g, :n_max],
                                  kv_fp8).astype(f32)
            for h in range(g * rep, (g + 1) * rep):
                m = np.full(ln, -np.inf, dtype=f32)
                l = np.zeros(ln, dtype=f32)
                o = np.zeros((ln, d), dtype=f32)
                for first in range(0, n_max, ktile):
                    j = np.arange(first, min(n_max, first + ktile))
                    s = (q[i, :ln, h] @ kk[j].T).astype(f32) * f32(scale)
                    s = np.where(j[None, :] <= last[:, None], s,
                                 f32(-np.inf)).astype(f32)
                    m_new = np.maximum(m, s.max(axis=1))
                    alpha = np.exp(m - m_new, dtype=f32)
                    p = np.exp(s - m_new[:, None], dtype=f32)
                    l = (l * alpha + p.sum(axis=1, dtype=f32)).astype(f32)
                    o = (o * alpha[:, None]
                         + (_bf16_round_f32(p) @ vv[j]).astype(f32)
                         ).astype(f32)
                    m = m_new
                out[i, :ln, h] = o / l[:, None]
    return ar._bf16_rne_bits(out).reshape(b, c_len, hq, d)


def softmax_edge_cases(qt, kt, kv_fp8, shape=(1, 4, 2, 64)):
    """(name, q bits, K store, V store, pos, lens, max_len) for one
    launch each, scale 1, identity row_map:
      equal     q = 0: all scores equal, the chunk's queries end in the
                second and third key tile;
      dominant  scores -198 everywhere but +198 at key 2 kt, the first
                key of the last tile of the queries that see it (the
                first two queries of the chunk do not);
      single    pos = 0: query c = 0 sees one key;
      c1        a chunk of one token."""
    b, hq, hk, d = shape
    c = chunk_for(qt)
    L = cache_len_for(qt, kt)
    q, k, v = random_case(shape, c, L, b, kv_fp8, seed=77)
    one = lambda x: np.full(b, x, dtype=np.int64)
    cases = [("equal", np.zeros_like(q), k, v, one(2 * kt - qt - 1), one(c),
              2 * kt + qt + 8)]
    qd = np.zeros((b, c, hq, d), dtype=np.float32)
    qd[..., 0] = 16.5
    kd = np.zeros((b, hk, L, d), dtype=np.float32)
    kd[..., 0] = -12.0
    kd[:, :, 2 * kt, 0] = 12.0
    cases.append(("dominant", ar._bf16_bits(qd), ar.encode_store(kd, kv_fp8),
                  v, one(2 * kt - 2), one(c), 2 * kt + qt + 8))
    cases.append(("single", q, k, v, one(0), one(c), 2 * kt))
    cases.append(("c1", q[:, :1], k, v, one(kt), one(1), 2 * kt))
    return cases
