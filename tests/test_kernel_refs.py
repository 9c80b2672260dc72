"""CPU checks of the reference helpers in tests/kernel_refs.py: the GPU
edge-case tests are only as good as these oracles."""

import numpy as np
import pytest

import kernel_refs as kr


def _random_f32_bits(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(
        np.uint32).view(np.float32)


def test_bf16_wire_matches_cpu_codec():
    """bits >> 16 / bits << 16 are byte-equal to the wire codec, NaN
    payloads, Inf, subnormals and low-half 0xFFFF included."""
    from client_amd.utils import deserialize_bf16_tensor, serialize_bf16_tensor

    x = np.concatenate([
        _random_f32_bits(100000, 1),
        np.array([0x7F800000, 0xFF800000, 0x7FC00001, 0x7F80FFFF, 0x0000FFFF,
                  0x80000001, 0x3F80FFFF, 0x00000000, 0x80000000],
                 dtype=np.uint32).view(np.float32)])
    wire = serialize_bf16_tensor(x).item()
    enc = kr.bf16_wire_encode(x)
    assert enc.tobytes() == wire
    back = deserialize_bf16_tensor(wire)
    np.testing.assert_array_equal(kr.bf16_wire_decode(enc).view(np.uint32),
                                  np.asarray(back).reshape(-1).view(np.uint32))


def test_fp8_decode_table_matches_torch():
    torch = pytest.importorskip("torch")
    tab = kr.fp8_e4m3_decode_table()
    assert np.isnan(tab[0x7F]) and np.isnan(tab[0xFF])
    assert np.isnan(tab).sum() == 2
    assert tab[0x7E] == 448.0 and tab[0xFE] == -448.0
    assert tab[0x01] == 2.0 ** -9 and tab[0x08] == 2.0 ** -6
    assert tab[0x00] == 0 and not np.signbit(tab[0x00])
    assert tab[0x80] == 0 and np.signbit(tab[0x80])
    ref = torch.arange(256, dtype=torch.uint8).view(
        torch.float8_e4m3fn).float().numpy().astype(np.float64)
    np.testing.assert_array_equal(tab, ref)
    assert np.all(np.diff(kr.fp8_finite_values()) > 0)


def _torch_fp8(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(
        torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_fp8_encode_agrees_with_torch_up_to_464():
    """Every decoded value, every midpoint, midpoints +-1 fp32 ulp, the
    subnormal and zero edges, and 1e6 random fp32 bit patterns, all with
    |x| <= 464."""
    pytest.importorskip("torch")
    finite, _ = kr.fp8_edge_inputs()
    assert np.all(np.abs(finite) <= kr.FP8_TORCH_FINITE_LIMIT)
    # 127 values + 126 midpoints (+-1 ulp) per sign are all present
    assert len(finite) >= 2 * (127 + 3 * 126)
    np.testing.assert_array_equal(kr.fp8_e4m3_encode(finite),
                                  _torch_fp8(finite))
    rnd = _random_f32_bits(1000000, 2)
    rnd = rnd[np.abs(rnd) <= kr.FP8_TORCH_FINITE_LIMIT]  # drops NaN too
    assert len(rnd) > 400000
    np.testing.assert_array_equal(kr.fp8_e4m3_encode(rnd), _torch_fp8(rnd))
    # random values inside the fp8 range proper (bit patterns are mostly
    # tiny or huge)
    rng = np.random.default_rng(3)
    mid = (rng.standard_normal(200000) * 64).astype(np.float32)
    mid = mid[np.abs(mid) <= kr.FP8_TORCH_FINITE_LIMIT]
    np.testing.assert_array_equal(kr.fp8_e4m3_encode(mid), _torch_fp8(mid))


def test_fp8_encode_round_trips_every_code_and_ties_to_even():
    tab = kr.fp8_e4m3_decode_table()
    codes = np.array([c for c in range(256) if (c & 0x7F) != 0x7F],
                     dtype=np.uint8)
    np.testing.assert_array_equal(
        kr.fp8_e4m3_encode(tab[codes].astype(np.float32)), codes)
    vals = kr.fp8_finite_values()
    mids = ((vals[:-1] + vals[1:]) / 2).astype(np.float32)
    got = kr.fp8_e4m3_encode(mids)
    lo = np.arange(0x7E, dtype=np.uint8)
    np.testing.assert_array_equal(got, np.where(lo % 2 == 0, lo, lo + 1))
    # sign of zero, and of values that round to zero
    z = np.array([0.0, -0.0, 2.0 ** -10, -(2.0 ** -10), 1e-45, -1e-45],
                 dtype=np.float32)
    np.testing.assert_array_equal(kr.fp8_e4m3_encode(z),
                                  [0x00, 0x80, 0x00, 0x80, 0x00, 0x80])


def test_fp8_encode_saturates_where_torch_gives_nan():
    """Above 464 the contract differs from torch only by 0x7E (saturate)
    versus 0x7F (NaN); Inf and NaN give a NaN code in both."""
    pytest.importorskip("torch")
    _, beyond = kr.fp8_edge_inputs()
    rnd = _random_f32_bits(1000000, 4)
    rnd = rnd[~(np.abs(rnd) <= kr.FP8_TORCH_FINITE_LIMIT)]
    x = np.concatenate([beyond, rnd])
    ours = kr.fp8_e4m3_encode(x)
    theirs = _torch_fp8(x)
    finite = np.isfinite(x)
    assert finite.any() and (~finite).any()
    np.testing.assert_array_equal(ours[finite] & 0x7F, 0x7E)
    np.testing.assert_array_equal(theirs & 0x7F, 0x7F)
    np.testing.assert_array_equal(ours[~finite] & 0x7F, 0x7F)
    # signs agree wherever the input is not NaN
    notnan = ~np.isnan(x)
    np.testing.assert_array_equal(ours[notnan] & 0x80, theirs[notnan] & 0x80)


def test_ulp_bf16_and_bound():
    np.testing.assert_array_equal(
        kr.ulp_bf16([1.0, 1.99, 2.0, -3.0, 0.75, 2.0 ** -20, 0.0]),
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8,
         2.0 ** -27, 0.0])
    # the spacing of bf16 numbers around r is ulp_bf16(r)
    bits = np.array([0x3F80, 0x3F81, 0x4000, 0x4001], dtype=np.uint16)
    v = kr.bf16_bits_to_f64(bits)
    assert v[1] - v[0] == kr.ulp_bf16(v[0])
    assert v[3] - v[2] == kr.ulp_bf16(v[2])
    # a correctly rounded value passes with delta = 0, a truncated one
    # (a full ulp below) does not
    r = np.array([[1.0 + 2.0 ** -7 * 0.9]])
    kr.assert_within_bf16_bound(np.array([[0x3F81]], np.uint16), r, 0.0)
    with pytest.raises(AssertionError):
        kr.assert_within_bf16_bound(np.array([[0x3F80]], np.uint16), r, 0.0)


def test_bf16_refs_against_torch_cpu():
    """rmsnorm / rope / GEMM references agree with the obvious torch CPU
    float64 formulas."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)

    def bits(*shape):
        return kr.bf16_wire_encode(
            rng.standard_normal(shape).astype(np.float32)).reshape(shape)

    def t64(b):
        return torch.from_numpy(kr.bf16_bits_to_f64(b))

    xb, wb = bits(3, 64), bits(64)
    r, delta = kr.rmsnorm_ref(xb, wb, 1e-5)
    x, w = t64(xb), t64(wb)
    ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True)
                          + float(np.float32(1e-5))) * w
    np.testing.assert_allclose(r, ref.numpy(), rtol=1e-13)
    np.testing.assert_array_equal(delta, 2.0 ** -18 * np.abs(r))

    b, h, d, seq = 3, 2, 8, 5
    inv = 1.0 / (10000 ** (np.arange(0, d, 2) / d))
    fr = np.outer(np.arange(seq), inv)
    cos, sin = np.cos(fr).astype(np.float32), np.sin(fr).astype(np.float32)
    pos = np.array([0, 4, 2])
    qb = bits(b, h, d)
    r, delta = kr.rope_ref(qb, cos, sin, pos, q_scale=0.5)
    q = kr.bf16_bits_to_f64(qb)
    for i in range(b):
        for j in range(d // 2):
            c, s = float(cos[pos[i], j]), float(sin[pos[i], j])
            x1, x2 = q[i, :, 2 * j], q[i, :, 2 * j + 1]
            np.testing.assert_allclose(r[i, :, 2 * j], (x1 * c - x2 * s) * .5,
                                       rtol=1e-14, atol=0)
            np.testing.assert_allclose(r[i, :, 2 * j + 1],
                                       (x1 * s + x2 * c) * .5, rtol=1e-14,
                                       atol=0)
            np.testing.assert_array_equal(
                delta[i, :, 2 * j], 2.0 ** -21 * (abs(x1) + abs(x2)) * .5)
    # pos = 0 is the identity
    np.testing.assert_array_equal(kr.rope_ref(qb, cos, sin,
                                              np.zeros(b, int))[0], q)

    xb, wb = bits(8, 512), bits(5, 512)
    r, delta = kr.decode_gemm_ref(xb, wb)
    ref = t64(xb) @ t64(wb).t()
    np.testing.assert_allclose(r, ref.numpy(), rtol=1e-12, atol=1e-12)
    assert np.all(delta >= 2.0 ** -17 * np.abs(r))


def test_preprocess_ref_identity_and_scale():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    mean, std = [104.0, 117.0, 123.0], [0.5, 2.0, 0.017]
    for mode in (0, 1, 2):
        ref = kr.preprocess_ref(img, 9, 13, mode, mean, std)
        exact = kr.preprocess_identity_fp32(img, mode, mean, std)
        atol = kr.preprocess_atol(mode, std)
        # fp32 normalize of the exact pixel is far inside the tolerance
        assert np.all(np.abs(exact - ref) <= atol * 1e-3)
    np.testing.assert_allclose(kr.preprocess_atol(0, std).ravel(),
                               [0.01, 0.04, 0.00034])
    np.testing.assert_allclose(kr.preprocess_atol(1, std).ravel(),
                               [0.02 / 127.5] * 3)
    # a constant image stays constant under any resize
    const = np.full((1, 1, 3), 200, dtype=np.uint8)
    np.testing.assert_array_equal(
        kr.preprocess_ref(const, 4, 4, 2, [0, 0, 0], std), 200.0)


def test_cast_range_check_needs_no_gpu():
    """The range check of the two cast entry points runs before any
    device call, so it can be exercised on a handle that owns no
    memory."""
    import client_amd.utils.hip_shared_memory as hipshm

    class Handle:
        _byte_size = 64
        _device_id = 0
        _base_addr = 0

        def _ensure_scratch(self, nbytes):
            raise AssertionError("reached the upload")

    h = Handle()
    x = np.zeros(40, dtype=np.float32)
    for val, wire, off in [(x[:33], "BF16", 0), (x[:32], "BF16", 2),
                           (x[:40], "BF16", -16), (x[:8], "FP8E4M3", 57),
                           (x[:1], "FP8E4M3", -1), (x[:17], "FP32", 0),
                           (x[:1], "INT8", 0)]:
        with pytest.raises(hipshm.CudaSharedMemoryException):
            hipshm.set_shared_memory_region_cast(h, val, wire, offset=off)
    for wire, shape, off in [("BF16", [33], 0), ("BF16", [4, 8], 2),
                             ("BF16", [1], -2), ("FP8E4M3", [65], 0),
                             ("FP32", [16], 4), ("INT8", [1], 0)]:
        with pytest.raises(hipshm.CudaSharedMemoryException):
            hipshm.get_contents_cast(h, wire, shape, offset=off)
    # in range: gets past the check
    with pytest.raises(AssertionError, match="reached the upload"):
        hipshm.set_shared_memory_region_cast(h, x[:32], "BF16")
