"""Edge-case reference tests for the data-plane kernels: the bf16 / fp8
casts, gather_pack and the image preprocess (require an MI355X).

Every case is the smallest that reaches the branch in question; the
oracles live in tests/kernel_refs.py and are checked on the CPU by
tests/test_kernel_refs.py. The decode-path kernels are covered in
tests/test_decode_edges_gpu.py.
"""

import numpy as np
import pytest

import kernel_refs as kr

pytestmark = pytest.mark.gpu

SMALL_N = (0, 1, 7, 8, 9, 15, 16, 17, 31, 33)
# two full sweeps of the widest cast kernel (2048 blocks x 256 lanes x 16
# elements) plus one vector plus a tail
TWO_SWEEPS_N = 2 * 2048 * 256 * 16 + 16 + 5
# two sweeps of a scalar fallback kernel (one element per lane) plus a tail
SCALAR_TWO_SWEEPS_N = 2 * 2048 * 256 + 5
PAD = 64  # canary bytes after every written range


@pytest.fixture(scope="module")
def hipshm():
    import client_amd.utils.hip_shared_memory as hipshm

    from client_amd.ops import gpu_available

    if not gpu_available():
        pytest.skip("no HIP device")
    return hipshm


@pytest.fixture(scope="module")
def hr(hipshm):
    from client_amd.ops import hip_runtime

    return hip_runtime


def _random_f32_bits(n, seed):
    """fp32 values from random bit patterns: NaN payloads, Inf,
    subnormals and low halves of 0xFFFF all occur."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(
        np.uint32).view(np.float32)


def _periodic(unique, n):
    """n elements repeating `unique` (a period that is no multiple of any
    sweep size, so a read from the wrong sweep shows)."""
    return np.resize(unique, n)


class _Region:
    """A shared-memory region pre-filled with a random byte pattern."""

    def __init__(self, hipshm, size, seed):
        self.hipshm = hipshm
        self.size = size
        self.h = hipshm.create_shared_memory_region("edge", size, 0)
        self.pattern = np.random.default_rng(seed).integers(
            0, 256, size, dtype=np.uint8)
        hipshm.set_shared_memory_region(self.h, [self.pattern])

    def dump(self):
        return self.hipshm.get_contents_as_numpy(self.h, np.uint8,
                                                 [self.size])

    def expect(self, offset, payload):
        """The pattern with `payload` bytes at `offset`."""
        exp = self.pattern.copy()
        b = np.frombuffer(payload.tobytes(), dtype=np.uint8)
        exp[offset:offset + b.size] = b
        return exp

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.hipshm.destroy_shared_memory_region(self.h)


def _assert_bytes_equal(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(
            f"{what}: {bad.size} bytes differ, first at {bad[0]} "
            f"(got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x}), last at "
            f"{bad[-1]} of {got.size}")


def _assert_f32_match_table(got, exp, what):
    """NaN exactly where the table has NaN; bit equality elsewhere (so
    the sign of zero counts)."""
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    exp = np.asarray(exp, dtype=np.float64).reshape(-1)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions"
    assert np.array_equal(got[~nan].view(np.uint32),
                          exp[~nan].astype(np.float32).view(np.uint32)), what


# ---------------------------------------------------------------------------
# bf16 casts
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("offset", [0, 16, 2, 6, 14])
def test_cast_bf16_small_sizes_and_offsets(hipshm, offset):
    """Offsets 0/16 take the vector kernels, 2/6/14 the scalar
    fallbacks, in both directions; bytes outside the written range stay
    untouched."""
    for n in SMALL_N:
        x = _random_f32_bits(n, 100 + n)
        with _Region(hipshm, offset + 2 * n + PAD, n) as reg:
            nbytes = hipshm.set_shared_memory_region_cast(
                reg.h, x, "BF16", offset=offset)
            assert nbytes == 2 * n
            enc = kr.bf16_wire_encode(x)
            _assert_bytes_equal(reg.dump(), reg.expect(offset, enc),
                                f"pack n={n} offset={offset}")
            back = hipshm.get_contents_cast(reg.h, "BF16", [n], offset=offset)
            assert back.dtype == np.float32 and back.shape == (n,)
            assert np.array_equal(back.view(np.uint32),
                                  kr.bf16_wire_decode(enc).view(np.uint32)), (
                f"unpack n={n} offset={offset}")
            _assert_bytes_equal(reg.dump(), reg.expect(offset, enc),
                                f"unpack wrote the region n={n}")


@pytest.mark.parametrize("offset,n", [(0, TWO_SWEEPS_N),
                                      (2, SCALAR_TWO_SWEEPS_N)],
                         ids=["vector", "scalar"])
def test_cast_bf16_more_than_one_sweep(hipshm, offset, n):
    x = _periodic(_random_f32_bits(1000003, 7), n)
    with _Region(hipshm, offset + 2 * n + PAD, 8) as reg:
        hipshm.set_shared_memory_region_cast(reg.h, x, "BF16", offset=offset)
        enc = kr.bf16_wire_encode(x)
        _assert_bytes_equal(reg.dump(), reg.expect(offset, enc), "pack")
        back = hipshm.get_contents_cast(reg.h, "BF16", [n], offset=offset)
        assert np.array_equal(back.view(np.uint32),
                              kr.bf16_wire_decode(enc).view(np.uint32))


# ---------------------------------------------------------------------------
# fp8 e4m3 casts
# ---------------------------------------------------------------------------


def _fp8_inputs():
    finite, beyond = kr.fp8_edge_inputs()
    rng = np.random.default_rng(21)
    x = np.concatenate([
        finite, beyond, _random_f32_bits(4096, 22),
        (rng.standard_normal(4096) * 64).astype(np.float32),
        (rng.standard_normal(1024) * 2.0 ** -7).astype(np.float32)])
    # vector body plus a 5-element tail on the aligned path
    return x[:len(x) - (len(x) - 5) % 8]


def _check_fp8_codes(got, x, what):
    exp = kr.fp8_e4m3_encode(x)
    finite = np.isfinite(x)
    # finite inputs: exact code, saturation and the sign of zero included
    if not np.array_equal(got[finite], exp[finite]):
        bad = np.flatnonzero(got[finite] != exp[finite])
        xs = x[finite][bad]
        sat = np.abs(xs) > kr.FP8_TORCH_FINITE_LIMIT
        zero = (exp[finite][bad] & 0x7F) == 0
        i = bad[0]
        raise AssertionError(
            f"{what}: {bad.size} finite inputs give a wrong code "
            f"({int(sat.sum())} above 464, {int(zero.sum())} with a zero "
            f"result); first x={x[finite][i]!r} "
            f"(bits {x[finite][i:i + 1].view(np.uint32)[0]:#010x}) "
            f"got {got[finite][i]:#04x} expected {exp[finite][i]:#04x}")
    # NaN and +-Inf: a NaN code
    assert np.all(got[~finite] & 0x7F == 0x7F), (
        f"{what}: non-finite inputs", x[~finite], got[~finite])


@pytest.mark.parametrize("offset", [0, 1, 3, 9])
def test_cast_fp8_encode_edges(hipshm, offset):
    """Every code value, every midpoint and its fp32 neighbours, the
    subnormal and zero edges, saturation above 448 and non-finite
    inputs, on the vector path (offset 0) and the scalar path."""
    x = _fp8_inputs()
    n = len(x)
    assert n % 8 == 5
    assert (~np.isfinite(x)).sum() >= 6
    with _Region(hipshm, offset + n + PAD, 23) as reg:
        assert hipshm.set_shared_memory_region_cast(
            reg.h, x, "FP8E4M3", offset=offset) == n
        dump = reg.dump()
        _assert_bytes_equal(dump[:offset], reg.pattern[:offset], "before")
        _assert_bytes_equal(dump[offset + n:], reg.pattern[offset + n:],
                            "after")
        _check_fp8_codes(dump[offset:offset + n], x, f"offset={offset}")


@pytest.mark.parametrize("offset", [0, 1, 3, 9])
def test_cast_fp8_decode_all_codes(hipshm, offset):
    """All 256 codes, repeated to cover the vector body and its tail:
    exact table values, NaN where the table has NaN."""
    tab = kr.fp8_e4m3_decode_table()
    codes = np.resize(np.arange(256, dtype=np.uint8), 3 * 256 + 5)
    with _Region(hipshm, offset + codes.size + PAD, 24) as reg:
        hipshm.set_shared_memory_region(reg.h, [codes], offset=offset)
        got = hipshm.get_contents_cast(reg.h, "FP8E4M3", [codes.size],
                                       offset=offset)
        _assert_f32_match_table(got, tab[codes], f"offset={offset}")
        _assert_bytes_equal(reg.dump(), reg.expect(offset, codes),
                            "decode wrote the region")


@pytest.mark.parametrize("offset", [0, 16, 1, 3, 9])
def test_cast_fp8_small_sizes_and_offsets(hipshm, offset):
    rng = np.random.default_rng(25)
    tab = kr.fp8_e4m3_decode_table()
    for n in SMALL_N:
        x = (rng.standard_normal(n) * 32).astype(np.float32)
        with _Region(hipshm, offset + n + PAD, 26 + n) as reg:
            assert hipshm.set_shared_memory_region_cast(
                reg.h, x, "FP8E4M3", offset=offset) == n
            enc = kr.fp8_e4m3_encode(x)
            _assert_bytes_equal(reg.dump(), reg.expect(offset, enc),
                                f"pack n={n} offset={offset}")
            back = hipshm.get_contents_cast(reg.h, "FP8E4M3", [n],
                                            offset=offset)
            _assert_f32_match_table(back, tab[enc],
                                    f"unpack n={n} offset={offset}")


@pytest.mark.parametrize("offset,n", [(0, TWO_SWEEPS_N),
                                      (1, SCALAR_TWO_SWEEPS_N)],
                         ids=["vector", "scalar"])
def test_cast_fp8_more_than_one_sweep(hipshm, offset, n):
    rng = np.random.default_rng(27)
    unique = np.concatenate([
        _random_f32_bits(500000, 28),
        (rng.standard_normal(500003) * 64).astype(np.float32)])
    x = _periodic(unique, n)
    tab = kr.fp8_e4m3_decode_table()
    with _Region(hipshm, offset + n + PAD, 29) as reg:
        hipshm.set_shared_memory_region_cast(reg.h, x, "FP8E4M3",
                                             offset=offset)
        dump = reg.dump()
        _assert_bytes_equal(dump[:offset], reg.pattern[:offset], "before")
        _assert_bytes_equal(dump[offset + n:], reg.pattern[offset + n:],
                            "after")
        got = dump[offset:offset + n]
        _check_fp8_codes(got[:len(unique)], unique, "first period")
        # the rest repeats the first period exactly
        _assert_bytes_equal(got, _periodic(got[:len(unique)], n), "periods")
        back = hipshm.get_contents_cast(reg.h, "FP8E4M3", [n], offset=offset)
        _assert_f32_match_table(back, tab[got], "unpack")


# ---------------------------------------------------------------------------
# casts called directly with an offset SOURCE (encode) / DESTINATION (decode)
# ---------------------------------------------------------------------------


def _dev_buffer(hr, host_u8):
    ptr = hr.malloc(0, host_u8.size)
    hr.memcpy_h2d(ptr, host_u8, host_u8.size, 0, True)
    return ptr


def _dev_read(hr, ptr, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    hr.memcpy_d2h_into(ptr, out, nbytes, 0)
    return out


@pytest.mark.parametrize("n", [33, SCALAR_TWO_SWEEPS_N])
def test_casts_with_unaligned_other_side(hr, n):
    """The launchers test (src | dst) & 15: an fp32 source at +4 bytes
    (encode) and an fp32 destination at +4 bytes (decode) must select
    the scalar kernels too, and write exactly n elements."""
    rng = np.random.default_rng(31)
    x = _periodic(_random_f32_bits(100003, 32), n)
    tab = kr.fp8_e4m3_decode_table()
    src_host = np.concatenate([np.zeros(4, np.uint8), x.view(np.uint8)])
    src = _dev_buffer(hr, src_host)
    try:
        for name, esz, enc in (("bf16", 2, kr.bf16_wire_encode(x)),
                               ("fp8e4m3", 1, None)):
            pat = rng.integers(0, 256, n * esz + PAD, dtype=np.uint8)
            dst = _dev_buffer(hr, pat)
            try:
                getattr(hr, f"cast_fp32_{name}")(src + 4, dst, n, 0, True, 0)
                got = _dev_read(hr, dst, pat.size)
                _assert_bytes_equal(got[n * esz:], pat[n * esz:],
                                    f"{name} encode canary")
                if enc is None:
                    _check_fp8_codes(got[:n], x, "fp8 encode, source +4")
                else:
                    _assert_bytes_equal(got[:n * esz],
                                        enc.view(np.uint8), "bf16 encode")
                # decode the bytes just written into an fp32 buffer at +4
                wire = got[:n * esz].copy()
                opat = rng.integers(0, 256, 4 + 4 * n + PAD, dtype=np.uint8)
                out = _dev_buffer(hr, opat)
                try:
                    getattr(hr, f"cast_{name}_fp32")(dst, out + 4, n, 0,
                                                     True, 0)
                    o = _dev_read(hr, out, opat.size)
                    _assert_bytes_equal(o[:4], opat[:4], "decode before")
                    _assert_bytes_equal(o[4 + 4 * n:], opat[4 + 4 * n:],
                                        "decode after")
                    f = o[4:4 + 4 * n].copy().view(np.float32)
                    if esz == 2:
                        assert np.array_equal(
                            f.view(np.uint32),
                            kr.bf16_wire_decode(wire.view(np.uint16)).view(
                                np.uint32))
                    else:
                        _assert_f32_match_table(f, tab[wire], "fp8 decode")
                finally:
                    hr.free(out)
            finally:
                hr.free(dst)
    finally:
        hr.free(src)


# ---------------------------------------------------------------------------
# range checks of the two cast entry points
# ---------------------------------------------------------------------------


def test_cast_range_checks(hipshm):
    """offset + nbytes beyond the region, or a negative offset, raise in
    both functions before anything is uploaded or launched."""
    exc = hipshm.CudaSharedMemoryException
    x = np.arange(40, dtype=np.float32)
    with _Region(hipshm, 64, 41) as reg:
        bad_sets = [
            (x[:33], "BF16", 0),     # 66 bytes into 64
            (x[:32], "BF16", 2),     # fits only at offset 0
            (x[:1], "BF16", 63),
            (x[:1], "BF16", -2),
            (x[:40], "BF16", -16),   # would fit if the offset were ignored
            (np.zeros(65, np.float32), "FP8E4M3", 0),
            (x[:8], "FP8E4M3", 57),
            (x[:8], "FP8E4M3", -1),
            (x[:17], "FP32", 0),
            (x[:1], "FP32", 64),
        ]
        for val, wire, off in bad_sets:
            with pytest.raises(exc):
                hipshm.set_shared_memory_region_cast(reg.h, val, wire,
                                                     offset=off)
        bad_gets = [("BF16", [33], 0), ("BF16", [4, 8], 2), ("BF16", [1], -2),
                    ("FP8E4M3", [65], 0), ("FP8E4M3", [8], 57),
                    ("FP8E4M3", [8], -1), ("FP32", [17], 0),
                    ("FP32", [1], -4)]
        for wire, shape, off in bad_gets:
            with pytest.raises(exc):
                hipshm.get_contents_cast(reg.h, wire, shape, offset=off)
        # nothing was uploaded (no scratch allocated) and nothing written
        assert reg.h._scratch_size == 0
        _assert_bytes_equal(reg.dump(), reg.pattern, "region")
        with pytest.raises(exc):
            hipshm.set_shared_memory_region_cast(reg.h, x[:4], "INT8")
        # the exact fit is accepted
        assert hipshm.set_shared_memory_region_cast(reg.h, x[:32],
                                                    "BF16") == 64
        assert hipshm.set_shared_memory_region_cast(reg.h, x[:8], "FP8E4M3",
                                                    offset=56) == 8
        hipshm.get_contents_cast(reg.h, "BF16", [32])


# ---------------------------------------------------------------------------
# gather_pack
# ---------------------------------------------------------------------------

_TORCH_INT = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def _rand_tensor(numel, esz, seed):
    """Flat device tensor of `numel` elements of size `esz` holding
    random bytes."""
    import torch

    raw = np.random.default_rng(seed).integers(0, 256, numel * esz,
                                               dtype=np.uint8)
    return torch.from_numpy(raw).view(getattr(torch, _TORCH_INT[esz])).cuda()


def _check_pack(hr, view, what, dst_off=0):
    """gather_pack(view) must equal view.contiguous() byte for byte and
    leave the bytes around the destination alone."""
    import torch

    esz = view.element_size()
    nbytes = view.numel() * esz
    ref = np.frombuffer(view.contiguous().cpu().numpy().tobytes(),
                        dtype=np.uint8)
    assert ref.size == nbytes
    pat = np.random.default_rng(nbytes).integers(
        0, 256, dst_off + nbytes + PAD, dtype=np.uint8)
    dst = _dev_buffer(hr, pat)
    try:
        torch.cuda.synchronize()
        hr.gather_pack(view.data_ptr(), dst + dst_off, esz, list(view.shape),
                       list(view.stride()), 0, True)
        got = _dev_read(hr, dst, pat.size)
    finally:
        hr.free(dst)
    exp = pat.copy()
    exp[dst_off:dst_off + nbytes] = ref
    _assert_bytes_equal(got, exp, f"{what} shape={tuple(view.shape)} "
                        f"strides={tuple(view.stride())} esz={esz}")


TILED_SHAPES = [(16, 16), (17, 16), (64, 64), (65, 127), (130, 67)]


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
def test_gather_pack_tiled_shapes(hr, esz):
    """LDS-tiled transpose path at one full tile, ragged tiles, odd
    extents and more than one tile per axis, for every element size.
    The view has shape (rows, cols) and strides (1, rows)."""
    for rows, cols in TILED_SHAPES:
        parent = _rand_tensor(cols * rows, esz, rows * 1000 + cols).view(
            cols, rows)
        _check_pack(hr, parent.t(), "tiled")


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
def test_gather_pack_tiled_outer_dims(hr, esz):
    """Both outer dims > 1 with non-contiguous outer strides."""
    base = _rand_tensor(6 * 3 * 20 * 24, esz, 50 + esz).view(6, 3, 20, 24)
    view = base[::2].transpose(-1, -2)
    assert view.shape == (3, 3, 24, 20) and view.stride(2) == 1
    _check_pack(hr, view, "tiled 4-D")
    # and a sliced parent: col_stride != rows
    parent = _rand_tensor(40 * 50, esz, 60 + esz).view(40, 50)
    view = parent[:, 3:36].t()
    assert view.stride() == (1, 50) and view.shape == (33, 40)
    _check_pack(hr, view, "tiled sliced parent")
    # stride-0 columns (expand) also match the tiled condition
    col = _rand_tensor(24, esz, 70 + esz).view(24, 1)
    _check_pack(hr, col.expand(24, 20), "tiled expand")


def test_gather_pack_pair16_alignment_gate(hr):
    """2-byte elements: the pair-per-lane kernel needs 4-byte-aligned
    u32 accesses. Cases on both sides of the launcher's gate."""
    import torch

    # aligned side, ragged: odd rows from a parent with an even row
    # pitch (single-element load branch, partial tiles)
    parent = _rand_tensor(66 * 130, 2, 1).view(66, 130)
    view = parent[:, :129].t()
    assert view.shape == (129, 66) and view.stride() == (1, 130)
    _check_pack(hr, view, "pair ragged rows")
    view = parent[:, 2:19].t()  # even element offset, 17 rows
    _check_pack(hr, view, "pair 17 rows")
    # aligned side, batched with even strides
    base = _rand_tensor(3 * 34 * 66, 2, 2).view(3, 34, 66)
    _check_pack(hr, base.transpose(-1, -2), "pair batched")
    # odd cols
    _check_pack(hr, _rand_tensor(67 * 130, 2, 3).view(67, 130).t(),
                "odd cols")
    # odd rows, so col_stride is odd
    _check_pack(hr, _rand_tensor(64 * 65, 2, 4).view(64, 65).t(), "odd rows")
    # sliced parent: odd col_stride != rows
    parent = _rand_tensor(64 * 131, 2, 5).view(64, 131)
    view = parent[:, :100].t()
    assert view.stride() == (1, 131)
    _check_pack(hr, view, "odd col_stride")
    # odd element offset inside an even-pitch parent
    parent = _rand_tensor(64 * 130, 2, 6).view(64, 130)
    _check_pack(hr, parent[:, 1:65].t(), "odd column offset")
    # base pointer offset by one element
    flat = _rand_tensor(64 * 64 + 1, 2, 7)
    view = flat[1:].view(64, 64).t()
    assert view.data_ptr() % 4 == 2
    _check_pack(hr, view, "base +1 element")
    # batched with an odd outer stride (s1 = 2049), even col_stride
    flat = _rand_tensor(7200, 2, 8)
    view = torch.as_strided(flat, (3, 32, 64), (2049, 1, 32))
    _check_pack(hr, view, "odd s1")
    view = torch.as_strided(flat, (2, 2, 32, 64), (3001, 2050, 1, 32))
    _check_pack(hr, view, "odd s0")
    # destination 2-byte aligned only
    parent = _rand_tensor(64 * 64, 2, 9).view(64, 64)
    _check_pack(hr, parent.t(), "dst +2", dst_off=2)


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
def test_gather_pack_plain_kernel(hr, esz):
    """Views that do not match the transpose pattern go through the
    per-element gather_pack_kernel."""
    x = _rand_tensor(20 * 30, esz, 80 + esz).view(20, 30)
    _check_pack(hr, x[:, ::2], "x[:, ::2]")
    _check_pack(hr, x[::3, 1:], "x[::3, 1:]")
    _check_pack(hr, x.reshape(-1)[::5], "1-D x[::5]")
    _check_pack(hr, x[:1, :7].expand(5, 7), "expand rows")
    _check_pack(hr, x[:5, :1].expand(5, 7), "expand cols")
    nhwc = _rand_tensor(2 * 5 * 6 * 3, esz, 90 + esz).view(2, 5, 6, 3)
    view = nhwc.permute(0, 3, 1, 2)
    assert view.stride() == (90, 1, 18, 3)
    _check_pack(hr, view, "NHWC -> NCHW")
    _check_pack(hr, x[:8, :8].t(), "8x8 transpose")
    _check_pack(hr, x[:15, :20].t(), "20x15 transpose, one extent < 16")
    y = _rand_tensor(4 * 6, esz, 95 + esz).view(1, 4, 1, 6)
    _check_pack(hr, y[:, ::2], "size-1 dims")
    _check_pack(hr, y.view(4, 1, 6).transpose(0, 2), "size-1 middle dim")


def test_gather_pack_batch_limit_falls_back(hr):
    """More than 65 535 outer batches of 16x16 bytes: the tiled path's
    grid.z limit sends this to the plain kernel."""
    x = _rand_tensor(65537 * 16 * 16, 1, 99).view(65537, 16, 16)
    _check_pack(hr, x.transpose(-1, -2), "65537 batches")


# ---------------------------------------------------------------------------
# image preprocess
# ---------------------------------------------------------------------------

MEAN = [104.0, 117.0, 123.0]
STD = [0.5, 2.0, 0.017]

# (ih, iw, oh, ow): upscale; identity (exact); 1-pixel and 1-row
# sources; an output that is no multiple of 256 lanes; more than
# 2048 * 256 outputs (second grid-stride sweep)
PREPROCESS_SIZES = [
    (5, 7, 16, 12),
    (9, 13, 9, 13),
    (1, 1, 4, 4),
    (1, 9, 3, 3),
    (300, 451, 37, 53),
    (64, 64, 725, 725),
]


def _run_preprocess(hr, imgs, oh, ow, mode, out_bf16, batched):
    """Returns the output as raw little-endian words (uint32 for fp32
    output, uint16 for bf16), shape [n, 3, oh, ow]; checks the canary
    behind the written range."""
    n = imgs.shape[0]
    _, ih, iw, _ = imgs.shape
    esz = 2 if out_bf16 else 4
    nbytes = n * 3 * oh * ow * esz
    pat = np.random.default_rng(nbytes + mode).integers(
        0, 256, nbytes + PAD, dtype=np.uint8)
    src = _dev_buffer(hr, np.ascontiguousarray(imgs).reshape(-1))
    dst = _dev_buffer(hr, pat)
    try:
        if batched:
            hr.image_preprocess_batched(src, dst, n, ih, iw, oh, ow, mode,
                                        out_bf16, MEAN, STD, 0, True)
        else:
            assert n == 1
            hr.image_preprocess(src, dst, ih, iw, oh, ow, mode, out_bf16,
                                MEAN, STD, 0, True)
        got = _dev_read(hr, dst, pat.size)
    finally:
        hr.free(src)
        hr.free(dst)
    _assert_bytes_equal(got[nbytes:], pat[nbytes:], "preprocess canary")
    words = got[:nbytes].copy().view(np.uint16 if out_bf16 else np.uint32)
    return words.reshape(n, 3, oh, ow)


def _check_preprocess(words, img, oh, ow, mode, what, ref):
    out = words.view(np.float32).astype(np.float64)
    err = np.abs(out - ref)
    atol = kr.preprocess_atol(mode, STD)
    assert np.all(err <= atol), (
        f"{what}: max err per channel {err.max(axis=(1, 2))} > "
        f"{atol.ravel()}")
    if img.shape[:2] == (oh, ow):
        exact = kr.preprocess_identity_fp32(img, mode, MEAN, STD)
        assert np.array_equal(words, exact.view(np.uint32)), (
            f"{what}: identity size is not bit-exact")


@pytest.mark.parametrize("size", PREPROCESS_SIZES,
                         ids=lambda s: "{}x{}to{}x{}".format(*s))
def test_image_preprocess_edges(hr, size):
    """Single and batched kernels, all three modes (mode 0 with a
    per-channel std), fp32 against the float64 reference and bf16
    output as the truncated fp32 output."""
    ih, iw, oh, ow = size
    rng = np.random.default_rng(ih * 1000 + ow)
    imgs = rng.integers(0, 256, (3, ih, iw, 3), dtype=np.uint8)
    for mode in (0, 1, 2):
        what = f"mode {mode}"
        # one float64 reference per image, shared by the checks below
        refs = [kr.preprocess_ref(img, oh, ow, mode, MEAN, STD)
                for img in imgs]
        single = _run_preprocess(hr, imgs[:1], oh, ow, mode, False, False)
        _check_preprocess(single[0], imgs[0], oh, ow, mode, what + " single",
                          refs[0])
        single16 = _run_preprocess(hr, imgs[:1], oh, ow, mode, True, False)
        assert np.array_equal(single16, (single >> 16).astype(np.uint16)), (
            what + " single bf16 is not the truncated fp32 output")
        for n in (1, 3):
            b = _run_preprocess(hr, imgs[:n], oh, ow, mode, False, True)
            for i in range(n):
                _check_preprocess(b[i], imgs[i], oh, ow, mode,
                                  f"{what} batched n={n} image {i}", refs[i])
            # image i of the 16-bit buffer starts at element i*3*oh*ow
            b16 = _run_preprocess(hr, imgs[:n], oh, ow, mode, True, True)
            assert np.array_equal(b16, (b >> 16).astype(np.uint16)), (
                f"{what} batched n={n} bf16 is not the truncated fp32 "
                "output")
