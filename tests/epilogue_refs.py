"""References for the ResNet epilogue kernels (bias (+ residual)
(+ ReLU) over bf16), computed by torch on the CPU in fp32.

Used by tests/test_channels_last_gpu.py and
tests/test_epilogue_special_gpu.py; checked on the CPU by
tests/test_epilogue_refs.py. Nothing here touches a GPU.
"""

import torch

BF16_MAX = 3.3895313892515355e38  # 0x7F7F
MIN_NORMAL = 2.0 ** -126

# what x and the residual draw from
SPECIAL_VALUES = [
    0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -7, float("inf"), float("-inf"),
    float("nan"), BF16_MAX, -BF16_MAX, MIN_NORMAL,
]

# fp32 NaNs whose payload the integer rounding formula carries into the
# sign bit (0x7FFFFFFF + 0x7FFF wraps to 0x8000xxxx, i.e. -0.0; the
# negative one wraps to +0.0)
NAN_PAYLOAD_BITS = (0x7FFFFFFF, 0xFFFFFFFF)


def special_bias():
    """16 fp32 biases: the zeros, +/-2^-8 (half a bf16 ulp of 1.0: the
    ties), infinities, values that overflow next to bf16 max, the
    canonical NaN, the two all-ones-payload NaNs, and a few ordinary
    values on either side of the tie."""
    plain = torch.tensor([
        0.0, -0.0, 2.0 ** -8, -(2.0 ** -8), float("inf"), float("-inf"),
        1e38, -1e38, float("nan"),
        1.0, -1.0, 0.5, 2.0 ** -9, 3 * 2.0 ** -9,
    ], dtype=torch.float32)
    payload = torch.tensor(
        [b - (1 << 32) if b >= (1 << 31) else b for b in NAN_PAYLOAD_BITS],
        dtype=torch.int32).view(torch.float32)
    bias = torch.cat([plain[:9], payload, plain[9:]])
    assert bias.numel() == 16
    return bias


def special_case(shape):
    """(x, res, bias) on the CPU, x and res bf16 of the NCHW `shape`
    with 16 channels: inside every channel's plane, element p holds
    x = SPECIAL_VALUES[p % 11] and res = SPECIAL_VALUES[(p // 11) % 11],
    so a plane of 121 or more elements meets every (x, res) pair with
    that channel's bias."""
    n, c, h, w = shape
    assert c == 16
    vals = torch.tensor(SPECIAL_VALUES, dtype=torch.float32).to(torch.bfloat16)
    k = len(SPECIAL_VALUES)
    p = torch.arange(h * w)
    x = vals[p % k].view(1, 1, h, w).expand(n, c, h, w).contiguous()
    res = vals[(p // k) % k].view(1, 1, h, w).expand(n, c, h, w).contiguous()
    return x, res, special_bias()


def count_triples(x, res, bias):
    """Number of distinct (x bits, res bits, bias bits) triples; res may
    be None (pairs then)."""
    cols = [x.contiguous().view(torch.int16).to(torch.int64).reshape(-1)]
    if res is not None:
        cols.append(
            res.contiguous().view(torch.int16).to(torch.int64).reshape(-1))
    b = bias.view(torch.int32).to(torch.int64).view(1, -1, 1, 1)
    cols.append(b.expand(x.shape).reshape(-1))
    return torch.unique(torch.stack(cols, 1), dim=0).shape[0]


def all_triples(with_res):
    k = len(SPECIAL_VALUES)
    return k * (k if with_res else 1) * 16


def epilogue_ref(x, res, bias, relu):
    """((x + res) + bias[c]) in fp32 -> optional ReLU -> bf16, on the
    CPU. x and res are bf16 [N, C, H, W] in any memory format and on any
    device, res may be None, bias is fp32 [C]."""
    ref = x.detach().cpu().float()
    if res is not None:
        ref = ref + res.detach().cpu().float()
    ref = ref + bias.detach().cpu().float().view(1, -1, 1, 1)
    if relu:
        ref = torch.relu(ref)
    return ref.to(torch.bfloat16)


def assert_bits_equal(got, ref, what=None):
    """Bit equality of two bf16 tensors of the same logical shape."""
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    same = got.view(torch.int16) == ref.view(torch.int16)
    assert bool(same.all()), (what, int((~same).sum()),
                              (~same).nonzero()[:4].tolist())


def assert_special_equal(got, ref, what=None):
    """NaN exactly where the reference has NaN; every other element
    equal as a float (the sign of a zero is not pinned)."""
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    nan = torch.isnan(ref)
    bad_nan = torch.isnan(got) != nan
    assert not bool(bad_nan.any()), (
        what, "NaN positions differ", int(bad_nan.sum()),
        bad_nan.nonzero()[:4].tolist())
    bad = (got.float() != ref.float()) & ~nan
    assert not bool(bad.any()), (
        what, int(bad.sum()), bad.nonzero()[:4].tolist(),
        got[bad][:4].tolist(), ref[bad][:4].tolist())


def assert_special_reference_is_rich(x, res, bias, relu, ref):
    """The special-value reference holds every class of result the
    kernels have to get right."""
    s = x.float() if res is None else x.float() + res.float()
    b = bias.view(1, -1, 1, 1).expand(ref.shape)
    r = ref.float()
    assert bool(torch.isnan(ref).any())
    assert bool((r == float("inf")).any())
    if relu:
        before = epilogue_ref(x, res, bias, False).float()
        assert bool(((before < 0) & (r == 0)).any())
        assert not bool((r < 0).any())
    else:
        assert bool((r == float("-inf")).any())
    # ties: 2^-8 is half a bf16 ulp at 1.0
    down = (s == 1.0) & (b == 2.0 ** -8)
    up = (s == 1.0 + 2.0 ** -7) & (b == 2.0 ** -8)
    assert bool(down.any()) and bool((r[down] == 1.0).all())
    assert bool(up.any()) and bool((r[up] == 1.015625).all())
