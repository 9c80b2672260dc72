"""Non-finite inputs, signed zeros, overflow and exact rounding ties
through the three ResNet epilogue kernel families (per-plane NCHW, flat
NCHW, channels-last) against the fp32 CPU reference of
tests/epilogue_refs.py (require an MI355X)."""

import pytest

import epilogue_refs as er

pytestmark = pytest.mark.gpu

# (family, NCHW shape): plane 2304 stays on the per-plane kernels, 144
# and the odd 143 (vectors crossing plane boundaries, scalar tail) take
# the flat kernels, and the last runs the channels-last kernel on the
# same values laid out NHWC
CASES = [
    ("plane", (1, 16, 48, 48)),
    ("flat", (1, 16, 12, 12)),
    ("flat", (1, 16, 11, 13)),
    ("cl", (1, 16, 12, 12)),
]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _run(family, x, res, bias, relu, via_bias_act=False):
    """One out-of-place launch on GPU copies of the CPU tensors; returns
    the output as a logical NCHW tensor."""
    import torch

    from client_amd.ops import hip_runtime as hr

    n, c, h, w = x.shape
    if family == "cl":
        def dev(t):  # NHWC memory, viewed as NCHW
            return t.permute(0, 2, 3, 1).contiguous().cuda().permute(
                0, 3, 1, 2)
    else:
        def dev(t):
            return t.contiguous().cuda()
    xd = dev(x)
    rd = None if res is None else dev(res)
    bd = bias.cuda()
    # the payload NaNs must reach the device as they are
    assert torch.equal(bd.cpu().view(torch.int32), bias.view(torch.int32))
    out = dev(torch.full(x.shape, 7.0, dtype=torch.bfloat16))
    rp = 0 if rd is None else rd.data_ptr()
    if family == "cl":
        hr.bias_res_act_cl_bf16(xd.data_ptr(), rp, bd.data_ptr(),
                                out.data_ptr(), xd.numel(), c, relu,
                                _stream())
    elif via_bias_act:
        hr.bias_act_bf16(xd.data_ptr(), bd.data_ptr(), out.data_ptr(),
                         n * c, h * w, c, relu, _stream())
    else:
        hr.bias_res_act_bf16(xd.data_ptr(), rp, bd.data_ptr(),
                             out.data_ptr(), n * c, h * w, c, relu,
                             _stream())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("family,shape", CASES,
                         ids=[f"{f}-" + "x".join(map(str, s))
                              for f, s in CASES])
def test_special_values(family, shape, relu, with_res):
    """Every (x, residual, bias) combination of zeros, +/-1, the tie
    operand 1 + 2^-7, +/-inf, NaN, +/-bf16 max and 2^-126 with biases
    that include +/-2^-8, +/-inf, +/-1e38, and NaNs with an all-ones
    payload: NaN where the reference has NaN, equal values elsewhere."""
    x, res, bias = er.special_case(shape)
    if not with_res:
        res = None
    covered = er.count_triples(x, res, bias)
    wanted = er.all_triples(with_res)
    assert covered >= 0.98 * wanted, (covered, wanted)
    ref = er.epilogue_ref(x, res, bias, relu)
    er.assert_special_reference_is_rich(x, res, bias, relu, ref)

    got = _run(family, x, res, bias, relu)
    er.assert_special_equal(got, ref, (family, shape, relu, with_res))
    if family != "cl" and not with_res:
        got = _run(family, x, None, bias, relu, via_bias_act=True)
        er.assert_special_equal(got, ref, ("bias_act", shape, relu))
