"""The fused 1x1 conv + bias (+ residual) + ReLU MFMA kernel against torch
references, kernel by kernel and through the whole fused ResNet50
(require an MI355X). tests/test_conv1x1_index.py checks the same shapes'
addressing on the CPU."""

import pytest

pytestmark = pytest.mark.gpu

# (N, C, K, H, W)
CASES = [
    (1, 64, 64, 7, 7),        # one ragged tile
    (3, 64, 64, 7, 7),        # tiles spanning images, ragged last tile, odd HW
    (2, 64, 128, 14, 14),     # an image larger than a tile, two channel tiles
    (1, 64, 64, 9, 5),        # non-square, odd
    (1, 32, 64, 1, 1),        # one pixel, one chunk
    (2, 2048, 64, 7, 7),      # the longest reduction
    (1, 64, 256, 56, 56),     # the served plane: 64 columns, 16-byte stores
    (2, 64, 64, 4, 6),        # 16-byte stores with tiles spanning images
    (6, 64, 256, 56, 56),     # 128 columns, 16-byte stores
    (42, 64, 512, 14, 14),    # 128 columns, dword loads, 2-byte stores
    (336, 64, 256, 7, 7),     # 128 columns, 2-byte loads and stores
]
IDS = ["x".join(map(str, c)) for c in CASES]
MODES = ["act", "res"]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _epilogue_ref(x, r, bias, relu):
    import torch

    ref = x.float()
    if r is not None:
        ref = ref + r.float()
    ref = ref + bias.view(1, -1, 1, 1)
    if relu:
        ref = ref.relu()
    return ref.to(torch.bfloat16)


def _run(x, w, bias, residual, relu):
    """The kernel, called directly (no dispatch table)."""
    import torch

    from client_amd.models.resnet import pack_conv1x1_weight
    from client_amd.ops import hip_runtime as hr

    n, c, h, wd = x.shape
    k = w.shape[0]
    out = torch.full((n, k, h, wd), 7.0, device="cuda",
                     dtype=torch.bfloat16)
    wp = pack_conv1x1_weight(w)
    hr.conv1x1_bias_act_bf16(
        x.data_ptr(), wp.data_ptr(), bias.data_ptr(),
        0 if residual is None else residual.data_ptr(), out.data_ptr(), n,
        c, k, h, wd, relu, _stream())
    torch.cuda.synchronize()
    return out


def _conv_f32(x, w):
    import torch.nn.functional as F

    return F.conv2d(x.float(), w.float())


def _random(case, seed, mode):
    import torch

    n, c, k, h, w = case
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, c, h, w), device="cuda",
                    generator=gen).to(torch.bfloat16)
    wt = (torch.randn((k, c, 1, 1), device="cuda", generator=gen)
          * 0.05).to(torch.bfloat16)
    bias = torch.randn(k, device="cuda", generator=gen)
    res = None
    if mode == "res":
        res = torch.randn((n, k, h, w), device="cuda",
                          generator=gen).to(torch.bfloat16)
    return x, wt, bias, res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_integer_layout(case, mode):
    """Small integers make every partial sum an exact fp32 integer, so
    any summation order gives the same bits: a wrong lane map, column
    offset, residual offset or weight packing shows as an unequal
    element."""
    import torch

    n, c, k, h, w = case
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(-2, 3, (n, c, h, w), device="cuda",
                      generator=gen).to(torch.bfloat16)
    wt = torch.randint(-1, 2, (k, c, 1, 1), device="cuda",
                       generator=gen).to(torch.bfloat16)
    bias = torch.randn(k, device="cuda", generator=gen)
    assert (bias > 0).any() and (bias < 0).any()
    res = None
    if mode == "res":
        res = torch.randint(-8, 9, (n, k, h, w), device="cuda",
                            generator=gen).to(torch.bfloat16)
    conv = _conv_f32(x, wt).to(torch.bfloat16)
    for relu in (False, True):
        ref = _epilogue_ref(conv, res, bias, relu)
        got = _run(x, wt, bias, res, relu)
        assert got.shape == ref.shape
        assert torch.equal(got, ref), (
            relu, (got.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_data_within_rounding_bound(case):
    """|got - ref| <= 2^-8 |ref| + C * 2^-24 * S, S = conv(|x|, |w|):
    one bf16 rounding of the result plus the worst-case fp32
    accumulation error of a reduction of length C."""
    import torch

    n, c, k, h, w = case
    x, wt, _, _ = _random(case, 5, "act")
    zero = torch.zeros(k, device="cuda")
    ref = _conv_f32(x, wt)
    s = _conv_f32(x.abs(), wt.abs())
    got = _run(x, wt, zero, None, False).float()
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + c * 2.0 ** -24 * s
    worst = (err / bound).max().item()
    print(f"{case}: max err/bound = {worst:.3f}, max err = "
          f"{err.max().item():.3e}")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deterministic_and_batch_invariant(case, mode):
    """Two runs are bit-equal, and image i of the batch equals the same
    image run alone (for the last three cases the batch takes a
    128-column kernel and the single image the 64-column one)."""
    import torch

    n = case[0]
    x, wt, bias, res = _random(case, 7, mode)
    a = _run(x, wt, bias, res, True)
    b = _run(x, wt, bias, res, True)
    assert torch.equal(a, b)
    for i in sorted({0, 1 % n, n // 2, n - 1}):
        r1 = None if res is None else res[i:i + 1].contiguous()
        one = _run(x[i:i + 1].contiguous(), wt, bias, r1, True)
        assert torch.equal(one[0], a[i]), i


def test_tile_variants_give_the_same_bits():
    """The 128-column kernels run for the batch, the 64-column kernels
    for a few images of it: the same images come out bit-equal, for each
    load/store width."""
    import torch

    from client_amd.ops import hip_runtime as hr

    assert hr.conv1x1_supported(6, 64, 256, 56, 56)
    for case in CASES[-3:]:
        for mode in MODES:
            x, wt, bias, res = _random(case, 9, mode)
            full = _run(x, wt, bias, res, True)
            r3 = None if res is None else res[1:4].contiguous()
            three = _run(x[1:4].contiguous(), wt, bias, r3, True)
            assert torch.equal(three, full[1:4]), (case, mode)


def test_unsupported_shapes_and_aliases_do_not_launch():
    import torch

    from client_amd.ops import hip_runtime as hr

    assert hr.conv1x1_supported(2, 64, 64, 14, 14)

    def refused(x, wp, bias, res, out, n, c, k, h, w):
        before = out.clone()
        with pytest.raises(RuntimeError):
            hr.conv1x1_bias_act_bf16(
                x.data_ptr(), wp.data_ptr(), bias.data_ptr(),
                0 if res is None else res.data_ptr(), out.data_ptr(), n, c,
                k, h, w, True, _stream())
        torch.cuda.synchronize()
        assert torch.equal(out, before)

    for bad in [(2, 48, 64, 14, 14), (2, 16, 64, 14, 14),
                (2, 64, 96, 14, 14), (2, 64, 64, 0, 14)]:
        assert not hr.conv1x1_supported(*bad)
        n, c, k, h, w = bad
        x = torch.zeros((n, c, max(h, 1), w), device="cuda",
                        dtype=torch.bfloat16)
        wp = torch.zeros((c * k,), device="cuda", dtype=torch.bfloat16)
        bias = torch.zeros(k, device="cuda")
        out = torch.full((n, k, max(h, 1), w), 7.0, device="cuda",
                         dtype=torch.bfloat16)
        refused(x, wp, bias, None, out, n, c, k, h, w)
    # aliases and misaligned pointers, on a supported shape
    n, c, k, h, w = 2, 64, 64, 14, 14
    x = torch.full((n, c, h, w), 7.0, device="cuda", dtype=torch.bfloat16)
    wp = torch.zeros((c * k + 8,), device="cuda", dtype=torch.bfloat16)
    bias = torch.zeros(k + 1, device="cuda")
    res = torch.full((n, k, h, w), 7.0, device="cuda", dtype=torch.bfloat16)
    out = torch.full((n * k * h * w + 8,), 7.0, device="cuda",
                     dtype=torch.bfloat16)
    refused(x, wp, bias, None, x, n, c, k, h, w)        # out == x
    refused(x, wp, bias, res, res, n, c, k, h, w)       # out == residual
    refused(x, wp, bias, None, out[1:], n, c, k, h, w)  # out not 16 B
    refused(x, wp[1:], bias, None, out, n, c, k, h, w)  # weights not 16 B
    refused(x, wp, bias, out[1:], out[8:], n, c, k, h, w)  # residual not 16 B


def test_eligible_only_on_table_shapes(monkeypatch):
    import torch

    from client_amd.models import resnet
    from client_amd.models.resnet import Conv1x1BiasAct

    # a table of its own, so the test does not depend on which shapes
    # were admitted
    monkeypatch.setattr(resnet, "CONV1X1_TABLE", frozenset({
        (64, 256, 56, 56, "res"), (256, 64, 56, 56, "act")}))
    monkeypatch.delenv("CLIENT_AMD_CONV1X1", raising=False)
    monkeypatch.delenv("CLIENT_AMD_FUSED_BIAS", raising=False)
    conv3 = torch.nn.Conv2d(64, 256, 1, bias=False).to("cuda",
                                                       torch.bfloat16)
    conv1 = torch.nn.Conv2d(256, 64, 1, bias=False).to("cuda",
                                                       torch.bfloat16)
    x64 = torch.zeros((2, 64, 56, 56), device="cuda", dtype=torch.bfloat16)
    x256 = torch.zeros((2, 256, 56, 56), device="cuda",
                       dtype=torch.bfloat16)
    assert Conv1x1BiasAct.eligible(x64, conv3, x256)
    assert Conv1x1BiasAct.eligible(x256, conv1)
    # the other mode of each shape is off the table
    assert not Conv1x1BiasAct.eligible(x64, conv3)
    assert not Conv1x1BiasAct.eligible(x256, conv1, x64)
    # off-table plane, fp32, non-contiguous input or residual
    assert not Conv1x1BiasAct.eligible(
        x256[:, :, :20, :20].contiguous(), conv1)
    assert not Conv1x1BiasAct.eligible(x256.float(), conv1)
    assert not Conv1x1BiasAct.eligible(x256[:, :, ::1, ::2], conv1)
    assert not Conv1x1BiasAct.eligible(
        x64, conv3, x256.contiguous(memory_format=torch.channels_last))
    assert not Conv1x1BiasAct.eligible(x64, conv3, x256.float())
    # a conv the kernel does not compute
    strided = torch.nn.Conv2d(256, 64, 1, stride=2, bias=False).to(
        "cuda", torch.bfloat16)
    assert not Conv1x1BiasAct.eligible(x256, strided)
    # each of the two switches
    monkeypatch.setenv("CLIENT_AMD_CONV1X1", "0")
    assert not Conv1x1BiasAct.eligible(x256, conv1)
    monkeypatch.setenv("CLIENT_AMD_CONV1X1", "1")
    assert Conv1x1BiasAct.eligible(x256, conv1)
    monkeypatch.setenv("CLIENT_AMD_FUSED_BIAS", "0")
    assert not Conv1x1BiasAct.eligible(x256, conv1)


@pytest.fixture(scope="module")
def fused_resnet():
    import torch

    from client_amd.models.resnet import ResNet50, fold_batchnorm

    torch.manual_seed(2)
    m = ResNet50().eval()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)
    return fold_batchnorm(m, fuse_eltwise=True).to("cuda", torch.bfloat16)


def _kernel_calls(model):
    from client_amd.models.resnet import Conv1x1BiasAct

    return sum(m.calls for m in model.modules()
               if isinstance(m, Conv1x1BiasAct))


def _table_eligible_convs(model, size):
    """Number of bottleneck 1x1 convs of a size x size forward whose
    shape/mode is in CONV1X1_TABLE, derived from the model and the
    table."""
    from client_amd.models.resnet import CONV1X1_TABLE, FusedBottleneck

    hw = (size - 1) // 2 + 1   # stem conv, stride 2
    hw = (hw - 1) // 2 + 1     # max-pool, stride 2
    count = 0
    for m in model.modules():
        if not isinstance(m, FusedBottleneck):
            continue
        k1, c1 = m.conv1.weight.shape[:2]
        count += (c1, k1, hw, hw, "act") in CONV1X1_TABLE
        hw = (hw - 1) // m.conv2.stride[0] + 1
        k3, c3 = m.conv3.weight.shape[:2]
        count += (c3, k3, hw, hw, "res") in CONV1X1_TABLE
    return count


@pytest.mark.parametrize("size", [64, 224])
def test_whole_model_switch_on_against_off(fused_resnet, size, monkeypatch):
    """Logits with the kernel against logits without it, and the
    kernel's run against itself, under the deterministic switch that
    makes the remaining library convs order-stable (as in
    tests/test_conv3x3_gpu.py)."""
    import torch

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(size)
    x = torch.randn(2, 3, size, size, device="cuda", dtype=torch.bfloat16)

    def forward(flag):
        monkeypatch.setenv("CLIENT_AMD_CONV1X1", flag)
        before = _kernel_calls(fused_resnet)
        with torch.inference_mode():
            y = fused_resnet(x)
        torch.cuda.synchronize()
        return y, _kernel_calls(fused_resnet) - before

    on, calls_on = forward("1")
    again, _ = forward("1")
    off, calls_off = forward("0")
    assert calls_off == 0
    # at 64x64 every plane is outside the table: the model falls back
    # throughout
    assert _table_eligible_convs(fused_resnet, 64) == 0
    assert calls_on == _table_eligible_convs(fused_resnet, size)
    assert torch.equal(on, again)
    assert on.float().std().item() > 0
    diff = (on.float() - off.float()).abs().max().item()
    print(f"size {size}: {calls_on} kernel calls, max |on - off| = "
          f"{diff:.4f}")
    assert torch.allclose(on.float(), off.float(), atol=0.15, rtol=0.05), diff


@pytest.mark.parametrize("mode", MODES)
def test_module_under_graph_capture(mode, monkeypatch):
    """Captured into a hipGraph and replayed twice, then with a new
    input, the module gives the eager result (the weights are packed by
    the eager warm-up call, before capture)."""
    import torch

    from client_amd.models import resnet
    from client_amd.models.resnet import (BiasAct, BiasResAct,
                                          Conv1x1BiasAct)

    monkeypatch.setattr(resnet, "CONV1X1_TABLE", frozenset({
        (128, 512, 28, 28, "res"), (128, 512, 28, 28, "act")}))
    torch.manual_seed(13)
    conv = torch.nn.Conv2d(128, 512, 1, bias=False).to("cuda",
                                                       torch.bfloat16)
    if mode == "res":
        ba = BiasResAct(torch.randn(512)).to("cuda")
        res = torch.randn(3, 512, 28, 28, device="cuda",
                          dtype=torch.bfloat16)
    else:
        ba = BiasAct(torch.randn(512), relu=True).to("cuda")
        res = None
    mod = Conv1x1BiasAct()
    x = torch.randn(3, 128, 28, 28, device="cuda", dtype=torch.bfloat16)
    assert Conv1x1BiasAct.eligible(x, conv, res)
    with torch.inference_mode():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = mod(x, conv, ba, res).clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = mod(x, conv, ba, res)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
        # new input (and residual), same graph
        x.copy_(torch.randn_like(x))
        if res is not None:
            res.copy_(torch.randn_like(res))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, mod(x, conv, ba, res))
        assert mod.calls == 3
