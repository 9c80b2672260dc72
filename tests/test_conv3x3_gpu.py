"""The fused 3x3 conv + bias + ReLU MFMA kernel against torch references,
kernel by kernel and through the whole fused ResNet50 (require an
MI355X). tests/test_conv3x3_index.py checks the same shapes' addressing
on the CPU."""

import pytest

pytestmark = pytest.mark.gpu

# (N, C, K, H, W, stride)
CASES = [
    (1, 64, 64, 7, 7, 1),      # one tile spanning less than it could hold
    (3, 64, 64, 7, 7, 1),      # tiles spanning images, ragged last tile
    (2, 64, 64, 14, 14, 1),    # an image larger than a 64-column tile
    (1, 64, 128, 9, 5, 1),     # non-square, odd W, K != C, two channel tiles
    (2, 64, 64, 20, 20, 1),    # rows that do not fill the tile's columns
    (1, 64, 64, 56, 56, 1),    # the served row length
    (2, 128, 128, 8, 8, 2),    # stride 2, even extent
    (2, 128, 128, 7, 7, 2),    # stride 2, odd extent
    (2, 512, 512, 7, 7, 1),    # the longest reduction (4608)
    (20, 64, 64, 56, 56, 1),   # enough tiles for the 128-column kernel
]
IDS = ["x".join(map(str, c)) for c in CASES]


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


def _run(x, w, bias, stride, relu):
    """The kernel, called directly (no dispatch table)."""
    import torch

    from client_amd.models.resnet import pack_conv3x3_weight
    from client_amd.ops import hip_runtime as hr

    n, c, h, wd = x.shape
    k = w.shape[0]
    out = torch.full((n, k, (h - 1) // stride + 1, (wd - 1) // stride + 1),
                     7.0, device="cuda", dtype=torch.bfloat16)
    wp = pack_conv3x3_weight(w)
    hr.conv3x3_bias_act_bf16(x.data_ptr(), wp.data_ptr(), bias.data_ptr(),
                             out.data_ptr(), n, c, k, h, wd, stride, relu,
                             _stream())
    torch.cuda.synchronize()
    return out


def _conv_f32(x, w, stride):
    import torch.nn.functional as F

    return F.conv2d(x.float(), w.float(), stride=stride, padding=1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_integer_layout(case):
    """Small integers make every partial sum an exact fp32 integer, so
    any summation order gives the same bits: a wrong lane map, tap
    offset, halo or weight packing shows as an unequal element."""
    import torch

    n, c, k, h, w, stride = case
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(-2, 3, (n, c, h, w), device="cuda",
                      generator=gen).to(torch.bfloat16)
    wt = torch.randint(-1, 2, (k, c, 3, 3), device="cuda",
                       generator=gen).to(torch.bfloat16)
    bias = torch.randn(k, device="cuda", generator=gen)
    assert (bias > 0).any() and (bias < 0).any()
    conv = _conv_f32(x, wt, stride).to(torch.bfloat16)
    for relu in (False, True):
        ref = _epilogue_ref(conv, None, bias, relu)
        got = _run(x, wt, bias, stride, relu)
        assert got.shape == ref.shape
        assert torch.equal(got, ref), (
            relu, (got.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_data_within_rounding_bound(case):
    """|got - ref| <= 2^-8 |ref| + 4608 * 2^-24 * S, S = conv(|x|, |w|):
    one bf16 rounding of the result plus the worst-case fp32
    accumulation error of the longest reduction."""
    import torch

    n, c, k, h, w, stride = case
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((n, c, h, w), device="cuda",
                    generator=gen).to(torch.bfloat16)
    wt = (torch.randn((k, c, 3, 3), device="cuda", generator=gen)
          * 0.05).to(torch.bfloat16)
    zero = torch.zeros(k, device="cuda")
    ref = _conv_f32(x, wt, stride)
    s = _conv_f32(x.abs(), wt.abs(), stride)
    got = _run(x, wt, zero, stride, False).float()
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 4608 * 2.0 ** -24 * s
    worst = (err / bound).max().item()
    print(f"{case}: max err/bound = {worst:.3f}, max err = "
          f"{err.max().item():.3e}")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_deterministic_and_batch_invariant(case):
    import torch

    n, c, k, h, w, stride = case
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((n, c, h, w), device="cuda",
                    generator=gen).to(torch.bfloat16)
    wt = (torch.randn((k, c, 3, 3), device="cuda", generator=gen)
          * 0.05).to(torch.bfloat16)
    bias = torch.randn(k, device="cuda", generator=gen)
    a = _run(x, wt, bias, stride, True)
    b = _run(x, wt, bias, stride, True)
    assert torch.equal(a, b)
    for i in range(n):
        one = _run(x[i:i + 1].contiguous(), wt, bias, stride, True)
        assert torch.equal(one[0], a[i]), i


def test_image_of_batch_3_equals_batch_1():
    """The case the issue names: image i of an N = 3 call on 7x7 planes
    (tiles span images) equals the N = 1 call on that image; and at
    56x56 images of a batch of 32, which takes the 128-column kernel,
    equal those of batches of 3 and 1, which take the 64-column one."""
    import torch

    gen = torch.Generator(device="cuda").manual_seed(9)
    small = torch.randn((3, 64, 7, 7), device="cuda",
                        generator=gen).to(torch.bfloat16)
    x = torch.randn((32, 64, 56, 56), device="cuda",
                    generator=gen).to(torch.bfloat16)
    wt = (torch.randn((64, 64, 3, 3), device="cuda", generator=gen)
          * 0.05).to(torch.bfloat16)
    bias = torch.randn(64, device="cuda", generator=gen)
    three = _run(small, wt, bias, 1, True)
    for i in range(3):
        one = _run(small[i:i + 1].contiguous(), wt, bias, 1, True)
        assert torch.equal(one[0], three[i]), i
    full = _run(x, wt, bias, 1, True)
    three = _run(x[:3].contiguous(), wt, bias, 1, True)
    assert torch.equal(three, full[:3])
    for i in (0, 2, 31):
        one = _run(x[i:i + 1].contiguous(), wt, bias, 1, True)
        assert torch.equal(one[0], full[i]), i


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[7]],
                         ids=[IDS[1], IDS[4], IDS[7]])
def test_nan_and_inf_propagate_as_through_conv2_bias_act(case):
    """NaN and +/-Inf in the input come out where conv2 -> BiasAct puts
    them today, which is where a direct convolution puts them;
    everything else stays within the rounding bound."""
    import torch
    import torch.nn.functional as F

    from client_amd.ops import hip_runtime as hr

    n, c, k, h, w, stride = case
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((n, c, h, w), device="cuda",
                    generator=gen).to(torch.bfloat16)
    wt = (torch.randn((k, c, 3, 3), device="cuda", generator=gen)
          * 0.05).to(torch.bfloat16)
    assert (wt != 0).all()
    bias = torch.randn(k, device="cuda", generator=gen)
    # a few specials, far enough apart that most outputs stay finite
    x[0, 1, 0, 0] = float("nan")
    x[0, 5, h - 1, w - 1] = float("inf")
    x[n - 1, 7, h // 2, w // 2] = float("-inf")
    x[n - 1, 9, h // 2, w // 2] = float("inf")  # inf - inf somewhere

    today = F.conv2d(x, wt, stride=stride, padding=1).contiguous()
    hr.bias_act_bf16(today.data_ptr(), bias.data_ptr(), today.data_ptr(),
                     n * k, today.shape[2] * today.shape[3], k, True,
                     _stream())
    torch.cuda.synchronize()
    # direct convolution on the CPU in fp64: a special value reaches
    # exactly the outputs whose 3x3 window holds it (a GPU library conv
    # may pick a transform-domain solver, which spreads them further)
    direct = F.conv2d(x.double().cpu(), wt.double().cpu(), stride=stride,
                      padding=1).to("cuda")
    ref = _epilogue_ref(direct.float().to(torch.bfloat16), None, bias, True)
    got = _run(x, wt, bias, stride, True)

    nan = torch.isnan(ref)
    inf = torch.isinf(ref)
    print(f"{case}: NaN direct {int(nan.sum())}, today "
          f"{int(torch.isnan(today).sum())}, kernel "
          f"{int(torch.isnan(got).sum())}; kernel != today at "
          f"{int((torch.isnan(got) != torch.isnan(today)).sum())}; Inf "
          f"direct {int(inf.sum())}, today {int(torch.isinf(today).sum())}, "
          f"kernel {int(torch.isinf(got).sum())}")
    assert nan.any() and not nan.all() and inf.any()
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(torch.isnan(got), torch.isnan(today))
    assert torch.equal(torch.isinf(got), inf)
    assert torch.equal(torch.isinf(got), torch.isinf(today))
    assert torch.equal(got[inf], ref[inf])
    assert torch.equal(got[inf], today[inf])
    fin = ~nan & ~inf
    # finite remainder: the pre-epilogue bound, widened by the one extra
    # bf16 rounding of the epilogue's result
    xf = torch.nan_to_num(x.float(), nan=0.0, posinf=0.0, neginf=0.0)
    s = _conv_f32(xf.abs(), wt.abs(), stride)
    bound = (2.0 ** -8 * direct.abs() + 4608 * 2.0 ** -24 * s
             + 2.0 ** -8 * ref.double().abs())
    err = (got.double() - ref.double()).abs()
    assert (err[fin] <= bound[fin]).all()


def test_unsupported_shapes_do_not_launch():
    import torch

    from client_amd.models.resnet import Conv3x3BiasAct
    from client_amd.ops import hip_runtime as hr

    # the launcher rejects what the kernel cannot run ...
    assert hr.conv3x3_supported(2, 64, 64, 14, 14, 1)
    for bad in [(2, 48, 64, 14, 14, 1), (2, 64, 96, 14, 14, 1),
                (2, 64, 64, 14, 200, 1), (2, 64, 64, 14, 14, 3)]:
        assert not hr.conv3x3_supported(*bad)
        n, c, k, h, w, stride = bad
        x = torch.zeros((n, c, h, w), device="cuda", dtype=torch.bfloat16)
        wp = torch.zeros((9 * c * k,), device="cuda", dtype=torch.bfloat16)
        bias = torch.zeros(k, device="cuda")
        out = torch.full((n, k, h, w), 7.0, device="cuda",
                         dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            hr.conv3x3_bias_act_bf16(x.data_ptr(), wp.data_ptr(),
                                     bias.data_ptr(), out.data_ptr(), n, c,
                                     k, h, w, stride, True, _stream())
        torch.cuda.synchronize()
        assert (out == 7.0).all()
    # ... and the module takes only shapes of its dispatch table
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).to(
        "cuda", torch.bfloat16)
    served = torch.zeros((2, 64, 56, 56), device="cuda",
                         dtype=torch.bfloat16)
    assert Conv3x3BiasAct.eligible(served, conv)
    assert not Conv3x3BiasAct.eligible(served[:, :, :20, :20].contiguous(),
                                       conv)
    assert not Conv3x3BiasAct.eligible(served.float(), conv)
    assert not Conv3x3BiasAct.eligible(served[:, :, ::1, ::2], conv)


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
    from client_amd.models.resnet import Conv3x3BiasAct

    return sum(m.calls for m in model.modules()
               if isinstance(m, Conv3x3BiasAct))


@pytest.mark.parametrize("size", [64, 224])
def test_whole_model_switch_on_against_off(fused_resnet, size, monkeypatch):
    """Logits with the kernel against logits without it, and the
    kernel's run against itself. The library convs that remain
    (the stem, the 1x1s, 512 @ 14x14 stride 2, and everything at 64x64)
    accumulate split-K sums with atomics by default, so as in
    test_fused_resnet_bit_exact_vs_torch_formulas the deterministic
    switch selects their order-stable solvers; run-to-run equality then
    tests this kernel and not the library."""
    import torch

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(size)
    x = torch.randn(2, 3, size, size, device="cuda", dtype=torch.bfloat16)

    def forward(flag):
        monkeypatch.setenv("CLIENT_AMD_CONV3X3", flag)
        before = _kernel_calls(fused_resnet)
        with torch.inference_mode():
            y = fused_resnet(x)
        torch.cuda.synchronize()
        return y, _kernel_calls(fused_resnet) - before

    on, calls_on = forward("1")
    again, _ = forward("1")
    off, calls_off = forward("0")
    assert calls_off == 0
    # 224x224 runs the served shapes, 15 of its 16 bottleneck 3x3 convs
    # being in the dispatch table; at 64x64 every plane is outside it and
    # the model falls back throughout
    assert calls_on == (15 if size == 224 else 0)
    assert torch.equal(on, again)
    assert on.float().std().item() > 0
    diff = (on.float() - off.float()).abs().max().item()
    print(f"size {size}: max |on - off| = {diff:.4f}")
    assert torch.allclose(on.float(), off.float(), atol=0.15, rtol=0.05), diff


def test_module_under_graph_capture():
    """Captured into a hipGraph and replayed twice, the module gives the
    eager result (the weights are packed by the eager warm-up call,
    before capture)."""
    import torch

    from client_amd.models.resnet import BiasAct, Conv3x3BiasAct

    torch.manual_seed(13)
    conv = torch.nn.Conv2d(128, 128, 3, padding=1, bias=False).to(
        "cuda", torch.bfloat16)
    ba = BiasAct(torch.randn(128), relu=True).to("cuda")
    mod = Conv3x3BiasAct()
    x = torch.randn(3, 128, 28, 28, device="cuda", dtype=torch.bfloat16)
    assert Conv3x3BiasAct.eligible(x, conv)
    with torch.inference_mode():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = mod(x, conv, ba).clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = mod(x, conv, ba)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
        # new input, same graph
        x.copy_(torch.randn_like(x))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, mod(x, conv, ba))
