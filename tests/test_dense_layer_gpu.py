"""The two DenseNet dense-layer kernels (dense_layer.hip) against float64
references computed with torch on the CPU, and the fused model against the
textbook module (require an MI355X)."""

import copy

import pytest

pytestmark = pytest.mark.gpu

# Kernel A: (N, C, C_buf, K, H, W, bias and ReLU). The last case is the
# wide tile: c1_plan takes 128 columns once ceil(N*3136/128) * (K/64) >=
# 512, that is from N = 11 on (test_plans_take_the_paths_the_cases_name).
A_CASES = [
    (1, 32, 64, 64, 1, 1, True),        # one chunk, one pixel
    (3, 64, 96, 128, 7, 7, True),       # tiles spanning images, odd HW
    (2, 96, 160, 128, 4, 6, True),      # 16-byte stores across images
    (2, 992, 1024, 128, 7, 7, True),    # the longest served reduction
    (2, 256, 256, 128, 14, 14, False),  # the transition
    (11, 64, 96, 128, 56, 56, True),    # the wide tile
]
# Kernel B: (N, C, C_buf, k0, H, W). The last case is the only one with
# more than one output row per tile: the plan keeps one row until that
# leaves 256 workgroups, here 80*7/2 = 280.
B_CASES = [
    (1, 32, 96, 64, 1, 1),       # single pixel, all halo
    (3, 128, 160, 96, 7, 7),     # tiles spanning images, odd HW
    (2, 128, 96, 64, 9, 5),      # non-square plane
    (1, 128, 96, 64, 56, 56),    # the widest served row
    (2, 128, 1024, 992, 7, 7),   # the last slot of the largest buffer
    (80, 32, 32, 0, 7, 7),       # two-row tiles spanning images
]


def _ids(cases):
    return ["x".join(str(int(v)) for v in c) for c in cases]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _a_inputs(case, seed, exact):
    """CPU tensors: the buffer (channels >= C are NaN, so one read past
    the prefix poisons the output), scale, shift, weight, bias."""
    import torch

    n, c, cb, k, h, w, _ = case
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((n, cb, h, w), float("nan"), dtype=torch.bfloat16)
    if exact:
        buf[:, :c] = torch.randint(-2, 3, (n, c, h, w), generator=g).float()
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,),
                                                            generator=g)]
        shift = torch.randint(-3, 4, (c,), generator=g).float()
        wt = torch.randint(-1, 2, (k, c, 1, 1), generator=g).float()
    else:
        buf[:, :c] = torch.randn((n, c, h, w), generator=g)
        scale = torch.rand(c, generator=g) + 0.5
        shift = torch.rand(c, generator=g) - 0.5
        wt = torch.randn((k, c, 1, 1), generator=g) * 0.05
    return buf, scale, shift, wt.to(torch.bfloat16), torch.randn(k,
                                                                 generator=g)


def _run_a(buf, c, scale, shift, wt, bias, relu):
    import torch

    from client_amd.models.resnet import pack_conv1x1_weight
    from client_amd.ops import hip_runtime as hr

    n, cb, h, w = buf.shape
    k = wt.shape[0]
    d = [t.cuda() for t in (buf, scale, shift, pack_conv1x1_weight(wt))]
    b = bias.cuda() if relu else None
    out = torch.full((n, k, h, w), 7.0, device="cuda", dtype=torch.bfloat16)
    hr.dense_conv1x1_bf16(d[0].data_ptr(), cb * h * w, d[1].data_ptr(),
                          d[2].data_ptr(), d[3].data_ptr(),
                          b.data_ptr() if relu else 0, out.data_ptr(), n, c,
                          k, h, w, relu, _stream())
    torch.cuda.synchronize()
    return out.cpu()


def _a_ref64(buf, c, scale, shift, wt):
    """(conv of the exact prologue value a, conv(|a|, |w|)), float64."""
    import torch

    a = (buf[:, :c].double() * scale.double().view(1, -1, 1, 1)
         + shift.double().view(1, -1, 1, 1)).relu().flatten(2)
    w64 = wt.double().flatten(1)
    shape = (buf.shape[0], wt.shape[0], *buf.shape[2:])
    return (torch.matmul(w64, a).view(shape),
            torch.matmul(w64.abs(), a).view(shape))


@pytest.mark.parametrize("case", A_CASES, ids=_ids(A_CASES))
def test_a_exact_integer_layout(case):
    """Every intermediate is exact (scale a power of two, integer shift of
    both signs so the ReLU clips), so the output is one bit pattern."""
    import torch

    c, relu = case[1], case[6]
    buf, scale, shift, wt, bias = _a_inputs(case, 3, True)
    ref = _a_ref64(buf, c, scale, shift, wt)[0].to(torch.bfloat16)
    if relu:
        ref = (ref.float() + bias.view(1, -1, 1, 1)).relu().to(
            torch.bfloat16)
    assert torch.equal(_run_a(buf, c, scale, shift, wt, bias, relu), ref)


@pytest.mark.parametrize("case", A_CASES, ids=_ids(A_CASES))
def test_a_random_data_within_bound(case):
    """|got - ref| <= 2^-8 |ref| + (2^-8 + (C+2) 2^-24) S: one output
    rounding; one prologue rounding plus its fma; fp32 accumulation."""
    c, relu = case[1], case[6]
    buf, scale, shift, wt, bias = _a_inputs(case, 5, False)
    ref, s = _a_ref64(buf, c, scale, shift, wt)
    if relu:
        ref = (ref + bias.double().view(1, -1, 1, 1)).relu()
    err = (_run_a(buf, c, scale, shift, wt, bias, relu).double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (2.0 ** -8 + (c + 2) * 2.0 ** -24) * s
    worst = (err / bound).max().item()
    print(f"A {case}: max err/bound = {worst:.3f}")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("case", A_CASES, ids=_ids(A_CASES))
def test_a_deterministic_batch_and_stride_invariant(case):
    import torch

    n, c, relu = case[0], case[1], case[6]
    buf, scale, shift, wt, bias = _a_inputs(case, 7, False)
    a = _run_a(buf, c, scale, shift, wt, bias, relu)
    assert torch.equal(a, _run_a(buf, c, scale, shift, wt, bias, relu))
    dense = buf[:, :c].contiguous()  # C_buf = C
    assert torch.equal(a, _run_a(dense, c, scale, shift, wt, bias, relu))
    for i in sorted({0, n // 2, n - 1}):
        one = _run_a(buf[i:i + 1], c, scale, shift, wt, bias, relu)
        assert torch.equal(one[0], a[i]), i


def _b_inputs(case, seed, exact):
    import torch

    n, c, cb, k0, h, w = case
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = torch.randint(-2, 3, (n, c, h, w), generator=g).float()
        wt = torch.randint(-1, 2, (32, c, 3, 3), generator=g).float()
    else:
        x = torch.randn((n, c, h, w), generator=g)
        wt = torch.randn((32, c, 3, 3), generator=g) * 0.05
    return x.to(torch.bfloat16), wt.to(torch.bfloat16)


def _run_b(x, wt, cb, k0):
    """Returns the 32 written channels; checks that every other element
    of the sentinel-filled buffer kept its bits."""
    import torch

    from client_amd.models.resnet import pack_conv3x3_weight
    from client_amd.ops import hip_runtime as hr

    n, c, h, w = x.shape
    sent = (torch.arange(n * cb * h * w, dtype=torch.int32) % 251 + 16000
            ).to(torch.int16).view(n, cb, h, w)
    buf = sent.cuda()
    xd, wp = x.cuda(), pack_conv3x3_weight(wt).cuda()
    hr.dense_conv3x3_k32_bf16(xd.data_ptr(), wp.data_ptr(), buf.data_ptr(),
                              n, c, h, w, k0, cb * h * w, _stream())
    torch.cuda.synchronize()
    got = buf.cpu()
    sent[:, k0:k0 + 32] = got[:, k0:k0 + 32]
    assert torch.equal(got, sent), "wrote outside the slot"
    return got[:, k0:k0 + 32].contiguous().view(torch.bfloat16)


def _b_ref64(x, wt):
    import torch.nn.functional as F

    return (F.conv2d(x.double(), wt.double(), padding=1),
            F.conv2d(x.double().abs(), wt.double().abs(), padding=1))


@pytest.mark.parametrize("case", B_CASES, ids=_ids(B_CASES))
def test_b_exact_integer_layout_and_slot(case):
    import torch

    x, wt = _b_inputs(case, 3, True)
    ref = _b_ref64(x, wt)[0].to(torch.bfloat16)
    assert torch.equal(_run_b(x, wt, case[2], case[3]), ref)


@pytest.mark.parametrize("case", B_CASES, ids=_ids(B_CASES))
def test_b_random_data_within_bound(case):
    """|got - ref| <= 2^-8 |ref| + 9C 2^-24 S."""
    x, wt = _b_inputs(case, 5, False)
    ref, s = _b_ref64(x, wt)
    err = (_run_b(x, wt, case[2], case[3]).double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 9 * case[1] * 2.0 ** -24 * s
    worst = (err / bound).max().item()
    print(f"B {case}: max err/bound = {worst:.3f}")
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("case", B_CASES, ids=_ids(B_CASES))
def test_b_deterministic_batch_and_slot_invariant(case):
    import torch

    n, _, cb, k0 = case[:4]
    x, wt = _b_inputs(case, 7, False)
    a = _run_b(x, wt, cb, k0)
    assert torch.equal(a, _run_b(x, wt, cb, k0))
    assert torch.equal(a, _run_b(x, wt, cb + 32, cb))  # another slot, stride
    for i in sorted({0, n // 2, n - 1}):
        assert torch.equal(_run_b(x[i:i + 1], wt, cb, k0)[0], a[i]), i


def test_plans_take_the_paths_the_cases_name():
    from client_amd.ops import hip_runtime as hr

    def tile(n):
        return hr.dense_conv1x1_tile(n, 64, 128, 56, 56, 96 * 3136)

    assert (tile(10), tile(11)) == (64, 128)
    assert hr.dense_conv3x3_k32_rows(80, 32, 7, 7, 0, 32 * 49) == 2
    assert hr.dense_conv3x3_k32_rows(3, 128, 7, 7, 96, 160 * 49) == 1


def test_refusals_do_not_launch():
    import torch

    from client_amd.ops import hip_runtime as hr

    bf = dict(device="cuda", dtype=torch.bfloat16)
    big = torch.full((1 << 16,), 7.0, **bf)
    wp = torch.zeros((1 << 16,), **bf)
    f32 = torch.zeros(1024, device="cuda")
    n, c, k, h, w = 2, 64, 128, 4, 4
    xs = 96 * h * w
    good = dict(x=big[32768:], xs=xs, wp=wp, out=big, n=n, c=c, k=k)
    assert hr.dense_conv1x1_supported(n, c, k, h, w, xs)
    for bad in [dict(c=48), dict(c=16), dict(k=96), dict(xs=c * h * w - 2),
                dict(out=big[1:]), dict(wp=wp[1:]), dict(x=big[32769:]),
                dict(out=big[32768 + xs:]),   # inside image 1's prefix
                dict(x=big[k * h * w:])]:     # x starts inside out
        a = {**good, **bad}
        if not set(bad) & {"out", "wp", "x"}:
            assert not hr.dense_conv1x1_supported(a["n"], a["c"], a["k"], h,
                                                  w, a["xs"])
        with pytest.raises(RuntimeError):
            hr.dense_conv1x1_bf16(
                a["x"].data_ptr(), a["xs"], f32.data_ptr(), f32.data_ptr(),
                a["wp"].data_ptr(), f32.data_ptr(), a["out"].data_ptr(),
                a["n"], a["c"], a["k"], h, w, True, _stream())
    cb, k0 = 96, 64
    good = dict(x=big[32768:], wp=wp, out=big, c=128, w=w, k0=k0)
    assert hr.dense_conv3x3_k32_supported(n, 128, h, w, k0, cb * h * w)
    for bad in [dict(c=48), dict(c=16), dict(w=65), dict(k0=cb - 16),
                dict(wp=wp[1:]),
                dict(x=big[(cb + k0) * h * w + 8:])]:  # inside image 1's slot
        a = {**good, **bad}
        if not set(bad) & {"wp", "x"}:
            assert not hr.dense_conv3x3_k32_supported(
                n, a["c"], h, a["w"], a["k0"], cb * h * a["w"])
        with pytest.raises(RuntimeError):
            hr.dense_conv3x3_k32_bf16(
                a["x"].data_ptr(), a["wp"].data_ptr(), a["out"].data_ptr(),
                n, a["c"], h, a["w"], a["k0"], cb * h * a["w"], _stream())
    torch.cuda.synchronize()
    assert (big == 7.0).all()


def _randomise_bn(model):
    import torch

    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)


@pytest.mark.parametrize("blocks,size", [((2, 2, 2, 2), 64),
                                         ((6, 12, 24, 16), 224)])
def test_whole_model_against_fp32_cpu(blocks, size, monkeypatch):
    """E_fused = max|fused bf16 - ref| <= 2 E_plain, the textbook bf16
    module's own error against the same fp32 CPU reference: both paths
    take the same count of bf16 roundings (the fused one rounds the folded
    weights once more); 2 covers the spread of a max over 2000 logits."""
    import torch

    from client_amd.models.densenet import (DenseNet121, FusedDenseBlock,
                                            FusedTransition,
                                            fuse_dense_layers)

    monkeypatch.delenv("CLIENT_AMD_DENSENET_FUSED", raising=False)
    torch.manual_seed(2)
    m = DenseNet121(blocks=blocks).eval()
    _randomise_bn(m)
    x = torch.randn(2, 3, size, size)
    fused = fuse_dense_layers(copy.deepcopy(m)).to("cuda", torch.bfloat16)
    plain = copy.deepcopy(m).to("cuda", torch.bfloat16)
    xd = x.to("cuda", torch.bfloat16)
    with torch.inference_mode():
        ref = m(xd.float().cpu())
        y1, y2, yp = fused(xd), fused(xd), plain(xd)
    calls = sum(b.calls for b in fused.modules()
                if isinstance(b, (FusedDenseBlock, FusedTransition)))
    assert calls == 2 * (2 * sum(blocks) + len(blocks) - 1)  # two forwards
    assert torch.equal(y1, y2)
    e_fused = (y1.float().cpu() - ref).abs().max().item()
    e_plain = (yp.float().cpu() - ref).abs().max().item()
    print(f"{blocks} @ {size}: E_fused = {e_fused:.4f}, E_plain = "
          f"{e_plain:.4f}, ratio {e_fused / e_plain:.2f}")
    assert e_fused <= 2 * e_plain


def test_block_under_graph_capture():
    """Captured and replayed twice, then with a new input, the block gives
    the eager result (the weights are packed by the eager warm-up)."""
    import torch

    from client_amd.models.densenet import DenseLayer, FusedDenseBlock

    torch.manual_seed(13)
    layers = [DenseLayer(64, 32).eval(), DenseLayer(96, 32).eval()]
    for layer in layers:
        _randomise_bn(layer)
    block = FusedDenseBlock(layers)
    x = torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = block(x).clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = block(x)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
        x.copy_(torch.randn_like(x))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, block(x))
        assert block.calls == 4 * 3
