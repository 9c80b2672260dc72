"""The channels-last (NHWC) ResNet epilogue path from the kernel up:
bias_res_act_cl_bf16 against the fp32 CPU reference, which kernel
BiasAct / BiasResAct pick for which input, the whole fused ResNet50 in
channels-last, and TorchModel with CLIENT_AMD_CHANNELS_LAST=1 (require
an MI355X)."""

import copy

import pytest

import epilogue_refs as er

pytestmark = pytest.mark.gpu

# (N, C, H, W) of NHWC-contiguous tensors: one vector in total; c0
# always 0; c0 cycling 0, 8, 16 with C no power of two; two served
# shapes; and 4,276,800 elements, more than one sweep of the
# 2048 x 256 x 8 grid (4,194,304 mod 264 = 136, so a lane's channel
# offset changes from the first sweep to the second)
CL_SHAPES = [
    (1, 8, 1, 1),
    (2, 8, 3, 5),
    (3, 24, 5, 7),
    (4, 64, 7, 7),
    (4, 2048, 7, 7),
    (2, 264, 90, 90),
]
IDS = ["x".join(map(str, s)) for s in CL_SHAPES]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _nhwc_cuda(t):
    """A CPU NCHW tensor as NHWC memory on the GPU, viewed as NCHW."""
    return t.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


def _cl_launch(x, res, bias, out, relu, n=None, channels=None):
    from client_amd.ops import hip_runtime as hr

    hr.bias_res_act_cl_bf16(
        x if isinstance(x, int) else x.data_ptr(),
        0 if res is None else (res if isinstance(res, int)
                               else res.data_ptr()),
        bias.data_ptr(),
        out if isinstance(out, int) else out.data_ptr(),
        x.numel() if n is None else n,
        bias.numel() if channels is None else channels, relu, _stream())


# ---------------------------------------------------------------------------
# the kernel, called directly
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("shape", CL_SHAPES, ids=IDS)
def test_cl_kernel_bit_exact(shape):
    """ReLU on and off, residual present and absent, in place and out
    of place into a pre-filled tensor (the source then stays as it
    was)."""
    import torch

    gen = torch.Generator().manual_seed(23)
    x_cpu = torch.randn(shape, generator=gen).to(torch.bfloat16)
    r_cpu = torch.randn(shape, generator=gen).to(torch.bfloat16)
    b_cpu = torch.randn(shape[1], generator=gen)
    x, r, bias = _nhwc_cuda(x_cpu), _nhwc_cuda(r_cpu), b_cpu.cuda()
    for relu in (False, True):
        for res_cpu, res in ((None, None), (r_cpu, r)):
            ref = er.epilogue_ref(x_cpu, res_cpu, b_cpu, relu)
            for inplace in (False, True):
                src = x.clone()
                assert src.stride() == x.stride()
                dst = src if inplace else torch.full_like(x, 7.0)
                _cl_launch(src, res, bias, dst, relu)
                torch.cuda.synchronize()
                er.assert_bits_equal(dst, ref,
                                     (relu, res is not None, inplace))
                if not inplace:
                    assert torch.equal(src, x)


@pytest.mark.parametrize("shape", [s for s in CL_SHAPES if s[1] <= 256],
                         ids=[i for s, i in zip(CL_SHAPES, IDS)
                              if s[1] <= 256])
def test_cl_kernel_exact_channel_layout(shape):
    """x = 0 and bias[c] = c (exact in bf16): the output, viewed as
    NCHW, is the channel index everywhere."""
    import torch

    n, c, h, w = shape
    x = _nhwc_cuda(torch.zeros(shape, dtype=torch.bfloat16))
    bias = torch.arange(c, dtype=torch.float32).cuda()
    out = torch.full_like(x, 7.0)
    _cl_launch(x, None, bias, out, False)
    torch.cuda.synchronize()
    want = torch.arange(c, dtype=torch.float32).view(1, c, 1, 1).expand(shape)
    assert torch.equal(out.float().cpu(), want)


def test_cl_kernel_argument_checks():
    """channels % 8 != 0 and pointers off 16-byte alignment raise and
    write nothing; n = 0 returns without writing."""
    import torch

    n_el = 2 * 24 * 3 * 5  # (2, 24, 3, 5)
    # 8 spare elements behind each tensor so data_ptr() + 2 stays inside
    bufs = [torch.full((n_el + 8,), v, device="cuda", dtype=torch.bfloat16)
            for v in (1.0, 2.0, 7.0)]
    x, r, out = bufs
    bias = torch.ones(24, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 7.0).all()) and bool((x == 1.0).all())

    for kwargs in (
        dict(x=x.data_ptr(), res=r.data_ptr(), out=out.data_ptr(),
             channels=12),
        dict(x=x.data_ptr() + 2, res=r.data_ptr(), out=out.data_ptr()),
        dict(x=x.data_ptr(), res=r.data_ptr() + 2, out=out.data_ptr()),
        dict(x=x.data_ptr(), res=r.data_ptr(), out=out.data_ptr() + 2),
        dict(x=x.data_ptr() + 2, res=None, out=out.data_ptr()),
        dict(x=x.data_ptr(), res=None, out=out.data_ptr() + 2),
    ):
        channels = kwargs.pop("channels", 24)
        with pytest.raises(RuntimeError):
            _cl_launch(kwargs["x"], kwargs["res"], bias, kwargs["out"], True,
                       n=n_el, channels=channels)
        assert untouched(), kwargs

    _cl_launch(x.data_ptr(), r.data_ptr(), bias, out.data_ptr(), True, n=0,
               channels=24)
    assert untouched()
    # and the valid call still works on these buffers
    _cl_launch(x.data_ptr(), r.data_ptr(), bias, out.data_ptr(), True,
               n=n_el, channels=24)
    torch.cuda.synchronize()
    assert bool((out[:n_el] == 4.0).all()) and bool((out[n_el:] == 7.0).all())


# ---------------------------------------------------------------------------
# module dispatch
# ---------------------------------------------------------------------------


@pytest.fixture
def counted(monkeypatch):
    """Counting wrappers round the extension's three epilogue entry
    points; the cl kernel is counted by caller kind (no residual:
    BiasAct, residual: BiasResAct)."""
    from client_amd.ops import hip_runtime as hr

    mod = hr._load()
    counts = {"bias_act_bf16": 0, "bias_res_act_bf16": 0, "cl_act": 0,
              "cl_res": 0}

    def wrap(name, key_of):
        real = getattr(mod, name)

        def counting(*args, **kwargs):
            counts[key_of(args)] += 1
            return real(*args, **kwargs)

        monkeypatch.setattr(mod, name, counting)

    wrap("bias_act_bf16", lambda a: "bias_act_bf16")
    wrap("bias_res_act_bf16", lambda a: "bias_res_act_bf16")
    wrap("bias_res_act_cl_bf16", lambda a: "cl_res" if a[1] else "cl_act")
    return counts


def _dispatch_inputs():
    """name -> (make(t) placing a CPU NCHW tensor for x, the same for
    the residual, expected path)"""
    import torch

    cl = torch.channels_last

    def nchw(t):
        return t.cuda()

    def nhwc(t):
        return t.cuda().contiguous(memory_format=cl)

    def sliced(t):
        big = torch.cat([t, t], 1).cuda()
        return big[:, :t.shape[1]]

    return {
        "nchw": ((2, 16, 5, 7), torch.bfloat16, nchw, nchw, "nchw"),
        "nhwc": ((2, 16, 5, 7), torch.bfloat16, nhwc, nhwc, "cl"),
        "nhwc_c12": ((2, 12, 5, 7), torch.bfloat16, nhwc, nhwc, "torch"),
        "nhwc_res_nchw": ((2, 16, 5, 7), torch.bfloat16, nhwc, nchw, "torch"),
        "nchw_res_nhwc": ((2, 16, 5, 7), torch.bfloat16, nchw, nhwc, "torch"),
        "slice": ((2, 16, 5, 7), torch.bfloat16, sliced, nchw, "torch"),
        "fp16": ((2, 16, 5, 7), torch.float16, nchw, nchw, "torch"),
        "fp32": ((2, 16, 5, 7), torch.float32, nhwc, nhwc, "torch"),
        # contiguous in both senses, whichever strides it carries
        "1x1": ((2, 16, 1, 1), torch.bfloat16, nchw, nchw, "nchw"),
        "1x1_cl_strides": ((2, 16, 1, 1), torch.bfloat16, nhwc, nhwc, "nchw"),
    }


DISPATCH = ["nchw", "nhwc", "nhwc_c12", "nhwc_res_nchw", "nchw_res_nhwc",
            "slice", "fp16", "fp32", "1x1", "1x1_cl_strides"]
# the two mixed-format kinds need a residual to disagree with
DISPATCH_CASES = [(k, m) for k in DISPATCH
                  for m in ("act_relu", "act_linear", "res")
                  if m == "res" or "_res_" not in k]


@pytest.mark.parametrize("kind,module", DISPATCH_CASES,
                         ids=[f"{k}-{m}" for k, m in DISPATCH_CASES])
def test_module_dispatch(kind, module, counted):
    """Which path BiasAct / BiasResAct take for which input, and what
    it returns: the kernels give the fp32 reference bit for bit, in
    place and in the input's memory format; everything else gives the
    documented torch sequence."""
    import torch

    from client_amd.models.resnet import BiasAct, BiasResAct

    shape, dtype, make_x, make_r, path = _dispatch_inputs()[kind]
    if module != "res":
        make_r = None
    gen = torch.Generator().manual_seed(29)
    x_cpu = torch.randn(shape, generator=gen).to(dtype)
    r_cpu = torch.randn(shape, generator=gen).to(dtype)
    b_cpu = torch.randn(shape[1], generator=gen)
    relu = module != "act_linear"
    if module == "res":
        m = BiasResAct(b_cpu).cuda()
    else:
        m = BiasAct(b_cpu, relu=relu).cuda()
    x = make_x(x_cpu)
    r = make_r(r_cpu) if make_r else None
    assert torch.equal(x.cpu(), x_cpu)
    strides = x.stride()
    if kind == "nhwc":
        assert not x.is_contiguous()
    if kind == "slice":
        assert not x.is_contiguous()
        assert not x.is_contiguous(memory_format=torch.channels_last)

    got = m(x, r) if module == "res" else m(x)
    torch.cuda.synchronize()

    nchw_name = "bias_res_act_bf16" if module == "res" else "bias_act_bf16"
    cl_name = "cl_res" if module == "res" else "cl_act"
    want_counts = dict.fromkeys(counted, 0)
    if path == "nchw":
        want_counts[nchw_name] = 1
    elif path == "cl":
        want_counts[cl_name] = 1
    assert counted == want_counts

    if path == "torch":
        bias = m.bias.view(1, -1, 1, 1).to(dtype)
        want = x + r + bias if module == "res" else x + bias
        if relu:
            want = want.relu()
        assert got is not x
        assert got.dtype == dtype
        assert torch.equal(got, want)
        assert torch.equal(x.cpu(), x_cpu)
    else:
        assert got is x
        assert got.stride() == strides
        ref = er.epilogue_ref(x_cpu, r_cpu if module == "res" else None,
                              b_cpu, relu)
        er.assert_bits_equal(got, ref, (kind, module))
        if r is not None:
            assert torch.equal(r.cpu(), r_cpu)


# ---------------------------------------------------------------------------
# whole model in channels-last
# ---------------------------------------------------------------------------


def _formula(x, r, bias, relu):
    """The reference formula on the device (fp32, then bf16)."""
    import torch

    ref = x.float()
    if r is not None:
        ref = ref + r.float()
    ref = ref + bias.float().view(1, -1, 1, 1)
    if relu:
        ref = ref.relu()
    return ref.to(torch.bfloat16)


@pytest.fixture(scope="module")
def resnets():
    """The recipe of test_flat_epilogue_gpu.py's fused_resnet, as the
    plain folded fp32 model, the fused bf16 model in NCHW and the fused
    bf16 model in channels-last."""
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
    plain = fold_batchnorm(copy.deepcopy(m), fuse_eltwise=False).to("cuda")
    nchw = fold_batchnorm(copy.deepcopy(m), fuse_eltwise=True).to(
        "cuda", torch.bfloat16)
    nhwc = fold_batchnorm(m, fuse_eltwise=True).to(
        "cuda", torch.bfloat16).to(memory_format=torch.channels_last)
    return plain, nchw, nhwc


def _conv3x3_calls(model):
    from client_amd.models.resnet import Conv3x3BiasAct

    return sum(m.calls for m in model.modules()
               if isinstance(m, Conv3x3BiasAct))


@pytest.mark.parametrize("size", [64, 224])
def test_channels_last_resnet_bit_exact_vs_torch_formulas(resnets, size,
                                                          counted,
                                                          monkeypatch):
    """Logits of the channels-last fused ResNet50 equal those of the
    same model with every epilogue and the stem computed by the fp32
    torch formulas, and the cl kernel ran once for every BiasAct and
    every BiasResAct of the model.

    The call counts are what rules out a fallback for BiasAct: the
    model's bias buffers went through .to(bfloat16), so the torch
    sequence x + bias.to(bf16) gives the same bits as the fp32 formula
    there; only for BiasResAct (two bf16 adds) does a fallback break
    the equality. The stem's BiasReluMaxPool has no channels-last
    kernel and takes its documented torch sequence here, which is
    bit-identical for the same reason. cudnn.deterministic: see
    test_flat_epilogue_gpu.py."""
    import torch
    import torch.nn.functional as F

    from client_amd.models import resnet

    _, _, model = resnets
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(size)
    x = torch.randn(2, 3, size, size, device="cuda", dtype=torch.bfloat16
                    ).contiguous(memory_format=torch.channels_last)
    before = _conv3x3_calls(model)
    with torch.inference_mode():
        got = model(x)
    torch.cuda.synchronize()
    n_act = sum(isinstance(m, resnet.BiasAct) for m in model.modules())
    assert n_act == 32  # two per bottleneck
    assert counted["cl_act"] == n_act, counted
    assert counted["cl_res"] == 16  # every bottleneck exit
    assert counted["bias_act_bf16"] == 0, counted
    assert counted["bias_res_act_bf16"] == 0, counted
    assert _conv3x3_calls(model) == before == 0

    def bias_act_ref(self, t):
        return _formula(t, None, self.bias, self.relu_flag)

    def bias_res_act_ref(self, t, residual):
        return _formula(t, residual, self.bias, True)

    def stem_ref(self, t):
        return F.max_pool2d(_formula(t, None, self.bias, True), 3, 2, 1)

    monkeypatch.setattr(resnet.BiasAct, "forward", bias_act_ref)
    monkeypatch.setattr(resnet.BiasResAct, "forward", bias_res_act_ref)
    monkeypatch.setattr(resnet.BiasReluMaxPool, "forward", stem_ref)
    with torch.inference_mode():
        ref = model(x)
    torch.cuda.synchronize()
    assert isinstance(model.bn1, resnet.BiasReluMaxPool)
    assert ref.std().item() > 0
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max()


@pytest.mark.parametrize("size", [64, 224])
def test_channels_last_resnet_as_accurate_as_nchw(resnets, size):
    """Max abs logit error against the plain folded fp32 model: the
    channels-last fused bf16 run may be at most twice as far off as the
    NCHW fused bf16 run (the same arithmetic behind other library conv
    solvers; the margin of the fp8-weights accuracy test)."""
    import torch

    plain, nchw, nhwc = resnets
    torch.manual_seed(size + 1)
    x = torch.randn(2, 3, size, size, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        want = plain(x.float())
        a = nchw(x.clone())
        b = nhwc(x.contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    err_nchw = (a.float() - want).abs().max().item()
    err_nhwc = (b.float() - want).abs().max().item()
    print(f"size {size}: max abs logit error vs fp32: NCHW {err_nchw:.5f}, "
          f"NHWC {err_nhwc:.5f}, logit std {want.std().item():.4f}")
    assert err_nchw > 0
    assert err_nhwc <= 2 * err_nchw, (err_nhwc, err_nchw)


# ---------------------------------------------------------------------------
# served path
# ---------------------------------------------------------------------------


def _small_net():
    import torch
    import torch.nn as nn

    from client_amd.models.resnet import Bottleneck, fold_batchnorm

    class SmallNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 64, 3, padding=1, bias=False)
            self.bn1 = nn.BatchNorm2d(64)
            self.relu = nn.ReLU(inplace=True)
            down = nn.Sequential(nn.Conv2d(64, 64, 1, bias=False),
                                 nn.BatchNorm2d(64))
            self.layer = nn.Sequential(Bottleneck(64, 16, 1, down),
                                       Bottleneck(64, 16))

        def forward(self, x):
            return self.layer(self.relu(self.bn1(self.conv1(x))))

    torch.manual_seed(31)
    m = SmallNet().eval()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)
    return fold_batchnorm(m, fuse_eltwise=True)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_torch_model_channels_last(use_graph, counted, monkeypatch):
    """TorchModel with CLIENT_AMD_CHANNELS_LAST=1: two different NCHW
    inputs come out as from the module called eagerly, through the cl
    kernel; with the graph, the second input replays the capture."""
    import torch

    from client_amd.models import resnet
    from client_amd.server.models import TorchModel

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setenv("CLIENT_AMD_CHANNELS_LAST", "1")
    net = _small_net()
    assert isinstance(net.bn1, resnet.BiasAct)
    assert all(isinstance(b, resnet.FusedBottleneck) for b in net.layer)
    tm = TorchModel("small", net, [("INPUT0", "BF16", (-1, 3, 16, 16))],
                    [("OUTPUT0", "BF16", (-1, 64, 16, 16))],
                    device="cuda:0", dtype=torch.bfloat16,
                    use_graph=use_graph)
    assert tm._channels_last and tm.use_graph == use_graph

    gen = torch.Generator().manual_seed(37)
    xs = [torch.randn(2, 3, 16, 16, generator=gen).to(torch.bfloat16).cuda()
          for _ in range(2)]
    assert all(t.is_contiguous() for t in xs)
    with torch.inference_mode():
        want = [tm.module(t.clone()).clone() for t in xs]
    torch.cuda.synchronize()
    assert not torch.equal(want[0], want[1])
    eager_calls = dict(counted)
    per_forward = (eager_calls["cl_act"] + eager_calls["cl_res"]) // 2
    assert eager_calls["cl_act"] == 2 * 5 and eager_calls["cl_res"] == 2 * 2
    assert eager_calls["bias_act_bf16"] == 0
    assert eager_calls["bias_res_act_bf16"] == 0

    out0 = tm._execute_direct([xs[0].clone()])[0]
    torch.cuda.synchronize()
    after_first = dict(counted)
    out1 = tm._execute_direct([xs[1].clone()])[0]
    torch.cuda.synchronize()
    after_second = dict(counted)
    assert torch.equal(out0, want[0])
    assert torch.equal(out1, want[1])
    assert after_second["bias_act_bf16"] == 0
    assert after_second["bias_res_act_bf16"] == 0

    def cl(c):
        return c["cl_act"] + c["cl_res"]

    assert cl(after_first) > cl(eager_calls)
    if use_graph:
        assert len(tm._graphs) == 1
        entry = next(iter(tm._graphs.values()))
        assert entry != "eager"
        # the replay launches no kernel from Python
        assert after_second == after_first
    else:
        assert not tm._graphs
        assert cl(after_second) - cl(after_first) == per_forward
