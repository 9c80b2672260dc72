"""ResNet-50 (v1.5) for the benchmark server.

The BASELINE north-star metric is perf_analyzer-style inferences/sec on
ResNet50 bs=8 with HIP-shm I/O. torchvision is not in
this image, so the standard architecture is defined here directly
(random-init weights; the benchmark uses synthetic inputs).
"""

import os

import torch.nn as nn


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch, width, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(in_ch, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1,
                               bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, width * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(width * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class ResNet50(nn.Module):
    def __init__(self, num_classes=1000):
        super().__init__()
        self.in_ch = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, 3)
        self.layer2 = self._make_layer(128, 4, stride=2)
        self.layer3 = self._make_layer(256, 6, stride=2)
        self.layer4 = self._make_layer(512, 3, stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)

    def _make_layer(self, width, blocks, stride=1):
        downsample = None
        out_ch = width * Bottleneck.expansion
        if stride != 1 or self.in_ch != out_ch:
            downsample = nn.Sequential(
                nn.Conv2d(self.in_ch, out_ch, 1, stride=stride, bias=False),
                nn.BatchNorm2d(out_ch),
            )
        layers = [Bottleneck(self.in_ch, width, stride, downsample)]
        self.in_ch = out_ch
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.in_ch, width))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        x = self.avgpool(x).flatten(1)
        return self.fc(x)


class BiasAct(nn.Module):
    """Per-channel bias (+optional ReLU) as one CDNA4 kernel pass.

    torch-on-ROCm emits a separate elementwise kernel for conv bias
    (miopen_convolution has no bias epilogue), so after BN folding the
    bias costs a full extra memory pass. Round-2 lever, gated by
    CLIENT_AMD_FUSED_BIAS=1 (kernel numerics are GPU-tested; default
    path keeps bias on the conv)."""

    def __init__(self, bias, relu=False):
        super().__init__()
        self.register_buffer("bias", bias.detach().float())
        self.relu_flag = relu

    def forward(self, x):
        import torch

        if x.is_cuda and x.dtype == torch.bfloat16:
            from ..ops import hip_runtime as hr

            if self.bias.dtype != torch.float32:
                # TorchModel's .to(bf16) sweeps buffers too; the kernel
                # reads fp32 bias — normalize once (pre-capture, the
                # eager warmup hits this before any hipGraph capture)
                self.bias.data = self.bias.data.float()

            c = x.shape[1]
            if x.is_contiguous():
                n = x.shape[0]
                plane = x.numel() // (n * c)
                hr.bias_act_bf16(
                    x.data_ptr(), self.bias.data_ptr(), x.data_ptr(),
                    n * c, plane, c, self.relu_flag,
                    torch.cuda.current_stream().cuda_stream)
                return x
            if (x.dim() == 4 and c % 8 == 0
                    and x.is_contiguous(
                        memory_format=torch.channels_last)):
                # NHWC memory: channel is the fastest dim — the cl
                # kernel keeps the fusion on MIOpen's native layout
                hr.bias_res_act_cl_bf16(
                    x.data_ptr(), 0, self.bias.data_ptr(), x.data_ptr(),
                    x.numel(), c, self.relu_flag,
                    torch.cuda.current_stream().cuda_stream)
                return x
        out = x + self.bias.view(1, -1, *([1] * (x.dim() - 2))).to(x.dtype)
        return out.relu_() if self.relu_flag else out


class BiasReluMaxPool(nn.Module):
    """ResNet stem epilogue: per-channel bias + ReLU + 3x3 stride-2
    pad-1 max-pool as ONE CDNA4 kernel pass over the biasless conv
    output. Separately this is a bias+ReLU pass that reads and writes
    the 64x112x112 map and torch's NCHW max-pool reading it again; the
    fused kernel reads it once and writes only the pooled map, with
    every element computed as BiasAct does (fp32 add, ReLU, RNE to
    bf16), so the result is bit-identical.

    Falls back to the torch sequence on CPU, for non-bf16 or
    non-contiguous input, and when CLIENT_AMD_FUSED_BIAS=0."""

    def __init__(self, bias):
        super().__init__()
        self.register_buffer("bias", bias.detach().float())

    def forward(self, x):
        import torch
        import torch.nn.functional as F

        if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
                and x.is_contiguous()
                and os.environ.get("CLIENT_AMD_FUSED_BIAS", "1") != "0"):
            from ..ops import hip_runtime as hr

            if self.bias.dtype != torch.float32:
                # TorchModel's .to(bf16) sweeps buffers; kernel reads fp32
                self.bias.data = self.bias.data.float()
            n, c, h, w = x.shape
            out = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1),
                              device=x.device, dtype=x.dtype)
            hr.bias_relu_maxpool_bf16(
                x.data_ptr(), self.bias.data_ptr(), out.data_ptr(), n * c,
                c, h, w, torch.cuda.current_stream().cuda_stream)
            return out
        out = x + self.bias.view(1, -1, *([1] * (x.dim() - 2))).to(x.dtype)
        return F.max_pool2d(out.relu_(), 3, 2, 1)


class BiasResAct(nn.Module):
    """Bottleneck-exit fusion: out = relu(x + bias[c] + residual) in ONE
    CDNA4 kernel pass. After BN folding torch-on-ROCm runs this as three
    separate elementwise kernels (bias add, residual add, relu) — three
    full memory passes over the activation per block
    (profiles/serving_rocprof_postfold_r01.txt). fp32 math in-kernel,
    RNE back to bf16."""

    def __init__(self, bias):
        super().__init__()
        self.register_buffer("bias", bias.detach().float())

    def forward(self, x, residual):
        import torch

        if (x.is_cuda and x.dtype == torch.bfloat16
                and residual.dtype == torch.bfloat16):
            from ..ops import hip_runtime as hr

            if self.bias.dtype != torch.float32:
                # TorchModel's .to(bf16) sweeps buffers; kernel reads fp32
                self.bias.data = self.bias.data.float()
            c = x.shape[1]
            if x.is_contiguous() and residual.is_contiguous():
                n = x.shape[0]
                plane = x.numel() // (n * c)
                hr.bias_res_act_bf16(
                    x.data_ptr(), residual.data_ptr(),
                    self.bias.data_ptr(), x.data_ptr(), n * c, plane, c,
                    True, torch.cuda.current_stream().cuda_stream)
                return x
            cl = torch.channels_last
            if (x.dim() == 4 and c % 8 == 0
                    and x.is_contiguous(memory_format=cl)
                    and residual.is_contiguous(memory_format=cl)):
                hr.bias_res_act_cl_bf16(
                    x.data_ptr(), residual.data_ptr(),
                    self.bias.data_ptr(), x.data_ptr(), x.numel(), c,
                    True, torch.cuda.current_stream().cuda_stream)
                return x
        out = x + residual + self.bias.view(
            1, -1, *([1] * (x.dim() - 2))
        ).to(x.dtype)
        return out.relu_()


# (C_in, C_out, H, W, stride) of the 3x3 convs that run on the fused
# conv3x3 kernel: the shapes at which it beat conv2 -> BiasAct at batch 8
# and batch 32 (scripts/bench_conv3x3.py; docs/PERFORMANCE.md). Every
# other shape keeps the library conv and the BiasAct pass; so does
# 512 @ 14x14 stride 2, which the kernel runs 40 % faster at batch 32
# but no faster at batch 8 (56 workgroups).
CONV3X3_TABLE = frozenset({
    (64, 64, 56, 56, 1),
    (128, 128, 56, 56, 2),
    (128, 128, 28, 28, 1),
    (256, 256, 28, 28, 2),
    (256, 256, 14, 14, 1),
    (512, 512, 7, 7, 1),
})


def pack_conv3x3_weight(weight):
    """[K, C, 3, 3] -> [3, 3, C/16, K, 16] contiguous: the order in which
    the conv3x3 kernel's MFMA A fragments (32 output channels x 16 input
    channels of one tap) are 1 KB contiguous runs."""
    k, c = weight.shape[:2]
    return (weight.detach().reshape(k, c // 16, 16, 3, 3)
            .permute(3, 4, 1, 0, 2).contiguous())


class Conv3x3BiasAct(nn.Module):
    """conv2 -> BiasAct of a bottleneck as ONE CDNA4 kernel: 3x3 conv
    (pad 1, stride 1 or 2) on the matrix cores reading and writing NCHW,
    with the bias + ReLU epilogue applied from the accumulators. The
    library path wraps each of these convs in NCHW<->NHWC transposes of
    input, output and (every call) weights, accumulates split-K partial
    sums with atomics in a zeroed fp32 workspace, casts it back, and is
    followed by the BiasAct pass.

    The module owns no parameters: it is handed the bottleneck's conv2
    and ba2, and keeps the weights repacked for the kernel in a device
    buffer keyed on the weight's storage and version, built on the first
    GPU call (before hipGraph capture: the eager warm-up passes run
    first). `eligible` says whether a call can take the kernel; the
    caller falls back to conv2 -> ba2 otherwise."""

    def __init__(self):
        super().__init__()
        self._packed = None
        self._key = None
        self.calls = 0  # kernel launches (tests assert it really ran)

    @staticmethod
    def eligible(x, conv):
        import torch

        if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
                and x.is_contiguous()):
            return False
        if (os.environ.get("CLIENT_AMD_FUSED_BIAS", "1") == "0"
                or os.environ.get("CLIENT_AMD_CONV3X3", "1") == "0"):
            return False
        w = conv.weight
        if not (conv.bias is None and conv.kernel_size == (3, 3)
                and conv.padding == (1, 1) and conv.dilation == (1, 1)
                and conv.groups == 1 and conv.stride in ((1, 1), (2, 2))
                and conv.padding_mode == "zeros"
                and w.dtype == torch.bfloat16 and w.device == x.device):
            return False
        return (w.shape[1], w.shape[0], x.shape[2], x.shape[3],
                conv.stride[0]) in CONV3X3_TABLE

    def _weights(self, w):
        try:
            version = w._version
        except RuntimeError:  # inference tensors track no version
            version = 0
        key = (w.data_ptr(), version)
        if self._key != key:
            self._packed = pack_conv3x3_weight(w)
            self._key = key
        return self._packed

    def forward(self, x, conv, ba):
        import torch

        from ..ops import hip_runtime as hr

        if ba.bias.dtype != torch.float32:
            # TorchModel's .to(bf16) sweeps buffers; kernel reads fp32
            ba.bias.data = ba.bias.data.float()
        n, c, h, w = x.shape
        k = conv.weight.shape[0]
        s = conv.stride[0]
        out = torch.empty((n, k, (h - 1) // s + 1, (w - 1) // s + 1),
                          device=x.device, dtype=x.dtype)
        hr.conv3x3_bias_act_bf16(
            x.data_ptr(), self._weights(conv.weight).data_ptr(),
            ba.bias.data_ptr(), out.data_ptr(), n, c, k, h, w, s,
            ba.relu_flag, torch.cuda.current_stream().cuda_stream)
        self.calls += 1
        return out


class FusedBottleneck(nn.Module):
    """Bottleneck with BN folded into the convs and every elementwise
    epilogue fused into one-pass CDNA4 kernels:

        conv1 -> BiasAct(relu)     1 pass  (was bias add + relu = 2)
        conv2 -> BiasAct(relu)     1 pass; one Conv3x3BiasAct kernel for
                                   the shapes in CONV3X3_TABLE
                                   (CLIENT_AMD_CONV3X3=0 disables)
        conv3 (biasless), identity = downsample conv (biasless) or x
              -> BiasResAct        1 pass  (was bias [+ds bias] + add
                                            + relu = 3-4 passes)

    The downsample conv's folded bias is per-channel on the same C as
    conv3's, so it is pre-summed into the exit bias."""

    def __init__(self, conv1, ba1, conv2, ba2, conv3, ds_conv, exit_bias):
        super().__init__()
        self.conv1, self.ba1 = conv1, ba1
        self.conv2, self.ba2 = conv2, ba2
        self.conv3 = conv3
        self.ds_conv = ds_conv
        self.exit = BiasResAct(exit_bias)
        self.conv3x3 = Conv3x3BiasAct()

    def forward(self, x):
        identity = self.ds_conv(x) if self.ds_conv is not None else x
        out = self.ba1(self.conv1(x))
        if Conv3x3BiasAct.eligible(out, self.conv2):
            out = self.conv3x3(out, self.conv2, self.ba2)
        else:
            out = self.ba2(self.conv2(out))
        out = self.conv3(out)
        return self.exit(out, identity)


def _strip_bias(conv):
    bias = conv.bias.detach().clone()
    conv.bias = None
    return bias


def _is_stem_pool(pool):
    """True for the 3x3 stride-2 pad-1 max-pool BiasReluMaxPool fuses."""
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    return (isinstance(pool, nn.MaxPool2d)
            and pair(pool.kernel_size) == (3, 3)
            and pair(pool.stride) == (2, 2)
            and pair(pool.padding) == (1, 1)
            and pair(pool.dilation) == (1, 1)
            and not pool.ceil_mode and not pool.return_indices)


def fold_batchnorm(module, fuse_eltwise=None):
    """Fold every Conv2d -> BatchNorm2d pair into the conv weights
    (algebraically exact in eval mode: W' = W*g/sqrt(v+eps),
    b' = b0*g/sqrt(v+eps) + beta - g*mean/sqrt(v+eps)). The serving
    profile showed BN kernels at ~29% of ResNet50 kernel time
    (profiles/serving_rocprof_r01.txt); folding removes them entirely.

    fuse_eltwise=True additionally rewrites every Bottleneck as a
    FusedBottleneck and the stem bias+relu+maxpool as one
    BiasReluMaxPool pass (standing in the bn1 slot; relu and maxpool
    become Identity), so the folded conv biases never run as separate
    torch elementwise kernels
    (default; CLIENT_AMD_FUSED_BIAS=0 disables). Pairs are detected by
    _modules adjacency (conv immediately followed by its BN, matching
    this file and torchvision layouts)."""
    from torch.nn.utils.fusion import fuse_conv_bn_eval

    if fuse_eltwise is None:
        fuse_eltwise = os.environ.get("CLIENT_AMD_FUSED_BIAS", "1") != "0"

    def fuse_pair(conv, bn):
        return fuse_conv_bn_eval(conv.eval(), bn.eval())

    if fuse_eltwise:
        # bottlenecks -> FusedBottleneck
        for m in list(module.modules()):
            for name, block in list(m._modules.items()):
                if not isinstance(block, Bottleneck):
                    continue
                c1 = fuse_pair(block.conv1, block.bn1)
                c2 = fuse_pair(block.conv2, block.bn2)
                c3 = fuse_pair(block.conv3, block.bn3)
                ba1 = BiasAct(_strip_bias(c1), relu=True)
                ba2 = BiasAct(_strip_bias(c2), relu=True)
                exit_bias = _strip_bias(c3)
                ds_conv = None
                if block.downsample is not None:
                    ds_conv = fuse_pair(block.downsample[0],
                                        block.downsample[1])
                    exit_bias = exit_bias + _strip_bias(ds_conv)
                m._modules[name] = FusedBottleneck(
                    c1, ba1, c2, ba2, c3, ds_conv, exit_bias
                )
        # stem: conv1+bn1+relu+maxpool -> biasless conv + one
        # BiasReluMaxPool pass in the bn1 slot (one BiasAct(relu) pass
        # and the model's own pool when the pool is not 3x3/s2/p1)
        if (isinstance(getattr(module, "conv1", None), nn.Conv2d)
                and isinstance(getattr(module, "bn1", None),
                               nn.BatchNorm2d)):
            fused = fuse_pair(module.conv1, module.bn1)
            module.conv1 = fused
            if (isinstance(getattr(module, "relu", None), nn.ReLU)
                    and _is_stem_pool(getattr(module, "maxpool", None))):
                module.bn1 = BiasReluMaxPool(_strip_bias(fused))
                module.maxpool = nn.Identity()
            else:
                module.bn1 = BiasAct(_strip_bias(fused), relu=True)
            module.relu = nn.Identity()

    # generic pass folds any remaining conv->bn adjacency (stem when
    # fuse_eltwise is off, custom models)
    for m in list(module.modules()):
        names = list(m._modules.keys())
        for a, b in zip(names, names[1:]):
            conv, bn = m._modules[a], m._modules[b]
            if isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d):
                m._modules[a] = fuse_pair(conv, bn)
                m._modules[b] = nn.Identity()
    return module


def resnet50(fold_bn=True):
    model = ResNet50()
    if fold_bn:
        model = fold_batchnorm(model.eval())
    return model
