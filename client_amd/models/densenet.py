"""DenseNet-121 (from scratch on torch.nn).

BASELINE.md config 3 names densenet_onnx (the canonical Triton qa
model) for the 8-replica concurrency sweep; this is the same
architecture served natively (random-init, synthetic inputs).

Two forms. The default is the textbook module: seven launches per dense
layer (BN, ReLU, 1x1 conv, BN, ReLU, 3x3 conv, cat). `fuse_dense_layers`
(densenet121(fused=True), the server's --densenet-fused) puts every dense
block on one buffer and every layer on the two kernels of
client_amd/ops/csrc/dense_layer.hip, and folds the stem's BN into its
conv (FusedStem; one launch of client_amd/ops/csrc/stem_conv.hip with
CLIENT_AMD_STEM_CONV=1, the server's --fused-stem).
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .resnet import (_is_stem_pool, pack_conv1x1_weight, pack_conv3x3_weight,
                     pack_stem_weight, stem_switch)


class DenseLayer(nn.Module):
    def __init__(self, in_ch, growth, bn_size=4):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(in_ch)
        self.conv1 = nn.Conv2d(in_ch, bn_size * growth, 1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.conv2 = nn.Conv2d(bn_size * growth, growth, 3, padding=1,
                               bias=False)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.conv1(self.relu(self.norm1(x)))
        out = self.conv2(self.relu(self.norm2(out)))
        return torch.cat([x, out], 1)


class Transition(nn.Module):
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.norm = nn.BatchNorm2d(in_ch)
        self.conv = nn.Conv2d(in_ch, out_ch, 1, bias=False)
        self.pool = nn.AvgPool2d(2, stride=2)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.pool(self.conv(self.relu(self.norm(x))))


class DenseNet121(nn.Module):
    def __init__(self, growth=32, blocks=(6, 12, 24, 16), num_classes=1000):
        super().__init__()
        ch = 64
        self.stem = nn.Sequential(
            nn.Conv2d(3, ch, 7, stride=2, padding=3, bias=False),
            nn.BatchNorm2d(ch), nn.ReLU(inplace=True),
            nn.MaxPool2d(3, stride=2, padding=1),
        )
        layers = []
        for i, n in enumerate(blocks):
            for _ in range(n):
                layers.append(DenseLayer(ch, growth))
                ch += growth
            if i != len(blocks) - 1:
                layers.append(Transition(ch, ch // 2))
                ch //= 2
        self.features = nn.Sequential(*layers)
        self.norm = nn.BatchNorm2d(ch)
        self.classifier = nn.Linear(ch, num_classes)

    def forward(self, x):
        x = self.features(self.stem(x))
        x = torch.relu(self.norm(x))
        x = torch.nn.functional.adaptive_avg_pool2d(x, 1).flatten(1)
        return self.classifier(x)


def _bn_affine(bn):
    """Eval-mode BatchNorm as y = x*scale + shift, in the BN's dtype."""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias.detach() - bn.running_mean * scale


def _fused_switch():
    return os.environ.get("CLIENT_AMD_DENSENET_FUSED", "1") != "0"


class _FoldedParams:
    """The folded tensors of a fused block, cached per (device, dtype,
    form): form "kernel" is what the HIP kernels read (fp32 scale, shift
    and bias, bf16 weights packed for the MFMA A operand), form "torch"
    the same algebra's operands for torch ops in the input's dtype.

    The masters are computed once at conversion, in the model's dtype at
    that time, and are deliberately not module buffers: a later
    `.to(torch.bfloat16)` of the model would round scale, shift and bias
    to bf16, and the folded weights a second time."""

    def __init__(self, masters):
        self.masters = masters  # list of tuples of tensors
        self._cache = {}

    def get(self, device, dtype, form, build):
        key = (str(device), dtype, form)
        if key not in self._cache:
            self._cache[key] = [build(*m) for m in self.masters]
        return self._cache[key]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class FusedDenseBlock(nn.Module):
    """A run of DenseLayers on one block buffer, two HIP kernels a layer.

    forward allocates one [N, C_end, H, W] tensor, copies the input into
    its channel prefix, and per layer l runs
      dense_conv1x1_bf16      norm1+ReLU prologue, conv1, norm2 folded into
                              weights and bias, ReLU: reads the prefix
                              [0, C_l) in place (image stride C_end*H*W)
      dense_conv3x3_k32_bf16  conv2, its 32 channels stored at
                              [C_l, C_l + 32) of the buffer
    so nothing is concatenated. On the CPU, for a dtype other than bf16,
    with CLIENT_AMD_DENSENET_FUSED=0 or for a shape the kernels refuse
    the same folded algebra runs as torch ops on the same buffer."""

    def __init__(self, layers):
        super().__init__()
        first = layers[0]
        self.c0 = first.conv1.in_channels
        self.mid = first.conv1.out_channels
        self.growth = first.conv2.out_channels
        self.n_layers = len(layers)
        self.c_end = self.c0 + self.growth * self.n_layers
        masters = []
        for layer in layers:
            s1, h1 = _bn_affine(layer.norm1)
            s2, h2 = _bn_affine(layer.norm2)
            w1 = layer.conv1.weight.detach() * s2.view(-1, 1, 1, 1)
            masters.append((s1, h1, w1, h2, layer.conv2.weight.detach()))
        self.folded = _FoldedParams(masters)
        self._supported = {}
        self.calls = 0  # kernel launches (tests assert they really ran)

    def _use_kernels(self, x):
        if not (x.is_cuda and x.dtype == torch.bfloat16 and _fused_switch()
                and self.growth == 32):
            return False
        key = tuple(x.shape)
        if key not in self._supported:
            from ..ops import hip_runtime as hr

            n, _, h, w = x.shape
            xs = self.c_end * h * w
            self._supported[key] = all(
                hr.dense_conv1x1_supported(n, c, self.mid, h, w, xs)
                and hr.dense_conv3x3_k32_supported(n, self.mid, h, w, c, xs)
                for c in range(self.c0, self.c_end, 32))
        return self._supported[key]

    def forward(self, x):
        n, c0, h, w = x.shape
        assert c0 == self.c0, (c0, self.c0)
        buf = torch.empty((n, self.c_end, h, w), device=x.device,
                          dtype=x.dtype)
        buf[:, :c0].copy_(x)
        if self._use_kernels(x):
            from ..ops import hip_runtime as hr

            def build(s1, h1, w1, b1, w2):
                dev = x.device
                return (s1.float().to(dev), h1.float().to(dev),
                        pack_conv1x1_weight(
                            w1.float().to(dev).to(torch.bfloat16)),
                        b1.float().to(dev),
                        pack_conv3x3_weight(
                            w2.to(dev).to(torch.bfloat16)))

            params = self.folded.get(x.device, x.dtype, "kernel", build)
            xs = self.c_end * h * w
            mid = torch.empty((n, self.mid, h, w), device=x.device,
                              dtype=x.dtype)
            for i, (s1, h1, w1, b1, w2) in enumerate(params):
                c = c0 + 32 * i
                hr.dense_conv1x1_bf16(
                    buf.data_ptr(), xs, s1.data_ptr(), h1.data_ptr(),
                    w1.data_ptr(), b1.data_ptr(), mid.data_ptr(), n, c,
                    self.mid, h, w, True, _stream())
                hr.dense_conv3x3_k32_bf16(
                    mid.data_ptr(), w2.data_ptr(), buf.data_ptr(), n,
                    self.mid, h, w, c, xs, _stream())
            self.calls += 2 * len(params)
            return buf

        def build(*tensors):
            return tuple(t.to(x.device, x.dtype) for t in tensors)

        params = self.folded.get(x.device, x.dtype, "torch", build)
        for i, (s1, h1, w1, b1, w2) in enumerate(params):
            c = c0 + self.growth * i
            a = torch.relu(buf[:, :c] * s1.view(1, -1, 1, 1)
                           + h1.view(1, -1, 1, 1))
            y = torch.relu(F.conv2d(a, w1) + b1.view(1, -1, 1, 1))
            buf[:, c:c + self.growth] = F.conv2d(y, w2, padding=1)
        return buf


class FusedTransition(nn.Module):
    """Transition with norm+ReLU as the prologue of the 1x1 conv kernel
    (no bias, no ReLU after it), then the module's average pool. The
    fallback conditions are FusedDenseBlock's."""

    def __init__(self, transition):
        super().__init__()
        scale, shift = _bn_affine(transition.norm)
        self.folded = _FoldedParams(
            [(scale, shift, transition.conv.weight.detach())])
        self.pool = transition.pool
        self.calls = 0

    def forward(self, x):
        n, c, h, w = x.shape
        k = self.folded.masters[0][2].shape[0]
        use = (x.is_cuda and x.dtype == torch.bfloat16 and _fused_switch()
               and x.is_contiguous())
        if use:
            from ..ops import hip_runtime as hr

            use = hr.dense_conv1x1_supported(n, c, k, h, w, c * h * w)
        if use:
            def build(s, sh, wt):
                dev = x.device
                return (s.float().to(dev), sh.float().to(dev),
                        pack_conv1x1_weight(wt.to(dev).to(torch.bfloat16)))

            (s, sh, wp), = self.folded.get(x.device, x.dtype, "kernel",
                                           build)
            out = torch.empty((n, k, h, w), device=x.device, dtype=x.dtype)
            hr.dense_conv1x1_bf16(
                x.data_ptr(), c * h * w, s.data_ptr(), sh.data_ptr(),
                wp.data_ptr(), 0, out.data_ptr(), n, c, k, h, w, False,
                _stream())
            self.calls += 1
            return self.pool(out)

        def build(*tensors):
            return tuple(t.to(x.device, x.dtype) for t in tensors)

        (s, sh, wt), = self.folded.get(x.device, x.dtype, "torch", build)
        a = torch.relu(x * s.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        return self.pool(F.conv2d(a, wt))


class FusedStem(nn.Module):
    """The stem (7x7 stride-2 conv, BN, ReLU, 3x3 stride-2 max-pool) with
    the BN folded into the conv: weight * scale per output channel, the
    shift as a bias. With CLIENT_AMD_STEM_CONV=1, on a HIP device, for
    contiguous bf16 input of a shape the kernel accepts it is one launch
    of stem_conv7x7_pool_bf16 (client_amd/ops/csrc/stem_conv.hip);
    otherwise the same folded algebra runs as torch ops."""

    def __init__(self, conv, bn):
        super().__init__()
        scale, shift = _bn_affine(bn)
        self.folded = _FoldedParams(
            [(conv.weight.detach() * scale.view(-1, 1, 1, 1), shift)])
        self.calls = 0  # kernel launches (tests assert it really ran)
        self.enabled = None  # None: CLIENT_AMD_STEM_CONV decides

    def forward(self, x):
        use = (stem_switch(self.enabled) and x.is_cuda
               and x.dtype == torch.bfloat16
               and x.dim() == 4 and x.shape[1] == 3 and x.is_contiguous())
        if use:
            from ..ops import hip_runtime as hr

            n, _, h, w = x.shape
            use = hr.stem_conv7x7_pool_supported(n, h, w)
        if use:
            def build(wt, b):
                dev = x.device
                return (pack_stem_weight(wt.to(dev).to(torch.bfloat16)),
                        b.float().to(dev))

            (wp, b), = self.folded.get(x.device, x.dtype, "kernel", build)
            oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            out = torch.empty((n, 64, (oh - 1) // 2 + 1, (ow - 1) // 2 + 1),
                              device=x.device, dtype=x.dtype)
            hr.stem_conv7x7_pool_bf16(x.data_ptr(), wp.data_ptr(),
                                      b.data_ptr(), out.data_ptr(), n, h, w,
                                      _stream())
            self.calls += 1
            return out

        def build(*tensors):
            return tuple(t.to(x.device, x.dtype) for t in tensors)

        (wt, b), = self.folded.get(x.device, x.dtype, "torch", build)
        y = F.conv2d(x, wt, stride=2, padding=3) + b.view(1, -1, 1, 1)
        return F.max_pool2d(y.relu_(), 3, 2, 1)


def _is_textbook_stem(stem):
    if not (isinstance(stem, nn.Sequential) and len(stem) == 4):
        return False
    conv, bn, relu, pool = stem
    return (isinstance(conv, nn.Conv2d) and conv.bias is None
            and tuple(conv.weight.shape) == (64, 3, 7, 7)
            and conv.stride == (2, 2) and conv.padding == (3, 3)
            and isinstance(bn, nn.BatchNorm2d)
            and isinstance(relu, nn.ReLU) and _is_stem_pool(pool))


def fuse_dense_layers(model):
    """Rewrite `model.features` (eval mode) so that each run of
    DenseLayers is one FusedDenseBlock and each Transition a
    FusedTransition, and `model.stem` as a FusedStem; sets
    `model.fused_dense_layers`, and `model.fused_stem` when
    CLIENT_AMD_STEM_CONV=1 now. Convert before moving the model to its
    serving dtype: the BN statistics are folded in the dtype the model
    has now."""
    model.eval()
    if _is_textbook_stem(getattr(model, "stem", None)):
        model.stem = FusedStem(model.stem[0], model.stem[1])
        if stem_switch():
            model.fused_stem = True
    out, run = [], []
    for m in model.features:
        if isinstance(m, DenseLayer):
            run.append(m)
            continue
        if run:
            out.append(FusedDenseBlock(run))
            run = []
        out.append(FusedTransition(m) if isinstance(m, Transition) else m)
    if run:
        out.append(FusedDenseBlock(run))
    model.features = nn.Sequential(*out)
    model.fused_dense_layers = True
    return model


def densenet121(fused=False):
    """fused=True: the dense layers and transitions on the HIP kernels
    of client_amd/ops/csrc/dense_layer.hip (fuse_dense_layers)."""
    model = DenseNet121()
    return fuse_dense_layers(model) if fused else model
