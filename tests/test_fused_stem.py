"""CPU tests of the fused ResNet stem module (bias + ReLU + 3x3/s2/p1
max-pool): its torch fallback and the fold_batchnorm wiring."""

import pytest


@pytest.mark.parametrize("shape", [(2, 8, 9, 11), (1, 3, 2, 2),
                                   (1, 64, 32, 32)])
def test_stem_fallback_equals_unfused_fp32_sequence(shape):
    import torch
    import torch.nn.functional as F

    from client_amd.models.resnet import BiasReluMaxPool

    torch.manual_seed(0)
    x = torch.randn(shape)
    bias = torch.randn(shape[1])
    mod = BiasReluMaxPool(bias)
    ref = F.max_pool2d(F.relu(x + bias.view(1, -1, 1, 1)), 3, 2, 1)
    out = mod(x.clone())
    assert out.dtype == torch.float32
    assert torch.equal(out, ref)


def test_stem_wiring_and_forward_matches_plain_fold():
    import copy

    import torch
    import torch.nn as nn

    from client_amd.models.resnet import (
        BiasAct,
        BiasReluMaxPool,
        ResNet50,
        fold_batchnorm,
    )

    torch.manual_seed(4)
    m = ResNet50().eval()
    m.bn1.running_mean.uniform_(-0.5, 0.5)
    m.bn1.running_var.uniform_(0.5, 2.0)
    m.bn1.bias.data.uniform_(-0.3, 0.3)
    fused = fold_batchnorm(copy.deepcopy(m), fuse_eltwise=True)
    assert isinstance(fused.bn1, BiasReluMaxPool)
    assert isinstance(fused.relu, nn.Identity)
    assert isinstance(fused.maxpool, nn.Identity)
    assert fused.conv1.bias is None

    def stem(model, x):
        return model.maxpool(model.relu(model.bn1(model.conv1(x))))

    x = torch.randn(2, 3, 33, 47)
    with torch.inference_mode():
        plain = fold_batchnorm(copy.deepcopy(m), fuse_eltwise=False)
        a, b = stem(plain, x), stem(fused, x)
    assert a.shape == b.shape
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)

    # a pool the kernel does not implement keeps its own module
    other = copy.deepcopy(m)
    other.maxpool = nn.MaxPool2d(2, stride=2)
    other = fold_batchnorm(other, fuse_eltwise=True)
    assert isinstance(other.bn1, BiasAct)
    assert isinstance(other.maxpool, nn.MaxPool2d)
