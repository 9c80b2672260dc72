"""The wide MXFP4-weight GEMM's plumbing, without a GPU: ``wide_gemm`` from
the quantise helper, and --mxfp4-weight-gemm down to the model config."""

import copy

import pytest
import torch

from client_amd.models.llama import LlamaModel, llama_tiny_config
from client_amd.models.weight_fp8 import LLAMA_BLOCK_LINEARS
from client_amd.models.weight_mxfp4 import (Mxfp4Linear,
                                            quantize_llama_weights_as)
from client_amd.server.__main__ import build_core, build_parser

MXFP4 = "mxfp4"


def test_quantize_sets_wide_gemm_on_every_layer():
    base = LlamaModel(llama_tiny_config()).eval()
    off, on = copy.deepcopy(base), copy.deepcopy(base)
    quantize_llama_weights_as(off, MXFP4)
    quantize_llama_weights_as(on, MXFP4, wide_gemm=True)
    for model, want in ((off, False), (on, True)):
        layers = [getattr(b, n) for b in model.blocks
                  for n in LLAMA_BLOCK_LINEARS]
        assert all(isinstance(q, Mxfp4Linear) and q.wide_gemm is want
                   for q in layers)
    x = torch.randn(24, base.blocks[0].wq.in_features)
    assert torch.equal(on.blocks[0].wq(x), off.blocks[0].wq(x))  # CPU route
    with pytest.raises(ValueError, match=MXFP4):
        quantize_llama_weights_as(base, "fp8_e4m3", wide_gemm=True)


def test_server_flag_and_model_config():
    parser = build_parser()
    assert parser.parse_args([]).mxfp4_weight_gemm is False
    args = parser.parse_args(["--weight-dtype", MXFP4, "--mxfp4-weight-gemm"])
    cores = [build_core(["llama_tiny"], device="cpu", dtype="fp32", **kw)
             for kw in ({}, dict(weight_dtype=MXFP4),
                        dict(weight_dtype=args.weight_dtype,
                             mxfp4_weight_gemm=args.mxfp4_weight_gemm))]
    try:
        plain, mx, wide = (c.models["llama_tiny"] for c in cores)
        assert "parameters" not in plain.config()
        assert mx.config()["parameters"] == {
            "weight_dtype": {"string_value": MXFP4}}
        cfg = wide.config()
        assert cfg.pop("parameters") == {
            "weight_dtype": {"string_value": MXFP4},
            "mxfp4_weight_gemm": {"string_value": "true"}}
        assert cfg == plain.config()
        assert wide.module.blocks[-1].w2.wide_gemm is True
        assert mx.module.blocks[-1].w2.wide_gemm is False
    finally:
        for c in cores:
            c.models["llama_tiny"]._scheduler.shutdown()


@pytest.mark.parametrize("weight_dtype", [None, "bf16", "fp8_e4m3"])
def test_flag_needs_mxfp4_weights(weight_dtype):
    with pytest.raises(SystemExit, match=MXFP4):
        build_core(["llama_tiny"], device="cpu", dtype="fp32",
                   weight_dtype=weight_dtype, mxfp4_weight_gemm=True)
