"""The wide fp8-weight GEMM's plumbing, without a GPU: ``fused_gemm`` from
the quantise helpers, and --fp8-weight-gemm down to the model config."""

import copy

import pytest
import torch

from client_amd.models.llama import LlamaModel, llama_tiny_config
from client_amd.models.weight_fp8 import (LLAMA_BLOCK_LINEARS,
                                          quantize_llama_weights)
from client_amd.models.weight_mxfp4 import quantize_llama_weights_as
from client_amd.server.__main__ import build_core, build_parser

FP8 = "fp8_e4m3"


def test_quantize_sets_fused_gemm_on_every_layer():
    base = LlamaModel(llama_tiny_config()).eval()
    off, on, on_as = (copy.deepcopy(base) for _ in range(3))
    quantize_llama_weights(off)
    quantize_llama_weights(on, fused_gemm=True)
    quantize_llama_weights_as(on_as, FP8, fused_gemm=True)
    for model, want in ((off, False), (on, True), (on_as, True)):
        assert all(getattr(b, n).fused_gemm is want
                   for b in model.blocks for n in LLAMA_BLOCK_LINEARS)
    with pytest.raises(ValueError, match=FP8):
        quantize_llama_weights_as(base, "mxfp4", fused_gemm=True)


def test_server_flag_and_model_config():
    parser = build_parser()
    assert parser.parse_args([]).fp8_weight_gemm is False
    args = parser.parse_args(["--weight-dtype", FP8, "--fp8-weight-gemm"])
    cores = [build_core(["llama_tiny"], device="cpu", dtype="fp32", **kw)
             for kw in ({}, dict(weight_dtype=FP8),
                        dict(weight_dtype=args.weight_dtype,
                             fp8_weight_gemm=args.fp8_weight_gemm))]
    try:
        plain, fp8, wide = (c.models["llama_tiny"] for c in cores)
        assert "parameters" not in plain.config()
        assert fp8.config()["parameters"] == {
            "weight_dtype": {"string_value": FP8}}
        cfg = wide.config()
        assert cfg.pop("parameters") == {
            "weight_dtype": {"string_value": FP8},
            "fp8_weight_gemm": {"string_value": "true"}}
        assert cfg == plain.config()
        assert wide.module.blocks[-1].w2.fused_gemm is True
        assert fp8.module.blocks[-1].w2.fused_gemm is False
    finally:
        for c in cores:
            c.models["llama_tiny"]._scheduler.shutdown()


@pytest.mark.parametrize("weight_dtype", [None, "bf16", "mxfp4"])
def test_flag_needs_fp8_weights(weight_dtype):
    with pytest.raises(SystemExit, match=FP8):
        build_core(["llama_tiny"], device="cpu", dtype="fp32",
                   weight_dtype=weight_dtype, fp8_weight_gemm=True)
