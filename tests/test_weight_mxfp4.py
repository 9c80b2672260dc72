"""MXFP4 weight-only linears on the CPU: quantiser, tiled layout, llama_tiny
bitwise against the same model with W_eff in plain linears, the server."""

import copy

import numpy as np
import pytest

import weight_mxfp4_refs as mr

torch = pytest.importorskip("torch")

from client_amd.models.llama import LlamaModel, llama_tiny_config  # noqa: E402
from client_amd.models.weight_mxfp4 import (  # noqa: E402
    LLAMA_BLOCK_LINEARS, Mxfp4Linear, dequantize_weight, pack,
    quantize_llama_weights, quantize_weight, split_nibbles, unpack)
from client_amd.server.__main__ import build_core, build_parser  # noqa: E402


def test_quantiser_rounding_scales_and_clamps():
    # every midpoint, the fp32 below it (negated) and above; amax goes last
    mids = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
    body = np.concatenate([mids, -np.nextafter(mids, np.float32(0)),
                           np.nextafter(mids, np.float32(8)),
                           np.zeros(11, np.float32)])
    want = [0, 2, 2, 4, 4, 6, 6] + [8, 9, 10, 11, 12, 13, 14] + [
        1, 2, 3, 4, 5, 6, 7]  # ties to the even code
    six = np.float32(6.0)
    tops = (six, -six, np.nextafter(six, np.float32(8)),
            np.nextafter(six, np.float32(0)))
    blocks = [np.ldexp(np.r_[body[:-1], t], j).astype(np.float32)
              for j in (-20, 0, 40) for t in tops]
    blocks += [np.zeros(32, np.float32),
               np.full(32, 1e-40, np.float32),                     # clamps
               np.r_[np.float32(-3e38), np.ones(31, np.float32)],  # at +-100
               np.ones(32, np.float32)]
    w = np.stack(blocks).reshape(4, -1)  # 4 rows of 4 blocks
    codes, scales = quantize_weight(torch.from_numpy(w))
    assert codes.shape == (4, 64) and scales.shape == (4, 4)
    c4 = split_nibbles(codes).numpy().reshape(-1, 32)
    # 6 2^j keeps e = j, one ulp above takes j + 1, one below keeps j
    assert list(scales.numpy().reshape(-1).astype(int) - 127) == [
        -20, -20, -19, -20, 0, 0, 1, 0, 40, 40, 41, 40, 0, -100, 100, -2]
    for b in (0, 1, 3, 4, 5, 7, 8, 9, 11):  # the blocks with e = j
        assert list(c4[b][:21]) == want, b
        assert c4[b][31] == (15 if b % 4 == 1 else 7)
    assert not c4[12].any() and not c4[13].any()
    assert c4[14][0] == 15 and (c4[15] == 6).all()  # saturated; 1 = 4 2^-2
    w32 = dequantize_weight(codes, scales, torch.float32)
    assert torch.equal(w32.to(torch.bfloat16).float(), w32)
    assert np.array_equal(w32.double().numpy(),
                          mr.w_eff(c4.reshape(4, -1), scales.numpy()))
    wb = torch.randn(5, 64)
    wb[3, 40] = float("inf")
    with pytest.raises(ValueError, match="row 3"):
        quantize_weight(wb)


@pytest.mark.parametrize("n,k", [(1, 32), (17, 96), (100, 160), (33, 256)])
def test_pack_round_trip(n, k):
    rng = np.random.default_rng(n * 1000 + k)
    codes = torch.from_numpy(rng.integers(1, 256, (n, k // 2), dtype=np.uint8))
    scales = torch.from_numpy(
        rng.integers(27, 127, (n, k // 32), dtype=np.uint8))
    pc, ps = pack(codes, scales)
    np_, kc = -(-n // 64) * 64, -(-k // 128)
    assert pc.shape == (np_ * kc * 64,) and ps.shape == (np_ * kc * 4,)
    got_c, got_s = unpack(pc, ps, n, k)
    assert torch.equal(got_c, codes) and torch.equal(got_s, scales)
    # no code is 0 and no scale 127 here: the pad is all the rest
    assert int((pc != 0).sum()) == n * k // 2
    assert int((ps != 127).sum()) == n * k // 32


def test_quantised_llama_tiny_bitwise_equal_weff_model():
    torch.manual_seed(0)
    cfg = llama_tiny_config()
    m = LlamaModel(cfg).eval()
    ref = copy.deepcopy(m)
    before, after = quantize_llama_weights(m, layer_cls=Mxfp4Linear)
    nk = 0
    for bq, br in zip(m.blocks, ref.blocks):
        for name in LLAMA_BLOCK_LINEARS:
            q, lin = getattr(bq, name), getattr(br, name)
            assert isinstance(q, Mxfp4Linear)
            lin.weight.data = q.effective_weight(torch.float32)
            nk += lin.weight.numel()
    assert (before, after) == (4 * nk, nk // 2 + nk // 32)
    b = 3
    with torch.inference_mode():
        toks = torch.randint(0, cfg.vocab_size, (b, 8))
        args = (toks, torch.zeros(b, dtype=torch.int64),
                torch.tensor([8, 5, 7]), torch.tensor([7, 4, 6]))
        kvs = [mod.make_kv_cache(b, "cpu", torch.float32) for mod in (m, ref)]
        assert torch.equal(m.forward_prefill_chunk(*args, kvs[0], 16),
                           ref.forward_prefill_chunk(*args, kvs[1], 16))
        pos = torch.tensor([8, 5, 7])
        for _ in range(3):
            tokens = torch.randint(0, cfg.vocab_size, (b, 1))
            assert torch.equal(m.forward_decode_batch(tokens, pos, kvs[0]),
                               ref.forward_decode_batch(tokens, pos, kvs[1]))
            pos = pos + 1
    ids = torch.randint(0, cfg.vocab_size, (2, 6))
    assert ([t.tolist() for t in m.generate(ids, 5)]
            == [t.tolist() for t in ref.generate(ids, 5)])


def test_server_flag_and_model_config():
    parser = build_parser()
    args = parser.parse_args(["--weight-dtype", "mxfp4"])
    with pytest.raises(SystemExit):
        parser.parse_args(["--weight-dtype", "int4"])
    cores = [build_core(["llama_tiny"], device="cpu", dtype="fp32", **kw)
             for kw in ({}, {"weight_dtype": "bf16"},
                        {"weight_dtype": args.weight_dtype})]
    try:
        plain, default, model = (c.models["llama_tiny"] for c in cores)
        assert "parameters" not in plain.config()
        assert default.config() == plain.config()
        assert model.config() == dict(plain.config(), parameters={
            "weight_dtype": {"string_value": "mxfp4"}})
        assert all(isinstance(getattr(blk, name), Mxfp4Linear)
                   for blk in model.module.blocks
                   for name in LLAMA_BLOCK_LINEARS)
    finally:
        for c in cores:
            sched = c.models["llama_tiny"]._scheduler
            if sched is not None:
                sched.shutdown()
