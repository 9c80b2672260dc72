"""Prefill-chunk attention microbenchmark (MI355X).

    python scripts/bench_prefill_attention.py --json out.json

µs per call of the fused gqa_prefill_attention over a bf16 and an e4m3
cache against the torch prefill attention block of
LlamaModel.forward_prefill_chunk as it stands (index_select of the
mapped cache rows and the bucket slice -> kv_load -> repeat_interleave
-> scaled_dot_product_attention with the materialised mask), at the 8B
shape hq=32, hk=8, d=128 with a chunk of C=128 tokens that ends at the
bucket's last position (the most keys a chunk of that bucket sees).
One "step" walks 32 distinct caches of 8 rows, as the 32 layers of a
prefill step do, so K/V are not served from the last call's cache lines.
Each variant's step is captured into a hipGraph, as serving runs it; a
time is the median over rounds of (device-event time of a replay) / 32,
the three variants alternating within a round. TF/s counts the useful
(causal) multiply-adds of both contractions, TB/s the K and V bytes of
the keys the chunk may see, read once.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_decode_attention import _capture, _time_step  # noqa: E402

HQ, HK, D, C = 32, 8, 128, 128
LAYERS = 32
CACHE_ROWS = 8
PEAK_BF16_FLOPS = 2.5e15  # dense bf16 MFMA roof, MI355X_MICROARCH.md
PEAK_BYTES_PER_S = 6.3e12  # achievable HBM read rate


def bench(torch, b, bucket, rounds, iters):
    import torch.nn.functional as F

    from client_amd.models import llama
    from client_amd.models.kv_cache import kv_encode_fp8, kv_load

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(bucket + b)
    cache_len = bucket + 1
    rep = HQ // HK
    pos = torch.full((b,), bucket - C, device=dev, dtype=torch.int64)
    lens = torch.full((b,), C, device=dev, dtype=torch.int64)
    row_map = torch.tensor([3, 5][:b], device=dev, dtype=torch.int64)
    # q as the fused path holds it ([B, C, H, d], 1/sqrt(d) folded in) and
    # as the torch path holds it ([B, H, C, d] view, unscaled)
    q_raw = (torch.randn(b, C, HQ, D, device=dev, generator=g) * D ** -0.25
             ).to(torch.bfloat16)
    q_fused = (q_raw.float() * D ** -0.5).to(torch.bfloat16)
    q_torch = q_raw.transpose(1, 2)
    caches16, caches8 = [], []
    for _ in range(LAYERS):
        k = torch.randn(CACHE_ROWS, HK, cache_len, D, device=dev,
                        generator=g) * D ** -0.25
        v = torch.randn(CACHE_ROWS, HK, cache_len, D, device=dev, generator=g)
        caches16.append((k.to(torch.bfloat16), v.to(torch.bfloat16)))
        caches8.append((kv_encode_fp8(k), kv_encode_fp8(v)))
        del k, v
    abs_pos = pos[:, None] + torch.arange(C, device=dev)[None, :]
    key_idx = torch.arange(bucket, device=dev)
    mask = torch.where(key_idx[None, None, :] <= abs_pos[:, :, None],
                       0.0, float("-inf"))[:, None]     # [B,1,C,bucket] fp32

    def torch_block(ck, cv):
        k_all = ck.index_select(0, row_map)[:, :, :bucket]
        v_all = cv.index_select(0, row_map)[:, :, :bucket]
        k_all = kv_load(k_all, q_torch.dtype).repeat_interleave(rep, dim=1)
        v_all = kv_load(v_all, q_torch.dtype).repeat_interleave(rep, dim=1)
        return F.scaled_dot_product_attention(
            q_torch, k_all, v_all, attn_mask=mask.to(q_torch.dtype))

    def fused_block(ck, cv):
        return llama._fused_prefill_attention(q_fused, ck, cv, pos, lens,
                                              row_map, bucket)

    def loop(block, caches):
        def run():
            for ck, cv in caches:
                block(ck, cv)
        return run

    variants = {"torch_bf16": loop(torch_block, caches16),
                "fused_bf16": loop(fused_block, caches16),
                "fused_fp8": loop(fused_block, caches8)}
    # outputs agree before anything is timed
    ref = torch_block(*caches16[0]).transpose(1, 2).float()
    got = fused_block(*caches16[0]).float()
    max_diff = float((ref - got).abs().max())
    variants = {name: _capture(torch, fn) for name, fn in variants.items()}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time_step(torch, fn, iters) / LAYERS)
    visible = int((abs_pos + 1).sum())        # (query, key) pairs computed
    flops = 4 * D * HQ * visible              # QK^T and PV, 2 flops per MAC
    out = {"b": b, "bucket": bucket, "chunk": C,
           "fused_vs_torch_max_abs_diff": max_diff, "useful_flops": flops}
    for name, ts in times.items():
        elem = 1 if name.endswith("fp8") else 2
        need = 2 * b * bucket * HK * D * elem
        us = statistics.median(ts)
        out[name] = {
            "us_per_call": round(us, 2),
            "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
            "TF_per_s": round(flops / us / 1e6, 2),
            "share_of_mfma_roof": round(flops / (us * 1e-6)
                                        / PEAK_BF16_FLOPS, 4),
            "kv_bytes": need,
            "kv_TB_per_s": round(need / us / 1e6, 3),
            "share_of_6.3TBps": round(need / (us * 1e-6) / PEAK_BYTES_PER_S,
                                      4),
        }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    ap.add_argument("--buckets", type=int, nargs="+",
                    default=[256, 1024, 4096])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a CPU run gives no timing")
    report = {"shape": {"hq": HQ, "hk": HK, "d": D, "chunk": C,
                        "cache_rows": CACHE_ROWS},
              "layers_per_step": LAYERS, "kernel": []}
    with torch.inference_mode():
        for bucket in args.buckets:
            for b in args.batches:
                r = bench(torch, b, bucket, args.rounds, args.iters)
                report["kernel"].append(r)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
