"""Decode-attention microbenchmark and fp8-cache drift report (MI355X).

    python scripts/bench_decode_attention.py --json out.json

Kernel time: µs per call of the fused gqa_decode_attention over a bf16
and an e4m3 cache against the torch 4-kernel path
(_gqa_decode_attention: matmul + add + softmax + matmul), at the 8B
decode shape b=8, hq=32, hk=8, d=128. One "step" walks 32 distinct
caches, as the 32 layers of a decode step do, so the K/V are not served
from the last call's cache lines. Each variant's step is captured into
a hipGraph, as serving runs it (eager launches of kernels this small
time the host); a time is the median over rounds of (device-event time
of a replay) / 32, the three variants alternating within a round.
Achieved bytes/s counts the bytes the algorithm needs: K and V of every
row's own keys.

Drift: the largest absolute logit difference between an fp8-cache and a
bf16-cache decode of llama_tiny and of one 8B-shaped layer with seeded
weights.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HQ, HK, D = 8, 32, 8, 128
LAYERS = 32
PEAK_BYTES_PER_S = 6.3e12  # achievable HBM read rate, MI355X_MICROARCH.md


def _capture(torch, fn):
    """fn as a replayable hipGraph, as the serving path runs it: eager
    launches of these small kernels time the host, not the GPU."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    return graph.replay


def _time_step(torch, fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # µs per step


def bench_kernel(torch, max_len, mixed, rounds, iters):
    from client_amd.models import llama
    from client_amd.models.kv_cache import kv_encode_fp8

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(max_len + int(mixed))
    cache_len = max_len + 1
    if mixed:
        lens = [max(1, max_len * (i + 1) // B) for i in range(B)]
    else:
        lens = [max_len] * B
    pos = torch.tensor([n - 1 for n in lens], device=dev, dtype=torch.int64)
    q = (torch.randn(B, HQ, 1, D, device=dev, generator=g) * D ** -0.75
         ).to(torch.bfloat16)
    caches16, caches8 = [], []
    for _ in range(LAYERS):
        k = torch.randn(B, HK, cache_len, D, device=dev, generator=g)
        v = torch.randn(B, HK, cache_len, D, device=dev, generator=g)
        caches16.append((k.to(torch.bfloat16), v.to(torch.bfloat16)))
        caches8.append((kv_encode_fp8(k), kv_encode_fp8(v)))
    key_idx = torch.arange(max_len, device=dev)[None]
    mask = torch.where(key_idx <= pos[:, None], 0.0, float("-inf"))[
        :, None, None, :].to(torch.bfloat16)
    rep = HQ // HK

    def run_torch():
        for ck, cv in caches16:
            llama._gqa_decode_attention(q, ck[:, :, :max_len],
                                        cv[:, :, :max_len], mask, rep,
                                        scaled=True)

    def run_fused(caches):
        def run():
            for ck, cv in caches:
                llama._fused_decode_attention(q, ck, cv, pos, max_len)
        return run

    variants = {"torch_bf16": run_torch,
                "fused_bf16": run_fused(caches16),
                "fused_fp8": run_fused(caches8)}
    # outputs agree before anything is timed
    ref = llama._gqa_decode_attention(
        q, caches16[0][0][:, :, :max_len], caches16[0][1][:, :, :max_len],
        mask, rep, scaled=True).float()
    got = llama._fused_decode_attention(q, *caches16[0], pos,
                                        max_len).float()
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
    keys = sum(lens)
    out = {"max_len": max_len, "rows": "mixed" if mixed else "full",
           "row_lengths": lens, "fused_vs_torch_max_abs_diff": max_diff}
    for name, ts in times.items():
        elem = 1 if name.endswith("fp8") else 2
        need = 2 * keys * HK * D * elem
        us = statistics.median(ts)
        out[name] = {
            "us_per_call": round(us, 2),
            "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
            "needed_bytes": need,
            "achieved_TB_per_s": round(need / us / 1e6, 3),
            "share_of_6.3TBps": round(need / (us * 1e-6) / PEAK_BYTES_PER_S,
                                      3),
        }
    return out


def _decode_logits(torch, model, kv_dtype, prompt, steps):
    """Greedy tokens come from the bf16-cache run so both caches see the
    same inputs; returns the logits of every decode step."""
    dev = prompt.device
    kv = model.make_kv_cache(1, dev, torch.bfloat16, kv_dtype)
    logits = [model.forward_step(prompt, 0, kv)]
    pos = prompt.shape[1]
    for tok in steps:
        logits.append(model.forward_decode_batch(
            tok.view(1, 1), torch.tensor([pos], device=dev), kv))
        pos += 1
    return torch.stack(logits).float()


def drift(torch, cfg, prompt_len, n_steps, seed):
    from client_amd.models.llama import LlamaModel

    dev = "cuda:0"
    torch.manual_seed(seed)
    with torch.device(dev):
        model = LlamaModel(cfg)
    model = model.to(torch.bfloat16).eval()
    g = torch.Generator(device=dev).manual_seed(seed)
    prompt = torch.randint(0, cfg.vocab_size, (1, prompt_len), device=dev,
                           generator=g)
    steps = torch.randint(0, cfg.vocab_size, (n_steps,), device=dev,
                          generator=g)
    with torch.inference_mode():
        a = _decode_logits(torch, model, None, prompt, steps)
        b = _decode_logits(torch, model, "fp8_e4m3", prompt, steps)
    return {"prompt_tokens": prompt_len, "decode_steps": n_steps,
            "max_abs_logit_diff": float((a - b).abs().max()),
            "logit_abs_max": float(a.abs().max()),
            "logit_std": float(a.std()),
            "argmax_agree": float((a.argmax(-1) == b.argmax(-1))
                                  .float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    ap.add_argument("--max-lens", type=int, nargs="+",
                    default=[256, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-drift", action="store_true")
    args = ap.parse_args()

    import torch

    from client_amd.models.llama import (LlamaConfig, llama3_8b_config,
                                         llama_tiny_config)

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a CPU run gives no timing")
    report = {"shape": {"b": B, "hq": HQ, "hk": HK, "d": D},
              "layers_per_step": LAYERS, "kernel": [], "drift": {}}
    for max_len in args.max_lens:
        for mixed in (False, True):
            r = bench_kernel(torch, max_len, mixed, args.rounds, args.iters)
            report["kernel"].append(r)
            print(json.dumps(r), flush=True)
    if not args.skip_drift:
        report["drift"]["llama_tiny"] = drift(
            torch, llama_tiny_config(), 40, 60, 0)
        big = llama3_8b_config()
        one = LlamaConfig(**{**big.__dict__, "n_layers": 1})
        report["drift"]["llama3_8b_one_layer"] = drift(torch, one, 256, 64, 0)
        print(json.dumps(report["drift"]), flush=True)
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
