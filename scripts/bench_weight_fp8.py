"""FP8-weight decode GEMM microbenchmark, memory and drift report (MI355X).

    python scripts/bench_weight_fp8.py --json out.json

Kernel time: µs per call of fp8w_decode_gemm_bf16 at M = 8 on the 8B
model's projection and FFN shapes against F.linear on bf16 weights of
the same shapes (the library GEMM, which is what serving runs without
--weight-dtype fp8_e4m3). One "step" walks enough distinct weight copies
that their total exceeds 512 MiB, so the 256 MiB Infinity Cache cannot
serve them. Each variant's step is captured into a hipGraph, as serving
runs it; a time is the median over rounds of (device-event time of a
replay) / copies, the two variants alternating within a round. Achieved
bytes/s counts the bytes the algorithm needs: N K for fp8, 2 N K for
bf16.

Memory: torch.cuda.memory_allocated() before and after
quantize_llama_weights on the 8B model (--memory).

Drift: the largest absolute logit difference and the argmax agreement
between the quantised and the bf16 model, same original seeded weights.
Random-init weights have no outlier channels, so this says nothing
about real checkpoints.
"""

import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M = 8
SHAPES = [(4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336)]
WALK_BYTES = 512 << 20
PEAK_BYTES_PER_S = 6.3e12  # achievable HBM read rate, MI355X_MICROARCH.md


def _capture(torch, fn):
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


def bench_kernel(torch, n, k, rounds, iters):
    import torch.nn.functional as F

    from client_amd.models.weight_fp8 import Fp8Linear, quantize_weight

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(n + k)
    x = torch.randn(M, k, device=dev, generator=g).to(torch.bfloat16)
    copies8 = WALK_BYTES // (n * k) + 1
    copies16 = WALK_BYTES // (2 * n * k) + 1
    w0 = torch.randn(n, k, device=dev, generator=g) * k ** -0.5
    lin0 = Fp8Linear(*quantize_weight(w0)).to(dev)
    fp8 = [lin0] + [copy.deepcopy(lin0) for _ in range(copies8 - 1)]
    w_eff = lin0.effective_weight(torch.bfloat16)
    bf16 = [w_eff] + [w_eff.clone() for _ in range(copies16 - 1)]

    def run_fp8():
        for lin in fp8:
            lin(x)

    def run_bf16():
        for w in bf16:
            F.linear(x, w)

    # outputs agree before anything is timed
    max_diff = float((lin0(x).float() - F.linear(x, w_eff).float())
                     .abs().max())
    variants = {"fp8_kernel": (_capture(torch, run_fp8), copies8, 1),
                "bf16_library": (_capture(torch, run_bf16), copies16, 2)}
    for fn, _, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (fn, copies, _) in variants.items():
            times[name].append(_time_step(torch, fn, iters) / copies)
    out = {"M": M, "N": n, "K": k, "fp8_vs_bf16_max_abs_diff": max_diff}
    for name, ts in times.items():
        _, copies, elem = variants[name]
        need = n * k * elem
        us = statistics.median(ts)
        out[name] = {
            "copies_per_step": copies,
            "us_per_call": round(us, 2),
            "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
            "needed_bytes": need,
            "achieved_TB_per_s": round(need / us / 1e6, 3),
            "share_of_6.3TBps": round(need / (us * 1e-6) / PEAK_BYTES_PER_S,
                                      3),
        }
    out["fp8_over_bf16_time"] = round(
        out["fp8_kernel"]["us_per_call"] / out["bf16_library"]["us_per_call"],
        3)
    return out


def _decode_logits(torch, model, prompt, steps):
    dev = prompt.device
    kv = model.make_kv_cache(1, dev, torch.bfloat16)
    logits = [model.forward_step(prompt, 0, kv)]
    pos = prompt.shape[1]
    for tok in steps:
        logits.append(model.forward_decode_batch(
            tok.view(1, 1), torch.tensor([pos], device=dev), kv))
        pos += 1
    return torch.stack(logits).float()


def drift(torch, cfg, prompt_len, n_steps, seed):
    from client_amd.models.llama import LlamaModel
    from client_amd.models.weight_fp8 import quantize_llama_weights

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
        a = _decode_logits(torch, model, prompt, steps)
        quantize_llama_weights(model)
        b = _decode_logits(torch, model, prompt, steps)
    return {"prompt_tokens": prompt_len, "decode_steps": n_steps,
            "max_abs_logit_diff": float((a - b).abs().max()),
            "logit_abs_max": float(a.abs().max()),
            "logit_std": float(a.std()),
            "argmax_agree": float((a.argmax(-1) == b.argmax(-1))
                                  .float().mean())}


def memory(torch):
    from client_amd.models.llama import LlamaModel, llama3_8b_config
    from client_amd.models.weight_fp8 import quantize_llama_weights

    dev = "cuda:0"
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    with torch.device(dev):
        model = LlamaModel(llama3_8b_config())
    model = model.to(torch.bfloat16).eval()
    before = torch.cuda.memory_allocated() - base
    replaced_before, replaced_after = quantize_llama_weights(model)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated() - base
    return {"allocated_before_bytes": before, "allocated_after_bytes": after,
            "block_weights_before_bytes": replaced_before,
            "block_weights_after_bytes_with_scratch": replaced_after}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-drift", action="store_true")
    ap.add_argument("--memory", action="store_true",
                    help="also build and quantise the 8B model")
    args = ap.parse_args()

    import torch

    from client_amd.models.llama import (LlamaConfig, llama3_8b_config,
                                         llama_tiny_config)

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a CPU run gives no timing")
    report = {"kernel": [], "drift": {}, "memory": None}
    with torch.inference_mode():
        for n, k in SHAPES:
            r = bench_kernel(torch, n, k, args.rounds, args.iters)
            report["kernel"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if not args.skip_drift:
        report["drift"]["llama_tiny"] = drift(
            torch, llama_tiny_config(), 40, 60, 0)
        big = llama3_8b_config()
        one = LlamaConfig(**{**big.__dict__, "n_layers": 1})
        report["drift"]["llama3_8b_one_layer"] = drift(torch, one, 256, 64, 0)
        print(json.dumps(report["drift"]), flush=True)
    if args.memory:
        report["memory"] = memory(torch)
        print(json.dumps(report["memory"]), flush=True)
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
