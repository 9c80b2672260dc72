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

Wide GEMM (--wide, nothing else then runs): the same method at M = 24 to
1024 for fp8w_gemm_bf16, the dequant route (fp8w_dequant_bf16 into the
shared scratch + F.linear) and F.linear on bf16 weights.

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
WIDE_M = (24, 64, 128, 512, 1024)
PEAK_BF16_FLOPS = 2.5e15  # dense bf16 MFMA roof, MI355X_MICROARCH.md


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


def bench_wide(torch, n, k, rounds, iters):
    """--wide: M > 16 on fp8w_gemm_bf16, on the dequant route (what
    Fp8Linear runs without fused_gemm) and on F.linear with bf16 weights
    of the same values; the method of bench_kernel. The bound of a call
    is the larger of 2 M N K FLOPs at the bf16 MFMA roof and the bytes
    the algorithm needs (codes or bf16 weights once, x once, y once) at
    the HBM read rate."""
    import torch.nn.functional as F

    from client_amd.models.weight_fp8 import Fp8Linear, quantize_weight
    from client_amd.ops import hip_runtime as hr

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(n + k)
    copies8 = WALK_BYTES // (n * k) + 1
    copies16 = WALK_BYTES // (2 * n * k) + 1
    w0 = torch.randn(n, k, device=dev, generator=g) * k ** -0.5
    lin0 = Fp8Linear(*quantize_weight(w0)).to(dev)
    fp8 = [lin0] + [copy.deepcopy(lin0) for _ in range(copies8 - 1)]
    for lin in fp8:  # one dequant scratch for all, as in a model
        lin._scratch = lin0._scratch
    w_eff = lin0.effective_weight(torch.bfloat16)
    bf16 = [w_eff] + [w_eff.clone() for _ in range(copies16 - 1)]
    rows = []
    for m in WIDE_M:
        x = torch.randn(m, k, device=dev, generator=g).to(torch.bfloat16)

        def run_fp8(fused):
            for lin in fp8:
                lin.fused_gemm = fused
                lin(x)

        def run_bf16():
            for w in bf16:
                F.linear(x, w)

        lin0.fused_gemm = True
        max_diff = float((lin0(x).float() - F.linear(x, w_eff).float())
                         .abs().max())
        # the route is fixed when the step is captured
        variants = {
            "fp8_gemm": (_capture(torch, lambda: run_fp8(True)), copies8, 1),
            "dequant_route": (_capture(torch, lambda: run_fp8(False)),
                              copies8, 1),
            "bf16_library": (_capture(torch, run_bf16), copies16, 2)}
        for fn, _, _ in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, (fn, copies, _) in variants.items():
                times[name].append(_time_step(torch, fn, iters) / copies)
        flops = 2 * m * n * k
        out = {"M": m, "N": n, "K": k, "tile": hr.fp8w_gemm_tile(m, n),
               "fp8_gemm_vs_bf16_max_abs_diff": max_diff}
        for name, ts in times.items():
            _, copies, elem = variants[name]
            need = n * k * elem + 2 * m * k + 2 * m * n
            t_flops = flops / PEAK_BF16_FLOPS
            t_bytes = need / PEAK_BYTES_PER_S
            us = statistics.median(ts)
            out[name] = {
                "copies_per_step": copies,
                "us_per_call": round(us, 2),
                "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                "TFLOP_per_s": round(flops / us / 1e6, 1),
                "needed_bytes": need,
                "bound": "flops" if t_flops > t_bytes else "bytes",
                "share_of_bound": round(max(t_flops, t_bytes) / (us * 1e-6),
                                        3),
            }
        out["fp8_gemm_over_dequant_time"] = round(
            out["fp8_gemm"]["us_per_call"]
            / out["dequant_route"]["us_per_call"], 3)
        out["fp8_gemm_over_bf16_time"] = round(
            out["fp8_gemm"]["us_per_call"]
            / out["bf16_library"]["us_per_call"], 3)
        rows.append(out)
        print(json.dumps(out), flush=True)
    return rows


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
    ap.add_argument("--wide", action="store_true",
                    help="only the M > 16 section: fp8w_gemm_bf16 against "
                         "the dequant route and the bf16 library GEMM")
    ap.add_argument("--memory", action="store_true",
                    help="also build and quantise the 8B model")
    args = ap.parse_args()

    import torch

    from client_amd.models.llama import (LlamaConfig, llama3_8b_config,
                                         llama_tiny_config)

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a CPU run gives no timing")
    if args.wide:
        report = {"wide": []}
        with torch.inference_mode():
            for n, k in SHAPES:
                report["wide"] += bench_wide(torch, n, k, args.rounds,
                                             args.iters)
                torch.cuda.empty_cache()
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)
        return
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
