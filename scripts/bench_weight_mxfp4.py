"""MXFP4-weight decode GEMM microbenchmark, memory and drift report (MI355X).

    python scripts/bench_weight_mxfp4.py --json out.json [--memory] [--drift]

Kernel time: µs per call at M = 8 on the 8B model's projection and FFN
shapes of mxfp4w_decode_gemm_bf16, fp8w_decode_gemm_bf16 and F.linear on
bf16 weights (the library GEMM), all three on the same W_eff-sized
problem in one process. As in bench_weight_fp8.py, one "step" walks
enough distinct weight copies that their total exceeds 512 MiB, each
variant's step is captured into a hipGraph, and a time is the median
over rounds of (device-event time of a replay) / copies, the variants
alternating within a round; min and max over rounds are the spread.
Achieved bytes/s counts the bytes the algorithm needs: N K (1/2 + 1/32)
for mxfp4, N K for fp8, 2 N K for bf16.

Wide GEMM (--wide, nothing else then runs): the same method at M = 24 to
1024 for mxfp4w_gemm_bf16, the dequant route (mxfp4w_dequant_bf16 into
the shared scratch + F.linear, what serving runs without
--mxfp4-weight-gemm) and F.linear on bf16 W_eff.

Memory (--memory): torch.cuda.memory_allocated() before and after
quantising the 8B model. Drift (--drift): the largest absolute logit
difference and the argmax agreement between the quantised and the bf16
model, same seeded weights. Random-init weights have no outlier
channels, so this says nothing about real checkpoints.
"""

import argparse
import copy
import json
import statistics

from bench_weight_fp8 import (M, PEAK_BF16_FLOPS, PEAK_BYTES_PER_S, SHAPES,
                              WALK_BYTES, WIDE_M, _capture, _decode_logits,
                              _time_step)


def bench_kernel(torch, n, k, rounds, iters):
    import torch.nn.functional as F

    from client_amd.models import weight_fp8, weight_mxfp4

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(n + k)
    x = torch.randn(M, k, device=dev, generator=g).to(torch.bfloat16)
    w0 = torch.randn(n, k, device=dev, generator=g) * k ** -0.5
    mx0 = weight_mxfp4.Mxfp4Linear(
        *weight_mxfp4.quantize_weight(w0)).to(dev)
    f80 = weight_fp8.Fp8Linear(*weight_fp8.quantize_weight(w0)).to(dev)
    w_eff = mx0.effective_weight(torch.bfloat16)
    # bytes per weight element times 32
    per32 = {"mxfp4_kernel": 17, "fp8_kernel": 32, "bf16_library": 64}
    need = {name: n * k * v // 32 for name, v in per32.items()}
    copies = {name: WALK_BYTES // b + 1 for name, b in need.items()}
    mx = [mx0] + [copy.deepcopy(mx0) for _ in range(copies["mxfp4_kernel"] - 1)]
    f8 = [f80] + [copy.deepcopy(f80) for _ in range(copies["fp8_kernel"] - 1)]
    bf = [w_eff] + [w_eff.clone() for _ in range(copies["bf16_library"] - 1)]

    # outputs agree before anything is timed
    max_diff = float((mx0(x).float() - F.linear(x, w_eff).float())
                     .abs().max())
    runs = {"mxfp4_kernel": lambda: [lin(x) for lin in mx],
            "fp8_kernel": lambda: [lin(x) for lin in f8],
            "bf16_library": lambda: [F.linear(x, w) for w in bf]}
    replays = {name: _capture(torch, fn) for name, fn in runs.items()}
    for fn in replays.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in replays}
    for _ in range(rounds):
        for name, fn in replays.items():
            times[name].append(_time_step(torch, fn, iters) / copies[name])
    out = {"M": M, "N": n, "K": k, "mxfp4_vs_bf16_max_abs_diff": max_diff}
    for name, ts in times.items():
        us = statistics.median(ts)
        out[name] = {
            "copies_per_step": copies[name],
            "us_per_call": round(us, 2),
            "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
            "needed_bytes": need[name],
            "achieved_TB_per_s": round(need[name] / us / 1e6, 3),
            "share_of_6.3TBps": round(
                need[name] / (us * 1e-6) / PEAK_BYTES_PER_S, 3),
        }
    for other in ("fp8_kernel", "bf16_library"):
        out[f"mxfp4_over_{other}_time"] = round(
            out["mxfp4_kernel"]["us_per_call"] / out[other]["us_per_call"], 3)
    return out


def bench_wide(torch, n, k, rounds, iters):
    """--wide: M > 16 on mxfp4w_gemm_bf16, on the dequant route (what
    Mxfp4Linear runs without wide_gemm) and on F.linear with bf16 W_eff;
    the method of bench_kernel. The bound of a call is the larger of
    2 M N K FLOPs at the bf16 MFMA roof and the bytes the algorithm needs
    (codes and scales, or bf16 weights, once, x once, y once) at the HBM
    read rate."""
    import torch.nn.functional as F

    from client_amd.models import weight_mxfp4
    from client_amd.ops import hip_runtime as hr

    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(n + k)
    w0 = torch.randn(n, k, device=dev, generator=g) * k ** -0.5
    mx0 = weight_mxfp4.Mxfp4Linear(
        *weight_mxfp4.quantize_weight(w0)).to(dev)
    w_eff = mx0.effective_weight(torch.bfloat16)
    wbytes = {"mxfp4_gemm": n * k * 17 // 32, "dequant_route": n * k * 17 // 32,
              "bf16_library": 2 * n * k}
    copies = {name: WALK_BYTES // b + 1 for name, b in wbytes.items()}
    mx = [mx0] + [copy.deepcopy(mx0) for _ in range(copies["mxfp4_gemm"] - 1)]
    for lin in mx:  # one dequant scratch for all, as in a model
        lin._scratch = mx0._scratch
    bf = [w_eff] + [w_eff.clone() for _ in range(copies["bf16_library"] - 1)]
    rows = []
    for m in WIDE_M:
        x = torch.randn(m, k, device=dev, generator=g).to(torch.bfloat16)

        def run_mx(wide):
            for lin in mx:
                lin.wide_gemm = wide
                lin(x)

        mx0.wide_gemm = True
        max_diff = float((mx0(x).float() - F.linear(x, w_eff).float())
                         .abs().max())
        # the route is fixed when the step is captured
        replays = {
            "mxfp4_gemm": _capture(torch, lambda: run_mx(True)),
            "dequant_route": _capture(torch, lambda: run_mx(False)),
            "bf16_library": _capture(
                torch, lambda: [F.linear(x, w) for w in bf])}
        for fn in replays.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in replays}
        for _ in range(rounds):
            for name, fn in replays.items():
                times[name].append(_time_step(torch, fn, iters) / copies[name])
        flops = 2 * m * n * k
        out = {"M": m, "N": n, "K": k, "tile": hr.mxfp4w_gemm_tile(m, n),
               "mxfp4_gemm_vs_bf16_max_abs_diff": max_diff}
        for name, ts in times.items():
            need = wbytes[name] + 2 * m * k + 2 * m * n
            t_flops = flops / PEAK_BF16_FLOPS
            t_bytes = need / PEAK_BYTES_PER_S
            us = statistics.median(ts)
            out[name] = {
                "copies_per_step": copies[name],
                "us_per_call": round(us, 2),
                "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                "TFLOP_per_s": round(flops / us / 1e6, 1),
                "needed_bytes": need,
                "bound": "flops" if t_flops > t_bytes else "bytes",
                "bound_us": round(max(t_flops, t_bytes) * 1e6, 2),
                "share_of_bound": round(max(t_flops, t_bytes) / (us * 1e-6),
                                        3),
            }
        for other in ("dequant_route", "bf16_library"):
            out[f"mxfp4_gemm_over_{other}_time"] = round(
                out["mxfp4_gemm"]["us_per_call"] / out[other]["us_per_call"],
                3)
        rows.append(out)
        print(json.dumps(out), flush=True)
    return rows


def drift(torch, cfg, prompt_len, n_steps, seed):
    from client_amd.models.llama import LlamaModel
    from client_amd.models.weight_mxfp4 import quantize_llama_weights_as

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
        quantize_llama_weights_as(model, "mxfp4")
        b = _decode_logits(torch, model, prompt, steps)
    return {"prompt_tokens": prompt_len, "decode_steps": n_steps,
            "max_abs_logit_diff": float((a - b).abs().max()),
            "logit_abs_max": float(a.abs().max()),
            "logit_std": float(a.std()),
            "argmax_agree": float((a.argmax(-1) == b.argmax(-1))
                                  .float().mean())}


def memory(torch):
    from client_amd.models.llama import LlamaModel, llama3_8b_config
    from client_amd.models.weight_mxfp4 import quantize_llama_weights_as

    dev = "cuda:0"
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    with torch.device(dev):
        model = LlamaModel(llama3_8b_config())
    model = model.to(torch.bfloat16).eval()
    before = torch.cuda.memory_allocated() - base
    replaced_before, replaced_after = quantize_llama_weights_as(model, "mxfp4")
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
    ap.add_argument("--drift", action="store_true")
    ap.add_argument("--wide", action="store_true",
                    help="only the M > 16 section: mxfp4w_gemm_bf16 against "
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
    report = {"kernel": [], "drift": None, "memory": None}
    with torch.inference_mode():
        for n, k in SHAPES:
            r = bench_kernel(torch, n, k, args.rounds, args.iters)
            report["kernel"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if args.drift:
        one = LlamaConfig(**{**llama3_8b_config().__dict__, "n_layers": 1})
        report["drift"] = {
            "llama_tiny": drift(torch, llama_tiny_config(), 40, 60, 0),
            "llama3_8b_one_layer": drift(torch, one, 256, 64, 0)}
        print(json.dumps(report["drift"]), flush=True)
    if args.memory:
        report["memory"] = memory(torch)
        print(json.dumps(report["memory"]), flush=True)
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
