"""Per-shape timing of the stride-1 1x1 convs of a ResNet50 forward with
their epilogue, at the shapes the served model runs, library path against
the fused conv1x1 kernel in one process.

Per shape and mode the two paths alternate, `--rounds` times:
  lib     conv(x) then the epilogue module: BiasAct for mode "act"
          (conv1), BiasResAct with the block's identity for mode "res"
          (conv3); mode "ds" is the layer1 downsample conv alone
  kernel  Conv1x1BiasAct, called whether or not the shape is in the
          dispatch table ("ds": zero bias, no ReLU)

A round is the median of `--repeats` windows of `--iters` calls, timed
with device events. By default the window is one hipGraph replay of the
captured calls, as the server replays its forward, so the figure holds no
Python call overhead; --timing eager launches them from Python instead.

Prints one JSON line per shape, mode and batch: each path's rounds in µs,
the kernel's TFLOP/s (2*N*HW*K*C) and GB/s over the bytes the fused path
must move (input + output + residual + weights, once each), and `admit`:
the kernel's slowest round is below the library's fastest. A shape/mode
belongs in CONV1X1_TABLE when `admit` holds at batch 8 and at batch 32;
the last line lists those, and mode "ds" apart: the model never routes it
to the kernel.

    python scripts/bench_conv1x1.py [--batches 8,32] [--only 256x64x56]
        [--out FILE.jsonl]
"""

import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="8,32")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--timing", choices=("graph", "eager"), default="graph")
ap.add_argument("--only", default=None, help="one shape, as CxKxH")
ap.add_argument("--out", default=None, help="append the JSON lines here")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

import torch  # noqa: E402

from client_amd.models import resnet  # noqa: E402

# (C_in, C_out, H = W, mode, occurrences per forward)
SHAPES = [
    (64, 64, 56, "act", 1),
    (256, 64, 56, "act", 2),
    (256, 128, 56, "act", 1),
    (512, 128, 28, "act", 3),
    (512, 256, 28, "act", 1),
    (1024, 256, 14, "act", 5),
    (1024, 512, 14, "act", 1),
    (2048, 512, 7, "act", 2),
    (64, 256, 56, "res", 3),
    (128, 512, 28, "res", 4),
    (256, 1024, 14, "res", 6),
    (512, 2048, 7, "res", 3),
    (64, 256, 56, "ds", 1),
]


def timed(fn):
    """µs per call: median of args.repeats windows of args.iters calls"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    graph = None
    if args.timing == "graph":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.iters):
                fn()
        graph.replay()
        torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        if graph is not None:
            graph.replay()
        else:
            for _ in range(args.iters):
                fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / args.iters)
    return statistics.median(out)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def main():
    torch.manual_seed(0)
    admitted = {}
    with torch.inference_mode():
        for c, k, h, mode, count in SHAPES:
            if args.only and args.only != f"{c}x{k}x{h}":
                continue
            for n in map(int, args.batches.split(",")):
                conv = torch.nn.Conv2d(c, k, 1, bias=False).to(
                    "cuda", torch.bfloat16)
                x = torch.randn(n, c, h, h, device="cuda",
                                dtype=torch.bfloat16)
                res = None
                if mode == "res":
                    ba = resnet.BiasResAct(torch.randn(k) * 0.1).to("cuda")
                    res = torch.randn(n, k, h, h, device="cuda",
                                      dtype=torch.bfloat16)

                    def lib():
                        ba(conv(x), res)
                elif mode == "act":
                    ba = resnet.BiasAct(torch.randn(k) * 0.1,
                                        relu=True).to("cuda")

                    def lib():
                        ba(conv(x))
                else:
                    ba = resnet.BiasAct(torch.zeros(k), relu=False).to(
                        "cuda")

                    def lib():
                        conv(x)
                mod = resnet.Conv1x1BiasAct()

                def kernel():
                    mod(x, conv, ba, res, relu=mode != "ds")

                rounds = {"lib": [], "kernel": []}
                for _ in range(args.rounds):
                    rounds["lib"].append(round(timed(lib), 2))
                    rounds["kernel"].append(round(timed(kernel), 2))
                us = statistics.median(rounds["kernel"])
                flop = 2.0 * n * h * h * k * c
                nbytes = 2 * (x.numel() + n * k * h * h * (2 if res is not None
                                                          else 1) + c * k)
                admit = max(rounds["kernel"]) < min(rounds["lib"])
                admitted.setdefault((c, k, h, h, mode), []).append(admit)
                emit({
                    "shape": [c, k, h, h], "mode": mode, "batch": n,
                    "per_forward": count, "timing": args.timing,
                    "lib_us": rounds["lib"], "kernel_us": rounds["kernel"],
                    "ratio": round(min(rounds["lib"]) / max(rounds["kernel"]),
                                   2),
                    "TFLOPs": round(flop / us / 1e6, 1),
                    "GBps": round(nbytes / us / 1e3, 1),
                    "admit": admit,
                })
    # "ds" has no table entry: the model does not route it to the kernel
    emit({"admitted": [list(key) for key, oks in admitted.items()
                       if all(oks) and key[4] != "ds"],
          "wins_but_not_wired": [list(key) for key, oks in admitted.items()
                                 if all(oks) and key[4] == "ds"]})


if __name__ == "__main__":
    main()
