"""Per-shape timing of the ResNet50 NCHW epilogue kernels at the shapes of
one batch-32 forward: bias+ReLU (33 launches), bias+residual+ReLU (16)
and the stem bias+ReLU+max-pool.

Each shape is launched back to back on one stream (in place, as the
model does) and timed with device events, so the tensors are as
cache-warm as they are behind the conv that feeds them in the served
graph. Prints one JSON line per shape with µs per launch and achieved
GB/s (bytes the pass must move: 4 B/element for bias+ReLU, 6 with the
residual, input + pooled output for the stem), then the per-forward sum
weighted by how often each shape occurs.

    python scripts/bench_epilogue.py [--repo OTHER_CHECKOUT] [--batch 32]

--repo times another checkout's build (e.g. the parent commit) with the
same script.
"""

import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import torch  # noqa: E402

from client_amd.ops import hip_runtime as hr  # noqa: E402

# (kind, channels, h, w, launches per forward)
SHAPES = [
    ("bias_act", 64, 112, 112, 1),  # stem (separate pass before the fusion)
    ("bias_act", 64, 56, 56, 6),
    ("bias_act", 128, 56, 56, 1),
    ("bias_act", 128, 28, 28, 7),
    ("bias_act", 256, 28, 28, 1),
    ("bias_act", 256, 14, 14, 11),
    ("bias_act", 512, 14, 14, 1),
    ("bias_act", 512, 7, 7, 5),
    ("bias_res_act", 256, 56, 56, 3),
    ("bias_res_act", 512, 28, 28, 4),
    ("bias_res_act", 1024, 14, 14, 6),
    ("bias_res_act", 2048, 7, 7, 3),
    ("maxpool_torch", 64, 112, 112, 1),
    ("stem_fused", 64, 112, 112, 1),
]


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / args.iters)
    return statistics.median(out)


def main():
    n = args.batch
    stream = torch.cuda.current_stream().cuda_stream
    have_stem = True
    try:
        hr.bias_relu_maxpool_bf16
    except AttributeError:
        have_stem = False
    torch.manual_seed(0)
    per_forward = 0.0
    for kind, c, h, w, count in SHAPES:
        x = torch.randn(n, c, h, w, device="cuda", dtype=torch.bfloat16)
        r = torch.randn_like(x)
        bias = torch.full((c,), 1e-3, device="cuda", dtype=torch.float32)
        numel = x.numel()
        if kind == "bias_act":
            if c == 64 and h == 112 and have_stem:
                continue  # the fused stem replaces this pass
            nbytes = 4 * numel

            def fn():
                hr.bias_act_bf16(x.data_ptr(), bias.data_ptr(), x.data_ptr(),
                                 n * c, h * w, c, True, stream)
        elif kind == "bias_res_act":
            nbytes = 6 * numel

            def fn():
                hr.bias_res_act_bf16(x.data_ptr(), r.data_ptr(),
                                     bias.data_ptr(), x.data_ptr(), n * c,
                                     h * w, c, True, stream)
        elif kind == "maxpool_torch":
            if have_stem:
                continue
            nbytes = 2 * numel + 2 * numel // 4

            def fn():
                torch.nn.functional.max_pool2d(x, 3, 2, 1)
        else:
            if not have_stem:
                continue
            out = torch.empty(n, c, h // 2, w // 2, device="cuda",
                              dtype=torch.bfloat16)
            nbytes = 2 * numel + 2 * out.numel()

            def fn():
                hr.bias_relu_maxpool_bf16(x.data_ptr(), bias.data_ptr(),
                                          out.data_ptr(), n * c, c, h, w,
                                          stream)
        us = timed(fn)
        per_forward += us * count
        print(json.dumps({
            "kind": kind, "shape": [n, c, h, w], "plane": h * w,
            "launches_per_forward": count, "us": round(us, 2),
            "GBps": round(nbytes / us / 1e3, 1),
        }), flush=True)
    print(json.dumps({"per_forward_us": round(per_forward, 1),
                      "fused_stem": have_stem}), flush=True)


if __name__ == "__main__":
    main()
