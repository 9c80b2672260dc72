"""BERT encoder attention microbenchmark (MI355X).

    python scripts/bench_encoder_attention.py --json out.json

µs per layer of the attention block of BertLayer at the BERT-large shape
(16 heads, d = 64, hidden 1024) and B = 8, both ways:

  torch   the nn.MultiheadAttention call (in-projection, attention with
          key_padding_mask when masked, out-projection);
  fused   what the fused path runs in its place: F.linear with the packed
          in-projection, encoder_attention on its output in place, and
          out_proj;
  kernel  encoder_attention alone on a ready qkv (the part that is new).

Once unmasked and once with the row lengths S, 3S/4, S/2, S/4 repeated to
fill the 8 rows. One "step" walks 24 distinct layers (weights and inputs),
as a forward does, so nothing is served from the last call's cache lines.
Each variant's step is captured into a hipGraph, as serving runs it; a
time is the median over rounds of (device-event time of a replay) / 24,
the variants alternating within a round.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_decode_attention import _capture, _time_step  # noqa: E402

HEADS, D, B = 16, 64, 8
HIDDEN = HEADS * D
LAYERS = 24


def bench(torch, s, masked, rounds, iters):
    import torch.nn.functional as F

    from client_amd.models.bert import BertEncoder, encoder_attention

    dev = "cuda:0"
    torch.manual_seed(s + int(masked))
    attns = [torch.nn.MultiheadAttention(HIDDEN, HEADS, batch_first=True)
             .to(dev).to(torch.bfloat16).eval() for _ in range(LAYERS)]
    xs = [torch.randn(B, s, HIDDEN, device=dev).to(torch.bfloat16)
          for _ in range(LAYERS)]
    if masked:
        lens = [s, 3 * s // 4, s // 2, s // 4] * (B // 4)
        mask = torch.zeros(B, s, dtype=torch.int64, device=dev)
        for i, n in enumerate(lens):
            mask[i, :n] = 1
    else:
        lens = [s] * B
        mask = None
    pad = None if mask is None else mask == 0
    key_mask, kv_len = BertEncoder._fused_mask(mask, B, s, dev)
    qkvs = [F.linear(x, a.in_proj_weight, a.in_proj_bias)
            for x, a in zip(xs, attns)]

    def torch_block(a, x, qkv):
        return a(x, x, x, key_padding_mask=pad, need_weights=False)[0]

    def fused_block(a, x, qkv):
        qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)
        return a.out_proj(encoder_attention(qkv, key_mask, kv_len, HEADS))

    def kernel_only(a, x, qkv):
        return encoder_attention(qkv, key_mask, kv_len, HEADS)

    def loop(block):
        def run():
            for a, x, qkv in zip(attns, xs, qkvs):
                block(a, x, qkv)
        return run

    # outputs agree at the real positions before anything is timed
    ref = torch_block(attns[0], xs[0], qkvs[0]).float()
    got = fused_block(attns[0], xs[0], qkvs[0]).float()
    max_diff = max(float((ref[i, :n] - got[i, :n]).abs().max())
                   for i, n in enumerate(lens))
    variants = {"torch": loop(torch_block), "fused": loop(fused_block),
                "kernel": loop(kernel_only)}
    variants = {name: _capture(torch, fn) for name, fn in variants.items()}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time_step(torch, fn, iters) / LAYERS)
    pairs = sum(n * n for n in lens)          # (query, key) pairs computed
    flops = 4 * D * HEADS * pairs             # QK^T and PV, 2 flops per MAC
    out = {"s": s, "b": B, "masked": masked, "row_lens": lens,
           "fused_vs_torch_max_abs_diff": max_diff,
           "useful_attention_flops": flops}
    for name, ts in times.items():
        us = statistics.median(ts)
        out[name] = {"us_per_layer": round(us, 2),
                     "us_min": round(min(ts), 2),
                     "us_max": round(max(ts), 2)}
    out["kernel"]["TF_per_s"] = round(
        flops / out["kernel"]["us_per_layer"] / 1e6, 2)
    out["fused_over_torch"] = round(
        out["fused"]["us_per_layer"] / out["torch"]["us_per_layer"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", required=True)
    ap.add_argument("--seqs", type=int, nargs="+", default=[128, 384, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a CPU run gives no timing")
    report = {"shape": {"heads": HEADS, "d": D, "b": B},
              "layers_per_step": LAYERS, "kernel": []}
    with torch.inference_mode():
        for s in args.seqs:
            for masked in (False, True):
                r = bench(torch, s, masked, args.rounds, args.iters)
                report["kernel"].append(r)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
