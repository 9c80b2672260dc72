"""Per-request token sampling: temperature, top-k, top-p and seed.

The contract, per row of logits (the HIP kernel sample_logits_bf16 in
client_amd/ops/csrc/kernels.hip and the numpy path below both follow
it; tests/sampling_refs.py states it in float64):

- Sanitised logits: NaN reads as -inf, +inf as the largest finite bf16.
  A row with no finite logit yields token 0.
- temperature == 0 yields the lowest index holding the maximum.
- Top-k, ties included: K = {i : l_i >= the k-th largest logit}.
  top_k <= 0 or >= vocab turns it off.
- Weights w_i = exp((l_i - l_max) / temperature) over K, S_K their sum.
- Top-p, ties included, over distinct values d_1 > d_2 > ... in K:
  M_j is the weight of {l_i >= d_j}, j* the smallest j with
  M_j >= top_p * S_K, N = {i : l_i >= d_j*}. top_p >= 1 turns it off.
- u = (x0 >> 8) * 2^-24 with x0 word 0 of Philox4x32-10, counter
  (step_lo32, step_hi32, 0, 0), key (seed_lo32, seed_hi32).
- The token is the first index of N, in index order, whose running sum
  of w exceeds u * S_N; if rounding leaves none, the last index of N.

The draw depends on (row contents, parameters, seed, step) alone: not on
the row's slot, on what else shares the batch, or on how often a
captured graph has been replayed.
"""

import math
import secrets
from dataclasses import dataclass
from typing import Optional

import numpy as np

BF16_MAX = 3.3895313892515355e38  # largest finite bf16

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


@dataclass
class SamplingParams:
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: Optional[int] = None

    def validate(self):
        """Raises ValueError naming the offending parameter."""
        t = float(self.temperature)
        if math.isnan(t) or t < 0.0:
            raise ValueError(
                f"temperature must be >= 0, got {self.temperature}")
        p = float(self.top_p)
        if math.isnan(p) or not (0.0 < p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}")
        if int(self.top_k) < 0:
            raise ValueError(f"top_k must be >= 0, got {self.top_k}")
        return self

    @property
    def is_greedy(self):
        return float(self.temperature) == 0.0

    def with_seed(self):
        """A copy whose seed is set: a missing one becomes a random
        64-bit value."""
        seed = self.seed if self.seed is not None else secrets.randbits(64)
        return SamplingParams(float(self.temperature), int(self.top_k),
                              float(self.top_p), int(seed) & (2 ** 64 - 1))


def seed_to_i64(seed):
    """An unsigned 64-bit seed as the int64 with the same bits (torch has
    no uint64 arithmetic; the kernel reads the bits back as u64)."""
    seed = int(seed) & (2 ** 64 - 1)
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def philox4x32_10(counter, key):
    """Philox4x32-10: counter 4 x u32, key 2 x u32 -> 4 x u32."""
    c0, c1, c2, c3 = (int(c) & _U32 for c in counter)
    k0, k1 = (int(k) & _U32 for k in key)
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _U32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _U32)
        k0 = (k0 + _W0) & _U32
        k1 = (k1 + _W1) & _U32
    return c0, c1, c2, c3


def uniform_for(seed, step):
    """The contract's u in [0, 1) for a (seed, step) pair."""
    seed = int(seed) & (2 ** 64 - 1)
    step = int(step) & (2 ** 64 - 1)
    x0 = philox4x32_10((step & _U32, step >> 32, 0, 0),
                       (seed & _U32, seed >> 32))[0]
    return (x0 >> 8) * 2.0 ** -24


def _sample_row(logits, temperature, top_k, top_p, seed, step):
    l = np.asarray(logits, dtype=np.float32).copy()
    l[np.isnan(l)] = -np.inf
    l[l == np.inf] = np.float32(BF16_MAX)
    if not np.isfinite(l).any():
        return 0
    if not temperature > 0.0:
        return int(np.argmax(l))  # first index of the maximum
    vocab = l.shape[0]
    keep = np.ones(vocab, dtype=bool)
    if 0 < top_k < vocab:
        keep = l >= np.partition(l, vocab - top_k)[vocab - top_k]
    # float64 weights: inside the error the contract's fp32 weights allow
    l64 = l.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = np.exp((l64 - l64.max()) / float(np.float32(temperature)))
    w = np.where(keep & (l > -np.inf), w, 0.0)
    if top_p < 1.0:
        vals, inv = np.unique(l[keep], return_inverse=True)  # ascending
        mass = np.bincount(inv, weights=w[keep], minlength=len(vals))
        tail = np.cumsum(mass[::-1])  # M_j for d_1 > d_2 > ...
        j = int(np.searchsorted(tail, np.float64(top_p) * w.sum(),
                                side="left"))
        j = min(j, len(vals) - 1)
        keep &= l >= vals[len(vals) - 1 - j]
        w = np.where(keep, w, 0.0)
    idx = np.flatnonzero(keep)
    c = np.cumsum(w[idx])
    hit = np.flatnonzero(c > uniform_for(seed, step) * c[-1])
    return int(idx[hit[0]] if len(hit) else idx[-1])


def _sample_host(logits, temperature, top_k, top_p, seed, step):
    l = np.asarray(logits, dtype=np.float32)
    rows = l.shape[0]
    t = np.asarray(temperature, dtype=np.float32).reshape(rows)
    k = np.asarray(top_k, dtype=np.int64).reshape(rows)
    p = np.asarray(top_p, dtype=np.float32).reshape(rows)
    s = np.asarray(seed).astype(np.int64).reshape(rows)
    n = np.asarray(step, dtype=np.int64).reshape(rows)
    return np.array(
        [_sample_row(l[i], float(t[i]), int(k[i]), float(p[i]),
                     int(s[i]), int(n[i])) for i in range(rows)],
        dtype=np.int64,
    )


def sample_tokens(logits, temperature, top_k, top_p, seed, step, out=None):
    """One token per row of ``logits`` [rows, vocab].

    temperature f32, top_k i32, top_p f32, seed i64 (the bits of the u64
    seed) and step i64 are per-row tensors of ``rows`` elements. A
    contiguous bf16 tensor on the GPU goes to the HIP kernel on the
    current stream, with every parameter tensor on the same device and
    nothing read back; it can be captured into a hipGraph. Everything
    else (host tensors, fp32) takes the numpy path of the same contract,
    which is what a scheduler on ``device="cpu"`` runs.
    Returns int64 [rows] (``out`` if given)."""
    import torch

    rows, vocab = logits.shape
    if (logits.is_cuda and logits.dtype == torch.bfloat16
            and logits.is_contiguous()):
        from ..ops import hip_runtime as hr

        if out is None:
            out = torch.empty(rows, dtype=torch.int64, device=logits.device)
        want = ((temperature, torch.float32), (top_k, torch.int32),
                (top_p, torch.float32), (seed, torch.int64),
                (step, torch.int64), (out, torch.int64))
        for t, dt in want:
            if (t.dtype != dt or t.device != logits.device
                    or t.numel() != rows or not t.is_contiguous()):
                raise ValueError(
                    "sample_tokens: parameter tensors must be contiguous, "
                    f"on {logits.device}, with {rows} elements and dtypes "
                    "f32/i32/f32/i64/i64 (out i64)")
        hr.sample_logits_bf16(
            logits.data_ptr(), temperature.data_ptr(), top_k.data_ptr(),
            top_p.data_ptr(), seed.data_ptr(), step.data_ptr(),
            out.data_ptr(), rows, vocab,
            torch.cuda.current_stream().cuda_stream,
        )
        return out

    def host(t):
        return t.detach().cpu().numpy() if torch.is_tensor(t) else t

    tokens = torch.from_numpy(_sample_host(
        host(logits.float()), host(temperature), host(top_k), host(top_p),
        host(seed), host(step)))
    if out is None:
        return tokens.to(logits.device)
    out.copy_(tokens)
    return out


def param_tensors(params_list, steps, device):
    """Per-row parameter tensors for ``sample_tokens`` from a list of
    SamplingParams (None = greedy) and their steps."""
    import torch

    ps = [p if p is not None else SamplingParams(seed=0)
          for p in params_list]
    return (
        torch.tensor([p.temperature for p in ps], dtype=torch.float32,
                     device=device),
        torch.tensor([p.top_k for p in ps], dtype=torch.int32,
                     device=device),
        torch.tensor([p.top_p for p in ps], dtype=torch.float32,
                     device=device),
        torch.tensor([seed_to_i64(p.seed or 0) for p in ps],
                     dtype=torch.int64, device=device),
        torch.tensor(list(steps), dtype=torch.int64, device=device),
    )
