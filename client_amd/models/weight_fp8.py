"""FP8 (e4m3) weight-only linear layers for the Llama decode path.

Format. A weight ``W[N, K]`` is stored as ``codes`` (uint8 OCP e4m3fn)
and ``scale_exp`` (int8 ``[N]``); its value is

    W_eff[n, k] = decode(codes[n, k]) * 2^scale_exp[n].

The scales are powers of two kept as integer exponents: ``module.to(dtype)``
cannot touch an int8 buffer, the multiply is exact, and every ``W_eff``
element (at most 4 significant bits times a power of two) is exactly a
bf16 value. So the quantised model is, by definition, the bf16 model
loaded with ``W_eff``; activations are never quantised (W8A16).

Layout. ``Fp8Linear.codes`` holds the codes pre-tiled for the decode
kernel (ops/csrc/weight_fp8.hip): tiles of 16 rows x 64 k, each one
lane-linear 1 KiB run,

    packed[((t * K/64 + c) * 64 + lane) * 16 + b]
        = codes[16 t + (lane & 15)][64 c + 16 (lane >> 4) + b],

rows padded to a multiple of 16. A wave's 16-byte lane loads are then
whole contiguous lines; with row-major codes the same load would touch
16 rows x 64 B. ``pack_codes`` / ``unpack_codes`` are the only code that
knows the permutation on the host; both kernels read it. K must be a
multiple of 64.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from .kv_cache import FP8_MAX, kv_decode_fp8, kv_encode_fp8

WEIGHT_DTYPES = ("bf16", "fp8_e4m3")

TILE_ROWS = 16
TILE_K = 64
MAX_DECODE_M = 16
SCALE_EXP_MIN = -100
SCALE_EXP_MAX = 100

LLAMA_BLOCK_LINEARS = ("wq", "wk", "wv", "wo", "w1", "w3", "w2")


def normalize_weight_dtype(weight_dtype):
    """None / "bf16" -> None (weights stay in the model dtype);
    "fp8_e4m3" stays; anything else raises."""
    if weight_dtype is None or weight_dtype == "bf16":
        return None
    if weight_dtype == "fp8_e4m3":
        return weight_dtype
    raise ValueError(f"unknown weight_dtype {weight_dtype!r}; expected one "
                     f"of {WEIGHT_DTYPES}")


def quantize_weight(w):
    """``w`` [N, K] float -> (codes uint8 [N, K] row-major, scale_exp int8
    [N]). Per row e = ceil(log2(amax / 448)) clamped to [-100, 100] (0
    for an all-zero row), the smallest exponent at which the row fits
    e4m3, and codes = kv_encode_fp8(w / 2^e): round to nearest even,
    saturation only on rows whose exponent was clamped. A non-finite
    weight raises ValueError naming the row."""
    if w.dim() != 2:
        raise ValueError(f"expected a [N, K] weight, got {tuple(w.shape)}")
    w = w.detach().float()
    bad = ~torch.isfinite(w).all(dim=1)
    if bad.any():
        row = int(torch.nonzero(bad)[0])
        raise ValueError(f"non-finite weight in row {row}")
    amax = w.abs().amax(dim=1)
    # amax = m 2^ex with m in [0.5, 1), 448 = 0.875 2^9: the smallest e
    # with amax <= 448 2^e, in integers
    m, ex = torch.frexp(amax)
    e = torch.where(m <= FP8_MAX / 512.0, ex - 9, ex - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    e = e.clamp(SCALE_EXP_MIN, SCALE_EXP_MAX)
    # exact: a power-of-two scaling (results below the fp32 normal range
    # are far below e4m3's and encode as zero either way)
    codes = kv_encode_fp8(torch.ldexp(w, -e[:, None]))
    return codes, e.to(torch.int8)


def dequantize_weight(codes, scale_exp, dtype):
    """Row-major ``codes`` [N, K] and ``scale_exp`` [N] -> W_eff [N, K]
    as ``dtype`` (exact for bf16 and wider)."""
    w = torch.ldexp(kv_decode_fp8(codes, torch.float32),
                    scale_exp.to(torch.int32)[:, None])
    return w.to(dtype)


def pack_codes(codes, pad=0):
    """Row-major codes [N, K] -> the flat tiled layout (module
    docstring), pad rows filled with ``pad``."""
    n, k = codes.shape
    if k % TILE_K != 0 or k == 0:
        raise ValueError(f"in_features {k} is not a multiple of {TILE_K}")
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    full = codes.new_full((tiles * TILE_ROWS, k), pad)
    full[:n] = codes
    # [t, r, c, q, b] -> [t, c, q, r, b]; lane = 16 q + r
    t = full.view(tiles, TILE_ROWS, k // TILE_K, 4, 16)
    return t.permute(0, 2, 3, 1, 4).contiguous().view(-1)


def unpack_codes(packed, n, k):
    """The inverse of pack_codes: flat tiled codes -> row-major [n, k]."""
    tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    t = packed.view(tiles, k // TILE_K, 4, TILE_ROWS, 16)
    full = t.permute(0, 3, 1, 2, 4).reshape(tiles * TILE_ROWS, k)
    return full[:n].contiguous()


class _Scratch:
    """One bf16 buffer for the dequantised weight of whichever layer is
    running, shared by the Fp8Linears of a model."""

    def __init__(self):
        self.buf = None

    def reserve(self, numel, device):
        if (self.buf is None or self.buf.device != device
                or self.buf.numel() < numel):
            self.buf = torch.empty(numel, device=device,
                                   dtype=torch.bfloat16)
        return self.buf


class Fp8Linear(nn.Module):
    """y = x @ W_eff^T, no bias. Buffers ``codes`` (tiled, see the module
    docstring) and ``scale_exp``.

    forward takes one of three routes:

    - decode: HIP device, bf16 x, 1 <= M <= 16 rows after flattening the
      leading dims: the MFMA decode GEMM (fp8w_decode_gemm_bf16), which
      streams the codes once and converts them in registers;
    - dequant: any other x on a HIP device (prefill chunks, decode
      batches above 16): fp8w_dequant_bf16 writes W_eff into a bf16
      scratch buffer and F.linear runs on it. The scratch is shared by
      all Fp8Linears of a model and sized to the largest at quantise
      time, so the step stays graph-capturable; sharing it assumes that
      one stream at a time runs the model, which is how the scheduler
      runs it;
    - CPU: F.linear on dequantize_weight.
    """

    def __init__(self, codes, scale_exp, scratch=None):
        super().__init__()
        n, k = codes.shape
        if scale_exp.shape != (n,):
            raise ValueError("scale_exp must be [out_features]")
        self.in_features = k
        self.out_features = n
        self.register_buffer("codes", pack_codes(codes))
        self.register_buffer("scale_exp",
                             scale_exp.to(torch.int8).contiguous())
        self._scratch = scratch if scratch is not None else _Scratch()

    @classmethod
    def from_linear(cls, lin, scratch=None):
        if lin.bias is not None:
            raise ValueError("Fp8Linear has no bias")
        return cls(*quantize_weight(lin.weight.data), scratch=scratch)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, e4m3")

    def row_major_codes(self):
        return unpack_codes(self.codes, self.out_features, self.in_features)

    def effective_weight(self, dtype=torch.float32):
        """W_eff [N, K] (torch; any device)."""
        return dequantize_weight(self.row_major_codes(), self.scale_exp,
                                 dtype)

    def dequant_to_scratch(self):
        """W_eff as a [N, K] bf16 view of the shared scratch (HIP)."""
        from ..ops import hip_runtime as hr

        n, k = self.out_features, self.in_features
        buf = self._scratch.reserve(n * k, self.codes.device)
        hr.fp8w_dequant_bf16(self.codes.data_ptr(),
                             self.scale_exp.data_ptr(), buf.data_ptr(), n, k,
                             torch.cuda.current_stream().cuda_stream)
        return buf[:n * k].view(n, k)

    def forward(self, x):
        n, k = self.out_features, self.in_features
        if not x.is_cuda:
            return F.linear(x, self.effective_weight(x.dtype))
        m = x.numel() // k
        if x.dtype == torch.bfloat16 and 1 <= m <= MAX_DECODE_M:
            from ..ops import hip_runtime as hr

            x2 = x.reshape(m, k).contiguous()
            y = torch.empty(m, n, device=x.device, dtype=torch.bfloat16)
            try:
                hr.fp8w_decode_gemm_bf16(
                    x2.data_ptr(), self.codes.data_ptr(),
                    self.scale_exp.data_ptr(), y.data_ptr(), m, n, k,
                    torch.cuda.current_stream().cuda_stream)
                return y.view(*x.shape[:-1], n)
            except RuntimeError:
                # rejected before any launch (a misaligned view of x)
                pass
        w = self.dequant_to_scratch()
        if w.dtype != x.dtype:
            w = w.to(x.dtype)
        return F.linear(x, w)


def quantize_llama_weights(model):
    """Replaces wq, wk, wv, wo, w1, w3 and w2 of every block of a
    LlamaModel in place by Fp8Linear, releasing each bf16 tensor as it
    goes. tok, the norms and lm_head keep the model dtype (logits
    precision; lm_head is 6 % of the 8B model's bytes). On a HIP device
    the shared dequant scratch is allocated here, sized to the largest
    layer. Returns (bytes_before, bytes_after) of the replaced weights,
    the scratch included in bytes_after."""
    scratch = _Scratch()
    before = after = 0
    largest = 0
    device = None
    for block in model.blocks:
        for name in LLAMA_BLOCK_LINEARS:
            lin = getattr(block, name)
            if isinstance(lin, Fp8Linear):
                continue
            w = lin.weight
            device = w.device
            before += w.numel() * w.element_size()
            q = Fp8Linear.from_linear(lin, scratch=scratch)
            setattr(block, name, q)
            del lin, w
            after += q.codes.numel() + q.scale_exp.numel()
            largest = max(largest, q.in_features * q.out_features)
    if device is not None and device.type == "cuda":
        after += 2 * scratch.reserve(largest, device).numel()
    return before, after
