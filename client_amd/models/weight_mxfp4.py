"""MXFP4 weight-only linear layers for the Llama decode path.

Format (OCP microscaling, fp4). A weight ``W[N, K]``, ``K % 32 == 0``, is
stored as

- ``codes``: 4-bit e2m1, sign in bit 3 and a magnitude index 0..7 into
  {0, 0.5, 1, 1.5, 2, 3, 4, 6}; in the logical row-major form uint8
  ``[N, K/2]``, the even k in the low nibble;
- ``scales``: uint8 e8m0 ``[N, K/32]`` of value ``2^(s - 127)``;

      W_eff[n, k] = e2m1(codes[n, k]) * 2^(scales[n, k // 32] - 127).

An e2m1 value has at most 2 significant bits, so every ``W_eff`` is
exactly a bf16 value, and the quantised model is, by definition, the bf16
model loaded with ``W_eff``; activations are never quantised (W4A16).

Layout. ``Mxfp4Linear`` holds both tensors pre-tiled for the kernels of
ops/csrc/weight_mxfp4.hip. Rows are padded to NP = 64 ceil(N/64) and K to
KP = 128 ceil(K/128) with zero codes and s = 127; kc = KP / 128:

    codes [((t * kc + c) * 64 + lane) * 16 + b]
        = bytes[16 t + (lane & 15)][64 c + 16 (lane >> 4) + b]
    scales[((T * kc + c) * 64 + lane) * 4 + i]
        = scales[64 T + 16 i + (lane & 15)][4 c + (lane >> 4)]

so a lane's 16-byte load is one 32-element block of one row, a wave's
load one contiguous 1 KiB run of 16 rows x 128 k, and the scales of the
four 16-row tiles of a 64-row group one dword per lane. ``pack`` /
``unpack`` are the only code that knows the permutation on the host.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from .weight_fp8 import (LLAMA_BLOCK_LINEARS, MAX_DECODE_M, Fp8Linear,
                         _Scratch, quantize_llama_weights)

WEIGHT_DTYPES = ("bf16", "fp8_e4m3", "mxfp4")

BLOCK = 32
ROW_GROUP = 64
TILE_ROWS = 16
TILE_K = 128
SCALE_BIAS = 127
SCALE_EXP_MIN = -100
SCALE_EXP_MAX = 100

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def normalize_weight_dtype(weight_dtype):
    """None / "bf16" -> None (weights stay in the model dtype);
    "fp8_e4m3" and "mxfp4" stay; anything else raises."""
    if weight_dtype is None or weight_dtype == "bf16":
        return None
    if weight_dtype in WEIGHT_DTYPES:
        return weight_dtype
    raise ValueError(f"unknown weight_dtype {weight_dtype!r}; expected one "
                     f"of {WEIGHT_DTYPES}")


def join_nibbles(codes4):
    """One code (0..15) per element [N, K] -> bytes [N, K/2], the even k
    in the low nibble."""
    c = codes4.to(torch.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous()


def split_nibbles(codes):
    """The inverse of join_nibbles."""
    n, half = codes.shape
    out = torch.empty(n, half, 2, dtype=torch.uint8, device=codes.device)
    out[:, :, 0] = codes & 0xF
    out[:, :, 1] = codes >> 4
    return out.view(n, 2 * half)


def quantize_weight(w):
    """``w`` [N, K] float -> (codes uint8 [N, K/2], scales uint8
    [N, K/32]). Per 32-element block e is the smallest exponent with
    amax <= 6 2^e, clamped to [-100, 100] (0 for an all-zero block),
    s = e + 127, and the codes are w / 2^e rounded to the nearest e2m1
    value, ties to the even code; saturation only in blocks whose
    exponent was clamped. A non-finite weight raises ValueError naming
    the row."""
    if w.dim() != 2:
        raise ValueError(f"expected a [N, K] weight, got {tuple(w.shape)}")
    n, k = w.shape
    if k % BLOCK != 0 or k == 0:
        raise ValueError(f"in_features {k} is not a multiple of {BLOCK}")
    w = w.detach().float()
    bad = ~torch.isfinite(w).all(dim=1)
    if bad.any():
        row = int(torch.nonzero(bad)[0])
        raise ValueError(f"non-finite weight in row {row}")
    blocks = w.view(n, k // BLOCK, BLOCK)
    amax = blocks.abs().amax(dim=2)
    # amax = m 2^ex with m in [0.5, 1), 6 = 0.75 2^3: the smallest e with
    # amax <= 6 2^e, in integers
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    e = e.clamp(SCALE_EXP_MIN, SCALE_EXP_MAX)
    # exact: a power-of-two scaling (what underflows is far below 0.25
    # and encodes as zero either way)
    a = torch.ldexp(blocks, -e[:, :, None]).abs()
    # the index is the number of midpoints passed; a tie goes to the even
    # index, so the midpoint above an even index needs > and the one
    # above an odd index >=
    idx = torch.zeros_like(a, dtype=torch.uint8)
    for j in range(7):
        mid = 0.5 * (E2M1_VALUES[j] + E2M1_VALUES[j + 1])
        idx += (a > mid) if j % 2 == 0 else (a >= mid)
    codes4 = idx | ((blocks < 0).to(torch.uint8) << 3)
    return (join_nibbles(codes4.view(n, k)),
            (e + SCALE_BIAS).to(torch.uint8))


def dequantize_weight(codes, scales, dtype):
    """Row-major ``codes`` [N, K/2] and ``scales`` [N, K/32] -> W_eff
    [N, K] as ``dtype`` (exact for bf16 and wider)."""
    c = split_nibbles(codes)
    n, k = c.shape
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES),
                         dtype=torch.float32, device=c.device)
    v = table[c.long()].view(n, k // BLOCK, BLOCK)
    e = scales.to(torch.int32) - SCALE_BIAS
    return torch.ldexp(v, e[:, :, None]).view(n, k).to(dtype)


def _padded(n, k):
    return (-(-n // ROW_GROUP) * ROW_GROUP, -(-k // TILE_K) * TILE_K)


def pack(codes, scales):
    """Row-major codes [N, K/2] and scales [N, K/32] -> the two flat
    tiled tensors (module docstring); the pad is zero codes, s = 127."""
    n, half = codes.shape
    k = 2 * half
    if k % BLOCK != 0 or k == 0:
        raise ValueError(f"in_features {k} is not a multiple of {BLOCK}")
    if scales.shape != (n, k // BLOCK):
        raise ValueError("scales must be [out_features, in_features / 32]")
    np_, kp = _padded(n, k)
    kc = kp // TILE_K
    full = codes.new_zeros((np_, kp // 2))
    full[:n, :half] = codes
    # [t, r, c, q, b] -> [t, c, q, r, b]; lane = 16 q + r
    pc = (full.view(np_ // TILE_ROWS, TILE_ROWS, kc, 4, 16)
          .permute(0, 2, 3, 1, 4).contiguous().view(-1))
    fs = scales.new_full((np_, 4 * kc), SCALE_BIAS)
    fs[:n, :k // BLOCK] = scales
    # [T, i, r, c, q] -> [T, c, q, r, i]
    ps = (fs.view(np_ // ROW_GROUP, 4, TILE_ROWS, kc, 4)
          .permute(0, 3, 4, 2, 1).contiguous().view(-1))
    return pc, ps


def unpack(packed_codes, packed_scales, n, k):
    """The inverse of pack: -> (codes [n, k/2], scales [n, k/32])."""
    np_, kp = _padded(n, k)
    kc = kp // TILE_K
    full = (packed_codes.view(np_ // TILE_ROWS, kc, 4, TILE_ROWS, 16)
            .permute(0, 3, 1, 2, 4).reshape(np_, kp // 2))
    fs = (packed_scales.view(np_ // ROW_GROUP, kc, 4, TILE_ROWS, 4)
          .permute(0, 4, 3, 1, 2).reshape(np_, 4 * kc))
    return (full[:n, :k // 2].contiguous(),
            fs[:n, :k // BLOCK].contiguous())


class Mxfp4Linear(nn.Module):
    """y = x @ W_eff^T, no bias. Buffers ``codes`` and ``scales``, both
    tiled (module docstring). forward takes the three routes of
    Fp8Linear: the MFMA decode GEMM (mxfp4w_decode_gemm_bf16) for bf16 x
    of 1..16 rows on a HIP device; mxfp4w_dequant_bf16 into the shared
    bf16 scratch plus F.linear for any other x on a HIP device; F.linear
    on effective_weight on the CPU.

    ``wide_gemm`` (default False) adds a fourth: bf16 x of more than 16
    rows on a HIP device runs the tiled MFMA GEMM (mxfp4w_gemm_bf16) on
    the same two buffers, which reads the codes straight into registers
    and stages x through LDS. With it set, no bf16 call with a contiguous,
    16-byte-aligned x touches the scratch."""

    def __init__(self, codes, scales, scratch=None, wide_gemm=False):
        super().__init__()
        self.wide_gemm = bool(wide_gemm)
        n, half = codes.shape
        self.in_features = 2 * half
        self.out_features = n
        # the kernels make the scale's float bits as s << 23, which is
        # 2^(s - 127) for 1 <= s <= 254 only (e8m0's 2^-127 and NaN are not
        # representable that way); the quantiser emits 27..227
        if scales.numel() and not (1 <= int(scales.min())
                                   and int(scales.max()) <= 254):
            raise ValueError("Mxfp4Linear scales must be in 1..254")
        pc, ps = pack(codes, scales.to(torch.uint8))
        self.register_buffer("codes", pc)
        self.register_buffer("scales", ps)
        self._scratch = scratch if scratch is not None else _Scratch()

    @classmethod
    def from_linear(cls, lin, scratch=None):
        if lin.bias is not None:
            raise ValueError("Mxfp4Linear has no bias")
        return cls(*quantize_weight(lin.weight.data), scratch=scratch)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, mxfp4")

    def weight_bytes(self):
        """The format's bytes: N K / 2 codes and N K / 32 scales. The
        tile padding (none on shapes that are multiples of 64 x 128) is
        not counted."""
        nk = self.in_features * self.out_features
        return nk // 2 + nk // BLOCK

    def row_major(self):
        return unpack(self.codes, self.scales, self.out_features,
                      self.in_features)

    def effective_weight(self, dtype=torch.float32):
        """W_eff [N, K] (torch; any device)."""
        return dequantize_weight(*self.row_major(), dtype)

    def dequant_to_scratch(self):
        """W_eff as a [N, K] bf16 view of the shared scratch (HIP)."""
        from ..ops import hip_runtime as hr

        n, k = self.out_features, self.in_features
        buf = self._scratch.reserve(n * k, self.codes.device)
        hr.mxfp4w_dequant_bf16(self.codes.data_ptr(), self.scales.data_ptr(),
                               buf.data_ptr(), n, k,
                               torch.cuda.current_stream().cuda_stream)
        return buf[:n * k].view(n, k)

    def forward(self, x):
        n, k = self.out_features, self.in_features
        if not x.is_cuda:
            return F.linear(x, self.effective_weight(x.dtype))
        m = x.numel() // k
        if x.dtype == torch.bfloat16 and (
                1 <= m <= MAX_DECODE_M or (self.wide_gemm and m >= 1)):
            x2 = x.reshape(m, k).contiguous()
            # the kernels' one requirement that a view of x can miss; any
            # error they raise beyond that is a real one and propagates
            if x2.data_ptr() % 16 == 0:
                from ..ops import hip_runtime as hr

                gemm = (hr.mxfp4w_decode_gemm_bf16 if m <= MAX_DECODE_M
                        else hr.mxfp4w_gemm_bf16)
                y = torch.empty(m, n, device=x.device, dtype=torch.bfloat16)
                gemm(x2.data_ptr(), self.codes.data_ptr(),
                     self.scales.data_ptr(), y.data_ptr(), m, n, k,
                     torch.cuda.current_stream().cuda_stream)
                return y.view(*x.shape[:-1], n)
        w = self.dequant_to_scratch()
        if w.dtype != x.dtype:
            w = w.to(x.dtype)
        return F.linear(x, w)


LAYER_CLASSES = {"fp8_e4m3": Fp8Linear, "mxfp4": Mxfp4Linear}


def quantize_llama_weights_as(model, weight_dtype, fused_gemm=False,
                              wide_gemm=False):
    """quantize_llama_weights with the layer class of ``weight_dtype``
    ("fp8_e4m3" or "mxfp4"). ``fused_gemm`` (the wide fp8 GEMM for
    M > 16) exists for "fp8_e4m3" only, ``wide_gemm`` (the wide MXFP4
    GEMM, Mxfp4Linear.wide_gemm on every created layer) for "mxfp4" only."""
    if fused_gemm and weight_dtype != "fp8_e4m3":
        raise ValueError(f"fused_gemm needs weight_dtype 'fp8_e4m3', not "
                         f"{weight_dtype!r}")
    if wide_gemm and weight_dtype != "mxfp4":
        raise ValueError(f"wide_gemm needs weight_dtype 'mxfp4', not "
                         f"{weight_dtype!r}")
    stats = quantize_llama_weights(model,
                                   layer_cls=LAYER_CLASSES[weight_dtype],
                                   fused_gemm=fused_gemm)
    if wide_gemm:
        for mod in model.modules():
            if isinstance(mod, Mxfp4Linear):
                mod.wide_gemm = True
    return stats


__all__ = ["WEIGHT_DTYPES", "LLAMA_BLOCK_LINEARS", "LAYER_CLASSES",
           "Mxfp4Linear", "normalize_weight_dtype", "quantize_weight",
           "dequantize_weight", "join_nibbles", "split_nibbles", "pack",
           "unpack", "quantize_llama_weights", "quantize_llama_weights_as"]
