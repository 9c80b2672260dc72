"""KV-cache storage formats for the Llama decode path.

``kv_dtype`` is ``None`` / ``"bf16"`` (the cache has the model dtype —
the name is the server's default, the fp32 CPU model keeps fp32) or
``"fp8_e4m3"``: a ``torch.uint8`` tensor of the same
``[b, n_kv, max_seq + 1, head_dim]`` shape holding OCP e4m3fn codes,
unscaled. uint8 is the storage type because every indexing op works on
it; it is viewed as ``torch.float8_e4m3fn`` only to convert.

An fp8 cache always holds the e4m3 encoding of the value the plain cache
would hold at that place: K is rotated and rounded to the model dtype as
before and then encoded, so the torch prefill and the HIP decode scatter
(rope_scatter_decode_fp8kv_bf16) write identical bytes for identical
inputs.
"""

import torch

KV_DTYPES = ("bf16", "fp8_e4m3")
FP8_MAX = 448.0


def normalize_kv_dtype(kv_dtype):
    """None / "bf16" -> None (cache in the model dtype); "fp8_e4m3"
    stays; anything else raises."""
    if kv_dtype is None or kv_dtype == "bf16":
        return None
    if kv_dtype == "fp8_e4m3":
        return kv_dtype
    raise ValueError(
        f"unknown kv_dtype {kv_dtype!r}; expected one of {KV_DTYPES}")


def is_fp8_cache(t):
    return t.dtype == torch.uint8


def kv_encode_fp8(x):
    """float tensor -> uint8 e4m3fn codes by the CastF32ToFp8 contract
    (kernels.hip): round to nearest even, finite values saturate to
    +-448, NaN stays NaN and +-Inf gives a NaN code, as the hardware
    convert does. The clamp is what saturates: a plain
    ``.to(float8_e4m3fn)`` gives NaN above 464."""
    x = x.float()
    y = torch.where(x.isinf(), float("nan"), x.clamp(-FP8_MAX, FP8_MAX))
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def kv_decode_fp8(codes, dtype):
    """uint8 e4m3fn codes -> ``dtype``. Exact: every e4m3 value is a
    bf16 (and fp32) value."""
    return codes.view(torch.float8_e4m3fn).to(dtype)


def kv_store(x, like):
    """``x`` in the representation of the cache tensor ``like``."""
    if is_fp8_cache(like):
        return kv_encode_fp8(x)
    return x


def kv_load(window, dtype):
    """A materialised cache window as ``dtype`` values."""
    if is_fp8_cache(window):
        return kv_decode_fp8(window, dtype)
    return window
