"""BERT-large encoder (from scratch on torch.nn).

BASELINE.md config 4: BERT-large sequence/streaming gRPC with dynamic
batching and HIP-shm I/O. Standard architecture (hidden 1024, 24
layers, 16 heads), random-init weights, synthetic token inputs.

``forward(input_ids, attention_mask=None)``: attention_mask [b, s], bool
or any integer dtype, nonzero = a real token. Keys at masked positions
take no part in any softmax, so a row's result does not depend on what
it was padded with or to.

Two attention paths. The torch path (the default, and the only one on
the CPU) is ``nn.MultiheadAttention`` with ``key_padding_mask``. With
``fused_attention`` set (environment CLIENT_AMD_BERT_FUSED_ATTN=1, or the
server's --bert-fused-attention), bf16 tensors on a HIP device and a
supported head dim, each layer runs the packed in-projection as one
linear, the ``encoder_attention`` HIP kernel on its output in place, and
the out-projection. Hidden states at positions past a row's last real
token differ between the two paths (the kernel writes zeros there, torch
attends from them); they are don't-care on both, and nothing a real
position computes reads them.
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

FUSED_HEAD_DIMS = (16, 32, 64, 128)


def encoder_attention(qkv, key_mask, kv_len, heads):
    """qkv [b, s, 3 * heads * d] bf16 (the packed in-projection output),
    key_mask [b, s] uint8, kv_len [b] int32 -> [b, s, heads * d] bf16 on
    the MFMA kernel, scale d ** -0.5."""
    from ..ops import hip_runtime as hr

    b, s, width = qkv.shape
    d = width // (3 * heads)
    out = torch.empty(b, s, heads * d, device=qkv.device, dtype=qkv.dtype)
    hr.encoder_attention(
        qkv.data_ptr(), key_mask.data_ptr(), kv_len.data_ptr(),
        out.data_ptr(), b, s, heads, d, d ** -0.5,
        torch.cuda.current_stream().cuda_stream)
    return out


class BertLayer(nn.Module):
    def __init__(self, hidden, heads, ffn):
        super().__init__()
        self.attn = nn.MultiheadAttention(hidden, heads, batch_first=True)
        self.ln1 = nn.LayerNorm(hidden)
        self.fc1 = nn.Linear(hidden, ffn)
        self.fc2 = nn.Linear(ffn, hidden)
        self.ln2 = nn.LayerNorm(hidden)
        self.act = nn.GELU()

    def forward(self, x, key_padding_mask=None, fused=None):
        """key_padding_mask [b, s] bool, True = padding (torch path);
        fused = (key_mask uint8, kv_len int32) selects the HIP kernel."""
        if fused is not None:
            attn = self.attn
            qkv = F.linear(x, attn.in_proj_weight, attn.in_proj_bias)
            a = attn.out_proj(encoder_attention(
                qkv.contiguous(), fused[0], fused[1], attn.num_heads))
        elif key_padding_mask is not None:
            a, _ = self.attn(x, x, x, key_padding_mask=key_padding_mask,
                             need_weights=False)
        else:
            a, _ = self.attn(x, x, x, need_weights=False)
        x = self.ln1(x + a)
        x = self.ln2(x + self.fc2(self.act(self.fc1(x))))
        return x


class BertEncoder(nn.Module):
    """input_ids [b, s] int64 (, attention_mask [b, s]) -> pooled
    [b, hidden] (first token)."""

    def __init__(self, vocab_size=30522, hidden=1024, layers=24, heads=16,
                 ffn=4096, max_pos=512):
        super().__init__()
        self.tok = nn.Embedding(vocab_size, hidden)
        self.pos = nn.Embedding(max_pos, hidden)
        self.ln = nn.LayerNorm(hidden)
        self.layers = nn.ModuleList(
            [BertLayer(hidden, heads, ffn) for _ in range(layers)]
        )
        self.pooler = nn.Linear(hidden, hidden)
        self.head_dim = hidden // heads
        self.fused_attention = (
            os.environ.get("CLIENT_AMD_BERT_FUSED_ATTN") == "1")

    def _use_fused(self, x):
        return (self.fused_attention and x.is_cuda
                and x.dtype == torch.bfloat16
                and self.head_dim in FUSED_HEAD_DIMS)

    @staticmethod
    def _fused_mask(attention_mask, b, s, device):
        """(key_mask [b, s] uint8, kv_len [b] int32) on the device, with
        no host synchronisation."""
        if attention_mask is None:
            return (torch.ones(b, s, device=device, dtype=torch.uint8),
                    torch.full((b,), s, device=device, dtype=torch.int32))
        on = attention_mask != 0
        steps = torch.arange(1, s + 1, device=device, dtype=torch.int32)
        kv_len = (on.to(torch.int32) * steps).amax(dim=1)
        return on.to(torch.uint8).contiguous(), kv_len.contiguous()

    def hidden_states(self, input_ids, attention_mask=None):
        """The last layer's hidden states [b, s, hidden]."""
        b, s = input_ids.shape
        pos_ids = torch.arange(s, device=input_ids.device)
        x = self.ln(self.tok(input_ids) + self.pos(pos_ids)[None])
        if self._use_fused(x):
            fused = self._fused_mask(attention_mask, b, s, x.device)
            for layer in self.layers:
                x = layer(x, fused=fused)
        elif attention_mask is not None:
            pad = attention_mask == 0
            for layer in self.layers:
                x = layer(x, key_padding_mask=pad)
        else:
            for layer in self.layers:
                x = layer(x)
        return x

    def forward(self, input_ids, attention_mask=None):
        x = self.hidden_states(input_ids, attention_mask)
        return torch.tanh(self.pooler(x[:, 0]))


def bert_large():
    return BertEncoder()


def bert_tiny():
    """Small config for CPU tests."""
    return BertEncoder(vocab_size=128, hidden=32, layers=2, heads=2, ffn=64,
                       max_pos=64)
