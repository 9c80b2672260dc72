"""The BERT encoder attention on an MI355X: the MFMA kernel against the
float64 reference, its bit independence of batch and padding, and
bert_tiny through the fused and the torch path, eager and captured.

Kernel outputs are bf16 and are checked per element against a float64
reference built from the exact inputs: |got - r| <= ulp_bf16(r)/2 +
delta, with delta derived in tests/encoder_attention_refs.py from the
operation count, never from the kernel's output.
"""

import copy

import numpy as np
import pytest

import encoder_attention_refs as er
import kernel_refs as kr
from test_decode_edges_gpu import PAD, _bits, _stream, _to_dev
from test_encoder_attention import LENS, tiny_batch

pytestmark = pytest.mark.gpu

NAN_OUT = 0x7FC1


@pytest.fixture(scope="module")
def hr():
    from client_amd.ops import gpu_available, hip_runtime

    if not gpu_available():
        pytest.skip("no HIP device")
    return hip_runtime


def _tiles(hr):
    kt = int(hr.ENCODER_ATTN_KTILE)
    return (int(hr.ENCODER_ATTN_QTILE), kt,
            int(getattr(hr, "ENCODER_ATTN_KSTAGE", kt)))


def _attend(hr, qkv_bits, key_mask, kv_len, scale):
    """Runs the kernel into a NaN-filled buffer; checks the sentinels
    behind out and that qkv, key_mask and kv_len are unchanged. Returns
    output bits [B, S, heads, d]."""
    import torch

    b, s, _, heads, d = qkv_bits.shape
    qkv, _ = _to_dev(qkv_bits)
    mask_d = torch.from_numpy(np.ascontiguousarray(key_mask)).cuda()
    len_d = torch.from_numpy(np.ascontiguousarray(kv_len,
                                                  dtype=np.int32)).cuda()
    n = b * s * heads * d
    out, tail = _to_dev(np.full((b, s, heads, d), NAN_OUT, np.uint16), PAD,
                        d + b + s)
    hr.encoder_attention(qkv.data_ptr(), mask_d.data_ptr(), len_d.data_ptr(),
                         out.data_ptr(), b, s, heads, d, scale, _stream())
    torch.cuda.synchronize()
    ob = _bits(out)
    assert np.array_equal(ob[n:], tail), "wrote past the output"
    assert np.array_equal(_bits(qkv), qkv_bits.reshape(-1)), "qkv changed"
    assert np.array_equal(mask_d.cpu().numpy(), key_mask), "mask changed"
    assert np.array_equal(len_d.cpu().numpy(), kv_len), "kv_len changed"
    return ob[:n].reshape(b, s, heads, d)


@pytest.mark.parametrize("shape", er.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_reference(hr, shape):
    """Every kv_len in every row slot with every mask pattern at every S;
    NaN patterns in every position at or past kv_len and 64 times larger
    K entries at masked keys: a kernel that loads and masks yields NaN, one
    that misses a mask byte a wrong softmax."""
    qt, kt, ks = _tiles(hr)
    n_cases = 0
    for qkv, mask, kv_len, scale in er.cases(shape, qt, kt, ks):
        got = _attend(hr, qkv, mask, kv_len, scale)
        r, delta, real = er.encoder_attention_ref(qkv, mask, kv_len, scale)
        kr.assert_within_bf16_bound(
            got, r, delta, f"encoder attention {shape} S={qkv.shape[1]} "
                           f"kv_len={kv_len} scale={scale}")
        assert np.all(got[~real] == 0), "c >= kv_len is not exact zero"
        n_cases += 1
    assert n_cases == len(er.seq_lens_for(qt, kt, ks)) * 6 * 4


def test_row_bits_invariant(hr):
    """A row's output bits for c < kv_len are the same in a mixed launch,
    alone with B = 1, with S cut to kv_len, and in another row slot."""
    qt, kt, ks = _tiles(hr)
    shape = (3, 4, 64)
    s = max(er.seq_lens_for(qt, kt, ks))
    base = er.random_case(shape, s, seed=5)
    kv_len = np.array([s, kt + 1, s - 3], dtype=np.int32)
    mask = np.stack([er.mask_row("ones", s, s, kt),
                     er.mask_row("third", s, kt + 1, kt),
                     er.mask_row("tile", s, s - 3, kt)])
    qkv = er.poison(base, mask, kv_len)
    mixed = _attend(hr, qkv, mask, kv_len, 0.125)
    order = np.array([2, 0, 1])
    moved = _attend(hr, qkv[order], mask[order], kv_len[order], 0.125)
    for i in (1, 2):
        n = int(kv_len[i])
        alone = _attend(hr, qkv[i:i + 1], mask[i:i + 1], kv_len[i:i + 1],
                        0.125)
        cut = _attend(hr, np.ascontiguousarray(qkv[i:i + 1, :n]),
                      np.ascontiguousarray(mask[i:i + 1, :n]),
                      kv_len[i:i + 1], 0.125)
        slot = int(np.nonzero(order == i)[0][0])
        for name, other in (("alone", alone[0, :n]), ("cut", cut[0]),
                            ("moved", moved[slot, :n])):
            assert np.array_equal(mixed[i, :n], other), (i, name)


def test_softmax_edges(hr):
    qt, kt, ks = _tiles(hr)
    for name, qkv, mask, kv_len in er.softmax_edge_cases(kt):
        got = _attend(hr, qkv, mask, kv_len, 1.0)
        r, delta, _ = er.encoder_attention_ref(qkv, mask, kv_len, 1.0)
        kr.assert_within_bf16_bound(got, r, delta,
                                    f"encoder attention {name}")
        if name == "dominant":
            # one key takes all the weight: the output is its V row
            want = np.broadcast_to(qkv[:, kt:kt + 1, 2], got.shape)
            assert np.array_equal(got, want)


def test_query_without_visible_key_is_zero(hr):
    """Reachable only through a hand-made mask: kv_len says five keys,
    every mask byte is zero."""
    qkv = er.random_case((1, 2, 64), 5)
    mask = np.zeros((1, 5), dtype=np.uint8)
    got = _attend(hr, qkv, mask, np.array([5], dtype=np.int32), 1.0)
    assert not got.any()


def test_argument_checks(hr):
    import torch

    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.full((1 << 14,), 0x1234, dtype=torch.int16, device="cuda")
    lens = torch.full((4,), 4, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()

    def call(qkv=p, b=2, s=4, heads=2, d=16):
        hr.encoder_attention(qkv, p, lens.data_ptr(), out.data_ptr(), b, s,
                             heads, d, 1.0, _stream())

    for bad in (dict(d=24), dict(d=8), dict(d=256), dict(heads=0),
                dict(b=-1), dict(qkv=p + 2)):
        with pytest.raises(RuntimeError):
            call(**bad)
    call(b=0)  # returns without a launch
    torch.cuda.synchronize()
    assert (out == 0x1234).all()


# ---------------------------------------------------------------------------
# bert_tiny, bf16
# ---------------------------------------------------------------------------


def _tiny_pair(seed):
    """(fp32 CPU model holding bf16-rounded weights, the same model in
    bf16 on the GPU)."""
    import torch

    from client_amd.models.bert import bert_tiny

    torch.manual_seed(seed)
    ref = bert_tiny().eval().to(torch.bfloat16).float()
    gpu = copy.deepcopy(ref).to("cuda:0").to(torch.bfloat16).eval()
    return ref, gpu


def test_fused_model_matches_torch_path(hr):
    """Both paths against the fp32 CPU model with the same weights, over
    pooled and the hidden states of real positions: the fused path's
    error is at most twice the torch path's (two bf16 pipelines that
    differ in where they round) plus 2^-8, one bf16 ulp at 1.0, the range
    of the tanh-pooled output."""
    import torch

    ref, gpu = _tiny_pair(9)
    ids, mask = tiny_batch()
    with torch.inference_mode():
        want = (ref(ids, mask), ref.hidden_states(ids, mask))
        err = {}
        for fused in (False, True):
            gpu.fused_attention = fused
            pooled = gpu(ids.cuda(), mask.cuda()).float().cpu()
            hidden = gpu.hidden_states(ids.cuda(), mask.cuda()).float().cpu()
            assert torch.isfinite(pooled).all()
            e = (pooled - want[0]).abs().max().item()
            for i, n in enumerate(LENS):
                assert torch.isfinite(hidden[i, :n]).all()
                e = max(e, (hidden[i, :n] - want[1][i, :n]).abs().max().item())
            err[fused] = e
    print(f"bert_tiny bf16 vs fp32: err_torch={err[False]:.4e} "
          f"err_fused={err[True]:.4e}")
    assert err[True] <= 2 * err[False] + 2.0 ** -8, err


def test_fused_model_without_mask(hr):
    """No mask is an all-ones mask: the same bits."""
    import torch

    _, gpu = _tiny_pair(4)
    gpu.fused_attention = True
    ids, mask = tiny_batch()
    with torch.inference_mode():
        assert torch.equal(gpu(ids.cuda()),
                           gpu(ids.cuda(), torch.ones_like(mask).cuda()))


def test_fused_model_graph_capture_follows_the_mask(hr):
    """TorchModel captures the fused forward on the first call and
    replays it on the second with another mask of the same shape: each
    result is the eager forward's for its own mask, bit for bit (a mask
    baked into the graph, or a host sync in kv_len, would not be)."""
    import torch

    from client_amd.server.__main__ import build_core

    core = build_core(["bert_tiny"], device="cuda:0",
                      bert_fused_attention=True)
    model = core.models["bert_tiny"]
    assert model.module.fused_attention is True
    ids, mask_a = tiny_batch()
    mask_b = mask_a.clone()
    mask_b[0, 23:] = 0
    mask_b[1, :30] = 1
    mask_b[2, 0:3] = 1
    ids, mask_a, mask_b = ids.cuda(), mask_a.cuda(), mask_b.cuda()
    with torch.inference_mode():
        eager = {name: model.module(ids, m)
                 for name, m in (("a", mask_a), ("b", mask_b))}
        eager["none"] = model.module(ids)
    torch.cuda.synchronize()
    assert not torch.equal(eager["a"], eager["b"])
    got_a = model._execute_direct([ids, mask_a])[0]
    got_b = model._execute_direct([ids, mask_b])[0]
    got_none = model._execute_direct([ids])[0]
    torch.cuda.synchronize()
    assert len(model._graphs) == 2
    assert all(entry != "eager" for entry in model._graphs.values())
    assert torch.equal(got_a, eager["a"])
    assert torch.equal(got_b, eager["b"])
    assert torch.equal(got_none, eager["none"])
