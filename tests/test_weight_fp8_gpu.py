"""FP8 (e4m3) weight-only linears on an MI355X: the MFMA decode GEMM and
the dequant kernel against the float64 references of weight_fp8_refs.py,
Fp8Linear's routes, and llama_tiny quantised against the same model
carrying W_eff in plain bf16 linears.

Every device buffer is followed by a sentinel tail (NaN patterns behind
x, 0x7F codes behind the packed codes, 0x7FC1 behind y); after every
call the inputs are unchanged and the tails intact.
"""

import copy

import numpy as np
import pytest

import kernel_refs as kr
import weight_fp8_refs as wr

pytestmark = pytest.mark.gpu

PAD = 64
Y_FILL = 0x7FC1


@pytest.fixture(scope="module")
def hr():
    from client_amd.ops import gpu_available, hip_runtime

    if not gpu_available():
        pytest.skip("no HIP device")
    return hip_runtime


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _dev_u16(bits, tail_value):
    import torch

    flat = np.concatenate([np.ascontiguousarray(bits, np.uint16).reshape(-1),
                           np.full(PAD, tail_value, np.uint16)])
    return torch.from_numpy(flat.view(np.int16)).cuda(), flat


def _dev_u8(values, tail_value):
    import torch

    flat = np.concatenate([np.ascontiguousarray(values).reshape(-1)
                           .view(np.uint8),
                           np.full(PAD, tail_value, np.uint8)])
    return torch.from_numpy(flat).cuda(), flat


def _packed(codes):
    """The tiled layout, pad rows holding NaN codes."""
    import torch

    from client_amd.models.weight_fp8 import pack_codes

    return pack_codes(torch.from_numpy(np.ascontiguousarray(codes)),
                      pad=0x7F).numpy()


def _gemm(hr, x_bits, codes, se):
    """Runs the decode GEMM; checks every sentinel and that the inputs
    are unchanged. Returns y bits [M, N]."""
    import torch

    m, k = x_bits.shape
    n = codes.shape[0]
    x, x_flat = _dev_u16(x_bits, 0x7FC1)
    pk, pk_flat = _dev_u8(_packed(codes), 0x7F)
    s, s_flat = _dev_u8(np.asarray(se, np.int8), 0x7F)
    y, y_flat = _dev_u16(np.full((m, n), Y_FILL, np.uint16), Y_FILL)
    hr.fp8w_decode_gemm_bf16(x.data_ptr(), pk.data_ptr(), s.data_ptr(),
                             y.data_ptr(), m, n, k, _stream())
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[m * n:], y_flat[m * n:]), "wrote past y"
    assert np.array_equal(x.cpu().numpy().view(np.uint16), x_flat), "x changed"
    assert np.array_equal(pk.cpu().numpy(), pk_flat), "codes changed"
    assert np.array_equal(s.cpu().numpy(), s_flat), "scale_exp changed"
    return got[:m * n].reshape(m, n)


# ---------------------------------------------------------------------------
# decode GEMM
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("k", wr.EXACT_K)
@pytest.mark.parametrize("n", wr.EXACT_N)
@pytest.mark.parametrize("m", wr.EXACT_M)
def test_gemm_exact_integer_cases(hr, m, n, k):
    x_bits, codes, se, expected, _ = wr.exact_integer_case(m, n, k)
    got = _gemm(hr, x_bits, codes, se)
    assert np.array_equal(got, expected), (
        f"M={m} N={n} K={k}: {int((got != expected).sum())} of "
        f"{got.size} outputs differ")


@pytest.mark.parametrize("shape", wr.RANDOM_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_per_element_bound(hr, shape):
    x_bits, codes, se = wr.random_case(*shape)
    got = _gemm(hr, x_bits, codes, se)
    r, delta = wr.fp8w_gemm_ref(x_bits, codes, se)
    kr.assert_within_bf16_bound(got, r, delta, f"fp8w gemm {shape}")


def test_gemm_rows_independent(hr):
    """A row's output bits depend neither on M nor on the other rows."""
    x_bits, codes, se = wr.random_case(16, 100, 576, seed=3)
    full = _gemm(hr, x_bits, codes, se)
    again = _gemm(hr, x_bits, codes, se)
    assert np.array_equal(full, again), "two identical calls differ"
    alone = _gemm(hr, x_bits[5:6], codes, se)
    poisoned = np.full_like(x_bits, 0x7FC1)
    poisoned[1::2] = 0xFFC1
    poisoned[5] = x_bits[5]
    among_nan = _gemm(hr, poisoned, codes, se)
    assert np.array_equal(alone[0], full[5])
    assert np.array_equal(among_nan[5], full[5])
    assert np.all(np.isfinite(kr.bf16_bits_to_f64(full[5])))
    others = np.delete(kr.bf16_bits_to_f64(among_nan), 5, axis=0)
    assert np.all(np.isnan(others))


def test_gemm_argument_checks(hr):
    """Host-side rejections: nothing is launched, y keeps its fill."""
    import torch

    x = torch.zeros(17 * 128 + 64, dtype=torch.bfloat16, device="cuda")
    pk = torch.zeros(32 * 128 + 64, dtype=torch.uint8, device="cuda")
    s = torch.zeros(64, dtype=torch.int8, device="cuda")
    y = torch.full((17 * 32 + 64,), 0x1234, dtype=torch.int16, device="cuda")

    def call(m=8, n=32, k=128, dx=0, dc=0):
        hr.fp8w_decode_gemm_bf16(x.data_ptr() + dx, pk.data_ptr() + dc,
                                 s.data_ptr(), y.data_ptr(), m, n, k,
                                 _stream())

    for bad in (dict(m=0), dict(m=17), dict(k=96), dict(k=0), dict(n=0),
                dict(dx=2), dict(dc=2)):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (y == 0x1234).all()
    call()  # and the plain call is accepted
    torch.cuda.synchronize()
    assert (y[:8 * 32] == 0).all() and (y[8 * 32:] == 0x1234).all()


# ---------------------------------------------------------------------------
# dequant kernel
# ---------------------------------------------------------------------------


def _dequant(hr, codes, se):
    import torch

    n, k = codes.shape
    pk, pk_flat = _dev_u8(_packed(codes), 0x7F)
    s, s_flat = _dev_u8(np.asarray(se, np.int8), 0x7F)
    w, w_flat = _dev_u16(np.full((n, k), Y_FILL, np.uint16), Y_FILL)
    hr.fp8w_dequant_bf16(pk.data_ptr(), s.data_ptr(), w.data_ptr(), n, k,
                         _stream())
    torch.cuda.synchronize()
    got = w.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[n * k:], w_flat[n * k:]), "wrote past w_out"
    assert np.array_equal(pk.cpu().numpy(), pk_flat), "codes changed"
    assert np.array_equal(s.cpu().numpy(), s_flat), "scale_exp changed"
    return got[:n * k].reshape(n, k)


def _weff_bits(codes, se):
    w = wr.w_eff(codes, se)
    bits = kr.bf16_wire_encode(w.astype(np.float32)).reshape(w.shape)
    assert np.array_equal(kr.bf16_bits_to_f64(bits), w)  # exactly bf16
    return bits


@pytest.mark.parametrize("k", [64, 576])
@pytest.mark.parametrize("n", [1, 17, 64])
def test_dequant_bits(hr, n, k):
    rng = np.random.default_rng(n * 1000 + k)
    codes = wr.random_codes(rng, n, k)
    se = rng.integers(-8, 5, n).astype(np.int8)
    assert np.array_equal(_dequant(hr, codes, se), _weff_bits(codes, se))


def test_dequant_every_finite_code(hr):
    finite = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    assert finite.size == 254
    row = np.concatenate([finite, finite[:2]])  # K = 256
    codes = np.stack([row, row[::-1], np.roll(row, 37)])
    se = np.array([-100, 0, 100], np.int8)
    assert np.array_equal(_dequant(hr, codes, se), _weff_bits(codes, se))
    with pytest.raises(RuntimeError):
        hr.fp8w_dequant_bf16(0, 0, 0, 4, 96, _stream())


# ---------------------------------------------------------------------------
# Fp8Linear
# ---------------------------------------------------------------------------


def _count_calls(monkeypatch, hr):
    calls = {"gemm": 0, "dequant": 0}
    mod = hr._load()
    gemm, dequant = mod.fp8w_decode_gemm_bf16, mod.fp8w_dequant_bf16

    def gemm_spy(*a, **kw):
        calls["gemm"] += 1
        return gemm(*a, **kw)

    def dequant_spy(*a, **kw):
        calls["dequant"] += 1
        return dequant(*a, **kw)

    monkeypatch.setattr(mod, "fp8w_decode_gemm_bf16", gemm_spy)
    monkeypatch.setattr(mod, "fp8w_dequant_bf16", dequant_spy)
    return calls


def test_fp8_linear_routes(hr, monkeypatch):
    import torch

    from client_amd.models.weight_fp8 import Fp8Linear

    n, k = 100, 576
    x_bits, codes, se = wr.random_case(8, n, k, seed=11)
    lin = Fp8Linear(torch.from_numpy(codes), torch.from_numpy(se)).cuda()
    calls = _count_calls(monkeypatch, hr)

    x = torch.from_numpy(x_bits.view(np.int16)).view(torch.bfloat16).cuda()
    y = lin(x.view(2, 4, k))
    torch.cuda.synchronize()
    assert calls == {"gemm": 1, "dequant": 0}
    assert y.shape == (2, 4, n) and y.dtype == torch.bfloat16
    got = y.view(torch.int16).cpu().numpy().view(np.uint16).reshape(8, n)
    r, delta = wr.fp8w_gemm_ref(x_bits, codes, se)
    kr.assert_within_bf16_bound(got, r, delta, "Fp8Linear M=8")

    x24_bits, _, _ = wr.random_case(24, n, k, seed=12)
    x24 = torch.from_numpy(x24_bits.view(np.int16)).view(torch.bfloat16).cuda()
    y24 = lin(x24)
    torch.cuda.synchronize()
    assert calls == {"gemm": 1, "dequant": 1}
    scratch = lin._scratch.buf[:n * k].view(torch.int16).cpu().numpy()
    assert np.array_equal(scratch.view(np.uint16).reshape(n, k),
                          _weff_bits(codes, se))
    got24 = y24.view(torch.int16).cpu().numpy().view(np.uint16)
    r, delta = wr.fp8w_gemm_ref(x24_bits, codes, se)
    kr.assert_within_bf16_bound(got24.reshape(24, n), r, delta,
                                "Fp8Linear M=24")


# ---------------------------------------------------------------------------
# llama_tiny, bf16
# ---------------------------------------------------------------------------


def _tiny_models(seed):
    """T: fp32 CPU model with W_eff weights; A: GPU bf16 model with W_eff
    in plain nn.Linears (the existing path); B: the quantised GPU
    model."""
    import torch

    from client_amd.models.llama import LlamaModel, llama_tiny_config
    from client_amd.models.weight_fp8 import (LLAMA_BLOCK_LINEARS,
                                              quantize_llama_weights)

    torch.manual_seed(seed)
    cfg = llama_tiny_config()
    base = LlamaModel(cfg).to(torch.bfloat16).eval()
    b_model = copy.deepcopy(base).to("cuda:0")
    quantize_llama_weights(b_model)
    a_model = copy.deepcopy(base).to("cuda:0")
    t_model = copy.deepcopy(base).float()
    for bb, ba, bt in zip(b_model.blocks, a_model.blocks, t_model.blocks):
        for name in LLAMA_BLOCK_LINEARS:
            w = getattr(bb, name).effective_weight(torch.float32)
            getattr(ba, name).weight.data = w.to(torch.bfloat16)
            getattr(bt, name).weight.data = w.cpu()
            assert torch.equal(getattr(ba, name).weight.data.float(), w)
    return cfg, t_model, a_model, b_model


def _teacher_forced(model, tokens, device, dtype, prefill, steps):
    import torch

    b = tokens.shape[0]
    kv = model.make_kv_cache(b, device, dtype)
    toks = tokens.to(device)
    out = []
    with torch.inference_mode():
        out.append(model.forward_prefill_chunk(
            toks[:, :prefill], torch.zeros(b, dtype=torch.int64,
                                           device=device),
            torch.full((b,), prefill, dtype=torch.int64, device=device),
            torch.full((b,), prefill - 1, dtype=torch.int64, device=device),
            kv, 32))
        for i in range(steps):
            pos = torch.full((b,), prefill + i, dtype=torch.int64,
                             device=device)
            out.append(model.forward_decode_batch(
                toks[:, prefill + i:prefill + i + 1], pos, kv, max_len=64))
    return torch.stack([o.float().cpu() for o in out])


def test_llama_tiny_quantised_error_within_twice_the_plain_path(hr,
                                                                monkeypatch):
    """max|B - T| <= 2 max|A - T| over the prefill-chunk logits (dequant
    route) and 20 decode steps (kernel route), teacher-forced. A and B
    round activations to bf16 at the same places and differ only in
    summation order. Measured on an MI355X: see docs/PERFORMANCE.md,
    "FP8 weights"."""
    import torch

    cfg, t_model, a_model, b_model = _tiny_models(5)
    prefill, steps = 24, 20
    tokens = torch.randint(0, cfg.vocab_size, (3, prefill + steps),
                           generator=torch.Generator().manual_seed(1))
    calls = _count_calls(monkeypatch, hr)
    lb = _teacher_forced(b_model, tokens, "cuda:0", torch.bfloat16, prefill,
                         steps)
    per_forward = 7 * cfg.n_layers
    assert calls == {"gemm": steps * per_forward, "dequant": per_forward}
    la = _teacher_forced(a_model, tokens, "cuda:0", torch.bfloat16, prefill,
                         steps)
    assert calls == {"gemm": steps * per_forward, "dequant": per_forward}
    lt = _teacher_forced(t_model, tokens, "cpu", torch.float32, prefill,
                         steps)
    assert torch.isfinite(lb).all()
    for name, sl in (("prefill", slice(0, 1)), ("decode", slice(1, None)),
                     ("all", slice(None))):
        err_a = float((la[sl] - lt[sl]).abs().max())
        err_b = float((lb[sl] - lt[sl]).abs().max())
        print(f"weight_fp8 llama_tiny {name}: max|A-T|={err_a:.6f} "
              f"max|B-T|={err_b:.6f}")
        assert err_a > 0
        assert err_b <= 2 * err_a, (name, err_b, err_a)


def _run(sched, prompt, n):
    q = sched.submit(prompt, n)
    toks = []
    while True:
        t = q.get(timeout=120)
        if t is sched.END:
            return toks
        toks.append(t)


def test_quantised_scheduler_graph_matches_eager(hr):
    from client_amd.models.weight_fp8 import Fp8Linear
    from client_amd.server.decode_scheduler import DecodeScheduler

    _, _, _, m = _tiny_models(7)
    assert isinstance(m.blocks[0].wq, Fp8Linear)
    prompts = [np.array([5, 17, 200, 31, 8, 99], dtype=np.int64),
               np.arange(3, 40, dtype=np.int64),
               np.array([9, 9, 1], dtype=np.int64)]
    got = {}
    for use_graph in (False, True):
        sched = DecodeScheduler(m, max_batch=2, device="cuda:0",
                                use_graph=use_graph, len_bucket=32)
        try:
            got[use_graph] = [_run(sched, p, 8) for p in prompts]
            if use_graph:
                assert sched._graphs and all(
                    g is not sched._EAGER for g in sched._graphs.values())
        finally:
            sched.shutdown()
    assert got[True] == got[False]
    assert all(len(t) == 8 for t in got[True])
