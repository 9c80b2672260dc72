"""MXFP4 weight-only linears on an MI355X against the float64 references of
weight_mxfp4_refs.py. Every device buffer is followed by a sentinel tail;
after every call the inputs are unchanged and the tails intact."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr  # noqa: E402
import weight_mxfp4_refs as mr
from test_weight_fp8_gpu import (Y_FILL, _dev_u8, _dev_u16, _run, _stream,
                                 _teacher_forced, _tiny_models,
                                 hr)  # noqa: F401
from client_amd.models import weight_fp8
from client_amd.models.weight_mxfp4 import Mxfp4Linear, join_nibbles, pack
from client_amd.server.decode_scheduler import DecodeScheduler

pytestmark = pytest.mark.gpu


def _call(hr, x_bits, codes, scales):
    """Runs the decode GEMM, or the dequant where x_bits is None; checks
    the sentinels and that the inputs are unchanged. Returns output bits."""
    n, k = codes.shape
    pc, ps = pack(join_nibbles(torch.from_numpy(codes)),
                  torch.from_numpy(scales))
    c, c_flat = _dev_u8(pc.numpy(), 0xFF)
    s, s_flat = _dev_u8(ps.numpy(), 0xFF)
    shape = (n, k) if x_bits is None else (x_bits.shape[0], n)
    y, y_flat = _dev_u16(np.full(shape, Y_FILL, np.uint16), Y_FILL)
    if x_bits is None:
        hr.mxfp4w_dequant_bf16(c.data_ptr(), s.data_ptr(), y.data_ptr(), n, k,
                               _stream())
    else:
        x, x_flat = _dev_u16(x_bits, 0x7FC1)
        hr.mxfp4w_decode_gemm_bf16(x.data_ptr(), c.data_ptr(), s.data_ptr(),
                                   y.data_ptr(), shape[0], n, k, _stream())
        assert np.array_equal(x.cpu().numpy().view(np.uint16), x_flat)
    got = y.cpu().numpy().view(np.uint16)
    size = shape[0] * shape[1]
    assert np.array_equal(got[size:], y_flat[size:]), "wrote past the output"
    assert np.array_equal(c.cpu().numpy(), c_flat), "codes changed"
    assert np.array_equal(s.cpu().numpy(), s_flat), "scales changed"
    return got[:size].reshape(shape)


@pytest.mark.parametrize("k", [32, 128, 160])
@pytest.mark.parametrize("n", [16, 48])
@pytest.mark.parametrize("m", [1, 8, 16])
def test_gemm_exact_integer_cases(hr, m, n, k):
    x_bits, codes, scales, expected = mr.exact_case(m, n, k)
    assert np.array_equal(_call(hr, x_bits, codes, scales), expected)


# The issue's shapes run the 2-tile workgroups with 4 waves (K < 2048) and
# with 16 (K = 4096, a pipelined pair of chunks per wave). Then:
# (16, 17, 4736), 37 chunks on 16 waves: a pair, on five waves plus a third
# chunk; (5, 20, 1920), 15 chunks on 4 waves, and (4, 20, 8320), 65 on 16:
# one round of the steady loop, then two or three chunks; (2, 20, 14336),
# w2's K, 7 chunks per wave: two rounds; (3, 12300, 256) the 4-tile
# workgroups (N > 12224) with 4 waves; (2, 12290, 2144) the same with 16
# waves, one or two chunks each, the last chunk cut by the K tail.
@pytest.mark.parametrize("shape", [
    (1, 1, 32), (7, 15, 96), (9, 17, 1024), (16, 33, 160), (8, 100, 4096),
    (16, 17, 4736), (5, 20, 1920), (4, 20, 8320), (2, 20, 14336),
    (3, 12300, 256), (2, 12290, 2144),
], ids=lambda s: "x".join(map(str, s)))
def test_gemm_per_element_bound(hr, shape):
    x_bits, codes, scales = mr.random_case(*shape)
    got = _call(hr, x_bits, codes, scales)
    kr.assert_within_bf16_bound(got, *mr.gemm_ref(x_bits, codes, scales),
                                f"mxfp4w gemm {shape}")


def test_gemm_rows_independent(hr):
    """At K = 96 the chunk's last block is pad, whose x is never used."""
    x_bits, codes, scales = mr.random_case(16, 100, 96, seed=3)
    full = _call(hr, x_bits, codes, scales)
    assert np.array_equal(full, _call(hr, x_bits, codes, scales))
    alone = _call(hr, x_bits[5:6], codes, scales)
    poisoned = np.full_like(x_bits, 0x7FC1)
    poisoned[1::2] = 0xFFC1
    poisoned[5] = x_bits[5]
    among_nan = _call(hr, poisoned, codes, scales)
    assert np.array_equal(alone[0], full[5])
    assert np.array_equal(among_nan[5], full[5])
    assert np.all(np.isfinite(kr.bf16_bits_to_f64(full[5])))
    others = np.delete(kr.bf16_bits_to_f64(among_nan), 5, axis=0)
    assert np.all(np.isnan(others))


@pytest.mark.parametrize("n,k", [(1, 32), (17, 160), (64, 256)])
def test_dequant_bits(hr, n, k):
    """All 16 codes under s = 27, 127 and 227."""
    codes = ((np.arange(k)[None, :] + 5 * np.arange(n)[:, None]) % 16
             ).astype(np.uint8)
    scales = np.array([27, 127, 227], np.uint8)[
        (np.arange(n)[:, None] + np.arange(k // 32)[None, :]) % 3]
    assert np.array_equal(_call(hr, None, codes, scales),
                          mr.w_eff_bits(codes, scales))


def test_argument_checks(hr):
    """Host-side rejections: nothing is launched, y keeps its fill."""
    x = torch.zeros(17 * 128 + 64, dtype=torch.bfloat16, device="cuda")
    pc = torch.zeros(64 * 64 + 64, dtype=torch.uint8, device="cuda")
    ps = torch.full((64 * 4 + 64,), 127, dtype=torch.uint8, device="cuda")
    y = torch.full((32 * 128 + 64,), 0x1234, dtype=torch.int16, device="cuda")

    def gemm(m=8, n=32, k=128, dx=0, dc=0):
        hr.mxfp4w_decode_gemm_bf16(x.data_ptr() + dx, pc.data_ptr() + dc,
                                   ps.data_ptr(), y.data_ptr(), m, n, k,
                                   _stream())

    def dequant(n=32, k=128, dx=0, dc=0):  # dx misaligns w_out here
        hr.mxfp4w_dequant_bf16(pc.data_ptr() + dc, ps.data_ptr(),
                               y.data_ptr() + dx, n, k, _stream())

    for fn, bads in ((gemm, (dict(m=0), dict(m=17))), (dequant, ())):
        for bad in bads + (dict(k=0), dict(k=48), dict(n=0), dict(dx=2),
                           dict(dc=2)):
            with pytest.raises(RuntimeError):
                fn(**bad)
    torch.cuda.synchronize()
    assert (y == 0x1234).all()
    gemm()  # and the plain call is accepted
    torch.cuda.synchronize()
    assert (y[:8 * 32] == 0).all() and (y[8 * 32:] == 0x1234).all()


def test_mxfp4_linear_routes(hr):
    """M = 8 runs the kernel (no scratch is allocated), M = 24 the dequant."""
    n, k = 100, 160
    _, codes, scales = mr.random_case(8, n, k, seed=11)
    lin = Mxfp4Linear(join_nibbles(torch.from_numpy(codes)),
                      torch.from_numpy(scales)).cuda()
    for m in (8, 24):
        x_bits, _, _ = mr.random_case(m, n, k, seed=12)
        x = torch.from_numpy(x_bits.view(np.int16)).view(torch.bfloat16).cuda()
        y = lin(x.view(m // 4, 4, k))
        assert y.shape == (m // 4, 4, n) and y.dtype == torch.bfloat16
        got = y.view(torch.int16).cpu().numpy().view(np.uint16).reshape(m, n)
        kr.assert_within_bf16_bound(got, *mr.gemm_ref(x_bits, codes, scales),
                                    f"Mxfp4Linear M={m}")
        assert (lin._scratch.buf is None) == (m == 8)
    scratch = lin._scratch.buf[:n * k].view(torch.int16).cpu().numpy()
    assert np.array_equal(scratch.view(np.uint16).reshape(n, k),
                          mr.w_eff_bits(codes, scales))


@pytest.fixture
def tiny_models(monkeypatch):
    """The fp8 file's (cfg, T, A, B) builder with Mxfp4Linear as B's layer."""
    monkeypatch.setattr(weight_fp8, "quantize_llama_weights",
                        functools.partial(weight_fp8.quantize_llama_weights,
                                          layer_cls=Mxfp4Linear))
    return _tiny_models


def test_llama_tiny_quantised_error_within_twice_the_plain_path(hr,
                                                                tiny_models):
    """max|B - T| <= 2 max|A - T| over a 24-token prefill chunk and 20 decode
    steps: A and B differ only in summation order (docs/PERFORMANCE.md)."""
    cfg, t_model, a_model, b_model = tiny_models(5)
    assert isinstance(b_model.blocks[0].wq, Mxfp4Linear)
    tokens = torch.randint(0, cfg.vocab_size, (3, 44),
                           generator=torch.Generator().manual_seed(1))
    lb, la = (_teacher_forced(mod, tokens, "cuda:0", torch.bfloat16, 24, 20)
              for mod in (b_model, a_model))
    lt = _teacher_forced(t_model, tokens, "cpu", torch.float32, 24, 20)
    assert torch.isfinite(lb).all()
    err_a = float((la - lt).abs().max())
    err_b = float((lb - lt).abs().max())
    print(f"weight_mxfp4 llama_tiny: max|A-T|={err_a:.6f} "
          f"max|B-T|={err_b:.6f}")
    assert 0 < err_a and err_b <= 2 * err_a, (err_b, err_a)


def test_quantised_scheduler_graph_matches_eager(hr, tiny_models):
    m = tiny_models(7)[3]
    prompts = [np.array([5, 17, 200, 31, 8, 99], dtype=np.int64),
               np.arange(3, 40, dtype=np.int64)]
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
    assert got[True] == got[False] and all(len(t) == 8 for t in got[True])
