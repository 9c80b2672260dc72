"""The wide MXFP4-weight GEMM (mxfp4w_gemm_bf16, M > 16) on an MI355X
against the float64 references of weight_mxfp4_refs.py, Mxfp4Linear's
routes with ``wide_gemm`` and llama_tiny through it. Sentinel tails as in
test_weight_mxfp4_gpu.py."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr  # noqa: E402
import weight_mxfp4_refs as mr
from test_weight_fp8_gpu import (Y_FILL, _dev_u8, _dev_u16, _stream,
                                 _teacher_forced, hr)  # noqa: F401
from test_weight_mxfp4_gpu import tiny_models  # noqa: F401
from client_amd.models.weight_mxfp4 import Mxfp4Linear, join_nibbles, pack
from client_amd.server.decode_scheduler import DecodeScheduler

pytestmark = pytest.mark.gpu

S, M, L = 64032, 128064, 256128  # the variants, 1000 BN + BM


def _gemm(hr, x_bits, codes, scales, tile=None):
    """Runs the wide GEMM; checks every sentinel and that the inputs are
    unchanged. Returns y bits [M, N]."""
    (m, k), n = x_bits.shape, codes.shape[0]
    assert tile is None or hr.mxfp4w_gemm_tile(m, n) == tile
    pc, ps = pack(join_nibbles(torch.from_numpy(codes)),
                  torch.from_numpy(scales))
    x, x_flat = _dev_u16(x_bits, 0x7FC1)
    c, c_flat = _dev_u8(pc.numpy(), 0xFF)
    s, s_flat = _dev_u8(ps.numpy(), 0xFF)
    y, y_flat = _dev_u16(np.full((m, n), Y_FILL, np.uint16), Y_FILL)
    hr.mxfp4w_gemm_bf16(x.data_ptr(), c.data_ptr(), s.data_ptr(),
                        y.data_ptr(), m, n, k, _stream())
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[m * n:], y_flat[m * n:]), "wrote past y"
    assert np.array_equal(x.cpu().numpy().view(np.uint16), x_flat), "x changed"
    assert np.array_equal(c.cpu().numpy(), c_flat), "codes changed"
    assert np.array_equal(s.cpu().numpy(), s_flat), "scales changed"
    return got[:m * n].reshape(m, n)


@pytest.mark.parametrize("k", [32, 160, 384])
@pytest.mark.parametrize("n", [16, 100])
@pytest.mark.parametrize("m", [17, 64, 130])
def test_gemm_exact_integer_cases(hr, m, n, k):
    x_bits, codes, scales, expected = mr.exact_case(m, n, k)
    assert np.array_equal(_gemm(hr, x_bits, codes, scales), expected)


# (M, N, K, variant). The host rule takes the largest variant with
# M > BM / 2 whose grid has 192 workgroups, else 64 x 32, hence the wide N.
# The steady loop runs three chunks per round from 5 chunks on and leaves
# 2, 3 or 4 to the tail.
SHAPES = [
    (1, 1, 32, S),         # M = 1, N = 1; three of the chunk's blocks masked
    (31, 17, 128, S),      # BM - 1; odd N: 2-byte stores; one chunk
    (33, 65, 160, S),      # BM + 1; N one past BN; a chunk and a ragged one
    (17, 100, 384, S),     # N % 4 == 0, pad rows; 3 chunks: one tail step
    (70, 20, 512, S),      # three row blocks; 4 chunks: two tail steps
    (17, 100, 640, S),     # 5 chunks: one round, tail of 2
    (24, 100, 768, S),     # 6 chunks: one round, tail of 3
    (20, 20, 896, S),      # 7 chunks: one round, tail of 4
    (24, 100, 4224, S),    # 33 chunks: ten rounds
    (63, 24577, 32, M),    # BM - 1, N one past a BN boundary
    (65, 12289, 128, M),   # BM + 1, N one past a BN boundary
    (65, 12292, 640, M),   # 8-byte stores; the steady loop of this variant
    (127, 49153, 64, L),   # BM - 1, N one past a BN boundary
    (129, 24577, 128, L),  # BM + 1
    (129, 24580, 640, L),  # 8-byte stores; the steady loop of this variant
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_per_element_bound(hr, shape):
    m, n, k, tile = shape
    x_bits, codes, scales = mr.random_case(m, n, k)
    got = _gemm(hr, x_bits, codes, scales, tile)
    kr.assert_within_bf16_bound(got, *mr.gemm_ref(x_bits, codes, scales),
                                f"mxfp4w wide gemm {shape}")


def test_rows_independent_of_m_and_variant(hr):
    """One x row among NaN rows, at another index in an M that selects
    each variant: the same finite bits every time. At K = 160 the second
    chunk's k >= K lies in the next row of x, which is NaN."""
    n, k = 24577, 160
    x_bits, codes, scales = mr.random_case(1, n, k, seed=3)
    rows = []
    for m, at, tile in ((24, 5, S), (63, 40, M), (130, 127, L)):
        poisoned = np.full((m, k), 0x7FC1, np.uint16)
        poisoned[1::2] = 0xFFC1
        poisoned[at] = x_bits[0]
        got = _gemm(hr, poisoned, codes, scales, tile)
        assert np.all(np.isnan(kr.bf16_bits_to_f64(np.delete(got, at, 0))))
        rows.append(got[at])
    assert np.all(np.isfinite(kr.bf16_bits_to_f64(rows[0])))
    assert np.array_equal(rows[0], rows[1])
    assert np.array_equal(rows[0], rows[2])


def test_gemm_argument_checks(hr):
    """Host-side rejections: nothing is launched, y keeps its fill."""
    x = torch.zeros(24 * 128 + 64, dtype=torch.bfloat16, device="cuda")
    pc = torch.zeros(64 * 64 + 64, dtype=torch.uint8, device="cuda")
    ps = torch.full((64 * 4 + 64,), 127, dtype=torch.uint8, device="cuda")
    y = torch.full((24 * 32 + 64,), 0x1234, dtype=torch.int16, device="cuda")

    def call(m=24, n=32, k=128, dx=0, dc=0, ds=0):
        hr.mxfp4w_gemm_bf16(x.data_ptr() + dx, pc.data_ptr() + dc,
                            ps.data_ptr() + ds, y.data_ptr(), m, n, k,
                            _stream())

    for bad in (dict(m=0), dict(n=0), dict(k=0), dict(m=-1), dict(k=48),
                dict(dx=2), dict(dc=2), dict(ds=2)):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (y == 0x1234).all()
    assert hr.mxfp4w_gemm_tile(0, 32) == 0 and hr.mxfp4w_gemm_tile(24, 0) == 0
    call()  # and the plain call is accepted
    torch.cuda.synchronize()
    assert (y[:24 * 32] == 0).all() and (y[24 * 32:] == 0x1234).all()


def _count_calls(monkeypatch, hr):
    calls = {"gemm": 0, "decode_gemm": 0, "dequant": 0}
    mod = hr._load()
    for name in calls:
        def spy(*a, _name=name, _fn=getattr(mod, f"mxfp4w_{name}_bf16")):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(mod, f"mxfp4w_{name}_bf16", spy)
    return calls


def test_mxfp4_linear_routes_with_wide_gemm(hr, monkeypatch):
    n, k = 100, 576
    _, codes, scales = mr.random_case(8, n, k, seed=11)
    lin = Mxfp4Linear(join_nibbles(torch.from_numpy(codes)),
                      torch.from_numpy(scales), wide_gemm=True).cuda()
    calls = _count_calls(monkeypatch, hr)
    for shape, gemm, decode in (((24, k), 1, 0), ((2, 20, k), 2, 0),
                                ((8, k), 2, 1)):
        m = int(np.prod(shape[:-1]))
        x_bits, _, _ = mr.random_case(m, n, k, seed=12)
        x = torch.from_numpy(x_bits.view(np.int16)).view(torch.bfloat16)
        y = lin(x.cuda().view(shape))
        torch.cuda.synchronize()
        assert calls == {"gemm": gemm, "decode_gemm": decode, "dequant": 0}
        assert y.shape == (*shape[:-1], n) and y.dtype == torch.bfloat16
        got = y.view(torch.int16).cpu().numpy().view(np.uint16).reshape(m, n)
        kr.assert_within_bf16_bound(got, *mr.gemm_ref(x_bits, codes, scales),
                                    f"Mxfp4Linear {shape}")
    assert lin._scratch.buf is None


def _wide(models):
    for mod in models[3].modules():
        if isinstance(mod, Mxfp4Linear):
            mod.wide_gemm = True
    return models


def test_llama_tiny_error_within_twice_the_plain_path(hr, tiny_models,
                                                      monkeypatch):
    """max|B - T| <= 2 max|A - T| over the prefill-chunk logits (M = 72,
    the wide kernel), teacher-forced, as in test_weight_mxfp4_gpu.py.
    Measured on an MI355X: see docs/PERFORMANCE.md, "Wide GEMM
    (`--mxfp4-weight-gemm`)"."""
    cfg, t_model, a_model, b_model = _wide(tiny_models(5))
    tokens = torch.randint(0, cfg.vocab_size, (3, 28),
                           generator=torch.Generator().manual_seed(1))
    calls = _count_calls(monkeypatch, hr)
    lb = _teacher_forced(b_model, tokens, "cuda:0", torch.bfloat16, 24, 4)
    assert calls == {"gemm": 7 * cfg.n_layers,
                     "decode_gemm": 4 * 7 * cfg.n_layers, "dequant": 0}
    la = _teacher_forced(a_model, tokens, "cuda:0", torch.bfloat16, 24, 4)
    lt = _teacher_forced(t_model, tokens, "cpu", torch.float32, 24, 4)
    assert torch.isfinite(lb).all()
    err_a = float((la[0] - lt[0]).abs().max())
    err_b = float((lb[0] - lt[0]).abs().max())
    print(f"weight_mxfp4 wide llama_tiny prefill: max|A-T|={err_a:.6f} "
          f"max|B-T|={err_b:.6f}")
    assert 0 < err_a and err_b <= 2 * err_a


def test_scheduler_graph_matches_eager(hr, tiny_models):
    m = _wide(tiny_models(7))[3]
    rng = np.random.default_rng(0)
    prompts = [rng.integers(1, 250, 3 + i % 7).astype(np.int64)
               for i in range(18)]
    got = {}
    for use_graph in (False, True):
        sched = DecodeScheduler(m, max_batch=20, device="cuda:0",
                                use_graph=use_graph, len_bucket=32)
        try:
            queues = [sched.submit(p, 6) for p in prompts]
            got[use_graph] = [list(iter(lambda q=q: q.get(timeout=120),
                                        sched.END)) for q in queues]
            assert not use_graph or (sched._graphs and all(
                g is not sched._EAGER for g in sched._graphs.values()))
        finally:
            sched.shutdown()
    assert got[True] == got[False]
    assert all(len(t) == 6 for t in got[True])
