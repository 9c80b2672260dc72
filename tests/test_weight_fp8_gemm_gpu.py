"""The wide fp8-weight GEMM (fp8w_gemm_bf16, M > 16) on an MI355X against
the float64 references of weight_fp8_refs.py, Fp8Linear's routes with
``fused_gemm`` and llama_tiny through it. Sentinel tails as in
test_weight_fp8_gpu.py."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr  # noqa: E402
import weight_fp8_refs as wr
from test_weight_fp8_gpu import (Y_FILL, _dev_u8, _dev_u16, _packed, _stream,
                                 _teacher_forced, _tiny_models,
                                 hr)  # noqa: F401
from client_amd.models.weight_fp8 import Fp8Linear
from client_amd.server.decode_scheduler import DecodeScheduler

pytestmark = pytest.mark.gpu


def _gemm(hr, x_bits, codes, se, tile=None):
    """Runs the wide GEMM; checks every sentinel and that the inputs are
    unchanged. Returns y bits [M, N]."""
    (m, k), n = x_bits.shape, codes.shape[0]
    assert tile is None or hr.fp8w_gemm_tile(m, n) == tile
    x, x_flat = _dev_u16(x_bits, 0x7FC1)
    pk, pk_flat = _dev_u8(_packed(codes), 0x7F)
    s, s_flat = _dev_u8(np.asarray(se, np.int8), 0x7F)
    y, y_flat = _dev_u16(np.full((m, n), Y_FILL, np.uint16), Y_FILL)
    hr.fp8w_gemm_bf16(x.data_ptr(), pk.data_ptr(), s.data_ptr(),
                      y.data_ptr(), m, n, k, _stream())
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[m * n:], y_flat[m * n:]), "wrote past y"
    assert np.array_equal(x.cpu().numpy().view(np.uint16), x_flat), "x changed"
    assert np.array_equal(pk.cpu().numpy(), pk_flat), "codes changed"
    assert np.array_equal(s.cpu().numpy(), s_flat), "scale_exp changed"
    return got[:m * n].reshape(m, n)


@pytest.mark.parametrize("k", wr.EXACT_K)
@pytest.mark.parametrize("n", wr.EXACT_N)
@pytest.mark.parametrize("m", [17, 64, 130])
def test_gemm_exact_integer_cases(hr, m, n, k):
    x_bits, codes, se, expected, _ = wr.exact_integer_case(m, n, k)
    assert np.array_equal(_gemm(hr, x_bits, codes, se), expected)


# (M, N, K, the tile edge BM = BN the host rule picks: the largest of 128
# and 64 whose grid has 192 workgroups, else 32, hence the wide N)
SHAPES = [
    (1, 1, 64, 32),        # M = 1, N = 1: the block's second code tile is
                           # beyond the padded N and is clamped; one chunk
    (31, 17, 128, 32),     # BM - 1; N = 17; prologue + tail, no steady loop
    (33, 100, 192, 32),    # BM + 1; N = 100: 8-byte stores, the last column
                           # block 4 wide; one steady iteration
    (17, 33, 64, 32),      # N one past BN; odd N: 2-byte stores
    (70, 49, 128, 32),     # three row blocks, the last ragged
    (24, 100, 4416, 32),   # 69 chunks: the steady loop with an odd tail
    (63, 12225, 64, 64),   # 64 tile, BM - 1, N one past a BN boundary
    (65, 6084, 64, 64),    # 64 tile, BM + 1, 8-byte stores
    (130, 4033, 128, 64),  # 64 tile, three row blocks, two chunks
    (127, 24452, 64, 128),   # 128 tile, BM - 1, 8-byte stores
    (129, 12161, 128, 128),  # 128 tile, BM + 1, N one past BN, two chunks
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_per_element_bound(hr, shape):
    m, n, k, tile = shape
    x_bits, codes, se = wr.random_case(m, n, k)
    got = _gemm(hr, x_bits, codes, se, tile)
    r, delta = wr.fp8w_gemm_ref(x_bits, codes, se)
    kr.assert_within_bf16_bound(got, r, delta, f"fp8w wide gemm {shape}")


def test_rows_independent_of_m_and_tile(hr):
    """One x row among NaN rows, at another index in an M that selects
    each tile variant: the same finite bits every time."""
    n, k = 8192, 128
    x_bits, codes, se = wr.random_case(1, n, k, seed=3)
    rows = []
    for m, at, tile in ((24, 5, 32), (129, 100, 64), (257, 256, 128)):
        poisoned = np.full((m, k), 0x7FC1, np.uint16)
        poisoned[1::2] = 0xFFC1
        poisoned[at] = x_bits[0]
        got = _gemm(hr, poisoned, codes, se, tile)
        assert np.array_equal(got, _gemm(hr, poisoned, codes, se))
        assert np.all(np.isnan(kr.bf16_bits_to_f64(np.delete(got, at, 0))))
        rows.append(got[at])
    assert np.all(np.isfinite(kr.bf16_bits_to_f64(rows[0])))
    assert np.array_equal(rows[0], rows[1])
    assert np.array_equal(rows[0], rows[2])


def test_gemm_argument_checks(hr):
    """Host-side rejections: nothing is launched, y keeps its fill."""
    x = torch.zeros(24 * 128 + 64, dtype=torch.bfloat16, device="cuda")
    pk = torch.zeros(32 * 128 + 64, dtype=torch.uint8, device="cuda")
    s = torch.zeros(64, dtype=torch.int8, device="cuda")
    y = torch.full((24 * 32 + 64,), 0x1234, dtype=torch.int16, device="cuda")

    def call(m=24, n=32, k=128, dx=0, dc=0):
        hr.fp8w_gemm_bf16(x.data_ptr() + dx, pk.data_ptr() + dc,
                          s.data_ptr(), y.data_ptr(), m, n, k, _stream())

    for bad in (dict(m=0), dict(n=0), dict(k=0), dict(k=96), dict(dx=2),
                dict(dc=2)):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()
    assert (y == 0x1234).all()
    call()  # and the plain call is accepted
    torch.cuda.synchronize()
    assert (y[:24 * 32] == 0).all() and (y[24 * 32:] == 0x1234).all()


def _count_calls(monkeypatch, hr):
    calls = {"gemm": 0, "decode_gemm": 0, "dequant": 0}
    mod = hr._load()
    for name in calls:
        def spy(*a, _name=name, _fn=getattr(mod, f"fp8w_{name}_bf16")):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(mod, f"fp8w_{name}_bf16", spy)
    return calls


def test_fp8_linear_routes_with_fused_gemm(hr, monkeypatch):
    n, k = 100, 576
    _, codes, se = wr.random_case(8, n, k, seed=11)
    lin = Fp8Linear(torch.from_numpy(codes), torch.from_numpy(se),
                    fused_gemm=True).cuda()
    calls = _count_calls(monkeypatch, hr)
    for shape, gemm, decode in (((24, k), 1, 0), ((2, 20, k), 2, 0),
                                ((8, k), 2, 1)):
        m = int(np.prod(shape[:-1]))
        x_bits, _, _ = wr.random_case(m, n, k, seed=12)
        x = torch.from_numpy(x_bits.view(np.int16)).view(torch.bfloat16)
        y = lin(x.cuda().view(shape))
        torch.cuda.synchronize()
        assert calls == {"gemm": gemm, "decode_gemm": decode, "dequant": 0}
        assert y.shape == (*shape[:-1], n) and y.dtype == torch.bfloat16
        got = y.view(torch.int16).cpu().numpy().view(np.uint16).reshape(m, n)
        r, delta = wr.fp8w_gemm_ref(x_bits, codes, se)
        kr.assert_within_bf16_bound(got, r, delta, f"Fp8Linear {shape}")


def _fused_tiny_models(seed):
    models = _tiny_models(seed)
    for mod in models[3].modules():
        if isinstance(mod, Fp8Linear):
            mod.fused_gemm = True
    return models


def test_llama_tiny_error_within_twice_the_plain_path(hr, monkeypatch):
    """max|B - T| <= 2 max|A - T| over the prefill-chunk logits (M = 72,
    the wide kernel), teacher-forced, as in test_weight_fp8_gpu.py.
    Measured on an MI355X: see docs/PERFORMANCE.md, "Wide GEMM"."""
    cfg, t_model, a_model, b_model = _fused_tiny_models(5)
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
    print(f"weight_fp8 wide llama_tiny prefill: max|A-T|={err_a:.6f} "
          f"max|B-T|={err_b:.6f}")
    assert 0 < err_a and err_b <= 2 * err_a


def test_scheduler_graph_matches_eager(hr):
    m = _fused_tiny_models(7)[3]
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
