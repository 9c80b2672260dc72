"""FP8 (e4m3) weight-only linears on the CPU: the quantiser and storage
format, the tiled layout, llama_tiny quantised against the same model
carrying W_eff in plain nn.Linear weights (bitwise), server plumbing, and
the self-checks of the references the GPU tests use."""

import copy

import numpy as np
import pytest

import kernel_refs as kr
import weight_fp8_refs as wr

torch = pytest.importorskip("torch")

FP8 = "fp8_e4m3"


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------


def _quantiser_rows():
    """fp32 [rows, 64] with the rows the quantiser can get wrong, and
    (zero_row, clamped_rows)."""
    rng = np.random.default_rng(0)
    k = 64
    rows = []
    for j in (-20, -1, 0, 3, 40):
        base = rng.uniform(-1, 1, k).astype(np.float32) * np.float32(100.0)
        # amax exactly 448 2^j
        r = np.ldexp(base, j).astype(np.float32)
        r[5] = np.ldexp(np.float32(-448.0), j)
        rows.append(r)
        # amax one fp32 ulp above 448 2^j
        r = r.copy()
        r[5] = np.nextafter(np.ldexp(np.float32(448.0), j),
                            np.float32(np.inf))
        rows.append(r)
    rows.append(rng.standard_normal(k).astype(np.float32))
    zero_row = len(rows)
    rows.append(np.zeros(k, dtype=np.float32))
    # fp32 subnormals: the exponent clamps at -100
    clamped = [len(rows)]
    rows.append(rng.integers(1, 0x7FFFFF, k).astype(np.uint32)
                .view(np.float32) * np.where(rng.random(k) < 0.5, -1, 1)
                .astype(np.float32))
    # one huge outlier among ordinary values
    r = rng.standard_normal(k).astype(np.float32)
    r[17] = np.float32(3.0e5)
    rows.append(r)
    # beyond 448 2^100: the exponent clamps at +100 and the row saturates
    clamped.append(len(rows))
    r = rng.standard_normal(k).astype(np.float32)
    r[3] = np.float32(-3.0e38)
    rows.append(r)
    return np.stack(rows), zero_row, clamped


def test_quantize_weight_matches_cast_contract():
    from client_amd.models.weight_fp8 import quantize_weight

    w, zero_row, clamped = _quantiser_rows()
    codes, se = quantize_weight(torch.from_numpy(w))
    assert codes.dtype == torch.uint8 and codes.shape == w.shape
    assert se.dtype == torch.int8 and se.shape == (w.shape[0],)
    codes, se = codes.numpy(), se.numpy().astype(np.int64)

    amax = np.abs(w.astype(np.float64)).max(axis=1)
    for row in range(w.shape[0]):
        if row == zero_row:
            assert se[row] == 0 and not codes[row].any()
            continue
        # e = ceil(log2(amax / 448)), in exact arithmetic
        e = int(np.clip(se[row], -100, 100))
        if row not in clamped:
            assert amax[row] <= 448.0 * 2.0 ** e, row
            assert amax[row] > 448.0 * 2.0 ** (e - 1), row
        else:
            assert abs(e) == 100
        scaled = np.ldexp(w[row].astype(np.float64), -e).astype(np.float32)
        assert np.array_equal(codes[row], kr.fp8_e4m3_encode(scaled)), row
        top = np.abs(wr.decode_codes(codes[row])).max()
        if row not in clamped:
            # amax / 2^e is in (224, 448] (asserted above, exactly); its
            # code decodes into [224, 448]: a scaled amax one fp32 ulp
            # above 224 rounds to the code of 224 itself
            assert 224.0 <= top <= 448.0, (row, top)
            if amax[row] >= 232.0 * 2.0 ** e:  # past the midpoint to 240
                assert top > 224.0, (row, top)
    # the exact-448 rows keep e = j, the rows one ulp above take j + 1
    assert list(se[:10]) == [-20, -19, -1, 0, 0, 1, 3, 4, 40, 41]
    assert se[clamped[0]] == -100 and se[clamped[1]] == 100
    assert (codes[clamped[1]] & 0x7F).max() == 0x7E  # saturated, not NaN

    # any float dtype, and GPU-independent: bf16 weights give the codes
    # of their fp32 values
    wb = torch.from_numpy(w[:12]).to(torch.bfloat16)
    cb, sb = quantize_weight(wb)
    cf, sf = quantize_weight(wb.float())
    assert torch.equal(cb, cf) and torch.equal(sb, sf)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_quantize_weight_rejects_non_finite(bad):
    from client_amd.models.weight_fp8 import quantize_weight

    w = torch.randn(5, 64)
    w[3, 7] = bad
    with pytest.raises(ValueError, match="row 3"):
        quantize_weight(w)


def test_dequantize_is_exact_in_bf16():
    from client_amd.models.weight_fp8 import (dequantize_weight,
                                              quantize_weight)

    w, _, _ = _quantiser_rows()
    codes, se = quantize_weight(torch.from_numpy(w))
    want = wr.w_eff(codes.numpy(), se.numpy())
    got = dequantize_weight(codes, se, torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == w.shape
    assert np.array_equal(got.float().double().numpy(), want)
    got32 = dequantize_weight(codes, se, torch.float32)
    assert np.array_equal(got32.double().numpy(), want)
    # every finite code at three exponents
    allc = torch.from_numpy(
        np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8))
    for e in (-100, 0, 100):
        c = allc[None].repeat(2, 1)
        s = torch.full((2,), e, dtype=torch.int8)
        got = dequantize_weight(c, s, torch.bfloat16).float().double().numpy()
        assert np.array_equal(got, wr.w_eff(c.numpy(), s.numpy()))


def test_weight_dtype_names():
    from client_amd.models.weight_fp8 import (WEIGHT_DTYPES,
                                              normalize_weight_dtype)

    assert WEIGHT_DTYPES == ("bf16", FP8)
    assert normalize_weight_dtype(None) is None
    assert normalize_weight_dtype("bf16") is None
    assert normalize_weight_dtype(FP8) == FP8
    with pytest.raises(ValueError):
        normalize_weight_dtype("fp8")


@pytest.mark.parametrize("n,k", [(1, 64), (16, 64), (17, 128), (100, 576)])
def test_pack_codes_round_trip_and_layout(n, k):
    from client_amd.models.weight_fp8 import pack_codes, unpack_codes

    rng = np.random.default_rng(n * 1000 + k)
    codes = rng.integers(0, 256, (n, k), dtype=np.uint8)
    packed = pack_codes(torch.from_numpy(codes), pad=0x7F)
    tiles = (n + 15) // 16
    assert packed.shape == (tiles * 16 * k,)
    assert torch.equal(unpack_codes(packed, n, k), torch.from_numpy(codes))
    # the layout statement of weight_fp8.hip, element by element
    p = packed.numpy()
    kc = k // 64
    full = np.full((tiles * 16, k), 0x7F, np.uint8)
    full[:n] = codes
    for t, c, lane, b in [(0, 0, 0, 0), (tiles - 1, kc - 1, 63, 15),
                          (tiles - 1, 0, 17, 3), (0, kc - 1, 46, 9)]:
        got = p[((t * kc + c) * 64 + lane) * 16 + b]
        assert got == full[16 * t + (lane & 15), 64 * c + 16 * (lane >> 4) + b]
    with pytest.raises(ValueError):
        pack_codes(torch.zeros(4, 96, dtype=torch.uint8))


# ---------------------------------------------------------------------------
# llama_tiny: quantised == the same model with W_eff in nn.Linear
# ---------------------------------------------------------------------------


def _pair(seed):
    """(cfg, quantised model, reference): the reference is a deep copy
    whose seven linears per block carry W_eff as plain weights."""
    from client_amd.models.llama import LlamaModel, llama_tiny_config
    from client_amd.models.weight_fp8 import (LLAMA_BLOCK_LINEARS, Fp8Linear,
                                              quantize_llama_weights)

    torch.manual_seed(seed)
    cfg = llama_tiny_config()
    m = LlamaModel(cfg).eval()
    ref = copy.deepcopy(m)
    before, after = quantize_llama_weights(m)
    for bq, br in zip(m.blocks, ref.blocks):
        for name in LLAMA_BLOCK_LINEARS:
            q = getattr(bq, name)
            assert isinstance(q, Fp8Linear)
            lin = getattr(br, name)
            assert (q.out_features, q.in_features) == tuple(lin.weight.shape)
            assert not (lin.weight == q.effective_weight()).all()
            lin.weight.data = q.effective_weight(torch.float32)
    assert isinstance(m.lm_head, torch.nn.Linear)
    per_block = sum(p.numel() for p in ref.blocks[0].parameters()
                    if p.dim() == 2)
    assert before == 4 * cfg.n_layers * per_block
    # one byte per weight and one per row (tiny's rows are multiples of 16)
    rows = sum(getattr(ref.blocks[0], n).weight.shape[0]
               for n in LLAMA_BLOCK_LINEARS)
    assert after == cfg.n_layers * (per_block + rows)
    return cfg, m, ref


def test_quantised_forwards_bitwise_equal_weff_model():
    cfg, m, ref = _pair(0)
    b = 3
    plens = (9, 4, 12)
    kvs = [mod.make_kv_cache(b, "cpu", torch.float32) for mod in (m, ref)]
    with torch.inference_mode():
        for row, plen in enumerate(plens):
            ids = torch.randint(0, cfg.vocab_size, (1, plen))
            more = torch.randint(0, cfg.vocab_size, (1, 3))
            outs = []
            for mod, kv in zip((m, ref), kvs):
                row_kv = [(ck[row:row + 1], cv[row:row + 1]) for ck, cv in kv]
                a = mod.forward_step(ids, 0, row_kv)
                # a continuation chunk (s > 1 at pos > 0)
                c = mod.forward_step(more, plen, row_kv)
                outs.append((a, c))
            assert torch.equal(outs[0][0], outs[1][0])
            assert torch.equal(outs[0][1], outs[1][1])
        pos = torch.tensor([p + 3 for p in plens])
        for _ in range(3):
            tokens = torch.randint(0, cfg.vocab_size, (b, 1))
            lq = m.forward_decode_batch(tokens, pos, kvs[0])
            lr = ref.forward_decode_batch(tokens, pos, kvs[1], )
            assert torch.equal(lq, lr)
            pos = pos + 1
        # the chunked-prefill forward
        toks = torch.randint(0, cfg.vocab_size, (2, 8))
        args = (toks, torch.tensor([0, 0]), torch.tensor([8, 5]),
                torch.tensor([7, 4]))
        kq = m.make_kv_cache(2, "cpu", torch.float32)
        kr_ = ref.make_kv_cache(2, "cpu", torch.float32)
        assert torch.equal(m.forward_prefill_chunk(*args, kq, 16),
                           ref.forward_prefill_chunk(*args, kr_, 16))
    for (a, b_), (c, d) in zip(*kvs):
        assert torch.equal(a, c) and torch.equal(b_, d)
    # generate
    ids = torch.randint(0, cfg.vocab_size, (2, 6))
    assert ([t.tolist() for t in m.generate(ids, 5)]
            == [t.tolist() for t in ref.generate(ids, 5)])


def _drain(sched, queues):
    got = []
    for q in queues:
        toks = []
        while True:
            t = q.get(timeout=60)
            if t is sched.END:
                break
            toks.append(t)
        got.append(toks)
    return got


def _scheduler_streams(model, prompts, n_new, **kw):
    from client_amd.server.decode_scheduler import DecodeScheduler

    sched = DecodeScheduler(model, max_batch=4, device="cpu",
                            dtype=torch.float32, **kw)
    try:
        return _drain(sched, [sched.submit(p[0].numpy(), n_new)
                              for p in prompts])
    finally:
        sched.shutdown()


@pytest.mark.parametrize("plens,seeds", [((23, 7, 40), (9,)),
                                         ((4, 30, 45), (0, 1, 2))],
                         ids=["chunked_prefill", "mid_prefill"])
def test_scheduler_streams_equal_weff_model(plens, seeds):
    for seed in seeds:
        cfg, m, ref = _pair(seed)
        prompts = [torch.randint(0, cfg.vocab_size, (1, n)) for n in plens]
        got = _scheduler_streams(m, prompts, 6, prefill_chunk=8)
        want = _scheduler_streams(ref, prompts, 6, prefill_chunk=8)
        assert got == want, f"seed {seed}"
        assert got == [[int(t[0]) for t in m.generate(p, 6)]
                       for p in prompts], f"seed {seed}"


def test_module_casts_leave_codes_alone():
    from client_amd.models.weight_fp8 import Fp8Linear, quantize_weight

    torch.manual_seed(3)
    q = Fp8Linear(*quantize_weight(torch.randn(33, 128)))
    assert (q.in_features, q.out_features) == (128, 33)
    assert set(dict(q.named_buffers())) == {"codes", "scale_exp"}
    assert not list(q.parameters())
    codes, se = q.codes.clone(), q.scale_exp.clone()
    for dt in (torch.bfloat16, torch.float32):
        q = q.to(dt)
        assert q.codes.dtype == torch.uint8 and torch.equal(q.codes, codes)
        assert q.scale_exp.dtype == torch.int8
        assert torch.equal(q.scale_exp, se)
        x = torch.randn(2, 5, 128).to(dt)
        y = q(x)
        assert y.dtype == dt and y.shape == (2, 5, 33)
        assert torch.equal(
            y, torch.nn.functional.linear(x, q.effective_weight(dt)))
    with pytest.raises(ValueError):
        Fp8Linear.from_linear(torch.nn.Linear(64, 8, bias=True))


# ---------------------------------------------------------------------------
# server
# ---------------------------------------------------------------------------


def test_server_flag_and_model_config():
    from client_amd.models.weight_fp8 import Fp8Linear
    from client_amd.server.__main__ import build_core, build_parser
    from client_amd.server.grpc_server import GrpcServer
    import client_amd.grpc as grpcclient

    parser = build_parser()
    assert parser.parse_args([]).weight_dtype == "bf16"
    args = parser.parse_args(["--weight-dtype", FP8])
    assert args.weight_dtype == FP8
    with pytest.raises(SystemExit):
        parser.parse_args(["--weight-dtype", "int4"])

    plain = build_core(["llama_tiny"], device="cpu", dtype="fp32")
    default = build_core(["llama_tiny"], device="cpu", dtype="fp32",
                         weight_dtype="bf16")
    core = build_core(["llama_tiny"], device="cpu", dtype="fp32",
                      weight_dtype=args.weight_dtype)
    try:
        base_cfg = plain.models["llama_tiny"].config()
        assert "parameters" not in base_cfg
        assert default.models["llama_tiny"].config() == base_cfg
        for c in (plain, default):
            assert not any(isinstance(mod, Fp8Linear)
                           for mod in c.models["llama_tiny"].module.modules())
        model = core.models["llama_tiny"]
        cfg = model.config()
        assert cfg.pop("parameters") == {
            "weight_dtype": {"string_value": FP8}}
        assert cfg == base_cfg
        m = model.module
        assert isinstance(m.blocks[0].wq, Fp8Linear)
        assert isinstance(m.blocks[-1].w2, Fp8Linear)

        server = GrpcServer(core, host="127.0.0.1", port=0)
        server.start()
        try:
            client = grpcclient.InferenceServerClient(
                f"127.0.0.1:{server.port}")
            served = client.get_model_config("llama_tiny", as_json=True)
            assert (served["config"]["parameters"]["weight_dtype"]
                    ["string_value"]) == FP8
            # generates over gRPC (decoupled streaming)
            import queue

            got = queue.Queue()
            client.start_stream(
                callback=lambda result, error: got.put((result, error)))
            ids = np.array([5, 17, 200, 31], dtype=np.int64)
            i0 = grpcclient.InferInput("input_ids", [4], "INT64")
            i0.set_data_from_numpy(ids)
            i1 = grpcclient.InferInput("max_tokens", [1], "INT32")
            i1.set_data_from_numpy(np.array([4], np.int32))
            client.async_stream_infer("llama_tiny", [i0, i1])
            toks = []
            try:
                for _ in range(4):
                    r, e = got.get(timeout=30)
                    assert e is None, e
                    toks.append(int(r.as_numpy("token_id")[0]))
            finally:
                client.stop_stream()
                client.close()
        finally:
            server.stop(grace=1)
        with torch.inference_mode():
            want = [int(t[0]) for t in m.generate(
                torch.from_numpy(ids)[None], 4)]
        assert toks == want
    finally:
        for c in (plain, default, core):
            sched = c.models["llama_tiny"]._scheduler
            if sched is not None:
                sched.shutdown()


# ---------------------------------------------------------------------------
# the references, before a GPU is involved
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("m", wr.EXACT_M)
@pytest.mark.parametrize("n", wr.EXACT_N)
@pytest.mark.parametrize("k", wr.EXACT_K)
def test_exact_integer_cases_are_exact(m, n, k):
    x_bits, codes, se, expected, top = wr.exact_integer_case(m, n, k)
    assert top <= 2 * k <= 256
    x = kr.bf16_bits_to_f64(x_bits)
    w = wr.decode_codes(codes)
    assert set(np.unique(x)) <= {-1.0, 0.0, 1.0}
    assert set(np.unique(w)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(np.unique(se)) <= set(range(-3, 3)) and len(set(se)) > 1
    if m > 1:
        assert not np.array_equal(x[0], x[1])
        assert not np.array_equal(x[:, :m], x[:, :m].T)
    assert not np.array_equal(w[0], w[1])
    assert not np.array_equal(w[:16, :16], w[:16, :16].T)
    # the float64 reference agrees with zero tolerance, and so does any
    # fp32 summation order
    r, _ = wr.fp8w_gemm_ref(x_bits, codes, se)
    assert np.array_equal(kr.bf16_bits_to_f64(expected), r)
    got = wr.emulate_fp32(x_bits, codes, se, np.random.default_rng(k + n))
    assert np.array_equal(got, expected)


@pytest.mark.parametrize("shape", wr.RANDOM_SHAPES[:10],
                         ids=lambda s: "x".join(map(str, s)))
def test_fp32_emulation_within_bound(shape):
    """A shuffled-order fp32 accumulation of the GPU tests' inputs stays
    inside the bound the kernel is held to."""
    x_bits, codes, se = wr.random_case(*shape)
    assert se.min() >= -8 and se.max() <= 4
    r, delta = wr.fp8w_gemm_ref(x_bits, codes, se)
    for seed in (0, 1):
        got = wr.emulate_fp32(x_bits, codes, se, np.random.default_rng(seed))
        kr.assert_within_bf16_bound(got, r, delta, f"emulation {shape}")


def test_random_shapes_cover_the_axes():
    ms, ns, ks = (set(s[i] for s in wr.RANDOM_SHAPES) for i in range(3))
    assert ms >= {1, 7, 8, 9, 16}
    assert ns >= {1, 15, 16, 17, 33, 100}
    assert ks >= {64, 128, 576, 1024}


def test_bf16_rne_bits_matches_torch():
    rng = np.random.default_rng(4)
    x = rng.standard_normal(4096).astype(np.float32)
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]  # ties
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(wr.bf16_rne_bits(x), want.view(np.uint16))
