"""FP8 (e4m3) KV cache on the CPU: the host-side format contract, the
torch paths of the three Llama forwards over a uint8 cache, scheduler
and server plumbing, and the decode-attention error bound checked
against an fp32 emulation of the kernel's algorithm."""

import numpy as np
import pytest

import attention_refs as ar
import kernel_refs as kr

torch = pytest.importorskip("torch")

FP8 = "fp8_e4m3"


# ---------------------------------------------------------------------------
# encode / decode
# ---------------------------------------------------------------------------


def test_kv_encode_matches_cast_contract():
    from client_amd.models.kv_cache import kv_encode_fp8

    finite, beyond = kr.fp8_edge_inputs()
    x = np.concatenate([finite, beyond])
    got = kv_encode_fp8(torch.from_numpy(x)).numpy()
    assert got.dtype == np.uint8
    exp = kr.fp8_e4m3_encode(x)
    finite = np.isfinite(x)
    assert np.array_equal(got[finite], exp[finite])
    # NaN stays NaN and +-Inf gives a NaN code (the sign bit of a NaN
    # code is not part of the contract)
    assert np.all(got[~finite] & 0x7F == 0x7F)
    assert np.all(exp[~finite] & 0x7F == 0x7F)
    # saturation, not NaN, above 464; signed zeros keep their sign
    t = torch.tensor([500.0, 460.0, -1000.0, 0.0, -0.0])
    assert kv_encode_fp8(t).tolist() == [0x7E, 0x7E, 0xFE, 0x00, 0x80]
    # any float dtype
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert kv_encode_fp8(t.to(dt)).tolist() == [0x7E, 0x7E, 0xFE, 0, 0x80]


def test_kv_decode_matches_table():
    from client_amd.models.kv_cache import kv_decode_fp8, kv_encode_fp8

    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    tab = kr.fp8_e4m3_decode_table()
    nan = np.isnan(tab)
    for dt in (torch.float32, torch.bfloat16):
        got = kv_decode_fp8(codes, dt)
        assert got.dtype == dt
        got = got.double().numpy()
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan], tab[~nan])  # exact, bf16 included
        assert np.array_equal(np.signbit(got[~nan]), np.signbit(tab[~nan]))
    # the inverse of encode on every finite code
    back = kv_encode_fp8(kv_decode_fp8(codes, torch.float32)).numpy()
    assert np.array_equal(back[~nan], codes.numpy()[~nan])


def test_kv_dtype_names():
    from client_amd.models.kv_cache import normalize_kv_dtype

    assert normalize_kv_dtype(None) is None
    assert normalize_kv_dtype("bf16") is None
    assert normalize_kv_dtype(FP8) == FP8
    with pytest.raises(ValueError):
        normalize_kv_dtype("fp8")


# ---------------------------------------------------------------------------
# cache tensors
# ---------------------------------------------------------------------------


def _tiny(seed):
    from client_amd.models.llama import LlamaModel, llama_tiny_config

    torch.manual_seed(seed)
    cfg = llama_tiny_config()
    return cfg, LlamaModel(cfg).eval()


def _nbytes(cache):
    return sum(t.numel() * t.element_size() for pair in cache for t in pair)


def test_fp8_cache_tensors():
    cfg, m = _tiny(0)
    plain32 = m.make_kv_cache(3, "cpu", torch.float32)
    plain16 = m.make_kv_cache(3, "cpu", torch.bfloat16, kv_dtype="bf16")
    fp8 = m.make_kv_cache(3, "cpu", torch.float32, kv_dtype=FP8)
    assert len(fp8) == cfg.n_layers
    for (ck, cv), (pk, pv) in zip(fp8, plain32):
        assert ck.dtype == cv.dtype == torch.uint8
        assert ck.shape == pk.shape and cv.shape == pv.shape
        assert not ck.any() and not cv.any()
    assert plain16[0][0].dtype == torch.bfloat16
    assert 2 * _nbytes(fp8) == _nbytes(plain16)
    assert 4 * _nbytes(fp8) == _nbytes(plain32)
    with pytest.raises(ValueError):
        m.make_kv_cache(1, "cpu", torch.float32, kv_dtype="int4")


def test_layer0_bytes_are_encoded_plain_cache():
    """Layer 0's K/V do not depend on attention, so an fp8 cache holds
    exactly encode(plain cache) there: at every written position, by
    prefill (forward_step) and by two decode steps at different row
    positions; zero elsewhere, but for the scratch position."""
    from client_amd.models.kv_cache import kv_encode_fp8

    cfg, m = _tiny(11)
    b = 2
    plens = (5, 9)
    caches = {None: m.make_kv_cache(b, "cpu", torch.float32),
              FP8: m.make_kv_cache(b, "cpu", torch.float32, kv_dtype=FP8)}
    prompts = [torch.randint(0, cfg.vocab_size, (1, n)) for n in plens]
    steps = [torch.randint(0, cfg.vocab_size, (b, 1)) for _ in range(2)]
    with torch.inference_mode():
        for kv in caches.values():
            for row, ids in enumerate(prompts):
                m.forward_step(ids, 0, [(ck[row:row + 1], cv[row:row + 1])
                                        for ck, cv in kv])
            pos = torch.tensor(plens)
            for toks in steps:
                m.forward_decode_batch(toks, pos, kv)
                pos = pos + 1
    for which in (0, 1):
        plain = caches[None][0][which]
        codes = caches[FP8][0][which]
        assert plain.abs().max() > 0
        assert torch.equal(codes, kv_encode_fp8(plain))
        for row, plen in enumerate(plens):
            assert codes[row, :, :plen + 2].any(dim=-1).all()
            assert not codes[row, :, plen + 2:m.scratch_pos].any()


# ---------------------------------------------------------------------------
# the existing model and scheduler properties, both sides on an fp8 cache
# ---------------------------------------------------------------------------


def test_decode_batch_padded_maxlen_equivalent_fp8():
    cfg, m = _tiny(5)
    b = 3
    kv1 = m.make_kv_cache(b, "cpu", torch.float32, kv_dtype=FP8)
    kv2 = m.make_kv_cache(b, "cpu", torch.float32, kv_dtype=FP8)
    with torch.inference_mode():
        for row, plen in enumerate((4, 7, 2)):
            ids = torch.randint(0, cfg.vocab_size, (1, plen))
            row_kv1 = [(ck[row:row+1], cv[row:row+1]) for ck, cv in kv1]
            row_kv2 = [(ck[row:row+1], cv[row:row+1]) for ck, cv in kv2]
            m.forward_step(ids, 0, row_kv1)
            m.forward_step(ids, 0, row_kv2)
        tokens = torch.randint(0, cfg.vocab_size, (b, 1))
        pos = torch.tensor([4, 7, 2])
        exact = m.forward_decode_batch(tokens, pos, kv1)
        padded = m.forward_decode_batch(tokens, pos, kv2, max_len=64)
    torch.testing.assert_close(exact, padded, rtol=1e-5, atol=1e-5)
    for (a, _), (c, _) in zip(kv1, kv2):
        assert a.dtype == torch.uint8 and torch.equal(a, c)


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


def _scheduler_matches_generate(m, prompts, n_new, **kw):
    from client_amd.server.decode_scheduler import DecodeScheduler

    expected = [[int(t[0]) for t in m.generate(p, n_new, kv_dtype=FP8)]
                for p in prompts]
    sched = DecodeScheduler(m, max_batch=4, device="cpu",
                            dtype=torch.float32, kv_dtype=FP8, **kw)
    try:
        assert sched.kv_cache[0][0].dtype == torch.uint8
        got = _drain(sched, [sched.submit(p[0].numpy(), n_new)
                             for p in prompts])
    finally:
        sched.shutdown()
    return got, expected


def test_decode_scheduler_matches_sequential_fp8():
    cfg, m = _tiny(3)
    prompts = [torch.randint(0, cfg.vocab_size, (1, n)) for n in (5, 9, 3)]
    got, expected = _scheduler_matches_generate(m, prompts, 6)
    assert got == expected


def test_chunked_prefill_matches_full_fp8():
    cfg, m = _tiny(9)
    prompts = [torch.randint(0, cfg.vocab_size, (1, n)) for n in (23, 7, 40)]
    got, expected = _scheduler_matches_generate(m, prompts, 6,
                                                prefill_chunk=8)
    assert got == expected


def test_mid_prefill_rows_not_corrupted_by_decode_fp8():
    for seed in range(5):
        cfg, m = _tiny(seed)
        prompts = [torch.randint(0, cfg.vocab_size, (1, n))
                   for n in (4, 30, 45)]
        got, expected = _scheduler_matches_generate(m, prompts, 8,
                                                    prefill_chunk=8)
        assert got == expected, f"divergence at seed {seed}"


# ---------------------------------------------------------------------------
# server
# ---------------------------------------------------------------------------


def test_server_flag_and_model_config():
    from client_amd.server.__main__ import build_core, build_parser
    from client_amd.server.grpc_server import GrpcServer
    import client_amd.grpc as grpcclient

    parser = build_parser()
    assert parser.parse_args([]).kv_cache_dtype == "bf16"
    args = parser.parse_args(["--kv-cache-dtype", FP8])
    assert args.kv_cache_dtype == FP8
    with pytest.raises(SystemExit):
        parser.parse_args(["--kv-cache-dtype", "int4"])

    plain = build_core(["llama_tiny"], device="cpu", dtype="fp32")
    default = build_core(["llama_tiny"], device="cpu", dtype="fp32",
                         kv_cache_dtype="bf16")
    core = build_core(["llama_tiny"], device="cpu", dtype="fp32",
                      kv_cache_dtype=args.kv_cache_dtype)
    try:
        base_cfg = plain.models["llama_tiny"].config()
        assert "parameters" not in base_cfg
        assert default.models["llama_tiny"].config() == base_cfg
        model = core.models["llama_tiny"]
        cfg = model.config()
        assert cfg.pop("parameters") == {
            "kv_cache_dtype": {"string_value": FP8}}
        assert cfg == base_cfg
        assert model._scheduler.kv_cache[0][0].dtype == torch.uint8

        # a client sees it over gRPC, and the model generates
        server = GrpcServer(core, host="127.0.0.1", port=0)
        server.start()
        try:
            client = grpcclient.InferenceServerClient(
                f"127.0.0.1:{server.port}")
            served = client.get_model_config("llama_tiny", as_json=True)
            assert (served["config"]["parameters"]["kv_cache_dtype"]
                    ["string_value"]) == FP8
            client.close()
        finally:
            server.stop(grace=1)
        ids = np.array([5, 17, 200, 31], dtype=np.int64)
        toks = [int(out["token_id"][0]) for out in model.execute_decoupled(
            {"input_ids": ids, "max_tokens": np.array([4], np.int32)}, {})]
        m = model.module
        with torch.inference_mode():
            want = [int(t[0]) for t in m.generate(
                torch.from_numpy(ids)[None], 4, kv_dtype=FP8)]
        assert toks == want
    finally:
        for c in (plain, default, core):
            sched = c.models["llama_tiny"]._scheduler
            if sched is not None:
                sched.shutdown()


# ---------------------------------------------------------------------------
# the decode-attention bound, before a GPU is involved
# ---------------------------------------------------------------------------


def _split():
    from client_amd.ops import hip_runtime as hr

    return int(hr.GQA_DECODE_SPLIT)


@pytest.mark.parametrize("kv_fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("shape", ar.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_fp32_emulation_within_bound(shape, kv_fp8):
    """The split + online-softmax + combine algorithm in numpy fp32, on
    the inputs of the GPU tests, stays inside attention_refs' bound
    against the float64 reference."""
    split = _split()
    q, k, v = ar.random_case(shape, split, kv_fp8)
    scale = 1.0
    for pos, max_len in ar.launches_for(shape[0], split):
        kp = ar.poison(k, pos, max_len, kv_fp8)
        vp = ar.poison(v, pos, max_len, kv_fp8)
        got = ar.emulate_fp32(q, kp, vp, pos, max_len, scale, kv_fp8, split)
        r, delta = ar.decode_attention_ref(q, kp, vp, pos, max_len, scale,
                                           kv_fp8)
        kr.assert_within_bf16_bound(
            got, r, delta, f"emulation {shape} pos={pos} max_len={max_len}")


@pytest.mark.parametrize("kv_fp8", [False, True], ids=["bf16", "fp8"])
def test_fp32_emulation_softmax_edges(kv_fp8):
    split = _split()
    for name, q, k, v, pos, max_len in ar.softmax_edge_cases(split, kv_fp8):
        got = ar.emulate_fp32(q, k, v, pos, max_len, 1.0, kv_fp8, split)
        r, delta = ar.decode_attention_ref(q, k, v, pos, max_len, 1.0,
                                           kv_fp8)
        kr.assert_within_bf16_bound(got, r, delta, f"emulation {name}")
