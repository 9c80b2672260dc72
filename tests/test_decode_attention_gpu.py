"""The fp8 KV-cache decode path on an MI355X: the fused GQA decode-
attention kernel (bf16 and e4m3 caches), the fp8 RoPE + scatter kernel,
and llama_tiny through both with an fp8 cache.

Attention outputs are bf16 computed with fp32 math and are checked per
element against a float64 reference built from the exact stored inputs:
|got - r| <= ulp_bf16(r)/2 + delta, with delta derived in
tests/attention_refs.py from the operation count, never from the
kernel's output.
"""

import numpy as np
import pytest

import attention_refs as ar
import kernel_refs as kr
from test_decode_edges_gpu import (PAD, _bf16_bits, _bits, _positions,
                                   _randn_bits, _rope_tables, _stream,
                                   _to_dev)

pytestmark = pytest.mark.gpu

KV = [False, True]
KV_IDS = ["bf16", "fp8"]


@pytest.fixture(scope="module")
def hr():
    from client_amd.ops import gpu_available, hip_runtime

    if not gpu_available():
        pytest.skip("no HIP device")
    return hip_runtime


def _store_to_dev(store, kv_fp8):
    import torch

    if kv_fp8:
        return torch.from_numpy(np.ascontiguousarray(store)).cuda()
    return _to_dev(store)[0]


def _store_bits(t, kv_fp8):
    return t.cpu().numpy().reshape(-1) if kv_fp8 else _bits(t)


def _attend(hr, q_bits, k_store, v_store, pos, max_len, kv_fp8, scale=1.0):
    """Runs the kernel; checks the sentinels behind out and that q, K, V
    and pos are unchanged. Returns output bits [b, hq, d]."""
    import torch

    b, hq, d = q_bits.shape
    hk, cache_len = k_store.shape[1:3]
    q, _ = _to_dev(q_bits)
    ck = _store_to_dev(k_store, kv_fp8)
    cv = _store_to_dev(v_store, kv_fp8)
    pos_d = torch.from_numpy(np.asarray(pos, dtype=np.int64)).cuda()
    out, tail = _to_dev(np.full((b, hq, d), 0x7FC1, np.uint16), PAD, d + b)
    ws_bytes = hr.gqa_decode_attention_workspace_bytes(b, hq, d, max_len)
    ws = torch.full((ws_bytes // 4,), float("nan"), device="cuda",
                    dtype=torch.float32)
    hr.gqa_decode_attention(q.data_ptr(), ck.data_ptr(), cv.data_ptr(),
                            pos_d.data_ptr(), out.data_ptr(), ws.data_ptr(),
                            ws_bytes, b, hq, hk, d, scale, max_len, cache_len,
                            kv_fp8, _stream())
    torch.cuda.synchronize()
    ob = _bits(out)
    assert np.array_equal(ob[b * hq * d:], tail), "wrote past the output"
    assert np.array_equal(_bits(q), q_bits.reshape(-1)), "q changed"
    assert np.array_equal(_store_bits(ck, kv_fp8), k_store.reshape(-1))
    assert np.array_equal(_store_bits(cv, kv_fp8), v_store.reshape(-1))
    assert np.array_equal(pos_d.cpu().numpy(), pos), "pos changed"
    return ob[:b * hq * d].reshape(b, hq, d)


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
@pytest.mark.parametrize("shape", ar.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_attention_rows_at_mixed_positions(hr, shape, kv_fp8):
    """Rows at different positions within one launch, every max_len, NaN
    patterns at every key position j >= n_i: a kernel that loads and
    masks, or does not clamp the inactive row's length to max_len,
    yields NaN."""
    split = hr.GQA_DECODE_SPLIT
    q, k, v = ar.random_case(shape, split, kv_fp8)
    for scale in (1.0, 0.75):
        for pos, max_len in ar.launches_for(shape[0], split):
            kp = ar.poison(k, pos, max_len, kv_fp8)
            vp = ar.poison(v, pos, max_len, kv_fp8)
            got = _attend(hr, q, kp, vp, pos, max_len, kv_fp8, scale)
            r, delta = ar.decode_attention_ref(q, kp, vp, pos, max_len,
                                               scale, kv_fp8)
            kr.assert_within_bf16_bound(
                got, r, delta,
                f"attention {shape} fp8={kv_fp8} pos={pos} "
                f"max_len={max_len} scale={scale}")


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
def test_attention_softmax_edges(hr, kv_fp8):
    split = hr.GQA_DECODE_SPLIT
    for name, q, k, v, pos, max_len in ar.softmax_edge_cases(split, kv_fp8):
        kp = ar.poison(k, pos, max_len, kv_fp8)
        vp = ar.poison(v, pos, max_len, kv_fp8)
        got = _attend(hr, q, kp, vp, pos, max_len, kv_fp8)
        r, delta = ar.decode_attention_ref(q, kp, vp, pos, max_len, 1.0,
                                           kv_fp8)
        kr.assert_within_bf16_bound(got, r, delta,
                                    f"attention {name} fp8={kv_fp8}")
        if name == "single":
            # one key: the output is V's row, exactly
            want = ar.decode_stored(v[:, :, 0], kv_fp8)
            rep = q.shape[1] // k.shape[1]
            assert np.array_equal(kr.bf16_bits_to_f64(got),
                                  np.repeat(want, rep, axis=1))


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
def test_attention_row_bits_invariant(hr, kv_fp8):
    """A row's output bits do not depend on the batch size, the row's
    index, the other rows' lengths or max_len."""
    split = hr.GQA_DECODE_SPLIT
    shape = (3, 8, 2, 128)
    q3, k3, v3 = ar.random_case(shape, split, kv_fp8, seed=5)
    max_lens = ar.max_lens_for(split)
    for n in (split - 3, split + 1, 2 * split):
        pos3 = np.array([2 * split + 7, 2 * split + 3, n - 1], dtype=np.int64)
        seen = []
        for max_len in (ml for ml in max_lens if ml >= n):
            got = _attend(hr, q3, ar.poison(k3, pos3, max_len, kv_fp8),
                          ar.poison(v3, pos3, max_len, kv_fp8), pos3,
                          max_len, kv_fp8)
            seen.append(got[2])
            pos1 = pos3[2:]
            got = _attend(hr, q3[2:], ar.poison(k3[2:], pos1, max_len, kv_fp8),
                          ar.poison(v3[2:], pos1, max_len, kv_fp8), pos1,
                          max_len, kv_fp8)
            seen.append(got[0])
        assert len(seen) >= 2
        for other in seen[1:]:
            assert np.array_equal(seen[0], other), f"n={n}"


def test_attention_argument_checks(hr):
    import torch

    split = hr.GQA_DECODE_SPLIT
    L = ar.cache_len_for(split)
    s = _stream()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 0x1234, dtype=torch.int16, device="cuda")
    pos = torch.zeros(4, dtype=torch.int64, device="cuda")

    def call(b, hq, hk, d, max_len=split, ws_bytes=None, cache_len=L):
        if ws_bytes is None:
            ws_bytes = hr.gqa_decode_attention_workspace_bytes(
                b, hq, d, max_len)
        hr.gqa_decode_attention(buf.data_ptr(), buf.data_ptr(),
                                buf.data_ptr(), pos.data_ptr(),
                                out.data_ptr(), buf.data_ptr(), ws_bytes, b,
                                hq, hk, d, 1.0, max_len, cache_len, True, s)

    need = hr.gqa_decode_attention_workspace_bytes(2, 4, 16, 2 * split)
    assert need >= 2 * 4 * 2 * (16 + 2) * 4
    for bad in (dict(d=24), dict(d=256), dict(hq=3, hk=2), dict(hq=18, hk=2),
                dict(ws_bytes=need - 4, max_len=2 * split),
                dict(max_len=L + 1), dict(max_len=0)):
        args = dict(b=2, hq=4, hk=2, d=16)
        args.update(bad)
        with pytest.raises(RuntimeError):
            call(**args)
    call(0, 4, 2, 16)  # b = 0 returns without a launch
    torch.cuda.synchronize()
    assert (out == 0x1234).all()


# ---------------------------------------------------------------------------
# rope_scatter_decode_fp8kv_bf16
# ---------------------------------------------------------------------------

SCATTER_SHAPES = [(3, 4, 2, 16), (2, 8, 2, 128)]


def _fp8_scatter_case(hr, shape, cache_len, q_scale, flip, skip_row=None):
    import torch

    b, hq, hk, d = shape
    cos, sin = _rope_tables(d, cache_len)
    cos_d = torch.from_numpy(cos).cuda()
    sin_d = torch.from_numpy(sin).cuda()
    rng = np.random.default_rng(b * 1000 + d + cache_len)
    qb = _randn_bits(rng, b, hq, d)
    kb = _randn_bits(rng, b, hk, d)
    # v holds random bit patterns: NaNs, Infs and finite values beyond
    # +-448 included
    vb = rng.integers(0, 2 ** 16, (b, hk, d), dtype=np.uint16)
    vb[0, 0, :4] = (0x7FC1, 0xFF81, int(_bf16_bits(1000.0)),
                    int(_bf16_bits(-449.0)))
    pos = _positions(b, cache_len, flip)
    if skip_row is not None:
        pos[skip_row] = cache_len
    live = pos < cache_len
    pos_d = torch.from_numpy(pos).cuda()
    what = f"fp8 scatter {shape} cache_len={cache_len} q_scale={q_scale}"

    # the bf16 kernel on the same inputs (live rows only: it has no
    # position guard) says what the cache would hold in bf16
    ref_pos = np.where(live, pos, 0)
    q_ref, _ = _to_dev(qb)
    k, _ = _to_dev(kb)
    v, _ = _to_dev(vb)
    ck16, _ = _to_dev(np.zeros((b, hk, cache_len, d), np.uint16))
    cv16, _ = _to_dev(np.zeros((b, hk, cache_len, d), np.uint16))
    hr.rope_scatter_decode_bf16(
        q_ref.data_ptr(), k.data_ptr(), v.data_ptr(), ck16.data_ptr(),
        cv16.data_ptr(), cos_d.data_ptr(), sin_d.data_ptr(),
        torch.from_numpy(ref_pos).cuda().data_ptr(), b, hq, hk, d, cache_len,
        q_scale=q_scale, stream_handle=_stream())

    q, qtail = _to_dev(qb, PAD, 3)
    # caches pre-filled with random bytes
    ckb = rng.integers(0, 256, (b, hk, cache_len, d), dtype=np.uint8)
    cvb = rng.integers(0, 256, (b, hk, cache_len, d), dtype=np.uint8)
    tails = [rng.integers(0, 256, PAD, dtype=np.uint8) for _ in range(2)]
    ck = torch.from_numpy(np.concatenate([ckb.reshape(-1), tails[0]])).cuda()
    cv = torch.from_numpy(np.concatenate([cvb.reshape(-1), tails[1]])).cuda()
    hr.rope_scatter_decode_fp8kv_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), ck.data_ptr(),
        cv.data_ptr(), cos_d.data_ptr(), sin_d.data_ptr(), pos_d.data_ptr(),
        b, hq, hk, d, cache_len, q_scale=q_scale, stream_handle=_stream())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(k), kb.reshape(-1)), what + ": k changed"
    assert np.array_equal(_bits(v), vb.reshape(-1)), what + ": v changed"

    got_q = _bits(q)
    assert np.array_equal(got_q[qb.size:], qtail), what + ": q sentinel"
    got_q = got_q[:qb.size].reshape(qb.shape)
    want_q = _bits(q_ref).reshape(qb.shape)
    assert np.array_equal(got_q[live], want_q[live]), what + ": q bits"
    assert np.array_equal(got_q[~live], qb[~live]), what + ": skipped q"

    rows = np.arange(b)[live]
    for name, t, tail, before, t16 in (("ck", ck, tails[0], ckb, ck16),
                                       ("cv", cv, tails[1], cvb, cv16)):
        got = t.cpu().numpy()
        assert np.array_equal(got[before.size:], tail), (
            f"{what}: {name} sentinel")
        got = got[:before.size].reshape(before.shape)
        slot = got[rows, :, pos[live]]                      # [live, hk, d]
        bf16_slot = _bits(t16).reshape(before.shape)[rows, :, pos[live]]
        vals = kr.bf16_wire_decode(bf16_slot).reshape(bf16_slot.shape)
        want = kr.fp8_e4m3_encode(vals).reshape(slot.shape)
        finite = np.isfinite(vals)
        assert np.array_equal(slot[finite], want[finite]), (
            f"{what}: {name} codes")
        assert np.all(slot[~finite] & 0x7F == 0x7F), f"{what}: {name} NaN"
        big = finite & (np.abs(vals) > 448)
        assert np.all(slot[big] & 0x7F == 0x7E), f"{what}: {name} saturation"
        if name == "cv":
            assert big.any() and (~finite).any()
        else:
            # the codes are within half an e4m3 ulp of a value inside
            # rope_ref's bf16 bound
            rk, dk = kr.rope_ref(kb, cos, sin, ref_pos)
            rk, dk = rk[live], dk[live]
            dec = ar.decode_stored(slot, True)
            lim = kr.bf16_bound(rk, dk)
            lim = lim + ar.fp8_half_ulp(np.abs(rk) + lim)
            assert np.all(np.abs(dec - rk) <= lim), what + ": k bound"
        untouched = np.ones(before.shape[:3], dtype=bool)
        untouched[rows, :, pos[live]] = False
        assert np.array_equal(got[untouched], before[untouched]), (
            f"{what}: {name} changed outside [row, :, pos[row]]")


@pytest.mark.parametrize("shape", SCATTER_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_fp8_scatter_edges(hr, shape):
    d = shape[3]
    for cache_len in (1, 33):
        for q_scale in (1.0, d ** -0.5):
            for flip in (False, True):
                _fp8_scatter_case(hr, shape, cache_len, q_scale, flip)


@pytest.mark.parametrize("shape", SCATTER_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_fp8_scatter_row_past_cache_writes_nothing(hr, shape):
    _fp8_scatter_case(hr, shape, 33, shape[3] ** -0.5, False, skip_row=1)
    _fp8_scatter_case(hr, shape, 33, 1.0, True, skip_row=0)


# ---------------------------------------------------------------------------
# llama_tiny, bf16, fp8 cache
# ---------------------------------------------------------------------------

FP8 = "fp8_e4m3"


def _tiny_gpu(seed):
    import torch

    from client_amd.models.llama import LlamaModel, llama_tiny_config

    torch.manual_seed(seed)
    cfg = llama_tiny_config()
    return cfg, LlamaModel(cfg).to("cuda:0").to(torch.bfloat16).eval()


def test_fused_decode_matches_torch_fallback(hr, monkeypatch):
    """Logits of the fused path (fp8 scatter + attention kernels)
    against the torch fallback (encode on scatter, dequantised window)
    on the same cache state; the bound test_gqa_bmm_decode_matches_sdpa
    applies to two attention implementations over the same weights."""
    import torch

    from client_amd.models import llama

    cfg, m = _tiny_gpu(21)
    b = 3
    plens = (4, 17, 9)
    kv = m.make_kv_cache(b, "cuda:0", torch.bfloat16, kv_dtype=FP8)
    with torch.inference_mode():
        for row, plen in enumerate(plens):
            ids = torch.randint(0, cfg.vocab_size, (1, plen), device="cuda:0")
            m.forward_step(ids, 0, [(ck[row:row + 1], cv[row:row + 1])
                                    for ck, cv in kv])
        kv2 = [(ck.clone(), cv.clone()) for ck, cv in kv]
        tokens = torch.randint(0, cfg.vocab_size, (b, 1), device="cuda:0")
        pos = torch.tensor(plens, device="cuda:0")
        fused = m.forward_decode_batch(tokens, pos, kv, max_len=32)
        monkeypatch.setattr(llama, "_fused_attn_supported",
                            lambda *a: False)
        fallback = m.forward_decode_batch(tokens, pos, kv2, max_len=32)
    torch.cuda.synchronize()
    assert torch.isfinite(fused).all()
    torch.testing.assert_close(fused.float(), fallback.float(), atol=0.25,
                               rtol=0.05)
    # layer 0's K/V do not depend on attention: identical bytes from the
    # HIP scatter and from the torch encode
    assert torch.equal(kv[0][0], kv2[0][0])
    assert torch.equal(kv[0][1], kv2[0][1])


def _run(sched, prompt, n, sampling=None):
    q = sched.submit(prompt, n, sampling)
    toks = []
    while True:
        t = q.get(timeout=120)
        if t is sched.END:
            return toks
        toks.append(t)


def test_fp8_scheduler_graph_matches_eager(hr):
    import torch

    from client_amd.server.decode_scheduler import DecodeScheduler

    cfg, m = _tiny_gpu(7)
    prompts = [np.array([5, 17, 200, 31, 8, 99], dtype=np.int64),
               np.arange(3, 40, dtype=np.int64)]
    got = {}
    for use_graph in (False, True):
        sched = DecodeScheduler(m, max_batch=2, device="cuda:0",
                                use_graph=use_graph, len_bucket=32,
                                kv_dtype=FP8)
        try:
            assert sched.kv_cache[0][0].dtype == torch.uint8
            got[use_graph] = [_run(sched, p, 10) for p in prompts]
            if use_graph:
                assert sched._graphs and all(
                    g is not sched._EAGER for g in sched._graphs.values())
        finally:
            sched.shutdown()
    assert got[True] == got[False]
    assert all(len(t) == 10 for t in got[True])


def test_fp8_seeded_sampling_independent_of_batch(hr):
    """A seeded sampled request yields the same tokens alone and
    alongside two other requests."""
    from client_amd.models.sampling import SamplingParams
    from client_amd.server.decode_scheduler import DecodeScheduler

    cfg, m = _tiny_gpu(7)
    prompt = np.array([5, 17, 200, 31, 8, 99], dtype=np.int64)
    others = [np.arange(3, 50, dtype=np.int64),
              np.array([9, 9, 1], dtype=np.int64)]
    params = SamplingParams(temperature=1.0, top_k=40, top_p=0.95, seed=1234)
    sched = DecodeScheduler(m, max_batch=4, device="cuda:0", use_graph=True,
                            len_bucket=32, kv_dtype=FP8)
    try:
        alone = _run(sched, prompt, 12, params)
        # the two others are decoding before the seeded request arrives
        # and still are when it ends
        busy = [sched.submit(others[0], 30),
                sched.submit(others[1], 30, SamplingParams(
                    temperature=0.8, seed=5))]
        first = [q.get(timeout=120) for q in busy]
        shared = _run(sched, prompt, 12, params)
        rest = []
        for q in busy:
            toks = []
            while True:
                t = q.get(timeout=120)
                if t is sched.END:
                    break
                toks.append(t)
            rest.append(toks)
        assert len(alone) == 12 and len(first) == 2
        assert all(len(t) == 29 for t in rest)
        assert shared == alone
    finally:
        sched.shutdown()
