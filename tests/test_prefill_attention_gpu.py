"""The fused prefill path on an MI355X: the MFMA chunk-attention kernel
over bf16 and e4m3 caches, the prefill RoPE + scatter kernels against
the decode kernels, and llama_tiny through both.

Attention outputs are bf16 and are checked per element against a
float64 reference built from the exact stored inputs:
|got - r| <= ulp_bf16(r)/2 + delta, with delta derived in
tests/prefill_attention_refs.py from the operation count, never from
the kernel's output.
"""

import numpy as np
import pytest

import attention_refs as ar
import kernel_refs as kr
import prefill_attention_refs as pr
from test_decode_edges_gpu import (PAD, _bits, _randn_bits, _rope_tables,
                                   _stream, _to_dev)

pytestmark = pytest.mark.gpu

KV = [False, True]
KV_IDS = ["bf16", "fp8"]


@pytest.fixture(scope="module")
def hr():
    from client_amd.ops import gpu_available, hip_runtime

    if not gpu_available():
        pytest.skip("no HIP device")
    return hip_runtime


def _tiles(hr):
    return int(hr.GQA_PREFILL_QTILE), int(hr.GQA_PREFILL_KTILE)


def _store_to_dev(store, kv_fp8):
    import torch

    if kv_fp8:
        return torch.from_numpy(np.ascontiguousarray(store)).cuda()
    return _to_dev(store)[0]


def _store_bits(t, kv_fp8):
    return t.cpu().numpy().reshape(-1) if kv_fp8 else _bits(t)


def _i64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _attend(hr, q_bits, k_store, v_store, pos, lens, row_map, max_len,
            kv_fp8, scale=1.0):
    """Runs the kernel; checks the sentinels behind out and that q, K, V,
    pos, lens and map are unchanged. Returns output bits [B, C, hq, d]."""
    import torch

    b, c, hq, d = q_bits.shape
    rows, hk, cache_len = k_store.shape[:3]
    q, _ = _to_dev(q_bits)
    ck = _store_to_dev(k_store, kv_fp8)
    cv = _store_to_dev(v_store, kv_fp8)
    pos_d, lens_d, map_d = _i64(pos), _i64(lens), _i64(row_map)
    n = b * c * hq * d
    out, tail = _to_dev(np.full((b, c, hq, d), 0x7FC1, np.uint16), PAD, d + b)
    ws_bytes = hr.gqa_prefill_attention_workspace_bytes(b, c, hq, d, max_len)
    ws = torch.full((ws_bytes // 4 + 1,), float("nan"), device="cuda",
                    dtype=torch.float32)
    hr.gqa_prefill_attention(
        q.data_ptr(), ck.data_ptr(), cv.data_ptr(), pos_d.data_ptr(),
        lens_d.data_ptr(), map_d.data_ptr(), out.data_ptr(), ws.data_ptr(),
        ws_bytes, b, c, hq, hk, d, scale, max_len, cache_len, rows, kv_fp8,
        _stream())
    torch.cuda.synchronize()
    ob = _bits(out)
    assert np.array_equal(ob[n:], tail), "wrote past the output"
    assert np.array_equal(_bits(q), np.asarray(q_bits).reshape(-1)), "q changed"
    assert np.array_equal(_store_bits(ck, kv_fp8), k_store.reshape(-1))
    assert np.array_equal(_store_bits(cv, kv_fp8), v_store.reshape(-1))
    assert np.array_equal(pos_d.cpu().numpy(), pos), "pos changed"
    assert np.array_equal(lens_d.cpu().numpy(), lens), "lens changed"
    assert np.array_equal(map_d.cpu().numpy(), row_map), "row_map changed"
    return ob[:n].reshape(b, c, hq, d)


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
@pytest.mark.parametrize("shape", pr.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_attention_mixed_rows(hr, shape, kv_fp8):
    """Rows at different positions and lengths in one launch, the causal
    diagonal crossing query and key tiles, NaN patterns behind every
    row's own keys and in every unmapped cache row: a kernel that loads
    and masks, or reads the wrong cache row, yields NaN."""
    qt, kt = _tiles(hr)
    for q, kp, vp, pos, lens, row_map, max_len, scale in pr.mixed_row_cases(
            shape, qt, kt, kv_fp8):
        got = _attend(hr, q, kp, vp, pos, lens, row_map, max_len, kv_fp8,
                      scale)
        r, delta, real = pr.prefill_attention_ref(
            q, kp, vp, pos, lens, row_map, max_len, scale, kv_fp8)
        kr.assert_within_bf16_bound(
            got, r, delta, f"prefill attention {shape} fp8={kv_fp8} "
                           f"pos={pos} lens={lens} map={row_map} "
                           f"max_len={max_len}")
        assert np.all(got[~real] == 0), "c >= row_lens is not exact zero"


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
def test_attention_softmax_edges(hr, kv_fp8):
    qt, kt = _tiles(hr)
    for name, q, k, v, pos, lens, max_len in pr.softmax_edge_cases(
            qt, kt, kv_fp8):
        row_map = np.arange(q.shape[0], dtype=np.int64)
        kp = pr.poison(k, pos, lens, row_map, max_len, kv_fp8)
        vp = pr.poison(v, pos, lens, row_map, max_len, kv_fp8)
        got = _attend(hr, q, kp, vp, pos, lens, row_map, max_len, kv_fp8)
        r, delta, _ = pr.prefill_attention_ref(q, kp, vp, pos, lens, row_map,
                                               max_len, 1.0, kv_fp8)
        kr.assert_within_bf16_bound(got, r, delta,
                                    f"prefill attention {name} fp8={kv_fp8}")
        if name == "single":
            # one key: query 0's output is V's row, exactly
            want = ar.decode_stored(v[:, :, 0], kv_fp8)
            rep = q.shape[2] // k.shape[1]
            assert np.array_equal(kr.bf16_bits_to_f64(got[:, 0]),
                                  np.repeat(want, rep, axis=1))


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
def test_attention_row_bits_invariant(hr, kv_fp8):
    """A row's output bits do not depend on the batch size, the row's
    index, the cache row it is mapped to, the other rows or max_len."""
    qt, kt = _tiles(hr)
    shape = (3, 8, 2, 128)
    c, L = pr.chunk_for(qt), pr.cache_len_for(qt, kt)
    q3, k3, v3 = pr.random_case(shape, c, L, 3, kv_fp8, seed=5)
    pos3 = np.array([1, kt + 1, kt - 1], dtype=np.int64)
    lens3 = np.array([c, qt - 1, qt + 1], dtype=np.int64)
    ident = np.arange(3, dtype=np.int64)
    small, large = 2 * kt, 2 * kt + qt + 8
    assert (pos3 + lens3).max() <= small

    def run(q, k, v, pos, lens, row_map, max_len):
        return _attend(hr, q, pr.poison(k, pos, lens, row_map, max_len,
                                        kv_fp8),
                       pr.poison(v, pos, lens, row_map, max_len, kv_fp8),
                       pos, lens, row_map, max_len, kv_fp8)

    base = run(q3, k3, v3, pos3, lens3, ident, small)[2]
    # alone
    one = np.zeros(1, dtype=np.int64)
    alone = run(q3[2:], k3[2:], v3[2:], pos3[2:], lens3[2:], one, small)[0]
    # through another cache row of a larger cache, next to other rows
    k5 = np.concatenate([k3[1:2], k3[0:1], k3[0:1], k3[2:3], k3[1:2]])
    v5 = np.concatenate([v3[1:2], v3[0:1], v3[0:1], v3[2:3], v3[1:2]])
    remap = np.array([1, 4, 3], dtype=np.int64)
    moved = run(q3, k5, v5, pos3, lens3, remap, small)[2]
    # a larger bucket
    wide = run(q3, k3, v3, pos3, lens3, ident, large)[2]
    for name, other in (("alone", alone), ("remapped", moved),
                        ("max_len", wide)):
        assert np.array_equal(base, other), name


def test_attention_argument_checks(hr):
    import torch

    qt, kt = _tiles(hr)
    L = pr.cache_len_for(qt, kt)
    s = _stream()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((1 << 16,), 0x1234, dtype=torch.int16, device="cuda")
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")

    def call(b=2, c=4, hq=4, hk=2, d=16, max_len=kt, ws_bytes=None,
             cache_len=L):
        if ws_bytes is None:
            ws_bytes = hr.gqa_prefill_attention_workspace_bytes(b, c, hq, d,
                                                                max_len)
        hr.gqa_prefill_attention(
            buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), idx.data_ptr(),
            idx.data_ptr(), idx.data_ptr(), out.data_ptr(), buf.data_ptr(),
            ws_bytes, b, c, hq, hk, d, 1.0, max_len, cache_len, 2, True, s)

    need = hr.gqa_prefill_attention_workspace_bytes(2, 4, 4, 16, kt)
    for bad in (dict(d=24), dict(d=256), dict(hq=3, hk=2), dict(hq=18, hk=2),
                dict(ws_bytes=need - 4), dict(max_len=L + 1),
                dict(max_len=0)):
        with pytest.raises(RuntimeError):
            call(**bad)
    call(b=0)  # returns without a launch
    torch.cuda.synchronize()
    assert (out == 0x1234).all()


# ---------------------------------------------------------------------------
# rope_scatter_prefill_bf16 / rope_scatter_prefill_fp8kv_bf16
# ---------------------------------------------------------------------------


def _decode_reference(hr, qb, kb, vb, cos_d, sin_d, p_abs, cache_len, kv_fp8,
                      q_scale):
    """The decode kernel on tokens qb [n, hq, d], kb/vb [n, hk, d] at
    positions p_abs [n] (all inside the cache). Returns (q bits
    [n, hq, d], K slot [n, hk, d], V slot [n, hk, d])."""
    import torch

    n, hq, d = qb.shape
    hk = kb.shape[1]
    q, _ = _to_dev(qb)
    k, _ = _to_dev(kb)
    v, _ = _to_dev(vb)
    if kv_fp8:
        ck = torch.zeros(n * hk * cache_len * d, dtype=torch.uint8,
                         device="cuda")
        cv = torch.zeros_like(ck)
        fn = hr.rope_scatter_decode_fp8kv_bf16
    else:
        ck, _ = _to_dev(np.zeros((n, hk, cache_len, d), np.uint16))
        cv, _ = _to_dev(np.zeros((n, hk, cache_len, d), np.uint16))
        fn = hr.rope_scatter_decode_bf16
    fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), ck.data_ptr(), cv.data_ptr(),
       cos_d.data_ptr(), sin_d.data_ptr(), _i64(p_abs).data_ptr(), n, hq, hk,
       d, cache_len, q_scale=q_scale, stream_handle=_stream())
    torch.cuda.synchronize()
    rows = np.arange(n)
    slots = [_store_bits(t, kv_fp8).reshape(n, hk, cache_len, d)[rows, :,
                                                                 p_abs]
             for t in (ck, cv)]
    return _bits(q).reshape(n, hq, d), slots[0], slots[1]


def _scatter_case(hr, shape, kv_fp8, pos, lens, row_map, rows, q_scale):
    import torch

    qt, kt = _tiles(hr)
    b, hq, hk, d = shape
    c, L = pr.chunk_for(qt), pr.cache_len_for(qt, kt)
    cos, sin = _rope_tables(d, L)
    cos_d = torch.from_numpy(cos).cuda()
    sin_d = torch.from_numpy(sin).cuda()
    rng = np.random.default_rng(b * 1000 + d + int(kv_fp8))
    qb = _randn_bits(rng, b, c, hq, d)
    kb = _randn_bits(rng, b, c, hk, d)
    vb = _randn_bits(rng, b, c, hk, d)
    what = f"prefill scatter {shape} fp8={kv_fp8} pos={pos} lens={lens}"

    # tokens that write: real, and inside the cache
    ci = np.arange(c)[None, :]
    p_abs = pos[:, None] + ci                               # [b, c]
    live = (ci < lens[:, None]) & (p_abs < L)
    bi, cc = np.nonzero(live)
    want_q, want_k, want_v = _decode_reference(
        hr, qb[bi, cc], kb[bi, cc], vb[bi, cc], cos_d, sin_d, p_abs[bi, cc],
        L, kv_fp8, q_scale)

    # caches pre-filled with random bits (NaN patterns included)
    if kv_fp8:
        before = [rng.integers(0, 256, (rows, hk, L, d), dtype=np.uint8)
                  for _ in range(2)]
        tails = [rng.integers(0, 256, PAD, dtype=np.uint8) for _ in range(2)]
        caches = [torch.from_numpy(np.concatenate([a.reshape(-1), t])).cuda()
                  for a, t in zip(before, tails)]
    else:
        before = [rng.integers(0, 2 ** 16, (rows, hk, L, d), dtype=np.uint16)
                  for _ in range(2)]
        caches, tails = zip(*[_to_dev(a, PAD, 5 + n)
                              for n, a in enumerate(before)])
    q, qtail = _to_dev(qb, PAD, 3)
    k, _ = _to_dev(kb)
    v, _ = _to_dev(vb)
    pos_d, lens_d, map_d = _i64(pos), _i64(lens), _i64(row_map)
    fn = (hr.rope_scatter_prefill_fp8kv_bf16 if kv_fp8
          else hr.rope_scatter_prefill_bf16)
    fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), caches[0].data_ptr(),
       caches[1].data_ptr(), cos_d.data_ptr(), sin_d.data_ptr(),
       pos_d.data_ptr(), lens_d.data_ptr(), map_d.data_ptr(), b, c, hq, hk, d,
       L, rows, q_scale=q_scale, stream_handle=_stream())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(k), kb.reshape(-1)), what + ": k changed"
    assert np.array_equal(_bits(v), vb.reshape(-1)), what + ": v changed"
    assert np.array_equal(pos_d.cpu().numpy(), pos)
    assert np.array_equal(lens_d.cpu().numpy(), lens)
    assert np.array_equal(map_d.cpu().numpy(), row_map)

    got_q = _bits(q)
    assert np.array_equal(got_q[qb.size:], qtail), what + ": q sentinel"
    got_q = got_q[:qb.size].reshape(qb.shape)
    assert np.array_equal(got_q[live], want_q), what + ": q bits"
    assert np.array_equal(got_q[~live], qb[~live]), what + ": skipped q"

    for name, t, tail, old, want in (
            ("ck", caches[0], tails[0], before[0], want_k),
            ("cv", caches[1], tails[1], before[1], want_v)):
        got = _store_bits(t, kv_fp8)
        assert np.array_equal(got[old.size:], tail), f"{what}: {name} sentinel"
        expect = old.copy()
        expect[row_map[bi], :, p_abs[bi, cc]] = want
        bad = got[:old.size].reshape(old.shape) != expect
        assert not bad.any(), (
            f"{what}: {name} differs at {np.argwhere(bad)[:4].tolist()}")
    return int(live.sum()), int((~live).sum())


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
@pytest.mark.parametrize("shape", pr.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_scatter_matches_decode_kernel(hr, shape, kv_fp8):
    """Written positions are bit-identical to the decode kernel's for
    the same token and position, every other cache byte is unchanged,
    and q is unchanged for c >= len; the (pos, lens, row_map) of the
    attention launches."""
    qt, kt = _tiles(hr)
    b, d = shape[0], shape[3]
    launches = pr.launches_for(b, qt, kt)
    for n_map, (row_map, rows) in enumerate(pr.row_maps_for(b)):
        for n in (1, 5, 9):
            pos, lens, _ = launches[n]
            _scatter_case(hr, shape, kv_fp8, pos, lens, row_map, rows,
                          1.0 if n_map else d ** -0.5)


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
def test_scatter_past_cache_writes_nothing(hr, kv_fp8):
    """A row whose positions run past cache_len writes its tokens inside
    the cache and nothing for the others."""
    qt, kt = _tiles(hr)
    L = pr.cache_len_for(qt, kt)
    shape = (3, 8, 2, 128)
    pos = np.array([L - 2, 3, L], dtype=np.int64)
    lens = np.array([5, 2, 4], dtype=np.int64)
    row_map = np.array([2, 0, 1], dtype=np.int64)
    n_live, n_skipped = _scatter_case(hr, shape, kv_fp8, pos, lens, row_map,
                                      3, 128 ** -0.5)
    assert n_live == 2 + 2 and n_skipped == 3 * pr.chunk_for(qt) - 4


def test_scatter_argument_checks(hr):
    import torch

    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    for fn in (hr.rope_scatter_prefill_bf16,
               hr.rope_scatter_prefill_fp8kv_bf16):
        for bad in (dict(d=24), dict(d=8), dict(d=256), dict(cache_len=0),
                    dict(cache_rows=0), dict(hk=0)):
            args = dict(b=2, c=4, hq=4, hk=2, d=16, cache_len=8, cache_rows=2)
            args.update(bad)
            with pytest.raises(RuntimeError):
                fn(p, p, p, p, p, p, p, idx.data_ptr(), idx.data_ptr(),
                   idx.data_ptr(), stream_handle=_stream(), **args)
        with pytest.raises(RuntimeError):  # misaligned q
            fn(p + 2, p, p, p, p, p, p, idx.data_ptr(), idx.data_ptr(),
               idx.data_ptr(), 2, 4, 4, 2, 16, 8, 2,
               stream_handle=_stream())
        fn(p, p, p, p, p, p, p, idx.data_ptr(), idx.data_ptr(),
           idx.data_ptr(), 0, 4, 4, 2, 16, 8, 2, stream_handle=_stream())
    torch.cuda.synchronize()
    assert (buf == 0).all()


# ---------------------------------------------------------------------------
# llama_tiny, bf16, both cache dtypes
# ---------------------------------------------------------------------------

KV_DTYPES = [None, "fp8_e4m3"]


def _tiny_gpu(seed):
    import torch

    from client_amd.models.llama import LlamaModel, llama_tiny_config

    torch.manual_seed(seed)
    cfg = llama_tiny_config()
    return cfg, LlamaModel(cfg).to("cuda:0").to(torch.bfloat16).eval()


@pytest.mark.parametrize("kv_dtype", KV_DTYPES, ids=KV_IDS)
def test_fused_prefill_chunk_matches_torch(hr, kv_dtype):
    """Two chunks per row (the second attends to the first through the
    cache) with the flag on against off: logits within the project's
    fused-vs-fallback tolerance, layer 0's V cache identical up to the
    scratch position, which only the torch path writes."""
    import torch

    cfg, m = _tiny_gpu(21)
    dev = "cuda:0"
    row_map = torch.tensor([2, 0], device=dev)
    chunks = [(torch.tensor([0, 0], device=dev),
               torch.tensor([8, 5], device=dev)),
              (torch.tensor([8, 5], device=dev),
               torch.tensor([3, 8], device=dev))]
    toks = [torch.randint(0, cfg.vocab_size, (2, 8), device=dev)
            for _ in chunks]
    got = {}
    for flag in (False, True):
        m.fused_prefill = flag
        kv = m.make_kv_cache(3, dev, torch.bfloat16, kv_dtype=kv_dtype)
        logits = []
        with torch.inference_mode():
            for t, (pos, lens) in zip(toks, chunks):
                logits.append(m.forward_prefill_chunk(
                    t, pos, lens, lens - 1, kv, 32, row_map=row_map))
        torch.cuda.synchronize()
        got[flag] = (logits, kv)
    for fused, ref in zip(got[True][0], got[False][0]):
        assert torch.isfinite(fused).all()
        torch.testing.assert_close(fused.float(), ref.float(), atol=0.25,
                                   rtol=0.05)
    s = cfg.max_seq
    v_fused, v_ref = got[True][1][0][1], got[False][1][0][1]
    assert torch.equal(v_fused[:, :, :s], v_ref[:, :, :s])
    assert v_fused[:, :, :13].any() and not v_fused[1].any()
    # the two runs took different paths: padded tokens write the scratch
    # position in torch and nothing in the fused kernels
    assert v_ref[:, :, s].any() and not v_fused[:, :, s].any()


def _run(sched, prompt, n, sampling=None):
    q = sched.submit(prompt, n, sampling)
    toks = []
    while True:
        t = q.get(timeout=120)
        if t is sched.END:
            return toks
        toks.append(t)


@pytest.mark.parametrize("kv_dtype", KV_DTYPES, ids=KV_IDS)
def test_fused_prefill_scheduler_graph_matches_eager(hr, kv_dtype):
    from client_amd.server.decode_scheduler import DecodeScheduler

    cfg, m = _tiny_gpu(7)
    m.fused_prefill = True
    prompts = [np.array([5, 17, 200, 31, 8, 99], dtype=np.int64),
               np.arange(3, 40, dtype=np.int64)]
    got = {}
    for use_graph in (False, True):
        sched = DecodeScheduler(m, max_batch=2, device="cuda:0",
                                use_graph=use_graph, len_bucket=32,
                                prefill_chunk=8, kv_dtype=kv_dtype)
        try:
            got[use_graph] = [_run(sched, p, 10) for p in prompts]
            if use_graph:
                assert sched._pf_graphs and all(
                    g is not sched._EAGER for g in sched._pf_graphs.values())
        finally:
            sched.shutdown()
    assert got[True] == got[False]
    assert all(len(t) == 10 for t in got[True])


@pytest.mark.parametrize("kv_dtype", KV_DTYPES, ids=KV_IDS)
def test_fused_prefill_seeded_sampling_independent_of_batch(hr, kv_dtype):
    """A seeded sampled request yields the same tokens alone and
    alongside two other requests."""
    from client_amd.models.sampling import SamplingParams
    from client_amd.server.decode_scheduler import DecodeScheduler

    cfg, m = _tiny_gpu(7)
    m.fused_prefill = True
    prompt = np.arange(60, 81, dtype=np.int64)  # three chunks of 8
    others = [np.arange(3, 50, dtype=np.int64),
              np.array([9, 9, 1], dtype=np.int64)]
    params = SamplingParams(temperature=1.0, top_k=40, top_p=0.95, seed=1234)
    sched = DecodeScheduler(m, max_batch=4, device="cuda:0", use_graph=True,
                            len_bucket=32, prefill_chunk=8,
                            kv_dtype=kv_dtype)
    try:
        alone = _run(sched, prompt, 12, params)
        busy = [sched.submit(others[0], 30),
                sched.submit(others[1], 30, SamplingParams(
                    temperature=0.8, seed=5))]
        first = [q.get(timeout=120) for q in busy]
        shared = _run(sched, prompt, 12, params)
        for q in busy:
            while q.get(timeout=120) is not sched.END:
                pass
        assert len(alone) == 12 and len(first) == 2
        assert shared == alone
    finally:
        sched.shutdown()
