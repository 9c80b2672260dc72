"""The fused prefill path without a GPU: the bound of
tests/prefill_attention_refs.py against the emulation of the kernel's
algorithm on every input the GPU tests use, the extension's exports, the
server flag, and the CPU fallback of LlamaModel.fused_prefill."""

import numpy as np
import pytest
import torch

import attention_refs as ar
import kernel_refs as kr
import prefill_attention_refs as pr

KV = [False, True]
KV_IDS = ["bf16", "fp8"]


def _tiles():
    from client_amd.ops import hip_runtime as hr

    return int(hr.GQA_PREFILL_QTILE), int(hr.GQA_PREFILL_KTILE)


def test_extension_exports():
    from client_amd.ops import hip_runtime as hr

    qt, kt = _tiles()
    assert qt >= 1 and kt >= 1
    for name in ("rope_scatter_prefill_bf16",
                 "rope_scatter_prefill_fp8kv_bf16", "gqa_prefill_attention",
                 "gqa_prefill_attention_workspace_bytes"):
        assert callable(getattr(hr, name)), name
    assert hr.gqa_prefill_attention_workspace_bytes(2, qt + 3, 8, 128,
                                                    4 * kt) >= 0


def test_launches_cover_the_edges():
    qt, kt = _tiles()
    L = pr.cache_len_for(qt, kt)
    for b in (1, 2, 3):
        launches = pr.launches_for(b, qt, kt)
        assert len(launches) == 12
        for slot in range(b):
            assert ({int(p[slot]) for p, _, _ in launches}
                    == set(pr.positions_for(qt, kt)))
            assert ({int(n[slot]) for _, n, _ in launches}
                    == set(pr.lens_for(qt)))
        assert any(ml % kt == 0 for _, _, ml in launches)
        assert all((p + n).max() <= ml <= L - 1 for p, n, ml in launches)


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
@pytest.mark.parametrize("shape", pr.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_emulation_within_bound(shape, kv_fp8):
    """Key tiles, online rescale and the bf16 rounding of P in numpy
    fp32, on the inputs of the GPU tests, stay inside the bound against
    the float64 reference; queries that are not real give zeros."""
    qt, kt = _tiles()
    n_cases = 0
    for q, kp, vp, pos, lens, row_map, max_len, scale in pr.mixed_row_cases(
            shape, qt, kt, kv_fp8):
        got = pr.emulate_prefill(q, kp, vp, pos, lens, row_map, max_len,
                                 scale, kv_fp8, kt)
        r, delta, real = pr.prefill_attention_ref(
            q, kp, vp, pos, lens, row_map, max_len, scale, kv_fp8)
        kr.assert_within_bf16_bound(
            got, r, delta, f"emulation {shape} pos={pos} lens={lens} "
                           f"max_len={max_len}")
        assert np.all(got[~real] == 0)
        assert real.sum() == np.minimum(lens, q.shape[1]).sum()
        n_cases += 1
    assert n_cases == 15


@pytest.mark.parametrize("kv_fp8", KV, ids=KV_IDS)
def test_emulation_softmax_edges(kv_fp8):
    qt, kt = _tiles()
    for name, q, k, v, pos, lens, max_len in pr.softmax_edge_cases(
            qt, kt, kv_fp8):
        row_map = np.arange(q.shape[0])
        got = pr.emulate_prefill(q, k, v, pos, lens, row_map, max_len, 1.0,
                                 kv_fp8, kt)
        r, delta, _ = pr.prefill_attention_ref(q, k, v, pos, lens, row_map,
                                               max_len, 1.0, kv_fp8)
        kr.assert_within_bf16_bound(got, r, delta, f"emulation {name}")


def test_bound_is_decode_bound_plus_p_rounding():
    """For single queries the reference and the bound are those of
    attention_refs.decode_attention_ref with n = the visible keys, plus
    2^-8 A."""
    qt, kt = _tiles()
    shape = (2, 8, 2, 128)
    c, L = pr.chunk_for(qt), pr.cache_len_for(qt, kt)
    q, k, v = pr.random_case(shape, c, L, 2, False, seed=3)
    pos = np.array([kt - 1, 3], dtype=np.int64)
    lens = np.array([c, 5], dtype=np.int64)
    row_map = np.array([1, 0], dtype=np.int64)
    max_len = 2 * kt
    r, delta, real = pr.prefill_attention_ref(q, k, v, pos, lens, row_map,
                                              max_len, 0.5, False)
    for i, ci in ((0, 0), (0, c - 1), (1, 4)):
        assert real[i, ci]
        p1 = np.array([pos[i] + ci], dtype=np.int64)
        rm = row_map[i]
        r1, d1 = ar.decode_attention_ref(q[i:i + 1, ci], k[rm:rm + 1],
                                         v[rm:rm + 1], p1, max_len, 0.5,
                                         False)
        np.testing.assert_allclose(r[i, ci], r1[0], rtol=1e-12, atol=1e-15)
        n = int(ar.row_lengths(p1, max_len)[0])
        vv = np.abs(ar.decode_stored(v[rm, :, :n], False))
        kk = ar.decode_stored(k[rm, :, :n], False)
        for h in range(shape[1]):
            g = h // 4
            s = (kk[g] @ kr.bf16_bits_to_f64(q[i, ci, h])) * 0.5
            p = np.exp(s - s.max())
            p /= p.sum()
            np.testing.assert_allclose(delta[i, ci, h],
                                       d1[0, h] + 2.0 ** -8 * (p @ vv[g]),
                                       rtol=1e-9)
    assert not real[1, 5] and np.all(delta[1, 5] == 0)


def test_server_flag_and_model_config():
    from client_amd.server.__main__ import build_core, build_parser

    parser = build_parser()
    assert parser.parse_args([]).fused_prefill is False
    args = parser.parse_args(["--fused-prefill"])
    assert args.fused_prefill is True

    plain = build_core(["llama_tiny"], device="cpu", dtype="fp32")
    core = build_core(["llama_tiny"], device="cpu", dtype="fp32",
                      fused_prefill=args.fused_prefill)
    try:
        base = plain.models["llama_tiny"]
        assert base.module.fused_prefill is False
        base_cfg = base.config()
        assert "parameters" not in base_cfg
        model = core.models["llama_tiny"]
        assert model.module.fused_prefill is True
        cfg = model.config()
        assert cfg.pop("parameters") == {
            "fused_prefill": {"string_value": "true"}}
        assert cfg == base_cfg
    finally:
        for c in (plain, core):
            sched = c.models["llama_tiny"]._scheduler
            if sched is not None:
                sched.shutdown()


@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"], ids=KV_IDS)
def test_flag_on_cpu_takes_the_fallback(kv_dtype):
    """fused_prefill needs bf16 on a HIP device; anywhere else
    forward_prefill_chunk runs what it ran before, bit for bit."""
    from client_amd.models.llama import LlamaModel, llama_tiny_config

    torch.manual_seed(11)
    cfg = llama_tiny_config()
    m = LlamaModel(cfg).eval()
    assert m.fused_prefill is False
    tokens = torch.randint(0, cfg.vocab_size, (2, 8))
    pos = torch.tensor([0, 5])
    lens = torch.tensor([8, 3])
    last = torch.tensor([7, 2])
    row_map = torch.tensor([2, 0])
    got = {}
    for flag in (False, True):
        m.fused_prefill = flag
        kv = m.make_kv_cache(3, "cpu", torch.float32, kv_dtype=kv_dtype)
        with torch.inference_mode():
            got[flag] = (m.forward_prefill_chunk(tokens, pos, lens, last, kv,
                                                 16, row_map=row_map), kv)
    assert torch.equal(got[True][0], got[False][0])
    for (a, b), (c, d) in zip(got[True][1], got[False][1]):
        assert torch.equal(a, c) and torch.equal(b, d)
