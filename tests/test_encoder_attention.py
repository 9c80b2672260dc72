"""The BERT attention mask without a GPU: the bound of
tests/encoder_attention_refs.py against the emulation of the kernel's
algorithm on every input the GPU tests use, the masked model on the
torch path, the served optional input, and the batcher's grouping of
requests by shape."""

import threading

import numpy as np
import pytest
import torch

import encoder_attention_refs as er
import kernel_refs as kr

QT = KT = 32  # the CPU checks use these tiles, whatever the kernel's


def test_extension_exports():
    from client_amd.ops import hip_runtime as hr

    assert callable(hr.encoder_attention)
    qt, kt = int(hr.ENCODER_ATTN_QTILE), int(hr.ENCODER_ATTN_KTILE)
    ks = int(getattr(hr, "ENCODER_ATTN_KSTAGE", kt))
    assert qt >= 1 and kt >= 1 and ks % kt == 0
    # the BERT-large serving shape fills the 256 CUs
    assert -(-128 // qt) * 16 * 8 >= 256


def test_cases_cover_the_edges():
    for b in (2, 3):
        for s in er.seq_lens_for(QT, KT, KT):
            launches = er.launches_for(b, s, KT)
            for slot in range(b):
                assert ({int(n[slot]) for n in launches}
                        == set(er.kv_lens_for(s, KT)))
    s = 2 * KT + QT + 5
    for pattern in er.PATTERNS:
        for n in er.kv_lens_for(s, KT):
            m = er.mask_row(pattern, s, n, KT)
            last = int(np.nonzero(m)[0].max()) + 1 if m.any() else 0
            assert last == n, (pattern, n)
    tile = er.mask_row("tile", s, s, KT)
    assert tile[:KT].all() and not tile[KT:2 * KT].any() and tile[2 * KT:].all()
    assert len(er.seq_lens_for(QT, KT, 4 * KT)) == 4


@pytest.mark.parametrize("shape", er.SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_emulation_within_bound(shape):
    """Key tiles, masked keys at -inf, online rescale and the bf16
    rounding of P in numpy fp32, on the inputs of the GPU tests, stay
    inside the bound against the float64 reference; queries at or past
    kv_len give zeros; a row's bits do not change when S is cut to its
    kv_len."""
    n_cases = 0
    for qkv, mask, kv_len, scale in er.cases(shape, QT, KT, KT):
        got = er.emulate_encoder(qkv, mask, kv_len, scale, KT)
        r, delta, real = er.encoder_attention_ref(qkv, mask, kv_len, scale)
        kr.assert_within_bf16_bound(
            got, r, delta, f"emulation {shape} S={qkv.shape[1]} "
                           f"kv_len={kv_len}")
        assert np.all(got[~real] == 0)
        assert real.sum() == kv_len.sum()
        for i, n in enumerate(kv_len):
            n = int(n)
            if 0 < n < qkv.shape[1]:
                cut = er.emulate_encoder(qkv[i:i + 1, :n], mask[i:i + 1, :n],
                                         kv_len[i:i + 1], scale, KT)
                assert np.array_equal(cut[0], got[i, :n])
        n_cases += 1
    assert n_cases == 3 * 6 * 4


def test_emulation_softmax_edges_and_no_visible_key():
    for name, qkv, mask, kv_len in er.softmax_edge_cases(KT):
        got = er.emulate_encoder(qkv, mask, kv_len, 1.0, KT)
        r, delta, _ = er.encoder_attention_ref(qkv, mask, kv_len, 1.0)
        kr.assert_within_bf16_bound(got, r, delta, f"emulation {name}")
    qkv = er.random_case((1, 2, 64), 5)
    mask = np.zeros((1, 5), dtype=np.uint8)
    kv_len = np.array([5], dtype=np.int32)
    assert not er.emulate_encoder(qkv, mask, kv_len, 1.0, KT).any()
    r, delta, real = er.encoder_attention_ref(qkv, mask, kv_len, 1.0)
    assert real.all() and not r.any() and not delta.any()


# ---------------------------------------------------------------------------
# bert_tiny, fp32 on the CPU
# ---------------------------------------------------------------------------

LENS = (40, 17, 1)
WIDTH = 40


def tiny_batch(seed=3):
    """ids [3, 40] and mask for rows of 40, 17 and 1 real tokens."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 128, (len(LENS), WIDTH), generator=g)
    mask = torch.zeros(len(LENS), WIDTH, dtype=torch.int64)
    for i, n in enumerate(LENS):
        mask[i, :n] = 1
    return ids, mask


def _tiny(seed=0):
    from client_amd.models.bert import bert_tiny

    torch.manual_seed(seed)
    return bert_tiny().eval()


def test_model_mask_is_padding_invariant():
    m = _tiny()
    ids, mask = tiny_batch()
    with torch.inference_mode():
        pooled = m(ids, mask)
        hidden = m.hidden_states(ids, mask)
        assert torch.isfinite(pooled).all()
        for i, n in enumerate(LENS):
            assert torch.isfinite(hidden[i, :n]).all()
            alone = m(ids[i:i + 1, :n])
            alone_hidden = m.hidden_states(ids[i:i + 1, :n])
            torch.testing.assert_close(pooled[i:i + 1], alone)
            torch.testing.assert_close(hidden[i:i + 1, :n], alone_hidden)
        # bool and int32 masks are the same mask
        assert torch.equal(m(ids, mask.bool()), pooled)
        assert torch.equal(m(ids, mask.to(torch.int32) * 7), pooled)


def test_model_without_mask_is_unchanged():
    m = _tiny()
    ids, _ = tiny_batch()
    with torch.inference_mode():
        assert torch.equal(m(ids), m(ids, None))
        assert torch.equal(m(ids), m(ids, attention_mask=None))
        # what the parent computed: the layers called with x alone
        x = m.ln(m.tok(ids) + m.pos(torch.arange(WIDTH))[None])
        for layer in m.layers:
            a, _ = layer.attn(x, x, x, need_weights=False)
            x = layer.ln1(x + a)
            x = layer.ln2(x + layer.fc2(layer.act(layer.fc1(x))))
        assert torch.equal(m(ids), torch.tanh(m.pooler(x[:, 0])))


def test_model_ignores_ids_at_masked_positions():
    m = _tiny()
    ids, mask = tiny_batch()
    other = ids.clone()
    other[mask == 0] = (other[mask == 0] + 61) % 128
    assert not torch.equal(other, ids)
    with torch.inference_mode():
        assert torch.equal(m(ids, mask), m(other, mask))


def test_model_mask_with_holes_and_masked_first_token_is_finite():
    m = _tiny()
    ids, mask = tiny_batch()
    mask[0, 5:9] = 0
    mask[1, 0] = 0
    with torch.inference_mode():
        assert torch.isfinite(m(ids, mask)).all()


def test_fused_flag_on_cpu_takes_the_torch_path(monkeypatch):
    from client_amd.models.bert import bert_tiny

    m = _tiny()
    assert m.fused_attention is False
    ids, mask = tiny_batch()
    with torch.inference_mode():
        want = m(ids, mask)
        m.fused_attention = True
        assert torch.equal(m(ids, mask), want)
    monkeypatch.setenv("CLIENT_AMD_BERT_FUSED_ATTN", "1")
    assert bert_tiny().fused_attention is True


def test_seeded_weights_are_unchanged():
    """The mask adds no parameter and draws no random number: the state
    dict has the parent's names and a seeded model the same first and
    last weights as a bare module list built in the same order."""
    m = _tiny(5)
    names = list(m.state_dict())
    assert names[:4] == ["tok.weight", "pos.weight", "ln.weight", "ln.bias"]
    assert "layers.0.attn.in_proj_weight" in names
    assert names[-2:] == ["pooler.weight", "pooler.bias"]
    assert len(names) == 4 + 2 * 12 + 2
    torch.manual_seed(5)
    tok = torch.nn.Embedding(128, 32)
    assert torch.equal(tok.weight, m.tok.weight)


# ---------------------------------------------------------------------------
# served over gRPC on the CPU
# ---------------------------------------------------------------------------


def test_bert_tiny_served_with_optional_mask():
    import client_amd.grpc as grpcclient
    from client_amd.server.__main__ import build_core, build_parser
    from client_amd.server.grpc_server import GrpcServer

    parser = build_parser()
    assert parser.parse_args([]).bert_fused_attention is False
    assert parser.parse_args(
        ["--bert-fused-attention"]).bert_fused_attention is True

    core = build_core(["bert_tiny"], device="cpu", dtype="fp32")
    model = core.models["bert_tiny"]
    cfg = model.config()
    assert [(i["name"], i.get("optional", False)) for i in cfg["input"]] == [
        ("input_ids", False), ("attention_mask", True)]
    assert "parameters" not in cfg
    fused = build_core(["bert_tiny"], device="cpu", dtype="fp32",
                       bert_fused_attention=True).models["bert_tiny"]
    assert fused.module.fused_attention is True
    assert fused.config()["parameters"] == {
        "fused_attention": {"string_value": "true"}}

    ids, mask = tiny_batch()
    ids, mask = ids.numpy(), mask.numpy()
    server = GrpcServer(core, host="127.0.0.1", port=0)
    server.start()
    try:
        client = grpcclient.InferenceServerClient(f"127.0.0.1:{server.port}")

        def infer(ids, mask=None, mask_first=False):
            inputs = [grpcclient.InferInput("input_ids", list(ids.shape),
                                            "INT64")]
            inputs[0].set_data_from_numpy(ids)
            if mask is not None:
                inp = grpcclient.InferInput("attention_mask",
                                            list(mask.shape), "INT64")
                inp.set_data_from_numpy(mask)
                inputs.insert(0 if mask_first else 1, inp)
            return client.infer("bert_tiny", inputs).as_numpy("pooled")

        plain = infer(ids)
        assert plain.shape == (3, 32) and np.isfinite(plain).all()
        with torch.inference_mode():
            want = model.module(torch.from_numpy(ids)).numpy()
        np.testing.assert_array_equal(plain, want)

        masked = infer(ids, mask)
        assert masked.shape == (3, 32) and np.isfinite(masked).all()
        # the request's order of inputs does not matter
        np.testing.assert_array_equal(infer(ids, mask, mask_first=True),
                                      masked)
        for i, n in enumerate(LENS):
            alone = infer(np.ascontiguousarray(ids[i:i + 1, :n]))
            torch.testing.assert_close(torch.tensor(masked[i:i + 1]),
                                       torch.tensor(alone))
        assert not np.array_equal(masked[1], plain[1])

        config = client.get_model_config("bert_tiny").config
        assert [(i.name, i.optional) for i in config.input] == [
            ("input_ids", False), ("attention_mask", True)]

        # the load generator sends an optional input only when asked to:
        # a BERT run is the workload it was
        from client_amd.perf.analyzer import PerfAnalyzer

        url = f"127.0.0.1:{server.port}"
        pa = PerfAnalyzer(url, model_name="bert_tiny", batch_size=2,
                          shapes={"input_ids": [24]})
        assert pa._model_io(client)[0] == [("input_ids", "INT64", [2, 24])]
        pa = PerfAnalyzer(url, model_name="bert_tiny", batch_size=2,
                          shapes={"input_ids": [24],
                                  "attention_mask": [24]})
        assert pa._model_io(client)[0] == [
            ("input_ids", "INT64", [2, 24]),
            ("attention_mask", "INT64", [2, 24])]

        with pytest.raises(Exception, match="input_ids"):
            inp = grpcclient.InferInput("attention_mask", list(mask.shape),
                                        "INT64")
            inp.set_data_from_numpy(mask)
            client.infer("bert_tiny", [inp])
        client.close()
    finally:
        server.stop(grace=1)


# ---------------------------------------------------------------------------
# dynamic batcher
# ---------------------------------------------------------------------------


class _FakeModel:
    """Records the batch shapes it is called with; the first call waits
    for `gate`, so the test can queue further items behind it."""

    def __init__(self):
        self.calls = []
        self.gate = threading.Event()
        self.entered = threading.Event()

    def _execute_direct(self, tensors):
        self.calls.append([tuple(t.shape) for t in tensors])
        if len(self.calls) == 1:
            self.entered.set()
            assert self.gate.wait(timeout=30)
        return [tensors[0].float().sum(dim=1, keepdim=True)]


def _batched(shapes):
    """Queues one item per shape behind a blocked first call; returns
    (model, per-item outputs, inputs)."""
    from client_amd.server.batcher import DynamicBatcher

    model = _FakeModel()
    batcher = DynamicBatcher(model, preferred_batch_size=8,
                             max_queue_delay_us=2000, max_batch_size=8)
    results, errors = {}, {}

    def submit(key, t):
        try:
            results[key] = batcher.infer([t])
        except Exception as e:  # reported by the caller
            errors[key] = e

    try:
        blocker = torch.ones(8, 3, dtype=torch.int64)  # a full batch
        ins = [torch.arange(s[0] * s[1]).reshape(s) for s in shapes]
        threads = [threading.Thread(target=submit, args=("first", blocker))]
        threads[0].start()
        assert model.entered.wait(timeout=30)
        for n, t in enumerate(ins):
            th = threading.Thread(target=submit, args=(n, t))
            th.start()
            threads.append(th)
            # queued in this order (the worker is inside the first call,
            # so the notify of each append wakes this wait)
            with batcher._cv:
                assert batcher._cv.wait_for(
                    lambda: len(batcher._queue) >= n + 1, timeout=30)
        model.gate.set()
        for th in threads:
            th.join(timeout=30)
    finally:
        batcher.shutdown()
    assert not errors, errors
    return model, results, ins


def test_batcher_runs_different_shapes_as_separate_batches():
    model, results, ins = _batched([(2, 5), (1, 9)])
    assert model.calls[1:] == [[(2, 5)], [(1, 9)]]
    for n, t in enumerate(ins):
        assert torch.equal(results[n][0], t.float().sum(dim=1, keepdim=True))


def test_batcher_still_merges_equal_shapes():
    model, results, ins = _batched([(2, 5), (1, 5)])
    assert model.calls[1:] == [[(3, 5)]]
    for n, t in enumerate(ins):
        assert torch.equal(results[n][0], t.float().sum(dim=1, keepdim=True))
