"""The sample_logits_bf16 kernel against the float64 contract in
tests/sampling_refs.py (requires an MI355X).

Exact properties (greedy, top_k=1, tiny top_p, membership in the
tie-inclusive top-k set, sentinels, untouched inputs, independence of the
row index and the batch) are asserted without tolerance. A sampled
token is checked by the acceptance rule of sampling_refs with its
derived eps; before the kernel's output is read, the reference alone
must show that at most 20 % of a case's rows admit more than one token
(the flat case, where neighbours legitimately tie, is exempt).
"""

import numpy as np
import pytest

import sampling_refs as sr

pytestmark = pytest.mark.gpu

PAD = 64  # sentinel elements behind the output
SENTINEL = -0x5A5A5A5A5A5A5A5B

SHAPES = [(1, 1), (3, 7), (8, 8), (5, 255), (8, 256), (3, 1000), (2, 4104),
          (8, 128256)]

# (temperature, top_k, top_p), all at T <= 1
CONFIGS = [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 5, 1.0), (0.5, 0, 0.5),
           (1.0, 3, 0.8), (0.8, 0, 0.95), (1.0, 1000, 0.99), (0.3, 40, 1.0)]
# seeds and steps that use the high halves of both 64-bit words
SEEDS = [1000, 2 ** 63 + 12345, 2 ** 64 - 1, 1003, 7, 2 ** 32 + 1, 1006, 0]
STEPS = [0, 1, 2 ** 32 + 7, 5, 2 ** 40, 3, 9, 2 ** 31]

HAND_ROW = [0.0, 1.0, 2.0, 3.0, -1.0, 2.5, -8.0, 0.5]
HAND_CASES = [(0.05, 3), (0.3, 3), (0.55, 3), (0.8, 5), (0.97, 5)]


@pytest.fixture(scope="module")
def gpu():
    from client_amd.ops import gpu_available

    if not gpu_available():
        pytest.skip("no HIP device")
    import torch

    return torch


def _values(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


_LOGITS = {}


def _logits(rows, vocab, seed=0):
    """4 * N(0, 1) rounded to bf16: (float32 values, uint16 bits)."""
    key = (rows, vocab, seed)
    if key not in _LOGITS:
        rng = np.random.default_rng(1234 + 7919 * seed + vocab)
        _LOGITS[key] = sr.bf16_round(4.0 * rng.standard_normal((rows, vocab)))
    vals, bits = _LOGITS[key]
    return vals.copy(), bits.copy()


def _run(torch, bits, temperature, top_k, top_p, seeds, steps):
    """One launch through sample_tokens. Checks the sentinel behind the
    output and that no input changed; returns the tokens."""
    from client_amd.models.sampling import sample_tokens, seed_to_i64

    rows, vocab = bits.shape
    host = [
        torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)),
        torch.tensor(temperature, dtype=torch.float32),
        torch.tensor(top_k, dtype=torch.int32),
        torch.tensor(top_p, dtype=torch.float32),
        torch.tensor([seed_to_i64(s) for s in seeds], dtype=torch.int64),
        torch.tensor([seed_to_i64(s) for s in steps], dtype=torch.int64),
    ]
    dev = [t.cuda() for t in host]
    logits = dev[0].view(torch.bfloat16)
    buf = torch.full((rows + PAD,), SENTINEL, dtype=torch.int64,
                     device="cuda")
    out = sample_tokens(logits, *dev[1:], out=buf[:rows])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert (got[rows:] == SENTINEL).all(), "wrote past the output"
    for name, d, h in zip(("logits", "temperature", "top_k", "top_p",
                           "seed", "step"), dev, host):
        assert torch.equal(d.cpu(), h), f"{name} changed"
    tokens = got[:rows]
    assert ((tokens >= 0) & (tokens < vocab)).all(), tokens
    return tokens


def _row_params(rows, offset):
    cfg = [CONFIGS[(i + offset) % len(CONFIGS)] for i in range(rows)]
    return ([c[0] for c in cfg], [c[1] for c in cfg], [c[2] for c in cfg],
            [SEEDS[(i + offset) % 8] for i in range(rows)],
            [STEPS[(i + 3 * offset) % 8] for i in range(rows)])


def _check_accepted(vals, tokens, temperature, top_k, top_p, seeds, steps,
                    cap):
    """The acceptance rule per row; with ``cap``, first the reference's
    own 20 % bound on ambiguous rows."""
    rows, vocab = vals.shape
    eps = sr.eps_for(vocab)
    sets = [sr.acceptable(vals[r], temperature[r], top_k[r], top_p[r],
                          float(sr.uniform(seeds[r], steps[r])), eps)
            for r in range(rows)]
    if cap:
        ambiguous = sum(len(s) > 1 for s in sets)
        assert ambiguous <= 0.2 * rows, (
            f"{ambiguous} of {rows} rows admit several tokens: pick "
            "another seed for this case")
    for r in range(rows):
        assert len(sets[r]) >= 1
        assert tokens[r] in sets[r], (
            f"row {r}: token {tokens[r]} not in {sets[r][:8]} "
            f"(T={temperature[r]}, k={top_k[r]}, p={top_p[r]})")
        assert sr.topk_mask(vals[r], top_k[r])[tokens[r]]


@pytest.mark.parametrize("shape_idx", range(len(SHAPES)),
                         ids=[f"{r}x{v}" for r, v in SHAPES])
def test_sampled_token_is_accepted(gpu, shape_idx):
    rows, vocab = SHAPES[shape_idx]
    vals, bits = _logits(rows, vocab)
    params = _row_params(rows, shape_idx)
    tokens = _run(gpu, bits, *params)
    _check_accepted(vals, tokens, *params, cap=True)


def test_flat_distribution(gpu):
    """T = 1.5 without truncation over the real vocabulary: many
    neighbours are legitimately acceptable, so only the interval rule
    applies."""
    rows, vocab = 8, 128256
    vals, bits = _logits(rows, vocab, seed=1)
    params = ([1.5] * rows, [0] * rows, [1.0] * rows, SEEDS, STEPS)
    tokens = _run(gpu, bits, *params)
    _check_accepted(vals, tokens, *params, cap=False)


@pytest.mark.parametrize("shape_idx", range(len(SHAPES)),
                         ids=[f"{r}x{v}" for r, v in SHAPES])
def test_exact_properties(gpu, shape_idx):
    rows, vocab = SHAPES[shape_idx]
    vals, bits = _logits(rows, vocab, seed=2)
    # a second copy of each row's maximum: before it in odd rows, behind
    # it in even rows, so "lowest index" is not always the first found
    for r in range(rows):
        first = int(np.argmax(vals[r]))
        other = (first // 2) if r % 2 else min(vocab - 1, first + 1 + r)
        bits[r, other] = bits[r, first]
    vals = _values(bits)
    expect = np.array([sr.greedy(vals[r]) for r in range(rows)])
    zeros, ones = [0.0] * rows, [1.0] * rows
    seeds, steps = SEEDS[:rows], STEPS[:rows]

    # temperature 0, whatever the other parameters say
    got = _run(gpu, bits, zeros, [3] * rows, [0.5] * rows, seeds, steps)
    assert (got == expect).all()
    vmax = vals.max(axis=1)
    for seed_shift in (0, 1):
        s = [x ^ seed_shift for x in seeds]
        # top_k = 1 keeps the maximum alone (all its copies: ties stay)
        got = _run(gpu, bits, ones, [1] * rows, ones, s, steps)
        assert (vals[np.arange(rows), got] == vmax).all()
        # top_p = 1e-6 is reached by the largest distinct value at once
        got = _run(gpu, bits, [0.9] * rows, [0] * rows, [1e-6] * rows, s,
                   steps)
        assert (vals[np.arange(rows), got] == vmax).all()
    # and with a unique maximum top_k = 1 is the argmax itself
    vals1, bits1 = _logits(rows, vocab, seed=3)
    unique = [r for r in range(rows)
              if (vals1[r] == vals1[r].max()).sum() == 1]
    got = _run(gpu, bits1, ones, [1] * rows, ones, seeds, steps)
    for r in unique:
        assert got[r] == int(np.argmax(vals1[r]))


def test_hand_built_row(gpu):
    """[0, 1, 2, 3, -1, 2.5, -8, 0.5], top_k=3, top_p=0.8, T=1: token 3
    for u < 0.6225, else token 5."""
    eps = sr.eps_for(len(HAND_ROW))
    seeds = [sr.find_seed(u, step=4) for u, _ in HAND_CASES]
    n = len(seeds)
    for seed, (_, expected) in zip(seeds, HAND_CASES):
        ok = sr.acceptable(HAND_ROW, 1.0, 3, 0.8,
                           float(sr.uniform(seed, 4)), eps)
        assert list(ok) == [expected]
    _, bits = sr.bf16_round(np.tile(np.float32(HAND_ROW), (n, 1)))
    got = _run(gpu, bits, [1.0] * n, [3] * n, [0.8] * n, seeds, [4] * n)
    assert got.tolist() == [e for _, e in HAND_CASES]


def test_ties_nan_inf_rows(gpu):
    """Ties across the top-k cut; NaN (several payloads) reads as -inf,
    +inf as the largest finite value, -0 equals +0; rows with nothing
    finite yield token 0."""
    def b(x):
        return int(sr.bf16_round(np.float32([x]))[1][0])

    NAN1, NAN2, NAN3 = 0x7FC0, 0xFFC1, 0x7F81
    PINF, NINF, NZERO = 0x7F80, 0xFF80, 0x8000
    rows = np.array([
        [b(1), b(2), b(2), b(.5), b(2), b(3), b(-1), b(0)],
        [NAN1, b(1), NAN2, b(4), NINF, b(0), b(4), NAN3],
        [b(0), PINF, b(1), b(2), b(3), NINF, PINF, b(1)],
        [NINF] * 8,
        [NAN1, NINF, NAN2, NINF, NAN3, NINF, NAN1, NAN2],
        [NZERO, b(0), b(-1), NZERO, b(-2), b(0), b(-1), b(-3)],
        [NAN2, NAN1, b(-3), NINF, b(-3), NAN3, NINF, NAN1],
    ], dtype=np.uint16)
    vals = _values(rows)
    temperature = [1.0, 0.8, 1.0, 1.0, 0.0, 1.0, 0.6]
    top_k = [2, 0, 0, 3, 0, 1, 0]
    top_p = [1.0, 0.9, 1.0, 0.5, 1.0, 1.0, 1.0]
    n = len(rows)
    eps = sr.eps_for(8)
    allowed = [(1, 2, 4, 5), (3, 6), (1, 6), (0,), (0,), (0, 1, 3, 5),
               (2, 4)]
    for seed in range(8):
        seeds, steps = [seed] * n, [seed + 1] * n
        got = _run(gpu, rows, temperature, top_k, top_p, seeds, steps)
        u = float(sr.uniform(seed, seed + 1))
        for r in range(n):
            assert got[r] in allowed[r], (r, got[r])
            assert got[r] in sr.acceptable(vals[r], temperature[r], top_k[r],
                                           top_p[r], u, eps)
    # temperature 0: lowest index of the maximum (-0 and +0 tie)
    got = _run(gpu, rows, [0.0] * n, top_k, top_p, [3] * n, [0] * n)
    assert got.tolist() == [5, 3, 1, 0, 0, 0, 2]


@pytest.mark.parametrize("vocab", [7, 255, 1000])
def test_row_independence(gpu, vocab):
    """The same (row, parameters, seed, step) gives the same token at any
    row index and in batches of 1, 3 and 8. With vocab 7 the row's
    alignment changes with its index too."""
    vals, bits = _logits(8, vocab, seed=4)
    t, k, p, seeds, steps = _row_params(8, 5)

    def run(order):
        return _run(gpu, bits[order], [t[i] for i in order],
                    [k[i] for i in order], [p[i] for i in order],
                    [seeds[i] for i in order], [steps[i] for i in order])

    base = run(list(range(8)))
    perm = [7, 6, 5, 4, 3, 2, 1, 0]
    assert (run(perm) == base[perm]).all()
    perm = [3, 0, 6, 1, 7, 5, 2, 4]
    assert (run(perm) == base[perm]).all()
    for order in ([5, 0, 2], [1, 7, 4], [7], [3], [0]):
        assert (run(order) == base[order]).all()


def test_graph_capture_replays_follow_the_step_tensor(gpu):
    """One captured launch, replayed after changing only the device step
    tensor, equals the eager result for that step."""
    torch = gpu
    from client_amd.models.sampling import sample_tokens, seed_to_i64

    rows, vocab = 8, 1000
    _, bits = _logits(rows, vocab, seed=5)
    logits = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    temperature = torch.full((rows,), 1.0, device="cuda")
    top_k = torch.zeros(rows, dtype=torch.int32, device="cuda")
    top_p = torch.ones(rows, device="cuda")
    seed = torch.tensor([seed_to_i64(s) for s in SEEDS], device="cuda")
    step = torch.zeros(rows, dtype=torch.int64, device="cuda")
    args = (logits, temperature, top_k, top_p, seed, step)

    eager = {}
    for s in (1, 2, 3):
        step.fill_(s)
        eager[s] = sample_tokens(*args).cpu().tolist()
    assert len({tuple(v) for v in eager.values()}) == 3, (
        "different steps must differ somewhere across 8 rows")

    step.fill_(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sample_tokens(*args)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = sample_tokens(*args)
    for s in (3, 1, 2):
        step.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().tolist() == eager[s]


def test_scheduler_graph_mode_seeded_sampling(gpu):
    """llama_tiny in bf16 with captured graphs: a seeded sampled request
    reproduces, and a greedy request before and after it is unchanged."""
    torch = gpu
    from client_amd.models.llama import LlamaModel, llama_tiny_config
    from client_amd.models.sampling import SamplingParams
    from client_amd.server.decode_scheduler import DecodeScheduler

    torch.manual_seed(7)
    cfg = llama_tiny_config()
    model = LlamaModel(cfg).to("cuda:0").to(torch.bfloat16).eval()
    prompt = np.array([5, 17, 200, 31, 8, 99], dtype=np.int64)
    sched = DecodeScheduler(model, max_batch=2, device="cuda:0",
                            use_graph=True, len_bucket=32)

    def run(sampling=None):
        q = sched.submit(prompt, 10, sampling)
        toks = []
        while True:
            t = q.get(timeout=120)
            if t is sched.END:
                return toks
            toks.append(t)

    try:
        params = SamplingParams(temperature=1.0, top_k=40, top_p=0.95,
                                seed=2 ** 63 + 9)
        before = run()
        first = run(params)
        second = run(params)
        after = run()
        assert len(before) == len(first) == 10
        assert first == second
        assert before == after
        # greedy and sampled steps live in separate cache entries, and the
        # sampled ones were captured, not run eager
        assert 32 in sched._graphs and (32, True) in sched._graphs
        assert sched._graphs[(32, True)] is not sched._EAGER
        assert sched._pf_graphs[(1, 32, True)] is not sched._EAGER
    finally:
        sched.shutdown()
