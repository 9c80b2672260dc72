"""HIP shared-memory + CDNA4 kernel tests (require an MI355X).

GPU tier of SURVEY.md §4: ports of the reference
tests/test_cuda_shared_memory.py plus numerics checks of the CDNA4
cast/pack/preprocess kernels against plain fp32 numpy references.
"""

import multiprocessing as mp

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipshm():
    import client_amd.utils.hip_shared_memory as hipshm

    from client_amd.ops import gpu_available

    if not gpu_available():
        pytest.skip("no HIP device")
    return hipshm


def test_create_destroy(hipshm):
    h = hipshm.create_shared_memory_region("r0", 4096, 0)
    assert ("r0", 4096, 0) in hipshm.allocated_shared_memory_regions()
    hipshm.destroy_shared_memory_region(h)
    assert ("r0", 4096, 0) not in hipshm.allocated_shared_memory_regions()


def test_raw_handle(hipshm):
    import base64

    h = hipshm.create_shared_memory_region("r1", 4096, 0)
    try:
        b64 = hipshm.get_raw_handle(h)
        raw = base64.b64decode(b64)
        assert len(raw) == 64  # hipIpcMemHandle_t is 64 bytes
        assert hipshm.get_raw_handle_bytes(h) == raw
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_numpy_roundtrip(hipshm):
    h = hipshm.create_shared_memory_region("r2", 1 << 20, 0)
    try:
        x = np.random.rand(13, 7).astype(np.float32)
        y = np.arange(11, dtype=np.int64)
        hipshm.set_shared_memory_region(h, [x, y])
        out_x = hipshm.get_contents_as_numpy(h, np.float32, [13, 7])
        out_y = hipshm.get_contents_as_numpy(h, np.int64, [11], offset=x.nbytes)
        np.testing.assert_array_equal(out_x, x)
        np.testing.assert_array_equal(out_y, y)
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_bytes_roundtrip(hipshm):
    h = hipshm.create_shared_memory_region("r3", 1 << 16, 0)
    try:
        s = np.array([b"hip", b"", b"\xff\x00shm"], dtype=np.object_)
        hipshm.set_shared_memory_region(h, [s])
        out = hipshm.get_contents_as_numpy(h, np.object_, [3])
        np.testing.assert_array_equal(out, s)
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_cast_bf16_wire_exact(hipshm):
    """Device pack kernel must be byte-exact with the CPU wire codec
    (truncation semantics, reference utils/__init__.py:294-330)."""
    from client_amd.utils import deserialize_bf16_tensor, serialize_bf16_tensor

    n = 1 << 20
    x = (np.random.randn(n) * 100).astype(np.float32)
    h = hipshm.create_shared_memory_region("r4", n * 2, 0)
    try:
        nbytes = hipshm.set_shared_memory_region_cast(h, x, "BF16")
        assert nbytes == n * 2
        raw = hipshm.get_contents_as_numpy(h, np.uint8, [n * 2])
        wire = serialize_bf16_tensor(x).item()
        np.testing.assert_array_equal(raw, np.frombuffer(wire, np.uint8))
        # device unpack matches CPU deserialize
        back = hipshm.get_contents_cast(h, "BF16", [n])
        np.testing.assert_array_equal(back, deserialize_bf16_tensor(wire))
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_cast_bf16_odd_sizes(hipshm):
    from client_amd.utils import serialize_bf16_tensor

    for n in (1, 7, 8, 9, 255, 1000003):
        x = np.random.randn(n).astype(np.float32)
        h = hipshm.create_shared_memory_region("r5", max(n * 2, 16), 0)
        try:
            hipshm.set_shared_memory_region_cast(h, x, "BF16")
            raw = hipshm.get_contents_as_numpy(h, np.uint8, [n * 2])
            np.testing.assert_array_equal(
                raw,
                np.frombuffer(serialize_bf16_tensor(x).item(), np.uint8),
                err_msg=f"n={n}",
            )
        finally:
            hipshm.destroy_shared_memory_region(h)


def test_cast_fp8_roundtrip(hipshm):
    """fp8 e4m3 (OCP fn): verify against torch's float8_e4m3fn cast."""
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("torch has no float8_e4m3fn")
    n = 1 << 16
    x = (np.random.randn(n) * 4).astype(np.float32)
    h = hipshm.create_shared_memory_region("r6", n * 4, 0)
    try:
        hipshm.set_shared_memory_region_cast(h, x, "FP8E4M3")
        raw = hipshm.get_contents_as_numpy(h, np.uint8, [n])
        expected = (
            torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        )
        np.testing.assert_array_equal(raw, expected)
        back = hipshm.get_contents_cast(h, "FP8E4M3", [n])
        expected_f = torch.from_numpy(x).to(torch.float8_e4m3fn).float().numpy()
        np.testing.assert_array_equal(back, expected_f)
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_dlpack_from_torch(hipshm):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch GPU")
    x = torch.randn(64, 32, device="cuda:0")
    h = hipshm.create_shared_memory_region("r7", x.numel() * 4, 0)
    try:
        hipshm.set_shared_memory_region_from_dlpack(h, [x])
        out = hipshm.get_contents_as_numpy(h, np.float32, [64, 32])
        np.testing.assert_array_equal(out, x.cpu().numpy())
        # non-contiguous device tensor -> gather_pack kernel path
        xt = x.t()  # strided view (32, 64)
        hipshm.set_shared_memory_region_from_dlpack(h, [xt])
        out = hipshm.get_contents_as_numpy(h, np.float32, [32, 64])
        np.testing.assert_array_equal(out, x.t().cpu().numpy())
        # host tensor path
        xc = torch.randn(16, 16)
        hipshm.set_shared_memory_region_from_dlpack(h, [xc])
        out = hipshm.get_contents_as_numpy(h, np.float32, [16, 16])
        np.testing.assert_array_equal(out, xc.numpy())
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_dlpack_export_zero_copy(hipshm):
    """Region exported as DLPack (kDLROCM) wraps into torch with no copy."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch GPU")
    h = hipshm.create_shared_memory_region("r8", 1024 * 4, 0)
    try:
        smt = hipshm.as_shared_memory_tensor(h, "FP32", [1024])
        t = torch.from_dlpack(smt)
        assert t.is_cuda and t.shape == (1024,)
        t.fill_(3.5)
        torch.cuda.synchronize()
        out = hipshm.get_contents_as_numpy(h, np.float32, [1024])
        np.testing.assert_array_equal(out, np.full(1024, 3.5, np.float32))
    finally:
        hipshm.destroy_shared_memory_region(h)


def _ref_preprocess(img, oh, ow, mode, mean, std):
    """numpy reference of the kernel's pixel-center bilinear + normalize."""
    ih, iw, _ = img.shape
    out = np.empty((3, oh, ow), dtype=np.float32)
    sy, sx = ih / oh, iw / ow
    fy = (np.arange(oh) + 0.5) * sy - 0.5
    fx = (np.arange(ow) + 0.5) * sx - 0.5
    y0 = np.minimum(np.maximum(0, np.floor(fy).astype(int)), ih - 1)
    x0 = np.minimum(np.maximum(0, np.floor(fx).astype(int)), iw - 1)
    y1 = np.minimum(ih - 1, y0 + 1)
    x1 = np.minimum(iw - 1, x0 + 1)
    wy = np.where(fy < 0, 0.0, fy - np.floor(fy))[:, None]
    wx = np.where(fx < 0, 0.0, fx - np.floor(fx))[None, :]
    for c in range(3):
        p = img[:, :, c].astype(np.float32)
        v = ((1 - wy) * ((1 - wx) * p[y0][:, x0] + wx * p[y0][:, x1])
             + wy * ((1 - wx) * p[y1][:, x0] + wx * p[y1][:, x1]))
        if mode == 1:
            v = v / 127.5 - 1.0
        elif mode == 2:
            v = v - mean[c]
        else:
            v = (v - mean[c]) * std[c]
        out[c] = v
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_image_preprocess_kernel(hipshm, mode):
    from client_amd.ops import hip_runtime as hr

    ih, iw, oh, ow = 300, 451, 224, 224
    img = np.random.randint(0, 256, (ih, iw, 3), dtype=np.uint8)
    mean = [104.0, 117.0, 123.0]
    std = [1.0, 1.0, 1.0]
    src = hr.malloc(0, img.nbytes)
    dst = hr.malloc(0, 3 * oh * ow * 4)
    try:
        hr.memcpy_h2d(src, img.reshape(-1), img.nbytes, 0, True)
        hr.image_preprocess(src, dst, ih, iw, oh, ow, mode, False, mean, std,
                            0, True)
        out = np.empty(3 * oh * ow, dtype=np.float32)
        hr.memcpy_d2h_into(dst, out.view(np.uint8), out.nbytes, 0)
        ref = _ref_preprocess(img, oh, ow, mode, mean, std)
        # kernel computes in fp32 (fmaf contraction); the float64 numpy
        # reference differs by up to ~8e-3 on the 0..255 pixel scale
        # (measured maxdiff 0.0077 = 3e-5 relative) — far below the u8
        # quantization step. The 0.02 is on the pixel scale; the output
        # scale of the mode applies to it (mode 1 maps 0..255 to -1..1,
        # mode 0 multiplies by std_c).
        scale = (np.full(3, 1 / 127.5) if mode == 1 else
                 np.abs(np.asarray(std)) if mode == 0 else np.ones(3))
        err = np.abs(out.reshape(3, oh, ow).astype(np.float64) - ref)
        assert np.all(err <= 0.02 * scale.reshape(3, 1, 1)), (
            err.max(axis=(1, 2)))
    finally:
        hr.free(src)
        hr.free(dst)


def _ipc_child(handle_bytes, n, conn):
    """Child process: open the IPC handle, double the data in-place."""
    try:
        import os

        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import time

        from client_amd.ops import hip_runtime as hr
        import numpy as np

        ptr = None
        for attempt in range(3):
            try:
                ptr = hr.ipc_open_mem_handle(handle_bytes)
                break
            except RuntimeError:
                if attempt == 2:
                    raise
                time.sleep(1.0)
        data = np.frombuffer(hr.memcpy_d2h(ptr, n * 4, 0), dtype=np.float32)
        hr.memcpy_h2d(ptr, (data * 2).view(np.uint8), n * 4, 0, True)
        hr.ipc_close_mem_handle(ptr)
        conn.send("ok")
    except Exception as e:  # pragma: no cover
        conn.send(f"error: {e}")


def test_ipc_cross_process(hipshm):
    """The actual IPC contract: a second process opens the region via the
    64-byte handle and mutates it (the server side of SURVEY.md §3.5)."""
    n = 4096
    h = hipshm.create_shared_memory_region("ipc0", n * 4, 0)
    try:
        x = np.random.rand(n).astype(np.float32)
        hipshm.set_shared_memory_region(h, [x])
        raw = hipshm.get_raw_handle_bytes(h)
        ctx = mp.get_context("spawn")
        parent, child = ctx.Pipe()
        p = ctx.Process(target=_ipc_child, args=(raw, n, child))
        p.start()
        assert parent.poll(120), "ipc child timed out"
        msg = parent.recv()
        p.join(30)
        assert msg == "ok", msg
        out = hipshm.get_contents_as_numpy(h, np.float32, [n])
        np.testing.assert_allclose(out, x * 2, rtol=1e-6)
    finally:
        hipshm.destroy_shared_memory_region(h)


def test_rccl_broadcast_region_tensor(hipshm):
    """The bench.py fan-out path: a HIP-shm region wrapped via DLPack is
    a valid RCCL collective operand. world_size=1 nccl group (the 8-GPU
    case is driver-run; this pins the API path)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch GPU")
    import os

    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29611")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        n = 1 << 16
        h = hipshm.create_shared_memory_region("bcast0", n * 2, 0)
        try:
            x = np.random.rand(n).astype(np.float32)
            hipshm.set_shared_memory_region_cast(h, x, "BF16")
            smt = hipshm.as_shared_memory_tensor(h, "BF16", [n])
            t = torch.from_dlpack(smt)
            assert t.dtype == torch.bfloat16 and t.is_cuda
            dist.broadcast(t, src=0)
            torch.cuda.synchronize()
            back = hipshm.get_contents_cast(h, "BF16", [n])
            from client_amd.utils import (
                deserialize_bf16_tensor,
                serialize_bf16_tensor,
            )

            np.testing.assert_array_equal(
                back, deserialize_bf16_tensor(serialize_bf16_tensor(x).item())
            )
        finally:
            hipshm.destroy_shared_memory_region(h)
    finally:
        dist.destroy_process_group()


def test_decode_scheduler_graph_matches_eager(hipshm):
    """hipGraph-captured decode must produce the same tokens as the
    eager decode path on the same weights (GPU)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch GPU")
    from client_amd.models.llama import LlamaModel, llama_tiny_config
    from client_amd.server.decode_scheduler import DecodeScheduler

    torch.manual_seed(7)
    cfg = llama_tiny_config()
    m = LlamaModel(cfg).to("cuda:0").eval()
    prompts = [np.random.randint(0, cfg.vocab_size, n) for n in (6, 10)]

    def run(use_graph):
        sched = DecodeScheduler(m, max_batch=2, device="cuda:0",
                                use_graph=use_graph, len_bucket=32)
        try:
            queues = [sched.submit(p, 8) for p in prompts]
            out = []
            for q in queues:
                toks = []
                while True:
                    t = q.get(timeout=120)
                    if t is sched.END:
                        break
                    toks.append(t)
                out.append(toks)
            return out
        finally:
            sched.shutdown()

    eager = run(False)
    graph = run(True)
    assert eager == graph
    assert all(len(t) == 8 for t in eager)


def test_fused_rmsnorm_and_rope_numerics(hipshm):
    """Fused decode kernels vs the plain torch reference (bf16, fp32
    internal math)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch GPU")
    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(11)
    stream = torch.cuda.current_stream().cuda_stream

    # rmsnorm
    rows, dim = 8, 4096
    x = torch.randn(rows, dim, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(dim, device="cuda", dtype=torch.bfloat16)
    out = torch.empty_like(x)
    hr.rmsnorm_bf16(x.data_ptr(), w.data_ptr(), out.data_ptr(), rows, dim,
                    1e-5, stream)
    torch.cuda.synchronize()
    xf = x.float()
    ref = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)
           * w.float()).to(torch.bfloat16)
    # reduction order differs (tree vs torch mean): allow 2 ulp of bf16
    torch.testing.assert_close(out.float(), ref.float(), rtol=2e-2,
                               atol=2e-2)

    # rope (q+k fused, per-row positions)
    b, hq, hk, d = 4, 8, 2, 128
    max_seq = 64
    inv = 1.0 / (10000 ** (torch.arange(0, d, 2, device="cuda").float() / d))
    t = torch.arange(max_seq, device="cuda").float()
    freqs = torch.outer(t, inv)
    cos, sin = torch.cos(freqs).contiguous(), torch.sin(freqs).contiguous()
    pos = torch.tensor([3, 17, 0, 42], dtype=torch.int64, device="cuda")
    q = torch.randn(b, hq, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, hk, d, device="cuda", dtype=torch.bfloat16)
    q2, k2 = q.clone(), k.clone()
    hr.rope_decode_bf16(q2.data_ptr(), k2.data_ptr(), cos.data_ptr(),
                        sin.data_ptr(), pos.data_ptr(), b, hq, hk, d, stream)
    torch.cuda.synchronize()

    def ref_rope(x, heads):
        c = cos[pos][:, None, :]  # [b,1,d/2]
        s = sin[pos][:, None, :]
        x1, x2 = x[..., 0::2].float(), x[..., 1::2].float()
        out = torch.empty_like(x)
        out[..., 0::2] = (x1 * c - x2 * s).to(torch.bfloat16)
        out[..., 1::2] = (x1 * s + x2 * c).to(torch.bfloat16)
        return out

    torch.testing.assert_close(q2.float(), ref_rope(q, hq).float(),
                               rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(k2.float(), ref_rope(k, hk).float(),
                               rtol=1e-2, atol=1e-2)


def test_region_lifecycle_no_leak(hipshm):
    """HIP memory growth check (GPU analog of the reference's
    memory_growth tests): 200 create/pack/destroy cycles must not leak
    device memory."""
    from client_amd.ops import hip_runtime as hr

    n = 1 << 18
    x = np.random.rand(n).astype(np.float32)
    # warmup (stream/scratch pools allocate lazily)
    for _ in range(5):
        h = hipshm.create_shared_memory_region("leak_w", n * 2, 0)
        hipshm.set_shared_memory_region_cast(h, x, "BF16")
        hipshm.destroy_shared_memory_region(h)
    free_before, _ = hr.mem_info(0)
    for i in range(200):
        h = hipshm.create_shared_memory_region(f"leak_{i}", n * 2, 0)
        hipshm.set_shared_memory_region_cast(h, x, "BF16")
        hipshm.destroy_shared_memory_region(h)
    free_after, _ = hr.mem_info(0)
    leaked = free_before - free_after
    assert leaked < 64 * 2**20, f"leaked {leaked/2**20:.1f} MiB over 200 cycles"


@pytest.mark.gpu
def test_bias_act_kernel_numerics(hipshm):
    """bias_act_bf16 vs torch reference across plane sizes incl. the
    odd 7x7=49 tail path, with and without ReLU, in-place."""
    import torch

    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(3)
    for (c, h, w) in [(64, 56, 56), (256, 7, 7), (32, 14, 14), (8, 3, 5)]:
        x = torch.randn(4, c, h, w, device="cuda", dtype=torch.bfloat16)
        bias = torch.randn(c, device="cuda", dtype=torch.float32)
        for relu in (False, True):
            ref = x.float() + bias.view(1, -1, 1, 1)
            if relu:
                ref = ref.relu()
            ref = ref.to(torch.bfloat16)
            y = x.clone()
            hr.bias_act_bf16(
                y.data_ptr(), bias.data_ptr(), y.data_ptr(),
                4 * c, h * w, c, relu,
                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(y, ref), (c, h, w, relu)


@pytest.mark.gpu
def test_bias_res_act_kernel_numerics(hipshm):
    """bias_res_act_bf16 (bias + residual + ReLU, one pass) vs torch
    reference across resnet plane sizes incl. odd 7x7=49, in-place."""
    import torch

    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(5)
    for (c, h, w) in [(256, 56, 56), (2048, 7, 7), (512, 14, 14),
                      (8, 3, 5)]:
        x = torch.randn(4, c, h, w, device="cuda", dtype=torch.bfloat16)
        r = torch.randn(4, c, h, w, device="cuda", dtype=torch.bfloat16)
        bias = torch.randn(c, device="cuda", dtype=torch.float32)
        ref = (x.float() + r.float() + bias.view(1, -1, 1, 1)).relu()
        ref = ref.to(torch.bfloat16)
        y = x.clone()
        hr.bias_res_act_bf16(
            y.data_ptr(), r.data_ptr(), bias.data_ptr(), y.data_ptr(),
            4 * c, h * w, c, True,
            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(y, ref), (c, h, w)


@pytest.mark.gpu
def test_fused_bottleneck_matches_plain_fold_gpu():
    """The full fused ResNet50 forward (BiasAct + BiasResAct kernels) on
    bf16 must match the plain-folded model within bf16 tolerance."""
    import copy

    import torch

    from client_amd.models.resnet import ResNet50, fold_batchnorm

    torch.manual_seed(2)
    m = ResNet50().eval()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)
    plain = fold_batchnorm(copy.deepcopy(m), fuse_eltwise=False)
    fused = fold_batchnorm(copy.deepcopy(m), fuse_eltwise=True)
    plain = plain.to("cuda", torch.bfloat16)
    fused = fused.to("cuda", torch.bfloat16)
    x = torch.randn(8, 3, 224, 224, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        a = plain(x).float()
        b = fused(x).float()
    torch.cuda.synchronize()
    # fused kernels do the adds in fp32 (plain path adds in bf16); the
    # logits land within a few bf16 ulps of each other
    assert torch.allclose(a, b, atol=0.15, rtol=0.05), (
        (a - b).abs().max().item()
    )


@pytest.mark.gpu
def test_gather_pack_tiled_transpose(hipshm):
    """The transpose-pattern fast path (LDS 64x64 tiles) must be
    bit-identical to the naive gather for 2-D/3-D transposes across
    dtypes and ragged extents."""
    import torch

    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(7)
    cases = [
        ((512, 768), torch.float32),
        ((1000, 333), torch.float32),   # ragged tiles
        ((256, 512), torch.bfloat16),
        ((128, 96), torch.float64),
        ((4, 256, 192), torch.float32),  # batched transpose of last 2
    ]
    for shape, dt in cases:
        x = (torch.randn(shape, device="cuda") * 100).to(dt)
        xt = x.transpose(-1, -2)  # strided view: innermost dim strided
        n = x.numel()
        esz = x.element_size()
        dst = hr.malloc(0, n * esz)
        try:
            hr.gather_pack(x.data_ptr(), dst, esz,
                           list(xt.shape), list(xt.stride()), 0, True)
            out = np.empty(n * esz, dtype=np.uint8)
            hr.memcpy_d2h_into(dst, out, n * esz, 0)
            refc = xt.contiguous().cpu()
            if dt == torch.bfloat16:
                refc = refc.view(torch.uint16)
            ref = refc.numpy().view(np.uint8).reshape(-1)
            np.testing.assert_array_equal(out, ref, err_msg=str((shape, dt)))
        finally:
            hr.free(dst)


@pytest.mark.gpu
def test_image_preprocess_batched_matches_single(hipshm):
    """One batched launch must produce exactly the per-image kernel's
    output for every image in the batch."""
    from client_amd.ops import hip_runtime as hr

    nimg, ih, iw, oh, ow = 8, 300, 451, 224, 224
    imgs = np.random.randint(0, 256, (nimg, ih, iw, 3), dtype=np.uint8)
    mean = [104.0, 117.0, 123.0]
    std = [1.0, 1.0, 1.0]
    src = hr.malloc(0, imgs.nbytes)
    dst_b = hr.malloc(0, nimg * 3 * oh * ow * 4)
    dst_1 = hr.malloc(0, 3 * oh * ow * 4)
    try:
        hr.memcpy_h2d(src, imgs.reshape(-1), imgs.nbytes, 0, True)
        hr.image_preprocess_batched(src, dst_b, nimg, ih, iw, oh, ow, 2,
                                    False, mean, std, 0, True)
        batched = np.empty(nimg * 3 * oh * ow, dtype=np.float32)
        hr.memcpy_d2h_into(dst_b, batched.view(np.uint8), batched.nbytes, 0)
        batched = batched.reshape(nimg, 3, oh, ow)
        for i in range(nimg):
            img_off = src + i * ih * iw * 3
            hr.image_preprocess(img_off, dst_1, ih, iw, oh, ow, 2, False,
                                mean, std, 0, True)
            single = np.empty(3 * oh * ow, dtype=np.float32)
            hr.memcpy_d2h_into(dst_1, single.view(np.uint8), single.nbytes,
                               0)
            np.testing.assert_array_equal(
                batched[i], single.reshape(3, oh, ow), err_msg=f"img {i}"
            )
    finally:
        hr.free(src)
        hr.free(dst_b)
        hr.free(dst_1)


@pytest.mark.gpu
def test_gqa_bmm_decode_matches_sdpa():
    """The grouped-bmm decode attention (no K/V materialization) must
    produce the same generations as the repeat_interleave+sdpa path."""
    import torch

    from client_amd.models import llama as L

    torch.manual_seed(11)
    cfg = L.llama_tiny_config()
    m = L.LlamaModel(cfg).eval().to("cuda", torch.bfloat16)
    tokens = torch.randint(0, cfg.vocab_size, (3, 1), device="cuda")
    pos = torch.tensor([5, 9, 2], device="cuda")
    kv = m.make_kv_cache(3, "cuda", torch.bfloat16)
    for ck, cv in kv:
        ck.normal_()
        cv.normal_()
    kv2 = [(ck.clone(), cv.clone()) for ck, cv in kv]

    old = L._GQA_BMM
    try:
        with torch.inference_mode():
            L._GQA_BMM = True
            a = m.forward_decode_batch(tokens, pos, kv, max_len=16)
            L._GQA_BMM = False
            b = m.forward_decode_batch(tokens, pos, kv2, max_len=16)
    finally:
        L._GQA_BMM = old
    torch.cuda.synchronize()
    assert torch.allclose(a.float(), b.float(), atol=0.25, rtol=0.05), (
        (a.float() - b.float()).abs().max().item()
    )
    # the decision that matters: identical argmax tokens
    assert torch.equal(a.argmax(-1), b.argmax(-1))


@pytest.mark.gpu
def test_bias_res_act_channels_last_numerics():
    """Channels-last fused bias(+residual)+ReLU must be bit-exact with
    the NCHW kernel result order ((x+res)+bias, RNE) on NHWC tensors."""
    import torch

    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(13)
    for (c, h, w) in [(64, 56, 56), (2048, 7, 7), (8, 5, 3)]:
        cl = torch.channels_last
        x = torch.randn(4, c, h, w, device="cuda", dtype=torch.bfloat16
                        ).contiguous(memory_format=cl)
        r = torch.randn(4, c, h, w, device="cuda", dtype=torch.bfloat16
                        ).contiguous(memory_format=cl)
        bias = torch.randn(c, device="cuda", dtype=torch.float32)
        ref = (x.float() + r.float() + bias.view(1, -1, 1, 1)).relu()
        ref = ref.to(torch.bfloat16)
        y = x.clone()  # preserves channels_last
        hr.bias_res_act_cl_bf16(
            y.data_ptr(), r.data_ptr(), bias.data_ptr(), y.data_ptr(),
            y.numel(), c, True, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(y, ref), (c, h, w)
        # bias-only + relu path (res = null)
        y2 = x.clone()
        ref2 = (x.float() + bias.view(1, -1, 1, 1)).relu().to(torch.bfloat16)
        hr.bias_res_act_cl_bf16(
            y2.data_ptr(), 0, bias.data_ptr(), y2.data_ptr(),
            y2.numel(), c, True, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(y2, ref2), (c, h, w)


@pytest.mark.gpu
def test_decode_gemm_numerics():
    """Skinny decode GEMM vs torch linear (fp32-accum reference) on the
    real decode shapes; bf16-ulp agreement."""
    import torch

    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(17)
    for (n, k) in [(4096, 4096), (1024, 4096), (14336, 4096),
                   (4096, 14336), (128256, 4096), (512, 512)]:
        x = torch.randn(8, k, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16) * 0.02
        y = torch.empty(8, n, device="cuda", dtype=torch.bfloat16)
        hr.decode_gemm_bf16(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                            n, k, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref = (x.float() @ w.float().t())
        got = y.float()
        # both accumulate in fp32; reduction ORDER differs, so allow a
        # few bf16 ulps relative to the magnitude
        tol = ref.abs().max().item() * 2 ** -7 + 1e-2
        assert (got - ref).abs().max().item() < tol, (
            n, k, (got - ref).abs().max().item()
        )


@pytest.mark.gpu
def test_decode_gemm_in_model_matches_torch():
    """forward_decode_batch with the kernel GEMMs produces the same
    argmax tokens as the torch-linear path."""
    import torch

    from client_amd.models import llama as L

    torch.manual_seed(19)
    cfg = L.LlamaConfig(vocab_size=2048, dim=512, n_layers=2, n_heads=8,
                        n_kv_heads=4, ffn_dim=1024, max_seq=128)
    m = L.LlamaModel(cfg).eval().to("cuda", torch.bfloat16)
    tokens = torch.randint(0, cfg.vocab_size, (8, 1), device="cuda")
    pos = torch.randint(1, 64, (8,), device="cuda")
    kv = m.make_kv_cache(8, "cuda", torch.bfloat16)
    for ck, cv in kv:
        ck.normal_(std=0.1)
        cv.normal_(std=0.1)
    kv2 = [(ck.clone(), cv.clone()) for ck, cv in kv]
    old = L._DECODE_GEMM
    try:
        with torch.inference_mode():
            L._DECODE_GEMM = True
            a = m.forward_decode_batch(tokens, pos, kv, max_len=64)
            L._DECODE_GEMM = False
            b = m.forward_decode_batch(tokens, pos, kv2, max_len=64)
    finally:
        L._DECODE_GEMM = old
    torch.cuda.synchronize()
    assert torch.allclose(a.float(), b.float(), atol=0.3, rtol=0.05)
    assert (a.argmax(-1) == b.argmax(-1)).float().mean() > 0.9


@pytest.mark.gpu
def test_rope_scatter_decode_kernel():
    """Fused RoPE+KV-scatter: q rotated in place, rotated k / copied v
    land at each row's cache position, rest of the cache untouched."""
    import torch

    from client_amd.models.llama import precompute_rope
    from client_amd.ops import hip_runtime as hr

    torch.manual_seed(23)
    b, hq, hk, d, clen = 8, 8, 4, 64, 33
    cos, sin = precompute_rope(d, clen, 10000.0, "cuda")
    q = torch.randn(b, hq, 1, d, device="cuda", dtype=torch.bfloat16
                    ).contiguous()
    k = torch.randn(b, hk, 1, d, device="cuda", dtype=torch.bfloat16
                    ).contiguous()
    v = torch.randn(b, hk, 1, d, device="cuda", dtype=torch.bfloat16
                    ).contiguous()
    ck = torch.zeros(b, hk, clen, d, device="cuda", dtype=torch.bfloat16)
    cv = torch.zeros_like(ck)
    pos = torch.randint(0, clen, (b,), device="cuda", dtype=torch.int64)

    def rope_ref(t):
        c = cos[pos][:, None, None, :].float()
        s = sin[pos][:, None, None, :].float()
        tf = t.float()
        t1, t2 = tf[..., 0::2], tf[..., 1::2]
        out = torch.empty_like(tf)
        out[..., 0::2] = t1 * c - t2 * s
        out[..., 1::2] = t1 * s + t2 * c
        return out.to(torch.bfloat16)

    q_ref = (rope_ref(q).float() * 0.5).to(torch.bfloat16)
    k_ref = rope_ref(k)
    hr.rope_scatter_decode_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), ck.data_ptr(),
        cv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(),
        b, hq, hk, d, clen, q_scale=0.5,
        stream_handle=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(q, q_ref)
    ar = torch.arange(b, device="cuda")
    assert torch.equal(ck[ar, :, pos], k_ref[:, :, 0])
    assert torch.equal(cv[ar, :, pos], v[:, :, 0])
    # everything else stays zero
    mask = torch.ones(b, hk, clen, d, device="cuda", dtype=torch.bool)
    mask[ar, :, pos] = False
    assert ck[mask].abs().sum() == 0
    assert cv[mask].abs().sum() == 0


@pytest.mark.gpu
def test_overlapped_broadcaster_pipeline_nccl_world1(hipshm):
    """The full bench.py world>1 pipeline machinery on CUDA under an
    nccl world=1 group: ping-pong HIP-shm staging regions, pack kernel
    on the HIP-runtime stream, ExternalStream event ordering, the
    side-stream collective with work.wait(), hipEvent bcast timing and
    the stream-synchronize host gate. (The 8-GPU run is driver-side;
    this pins every API the multi-rank path exercises.)"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch GPU")
    import os

    import torch.distributed as dist

    from client_amd.parallel import OverlappedBroadcaster

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29613")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        n = 1 << 14
        regions = [
            hipshm.create_shared_memory_region(f"ovl{b}", n * 2, 0)
            for b in range(2)
        ]
        try:
            bc = OverlappedBroadcaster(regions, (n,), "BF16", src=0)
            assert bc._cuda

            data = [np.random.rand(n).astype(np.float32)
                    for _ in range(7)]

            def pack_for(step):
                def pack_fn(buf_idx, v=data[step]):
                    hipshm.set_shared_memory_region_cast(
                        regions[buf_idx], v, "BF16", sync=False)
                return pack_fn

            # prologue + 6 pipelined steps, exactly bench.py's loop
            bc.stage_and_broadcast(0, pack_for(0))
            for step in range(6):
                bc.wait_ready()
                # serve step: buffer step%2 must hold data[step]
                got = hipshm.get_contents_cast(regions[step % 2],
                                               "BF16", [n])
                np.testing.assert_allclose(got, data[step], rtol=2e-2,
                                           atol=2e-2)
                nxt = step + 1
                if nxt < 7:
                    bc.stage_and_broadcast(nxt % 2, pack_for(nxt))
            bc.wait_ready()
            # hipEvent timings were recorded for every broadcast
            assert len(bc.bcast_ms) == 7
            assert all(t >= 0.0 for t in bc.bcast_ms)
        finally:
            for r in regions:
                hipshm.destroy_shared_memory_region(r)
    finally:
        dist.destroy_process_group()
