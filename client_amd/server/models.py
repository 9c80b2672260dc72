"""Model runtime for the client_amd test/benchmark server.

The reference repo is a client SDK with no server, but its test strategy
relies on a live server with canonical fixture models
(reference: src/c++/tests/cc_client_test.cc:42-129 uses
onnx_int32_int32_int32-style models; SURVEY.md §4 calls for a
fake-server fixture). This module provides:

- IdentityModel       — echoes inputs (the ``identity_fp32`` fixture)
- AddSubModel         — INPUT0+INPUT1 / INPUT0-INPUT1 (the simple_* fixture)
- SequenceModel       — server-held per-sequence accumulator state
- RepeatModel         — decoupled: N responses per request (repeat_int32)
- TorchModel          — a torch.nn.Module executed on an MI355X via
                        PyTorch-ROCm (bf16), used by the benchmark
"""

import threading
import time

import numpy as np

from ..utils import triton_to_np_dtype

# Process-wide: only one hipGraph capture at a time, and captures use
# thread_local error mode so concurrently-serving threads (other models
# on the same GPU) are not poisoned by capture state. Found by the
# mixed-load soak: global-mode capture made every other model fail with
# hipErrorStreamCaptureUnsupported.
class _RWLock:
    """Writer-priority readers/writer lock. Model EXECUTIONS hold it
    shared; hipGraph CAPTURES hold it exclusive. Rationale (r02 mixed
    co-serving soak): capturing a new shape while another model's
    MIOpen kernels launch concurrently invalidates the capture
    (thread_local capture mode does not protect MIOpen's launch path
    on this ROCm build), and torch's capture-failure cleanup then
    aborts the whole process from a noexcept context. Exclusivity at
    capture time prevents the poisoning outright; writer priority
    keeps a capture from starving under request traffic."""

    def __init__(self):
        self._cond = threading.Condition()
        self._readers = 0
        self._writer = False
        self._pending_writers = 0

    def acquire_read(self):
        with self._cond:
            while self._writer or self._pending_writers:
                self._cond.wait()
            self._readers += 1

    def release_read(self):
        with self._cond:
            self._readers -= 1
            if self._readers == 0:
                self._cond.notify_all()

    def acquire_write(self):
        with self._cond:
            self._pending_writers += 1
            while self._writer or self._readers:
                self._cond.wait()
            self._pending_writers -= 1
            self._writer = True

    def release_write(self):
        with self._cond:
            self._writer = False
            self._cond.notify_all()


class _WriteGuard:
    def __init__(self, lock):
        self._lock = lock

    def __enter__(self):
        self._lock.acquire_write()

    def __exit__(self, *exc):
        self._lock.release_write()


class _ReadGuard:
    def __init__(self, lock):
        self._lock = lock

    def __enter__(self):
        self._lock.acquire_read()

    def __exit__(self, *exc):
        self._lock.release_read()


_GRAPH_RW = _RWLock()
# capture sites: exclusive (name kept from r01 so call sites read the same)
GRAPH_CAPTURE_LOCK = _WriteGuard(_GRAPH_RW)
# model-execution sites: shared
GRAPH_EXEC_SHARED = _ReadGuard(_GRAPH_RW)


class Model:
    """Base model: subclasses implement execute(inputs, parameters)
    returning a dict name -> numpy array."""

    def __init__(self, name, inputs, outputs, max_batch_size=0, platform="python",
                 decoupled=False):
        # inputs/outputs: list of (name, datatype, shape) with -1 for dynamic dims
        self.name = name
        self.inputs = inputs
        self.outputs = outputs
        self.max_batch_size = max_batch_size
        self.platform = platform
        self.decoupled = decoupled
        self.versions = ["1"]

    def metadata(self):
        return {
            "name": self.name,
            "versions": self.versions,
            "platform": self.platform,
            "inputs": [
                {"name": n, "datatype": d, "shape": list(s)} for n, d, s in self.inputs
            ],
            "outputs": [
                {"name": n, "datatype": d, "shape": list(s)} for n, d, s in self.outputs
            ],
        }

    def config(self):
        return {
            "name": self.name,
            "platform": self.platform,
            "backend": self.platform,
            "max_batch_size": self.max_batch_size,
            "input": [
                {"name": n, "data_type": "TYPE_" + d, "dims": list(s)}
                for n, d, s in self.inputs
            ],
            "output": [
                {"name": n, "data_type": "TYPE_" + d, "dims": list(s)}
                for n, d, s in self.outputs
            ],
            "model_transaction_policy": {"decoupled": self.decoupled},
        }

    def execute(self, inputs, parameters):
        raise NotImplementedError


class IdentityModel(Model):
    """Echo each INPUTi to OUTPUTi. identity_fp32 fixture analog."""

    # the fixture identity accepts any rank (its [-1] dims are a
    # placeholder, not a 1-D contract) — skip server shape validation
    lax_shapes = True

    def __init__(self, name="identity_fp32", datatype="FP32", n_io=1):
        ios = [("INPUT" + str(i) if n_io > 1 else "INPUT0", datatype, [-1])
               for i in range(n_io)]
        outs = [("OUTPUT" + str(i) if n_io > 1 else "OUTPUT0", datatype, [-1])
                for i in range(n_io)]
        super().__init__(name, ios, outs)

    def execute(self, inputs, parameters):
        out = {}
        for (in_name, _, _), (out_name, _, _) in zip(self.inputs, self.outputs):
            out[out_name] = inputs[in_name]
        return out


class AddSubModel(Model):
    """OUTPUT0 = INPUT0 + INPUT1; OUTPUT1 = INPUT0 - INPUT1.

    Matches the canonical simple/onnx_int32_int32_int32 fixture shape
    used throughout the reference examples (e.g.
    src/python/examples/simple_http_infer_client.py).
    """

    def __init__(self, name="simple", datatype="INT32", shape=(-1, 16)):
        super().__init__(
            name,
            [("INPUT0", datatype, list(shape)), ("INPUT1", datatype, list(shape))],
            [("OUTPUT0", datatype, list(shape)), ("OUTPUT1", datatype, list(shape))],
        )

    def execute(self, inputs, parameters):
        a, b = inputs["INPUT0"], inputs["INPUT1"]
        if a.dtype == np.object_:
            # BYTES add/sub fixture: numeric strings
            ai = np.array([int(x) for x in a.reshape(-1)]).reshape(a.shape)
            bi = np.array([int(x) for x in b.reshape(-1)]).reshape(b.shape)
            return {
                "OUTPUT0": np.char.encode((ai + bi).astype(str), "utf-8").astype(np.object_),
                "OUTPUT1": np.char.encode((ai - bi).astype(str), "utf-8").astype(np.object_),
            }
        return {"OUTPUT0": a + b, "OUTPUT1": a - b}


class SequenceModel(Model):
    """Stateful sequence accumulator: the server holds per-sequence_id
    running sums; sequence_start resets, sequence_end finalizes
    (server-side analog of the reference's sequence examples,
    simple_grpc_sequence_stream_infer_client.cc)."""

    def __init__(self, name="sequence_accumulate", datatype="INT32"):
        super().__init__(name, [("INPUT", datatype, [1])], [("OUTPUT", datatype, [1])])
        self._state = {}

    def execute(self, inputs, parameters):
        seq_id = parameters.get("sequence_id", 0)
        start = parameters.get("sequence_start", False)
        end = parameters.get("sequence_end", False)
        val = inputs["INPUT"]
        if start or seq_id not in self._state:
            self._state[seq_id] = np.zeros_like(val)
        self._state[seq_id] = self._state[seq_id] + val
        out = self._state[seq_id].copy()
        if end:
            self._state.pop(seq_id, None)
        return {"OUTPUT": out}


class RepeatModel(Model):
    """Decoupled model: for input IN (shape [n]) and DELAY, produces one
    response per element (reference example:
    simple_grpc_custom_repeat.cc:135-176 drives the repeat_int32 model)."""

    def __init__(self, name="repeat_int32"):
        super().__init__(
            name,
            [("IN", "INT32", [-1]), ("DELAY", "UINT32", [-1]), ("WAIT", "UINT32", [1])],
            [("OUT", "INT32", [1]), ("IDX", "UINT32", [1])],
            decoupled=True,
        )

    def execute_decoupled(self, inputs, parameters):
        vals = inputs["IN"].reshape(-1)
        delays = inputs.get("DELAY")
        delays = delays.reshape(-1) if delays is not None else np.zeros(len(vals))
        for idx, v in enumerate(vals):
            if idx < len(delays) and delays[idx] > 0:
                time.sleep(float(delays[idx]) / 1000.0)
            yield {
                "OUT": np.array([v], dtype=np.int32),
                "IDX": np.array([idx], dtype=np.uint32),
            }

    def execute(self, inputs, parameters):
        # Non-decoupled fallback: return the first response only.
        for out in self.execute_decoupled(inputs, parameters):
            return out
        return {"OUT": np.zeros(1, np.int32), "IDX": np.zeros(1, np.uint32)}


class GenerateModel(Model):
    """Decoupled LLM token streaming: one response per generated token
    (the decoupled protocol is the reference's
    repeat_int32 shape, simple_grpc_custom_repeat.cc:135-176, applied to
    a real decode loop with KV cache).

    Optional per-request sampling inputs, each of shape [1]:
    ``temperature`` FP32 (default 0 = greedy), ``top_k`` INT32 (0 = off),
    ``top_p`` FP32 (1 = off) and ``seed`` UINT64 (random when absent).
    A request without any of them decodes greedily.

    ``kv_cache_dtype`` None / "bf16" keeps the KV cache in the model
    dtype; "fp8_e4m3" stores it as e4m3 codes (models/kv_cache.py), and
    the served config then carries a ``kv_cache_dtype`` parameter.

    ``weight_dtype`` None / "bf16" keeps the block weights in the model
    dtype; "fp8_e4m3" replaces the seven linears of every block by
    e4m3 weight-only layers (models/weight_fp8.py) after the device and
    dtype casts, and the served config then carries a ``weight_dtype``
    parameter.

    ``fused_prefill`` sets the module's ``fused_prefill`` (prefill chunks
    on the fused HIP kernels, models/llama.py); the served config then
    carries a ``fused_prefill`` parameter."""

    def __init__(self, name, llama_module, device="cuda:0", dtype=None,
                 use_scheduler=True, max_batch=8, prewarm_sampling=False,
                 kv_cache_dtype=None, fused_prefill=False,
                 weight_dtype=None):
        super().__init__(
            name,
            [("input_ids", "INT64", [-1]), ("max_tokens", "INT32", [1]),
             ("temperature", "FP32", [1]), ("top_k", "INT32", [1]),
             ("top_p", "FP32", [1]), ("seed", "UINT64", [1])],
            [("token_id", "INT64", [1]), ("index", "INT32", [1])],
            platform="pytorch",
            decoupled=True,
        )
        import torch

        from ..models.kv_cache import normalize_kv_dtype
        from ..models.weight_fp8 import (normalize_weight_dtype,
                                         quantize_llama_weights)

        self._torch = torch
        self.device = device
        self.kv_cache_dtype = normalize_kv_dtype(kv_cache_dtype)
        self.module = llama_module.to(device)
        if dtype is not None:
            self.module = self.module.to(dtype)
        self.module.eval()
        self.weight_dtype = normalize_weight_dtype(weight_dtype)
        if self.weight_dtype is not None:
            quantize_llama_weights(self.module)
        self.fused_prefill = bool(fused_prefill)
        if self.fused_prefill:
            self.module.fused_prefill = True
        self._scheduler = None
        if use_scheduler:
            from .decode_scheduler import DecodeScheduler

            self._scheduler = DecodeScheduler(
                self.module, max_batch=max_batch, device=device,
                kv_dtype=self.kv_cache_dtype,
            )
            # capture the first decode-graph buckets now, not inside the
            # first request's TTFT (cold capture ≈0.5 s per bucket).
            # 4 buckets = up to 1024 total tokens hiccup-free (an
            # uncaptured bucket showed up as one 86 ms ITL outlier in
            # the 512-token soak).
            self._scheduler.prewarm(n_buckets=4,
                                    sampling=prewarm_sampling)

    def config(self):
        cfg = super().config()
        params = {}
        if self.kv_cache_dtype is not None:
            params["kv_cache_dtype"] = {"string_value": self.kv_cache_dtype}
        if self.weight_dtype is not None:
            params["weight_dtype"] = {"string_value": self.weight_dtype}
        if self.fused_prefill:
            params["fused_prefill"] = {"string_value": "true"}
        if params:
            cfg["parameters"] = params
        return cfg

    def load_metrics(self):
        """ORCA named metrics for the endpoint-load-metrics header."""
        if self._scheduler is None:
            return {}
        return {"kv_cache_utilization": self._scheduler.kv_utilization}

    @staticmethod
    def _sampling_from(inputs):
        """SamplingParams from the optional inputs, or None when the
        request carries none of them. An invalid value is an
        InferenceError naming the input, raised before the request
        reaches the scheduler."""
        names = ("temperature", "top_k", "top_p", "seed")
        if not any(n in inputs for n in names):
            return None
        from ..models.sampling import SamplingParams
        from .core import InferenceError

        def scalar(name, cast, default):
            if name not in inputs:
                return default
            arr = np.asarray(inputs[name]).reshape(-1)
            if arr.size != 1:
                raise InferenceError(
                    f"input '{name}' must hold exactly one element, "
                    f"got {arr.size}")
            return cast(arr[0])

        params = SamplingParams(
            temperature=scalar("temperature", float, 0.0),
            top_k=scalar("top_k", int, 0),
            top_p=scalar("top_p", float, 1.0),
            seed=scalar("seed", int, None),
        )
        try:
            params.validate()
        except ValueError as e:
            raise InferenceError(f"invalid value for input '"
                                 f"{str(e).split(' ', 1)[0]}': {e}") from e
        return params

    def execute_decoupled(self, inputs, parameters):
        torch = self._torch
        max_tokens = int(inputs.get("max_tokens", np.array([16]))[0])
        sampling = self._sampling_from(inputs)
        if self._scheduler is not None:
            # continuous batching: concurrent streams share one decode
            # loop (see decode_scheduler.py)
            ids = np.ascontiguousarray(inputs["input_ids"].astype(np.int64))
            out = self._scheduler.submit(ids, max_tokens, sampling)
            idx = 0
            while True:
                tok = out.get(timeout=600)
                if tok is self._scheduler.END:
                    break
                yield {
                    "token_id": np.array([tok], dtype=np.int64),
                    "index": np.array([idx], dtype=np.int32),
                }
                idx += 1
            return
        input_ids = torch.from_numpy(
            np.ascontiguousarray(inputs["input_ids"].astype(np.int64))
        )[None]
        if sampling is not None and sampling.is_greedy:
            sampling = None
        for idx, tok in enumerate(
                self.module.generate(input_ids, max_tokens, sampling,
                                     kv_dtype=self.kv_cache_dtype)):
            yield {
                "token_id": tok.detach().cpu().numpy().astype(np.int64),
                "index": np.array([idx], dtype=np.int32),
            }

    def execute(self, inputs, parameters):
        for out in self.execute_decoupled(inputs, parameters):
            return out
        return {
            "token_id": np.zeros(1, np.int64),
            "index": np.zeros(1, np.int32),
        }


class PreprocessModel(Model):
    """Server-side image preprocessing: u8 HWC image -> fp32 CHW tensor
    (bilinear resize + normalize). On a GPU this runs the CDNA4
    image_preprocess kernel (client_amd.ops); CPU fixture runs numpy.
    Used standalone or as the first step of an ensemble (the reference's
    ensemble_image_client sends raw images to a preprocess+classify
    ensemble)."""

    def __init__(self, name="preprocess", size=224, mode=1,
                 mean=(104.0, 117.0, 123.0), std=(1.0, 1.0, 1.0),
                 device="cpu"):
        super().__init__(
            name,
            [("IMAGE", "UINT8", [-1, -1, 3])],
            [("TENSOR", "FP32", [1, 3, size, size])],
        )
        self.size = size
        self.mode = mode
        self.mean = list(mean)
        self.std = list(std)
        self.device = device
        # grow-only device scratch (one malloc amortized over the model
        # lifetime instead of malloc/free per request)
        self._scratch = {}

    def _scratch_buf(self, key, dev, nbytes):
        from ..ops import hip_runtime as hr

        ptr, size = self._scratch.get(key, (None, 0))
        if size < nbytes:
            if ptr is not None:
                hr.free(ptr)
            ptr = hr.malloc(dev, nbytes)
            self._scratch[key] = (ptr, nbytes)
        return self._scratch[key][0]

    def execute(self, inputs, parameters):
        img = inputs["IMAGE"].astype(np.uint8)
        batched = img.ndim == 4
        imgs = np.ascontiguousarray(img if batched else img[None])
        n, ih, iw, _ = imgs.shape
        oh = ow = self.size
        if self.device.startswith("cuda"):
            from ..ops import hip_runtime as hr

            dev = int(self.device.split(":")[1]) if ":" in self.device else 0
            src = self._scratch_buf("src", dev, imgs.nbytes)
            dst = self._scratch_buf("dst", dev, n * 3 * oh * ow * 4)
            hr.memcpy_h2d(src, imgs.reshape(-1), imgs.nbytes, dev, False)
            # one launch for the whole batch: the single-image kernel is
            # launch-bound at high rates (~27 us/launch vs 2-3 us of
            # kernel time at 224x224)
            hr.image_preprocess_batched(src, dst, n, ih, iw, oh, ow,
                                        self.mode, False, self.mean,
                                        self.std, dev, True)
            out = np.empty(n * 3 * oh * ow, dtype=np.float32)
            hr.memcpy_d2h_into(dst, out.view(np.uint8), out.nbytes, dev)
            return {"TENSOR": out.reshape(n, 3, oh, ow)}
        # CPU reference path (same pixel-center bilinear convention)
        sy, sx = ih / oh, iw / ow
        fy = (np.arange(oh) + 0.5) * sy - 0.5
        fx = (np.arange(ow) + 0.5) * sx - 0.5
        y0 = np.clip(np.floor(fy).astype(int), 0, ih - 1)
        x0 = np.clip(np.floor(fx).astype(int), 0, iw - 1)
        y1 = np.minimum(ih - 1, y0 + 1)
        x1 = np.minimum(iw - 1, x0 + 1)
        wy = np.where(fy < 0, 0.0, fy - np.floor(fy))[:, None]
        wx = np.where(fx < 0, 0.0, fx - np.floor(fx))[None, :]
        out = np.empty((n, 3, oh, ow), dtype=np.float32)
        for b in range(n):
            for c in range(3):
                p = imgs[b, :, :, c].astype(np.float32)
                v = ((1 - wy) * ((1 - wx) * p[y0][:, x0] + wx * p[y0][:, x1])
                     + wy * ((1 - wx) * p[y1][:, x0] + wx * p[y1][:, x1]))
                if self.mode == 1:
                    v = v / 127.5 - 1.0
                elif self.mode == 2:
                    v = v - self.mean[c]
                else:
                    v = (v - self.mean[c]) * self.std[c]
                out[b, c] = v
        return {"TENSOR": out}


class EnsembleModel(Model):
    """Ensemble scheduling: a linear pipeline of member models with
    tensor-name maps between steps (the core of Triton's ensemble
    extension; reference example ensemble_image_client feeds raw images
    to preprocess -> classify).

    steps: list of (model, input_map, output_map) where input_map maps
    the member's input names to ensemble-scope tensor names and
    output_map maps member output names to ensemble-scope names.
    """

    def __init__(self, name, inputs, outputs, steps):
        super().__init__(name, inputs, outputs, platform="ensemble")
        self.steps = steps

    def execute(self, inputs, parameters):
        pool = dict(inputs)
        for model, input_map, output_map in self.steps:
            member_inputs = {
                member_name: pool[ens_name]
                for member_name, ens_name in input_map.items()
            }
            result = model.execute(member_inputs, parameters)
            for member_name, ens_name in output_map.items():
                pool[ens_name] = result[member_name]
        return {name: pool[name] for name, _, _ in self.outputs}


class TorchModel(Model):
    """Executes a torch.nn.Module on the configured device.

    On an MI355X the module runs in bf16 out of HBM3E; inputs arriving
    via HIP-IPC shared memory are consumed as device tensors without any
    host round-trip (see server/shm.py + ops/_hip extension).
    """

    def __init__(self, name, module, inputs, outputs, device="cuda:0",
                 dtype=None, max_batch_size=0, use_graph=True,
                 optional_inputs=()):
        super().__init__(name, inputs, outputs, max_batch_size, platform="pytorch")
        # names of declared inputs a request may leave out; the module is
        # then called without them (they are its trailing arguments)
        self.optional_inputs = frozenset(optional_inputs)
        unknown = self.optional_inputs - {n for n, _, _ in inputs}
        if unknown:
            raise ValueError(f"optional inputs {sorted(unknown)} are not "
                             f"inputs of model '{name}'")
        import threading

        import torch

        self._torch = torch
        self.device = device
        self.module = module.to(device)
        if dtype is not None:
            self.module = self.module.to(dtype)
        self.dtype = dtype
        import os

        if os.environ.get("CLIENT_AMD_CHANNELS_LAST") == "1":
            # MIOpen's NHWC path: often the fast conv layout on CDNA
            self.module = self.module.to(memory_format=torch.channels_last)
            self._channels_last = True
        else:
            self._channels_last = False
        self.module.eval()
        # hipGraph capture-and-replay per input signature: the serving
        # loop is launch-bound in eager mode; replay submits the whole
        # forward as one graph (HIP graphs, not a tracing compiler).
        self.use_graph = use_graph and device.startswith("cuda")
        self._graphs = {}
        self._graph_lock = threading.Lock()
        self._batcher = None

    def config(self):
        cfg = super().config()
        for entry in cfg["input"]:
            if entry["name"] in self.optional_inputs:
                entry["optional"] = True
        if getattr(self.module, "fused_attention", False):
            cfg["parameters"] = {
                "fused_attention": {"string_value": "true"}}
        return cfg

    def enable_dynamic_batching(self, preferred_batch_size=32,
                                max_queue_delay_us=500, max_batch_size=64):
        """Triton-style dynamic batching in front of the forward."""
        from .batcher import DynamicBatcher

        self._batcher = DynamicBatcher(
            self, preferred_batch_size, max_queue_delay_us, max_batch_size
        )
        if self.max_batch_size == 0:
            self.max_batch_size = max_batch_size
        return self

    def warmup(self, batch_sizes=(8, 32)):
        """Pre-capture hipGraphs (and prime MIOpen kernel caches) for
        the given batch sizes so cold requests don't pay capture
        latency — the reference ModelWarmup analog (model_config.proto
        ModelWarmup; our decode path has the same in
        DecodeScheduler.prewarm)."""
        if not self.device.startswith("cuda"):
            return
        torch = self._torch
        for bs in batch_sizes:
            tensors = []
            for name, datatype, shape in self.inputs:
                if name in self.optional_inputs:
                    continue
                dims = [bs if d == -1 else d for d in shape]
                if len(shape) > 0 and shape[0] == -1:
                    dims[0] = bs
                npdt = triton_to_np_dtype(datatype)
                t = torch.zeros(dims, device=self.device,
                                dtype=torch.float32 if npdt in (np.float32,)
                                else torch.from_numpy(
                                    np.zeros(1, npdt)).dtype)
                if self.dtype is not None and t.is_floating_point():
                    t = t.to(self.dtype)
                tensors.append(t)
            self._execute_direct(tensors)

    def execute(self, inputs, parameters):
        torch = self._torch
        with torch.inference_mode():
            tensors = []
            for name, datatype, _ in self.inputs:
                if name not in inputs:
                    if name in self.optional_inputs:
                        continue
                    from .core import InferenceError

                    raise InferenceError(
                        f"expected inference input '{name}' for model "
                        f"'{self.name}'")
                arr = inputs[name]
                t = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
                if self.dtype is not None and t.is_floating_point():
                    t = t.to(self.dtype)
                tensors.append(t)
            result = self.module(*tensors)
            if not isinstance(result, (tuple, list)):
                result = (result,)
            out = {}
            for (name, datatype, _), t in zip(self.outputs, result):
                npdt = triton_to_np_dtype(datatype)
                tt = t
                if tt.dtype == torch.bfloat16:
                    tt = tt.float()
                out[name] = tt.detach().cpu().numpy().astype(npdt, copy=False)
            return out

    def _capture(self, device_tensors):
        torch = self._torch
        # EXCLUSIVE for warmup + capture: no other model may launch
        # kernels while a capture is open (see _RWLock rationale)
        with GRAPH_CAPTURE_LOCK:
            static_ins = [t.clone() for t in device_tensors]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.inference_mode():
                    for _ in range(3):
                        warm = self.module(*static_ins)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()  # hipGraph under ROCm
            with torch.inference_mode():
                with torch.cuda.graph(graph,
                                      capture_error_mode="thread_local"):
                    out = self.module(*static_ins)
        if not isinstance(out, (tuple, list)):
            out = (out,)
        return static_ins, graph, list(out)

    def execute_torch(self, device_tensors):
        """Device-resident entry point for the HIP-shm data plane. Routes
        through the dynamic batcher when enabled (the batcher worker
        calls _execute_direct on the merged batch)."""
        if self._batcher is not None:
            return self._batcher.infer(device_tensors)
        return self._execute_direct(device_tensors)

    def execute_torch_async(self, device_tensors):
        """Returns (outputs, done_event|None): the event marks the
        producing stream's completion, so callers can order their
        output copies on it instead of a full device synchronize (the
        batcher runs on its own stream — see DynamicBatcher.infer_async
        for the measured head-of-line cost this removes)."""
        if self._batcher is not None:
            return self._batcher.infer_async(device_tensors)
        outs = self._execute_direct(device_tensors)
        ev = None
        if outs and outs[0].is_cuda:
            # reused per-thread event (hipEventCreate churn is costly
            # on ROCm — see DynamicBatcher ring)
            tls = getattr(self, "_ev_tls", None)
            if tls is None:
                import threading

                tls = threading.local()
                self._ev_tls = tls
            ev = getattr(tls, "event", None)
            if ev is None:
                ev = self._torch.cuda.Event()
                tls.event = ev
            ev.record()
        return outs, ev

    def _execute_direct(self, device_tensors):
        """Run the forward on device tensors (no numpy, no host copies).

        With use_graph, the forward is hipGraph-captured per input
        signature and replayed; returned tensors are fresh clones so a
        later replay cannot clobber them. The lock only serializes
        launch submission — GPU work stays pipelined on the stream."""
        torch = self._torch
        if not self.use_graph:
            with GRAPH_EXEC_SHARED:
                with torch.inference_mode():
                    result = self.module(*device_tensors)
                    if not isinstance(result, (tuple, list)):
                        result = (result,)
                    return list(result)
        if self._channels_last:
            device_tensors = [
                t.to(memory_format=self._torch.channels_last)
                if t.dim() == 4 else t
                for t in device_tensors
            ]
        key = tuple((tuple(t.shape), t.dtype) for t in device_tensors)
        with self._graph_lock:
            entry = self._graphs.get(key)
            if entry is None:
                # a capture can be invalidated by concurrent work from
                # co-served models (hipErrorStreamCaptureInvalidated,
                # r02 mixed soak); retry once, then serve this
                # signature eager instead of erroring the request
                for _ in range(2):
                    try:
                        entry = self._capture(device_tensors)
                        break
                    except Exception:
                        entry = "eager"
                        try:
                            self._torch.cuda.synchronize()
                        except Exception:
                            pass
                self._graphs[key] = entry
            if entry == "eager":
                with GRAPH_EXEC_SHARED:
                    with self._torch.inference_mode():
                        result = self.module(*device_tensors)
                        if not isinstance(result, (tuple, list)):
                            result = (result,)
                        return list(result)
            static_ins, graph, static_outs = entry
            with GRAPH_EXEC_SHARED:
                for si, t in zip(static_ins, device_tensors):
                    si.copy_(t)
                graph.replay()
                return [o.clone() for o in static_outs]
