// client_amd._hip_c — MI355X-native HIP runtime + CDNA4 kernels.
//
// The GPU surface of the client stack: HIP-IPC shared
// memory (hipMalloc + hipIpcGetMemHandle / hipIpcOpenMemHandle), async
// copies on cached per-device streams, and hand-written gfx950 kernels
// for the work the reference does on the CPU (per-element BF16 loops,
// OpenCV preprocess) and for the served models' hot paths. Bound here:
//   - device_count / mem_info / malloc / free, ipc_{get,open,close}_mem_handle
//   - memcpy_h2d / memcpy_d2h / memcpy_d2h_into / memcpy_d2d /
//     memcpy_peer_async, stream_sync / stream_handle / stream_fence,
//     device_enable_peer_access / device_sync
//   - cast_fp32_bf16 / cast_bf16_fp32   (wire-exact truncate / zero-pad)
//   - cast_fp32_fp8e4m3 / cast_fp8e4m3_fp32 (OCP e4m3fn, CDNA4 native)
//   - gather_pack (strided -> contiguous, lifts the reference's DLPack
//     contiguity restriction, cuda_shared_memory/__init__.py:328-388)
//   - image_preprocess / image_preprocess_batched (u8 HWC -> resize
//     bilinear -> normalize -> CHW, replaces image_client.cc:86-190's
//     OpenCV path)
//   - bias_act_bf16 / bias_res_act_bf16 / bias_res_act_cl_bf16 /
//     bias_relu_maxpool_bf16 (ResNet50 conv epilogues, NCHW and NHWC)
//   - conv3x3_bias_act_bf16 (ResNet50 bottleneck 3x3 conv + bias + ReLU
//     on the matrix cores, NCHW)
//   - rmsnorm_bf16 / rope_decode_bf16 / rope_scatter_decode_bf16 /
//     decode_gemm_bf16 / sample_logits_bf16 (LLM decode step)
//     fp8w_decode_gemm_bf16 / fp8w_dequant_bf16 (fp8 weight-only linears)
//   - rope_scatter_decode_fp8kv_bf16 (the same scatter into an e4m3 KV
//     cache) / gqa_decode_attention + gqa_decode_attention_workspace_bytes
//     (fused split + combine decode attention over a bf16 or e4m3 cache;
//     GQA_DECODE_SPLIT is its split size in keys)
//   - rope_scatter_prefill_bf16 / rope_scatter_prefill_fp8kv_bf16 (RoPE +
//     scatter of a prefill chunk into mapped cache rows) /
//     gqa_prefill_attention + gqa_prefill_attention_workspace_bytes
//     (flash-style MFMA attention of a chunk over the cache in place;
//     GQA_PREFILL_QTILE / GQA_PREFILL_KTILE are its tile sizes)
//   - encoder_attention (BERT self-attention with a per-row key mask, read
//     in place from the packed qkv projection; ENCODER_ATTN_QTILE /
//     ENCODER_ATTN_KTILE / ENCODER_ATTN_KSTAGE are its tile sizes)
//
// The cast, pack and preprocess kernels are memory-bound streaming
// kernels: 16 B/lane vectorized access, 256-thread blocks (4 waves of
// 64), grid-stride with the grid capped at 2048 workgroups
// (cdna_hip_programming.md §6 G11/G13).
// Pure HIP — no CUDA headers, no torch dependency; torch interop is via
// DLPack in Python.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace py = pybind11;

#define HIP_CHECK(expr)                                                    \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                \
      throw std::runtime_error(std::string(#expr) + " failed: " +          \
                               hipGetErrorString(_e));                     \
    }                                                                      \
  } while (0)

// ---------------------------------------------------------------------------
// CDNA4 kernels + C-ABI launchers. kernels.hip is the single source of
// truth, shared with the C++ client library; it is INCLUDED here (one
// translation unit, one device image) — a separate-TU link was observed
// to abort at first launch on the GPU box.
// ---------------------------------------------------------------------------
#include "kernels.hip"

// ---------------------------------------------------------------------------
// Launch helpers
// ---------------------------------------------------------------------------

// raw device pointers cross the Python boundary as integers
static inline const void* cptr(uintptr_t p) {
  return reinterpret_cast<const void*>(p);
}
static inline void* mptr(uintptr_t p) { return reinterpret_cast<void*>(p); }

// Per-device cached streams: [0] = copy/pack stream, [1] = side stream for
// collective overlap (SURVEY.md §2.9 row 5 mandates the second stream).
static std::mutex g_stream_mu;
static std::unordered_map<int, std::vector<hipStream_t>> g_streams;

static hipStream_t get_stream(int device, int idx = 0) {
  std::lock_guard<std::mutex> lock(g_stream_mu);
  auto& vec = g_streams[device];
  while ((int)vec.size() <= idx) {
    int prev;
    HIP_CHECK(hipGetDevice(&prev));
    HIP_CHECK(hipSetDevice(device));
    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    vec.push_back(s);
    HIP_CHECK(hipSetDevice(prev));
  }
  return vec[idx];
}

// blocks until the stream drains (GIL released) when the caller asked
// for a synchronous call
static void sync_if(bool sync, hipStream_t s) {
  if (!sync) return;
  py::gil_scoped_release release;
  HIP_CHECK(hipStreamSynchronize(s));
}

// ---------------------------------------------------------------------------
// Python bindings
// ---------------------------------------------------------------------------

static std::pair<size_t, size_t> mem_info(int device) {
  int prev;
  HIP_CHECK(hipGetDevice(&prev));
  HIP_CHECK(hipSetDevice(device));
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  HIP_CHECK(hipSetDevice(prev));
  return {free_b, total_b};
}

static int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

static uintptr_t hip_malloc(int device, size_t byte_size) {
  int prev;
  HIP_CHECK(hipGetDevice(&prev));
  HIP_CHECK(hipSetDevice(device));
  void* ptr = nullptr;
  HIP_CHECK(hipMalloc(&ptr, byte_size));
  HIP_CHECK(hipSetDevice(prev));
  return reinterpret_cast<uintptr_t>(ptr);
}

static void hip_free(uintptr_t ptr) {
  HIP_CHECK(hipFree(mptr(ptr)));
}

static py::bytes ipc_get_mem_handle(uintptr_t ptr) {
  hipIpcMemHandle_t handle;
  HIP_CHECK(hipIpcGetMemHandle(&handle, mptr(ptr)));
  return py::bytes(reinterpret_cast<const char*>(&handle), sizeof(handle));
}

static uintptr_t ipc_open_mem_handle(py::bytes raw) {
  std::string s = raw;
  if (s.size() < sizeof(hipIpcMemHandle_t)) {
    s.resize(sizeof(hipIpcMemHandle_t), '\0');
  }
  hipIpcMemHandle_t handle;
  std::memcpy(&handle, s.data(), sizeof(handle));
  void* ptr = nullptr;
  HIP_CHECK(hipIpcOpenMemHandle(&ptr, handle, hipIpcMemLazyEnablePeerAccess));
  return reinterpret_cast<uintptr_t>(ptr);
}

static void ipc_close_mem_handle(uintptr_t ptr) {
  HIP_CHECK(hipIpcCloseMemHandle(mptr(ptr)));
}

static void memcpy_h2d(uintptr_t dst, py::buffer src, size_t byte_size,
                       int device, bool sync) {
  py::buffer_info info = src.request();
  if ((size_t)(info.size * info.itemsize) < byte_size)
    throw std::runtime_error("source buffer smaller than byte_size");
  hipStream_t s = get_stream(device);
  {
    py::gil_scoped_release release;
    HIP_CHECK(hipMemcpyAsync(mptr(dst), info.ptr, byte_size,
                             hipMemcpyHostToDevice, s));
    if (sync) HIP_CHECK(hipStreamSynchronize(s));
  }
}

static py::bytes memcpy_d2h(uintptr_t src, size_t byte_size, int device) {
  std::string out(byte_size, '\0');
  hipStream_t s = get_stream(device);
  {
    py::gil_scoped_release release;
    HIP_CHECK(hipMemcpyAsync(&out[0], mptr(src), byte_size,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  return py::bytes(out);
}

static void memcpy_d2h_into(uintptr_t src, py::buffer dst, size_t byte_size,
                            int device) {
  py::buffer_info info = dst.request(true);
  if ((size_t)(info.size * info.itemsize) < byte_size)
    throw std::runtime_error("destination buffer smaller than byte_size");
  hipStream_t s = get_stream(device);
  {
    py::gil_scoped_release release;
    HIP_CHECK(hipMemcpyAsync(info.ptr, mptr(src), byte_size,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

static void memcpy_d2d(uintptr_t dst, uintptr_t src, size_t byte_size,
                       int device, bool sync) {
  hipStream_t s = get_stream(device);
  {
    py::gil_scoped_release release;
    HIP_CHECK(hipMemcpyAsync(mptr(dst), mptr(src), byte_size,
                             hipMemcpyDeviceToDevice, s));
    if (sync) HIP_CHECK(hipStreamSynchronize(s));
  }
}

static void stream_sync(int device, int idx) {
  hipStream_t s = get_stream(device, idx);
  py::gil_scoped_release release;
  HIP_CHECK(hipStreamSynchronize(s));
}

static uintptr_t stream_handle(int device, int idx) {
  // raw hipStream_t of a cached stream, for torch.cuda.ExternalStream
  // interop (event-ordered overlap of pack kernels with RCCL
  // collectives — SURVEY.md §2.8 final row)
  return reinterpret_cast<uintptr_t>(get_stream(device, idx));
}

static void memcpy_peer_async(uintptr_t dst, int dst_device, uintptr_t src,
                              int src_device, size_t byte_size,
                              int stream_idx) {
  // direct xGMI point-to-point copy; with one call per destination GPU
  // on its own stream, the 7 copies of an 8-way scatter ride 7 distinct
  // xGMI links concurrently (ring bcast is per-link
  // bound; direct scatter is not)
  hipStream_t s = get_stream(src_device, stream_idx);
  py::gil_scoped_release release;
  HIP_CHECK(hipMemcpyPeerAsync(mptr(dst), dst_device, mptr(src), src_device,
                               byte_size, s));
}

static void stream_fence(int device, int from_idx, std::vector<int> to_idxs) {
  // device-side ordering: record an event on stream from_idx and make
  // every stream in to_idxs wait on it — no host block. Used to order
  // the 7-link peer scatter after the pack kernel.
  hipStream_t from = get_stream(device, from_idx);
  hipEvent_t ev;
  HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(ev, from));
  for (int idx : to_idxs) {
    HIP_CHECK(hipStreamWaitEvent(get_stream(device, idx), ev, 0));
  }
  // destruction is deferred by the runtime until the event completes
  HIP_CHECK(hipEventDestroy(ev));
}

static void device_enable_peer_access(int device, int peer) {
  int prev;
  HIP_CHECK(hipGetDevice(&prev));
  HIP_CHECK(hipSetDevice(device));
  hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
  if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
    HIP_CHECK(hipSetDevice(prev));
    throw std::runtime_error(std::string("hipDeviceEnablePeerAccess: ") +
                             hipGetErrorString(e));
  }
  HIP_CHECK(hipSetDevice(prev));
}

static void device_sync() {
  py::gil_scoped_release release;
  HIP_CHECK(hipDeviceSynchronize());
}

// ---- kernel wrappers (operate on raw device pointers) ----

static void cast_fp32_bf16(uintptr_t src, uintptr_t dst, long n, int device,
                           bool sync, int stream_idx) {
  hipStream_t s = get_stream(device, stream_idx);
  HIP_CHECK(ca_cast_fp32_bf16(cptr(src), mptr(dst), n, s));
  sync_if(sync, s);
}

static void cast_bf16_fp32(uintptr_t src, uintptr_t dst, long n, int device,
                           bool sync, int stream_idx) {
  hipStream_t s = get_stream(device, stream_idx);
  HIP_CHECK(ca_cast_bf16_fp32(cptr(src), mptr(dst), n, s));
  sync_if(sync, s);
}

static void cast_fp32_fp8e4m3(uintptr_t src, uintptr_t dst, long n, int device,
                              bool sync, int stream_idx) {
  hipStream_t s = get_stream(device, stream_idx);
  HIP_CHECK(ca_cast_fp32_fp8e4m3(cptr(src), mptr(dst), n, s));
  sync_if(sync, s);
}

static void cast_fp8e4m3_fp32(uintptr_t src, uintptr_t dst, long n, int device,
                              bool sync, int stream_idx) {
  hipStream_t s = get_stream(device, stream_idx);
  HIP_CHECK(ca_cast_fp8e4m3_fp32(cptr(src), mptr(dst), n, s));
  sync_if(sync, s);
}

static void gather_pack(uintptr_t src, uintptr_t dst, int elem_size,
                        std::vector<long> shape, std::vector<long> strides,
                        int device, bool sync) {
  // normalize to 4-D (pad leading dims with 1 / stride 0)
  while (shape.size() < 4) {
    shape.insert(shape.begin(), 1);
    strides.insert(strides.begin(), 0);
  }
  if (shape.size() > 4) throw std::runtime_error("gather_pack: >4D unsupported");
  hipStream_t s = get_stream(device);
  HIP_CHECK(ca_gather_pack(cptr(src), mptr(dst), elem_size, shape.data(),
                           strides.data(), s));
  sync_if(sync, s);
}

// The model-side kernels launch on the CALLER's stream (torch's current
// stream) so they compose with torch ops and hipGraph capture.

static void bias_act_bf16(uintptr_t x, uintptr_t bias, uintptr_t out,
                          long n_planes, long plane, int channels,
                          bool relu, uintptr_t stream_handle) {
  HIP_CHECK(ca_bias_act_bf16(cptr(x), cptr(bias), mptr(out), n_planes, plane,
                             channels, relu ? 1 : 0,
                             reinterpret_cast<hipStream_t>(stream_handle)));
}

static void conv3x3_bias_act_bf16(uintptr_t x, uintptr_t w_packed,
                                  uintptr_t bias, uintptr_t out, int n, int c,
                                  int k, int h, int w, int stride, bool relu,
                                  uintptr_t stream_handle) {
  HIP_CHECK(ca_conv3x3_bias_act_bf16(
      cptr(x), cptr(w_packed), cptr(bias), mptr(out), n, c, k, h, w, stride,
      relu ? 1 : 0, reinterpret_cast<hipStream_t>(stream_handle)));
}

// true when ca_conv3x3_bias_act_bf16 accepts the shape (host-side check)
static bool conv3x3_supported(int n, int c, int k, int h, int w, int stride) {
  Conv3x3Geom g;
  return c3_plan(&g, n, c, k, h, w, stride);
}

static void decode_gemm_bf16(uintptr_t x, uintptr_t w, uintptr_t y, int n,
                             int k, uintptr_t stream_handle) {
  HIP_CHECK(ca_decode_gemm_bf16(
      cptr(x), cptr(w), mptr(y), n, k,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void fp8w_decode_gemm_bf16(uintptr_t x, uintptr_t codes,
                                  uintptr_t scale_exp, uintptr_t y, int m,
                                  int n, int k, uintptr_t stream_handle) {
  HIP_CHECK(ca_fp8w_decode_gemm_bf16(
      cptr(x), cptr(codes), cptr(scale_exp), mptr(y), m, n, k,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void fp8w_dequant_bf16(uintptr_t codes, uintptr_t scale_exp,
                              uintptr_t w_out, int n, int k,
                              uintptr_t stream_handle) {
  HIP_CHECK(ca_fp8w_dequant_bf16(
      cptr(codes), cptr(scale_exp), mptr(w_out), n, k,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void bias_res_act_cl_bf16(uintptr_t x, uintptr_t res, uintptr_t bias,
                                 uintptr_t out, long n, int channels,
                                 bool relu, uintptr_t stream_handle) {
  HIP_CHECK(ca_bias_res_act_cl_bf16(
      cptr(x), cptr(res), cptr(bias), mptr(out), n, channels, relu ? 1 : 0,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void bias_res_act_bf16(uintptr_t x, uintptr_t res, uintptr_t bias,
                              uintptr_t out, long n_planes, long plane,
                              int channels, bool relu,
                              uintptr_t stream_handle) {
  HIP_CHECK(ca_bias_res_act_bf16(
      cptr(x), cptr(res), cptr(bias), mptr(out), n_planes, plane, channels,
      relu ? 1 : 0, reinterpret_cast<hipStream_t>(stream_handle)));
}

static void bias_relu_maxpool_bf16(uintptr_t x, uintptr_t bias, uintptr_t out,
                                   long n_planes, int channels, int h, int w,
                                   uintptr_t stream_handle) {
  HIP_CHECK(ca_bias_relu_maxpool_bf16(
      cptr(x), cptr(bias), mptr(out), n_planes, channels, h, w,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void rmsnorm_bf16(uintptr_t x, uintptr_t w, uintptr_t out,
                         long rows, int dim, double eps,
                         uintptr_t stream_handle) {
  HIP_CHECK(ca_rmsnorm_bf16(cptr(x), cptr(w), mptr(out), rows, dim,
                            (float)eps,
                            reinterpret_cast<hipStream_t>(stream_handle)));
}

static void rope_decode_bf16(uintptr_t q, uintptr_t k, uintptr_t cos_tab,
                             uintptr_t sin_tab, uintptr_t pos, int b, int hq,
                             int hk, int d, uintptr_t stream_handle) {
  HIP_CHECK(ca_rope_decode_bf16(
      mptr(q), mptr(k), cptr(cos_tab), cptr(sin_tab), cptr(pos), b, hq, hk, d,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void rope_scatter_decode_bf16(uintptr_t q, uintptr_t k, uintptr_t v,
                                     uintptr_t ck, uintptr_t cv,
                                     uintptr_t cos_tab, uintptr_t sin_tab,
                                     uintptr_t pos, int b, int hq, int hk,
                                     int d, long cache_len, float q_scale,
                                     uintptr_t stream_handle) {
  HIP_CHECK(ca_rope_scatter_decode_bf16(
      mptr(q), cptr(k), cptr(v), mptr(ck), mptr(cv), cptr(cos_tab),
      cptr(sin_tab), cptr(pos), b, hq, hk, d, cache_len, q_scale,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void rope_scatter_decode_fp8kv_bf16(
    uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t ck, uintptr_t cv,
    uintptr_t cos_tab, uintptr_t sin_tab, uintptr_t pos, int b, int hq,
    int hk, int d, long cache_len, float q_scale, uintptr_t stream_handle) {
  HIP_CHECK(ca_rope_scatter_decode_fp8kv_bf16(
      mptr(q), cptr(k), cptr(v), mptr(ck), mptr(cv), cptr(cos_tab),
      cptr(sin_tab), cptr(pos), b, hq, hk, d, cache_len, q_scale,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static long gqa_decode_attention_workspace_bytes(int b, int hq, int d,
                                                 long max_len) {
  return ca_gqa_decode_attention_workspace_bytes(b, hq, d, max_len);
}

static void gqa_decode_attention(uintptr_t q, uintptr_t ck, uintptr_t cv,
                                 uintptr_t pos, uintptr_t out,
                                 uintptr_t workspace, long workspace_bytes,
                                 int b, int hq, int hk, int d, float scale,
                                 long max_len, long cache_len, bool kv_fp8,
                                 uintptr_t stream_handle) {
  HIP_CHECK(ca_gqa_decode_attention(
      cptr(q), cptr(ck), cptr(cv), cptr(pos), mptr(out), mptr(workspace),
      workspace_bytes, b, hq, hk, d, scale, max_len, cache_len,
      kv_fp8 ? 1 : 0, reinterpret_cast<hipStream_t>(stream_handle)));
}

static void rope_scatter_prefill_bf16(
    uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t ck, uintptr_t cv,
    uintptr_t cos_tab, uintptr_t sin_tab, uintptr_t pos, uintptr_t row_lens,
    uintptr_t row_map, int b, int c, int hq, int hk, int d, long cache_len,
    long cache_rows, float q_scale, uintptr_t stream_handle) {
  HIP_CHECK(ca_rope_scatter_prefill_bf16(
      mptr(q), cptr(k), cptr(v), mptr(ck), mptr(cv), cptr(cos_tab),
      cptr(sin_tab), cptr(pos), cptr(row_lens), cptr(row_map), b, c, hq, hk,
      d, cache_len, cache_rows, q_scale,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void rope_scatter_prefill_fp8kv_bf16(
    uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t ck, uintptr_t cv,
    uintptr_t cos_tab, uintptr_t sin_tab, uintptr_t pos, uintptr_t row_lens,
    uintptr_t row_map, int b, int c, int hq, int hk, int d, long cache_len,
    long cache_rows, float q_scale, uintptr_t stream_handle) {
  HIP_CHECK(ca_rope_scatter_prefill_fp8kv_bf16(
      mptr(q), cptr(k), cptr(v), mptr(ck), mptr(cv), cptr(cos_tab),
      cptr(sin_tab), cptr(pos), cptr(row_lens), cptr(row_map), b, c, hq, hk,
      d, cache_len, cache_rows, q_scale,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static long gqa_prefill_attention_workspace_bytes(int b, int c, int hq, int d,
                                                  long max_len) {
  return ca_gqa_prefill_attention_workspace_bytes(b, c, hq, d, max_len);
}

static void gqa_prefill_attention(uintptr_t q, uintptr_t ck, uintptr_t cv,
                                  uintptr_t pos, uintptr_t row_lens,
                                  uintptr_t row_map, uintptr_t out,
                                  uintptr_t workspace, long workspace_bytes,
                                  int b, int c, int hq, int hk, int d,
                                  float scale, long max_len, long cache_len,
                                  long cache_rows, bool kv_fp8,
                                  uintptr_t stream_handle) {
  HIP_CHECK(ca_gqa_prefill_attention(
      cptr(q), cptr(ck), cptr(cv), cptr(pos), cptr(row_lens), cptr(row_map),
      mptr(out), mptr(workspace), workspace_bytes, b, c, hq, hk, d, scale,
      max_len, cache_len, cache_rows, kv_fp8 ? 1 : 0,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

static void encoder_attention(uintptr_t qkv, uintptr_t key_mask,
                              uintptr_t kv_len, uintptr_t out, int b, int s,
                              int heads, int d, float scale,
                              uintptr_t stream_handle) {
  HIP_CHECK(ca_encoder_attention(
      cptr(qkv), cptr(key_mask), cptr(kv_len), mptr(out), b, s, heads, d,
      scale, reinterpret_cast<hipStream_t>(stream_handle)));
}

static void image_preprocess(uintptr_t src, uintptr_t dst, int ih, int iw,
                             int oh, int ow, int mode, bool out_bf16,
                             std::vector<float> mean, std::vector<float> stdev,
                             int device, bool sync) {
  if (mean.size() != 3 || stdev.size() != 3)
    throw std::runtime_error("mean/std must have 3 channels");
  hipStream_t s = get_stream(device);
  HIP_CHECK(ca_image_preprocess(cptr(src), mptr(dst), ih, iw, oh, ow, mode,
                                out_bf16 ? 1 : 0, mean.data(), stdev.data(),
                                s));
  sync_if(sync, s);
}

static void image_preprocess_batched(uintptr_t src, uintptr_t dst,
                                     int n_images, int ih, int iw, int oh,
                                     int ow, int mode, bool out_bf16,
                                     std::vector<float> mean,
                                     std::vector<float> stdev, int device,
                                     bool sync) {
  if (mean.size() != 3 || stdev.size() != 3)
    throw std::runtime_error("mean/std must have 3 channels");
  hipStream_t s = get_stream(device);
  HIP_CHECK(ca_image_preprocess_batched(
      cptr(src), mptr(dst), n_images, ih, iw, oh, ow, mode, out_bf16 ? 1 : 0,
      mean.data(), stdev.data(), s));
  sync_if(sync, s);
}

static void sample_logits_bf16(uintptr_t logits, uintptr_t temperature,
                               uintptr_t top_k, uintptr_t top_p,
                               uintptr_t seed, uintptr_t step, uintptr_t out,
                               long rows, int vocab,
                               uintptr_t stream_handle) {
  HIP_CHECK(ca_sample_logits_bf16(
      cptr(logits), cptr(temperature), cptr(top_k), cptr(top_p), cptr(seed),
      cptr(step), mptr(out), rows, vocab,
      reinterpret_cast<hipStream_t>(stream_handle)));
}

PYBIND11_MODULE(_hip_c, m) {
  m.doc() = "client_amd MI355X HIP runtime + CDNA4 kernels";
  m.def("device_count", &device_count);
  m.def("mem_info", &mem_info, py::arg("device") = 0);
  m.def("malloc", &hip_malloc, py::arg("device"), py::arg("byte_size"));
  m.def("free", &hip_free, py::arg("ptr"));
  m.def("ipc_get_mem_handle", &ipc_get_mem_handle, py::arg("ptr"));
  m.def("ipc_open_mem_handle", &ipc_open_mem_handle, py::arg("raw_handle"));
  m.def("ipc_close_mem_handle", &ipc_close_mem_handle, py::arg("ptr"));
  m.def("memcpy_h2d", &memcpy_h2d, py::arg("dst"), py::arg("src"),
        py::arg("byte_size"), py::arg("device") = 0, py::arg("sync") = true);
  m.def("memcpy_d2h", &memcpy_d2h, py::arg("src"), py::arg("byte_size"),
        py::arg("device") = 0);
  m.def("memcpy_d2h_into", &memcpy_d2h_into, py::arg("src"), py::arg("dst"),
        py::arg("byte_size"), py::arg("device") = 0);
  m.def("memcpy_d2d", &memcpy_d2d, py::arg("dst"), py::arg("src"),
        py::arg("byte_size"), py::arg("device") = 0, py::arg("sync") = true);
  m.def("stream_sync", &stream_sync, py::arg("device") = 0,
        py::arg("stream_idx") = 0);
  m.def("stream_handle", &stream_handle, py::arg("device") = 0,
        py::arg("stream_idx") = 0);
  m.def("memcpy_peer_async", &memcpy_peer_async, py::arg("dst"),
        py::arg("dst_device"), py::arg("src"), py::arg("src_device"),
        py::arg("byte_size"), py::arg("stream_idx") = 0);
  m.def("device_enable_peer_access", &device_enable_peer_access,
        py::arg("device"), py::arg("peer"));
  m.def("stream_fence", &stream_fence, py::arg("device"),
        py::arg("from_idx"), py::arg("to_idxs"));
  m.def("device_sync", &device_sync);
  m.def("cast_fp32_bf16", &cast_fp32_bf16, py::arg("src"), py::arg("dst"),
        py::arg("n"), py::arg("device") = 0, py::arg("sync") = true,
        py::arg("stream_idx") = 0);
  m.def("cast_bf16_fp32", &cast_bf16_fp32, py::arg("src"), py::arg("dst"),
        py::arg("n"), py::arg("device") = 0, py::arg("sync") = true,
        py::arg("stream_idx") = 0);
  m.def("cast_fp32_fp8e4m3", &cast_fp32_fp8e4m3, py::arg("src"), py::arg("dst"),
        py::arg("n"), py::arg("device") = 0, py::arg("sync") = true,
        py::arg("stream_idx") = 0);
  m.def("cast_fp8e4m3_fp32", &cast_fp8e4m3_fp32, py::arg("src"), py::arg("dst"),
        py::arg("n"), py::arg("device") = 0, py::arg("sync") = true,
        py::arg("stream_idx") = 0);
  m.def("bias_act_bf16", &bias_act_bf16, py::arg("x"), py::arg("bias"),
        py::arg("out"), py::arg("n_planes"), py::arg("plane"),
        py::arg("channels"), py::arg("relu"), py::arg("stream_handle"));
  m.def("conv3x3_bias_act_bf16", &conv3x3_bias_act_bf16, py::arg("x"),
        py::arg("w_packed"), py::arg("bias"), py::arg("out"), py::arg("n"),
        py::arg("c"), py::arg("k"), py::arg("h"), py::arg("w"),
        py::arg("stride"), py::arg("relu"), py::arg("stream_handle"));
  m.def("conv3x3_supported", &conv3x3_supported, py::arg("n"), py::arg("c"),
        py::arg("k"), py::arg("h"), py::arg("w"), py::arg("stride"));
  m.def("bias_res_act_bf16", &bias_res_act_bf16, py::arg("x"), py::arg("res"),
        py::arg("bias"), py::arg("out"), py::arg("n_planes"), py::arg("plane"),
        py::arg("channels"), py::arg("relu"), py::arg("stream_handle"));
  m.def("decode_gemm_bf16", &decode_gemm_bf16, py::arg("x"), py::arg("w"),
        py::arg("y"), py::arg("n"), py::arg("k"), py::arg("stream_handle"));
  m.def("fp8w_decode_gemm_bf16", &fp8w_decode_gemm_bf16, py::arg("x"),
        py::arg("codes"), py::arg("scale_exp"), py::arg("y"), py::arg("m"),
        py::arg("n"), py::arg("k"), py::arg("stream_handle"));
  m.def("fp8w_dequant_bf16", &fp8w_dequant_bf16, py::arg("codes"),
        py::arg("scale_exp"), py::arg("w_out"), py::arg("n"), py::arg("k"),
        py::arg("stream_handle"));
  m.attr("FP8W_TILE_ROWS") = FW_ROWS;
  m.attr("FP8W_TILE_K") = FW_KCHUNK;
  m.attr("FP8W_MAX_M") = FW_MAX_M;
  m.def("bias_res_act_cl_bf16", &bias_res_act_cl_bf16, py::arg("x"),
        py::arg("res"), py::arg("bias"), py::arg("out"), py::arg("n"),
        py::arg("channels"), py::arg("relu"), py::arg("stream_handle"));
  m.def("bias_relu_maxpool_bf16", &bias_relu_maxpool_bf16, py::arg("x"),
        py::arg("bias"), py::arg("out"), py::arg("n_planes"),
        py::arg("channels"), py::arg("h"), py::arg("w"),
        py::arg("stream_handle"));
  m.def("rmsnorm_bf16", &rmsnorm_bf16, py::arg("x"), py::arg("w"),
        py::arg("out"), py::arg("rows"), py::arg("dim"), py::arg("eps"),
        py::arg("stream_handle"));
  m.def("sample_logits_bf16", &sample_logits_bf16, py::arg("logits"),
        py::arg("temperature"), py::arg("top_k"), py::arg("top_p"),
        py::arg("seed"), py::arg("step"), py::arg("out"), py::arg("rows"),
        py::arg("vocab"), py::arg("stream_handle"));
  m.def("rope_decode_bf16", &rope_decode_bf16, py::arg("q"), py::arg("k"),
        py::arg("cos_tab"), py::arg("sin_tab"), py::arg("pos"), py::arg("b"),
        py::arg("hq"), py::arg("hk"), py::arg("d"),
        py::arg("stream_handle"));
  m.def("rope_scatter_decode_bf16", &rope_scatter_decode_bf16, py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("ck"), py::arg("cv"),
        py::arg("cos_tab"), py::arg("sin_tab"), py::arg("pos"), py::arg("b"),
        py::arg("hq"), py::arg("hk"), py::arg("d"), py::arg("cache_len"),
        py::arg("q_scale") = 1.0f, py::arg("stream_handle") = 0);
  m.def("rope_scatter_decode_fp8kv_bf16", &rope_scatter_decode_fp8kv_bf16,
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("ck"),
        py::arg("cv"), py::arg("cos_tab"), py::arg("sin_tab"), py::arg("pos"),
        py::arg("b"), py::arg("hq"), py::arg("hk"), py::arg("d"),
        py::arg("cache_len"), py::arg("q_scale") = 1.0f,
        py::arg("stream_handle") = 0);
  m.attr("GQA_DECODE_SPLIT") = GA_SPLIT;
  m.def("gqa_decode_attention_workspace_bytes",
        &gqa_decode_attention_workspace_bytes, py::arg("b"), py::arg("hq"),
        py::arg("d"), py::arg("max_len"));
  m.def("gqa_decode_attention", &gqa_decode_attention, py::arg("q"),
        py::arg("ck"), py::arg("cv"), py::arg("pos"), py::arg("out"),
        py::arg("workspace"), py::arg("workspace_bytes"), py::arg("b"),
        py::arg("hq"), py::arg("hk"), py::arg("d"), py::arg("scale"),
        py::arg("max_len"), py::arg("cache_len"), py::arg("kv_fp8"),
        py::arg("stream_handle"));
  m.def("rope_scatter_prefill_bf16", &rope_scatter_prefill_bf16,
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("ck"),
        py::arg("cv"), py::arg("cos_tab"), py::arg("sin_tab"), py::arg("pos"),
        py::arg("row_lens"), py::arg("row_map"), py::arg("b"), py::arg("c"),
        py::arg("hq"), py::arg("hk"), py::arg("d"), py::arg("cache_len"),
        py::arg("cache_rows"), py::arg("q_scale") = 1.0f,
        py::arg("stream_handle") = 0);
  m.def("rope_scatter_prefill_fp8kv_bf16", &rope_scatter_prefill_fp8kv_bf16,
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("ck"),
        py::arg("cv"), py::arg("cos_tab"), py::arg("sin_tab"), py::arg("pos"),
        py::arg("row_lens"), py::arg("row_map"), py::arg("b"), py::arg("c"),
        py::arg("hq"), py::arg("hk"), py::arg("d"), py::arg("cache_len"),
        py::arg("cache_rows"), py::arg("q_scale") = 1.0f,
        py::arg("stream_handle") = 0);
  m.attr("GQA_PREFILL_QTILE") = PA_QTILE;
  m.attr("GQA_PREFILL_KTILE") = PA_KTILE;
  m.def("gqa_prefill_attention_workspace_bytes",
        &gqa_prefill_attention_workspace_bytes, py::arg("b"), py::arg("c"),
        py::arg("hq"), py::arg("d"), py::arg("max_len"));
  m.def("gqa_prefill_attention", &gqa_prefill_attention, py::arg("q"),
        py::arg("ck"), py::arg("cv"), py::arg("pos"), py::arg("row_lens"),
        py::arg("row_map"), py::arg("out"), py::arg("workspace"),
        py::arg("workspace_bytes"), py::arg("b"), py::arg("c"), py::arg("hq"),
        py::arg("hk"), py::arg("d"), py::arg("scale"), py::arg("max_len"),
        py::arg("cache_len"), py::arg("cache_rows"), py::arg("kv_fp8"),
        py::arg("stream_handle"));
  m.attr("ENCODER_ATTN_QTILE") = EA_QTILE;
  m.attr("ENCODER_ATTN_KTILE") = EA_KTILE;
  m.attr("ENCODER_ATTN_KSTAGE") = EA_KSTAGE;
  m.def("encoder_attention", &encoder_attention, py::arg("qkv"),
        py::arg("key_mask"), py::arg("kv_len"), py::arg("out"), py::arg("b"),
        py::arg("s"), py::arg("heads"), py::arg("d"), py::arg("scale"),
        py::arg("stream_handle"));
  m.def("gather_pack", &gather_pack, py::arg("src"), py::arg("dst"),
        py::arg("elem_size"), py::arg("shape"), py::arg("strides"),
        py::arg("device") = 0, py::arg("sync") = true);
  m.def("image_preprocess", &image_preprocess, py::arg("src"), py::arg("dst"),
        py::arg("ih"), py::arg("iw"), py::arg("oh"), py::arg("ow"),
        py::arg("mode") = 0, py::arg("out_bf16") = false,
        py::arg("mean") = std::vector<float>{0.f, 0.f, 0.f},
        py::arg("std") = std::vector<float>{1.f, 1.f, 1.f},
        py::arg("device") = 0, py::arg("sync") = true);
  m.def("image_preprocess_batched", &image_preprocess_batched, py::arg("src"),
        py::arg("dst"), py::arg("n_images"), py::arg("ih"), py::arg("iw"),
        py::arg("oh"), py::arg("ow"), py::arg("mode") = 0,
        py::arg("out_bf16") = false,
        py::arg("mean") = std::vector<float>{0.f, 0.f, 0.f},
        py::arg("std") = std::vector<float>{1.f, 1.f, 1.f},
        py::arg("device") = 0, py::arg("sync") = true);
}
