// C ABI for the CDNA4 kernels (implemented in
// client_amd/ops/csrc/kernels.hip, one compilation unit shared with the
// Python extension). Compile your program with hipcc and add
// kernels.hip to its sources, or link the cmake `clientamd_kernels`
// target. Every launcher takes an explicit hipStream_t and returns
// hipGetLastError() — callers own synchronization.
#pragma once

#include <hip/hip_runtime_api.h>

extern "C" {

// fp32 -> bf16 wire-exact truncation pack (the tritonclient BF16 codec
// semantics, 5.2 TB/s measured on MI355X)
hipError_t ca_cast_fp32_bf16(const void* src, void* dst, long n,
                             hipStream_t stream);
// bf16 -> fp32 zero-extension unpack
hipError_t ca_cast_bf16_fp32(const void* src, void* dst, long n,
                             hipStream_t stream);
// fp32 <-> fp8 OCP e4m3fn (RNE)
hipError_t ca_cast_fp32_fp8e4m3(const void* src, void* dst, long n,
                                hipStream_t stream);
hipError_t ca_cast_fp8e4m3_fp32(const void* src, void* dst, long n,
                                hipStream_t stream);
// strided (<=4-D) -> contiguous gather; shape/strides are 4-long host
// arrays in elements
hipError_t ca_gather_pack(const void* src, void* dst, int elem_size,
                          const long* shape, const long* strides,
                          hipStream_t stream);
// u8 HWC -> bilinear resize -> normalize -> CHW fp32/bf16
// (mode 0 = (x-mean)*std, 1 = INCEPTION, 2 = VGG)
hipError_t ca_image_preprocess(const void* src, void* dst, int ih, int iw,
                               int oh, int ow, int mode, int out_bf16,
                               const float* mean, const float* stdev,
                               hipStream_t stream);
// the same for n_images same-sized images stacked contiguously -> NCHW
hipError_t ca_image_preprocess_batched(const void* src, void* dst,
                                       int n_images, int ih, int iw, int oh,
                                       int ow, int mode, int out_bf16,
                                       const float* mean, const float* stdev,
                                       hipStream_t stream);
// NCHW bf16 conv epilogue, in place allowed: out = x + bias[c], optional ReLU
hipError_t ca_bias_act_bf16(const void* x, const void* bias, void* out,
                            long n_planes, long plane, int channels,
                            int do_relu, hipStream_t stream);
// ... with a residual: out = (x + res) + bias[c], optional ReLU (res may be null)
hipError_t ca_bias_res_act_bf16(const void* x, const void* res,
                                const void* bias, void* out, long n_planes,
                                long plane, int channels, int do_relu,
                                hipStream_t stream);
// fused 3x3 conv (pad 1, stride 1|2) + bias[k] + optional ReLU, NCHW bf16,
// out of place; w_packed is [3][3][C/16][K][16] bf16, bias fp32. Returns
// hipErrorInvalidValue, without a launch, for shapes it does not support
// (C % 32, K % 64, output rows wider than 64, footprint larger than LDS).
hipError_t ca_conv3x3_bias_act_bf16(const void* x, const void* w_packed,
                                    const void* bias, void* out, int N, int C,
                                    int K, int H, int W, int stride,
                                    int do_relu, hipStream_t stream);
// ... over a channels-last (NHWC) tensor of n elements; channels % 8 == 0
hipError_t ca_bias_res_act_cl_bf16(const void* x, const void* res,
                                   const void* bias, void* out, long n,
                                   int channels, int do_relu,
                                   hipStream_t stream);
// ResNet stem: bias + ReLU + 3x3 stride-2 pad-1 max-pool, NCHW bf16
hipError_t ca_bias_relu_maxpool_bf16(const void* x, const void* bias,
                                     void* out, long n_planes, int channels,
                                     int h, int w, hipStream_t stream);
// fused bf16 RMSNorm / per-row-position decode RoPE (LLM serving)
hipError_t ca_rmsnorm_bf16(const void* x, const void* w, void* out, long rows,
                           int dim, float eps, hipStream_t stream);
hipError_t ca_rope_decode_bf16(void* q, void* k, const void* cos_tab,
                               const void* sin_tab, const void* pos, int b,
                               int hq, int hk, int d, hipStream_t stream);
// decode RoPE that also scatters rotated k and v into the KV cache
// [b, hk, cache_len, d]; q is scaled by q_scale
hipError_t ca_rope_scatter_decode_bf16(void* q, const void* k, const void* v,
                                       void* ck, void* cv,
                                       const void* cos_tab,
                                       const void* sin_tab, const void* pos,
                                       int b, int hq, int hk, int d,
                                       long cache_len, float q_scale,
                                       hipStream_t stream);
// skinny decode GEMM y[8, N] = x[8, K] @ W[N, K]^T, bf16; K % 512 == 0
hipError_t ca_decode_gemm_bf16(const void* x, const void* w, void* y, int N,
                               int K, hipStream_t stream);
// fp8 (e4m3) weight-only linear for decode: y[M, N] = x[M, K] @ W_eff^T with
// W_eff[n, k] = e4m3(codes[n, k]) * 2^scale_exp[n]; x, y bf16, scale_exp int8
// [N]; codes in the 16-row x 64-k tiled layout of weight_fp8.hip.
// 1 <= M <= 16, K % 64 == 0, x and codes 16-byte aligned; anything else
// returns hipErrorInvalidValue without a launch
hipError_t ca_fp8w_decode_gemm_bf16(const void* x, const void* codes,
                                    const void* scale_exp, void* y, int M,
                                    int N, int K, hipStream_t stream);
// the same codes -> W_eff as row-major [N, K] bf16
hipError_t ca_fp8w_dequant_bf16(const void* codes, const void* scale_exp,
                                void* w_out, int N, int K,
                                hipStream_t stream);
// token sampling from bf16 logits [rows, vocab]: per-row temperature (f32),
// top_k (i32), top_p (f32), seed (u64) and step (i64) in device memory;
// out [rows] int64
hipError_t ca_sample_logits_bf16(const void* logits, const void* temperature,
                                 const void* top_k, const void* top_p,
                                 const void* seed, const void* step, void* out,
                                 long rows, int vocab, hipStream_t stream);

}  // extern "C"
