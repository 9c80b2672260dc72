// Fused 3x3 conv (pad 1, stride 1 or 2) + bias + optional ReLU for the
// ResNet50 bottlenecks: NCHW bf16 in, NCHW bf16 out, fp32 accumulation
// on v_mfma_f32_32x32x16_bf16. Included from kernels.hip (after the
// epilogue helpers it shares with bias_act_bf16_kernel).
//
// It replaces, per conv, the library path's NCHW<->NHWC transposes of
// input, output and weights, the zero + atomic-accumulate + cast of a
// split-K fp32 workspace, and the separate bias+ReLU pass. There is no
// split of the reduction and no atomic: an output element is one fixed
// chain (channel chunks in order, taps in order, MFMA k order), so its
// bits do not depend on the batch size, the image's position or the run.
//
// GEMM view: D[k][pixel] = sum over (tap, c) of Wt[k][tap, c] * X[tap, c]
// [pixel]. The weights are the A operand (rows = output channels), the
// input the B operand (columns = pixels), so a lane of the accumulator
// holds one pixel and consecutive lanes consecutive pixels: NCHW stores
// coalesce. Geometry, tiling and every address: conv3x3_index.h.
//
// Per workgroup: 64 output channels x (64 or 128) pixel columns, 4 waves
// as 2 (channels) x 2 (columns). Per 32-channel chunk the workgroup
// stages in LDS
//   - the weight chunk, already in A-fragment order in global memory
//     ([tap][C/16][K][16], packed once per weight tensor), 36 KB;
//   - the padded input footprint as [pixel][32 channels] (the B
//     fragment wants 8 contiguous channels per pixel, NCHW is pixel-
//     contiguous, so the transpose happens at the LDS store: 8 coalesced
//     2-byte loads, one ds_write_b128). 80-byte pixels keep 16
//     consecutive pixels' ds_read_b128 on distinct banks.
// Halo pixels are stored as zeros and never addressed in global memory.

#include "conv3x3_index.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 c3_frag_ab;
typedef __attribute__((ext_vector_type(16))) float c3_frag_cd;

// fp32 accumulator -> bf16 (RNE; NaN stays a quiet NaN), then the
// epilogue of bias_act_bf16_kernel: fp32 bias add, ReLU, RNE
__device__ __forceinline__ uint16_t c3_finish(float acc, float b,
                                              int do_relu) {
  return epilogue_finish(bf16_to_f32(f32_to_bf16_rne(acc)) + b, do_relu);
}

template <int NT>
__device__ __forceinline__ void conv3x3_body(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ wp,
    const float* __restrict__ bias, uint16_t* __restrict__ out,
    const Conv3x3Geom g, int do_relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char c3_lds[];
  unsigned char* lds_a = c3_lds;
  unsigned char* lds_x = c3_lds + C3_A_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1;  // 32-channel half of the 64
  const int wn = wave & 1;   // column half
  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int tile = blockIdx.x;
  const int m0 = blockIdx.y * C3_BM;

  const int p0 = c3_tile_p0(g, tile);
  const int items = c3_tile_fp(g, tile) * (C3_CK / 8);
  const long plane_in = (long)g.H * g.W;
  const long plane_out = (long)g.OH * g.OW;

  // staging items of this thread: item = cg * fp + pi, so consecutive
  // lanes take consecutive pixels of one 8-channel group
  long src[C3_MAXIT];
  int dst[C3_MAXIT];
  {
    const int fp = items / (C3_CK / 8);
#pragma unroll
    for (int i = 0; i < C3_MAXIT; ++i) {
      const int it = tid + i * C3_THREADS;
      src[i] = -1;
      dst[i] = -1;
      if (it < items) {
        const int cg = it / fp;
        const int pi = it - cg * fp;
        const long s = c3_stage_src(g, p0, pi);
        src[i] = s < 0 ? -1 : s + (long)cg * 8 * plane_in;
        dst[i] = pi * C3_PIX_BYTES + cg * 16;
      }
    }
  }

  // this lane's columns
  int col_pix[NT];
  long col_out[NT];
  bool col_ok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = (wn * NT + t) * 32 + lr;
    col_ok[t] = c3_column(g, tile, j, &col_pix[t], &col_out[t]);
  }

  c3_frag_cd acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int kc16 = g.C / 16;
  for (int c0 = 0; c0 < g.C; c0 += C3_CK) {
    __syncthreads();  // the previous chunk's fragment reads are done
    // weights: 18 (tap, 16-channel step) pieces of 64 rows x 32 B
#pragma unroll
    for (int i = 0; i < C3_A_BYTES / 16 / C3_THREADS; ++i) {
      const int v = tid + i * C3_THREADS;  // 16-byte unit
      const int piece = v >> 7;            // 128 units per piece
      const int tap = piece >> 1;
      const int kk = piece & 1;
      const long goff =
          (((long)tap * kc16 + (c0 >> 4) + kk) * g.K + m0) * 16 +
          (long)(v & 127) * 8;
      *(uint4*)(lds_a + v * 16) = *(const uint4*)(wp + goff);
    }
    // input footprint, transposed to [pixel][channel]
    const long coff = (long)c0 * plane_in;
#pragma unroll
    for (int i = 0; i < C3_MAXIT; ++i) {
      if (dst[i] >= 0) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (src[i] >= 0) {
          const uint16_t* p = x + src[i] + coff;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            w[c] = (uint32_t)p[(2 * c) * plane_in] |
                   ((uint32_t)p[(2 * c + 1) * plane_in] << 16);
        }
        *(uint4*)(lds_x + dst[i]) = uint4{w[0], w[1], w[2], w[3]};
      }
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int tpix = c3_tap_pix(g, tap / 3, tap % 3);
#pragma unroll
      for (int kk = 0; kk < C3_CK / 16; ++kk) {
        const c3_frag_ab a = *(const c3_frag_ab*)(
            lds_a + (((tap * 2 + kk) * C3_BM + wm * 32 + lr) * 16 + lh * 8) *
                        2);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const c3_frag_ab b = *(const c3_frag_ab*)(
              lds_x + (col_pix[t] + tpix) * C3_PIX_BYTES + kk * 32 +
              lh * 16);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0,
                                                           0, 0);
        }
      }
    }
  }

  // accumulator register r of lane (lr, lh) is output channel
  // (r&3) + 8*(r>>2) + 4*lh of the wave's 32, at the lane's pixel
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (!col_ok[t]) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      out[col_out[t] + k * plane_out] = c3_finish(acc[t][r], bias[k], do_relu);
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(C3_THREADS)
conv3x3_bias_act_n64_bf16_kernel(const uint16_t* __restrict__ x,
                                 const uint16_t* __restrict__ wp,
                                 const float* __restrict__ bias,
                                 uint16_t* __restrict__ out,
                                 const Conv3x3Geom g, int do_relu) {
  conv3x3_body<1>(x, wp, bias, out, g, do_relu);
}

extern "C" __global__ void __launch_bounds__(C3_THREADS)
conv3x3_bias_act_n128_bf16_kernel(const uint16_t* __restrict__ x,
                                  const uint16_t* __restrict__ wp,
                                  const float* __restrict__ bias,
                                  uint16_t* __restrict__ out,
                                  const Conv3x3Geom g, int do_relu) {
  conv3x3_body<2>(x, wp, bias, out, g, do_relu);
}

// x [N,C,H,W] bf16, w_packed [3][3][C/16][K][16] bf16 (from the
// [K][C][3][3] weight), bias [K] fp32, out [N,K,OH,OW] bf16, out of
// place. Shapes the kernel does not support (conv3x3_index.h, c3_plan)
// return hipErrorInvalidValue without a launch.
extern "C" hipError_t ca_conv3x3_bias_act_bf16(
    const void* x, const void* w_packed, const void* bias, void* out, int N,
    int C, int K, int H, int W, int stride, int do_relu,
    hipStream_t stream) {
  Conv3x3Geom g;
  if (!x || !w_packed || !bias || !out || x == out) {
    return hipErrorInvalidValue;
  }
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)x & 1) ||
      ((uintptr_t)out & 1) || ((uintptr_t)bias & 3)) {
    return hipErrorInvalidValue;
  }
  if (!c3_plan(&g, N, C, K, H, W, stride)) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)g.tiles, (uint32_t)(K / C3_BM));
  const size_t lds = (size_t)C3_A_BYTES + (size_t)g.fp_max * C3_PIX_BYTES;
  if (g.NT == 2) {
    hipLaunchKernelGGL(conv3x3_bias_act_n128_bf16_kernel, grid,
                       dim3(C3_THREADS), lds, stream, (const uint16_t*)x,
                       (const uint16_t*)w_packed, (const float*)bias,
                       (uint16_t*)out, g, do_relu);
  } else {
    hipLaunchKernelGGL(conv3x3_bias_act_n64_bf16_kernel, grid,
                       dim3(C3_THREADS), lds, stream, (const uint16_t*)x,
                       (const uint16_t*)w_packed, (const float*)bias,
                       (uint16_t*)out, g, do_relu);
  }
  return hipGetLastError();
}
