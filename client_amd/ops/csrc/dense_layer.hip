// The two kernels of a DenseNet dense layer on a block buffer: NCHW bf16,
// fp32 accumulation on v_mfma_f32_32x32x16_bf16. Included from
// kernels.hip after conv1x1.hip, whose barrier, fragment types and
// epilogue this file shares.
//
// A dense block keeps one [N, C_end, H, W] buffer. Layer l reads its
// channel prefix [0, C_l) and appends 32 channels at [C_l, C_l + 32):
//
//   A  dense_conv1x1:     a = bf16(relu(x*scale + shift))   (norm1, ReLU)
//                         y = relu(bf16(W' a) + bias)       (conv1, norm2
//                                                folded into W' and bias)
//   B  dense_conv3x3_k32: buffer[:, C_l : C_l+32] = bf16(W2 * y)   (conv2)
//
// so the seven launches of the textbook layer (BN, ReLU, conv, BN, ReLU,
// conv, cat) become two and nothing is concatenated. Neither kernel
// splits a reduction across workgroups or uses an atomic: an output
// element is one fixed chain, so its bits do not depend on the batch,
// the image's position, the tile width or the buffer's stride.
// Geometry and every address: dense_layer_index.h.
//
// Kernel A is the conv1x1.hip pipeline (64 output channels x 64 or 128
// columns per workgroup, weight chunk and pixel-major 80-byte pixels in
// two LDS buffers, one barrier per 32-channel chunk) with two changes.
// The input's image stride is a parameter, so a tile's columns come
// from the prefix of a wider buffer. And the BN+ReLU prologue runs
// between the global load and the transposing LDS store, in the
// registers the chunk was prefetched into: the MFMAs of the previous
// chunk cover the load, and the affine map, ReLU and RNE cost no pass
// over memory. scale[C] and shift[C] are staged in LDS once per
// workgroup (8 KB at C = 1024); a staging item's eight channels are two
// 16-byte broadcast reads of each per chunk. Keeping them in registers
// would cost 16 VGPRs per item and a reload per chunk anyway, and
// scalar loads cannot follow the per-thread channel group.
//
// Kernel B has 32 output channels, so conv3x3.hip's 2 (channels) x 2
// (columns) wave layout has nothing to split: all parallelism is
// pixels, and at 7x7 and batch 8 there are 392 of them. The four waves
// of a workgroup therefore split the reduction. Wave v takes the
// 32-channel chunks v, v+4, ... (C = 128: one each), stages its chunk's
// padded footprint in an LDS region of its own, and reads its A
// fragments straight from global memory: with one 32-row block of
// output channels no other wave wants them, the packed layout makes a
// fragment one coalesced 1 KB load, and all 18 of a chunk are issued
// before the staging so they arrive under it. The four partial tiles
// meet in LDS as fp32 and are added in wave order, each wave finishing
// a quarter of the registers, then rounded once (RNE) and stored into
// the buffer's slot. Workgroups are small and many: one output row each
// until there are more than DL3_WG_TARGET of them.

#include "dense_layer_index.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float dl_f32x4;

// norm1 + ReLU of one element: fp32 fma, ReLU (a NaN stays a NaN)
C1_LAMBDA_ATTR __device__ inline float dl_bn_relu(float x, float sc,
                                                  float sh) {
  const float f = fmaf(x, sc, sh);
  return f < 0.f ? 0.f : f;
}

template <int NT, int VL, bool VS>
C1_KERNEL_ATTR __device__ __forceinline__ void dense_conv1x1_body(
    const uint16_t* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const uint16_t* __restrict__ wp,
    const float* __restrict__ bias, uint16_t* __restrict__ out,
    const DenseConv1x1Geom dg, int do_relu) {
  constexpr int BN = 64 * NT;
  constexpr int ITEMS = BN / VL * (C1_CK / 8);
  constexpr int IT = (ITEMS + C1_THREADS - 1) / C1_THREADS;
  constexpr int XW = 4 * VL;  // dwords a staging item holds
  extern __shared__ __attribute__((aligned(16))) unsigned char dl_lds[];
  const Conv1x1Geom& g = dg.c;
  float* ss = (float*)dl_lds;  // scale[C], shift[C]
  unsigned char* bufs = dl_lds + dl_ss_bytes(g.C);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1;  // 32-channel half of the 64
  const int wn = wave & 1;   // column half
  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int tile = c1_block_tile(g, blockIdx.x);
  const int m0 = c1_block_m0(g, blockIdx.x);
  const int j0 = tile * BN;
  const long hw = g.HW;

  for (int i = tid; i < 2 * g.C; i += C1_THREADS)
    ss[i] = i < g.C ? scale[i] : shift[i - g.C];

  // staging items of this thread
  long src[IT];
  int dst[IT];
  int ch8[IT];  // first of the item's eight channels within a chunk
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int it = tid + i * C1_THREADS;
    src[i] = -1;
    dst[i] = -1;
    ch8[i] = 0;
    if (it < ITEMS) {
      const int cg = c1_item_cg(g, it);
      const int col = c1_item_col(g, it);
      const long s = dl_col_src(dg, j0 + col);
      src[i] = s < 0 ? -1 : s + (long)cg * 8 * hw;
      dst[i] = c1_lds_pix(col, cg);
      ch8[i] = cg * 8;
    }
  }

  c1_u32x4 wreg;
  uint32_t xreg[IT][XW];
  auto load_chunk = [&](int c0) C1_LAMBDA_ATTR {
    wreg = *(const c1_u32x4*)(wp + c1_w_off(g, c0, m0, tid));
    const long coff = (long)c0 * hw;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
#pragma unroll
      for (int q = 0; q < XW; ++q) xreg[i][q] = 0;
      if (src[i] >= 0) {
        const uint16_t* p = x + src[i] + coff;
        if (VL == 2) {
          // dword c: pixels (col, col + 1) of channel c
#pragma unroll
          for (int c = 0; c < 8; ++c)
            xreg[i][c] = *(const uint32_t*)(p + c * hw);
        } else {
          // dword c: channels (2c, 2c + 1) of pixel col
#pragma unroll
          for (int c = 0; c < 4; ++c)
            xreg[i][c] = (uint32_t)p[(2 * c) * hw] |
                         ((uint32_t)p[(2 * c + 1) * hw] << 16);
        }
      }
    }
  };
  // prologue on the prefetched registers, then the transposing store
  auto store_chunk = [&](int c0, unsigned char* lds_a,
                         unsigned char* lds_x) C1_LAMBDA_ATTR {
    *(c1_u32x4*)(lds_a + tid * 16) = wreg;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      if (dst[i] < 0) continue;
      const float* sp = ss + c0 + ch8[i];
      const dl_f32x4 s0 = *(const dl_f32x4*)sp;
      const dl_f32x4 s1 = *(const dl_f32x4*)(sp + 4);
      const dl_f32x4 h0 = *(const dl_f32x4*)(sp + g.C);
      const dl_f32x4 h1 = *(const dl_f32x4*)(sp + g.C + 4);
      const float sc[8] = {s0[0], s0[1], s0[2], s0[3],
                           s1[0], s1[1], s1[2], s1[3]};
      const float sh[8] = {h0[0], h0[1], h0[2], h0[3],
                           h1[0], h1[1], h1[2], h1[3]};
      if (VL == 2) {
        uint32_t v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
          v[c] = f32x2_to_bf16x2_cvt(
              dl_bn_relu(bf16x2_lo(xreg[i][c]), sc[c], sh[c]),
              dl_bn_relu(bf16x2_hi(xreg[i][c]), sc[c], sh[c]));
        uint32_t a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t e = v[2 * q], o = v[2 * q + 1];
          a[q] = (e & 0xffffu) | (o << 16);
          b[q] = (e >> 16) | (o & 0xffff0000u);
        }
        *(c1_u32x4*)(lds_x + dst[i]) = c1_u32x4{a[0], a[1], a[2], a[3]};
        *(c1_u32x4*)(lds_x + dst[i] + C1_PIX_BYTES) =
            c1_u32x4{b[0], b[1], b[2], b[3]};
      } else {
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          v[q] = f32x2_to_bf16x2_cvt(
              dl_bn_relu(bf16x2_lo(xreg[i][q]), sc[2 * q], sh[2 * q]),
              dl_bn_relu(bf16x2_hi(xreg[i][q]), sc[2 * q + 1],
                         sh[2 * q + 1]));
        *(c1_u32x4*)(lds_x + dst[i]) = c1_u32x4{v[0], v[1], v[2], v[3]};
      }
    }
  };

  c1_frag_cd acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  load_chunk(0);
  c1_barrier();  // scale and shift are staged
  int buf = 0;
  for (int c0 = 0; c0 < g.C; c0 += C1_CK) {
    unsigned char* lds_a = bufs + buf * c1_buf_bytes(NT);
    unsigned char* lds_x = lds_a + C1_A_BYTES;
    // this buffer's fragment reads of two chunks ago ended before the
    // previous chunk's barrier
    store_chunk(c0, lds_a, lds_x);
    c1_barrier();
    if (c0 + C1_CK < g.C) load_chunk(c0 + C1_CK);
#pragma unroll
    for (int kk = 0; kk < C1_CK / 16; ++kk) {
      const c1_frag_ab a =
          *(const c1_frag_ab*)(lds_a + c1_lds_a(kk, wm * 32 + lr, lh));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const c1_frag_ab b = *(const c1_frag_ab*)(
            lds_x + c1_lds_pix((wn * NT + t) * 32 + lr, 2 * kk + lh));
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0,
                                                         0);
      }
    }
    buf ^= 1;
  }

  // accumulator register r of lane (lr, lh) is output channel
  // (r&3) + 8*(r>>2) + 4*lh of the wave's 32, at the lane's column.
  // No bias: adding -0.0 leaves every value, -0.0 included, as it is.
  if (VS) {
    c1_barrier();  // every fragment read is done: LDS becomes [ch][col]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        *(uint16_t*)(bufs + c1_lds_ex(g, ch, (wn * NT + t) * 32 + lr)) =
            f32_to_bf16_rne(acc[t][r]);
      }
    c1_barrier();
    // 8 columns of one channel per lane; HW % 8 == 0 keeps them in one
    // image and 16-byte aligned
    constexpr int GROUPS = BN / 8;
    const int col = (tid % GROUPS) * 8;
    const long o = c1_col_out(g, j0 + col);
    if (o < 0) return;
#pragma unroll
    for (int ch = tid / GROUPS; ch < C1_BM; ch += C1_THREADS / GROUPS) {
      const int k = m0 + ch;
      const float b = bias ? bias[k] : -0.f;
      c1_u32x4 v = *(const c1_u32x4*)(bufs + c1_lds_ex(g, ch, col));
      uint32_t* w = (uint32_t*)&v;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        w[q] = epilogue_pair(w[q], 0, false, b, b, do_relu);
      *(c1_u32x4*)(out + o + (long)k * hw) = v;
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const long o = c1_col_out(g, j0 + (wn * NT + t) * 32 + lr);
      if (o < 0) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float f = bf16_to_f32(f32_to_bf16_rne(acc[t][r]));
        out[o + (long)k * hw] =
            epilogue_finish(f + (bias ? bias[k] : -0.f), do_relu);
      }
    }
  }
}

template <int NT>
C1_KERNEL_ATTR __device__ __forceinline__ void dense_conv3x3_k32_body(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ wp,
    uint16_t* __restrict__ out, const DenseConv3x3Geom g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dl_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;  // which chunks of the reduction
  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int tile = blockIdx.x;
  const int p0 = dl3_tile_p0(g, tile);
  const int fp = dl3_tile_fp(g, tile);
  const long hw = g.HW;
  unsigned char* lds_x = dl_lds + wave * g.fp_max * DL3_PIX_BYTES;

  // this lane's columns
  int col_pix[NT];
  long col_out[NT];
  bool col_ok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    col_ok[t] = dl3_column(g, tile, t * 32 + lr, &col_pix[t], &col_out[t]);

  c1_frag_cd acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int chunks = g.C / DL3_CK;
  for (int first = 0; first < chunks; first += 4) {
    const int chunk = first + wave;  // the same for the whole wave
    const bool mine = chunk < chunks;
    // the previous round's fragment reads of this region are done
    if (first) c1_barrier();
    c1_frag_ab a[18];
    if (mine) {
#pragma unroll
      for (int f = 0; f < 18; ++f)
        a[f] = *(const c1_frag_ab*)(
            wp + dl3_w_off(g, f >> 1, chunk * 2 + (f & 1), lr, lh));
      // the chunk's footprint, transposed to [pixel][channel]; item =
      // cg * fp + pi, so consecutive lanes take consecutive pixels
      const long coff = (long)chunk * DL3_CK * hw;
      for (int it = lane; it < fp * (DL3_CK / 8); it += 64) {
        const int cg = it / fp;
        const int pi = it - cg * fp;
        const long s = dl3_stage_src(g, p0, pi);
        uint32_t w[4] = {0, 0, 0, 0};
        if (s >= 0) {
          const uint16_t* p = x + s + coff + (long)cg * 8 * hw;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            w[c] = (uint32_t)p[(2 * c) * hw] |
                   ((uint32_t)p[(2 * c + 1) * hw] << 16);
        }
        *(c1_u32x4*)(lds_x + pi * DL3_PIX_BYTES + cg * 16) =
            c1_u32x4{w[0], w[1], w[2], w[3]};
      }
    }
    c1_barrier();
    if (mine) {
#pragma unroll
      for (int f = 0; f < 18; ++f) {
        const int tap = f >> 1;
        const int tpix = (tap / 3) * g.PW + tap % 3;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const c1_frag_ab b = *(const c1_frag_ab*)(
              lds_x + (col_pix[t] + tpix) * DL3_PIX_BYTES + (f & 1) * 32 +
              lh * 16);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f], b, acc[t],
                                                           0, 0, 0);
        }
      }
    }
  }

  c1_barrier();  // every fragment read is done: LDS becomes the partials
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      *(float*)(dl_lds + dl3_red_off(NT, wave, t, r, lane)) = acc[t][r];
  c1_barrier();
  // wave v finishes registers 4v..4v+3 of every lane: the four waves'
  // partials in wave order, one rounding. Register r of lane (lr, lh) is
  // output channel (r&3) + 8*(r>>2) + 4*lh.
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (!col_ok[t]) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = wave * 4 + q;
      float s = *(const float*)(dl_lds + dl3_red_off(NT, 0, t, r, lane));
#pragma unroll
      for (int v = 1; v < 4; ++v)
        s += *(const float*)(dl_lds + dl3_red_off(NT, v, t, r, lane));
      const int k = q + 8 * wave + 4 * lh;
      out[col_out[t] + (long)k * hw] = f32_to_bf16_rne(s);
    }
  }
}

}  // namespace

#define DL_KERNEL_A(name, NT, VL, VS)                                       \
  extern "C" __global__ void C1_KERNEL_ATTR __launch_bounds__(C1_THREADS)   \
  name(                                                                     \
      const uint16_t* __restrict__ x, const float* __restrict__ scale,      \
      const float* __restrict__ shift, const uint16_t* __restrict__ wp,     \
      const float* __restrict__ bias, uint16_t* __restrict__ out,           \
      const DenseConv1x1Geom g, int do_relu) {                              \
    dense_conv1x1_body<NT, VL, VS>(x, scale, shift, wp, bias, out, g,       \
                                   do_relu);                                \
  }

// n64 / n128: columns per workgroup; s, d, v: load and store widths as in
// conv1x1.hip
DL_KERNEL_A(dense_conv1x1_n64s_bf16_kernel, 1, 1, false)
DL_KERNEL_A(dense_conv1x1_n64d_bf16_kernel, 1, 2, false)
DL_KERNEL_A(dense_conv1x1_n64v_bf16_kernel, 1, 2, true)
DL_KERNEL_A(dense_conv1x1_n128s_bf16_kernel, 2, 1, false)
DL_KERNEL_A(dense_conv1x1_n128d_bf16_kernel, 2, 2, false)
DL_KERNEL_A(dense_conv1x1_n128v_bf16_kernel, 2, 2, true)
#undef DL_KERNEL_A

#define DL_KERNEL_B(name, NT)                                               \
  extern "C" __global__ void C1_KERNEL_ATTR __launch_bounds__(DL3_THREADS)  \
  name(const uint16_t* __restrict__ x, const uint16_t* __restrict__ wp,     \
       uint16_t* __restrict__ out, const DenseConv3x3Geom g) {              \
    dense_conv3x3_k32_body<NT>(x, wp, out, g);                              \
  }

DL_KERNEL_B(dense_conv3x3_k32_n32_bf16_kernel, 1)
DL_KERNEL_B(dense_conv3x3_k32_n64_bf16_kernel, 2)
#undef DL_KERNEL_B

// true when the byte ranges [a, a + na) and [b, b + nb) share a byte
static inline bool dl_overlap(const void* a, long na, const void* b,
                              long nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// x: bf16, image n at element n*xs, channels [0, C) of it read; scale,
// shift [C] fp32; w_packed [C/16][K][16] bf16; bias null or [K] fp32; out
// dense [N,K,H,W] bf16. Shapes the kernel does not support
// (dense_layer_index.h, dl_plan_a), xs < C*H*W, pointers that are not
// aligned (weights and out: 16 bytes, x, scale, shift, bias: 4) and an
// out that overlaps what is read of x return hipErrorInvalidValue
// without a launch.
extern "C" hipError_t ca_dense_conv1x1_bf16(
    const void* x, long xs, const void* scale, const void* shift,
    const void* w_packed, const void* bias, void* out, int N, int C, int K,
    int H, int W, int do_relu, hipStream_t stream) {
  DenseConv1x1Geom g;
  if (!x || !scale || !shift || !w_packed || !out) {
    return hipErrorInvalidValue;
  }
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)out & 15) ||
      ((uintptr_t)x & 3) || ((uintptr_t)scale & 3) ||
      ((uintptr_t)shift & 3) || ((uintptr_t)bias & 3)) {
    return hipErrorInvalidValue;
  }
  if (!dl_plan_a(&g, N, C, K, H, W, xs)) return hipErrorInvalidValue;
  const long hw = (long)H * W;
  if (dl_overlap(x, ((N - 1) * xs + C * hw) * 2, out, N * K * hw * 2)) {
    return hipErrorInvalidValue;
  }
  const dim3 grid((uint32_t)((long)g.c.tiles * g.c.mrows));
  const size_t lds = (size_t)dl_a_lds_bytes(g);
#define DL_LAUNCH(name)                                                     \
  hipLaunchKernelGGL(name, grid, dim3(C1_THREADS), lds, stream,             \
                     (const uint16_t*)x, (const float*)scale,               \
                     (const float*)shift, (const uint16_t*)w_packed,        \
                     (const float*)bias, (uint16_t*)out, g, do_relu)
  if (g.c.NT == 2) {
    if (g.c.VS) DL_LAUNCH(dense_conv1x1_n128v_bf16_kernel);
    else if (g.c.VL == 2) DL_LAUNCH(dense_conv1x1_n128d_bf16_kernel);
    else DL_LAUNCH(dense_conv1x1_n128s_bf16_kernel);
  } else {
    if (g.c.VS) DL_LAUNCH(dense_conv1x1_n64v_bf16_kernel);
    else if (g.c.VL == 2) DL_LAUNCH(dense_conv1x1_n64d_bf16_kernel);
    else DL_LAUNCH(dense_conv1x1_n64s_bf16_kernel);
  }
#undef DL_LAUNCH
  return hipGetLastError();
}

// x dense [N,C,H,W] bf16; w_packed [3][3][C/16][32][16] bf16; out: bf16
// buffer with image stride os, of which only elements
// n*os + (k0 + k)*H*W + p, k < 32, are written. Unsupported shapes
// (dl_plan_b), a slot past the buffer's image (k0 + 32 > os / (H*W)),
// misaligned pointers (weights: 16 bytes, x and out: 2) and an x that
// overlaps a written slot return hipErrorInvalidValue without a launch.
extern "C" hipError_t ca_dense_conv3x3_k32_bf16(
    const void* x, const void* w_packed, void* out, int N, int C, int H,
    int W, int k0, long os, hipStream_t stream) {
  DenseConv3x3Geom g;
  if (!x || !w_packed || !out) return hipErrorInvalidValue;
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)x & 1) ||
      ((uintptr_t)out & 1)) {
    return hipErrorInvalidValue;
  }
  if (!dl_plan_b(&g, N, C, H, W, k0, os)) return hipErrorInvalidValue;
  const long hw = (long)H * W;
  for (int n = 0; n < N; ++n) {
    const uint16_t* slot = (const uint16_t*)out + n * os + k0 * hw;
    if (dl_overlap(x, (long)N * C * hw * 2, slot, DL3_K * hw * 2)) {
      return hipErrorInvalidValue;
    }
  }
  const dim3 grid((uint32_t)g.tiles);
  const size_t lds = (size_t)dl3_lds_bytes(g);
  if (g.NT == 2) {
    hipLaunchKernelGGL(dense_conv3x3_k32_n64_bf16_kernel, grid,
                       dim3(DL3_THREADS), lds, stream, (const uint16_t*)x,
                       (const uint16_t*)w_packed, (uint16_t*)out, g);
  } else {
    hipLaunchKernelGGL(dense_conv3x3_k32_n32_bf16_kernel, grid,
                       dim3(DL3_THREADS), lds, stream, (const uint16_t*)x,
                       (const uint16_t*)w_packed, (uint16_t*)out, g);
  }
  return hipGetLastError();
}
