// client_amd CDNA4 kernels — single compilation unit shared by the
// Python extension (_hip_c) and the C++ client library. All launchers
// are C ABI taking an explicit hipStream_t so both stacks compose the
// kernels with their own streams/graphs. See client_amd/ops/csrc
// provenance comments on each kernel.
//
// Kernel bodies shared between entry points are templates; each
// launched kernel is a thin extern "C" entry point around its body so
// the symbol names in rocprofv3 traces stay stable.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>

#include <cstdint>

namespace {

inline int ca_grid_for(long work_items) {
  // memory-bound streaming grid: cap at 2048 workgroups, grid-stride
  // the rest (256 CUs x 8 blocks/CU)
  long blocks = (work_items + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// ---------------------------------------------------------------------------
// bf16 helpers. Two float -> bf16 roundings live in this file and must
// not be mixed: truncation for the wire codec, round-to-nearest-even
// everywhere else (the integer formula in the decode-GEMM, attention
// and conv3x3 kernels, the hardware convert in the epilogue and stem
// kernels). rmsnorm_bf16_kernel and the RoPE kernels round with the
// __float2bfloat16 intrinsic. All the RNE forms give a NaN for every
// NaN; which NaN (payload) is not pinned.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float bf16_to_f32(uint16_t h) {
  return __uint_as_float((uint32_t)h << 16);
}

// truncation (keep the high 16 bits) — byte-exact with the wire codec
// in client_amd.utils.serialize_bf16_tensor (reference semantics:
// utils/__init__.py:294-330)
__device__ __forceinline__ uint16_t f32_to_bf16_trunc(float f) {
  return (uint16_t)(__float_as_uint(f) >> 16);
}

// round-to-nearest-even (matches torch float->bf16 casts). A NaN stays
// a NaN of its sign, made quiet: the rounding add alone would carry a
// payload of 0x7F8000 and above (an fp32 bias can hold one, and fp32
// adds propagate it) through the exponent into the sign bit and store
// 0x7FFFFFFF as -0.0.
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  const uint16_t nan = (uint16_t)((u >> 16) | 0x0040u);
  const bool is_nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
  u += 0x7FFF + ((u >> 16) & 1);
  return is_nan ? nan : (uint16_t)(u >> 16);
}

// The same rounding by gfx950's packed convert (v_cvt_pk_bf16_f32: RNE,
// NaN stays NaN), one instruction per pair. The bandwidth-bound
// epilogues use it: there the integer formula with its NaN guard
// measured 2.5-8 % slower per call than without the guard.
typedef float ca_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 ca_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint16_t f32_to_bf16_cvt(float f) {
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}
// (lo, hi) -> packed u32, low half = lower address
__device__ __forceinline__ uint32_t f32x2_to_bf16x2_cvt(float lo, float hi) {
  const ca_f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, ca_bf16x2));
}

// the two bf16 halves of a packed u32 (low half = lower address)
__device__ __forceinline__ float bf16x2_lo(uint32_t w) {
  return __uint_as_float((w & 0xFFFFu) << 16);
}
__device__ __forceinline__ float bf16x2_hi(uint32_t w) {
  return __uint_as_float(w & 0xFFFF0000u);
}

}  // namespace

// ---------------------------------------------------------------------------
// Streaming casts
// ---------------------------------------------------------------------------

namespace {

// A conversion trait names the source and destination element types,
// the per-element convert, and how many elements a lane moves per
// iteration of the vector kernel.

// fp32 -> bf16 by truncation. 16 elems/lane (64 B loads, 32 B stores
// per lane per iteration) — measured against an 8-elem kernel on
// hardware.
struct CastF32ToBf16 {
  using Src = float;
  using Dst = uint16_t;
  static constexpr int kPerLane = 16;
  static __device__ __forceinline__ Dst convert(Src v) {
    return f32_to_bf16_trunc(v);
  }
};

// bf16 -> fp32 by zero-extension (wire-exact inverse).
struct CastBf16ToF32 {
  using Src = uint16_t;
  using Dst = float;
  static constexpr int kPerLane = 8;
  static __device__ __forceinline__ Dst convert(Src v) {
    return bf16_to_f32(v);
  }
};

// fp32 -> fp8 e4m3 (OCP fn, the CDNA4-native format — NOT MI300X fnuz;
// cdna_hip_programming.md §4). RNE via the __hip_fp8_e4m3 HW convert.
// Contract (tests/kernel_refs.py:fp8_e4m3_encode is the executable form):
//   - round to nearest, ties to the even code; subnormal step 2^-9;
//   - __hip_fp8_e4m3 converts with __HIP_SATFINITE: finite inputs whose
//     magnitude rounds above 448 SATURATE to +-448 (0x7E / 0xFE). This
//     differs from torch.float8_e4m3fn, which yields NaN above 464;
//   - NaN and +-Inf pass through the clamp and give a NaN code
//     ((code & 0x7F) == 0x7F);
//   - the sign of a zero result is preserved.
struct CastF32ToFp8 {
  using Src = float;
  using Dst = uint8_t;
  static constexpr int kPerLane = 8;
  static __device__ __forceinline__ Dst convert(Src v) {
    return __hip_fp8_e4m3(v).__x;
  }
};

struct CastFp8ToF32 {
  using Src = uint8_t;
  using Dst = float;
  static constexpr int kPerLane = 8;
  static __device__ __forceinline__ Dst convert(Src v) {
    __hip_fp8_e4m3 e;
    e.__x = v;
    return float(e);
  }
};

// moves BYTES between a lane's registers and global memory in 16-byte
// accesses (one 8-byte access for the 8 x fp8 side)
template <int BYTES>
__device__ __forceinline__ void copy_wide(void* dst, const void* src) {
  if constexpr (BYTES == 8) {
    *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(src);
  } else {
    static_assert(BYTES % 16 == 0, "whole 16-byte vectors");
#pragma unroll
    for (int k = 0; k < BYTES / 16; ++k)
      reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(src)[k];
  }
}

// Vector path (src and dst 16-byte aligned): grid-stride over groups of
// kPerLane elements, then the first lanes of the grid do the ragged tail.
template <typename C>
__device__ __forceinline__ void cast_vec_body(
    const typename C::Src* __restrict__ src,
    typename C::Dst* __restrict__ dst, long n) {
  constexpr int W = C::kPerLane;
  long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * W;
  long stride = (long)gridDim.x * blockDim.x * W;
  for (long i = i0; i + W <= n; i += stride) {
    alignas(16) typename C::Src in[W];
    alignas(16) typename C::Dst out[W];
    copy_wide<W * sizeof(typename C::Src)>(in, src + i);
#pragma unroll
    for (int j = 0; j < W; ++j) out[j] = C::convert(in[j]);
    copy_wide<W * sizeof(typename C::Dst)>(dst + i, out);
  }
  // tail (grid-stride tail handling: only the lanes owning the ragged end)
  long tail_start = (n / W) * W;
  long ti = tail_start + (blockIdx.x * blockDim.x + threadIdx.x);
  if (ti < n && (blockIdx.x * blockDim.x + threadIdx.x) < W) {
    dst[ti] = C::convert(src[ti]);
  }
}

// Scalar fallback for pointers not 16-byte aligned (region offsets are
// caller-controlled; hipMalloc bases are 256-B aligned so the vector
// path is the common case).
template <typename C>
__device__ __forceinline__ void cast_scalar_body(
    const typename C::Src* __restrict__ src,
    typename C::Dst* __restrict__ dst, long n) {
  long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = C::convert(src[i]);
}

}  // namespace

// (the fp32 -> bf16 vector kernel keeps the "_v2" of the A/B comparison
// it won, so profiler tables stay comparable)
extern "C" __global__ void cast_fp32_bf16_v2_kernel(
    const float* __restrict__ src, uint16_t* __restrict__ dst, long n) {
  cast_vec_body<CastF32ToBf16>(src, dst, n);
}

extern "C" __global__ void cast_fp32_bf16_scalar_kernel(
    const float* __restrict__ src, uint16_t* __restrict__ dst, long n) {
  cast_scalar_body<CastF32ToBf16>(src, dst, n);
}

extern "C" __global__ void cast_bf16_fp32_kernel(
    const uint16_t* __restrict__ src, float* __restrict__ dst, long n) {
  cast_vec_body<CastBf16ToF32>(src, dst, n);
}

extern "C" __global__ void cast_bf16_fp32_scalar_kernel(
    const uint16_t* __restrict__ src, float* __restrict__ dst, long n) {
  cast_scalar_body<CastBf16ToF32>(src, dst, n);
}

extern "C" __global__ void cast_fp32_fp8e4m3_kernel(
    const float* __restrict__ src, uint8_t* __restrict__ dst, long n) {
  cast_vec_body<CastF32ToFp8>(src, dst, n);
}

extern "C" __global__ void cast_fp32_fp8e4m3_scalar_kernel(
    const float* __restrict__ src, uint8_t* __restrict__ dst, long n) {
  cast_scalar_body<CastF32ToFp8>(src, dst, n);
}

extern "C" __global__ void cast_fp8e4m3_fp32_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, long n) {
  cast_vec_body<CastFp8ToF32>(src, dst, n);
}

extern "C" __global__ void cast_fp8e4m3_fp32_scalar_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, long n) {
  cast_scalar_body<CastFp8ToF32>(src, dst, n);
}

namespace {

// alignment dispatch shared by the four ca_cast_* launchers
template <typename C>
hipError_t ca_launch_cast(
    void (*vec_kernel)(const typename C::Src*, typename C::Dst*, long),
    void (*scalar_kernel)(const typename C::Src*, typename C::Dst*, long),
    const void* src, void* dst, long n, hipStream_t stream) {
  const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const long work = aligned ? (n + C::kPerLane - 1) / C::kPerLane : n;
  hipLaunchKernelGGL(aligned ? vec_kernel : scalar_kernel,
                     dim3(ca_grid_for(work)), dim3(256), 0, stream,
                     (const typename C::Src*)src, (typename C::Dst*)dst, n);
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t ca_cast_fp32_bf16(const void* src, void* dst, long n,
                                        hipStream_t stream) {
  return ca_launch_cast<CastF32ToBf16>(cast_fp32_bf16_v2_kernel,
                                       cast_fp32_bf16_scalar_kernel, src, dst,
                                       n, stream);
}

extern "C" hipError_t ca_cast_bf16_fp32(const void* src, void* dst, long n,
                                        hipStream_t stream) {
  return ca_launch_cast<CastBf16ToF32>(cast_bf16_fp32_kernel,
                                       cast_bf16_fp32_scalar_kernel, src, dst,
                                       n, stream);
}

extern "C" hipError_t ca_cast_fp32_fp8e4m3(const void* src, void* dst, long n,
                                           hipStream_t stream) {
  return ca_launch_cast<CastF32ToFp8>(cast_fp32_fp8e4m3_kernel,
                                      cast_fp32_fp8e4m3_scalar_kernel, src,
                                      dst, n, stream);
}

extern "C" hipError_t ca_cast_fp8e4m3_fp32(const void* src, void* dst, long n,
                                           hipStream_t stream) {
  return ca_launch_cast<CastFp8ToF32>(cast_fp8e4m3_fp32_kernel,
                                      cast_fp8e4m3_fp32_scalar_kernel, src,
                                      dst, n, stream);
}

// ---------------------------------------------------------------------------
// Strided gather / tiled transpose
// ---------------------------------------------------------------------------

// Strided -> contiguous gather (up to 4-D), element size 1/2/4/8 bytes.
// Lifts the reference's "DLPack tensor must be contiguous" restriction
// (cuda_shared_memory/__init__.py:345-352) with a device-side pack.
template <typename T>
__global__ void gather_pack_kernel(const char* __restrict__ src,
                                   T* __restrict__ dst, long n,
                                   long s0, long s1, long s2, long s3,
                                   long d0, long d1, long d2, long d3) {
  long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    long rem = i;
    long i3 = rem % d3; rem /= d3;
    long i2 = rem % d2; rem /= d2;
    long i1 = rem % d1; rem /= d1;
    long i0 = rem;
    const char* p = src + ((i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3) * (long)sizeof(T));
    dst[i] = *reinterpret_cast<const T*>(p);
  }
}

// LDS-tiled batched transpose: the gather_pack fast path for the
// pattern "innermost output dim is strided in the source, the dim
// before it is contiguous" (a transpose view, the worst case for the
// naive per-element kernel: 729 GB/s vs ~5 TB/s for contiguous casts —
// profiles/kernels_rocprof_r01.txt:18). 64x64 tile staged through LDS:
// loads coalesce along the source's contiguous dim, stores along the
// destination's, both full 64-lane wavefronts. +1 column pad keeps the
// LDS column reads conflict-free.
//
//   dst[b0][b1][r][c] = src[b0*s0 + b1*s1 + r + c*col_stride]
//   (r = contiguous source dim of extent rows; c of extent cols;
//    blockIdx.z enumerates the flattened (b0, b1) outer batch)
#define CA_TILE 64
template <typename T>
__global__ void transpose_tiled_kernel(const T* __restrict__ src,
                                       T* __restrict__ dst, long rows,
                                       long cols, long col_stride, long s0,
                                       long s1, long d1) {
  __shared__ T tile[CA_TILE][CA_TILE + 1];
  const long batch = blockIdx.z;
  const T* sb = src + (batch / d1) * s0 + (batch % d1) * s1;
  T* db = dst + batch * rows * cols;
  const long r0 = (long)blockIdx.x * CA_TILE;  // along rows (src-contig)
  const long c0 = (long)blockIdx.y * CA_TILE;  // along cols (dst-contig)
  const int tx = threadIdx.x % CA_TILE;        // fast lane index
  const int ty0 = threadIdx.x / CA_TILE;       // 4 rows/pass with 256 thr
  // load: lanes sweep the contiguous source dim (r), rows of the tile
  // are different c values
  for (int ty = ty0; ty < CA_TILE; ty += blockDim.x / CA_TILE) {
    const long c = c0 + ty;
    const long r = r0 + tx;
    if (r < rows && c < cols) {
      tile[ty][tx] = sb[r + c * col_stride];
    }
  }
  __syncthreads();
  // store: lanes sweep the contiguous destination dim (c)
  for (int ty = ty0; ty < CA_TILE; ty += blockDim.x / CA_TILE) {
    const long r = r0 + ty;
    const long c = c0 + tx;
    if (r < rows && c < cols) {
      db[r * cols + c] = tile[tx][ty];
    }
  }
}

// 2-byte specialization of the tiled transpose: each lane moves a PAIR
// of elements (u32) in both phases, restoring full bus width (the
// generic u16 path measured 2.3 TB/s vs 4.2 for fp32). Layout per
// 64x64 tile: load phase writes u32 pairs along the source-contiguous
// dim; store phase reads two adjacent tile rows and packs a u32 along
// the destination-contiguous dim. Ragged tile edges (odd rows/cols,
// partial tiles) are handled in the kernel by the single-element
// branches. The u32 global accesses need 4-byte alignment: r, c and the
// tile origins are even, so the launcher selects this kernel only when
// src and dst are 4-byte aligned and col_stride, s0, s1 and cols are
// even; everything else goes to transpose_tiled_kernel<uint16_t>.
extern "C" __global__ void transpose_tiled_pair16_kernel(
    const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, long rows,
    long cols, long col_stride, long s0, long s1, long d1) {
  __shared__ uint16_t tile[CA_TILE][CA_TILE + 2];
  const long batch = blockIdx.z;
  const uint16_t* sb = src + (batch / d1) * s0 + (batch % d1) * s1;
  uint16_t* db = dst + batch * rows * cols;
  const long r0 = (long)blockIdx.x * CA_TILE;
  const long c0 = (long)blockIdx.y * CA_TILE;
  const int tp = threadIdx.x % 32;   // pair index along the fast dim
  const int ty0 = threadIdx.x / 32;  // 8 slow-dim rows per pass
  // load: pairs along r (source-contiguous)
  for (int ty = ty0; ty < CA_TILE; ty += 8) {
    const long c = c0 + ty;
    const long r = r0 + 2 * tp;
    if (c < cols && r + 1 < rows) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(
          sb + r + c * col_stride);
      *reinterpret_cast<uint32_t*>(&tile[ty][2 * tp]) = v;
    } else if (c < cols && r < rows) {
      tile[ty][2 * tp] = sb[r + c * col_stride];
    }
  }
  __syncthreads();
  // store: pairs along c (destination-contiguous)
  for (int ty = ty0; ty < CA_TILE; ty += 8) {
    const long r = r0 + ty;
    const long c = c0 + 2 * tp;
    if (r < rows && c + 1 < cols) {
      uint32_t v = (uint32_t)tile[2 * tp][ty] |
                   ((uint32_t)tile[2 * tp + 1][ty] << 16);
      *reinterpret_cast<uint32_t*>(db + r * cols + c) = v;
    } else if (r < rows && c < cols) {
      db[r * cols + c] = tile[2 * tp][ty];
    }
  }
}

namespace {

// launches the tiled transpose or the per-element gather for one
// element type
template <typename T>
hipError_t ca_gather_pack_launch(const void* src, void* dst,
                                 const long* shape, const long* strides,
                                 bool tiled, hipStream_t stream) {
  if (!tiled) {
    const long n = shape[0] * shape[1] * shape[2] * shape[3];
    hipLaunchKernelGGL((gather_pack_kernel<T>), dim3(ca_grid_for(n)),
                       dim3(256), 0, stream, (const char*)src, (T*)dst, n,
                       strides[0], strides[1], strides[2], strides[3],
                       shape[0], shape[1], shape[2], shape[3]);
    return hipGetLastError();
  }
  const long rows = shape[2], cols = shape[3];
  dim3 grid((uint32_t)((rows + CA_TILE - 1) / CA_TILE),
            (uint32_t)((cols + CA_TILE - 1) / CA_TILE),
            (uint32_t)(shape[0] * shape[1]));
  bool pair_aligned = false;
  if constexpr (sizeof(T) == 2) {
    // pair-per-lane variant restores full bus width for 2-byte
    // elements (u16 path: 2.3 TB/s; fp32: 4.2). Its u32 accesses
    // are aligned only for 4-byte-aligned bases and even element
    // offsets; any odd stride/extent/base takes the u16 kernel.
    pair_aligned =
        (((uintptr_t)src | (uintptr_t)dst) & 3) == 0 &&
        ((strides[3] | strides[0] | strides[1] | cols) & 1) == 0;
  }
  if (pair_aligned) {
    hipLaunchKernelGGL(transpose_tiled_pair16_kernel, grid, dim3(256), 0,
                       stream, (const uint16_t*)src, (uint16_t*)dst, rows,
                       cols, strides[3], strides[0], strides[1], shape[1]);
  } else {
    hipLaunchKernelGGL((transpose_tiled_kernel<T>), grid, dim3(256), 0,
                       stream, (const T*)src, (T*)dst, rows, cols, strides[3],
                       strides[0], strides[1], shape[1]);
  }
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t ca_gather_pack(const void* src, void* dst,
                                     int elem_size, const long* shape,
                                     const long* strides,
                                     hipStream_t stream) {
  // shape/strides are 4-element host arrays (leading dims padded)
  // transpose-like fast path: dim 2 contiguous in the source, innermost
  // output dim strided -> LDS-tiled transpose (coalesced both ways;
  // the naive per-element path was 7x off peak on this pattern,
  // profiles/kernels_rocprof_r01.txt:18)
  const bool tiled = strides[2] == 1 && strides[3] != 1 && shape[2] >= 16 &&
                     shape[3] >= 16 && shape[0] * shape[1] <= 65535 &&
                     (shape[3] + CA_TILE - 1) / CA_TILE <= 65535;
  switch (elem_size) {
    case 1:
      return ca_gather_pack_launch<uint8_t>(src, dst, shape, strides, tiled,
                                            stream);
    case 2:
      return ca_gather_pack_launch<uint16_t>(src, dst, shape, strides, tiled,
                                             stream);
    case 4:
      return ca_gather_pack_launch<uint32_t>(src, dst, shape, strides, tiled,
                                             stream);
    case 8:
      return ca_gather_pack_launch<uint64_t>(src, dst, shape, strides, tiled,
                                             stream);
    default:
      return hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------
// Image preprocess
// ---------------------------------------------------------------------------

namespace {

// Image preprocess: u8 HWC (ih,iw,3) -> bilinear resize (oh,ow) ->
// normalize -> planar CHW fp32 (or bf16). One thread per output pixel
// computes all 3 channels (reads coalesce along ow; the 4 source pixels
// hit L1/L2 for neighbors). Modes: 0 = raw /1, 1 = INCEPTION
// (x/127.5 - 1), 2 = VGG (x - mean_c), matching image_client.cc:86-190.
//
// One image: simg is its u8 input, dimg / dimg16 the same CHW output
// viewed as fp32 / bf16, n = oh * ow its pixel count; the grid's x
// dimension strides over pixels starting at i.
__device__ __forceinline__ void image_preprocess_body(
    const uint8_t* __restrict__ simg, float* __restrict__ dimg,
    uint16_t* __restrict__ dimg16, const long n, long i, const long stride,
    int ih, int iw, int oh, int ow, int mode, int out_bf16, float m0,
    float m1, float m2, float s0, float s1, float s2) {
  const float scale_h = (float)ih / oh;
  const float scale_w = (float)iw / ow;
  for (; i < n; i += stride) {
    int oy = i / ow;
    int ox = i % ow;
    float fy = (oy + 0.5f) * scale_h - 0.5f;
    float fx = (ox + 0.5f) * scale_w - 0.5f;
    int y0 = max(0, (int)floorf(fy));
    int x0 = max(0, (int)floorf(fx));
    int y1 = min(ih - 1, y0 + 1);
    int x1 = min(iw - 1, x0 + 1);
    y0 = min(y0, ih - 1);
    x0 = min(x0, iw - 1);
    float wy = fy - floorf(fy);
    float wx = fx - floorf(fx);
    if (fy < 0) wy = 0.f;
    if (fx < 0) wx = 0.f;
    const uint8_t* p00 = simg + ((long)y0 * iw + x0) * 3;
    const uint8_t* p01 = simg + ((long)y0 * iw + x1) * 3;
    const uint8_t* p10 = simg + ((long)y1 * iw + x0) * 3;
    const uint8_t* p11 = simg + ((long)y1 * iw + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = (1 - wy) * ((1 - wx) * p00[c] + wx * p01[c]) +
                wy * ((1 - wx) * p10[c] + wx * p11[c]);
      float mean = c == 0 ? m0 : (c == 1 ? m1 : m2);
      float sc = c == 0 ? s0 : (c == 1 ? s1 : s2);
      if (mode == 1) {
        v = v / 127.5f - 1.0f;
      } else if (mode == 2) {
        v = v - mean;
      } else {
        v = (v - mean) * sc;
      }
      long out_idx = (long)c * n + i;  // CHW within the image
      if (out_bf16) {
        dimg16[out_idx] = f32_to_bf16_trunc(v);
      } else {
        dimg[out_idx] = v;
      }
    }
  }
}

}  // namespace

// One image per launch. Kept apart from the batched kernel below: run
// through that one, a single image pays the blockIdx.y offset
// arithmetic in the prologue, +0.24-0.28 us on a 2.9-3.4 us kernel
// (docs/PERFORMANCE.md, "Kernel file deduplication").
extern "C" __global__ void image_preprocess_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst,
    int ih, int iw, int oh, int ow, int mode, int out_bf16,
    float m0, float m1, float m2, float s0, float s1, float s2) {
  const long n = (long)oh * ow;
  const long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  image_preprocess_body(src, dst, reinterpret_cast<uint16_t*>(dst), n, i,
                        stride, ih, iw, oh, ow, mode, out_bf16, m0, m1, m2,
                        s0, s1, s2);
}

extern "C" hipError_t ca_image_preprocess(const void* src, void* dst, int ih,
                                          int iw, int oh, int ow, int mode,
                                          int out_bf16, const float* mean,
                                          const float* stdev,
                                          hipStream_t stream) {
  hipLaunchKernelGGL(image_preprocess_kernel,
                     dim3(ca_grid_for((long)oh * ow)), dim3(256), 0, stream,
                     (const uint8_t*)src, (float*)dst, ih, iw, oh, ow, mode,
                     out_bf16, mean[0], mean[1], mean[2], stdev[0], stdev[1],
                     stdev[2]);
  return hipGetLastError();
}

// Batched variant: N same-sized images in one launch (u8 HWC stacked
// contiguously -> NCHW). The single-image kernel is launch-bound at
// high request rates (~27 us/image vs ~2-3 us of kernel time for
// 224x224 — profiles/kernels_rocprof_r01.txt:19); the batch amortizes
// one launch over the whole request. blockIdx.y = image index (grid.y
// caps at 65535 — far above any sane batch).
extern "C" __global__ void image_preprocess_batched_kernel(
    const uint8_t* __restrict__ src, float* __restrict__ dst, int ih, int iw,
    int oh, int ow, int mode, int out_bf16, float m0, float m1, float m2,
    float s0, float s1, float s2) {
  const long in_img = (long)ih * iw * 3;
  const long n = (long)oh * ow;
  const uint8_t* simg = src + (long)blockIdx.y * in_img;
  float* dimg = dst + (long)blockIdx.y * 3 * n;
  uint16_t* dimg16 =
      reinterpret_cast<uint16_t*>(dst) + (long)blockIdx.y * 3 * n;
  const long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  image_preprocess_body(simg, dimg, dimg16, n, i, stride, ih, iw, oh, ow,
                        mode, out_bf16, m0, m1, m2, s0, s1, s2);
}

extern "C" hipError_t ca_image_preprocess_batched(
    const void* src, void* dst, int n_images, int ih, int iw, int oh, int ow,
    int mode, int out_bf16, const float* mean, const float* stdev,
    hipStream_t stream) {
  if (n_images < 1 || n_images > 65535) return hipErrorInvalidValue;
  dim3 grid((uint32_t)ca_grid_for((long)oh * ow), (uint32_t)n_images);
  hipLaunchKernelGGL(image_preprocess_batched_kernel, grid, dim3(256), 0,
                     stream, (const uint8_t*)src, (float*)dst, ih, iw, oh,
                     ow, mode, out_bf16, mean[0], mean[1], mean[2], stdev[0],
                     stdev[1], stdev[2]);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// LLM decode kernels
// ---------------------------------------------------------------------------

// Fused RMSNorm for bf16 rows: out = x * rsqrt(mean(x^2)+eps) * w,
// computed in fp32 (byte-compatible with the torch reference sequence
// float() -> pow/mean/rsqrt -> mul -> to(bf16), which launches ~7
// kernels; this is one). One workgroup per row; dim must be a multiple
// of 8 for the vectorized loads (4096/1024/... in practice).
extern "C" __global__ void rmsnorm_bf16_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
    uint16_t* __restrict__ out, int dim, float eps) {
  const int row = blockIdx.x;
  const uint16_t* xr = x + (long)row * dim;
  uint16_t* outr = out + (long)row * dim;
  float acc = 0.f;
  for (int i = threadIdx.x * 8; i < dim; i += blockDim.x * 8) {
    uint4 v = *reinterpret_cast<const uint4*>(xr + i);
    const uint16_t* e = reinterpret_cast<const uint16_t*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_to_f32(e[j]);
      acc += f * f;
    }
  }
  // wave + LDS reduction (64-wide waves)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  __shared__ float warp_sums[16];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) warp_sums[wave] = acc;
  __syncthreads();
  const int n_waves = (blockDim.x + 63) >> 6;
  if (threadIdx.x == 0) {
    float total = 0.f;
    for (int i = 0; i < n_waves; ++i) total += warp_sums[i];
    warp_sums[0] = rsqrtf(total / dim + eps);
  }
  __syncthreads();
  const float scale = warp_sums[0];
  for (int i = threadIdx.x * 8; i < dim; i += blockDim.x * 8) {
    uint4 v = *reinterpret_cast<const uint4*>(xr + i);
    uint4 wv = *reinterpret_cast<const uint4*>(w + i);
    const uint16_t* e = reinterpret_cast<const uint16_t*>(&v);
    const uint16_t* we = reinterpret_cast<const uint16_t*>(&wv);
    uint16_t o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_to_f32(e[j]);
      float wf = bf16_to_f32(we[j]);
      o[j] = __bfloat16_as_ushort(__float2bfloat16(f * scale * wf));
    }
    *reinterpret_cast<uint4*>(outr + i) = *reinterpret_cast<uint4*>(o);
  }
}

extern "C" hipError_t ca_rmsnorm_bf16(const void* x, const void* w, void* out,
                                      long rows, int dim, float eps,
                                      hipStream_t stream) {
  if (dim % 8 != 0) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;  // nothing to do; a zero grid is invalid
  hipLaunchKernelGGL(rmsnorm_bf16_kernel, dim3((uint32_t)rows), dim3(256), 0,
                     stream, (const uint16_t*)x, (const uint16_t*)w,
                     (uint16_t*)out, dim, eps);
  return hipGetLastError();
}

namespace {

// Rotates the bf16 pair src[2j], src[2j+1] by the angle (c, s), scales
// it, and writes it to dst[2j], dst[2j+1] (dst may be src). The x2
// products are rounded and the x1 products fused, written out so that
// every kernel that rotates gives the same bits whatever the compiler
// would contract around it (the prefill scatter must match the decode
// scatter bit for bit).
__device__ __forceinline__ void rope_rotate_pair(const uint16_t* src,
                                                 uint16_t* dst, int j,
                                                 float c, float s,
                                                 float scale) {
  const float x1 = bf16_to_f32(src[2 * j]);
  const float x2 = bf16_to_f32(src[2 * j + 1]);
  const float r1 = fmaf(x1, c, -(x2 * s));
  const float r2 = fmaf(x1, s, x2 * c);
  dst[2 * j] = __bfloat16_as_ushort(__float2bfloat16(r1 * scale));
  dst[2 * j + 1] = __bfloat16_as_ushort(__float2bfloat16(r2 * scale));
}

}  // namespace

// Fused decode-step RoPE for bf16 q AND k in one launch, with per-row
// positions (continuous batching): q [b, hq, d], k [b, hk, d]
// contiguous (s=1), cos/sin tables [max_seq, d/2] fp32, pos [b] int64.
// Replaces ~8 slicing/elementwise launches per projection.
extern "C" __global__ void rope_decode_bf16_kernel(
    uint16_t* __restrict__ q, uint16_t* __restrict__ k,
    const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    const long* __restrict__ pos, int b, int hq, int hk, int d) {
  const int half = d / 2;
  const long total = (long)b * (hq + hk) * half;
  long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    long rem = i;
    const int j = (int)(rem % half);  // rotation pair index
    rem /= half;
    const int head = (int)(rem % (hq + hk));
    const int row = (int)(rem / (hq + hk));
    uint16_t* base = (head < hq)
                         ? q + ((long)row * hq + head) * d
                         : k + ((long)row * hk + (head - hq)) * d;
    const float c = cos_tab[pos[row] * half + j];
    const float s = sin_tab[pos[row] * half + j];
    rope_rotate_pair(base, base, j, c, s, 1.0f);
  }
}

extern "C" hipError_t ca_rope_decode_bf16(void* q, void* k,
                                          const void* cos_tab,
                                          const void* sin_tab,
                                          const void* pos, int b, int hq,
                                          int hk, int d, hipStream_t stream) {
  long total = (long)b * (hq + hk) * (d / 2);
  hipLaunchKernelGGL(rope_decode_bf16_kernel, dim3(ca_grid_for(total)),
                     dim3(256), 0, stream, (uint16_t*)q, (uint16_t*)k,
                     (const float*)cos_tab, (const float*)sin_tab,
                     (const long*)pos, b, hq, hk, d);
  return hipGetLastError();
}

// RoPE + KV-cache scatter in ONE launch: rotates q (in place) and k
// (rotated values written straight into the cache at each row's
// position), and copies v into the cache — removing the two
// torch index_put launches per layer per decode step (64/step at 32
// layers; measured 28.9 ms / 5120 calls in the decode profile).
// ck/cv: [b, hk, cache_len, d]; k/v: [b, hk, d] contiguous.
extern "C" __global__ void rope_scatter_decode_bf16_kernel(
    uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint16_t* __restrict__ ck,
    uint16_t* __restrict__ cv, const float* __restrict__ cos_tab,
    const float* __restrict__ sin_tab, const long* __restrict__ pos, int b,
    int hq, int hk, int d, long cache_len, float q_scale) {
  const int half = d / 2;
  const long total = (long)b * (hq + 2 * hk) * half;
  long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    long rem = i;
    const int j = (int)(rem % half);
    rem /= half;
    const int head = (int)(rem % (hq + 2 * hk));
    const int row = (int)(rem / (hq + 2 * hk));
    const long p = pos[row];
    if (head < hq) {  // q: rotate in place (+ folded 1/sqrt(d) scale)
      uint16_t* base = q + ((long)row * hq + head) * d;
      rope_rotate_pair(base, base, j, cos_tab[p * half + j],
                       sin_tab[p * half + j], q_scale);
    } else if (head < hq + hk) {  // k: rotate -> cache
      const int h = head - hq;
      const uint16_t* base = k + ((long)row * hk + h) * d;
      uint16_t* dst =
          ck + (((long)row * hk + h) * cache_len + p) * d;
      rope_rotate_pair(base, dst, j, cos_tab[p * half + j],
                       sin_tab[p * half + j], 1.0f);
    } else {  // v: straight copy -> cache
      const int h = head - hq - hk;
      const uint16_t* base = v + ((long)row * hk + h) * d;
      uint16_t* dst =
          cv + (((long)row * hk + h) * cache_len + p) * d;
      dst[2 * j] = base[2 * j];
      dst[2 * j + 1] = base[2 * j + 1];
    }
  }
}

extern "C" hipError_t ca_rope_scatter_decode_bf16(
    void* q, const void* k, const void* v, void* ck, void* cv,
    const void* cos_tab, const void* sin_tab, const void* pos, int b,
    int hq, int hk, int d, long cache_len, float q_scale,
    hipStream_t stream) {
  long total = (long)b * (hq + 2 * hk) * (d / 2);
  hipLaunchKernelGGL(rope_scatter_decode_bf16_kernel,
                     dim3(ca_grid_for(total)), dim3(256), 0, stream,
                     (uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                     (uint16_t*)ck, (uint16_t*)cv, (const float*)cos_tab,
                     (const float*)sin_tab, (const long*)pos, b, hq, hk, d,
                     cache_len, q_scale);
  return hipGetLastError();
}

// The same step for an fp8 (OCP e4m3fn) KV cache: ck/cv hold one code
// per element. q is rotated exactly as above; k is rotated and rounded
// to bf16 by the same rope_rotate_pair, then encoded (CastF32ToFp8's
// contract: RNE, finite values saturate to +-448), so the cache holds
// the e4m3 encoding of what the bf16 cache would hold. A lane's two
// adjacent codes go out as one 16-bit store. Rows whose position is
// outside [0, cache_len) write nothing at all.
extern "C" __global__ void rope_scatter_decode_fp8kv_bf16_kernel(
    uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, uint8_t* __restrict__ ck,
    uint8_t* __restrict__ cv, const float* __restrict__ cos_tab,
    const float* __restrict__ sin_tab, const long* __restrict__ pos, int b,
    int hq, int hk, int d, long cache_len, float q_scale) {
  const int half = d / 2;
  const long total = (long)b * (hq + 2 * hk) * half;
  long i = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    long rem = i;
    const int j = (int)(rem % half);
    rem /= half;
    const int head = (int)(rem % (hq + 2 * hk));
    const int row = (int)(rem / (hq + 2 * hk));
    const long p = pos[row];
    if (p < 0 || p >= cache_len) continue;
    if (head < hq) {
      uint16_t* base = q + ((long)row * hq + head) * d;
      rope_rotate_pair(base, base, j, cos_tab[p * half + j],
                       sin_tab[p * half + j], q_scale);
      continue;
    }
    uint16_t pair[2];
    uint8_t* dst;
    if (head < hq + hk) {
      const int h = head - hq;
      rope_rotate_pair(k + ((long)row * hk + h) * d + 2 * j, pair, 0,
                       cos_tab[p * half + j], sin_tab[p * half + j], 1.0f);
      dst = ck + (((long)row * hk + h) * cache_len + p) * d;
    } else {
      const int h = head - hq - hk;
      const uint16_t* base = v + ((long)row * hk + h) * d;
      pair[0] = base[2 * j];
      pair[1] = base[2 * j + 1];
      dst = cv + (((long)row * hk + h) * cache_len + p) * d;
    }
    const uint32_t lo = CastF32ToFp8::convert(bf16_to_f32(pair[0]));
    const uint32_t hi = CastF32ToFp8::convert(bf16_to_f32(pair[1]));
    *reinterpret_cast<uint16_t*>(dst + 2 * j) = (uint16_t)(lo | (hi << 8));
  }
}

extern "C" hipError_t ca_rope_scatter_decode_fp8kv_bf16(
    void* q, const void* k, const void* v, void* ck, void* cv,
    const void* cos_tab, const void* sin_tab, const void* pos, int b,
    int hq, int hk, int d, long cache_len, float q_scale,
    hipStream_t stream) {
  // the packed 16-bit code stores need even addresses
  if (d % 2 != 0 || ((uintptr_t)ck | (uintptr_t)cv) % 2 != 0)
    return hipErrorInvalidValue;
  long total = (long)b * (hq + 2 * hk) * (d / 2);
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(rope_scatter_decode_fp8kv_bf16_kernel,
                     dim3(ca_grid_for(total)), dim3(256), 0, stream,
                     (uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,
                     (uint8_t*)ck, (uint8_t*)cv, (const float*)cos_tab,
                     (const float*)sin_tab, (const long*)pos, b, hq, hk, d,
                     cache_len, q_scale);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fused GQA decode attention (one query position per row, per-row
// lengths): out[i, h] = softmax_j(scale * q[i, h] . K[i, g, j]) V[i, g, j]
// over the keys j < n_i = min(pos[i] + 1, max_len) of kv head g = h / rep.
//
// Split kernel: grid (key split, kv head, row), GA_SPLIT keys per split.
// One workgroup serves all rep query heads of its kv head, so K/V are
// read once. A group of LPK lanes owns one key row and loads it 16 B per
// lane; all of a lane's K loads, then all its V loads, are issued before
// the first use. Scores go to LDS, wave r takes the exact fp32 softmax
// of head r over the split's keys (max m, p = exp(s - m), sum l), and the
// groups accumulate p * V in fp32, reduced across the groups of a wave
// by shuffles and across the four waves through LDS in a fixed order.
// The partial (m, l, acc[d]) of each (row, head, split) goes to an fp32
// workspace. Keys at j >= n_i are never loaded, and a split with no key
// writes nothing.
//
// Combine kernel: one workgroup per (row, head) merges the row's
// ceil(n_i / GA_SPLIT) partials in ascending order, each rescaled by
// exp(m_split - m_row), and rounds once (RNE) to bf16.
//
// No atomics and no arrival counters: the split a key falls in and every
// reduction order depend on the key's index alone, so a row's output
// bits do not depend on b, max_len, the row's index or its neighbours.
//
// The two kernels are templates on (storage type, head dim, padded rep)
// launched directly, 36 instantiations, not one extern "C" entry point
// each; their names in a trace carry the template arguments.
// ---------------------------------------------------------------------------
#define GA_SPLIT 128    // keys per split (exported to Python)
#define GA_THREADS 256
#define GA_WS_PAD 4     // floats ahead of acc[d] in a partial: m, l, 2 unused

namespace {

// 16 bytes of stored K/V -> fp32
__device__ __forceinline__ void ga_unpack(const uint4& w, float (&f)[8],
                                          const uint16_t*) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf16x2_lo(u[i]);
    f[2 * i + 1] = bf16x2_hi(u[i]);
  }
}
__device__ __forceinline__ void ga_unpack(const uint4& w, float (&f)[16],
                                          const uint8_t*) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#if defined(__gfx950__)
  // two codes per hardware convert
  typedef float ga_f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const ga_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[i], false);
    const ga_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
#else
#pragma unroll
  for (int i = 0; i < 16; ++i)
    f[i] = CastFp8ToF32::convert((uint8_t)(u[i / 4] >> (8 * (i % 4))));
#endif
}

template <typename T, int D, int REP>
__device__ __forceinline__ void ga_split_body(
    const uint16_t* __restrict__ q, const T* __restrict__ ck,
    const T* __restrict__ cv, const long* __restrict__ pos,
    float* __restrict__ ws, int hq, int hk, int rep, float scale,
    long max_len, long cache_len, int n_splits) {
  constexpr int VEC = 16 / (int)sizeof(T);  // elements per 16-byte load
  constexpr int LPK = D / VEC;              // lanes per key row
  constexpr int GROUPS = GA_THREADS / LPK;  // key rows in flight
  constexpr int KPG = (GA_SPLIT + GROUPS - 1) / GROUPS;  // keys per group
  static_assert(LPK >= 1 && LPK <= 16 && D % VEC == 0, "head dim");

  __shared__ float s_p[REP][GA_SPLIT];   // scores, then probabilities
  __shared__ float s_ml[REP][2];
  __shared__ float s_acc[4][REP][D];     // per-wave accumulators

  const int split = blockIdx.x;
  const int g_kv = blockIdx.y;
  const int row = blockIdx.z;
  long n = pos[row] + 1;
  if (n > max_len) n = max_len;
  const long first = (long)split * GA_SPLIT;
  if (first >= n) return;  // empty split (block-uniform)
  const int cnt = (int)((n - first < GA_SPLIT) ? (n - first) : GA_SPLIT);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int grp = tid / LPK;
  const int sub = tid % LPK;

  const long kv_base = (((long)row * hk + g_kv) * cache_len + first) * D;
  const T* kp = ck + kv_base + sub * VEC;
  const T* vp = cv + kv_base + sub * VEC;

  // loads return in issue order: q first, then K, then V, so the
  // scores start while V is still in flight. All loads are unconditional
  // (a branch around a load costs a wait at its join): a lane whose key
  // is past the split's last one re-reads that last key, a padded head
  // re-reads the last real head, and neither result is ever stored.
  constexpr int QW = VEC / 8;  // 16-byte words of a lane's q slice
  uint4 qbuf[REP][QW];
#pragma unroll
  for (int r = 0; r < REP; ++r) {
    const int rc = (r < rep) ? r : rep - 1;
    const uint16_t* qr =
        q + ((long)row * hq + (long)g_kv * rep + rc) * D + sub * VEC;
#pragma unroll
    for (int w = 0; w < QW; ++w)
      qbuf[r][w] = reinterpret_cast<const uint4*>(qr)[w];
  }
  uint4 kbuf[KPG], vbuf[KPG];
#pragma unroll
  for (int i = 0; i < KPG; ++i) {
    const int j = grp + i * GROUPS;
    const int jc = (j < cnt) ? j : cnt - 1;
    kbuf[i] = *reinterpret_cast<const uint4*>(kp + (long)jc * D);
  }
#pragma unroll
  for (int i = 0; i < KPG; ++i) {
    const int j = grp + i * GROUPS;
    const int jc = (j < cnt) ? j : cnt - 1;
    vbuf[i] = *reinterpret_cast<const uint4*>(vp + (long)jc * D);
  }
  // keep every load above issued before the first use: left alone, the
  // scheduler sinks each load to its use to save registers, and a split
  // then pays one memory latency per key instead of one in all
  __builtin_amdgcn_sched_barrier(0);

  // scores
  {
    float qf[REP][VEC];
#pragma unroll
    for (int r = 0; r < REP; ++r)
#pragma unroll
      for (int w = 0; w < QW; ++w) {
        float f[8];
        ga_unpack(qbuf[r][w], f, (const uint16_t*)nullptr);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[r][8 * w + e] = f[e];
      }
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      const int j = grp + i * GROUPS;
      float kf[VEC];
      ga_unpack(kbuf[i], kf, (const T*)nullptr);
#pragma unroll
      for (int r = 0; r < REP; ++r) {
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) dot += qf[r][e] * kf[e];
#pragma unroll
        for (int off = LPK / 2; off > 0; off >>= 1)
          dot += __shfl_xor(dot, off);
        if (sub == 0 && j < cnt) s_p[r][j] = dot * scale;
      }
    }
  }
  __syncthreads();

  // softmax over the split's keys: wave w takes heads w, w + 4
  for (int r = wave; r < REP; r += 4) {
    float m = -INFINITY;
    for (int j = lane; j < cnt; j += 64) m = fmaxf(m, s_p[r][j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float l = 0.f;
    for (int j = lane; j < cnt; j += 64) {
      const float p = __expf(s_p[r][j] - m);
      s_p[r][j] = p;
      l += p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off);
    if (lane == 0) {
      s_ml[r][0] = m;
      s_ml[r][1] = l;
    }
  }
  __syncthreads();

  // p * V
  float acc[REP][VEC];
#pragma unroll
  for (int r = 0; r < REP; ++r)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[r][e] = 0.f;
#pragma unroll
  for (int i = 0; i < KPG; ++i) {
    const int j = grp + i * GROUPS;
    if (j < cnt) {
      float vf[VEC];
      ga_unpack(vbuf[i], vf, (const T*)nullptr);
#pragma unroll
      for (int r = 0; r < REP; ++r) {
        const float p = s_p[r][j];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[r][e] += p * vf[e];
      }
    }
  }
  // across the groups of a wave, then across the waves
#pragma unroll
  for (int r = 0; r < REP; ++r)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float a = acc[r][e];
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) a += __shfl_xor(a, off);
      acc[r][e] = a;
    }
  if (lane < LPK) {
#pragma unroll
    for (int r = 0; r < REP; ++r)
#pragma unroll
      for (int e = 0; e < VEC; ++e) s_acc[wave][r][lane * VEC + e] = acc[r][e];
  }
  __syncthreads();
  for (int idx = tid; idx < rep * D; idx += GA_THREADS) {
    const int r = idx / D;
    const int e = idx % D;
    const float a =
        ((s_acc[0][r][e] + s_acc[1][r][e]) + s_acc[2][r][e]) + s_acc[3][r][e];
    float* part = ws + (((long)row * hq + (long)g_kv * rep + r) * n_splits +
                        split) * (D + GA_WS_PAD);
    part[GA_WS_PAD + e] = a;
    if (e < 2) part[e] = s_ml[r][e];
  }
}

template <int D>
__device__ __forceinline__ void ga_combine_body(
    const float* __restrict__ ws, const long* __restrict__ pos,
    uint16_t* __restrict__ out, int hq, long max_len, int n_splits) {
  const int head = blockIdx.x;
  const int row = blockIdx.y;
  const int e = threadIdx.x;  // blockDim.x == D
  long n = pos[row] + 1;
  if (n > max_len) n = max_len;
  const int used = (n <= 0) ? 0 : (int)((n + GA_SPLIT - 1) / GA_SPLIT);
  const float* part =
      ws + ((long)row * hq + head) * n_splits * (D + GA_WS_PAD);
  constexpr int STRIDE = D + GA_WS_PAD;
  // The row's maximum first (lane t reads the m of splits t, t + D, ...;
  // a max does not depend on the order), so that the loads of the second
  // pass are independent of each other and can be in flight together:
  // one load latency per split was most of this kernel's time.
  __shared__ float s_m[(D + 63) / 64];
  float m = -INFINITY;
  for (int s = e; s < used; s += D) m = fmaxf(m, part[(long)s * STRIDE]);
#pragma unroll
  for (int off = (D < 64 ? D : 64) / 2; off > 0; off >>= 1)
    m = fmaxf(m, __shfl_xor(m, off));
  if constexpr (D > 64) {
    if ((e & 63) == 0) s_m[e >> 6] = m;
    __syncthreads();
    m = s_m[0];
#pragma unroll
    for (int w = 1; w < D / 64; ++w) m = fmaxf(m, s_m[w]);
  }
  // every lane computes the same l, in ascending split order
  float l = 0.f, o = 0.f;
#pragma unroll 8
  for (int s = 0; s < used; ++s) {
    const float c = __expf(part[(long)s * STRIDE] - m);
    l += part[(long)s * STRIDE + 1] * c;
    o += part[(long)s * STRIDE + GA_WS_PAD + e] * c;
  }
  const float r = (used > 0) ? o / l : 0.f;
  out[((long)row * hq + head) * D + e] =
      __bfloat16_as_ushort(__float2bfloat16(r));
}

}  // namespace

template <typename T, int D, int REP>
__global__ void __launch_bounds__(GA_THREADS)
gqa_decode_split_kernel(const uint16_t* __restrict__ q,
                        const T* __restrict__ ck, const T* __restrict__ cv,
                        const long* __restrict__ pos, float* __restrict__ ws,
                        int hq, int hk, int rep, float scale, long max_len,
                        long cache_len, int n_splits) {
  ga_split_body<T, D, REP>(q, ck, cv, pos, ws, hq, hk, rep, scale, max_len,
                           cache_len, n_splits);
}

template <int D>
__global__ void gqa_decode_combine_kernel(const float* __restrict__ ws,
                                          const long* __restrict__ pos,
                                          uint16_t* __restrict__ out, int hq,
                                          long max_len, int n_splits) {
  ga_combine_body<D>(ws, pos, out, hq, max_len, n_splits);
}

namespace {

inline bool ga_shape_ok(int hq, int hk, int d) {
  if (d != 16 && d != 32 && d != 64 && d != 128) return false;
  if (hq <= 0 || hk <= 0 || hq % hk != 0 || hq / hk > 8) return false;
  return true;
}

inline long ga_n_splits(long max_len) {
  return (max_len + GA_SPLIT - 1) / GA_SPLIT;
}

template <typename T, int D>
hipError_t ga_launch(const void* q, const void* ck, const void* cv,
                     const void* pos, void* out, void* ws, int b, int hq,
                     int hk, float scale, long max_len, long cache_len,
                     hipStream_t stream) {
  const int rep = hq / hk;
  const int n_splits = (int)ga_n_splits(max_len);
  const dim3 grid((uint32_t)n_splits, (uint32_t)hk, (uint32_t)b);
#define GA_LAUNCH(REP)                                                       \
  hipLaunchKernelGGL((gqa_decode_split_kernel<T, D, REP>), grid,             \
                     dim3(GA_THREADS), 0, stream, (const uint16_t*)q,        \
                     (const T*)ck, (const T*)cv, (const long*)pos,           \
                     (float*)ws, hq, hk, rep, scale, max_len, cache_len,     \
                     n_splits)
  if (rep == 1) GA_LAUNCH(1);
  else if (rep == 2) GA_LAUNCH(2);
  else if (rep <= 4) GA_LAUNCH(4);
  else GA_LAUNCH(8);
#undef GA_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((gqa_decode_combine_kernel<D>),
                     dim3((uint32_t)hq, (uint32_t)b), dim3(D), 0, stream,
                     (const float*)ws, (const long*)pos, (uint16_t*)out, hq,
                     max_len, n_splits);
  return hipGetLastError();
}

template <typename T>
hipError_t ga_launch_d(int d, const void* q, const void* ck, const void* cv,
                       const void* pos, void* out, void* ws, int b, int hq,
                       int hk, float scale, long max_len, long cache_len,
                       hipStream_t stream) {
  switch (d) {
    case 16:
      return ga_launch<T, 16>(q, ck, cv, pos, out, ws, b, hq, hk, scale,
                              max_len, cache_len, stream);
    case 32:
      return ga_launch<T, 32>(q, ck, cv, pos, out, ws, b, hq, hk, scale,
                              max_len, cache_len, stream);
    case 64:
      return ga_launch<T, 64>(q, ck, cv, pos, out, ws, b, hq, hk, scale,
                              max_len, cache_len, stream);
    default:
      return ga_launch<T, 128>(q, ck, cv, pos, out, ws, b, hq, hk, scale,
                               max_len, cache_len, stream);
  }
}

}  // namespace

// bytes of fp32 workspace ca_gqa_decode_attention needs; 0 for an
// unsupported shape
extern "C" long ca_gqa_decode_attention_workspace_bytes(int b, int hq, int d,
                                                        long max_len) {
  if (b < 0 || hq <= 0 || d <= 0 || max_len <= 0) return 0;
  return (long)b * hq * ga_n_splits(max_len) * (d + GA_WS_PAD) *
         (long)sizeof(float);
}

// q/out [b, hq, d] bf16; ck/cv [b, hk, cache_len, d] bf16 bits, or e4m3
// codes with kv_fp8; pos [b] int64 on the device.
extern "C" hipError_t ca_gqa_decode_attention(
    const void* q, const void* ck, const void* cv, const void* pos, void* out,
    void* ws, long ws_bytes, int b, int hq, int hk, int d, float scale,
    long max_len, long cache_len, int kv_fp8, hipStream_t stream) {
  if (b < 0 || !ga_shape_ok(hq, hk, d)) return hipErrorInvalidValue;
  if (max_len <= 0 || max_len > cache_len) return hipErrorInvalidValue;
  if (b > 65535 || hk > 65535) return hipErrorInvalidValue;  // grid y, z
  if (b == 0) return hipSuccess;
  if (ws_bytes < ca_gqa_decode_attention_workspace_bytes(b, hq, d, max_len))
    return hipErrorInvalidValue;
  // 16-byte q and K/V row loads; fp32 workspace
  if (((uintptr_t)ck | (uintptr_t)cv | (uintptr_t)q) % 16 != 0 ||
      (uintptr_t)ws % 4 != 0 || (uintptr_t)out % 2 != 0)
    return hipErrorInvalidValue;
  if (kv_fp8)
    return ga_launch_d<uint8_t>(d, q, ck, cv, pos, out, ws, b, hq, hk, scale,
                                max_len, cache_len, stream);
  return ga_launch_d<uint16_t>(d, q, ck, cv, pos, out, ws, b, hq, hk, scale,
                               max_len, cache_len, stream);
}

// prefill-chunk RoPE + scatter and MFMA attention (share rope_rotate_pair,
// ga_unpack and ga_shape_ok with the above)
#include "prefill_attention.hip"

// BERT encoder attention with a per-row key mask (shares the fragment
// types and pa_head_dim_ok with the above)
#include "encoder_attention.hip"

// Skinny decode GEMM: y[8, N] = x[8, K] @ W[N, K]^T, bf16 in/out,
// fp32 accumulate. The decode batch is tiny (8 rows), so the GEMM is
// pure weight streaming — hipBLASLt's skinny-tile kernels measured
// 2.1-4.2 TB/s on these shapes (profiles/decode_rocprof_r02.txt);
// this kernel is weights-stationary: x lives in LDS (staged in K
// chunks), W streams once with 16-B coalesced lane loads, each lane
// keeps 8 fp32 accumulators (one per batch row), cross-lane reduce at
// the end. One wavefront per W row, 4 rows per workgroup, grid-stride
// over N.
#define DG_M 8          // decode batch rows (compile-time; pad to 8)
#define DG_KC 4096      // K chunk staged in LDS: 8*4096*2 B = 64 KB
extern "C" __global__ void __launch_bounds__(256)
decode_gemm_bf16_kernel(const uint16_t* __restrict__ x,
                        const uint16_t* __restrict__ w,
                        uint16_t* __restrict__ y, int N, int K) {
  __shared__ uint16_t xs[DG_M * DG_KC];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;  // 4 waves = 4 W rows
  float acc[DG_M];
#pragma unroll
  for (int m = 0; m < DG_M; ++m) acc[m] = 0.f;

  const long row0 = (long)blockIdx.x * 4;
  // grid-stride over row groups so any N works with a capped grid
  for (long nb = row0; nb < N; nb += (long)gridDim.x * 4) {
    const long n = nb + wave;
#pragma unroll
    for (int m = 0; m < DG_M; ++m) acc[m] = 0.f;
    for (int kc = 0; kc < K; kc += DG_KC) {
      const int kn = min(DG_KC, K - kc);
      // cooperative stage of x[:, kc:kc+kn] (row-major [M, K])
      __syncthreads();
      for (int idx = threadIdx.x * 8; idx < DG_M * kn;
           idx += blockDim.x * 8) {
        const int m = idx / kn;
        const int k = idx - m * kn;
        if (k + 8 <= kn) {
          *reinterpret_cast<uint4*>(xs + m * DG_KC + k) =
              *reinterpret_cast<const uint4*>(x + (long)m * K + kc + k);
        } else {
          for (int t = k; t < kn; ++t)
            xs[m * DG_KC + t] = x[(long)m * K + kc + t];
        }
      }
      __syncthreads();
      if (n < N) {
        const uint16_t* wr = w + n * (long)K + kc;
        // lane streams 8 W elems per iteration, 64 lanes cover 512
        for (int k0 = lane * 8; k0 + 8 <= kn; k0 += 64 * 8) {
          uint4 wv = *reinterpret_cast<const uint4*>(wr + k0);
          const uint16_t* we = reinterpret_cast<const uint16_t*>(&wv);
          float wf[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) wf[j] = bf16_to_f32(we[j]);
#pragma unroll
          for (int m = 0; m < DG_M; ++m) {
            const uint16_t* xr = xs + m * DG_KC + k0;
            uint4 xv = *reinterpret_cast<const uint4*>(xr);
            const uint16_t* xe = reinterpret_cast<const uint16_t*>(&xv);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
              s = fmaf(bf16_to_f32(xe[j]), wf[j], s);
            acc[m] += s;
          }
        }
        // (no ragged-K handling: the launcher rejects K % 512 != 0)
      }
    }
    if (n < N) {
      // cross-lane reduce each row's 8 accumulators
#pragma unroll
      for (int m = 0; m < DG_M; ++m) {
        float v = acc[m];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) y[(long)m * N + n] = f32_to_bf16_rne(v);
      }
    }
  }
}

extern "C" hipError_t ca_decode_gemm_bf16(const void* x, const void* w,
                                          void* y, int N, int K,
                                          hipStream_t stream) {
  // K must be a multiple of 512 (64 lanes x 8) — true for every
  // decode GEMM in the model family (4096, 14336, 1024); reject others
  // so callers fall back to torch.
  if (K % 512 != 0) return hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15)
    return hipErrorInvalidValue;
  long groups = ((long)N + 3) / 4;
  int grid = (int)(groups > 2048 ? 2048 : groups);
  hipLaunchKernelGGL(decode_gemm_bf16_kernel, dim3(grid), dim3(256), 0,
                     stream, (const uint16_t*)x, (const uint16_t*)w,
                     (uint16_t*)y, N, K);
  return hipGetLastError();
}

// fp8 (e4m3) weight-only linears: M <= 16 MFMA decode GEMM and dequant
#include "weight_fp8.hip"

// Token sampling from bf16 logits: temperature, top-k, top-p and a
// per-row counter-based random draw, one workgroup per row, placed
// where argmax sits in the decode step. Every per-row parameter is read
// from device memory, so a captured launch sees new values on replay.
//
// Contract per row (tests/sampling_refs.py is the float64 statement):
//   - logits are sanitised: NaN reads as -inf, +inf as the largest
//     finite bf16, -0 as +0; a row with no finite logit yields token 0
//   - temperature 0 (also negative or NaN, which callers reject) yields
//     the lowest index holding the maximum
//   - K = logits >= the k-th largest (ties included); weights
//     w = exp((l - l_max) / T); N = logits >= the largest distinct value
//     whose tail mass reaches top_p * S_K (ties included)
//   - u = (x0 >> 8) * 2^-24, x0 = word 0 of Philox4x32-10 with counter
//     (step, 0, 0) and key seed; the token is the first index of N, in
//     index order, whose running weight exceeds u * S_N
//
// bf16 maps monotonically onto a 16-bit key, so both thresholds are
// two-level 256-bin radix selections in LDS (counts for top-k, weight
// sums for top-p) and nothing is sorted. A weight depends on the key
// alone and is held as a 2^-44 fixed-point integer: every sum is an
// exact, order-independent integer sum, which makes the token a pure
// function of (row contents, parameters, seed, step) whatever the row
// index, batch or replay. The first pass reads the row from HBM, later
// passes hit L2. Each wave owns a contiguous chunk of the row, so the
// per-wave totals of the last pass locate the draw and only that wave
// walks its chunk again with a running scan. Rows may start on any
// 2-byte boundary: a scalar head and tail surround the 16 B/lane body.
#define SL_THREADS 1024
#define SL_WAVES (SL_THREADS / 64)
#define SL_COPIES 16         // histogram replicas: same-bin lanes spread
#define SL_KEY_NEG_INF 0x007Fu
#define SL_ONE (1ull << 44)  // fixed-point 1.0

namespace {

typedef unsigned long long sl_u64;

// sanitised bf16 bits -> key with the same order as the values; never 0,
// so 0 marks an absent element
__device__ __forceinline__ uint32_t sl_key(uint32_t x) {
  if ((x & 0x7FFFu) > 0x7F80u) x = 0xFF80u;  // NaN -> -inf
  else if (x == 0x7F80u) x = 0x7F7Fu;        // +inf -> largest finite
  else if (x == 0x8000u) x = 0u;             // -0 -> +0
  return (x & 0x8000u) ? (~x & 0xFFFFu) : (x | 0x8000u);
}

__device__ __forceinline__ float sl_key_value(uint32_t key) {
  const uint32_t h = (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu);
  return __uint_as_float(h << 16);
}

// A row as nvec 8-element vectors in index order: vector 0 is the
// scalar head (up to the first 16 B boundary), 1..nbody the aligned
// body, nbody+1 the scalar tail. Head and tail may be empty.
struct SlRow {
  const uint16_t* p;
  int vocab, head, nbody, nvec;
};

__device__ __forceinline__ SlRow sl_row(const uint16_t* logits, long row,
                                        int vocab) {
  SlRow r;
  r.p = logits + row * vocab;
  r.vocab = vocab;
  const int head = (int)(((16u - ((uintptr_t)r.p & 15u)) & 15u) >> 1);
  r.head = head < vocab ? head : vocab;
  r.nbody = (vocab - r.head) >> 3;
  r.nvec = r.nbody + 2;
  return r;
}

// Vector v of a row as loaded: raw bf16 pairs, index of the first
// element, number of elements present (0 for v outside the row)
struct SlVec {
  uint4 q;
  int e0, cnt;
};

__device__ __forceinline__ SlVec sl_load(const SlRow& r, int v, int end) {
  SlVec x;
  x.q = make_uint4(0u, 0u, 0u, 0u);
  x.e0 = 0;
  x.cnt = 0;
  if (v >= end) return x;
  if (v >= 1 && v <= r.nbody) {
    x.e0 = r.head + ((v - 1) << 3);
    x.cnt = 8;
    x.q = *reinterpret_cast<const uint4*>(r.p + x.e0);
    return x;
  }
  x.e0 = v == 0 ? 0 : r.head + (r.nbody << 3);
  x.cnt = v == 0 ? r.head : r.vocab - x.e0;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = j < x.cnt ? r.p[x.e0 + j] : 0u;
  x.q = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16),
                   h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  return x;
}

// keys of a loaded vector, 0 where the element does not exist
__device__ __forceinline__ void sl_keys(const SlVec& x, uint32_t k[8]) {
  const uint32_t w[4] = {x.q.x, x.q.y, x.q.z, x.q.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k[2 * j] = 2 * j < x.cnt ? sl_key(w[j] & 0xFFFFu) : 0u;
    k[2 * j + 1] = 2 * j + 1 < x.cnt ? sl_key(w[j] >> 16) : 0u;
  }
}

// Each wave owns a contiguous chunk of the row's vectors, [lo, hi), and
// walks it 64 vectors (1 KiB) at a time.
__device__ __forceinline__ void sl_chunk(const SlRow& r, int& lo, int& hi) {
  const int per = (r.nvec + SL_WAVES - 1) / SL_WAVES;
  lo = (int)(threadIdx.x >> 6) * per;
  hi = lo + per < r.nvec ? lo + per : r.nvec;
}

// f(keys, e0) over this thread's share of the row, in no particular
// order. Four loads are in flight per thread: with one workgroup per row
// a pass is bound by load latency, not by bandwidth.
template <typename F>
__device__ __forceinline__ void sl_for_each(const SlRow& r, F f) {
  int lo, hi;
  sl_chunk(r, lo, hi);
  for (int v = lo + (int)(threadIdx.x & 63); v < hi; v += 256) {
    SlVec x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = sl_load(r, v + 64 * u, hi);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      uint32_t k[8];
      sl_keys(x[u], k);
      f(k, x[u].e0);
    }
  }
}

// fixed-point weight of a key, 2^((l - l_max) * scale) with scale =
// log2(e) / T; the maximum is exactly 1 so a temperature too small to
// invert still leaves the maximum its mass
__device__ __forceinline__ sl_u64 sl_weight(uint32_t key, uint32_t maxkey,
                                            float lmax, float scale) {
  if (key == maxkey) return SL_ONE;
  const float w = exp2f((sl_key_value(key) - lmax) * scale);
  return w > 0.f ? (sl_u64)(w * 0x1p44f) : 0ull;
}

// block-wide max / sum, result in every thread; scratch holds SL_WAVES
__device__ __forceinline__ sl_u64 sl_block_max(sl_u64 v, sl_u64* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const sl_u64 t = __shfl_xor(v, off);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  sl_u64 m = scratch[0];
#pragma unroll
  for (int i = 1; i < SL_WAVES; ++i) m = scratch[i] > m ? scratch[i] : m;
  __syncthreads();
  return m;
}

__device__ __forceinline__ sl_u64 sl_block_sum(sl_u64 v, sl_u64* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  sl_u64 s = 0;
#pragma unroll
  for (int i = 0; i < SL_WAVES; ++i) s += scratch[i];
  __syncthreads();
  return s;
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ sl_u64 sl_wave_scan(sl_u64 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const sl_u64 t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// One histogram pass over the row: f(key, bin, val) says whether the key
// takes part and with what; returns this thread's sum of val. Ends with
// the histogram complete and visible.
template <typename F>
__device__ __forceinline__ sl_u64 sl_hist_pass(const SlRow& r, sl_u64* hist,
                                               F f) {
  for (int i = threadIdx.x; i < 256 * SL_COPIES; i += SL_THREADS) hist[i] = 0;
  __syncthreads();
  const int copy = threadIdx.x & (SL_COPIES - 1);
  sl_u64 local = 0;
  sl_for_each(r, [&](const uint32_t k[8], int) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int bin = 0;
      sl_u64 val = 0;
      if (k[j] != 0u && f(k[j], bin, val) && val != 0ull) {
        atomicAdd(&hist[bin * SL_COPIES + copy], val);
        local += val;
      }
    }
  });
  __syncthreads();
  return local;
}

struct SlSel {
  int bin;       // highest bin whose tail sum (itself included) >= need
  sl_u64 above;  // sum of the bins above it
  sl_u64 incl;   // above + the bin itself
};

// Radix-select step on a complete histogram: bin = -1 when even the sum
// of all bins stays below need. need >= 1. Called by every thread.
__device__ __forceinline__ SlSel sl_select(const sl_u64* hist, sl_u64 need,
                                           sl_u64* scratch, SlSel* sh) {
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  sl_u64 mine = 0;  // thread t < 256 owns bin 255 - t: scan order = top down
  if (tid < 256) {
    const sl_u64* h = hist + (255 - tid) * SL_COPIES;
#pragma unroll
    for (int c = 0; c < SL_COPIES; ++c) mine += h[c];
  }
  sl_u64 incl = sl_wave_scan(mine);
  if (tid == 0) sh->bin = -1;
  if ((tid & 63) == 63 && wave < 4) scratch[wave] = incl;
  __syncthreads();
  if (tid < 256) {
    for (int i = 0; i < wave; ++i) incl += scratch[i];
    if (incl >= need && incl - mine < need) {
      sh->bin = 255 - tid;
      sh->above = incl - mine;
      sh->incl = incl;
    }
  }
  __syncthreads();
  return *sh;
}

__device__ __forceinline__ uint32_t sl_philox_word0(sl_u64 seed, sl_u64 ctr) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0u, c3 = 0u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SL_THREADS)
sample_logits_bf16_kernel(const uint16_t* __restrict__ logits,
                          const float* __restrict__ temperature,
                          const int* __restrict__ top_k,
                          const float* __restrict__ top_p,
                          const sl_u64* __restrict__ seed,
                          const long* __restrict__ step,
                          long* __restrict__ out, int vocab) {
  __shared__ sl_u64 hist[256 * SL_COPIES];  // 32 KB
  __shared__ sl_u64 scratch[SL_WAVES];
  __shared__ SlSel sh_sel;
  __shared__ int sh_found;
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const SlRow r = sl_row(logits, row, vocab);
  const float temp = temperature[row];
  const int k = top_k[row];
  const float p = top_p[row];
  const bool sampled = temp > 0.f;  // NaN compares false
  const bool use_k = sampled && k > 0 && k < vocab;
  const bool use_p = sampled && p < 1.f;
  const int copy = tid & (SL_COPIES - 1);

  // pass 1 (HBM): maximum and its lowest index, packed so one max finds
  // both; with top-k on, also the level-1 count histogram
  if (use_k) {
    for (int i = tid; i < 256 * SL_COPIES; i += SL_THREADS) hist[i] = 0;
    __syncthreads();
  }
  sl_u64 best = 0;
  sl_for_each(r, [&](const uint32_t key[8], int e0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (key[j] == 0u) continue;
      const sl_u64 cand =
          ((sl_u64)key[j] << 32) | (sl_u64)(0xFFFFFFFFu - (uint32_t)(e0 + j));
      best = cand > best ? cand : best;
      if (use_k) atomicAdd(&hist[(key[j] >> 8) * SL_COPIES + copy], 1ull);
    }
  });
  best = sl_block_max(best, scratch);
  const uint32_t maxkey = (uint32_t)(best >> 32);
  const long argmax = (long)(0xFFFFFFFFu - (uint32_t)best);
  if (!sampled || maxkey <= SL_KEY_NEG_INF) {
    if (tid == 0) out[row] = maxkey <= SL_KEY_NEG_INF ? 0 : argmax;
    return;
  }

  // top-k: kk = key of the k-th largest, K = {key >= kk}
  uint32_t kk = 0u;
  if (use_k) {
    const SlSel s1 = sl_select(hist, (sl_u64)k, scratch, &sh_sel);
    if (s1.bin >= 0) {
      const uint32_t b1 = (uint32_t)s1.bin;
      sl_hist_pass(r, hist, [b1](uint32_t key, int& bin, sl_u64& val) {
        bin = (int)(key & 255u);
        val = 1ull;
        return (key >> 8) == b1;
      });
      const SlSel s2 =
          sl_select(hist, (sl_u64)k - s1.above, scratch, &sh_sel);
      if (s2.bin >= 0) kk = (b1 << 8) | (uint32_t)s2.bin;
    }
  }

  // top-p over the weights of K: nk = key of the last distinct value
  // kept, N = {key >= nk}
  const float lmax = sl_key_value(maxkey);
  const float scale = (1.0f / temp) * 1.44269504088896341f;
  uint32_t nk = kk;
  if (use_p) {
    const sl_u64 s_k = sl_block_sum(
        sl_hist_pass(r, hist,
                     [=](uint32_t key, int& bin, sl_u64& val) {
                       if (key < kk) return false;
                       bin = (int)(key >> 8);
                       val = sl_weight(key, maxkey, lmax, scale);
                       return true;
                     }),
        scratch);
    // smallest integer mass m with m >= top_p * s_k
    const double thr = ceil((double)p * (double)s_k);
    sl_u64 need = thr > 1.0 ? (sl_u64)thr : 1ull;
    if (need > s_k) need = s_k;
    const SlSel s1 = sl_select(hist, need, scratch, &sh_sel);
    if (s1.bin >= 0) {
      const uint32_t b1 = (uint32_t)s1.bin;
      sl_hist_pass(r, hist, [=](uint32_t key, int& bin, sl_u64& val) {
        if (key < kk || (key >> 8) != b1) return false;
        bin = (int)(key & 255u);
        val = sl_weight(key, maxkey, lmax, scale);
        return true;
      });
      const SlSel s2 = sl_select(hist, need - s1.above, scratch, &sh_sel);
      if (s2.bin >= 0) nk = (b1 << 8) | (uint32_t)s2.bin;
    }
  }

  // the weight of N per wave chunk; their sum is s_n. Chunks are in
  // index order, so the wave whose chunk holds the draw is known from
  // the totals alone.
  sl_u64 mine = 0;
  int last = -1;  // highest index of N this thread saw
  sl_for_each(r, [&](const uint32_t key[8], int e0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (key[j] != 0u && key[j] >= nk) {
        mine += sl_weight(key[j], maxkey, lmax, scale);
        last = e0 + j > last ? e0 + j : last;
      }
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
  if ((tid & 63) == 0) scratch[tid >> 6] = mine;
  if (tid == 0) sh_found = -1;
  __syncthreads();
  sl_u64 s_n = 0, before = 0;  // before: weight of the chunks in front
#pragma unroll
  for (int i = 0; i < SL_WAVES; ++i) {
    if (i < (tid >> 6)) before += scratch[i];
    s_n += scratch[i];
  }

  // the draw: first index of N whose running weight exceeds u * s_n,
  // i.e. exceeds floor(m * s_n / 2^24) with u = m * 2^-24
  const sl_u64 m = (sl_u64)(sl_philox_word0(seed[row], (sl_u64)step[row]) >> 8);
  const sl_u64 target = (__umul64hi(m, s_n) << 40) | ((m * s_n) >> 24);
  if (mine != 0ull && before <= target && target < before + mine) {
    // this wave's chunk holds it: walk the chunk in order, one wave scan
    // per 64 vectors, the next load issued before the current is used
    int lo, hi;
    sl_chunk(r, lo, hi);
    sl_u64 running = before;
    int v = lo + (tid & 63);
    SlVec cur = sl_load(r, v, hi);
    for (; v - (tid & 63) < hi; v += 64) {
      const SlVec nxt = sl_load(r, v + 64, hi);
      uint32_t key[8];
      sl_u64 w[8];
      sl_keys(cur, key);
      sl_u64 sum = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w[j] = (key[j] != 0u && key[j] >= nk)
                   ? sl_weight(key[j], maxkey, lmax, scale)
                   : 0ull;
        sum += w[j];
      }
      const sl_u64 incl = sl_wave_scan(sum);
      sl_u64 cum = running + incl - sum;  // weight before this lane
      const bool here = sum != 0ull && cum <= target && target < cum + sum;
      if (here) {
        int found = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          cum += w[j];
          if (found < 0 && w[j] != 0ull && cum > target) found = cur.e0 + j;
        }
        sh_found = found;
      }
      if (__any(here)) break;
      running += __shfl(incl, 63);
      cur = nxt;
    }
  }
  __syncthreads();
  int found = sh_found;
  if (found < 0) {
    // no running sum passed the target (only if every weight is zero):
    // the last index of N
    const sl_u64 l = sl_block_max((sl_u64)(last + 1), scratch);
    found = l > 0 ? (int)(l - 1) : (int)argmax;
  }
  if (tid == 0) out[row] = found;
}

extern "C" hipError_t ca_sample_logits_bf16(
    const void* logits, const void* temperature, const void* top_k,
    const void* top_p, const void* seed, const void* step, void* out,
    long rows, int vocab, hipStream_t stream) {
  if (rows < 0 || rows > 0x7FFFFFFFl || vocab < 1) return hipErrorInvalidValue;
  if ((uintptr_t)logits & 1) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;  // nothing to do; a zero grid is invalid
  hipLaunchKernelGGL(sample_logits_bf16_kernel, dim3((uint32_t)rows),
                     dim3(SL_THREADS), 0, stream, (const uint16_t*)logits,
                     (const float*)temperature, (const int*)top_k,
                     (const float*)top_p, (const sl_u64*)seed,
                     (const long*)step, (long*)out, vocab);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// ResNet epilogues: per-channel bias (+ residual) (+ ReLU) over bf16
// ---------------------------------------------------------------------------

namespace {

// optional ReLU, then RNE back to bf16
__device__ __forceinline__ uint16_t epilogue_finish(float f, int do_relu) {
  if (do_relu && f < 0.f) f = 0.f;
  return f32_to_bf16_cvt(f);
}

// One packed pair of bf16 elements through the epilogue: x (and the
// residual pair when has_res) with the biases of its two elements.
// The addition order (x + residual) + bias matches the torch reference
// sequence exactly (fp32 add is non-associative; a different order
// flips RNE boundary cases).
__device__ __forceinline__ uint32_t epilogue_pair(uint32_t xw, uint32_t rw,
                                                  bool has_res, float b_lo,
                                                  float b_hi, int do_relu) {
  float lo = bf16x2_lo(xw);
  float hi = bf16x2_hi(xw);
  if (has_res) {
    lo += bf16x2_lo(rw);
    hi += bf16x2_hi(rw);
  }
  lo += b_lo;
  hi += b_hi;
  if (do_relu && lo < 0.f) lo = 0.f;
  if (do_relu && hi < 0.f) hi = 0.f;
  return f32x2_to_bf16x2_cvt(lo, hi);
}

// the same for one element of a ragged end (res may be null)
__device__ __forceinline__ uint16_t epilogue_one(const uint16_t* x,
                                                 const uint16_t* res, long i,
                                                 float b, int do_relu) {
  float f = bf16_to_f32(x[i]);
  if (res) f += bf16_to_f32(res[i]);
  return epilogue_finish(f + b, do_relu);
}

}  // namespace

// Per-plane NCHW epilogue, in-place capable. Without the residual it
// absorbs the separate elementwise bias pass torch-on-ROCm emits for
// conv biases created by BatchNorm folding (55 ms / 5247 calls in the
// ResNet50 serving profile). With it, it is the bottleneck-exit fusion
// (out = relu(x + bias[c] + residual)): after BN folding, torch-on-ROCm
// runs this as three elementwise kernels (bias add, residual add,
// relu), i.e. 3 extra full memory passes over the activation per block
// exit; this kernel is one read-x + read-residual + write pass. fp32
// math, RNE back to bf16.
//
// One block per (n,c) plane: the fp32 bias loads once, elements stream
// 8-wide. There is no scalar tail: the launcher sends only planes with
// ca_epilogue_per_plane(plane), i.e. plane % 8 == 0, here; every other
// plane size (incl. 7x7=49) takes the flat kernels.
template <bool HAS_RES>
__device__ __forceinline__ void bias_res_act_plane_body(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
    const float* __restrict__ bias, uint16_t* __restrict__ out, long plane,
    int channels, int do_relu) {
  const long pidx = blockIdx.x;  // n*C + c
  const int c = (int)(pidx % channels);
  const float b = bias[c];
  const long vec_n = plane / 8;
  const uint4* xv = (const uint4*)(x + pidx * plane);
  const uint4* rv = HAS_RES ? (const uint4*)(res + pidx * plane) : nullptr;
  uint4* ov = (uint4*)(out + pidx * plane);
  for (long i = threadIdx.x; i < vec_n; i += blockDim.x) {
    uint4 v = xv[i];
    uint4 r = uint4{0, 0, 0, 0};
    if (HAS_RES) r = rv[i];
    uint32_t* w = (uint32_t*)&v;
    const uint32_t* rw = (const uint32_t*)&r;
    for (int j = 0; j < 4; ++j)
      w[j] = epilogue_pair(w[j], rw[j], HAS_RES, b, b, do_relu);
    ov[i] = v;
  }
}

extern "C" __global__ void bias_act_bf16_kernel(
    const uint16_t* __restrict__ x, const float* __restrict__ bias,
    uint16_t* __restrict__ out, long plane, int channels, int do_relu) {
  bias_res_act_plane_body<false>(x, nullptr, bias, out, plane, channels,
                                 do_relu);
}

extern "C" __global__ void bias_res_act_bf16_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
    const float* __restrict__ bias, uint16_t* __restrict__ out, long plane,
    int channels, int do_relu) {
  bias_res_act_plane_body<true>(x, res, bias, out, plane, channels, do_relu);
}

// Flat-indexed NCHW epilogue: the same per-element math as the
// per-plane kernels above, but swept over the whole n_planes*plane
// tensor as one stream of 16-byte vectors (8 bf16 per lane per
// iteration, grid-stride, every access 16-byte aligned). One block per
// (n,c) plane only fills the lanes at 56x56; at 28x28 / 14x14 / 7x7 a
// 256-thread block has 98 / 24 / 6 vectors, every other 14x14 or 7x7
// plane base is not 16-byte aligned, and layer4 at batch 32 is 65,536
// blocks of ~100 bytes each.
//
// A lane tracks (c, off) = (channel, offset inside the plane) of its
// vector's first element and advances both by the host-computed grid
// stride (step_c, step_off), so the loop has no division. A vector
// that crosses a plane boundary switches bias per element: with
// plane >= 8 it crosses at most one boundary (two biases, selected by
// position), with plane < 8 it walks the boundaries element by element.
// The last total % 8 elements take a scalar path in block 0.
template <bool HAS_RES>
__device__ __forceinline__ void bias_res_act_flat_body(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
    const float* __restrict__ bias, uint16_t* __restrict__ out, long total,
    long plane, int channels, long step_off, int step_c, int do_relu) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t e0 = tid * 8u;  // grid <= 2048 blocks: e0 < 2^22
  // plane <= e0 implies plane < 2^22, so the 32-bit division is exact
  const uint32_t q0 = (plane <= (long)e0) ? e0 / (uint32_t)plane : 0u;
  long off = (long)e0 - (long)q0 * plane;
  int c = (int)(q0 % (uint32_t)channels);
  const long stride = (long)gridDim.x * blockDim.x * 8;

  for (long e = e0; e + 8 <= total; e += stride) {
    uint4 v = *reinterpret_cast<const uint4*>(x + e);
    uint4 r = uint4{0, 0, 0, 0};
    if (HAS_RES) r = *reinterpret_cast<const uint4*>(res + e);

    float bv[8];
    if ((plane & 7) == 0) {
      // planes are whole vectors: no vector crosses a boundary
      const float b0 = bias[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = b0;
    } else if (plane >= 8) {
      const int c1 = (c + 1 == channels) ? 0 : c + 1;
      const float b0 = bias[c];
      const float b1 = bias[c1];
      // elements left in this plane (>= 1), clamped to the vector
      const int k = (plane - off >= 8) ? 8 : (int)(plane - off);
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = (j < k) ? b0 : b1;
    } else {
      long oj = off;
      int cj = c;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bv[j] = bias[cj];
        if (++oj == plane) {
          oj = 0;
          if (++cj == channels) cj = 0;
        }
      }
    }

    uint32_t* w = (uint32_t*)&v;
    const uint32_t* rw = (const uint32_t*)&r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = epilogue_pair(w[j], rw[j], HAS_RES, bv[2 * j], bv[2 * j + 1],
                           do_relu);
    *reinterpret_cast<uint4*>(out + e) = v;

    off += step_off;
    c += step_c;
    if (off >= plane) {
      off -= plane;
      ++c;
    }
    if (c >= channels) c -= channels;
  }

  // ragged end: at most 7 elements, first lanes of block 0
  const long ti = (total / 8) * 8 + tid;
  if (tid < 8 && ti < total) {
    out[ti] = epilogue_one(x, HAS_RES ? res : nullptr, ti,
                           bias[(ti / plane) % channels], do_relu);
  }
}

extern "C" __global__ void __launch_bounds__(256)
bias_act_flat_bf16_kernel(const uint16_t* __restrict__ x,
                          const float* __restrict__ bias,
                          uint16_t* __restrict__ out, long total, long plane,
                          int channels, long step_off, int step_c,
                          int do_relu) {
  bias_res_act_flat_body<false>(x, nullptr, bias, out, total, plane,
                                channels, step_off, step_c, do_relu);
}

extern "C" __global__ void __launch_bounds__(256)
bias_res_act_flat_bf16_kernel(const uint16_t* __restrict__ x,
                              const uint16_t* __restrict__ res,
                              const float* __restrict__ bias,
                              uint16_t* __restrict__ out, long total,
                              long plane, int channels, long step_off,
                              int step_c, int do_relu) {
  bias_res_act_flat_body<true>(x, res, bias, out, total, plane, channels,
                               step_off, step_c, do_relu);
}

namespace {

// The per-plane kernels keep the planes where every lane of a block owns
// at least one aligned vector (56x56 and larger): there they run at
// 6.2-6.6 TB/s at batch 32, 5-15 % ahead of the flat sweep. Everything
// smaller, or not a multiple of 8, takes the flat kernels.
inline bool ca_epilogue_per_plane(long plane) {
  return plane % 8 == 0 && plane >= 2048;
}

// shared launcher of the two flat epilogue kernels (res may be null)
hipError_t ca_launch_flat_epilogue(const void* x, const void* res,
                                   const void* bias, void* out,
                                   long n_planes, long plane, int channels,
                                   int do_relu, hipStream_t stream) {
  if (n_planes < 0 || plane < 0 || channels < 1) return hipErrorInvalidValue;
  const long total = n_planes * plane;
  if (total == 0) return hipSuccess;
  const int grid = ca_grid_for(total / 8);
  // per-iteration advance of a lane's (channel, offset-in-plane)
  const long stride = (long)grid * 256 * 8;
  const long step_off = stride % plane;
  const int step_c = (int)((stride / plane) % channels);
  if (res) {
    hipLaunchKernelGGL(bias_res_act_flat_bf16_kernel, dim3(grid), dim3(256),
                       0, stream, (const uint16_t*)x, (const uint16_t*)res,
                       (const float*)bias, (uint16_t*)out, total, plane,
                       channels, step_off, step_c, do_relu);
  } else {
    hipLaunchKernelGGL(bias_act_flat_bf16_kernel, dim3(grid), dim3(256), 0,
                       stream, (const uint16_t*)x, (const float*)bias,
                       (uint16_t*)out, total, plane, channels, step_off,
                       step_c, do_relu);
  }
  return hipGetLastError();
}

}  // namespace

// residual may be null (degenerates to bias[+relu])
extern "C" hipError_t ca_bias_res_act_bf16(const void* x, const void* res,
                                           const void* bias, void* out,
                                           long n_planes, long plane,
                                           int channels, int do_relu,
                                           hipStream_t stream) {
  if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) ||
      ((uintptr_t)res & 15)) {
    return hipErrorInvalidValue;  // 16B alignment for the uint4 path
  }
  if (!ca_epilogue_per_plane(plane)) {
    return ca_launch_flat_epilogue(x, res, bias, out, n_planes, plane,
                                   channels, do_relu, stream);
  }
  if (n_planes <= 0) return n_planes ? hipErrorInvalidValue : hipSuccess;
  if (res) {
    hipLaunchKernelGGL(bias_res_act_bf16_kernel, dim3((uint32_t)n_planes),
                       dim3(256), 0, stream, (const uint16_t*)x,
                       (const uint16_t*)res, (const float*)bias,
                       (uint16_t*)out, plane, channels, do_relu);
  } else {
    hipLaunchKernelGGL(bias_act_bf16_kernel, dim3((uint32_t)n_planes),
                       dim3(256), 0, stream, (const uint16_t*)x,
                       (const float*)bias, (uint16_t*)out, plane, channels,
                       do_relu);
  }
  return hipGetLastError();
}

extern "C" hipError_t ca_bias_act_bf16(const void* x, const void* bias,
                                       void* out, long n_planes, long plane,
                                       int channels, int do_relu,
                                       hipStream_t stream) {
  return ca_bias_res_act_bf16(x, nullptr, bias, out, n_planes, plane,
                              channels, do_relu, stream);
}

// fused 3x3 conv + bias + ReLU (shares epilogue_finish with the above)
#include "conv3x3.hip"

// Channels-LAST (NHWC-contiguous) variant: channel is the fastest
// dim, so each lane's 8 consecutive elements are 8 consecutive
// channels — loads of x, residual AND bias all coalesce. This is what
// lets the fused epilogues ride MIOpen's native NHWC conv path
// (channels_last measured catastrophic in r01 precisely because the
// NCHW-plane kernels fell back to eager torch ops on NHWC tensors).
// Requires channels % 8 == 0 (ResNet: 64..2048, all satisfy).
extern "C" __global__ void bias_res_act_cl_bf16_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
    const float* __restrict__ bias, uint16_t* __restrict__ out, long n,
    int channels, int do_relu) {
  long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 8;
  long stride = (long)gridDim.x * blockDim.x * 8;
  for (long i = i0; i + 8 <= n; i += stride) {
    const int c0 = (int)(i % channels);
    uint4 v = *reinterpret_cast<const uint4*>(x + i);
    uint4 r = res ? *reinterpret_cast<const uint4*>(res + i)
                  : uint4{0, 0, 0, 0};
    const float4 b0 = *reinterpret_cast<const float4*>(bias + c0);
    const float4 b1 = *reinterpret_cast<const float4*>(bias + c0 + 4);
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const uint32_t* w = (const uint32_t*)&v;
    const uint32_t* rw = (const uint32_t*)&r;
    uint16_t o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p = epilogue_pair(w[j], rw[j], res != nullptr, bv[2 * j],
                                       bv[2 * j + 1], do_relu);
      o[2 * j] = (uint16_t)p;
      o[2 * j + 1] = (uint16_t)(p >> 16);
    }
    *reinterpret_cast<uint4*>(out + i) = *reinterpret_cast<uint4*>(o);
  }
  // tail (n % 8 == 0 whenever channels % 8 == 0, but keep it safe)
  long tail = (n / 8) * 8;
  long ti = tail + (blockIdx.x * blockDim.x + threadIdx.x);
  if (ti < n && (blockIdx.x * blockDim.x + threadIdx.x) < 8) {
    out[ti] = epilogue_one(x, res, ti, bias[ti % channels], do_relu);
  }
}

extern "C" hipError_t ca_bias_res_act_cl_bf16(const void* x, const void* res,
                                              const void* bias, void* out,
                                              long n, int channels,
                                              int do_relu,
                                              hipStream_t stream) {
  if (channels % 8 != 0) return hipErrorInvalidValue;
  if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) ||
      ((uintptr_t)res & 15)) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(bias_res_act_cl_bf16_kernel,
                     dim3(ca_grid_for((n + 7) / 8)), dim3(256), 0, stream,
                     (const uint16_t*)x, (const uint16_t*)res,
                     (const float*)bias, (uint16_t*)out, n, channels,
                     do_relu);
  return hipGetLastError();
}

// ResNet stem epilogue in one pass: per-channel bias + ReLU + 3x3
// stride-2 pad-1 max-pool over an NCHW bf16 conv output. Replaces a
// bias+ReLU pass that read and wrote the full 112x112 map followed by
// torch's NCHW max-pool reading it again (49 us per batch-32 forward
// where the bytes alone take ~13 us). Each element is computed exactly
// as the epilogue kernels do (fp32 add, ReLU, RNE to bf16) and the max
// is taken over those bf16 values in torch's scan order with torch's
// rule (v > m || isnan(v)), so the result is bit-identical to
// max_pool2d(relu(x + b).to(bf16), 3, 2, 1), NaN included. Padding
// contributes nothing (-inf never wins).
//
// A thread produces 4 adjacent output pixels of one row from 9 input
// columns of up to 3 rows. VEC (w % 8 == 0, 16-byte aligned bases):
// each row is one aligned 16-byte load plus the left neighbour, and
// the 4 outputs leave as one 8-byte store.
template <bool VEC>
__device__ __forceinline__ void bias_relu_maxpool_body(
    const uint16_t* __restrict__ x, const float* __restrict__ bias,
    uint16_t* __restrict__ out, uint32_t total, int channels, int h, int w,
    int oh_n, int ow_n, int groups) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint32_t g = t % (uint32_t)groups;
  const uint32_t row = t / (uint32_t)groups;
  const int oh = (int)(row % (uint32_t)oh_n);
  const uint32_t pl = row / (uint32_t)oh_n;  // n*C + c
  const float b = bias[pl % (uint32_t)channels];

  // the epilogue's bf16 result, widened back to float for the max
  auto act = [&](uint16_t v) -> float {
    return bf16_to_f32(epilogue_finish(bf16_to_f32(v) + b, 1));
  };

  const float ninf = __uint_as_float(0xFF800000u);
  float m[4] = {ninf, ninf, ninf, ninf};
  const int iw0 = 8 * (int)g - 1;  // input column of r[0]
  const uint16_t* xp = x + (size_t)pl * h * w;

#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * oh - 1 + kh;
    if (ih < 0 || ih >= h) continue;
    const uint16_t* xr = xp + (size_t)ih * w;
    float r[9];
    if (VEC) {
      const uint4 v = *reinterpret_cast<const uint4*>(xr + iw0 + 1);
      const uint32_t* vw = (const uint32_t*)&v;
      r[0] = (iw0 >= 0) ? act(xr[iw0]) : ninf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[1 + 2 * j] = act((uint16_t)(vw[j] & 0xFFFFu));
        r[2 + 2 * j] = act((uint16_t)(vw[j] >> 16));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const int iw = iw0 + i;
        r[i] = (iw >= 0 && iw < w) ? act(xr[iw]) : ninf;
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float v = r[2 * o + kw];
        if (v > m[o] || v != v) m[o] = v;
      }
    }
  }

  // m[] holds bf16 values, so truncation is exact
  uint16_t* op = out + ((size_t)pl * oh_n + oh) * ow_n + 4 * g;
  if (VEC) {
    uint2 o2;
    o2.x = (__float_as_uint(m[0]) >> 16) | (__float_as_uint(m[1]) & 0xFFFF0000u);
    o2.y = (__float_as_uint(m[2]) >> 16) | (__float_as_uint(m[3]) & 0xFFFF0000u);
    *reinterpret_cast<uint2*>(op) = o2;
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (4 * (int)g + o < ow_n) op[o] = f32_to_bf16_trunc(m[o]);
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
bias_relu_maxpool_bf16_kernel(const uint16_t* __restrict__ x,
                              const float* __restrict__ bias,
                              uint16_t* __restrict__ out, uint32_t total,
                              int channels, int h, int w, int oh_n, int ow_n,
                              int groups) {
  bias_relu_maxpool_body<true>(x, bias, out, total, channels, h, w, oh_n,
                               ow_n, groups);
}

extern "C" __global__ void __launch_bounds__(256)
bias_relu_maxpool_scalar_bf16_kernel(const uint16_t* __restrict__ x,
                                     const float* __restrict__ bias,
                                     uint16_t* __restrict__ out,
                                     uint32_t total, int channels, int h,
                                     int w, int oh_n, int ow_n, int groups) {
  bias_relu_maxpool_body<false>(x, bias, out, total, channels, h, w, oh_n,
                                ow_n, groups);
}

// x: [n_planes = N*C, h, w] bf16, out: [n_planes, (h-1)/2+1, (w-1)/2+1]
extern "C" hipError_t ca_bias_relu_maxpool_bf16(const void* x,
                                                const void* bias, void* out,
                                                long n_planes, int channels,
                                                int h, int w,
                                                hipStream_t stream) {
  if (n_planes < 0 || channels < 1 || h < 1 || w < 1) {
    return hipErrorInvalidValue;
  }
  const int oh_n = (h - 1) / 2 + 1;
  const int ow_n = (w - 1) / 2 + 1;
  const int groups = (ow_n + 3) / 4;
  const long total = n_planes * oh_n * groups;  // one thread per 4 outputs
  if (total == 0) return hipSuccess;
  if (total > 0x7FFFFFFFL) return hipErrorInvalidValue;  // 32-bit indexing
  const dim3 grid((uint32_t)((total + 255) / 256));
  const bool vec = (w % 8 == 0) && !((uintptr_t)x & 15) &&
                   !((uintptr_t)out & 7);
  if (vec) {
    hipLaunchKernelGGL(bias_relu_maxpool_bf16_kernel, grid, dim3(256), 0,
                       stream, (const uint16_t*)x, (const float*)bias,
                       (uint16_t*)out, (uint32_t)total, channels, h, w, oh_n,
                       ow_n, groups);
  } else {
    hipLaunchKernelGGL(bias_relu_maxpool_scalar_bf16_kernel, grid, dim3(256),
                       0, stream, (const uint16_t*)x, (const float*)bias,
                       (uint16_t*)out, (uint32_t)total, channels, h, w, oh_n,
                       ow_n, groups);
  }
  return hipGetLastError();
}
