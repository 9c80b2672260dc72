// FP8 (e4m3) weight-only linear layers for LLM decode. Included by
// kernels.hip (uses its CastFp8ToF32 and ca_grid_for).
//
// Storage (client_amd/models/weight_fp8.py is the host side): a weight
// W[N, K] is `codes`, OCP e4m3fn bytes, and `scale_exp`, int8 [N];
// W_eff[n, k] = decode(codes[n, k]) * 2^scale_exp[n], which is exactly a
// bf16 value. K is a multiple of 64.
//
// `codes` is stored pre-tiled, so that one wave's 16-byte lane loads of
// one (16 rows x 64 k) tile are one lane-linear 1 KiB run:
//
//   packed[((t * K/64 + c) * 64 + lane) * 16 + b]
//       = codes[16 t + (lane & 15)][64 c + 16 (lane >> 4) + b]
//
// with the rows padded to a multiple of 16 (pad rows feed only output
// rows >= N, which nobody writes). Chosen over row-major [N, K] because
// there a wave's load touches 16 rows x 64 B, half a 128-byte line per
// row, and the tail tile needs its rows clamped; the weights are static,
// so the permutation costs nothing at run time. pack_codes /
// unpack_codes in weight_fp8.py are the executable statement.
//
// ca_fp8w_decode_gemm_bf16: y[M, N] = bf16_rne(2^scale_exp[n] *
// sum_k x[m, k] decode(codes[n, k])) for 1 <= M <= 16, W8A16 (x is not
// quantised). One workgroup per 16-row tile; its waves split the K/64
// chunks round robin; a wave's loads go global -> VGPR, FW_UNROLL chunks
// in flight before the first use; codes become bf16 in registers (every
// e4m3 value is a bf16 value: hardware convert to fp32, keep the high
// halves) and feed v_mfma_f32_16x16x32_bf16 as the A operand, the rows
// of x as B. A 16-byte weight load holds the k of two MFMA steps; the k
// order inside a step is permuted the same way on both operands. The
// waves' partial tiles are summed through LDS in wave order. Which wave
// sums which chunk, and the number of waves, depend on (N, K) alone:
// a row's output bits depend neither on M nor on the other rows.
//
// ca_fp8w_dequant_bf16: packed codes -> the bf16 bits of W_eff, row-major
// [N, K]; for the prefill route, which runs the library GEMM on it.

#define FW_ROWS 16      // output channels per tile (MFMA A rows)
#define FW_KCHUNK 64    // k per tile: 64 lanes x 16 B / 16 rows
#define FW_UNROLL 4     // chunks whose loads are in flight together
#define FW_MAX_M 16

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 fw_frag_ab;
typedef __attribute__((ext_vector_type(4))) float fw_frag_cd;
typedef __attribute__((ext_vector_type(2))) float fw_f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t fw_u32x4;

union fw_frag_u {
  fw_u32x4 u;
  fw_frag_ab f;
};

// two e4m3 codes (one 16-bit half of w) -> two bf16, the lower address
// in the low half
__device__ __forceinline__ uint32_t fw_codes2_to_bf16x2(uint32_t w, bool hi) {
#if defined(__gfx950__)
  const fw_f32x2 f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true)
                        : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  // (f[1] & 0xFFFF0000) | (f[0] >> 16)
  return __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]),
                               0x07060302u);
#else
  const uint32_t h = hi ? (w >> 16) : w;
  const float f0 = CastFp8ToF32::convert((uint8_t)(h & 0xFF));
  const float f1 = CastFp8ToF32::convert((uint8_t)((h >> 8) & 0xFF));
  return (__float_as_uint(f1) & 0xFFFF0000u) | (__float_as_uint(f0) >> 16);
#endif
}

// the 8 codes in (lo, hi) -> one MFMA operand fragment
__device__ __forceinline__ fw_frag_ab fw_codes8_to_frag(uint32_t lo,
                                                        uint32_t hi) {
  fw_frag_u a;
  a.u = fw_u32x4{fw_codes2_to_bf16x2(lo, false),
                 fw_codes2_to_bf16x2(lo, true),
                 fw_codes2_to_bf16x2(hi, false),
                 fw_codes2_to_bf16x2(hi, true)};
  return a.f;
}

// 2^e for e in [-126, 127]
__device__ __forceinline__ float fw_exp2i(int e) {
  return __uint_as_float((uint32_t)(127 + e) << 23);
}

// one chunk: two MFMA steps of 32 k each
__device__ __forceinline__ fw_frag_cd fw_chunk_mfma(const fw_u32x4& w,
                                                    const fw_u32x4& x0,
                                                    const fw_u32x4& x1,
                                                    fw_frag_cd acc) {
  fw_frag_u b0, b1;
  b0.u = x0;
  b1.u = x1;
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw_codes8_to_frag(w.x, w.y),
                                                b0.f, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw_codes8_to_frag(w.z, w.w),
                                                b1.f, acc, 0, 0, 0);
  return acc;
}

template <int WAVES>
__device__ __forceinline__ void fw_decode_gemm_body(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ packed,
    const int8_t* __restrict__ scale_exp, uint16_t* __restrict__ y, int M,
    int N, int K) {
  __shared__ alignas(16) float s_part[WAVES][64 * 4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile = blockIdx.x;
  const int kc = K / FW_KCHUNK;
  // lane (m, q): B holds x[m][64 c + 16 q + 8 s + j] at step s, the k of
  // the weight lane (r, q)'s bytes 8 s + j. Columns m >= M repeat row
  // M - 1: they feed only output columns nobody writes, and x is never
  // read beyond its last row.
  const int m = lane & 15;
  const int q = lane >> 4;
  const uint16_t* xrow =
      x + (long)(m < M ? m : M - 1) * K + 16 * q;
  const fw_u32x4* wt =
      reinterpret_cast<const fw_u32x4*>(packed) + (long)tile * kc * 64 + lane;

  fw_frag_cd acc = {0.f, 0.f, 0.f, 0.f};
  int c = wave;
  for (; c + (FW_UNROLL - 1) * WAVES < kc; c += FW_UNROLL * WAVES) {
    fw_u32x4 w[FW_UNROLL], x0[FW_UNROLL], x1[FW_UNROLL];
#pragma unroll
    for (int u = 0; u < FW_UNROLL; ++u)
      w[u] = __builtin_nontemporal_load(wt + (long)(c + u * WAVES) * 64);
#pragma unroll
    for (int u = 0; u < FW_UNROLL; ++u) {
      const uint16_t* xp = xrow + (long)(c + u * WAVES) * FW_KCHUNK;
      x0[u] = *reinterpret_cast<const fw_u32x4*>(xp);
      x1[u] = *reinterpret_cast<const fw_u32x4*>(xp + 8);
    }
    // every load of the step issued before the first use (left alone,
    // the scheduler sinks each load to its convert)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < FW_UNROLL; ++u)
      acc = fw_chunk_mfma(w[u], x0[u], x1[u], acc);
  }
  for (; c < kc; c += WAVES) {
    const fw_u32x4 w = __builtin_nontemporal_load(wt + (long)c * 64);
    const uint16_t* xp = xrow + (long)c * FW_KCHUNK;
    const fw_u32x4 x0 = *reinterpret_cast<const fw_u32x4*>(xp);
    const fw_u32x4 x1 = *reinterpret_cast<const fw_u32x4*>(xp + 8);
    acc = fw_chunk_mfma(w, x0, x1, acc);
  }

  // D[n = 4 (lane >> 4) + i][m = lane & 15] in acc[i]
  *reinterpret_cast<fw_frag_cd*>(&s_part[wave][lane * 4]) = acc;
  __syncthreads();
  // thread t < 256 owns element (lane t >> 2, register t & 3); the
  // partials are added in wave order
  for (int t = threadIdx.x; t < 64 * 4; t += WAVES * 64) {
    float s = s_part[0][t];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += s_part[w][t];
    const int l = t >> 2;
    const int om = l & 15;
    const int on = tile * FW_ROWS + 4 * (l >> 4) + (t & 3);
    if (om < M && on < N)
      y[(long)om * N + on] = __bfloat16_as_ushort(
          __float2bfloat16(s * fw_exp2i(scale_exp[on])));
  }
}

}  // namespace

template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64)
fp8w_decode_gemm_kernel(const uint16_t* __restrict__ x,
                        const uint8_t* __restrict__ packed,
                        const int8_t* __restrict__ scale_exp,
                        uint16_t* __restrict__ y, int M, int N, int K) {
  fw_decode_gemm_body<WAVES>(x, packed, scale_exp, y, M, N, K);
}

// One 16-byte lane load of packed codes (16 consecutive k of one row)
// per item, two 16-byte stores of bf16. A wave's stores are 16 rows x
// 128 B.
extern "C" __global__ void __launch_bounds__(256)
fp8w_dequant_kernel(const uint8_t* __restrict__ packed,
                    const int8_t* __restrict__ scale_exp,
                    uint16_t* __restrict__ w_out, int N, int K, long items) {
  const int kc = K / FW_KCHUNK;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items;
       i += stride) {
    const int lane = (int)(i & 63);
    const long tc = i >> 6;  // tile * kc + chunk
    const long n = (tc / kc) * FW_ROWS + (lane & 15);
    if (n >= N) continue;
    const int k = (int)(tc % kc) * FW_KCHUNK + 16 * (lane >> 4);
    const uint4 w = reinterpret_cast<const uint4*>(packed)[i];
    const float sc = fw_exp2i(scale_exp[n]);
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#if defined(__gfx950__)
      const fw_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[j], false);
      const fw_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u[j], true);
      const float f[4] = {lo[0], lo[1], hi[0], hi[1]};
#else
      float f[4];
      for (int b = 0; b < 4; ++b)
        f[b] = CastFp8ToF32::convert((uint8_t)(u[j] >> (8 * b)));
#endif
      // exact: at most 4 significant bits times a power of two, so the
      // product's low 16 bits are zero
      o[2 * j] = (__float_as_uint(f[1] * sc) & 0xFFFF0000u) |
                 (__float_as_uint(f[0] * sc) >> 16);
      o[2 * j + 1] = (__float_as_uint(f[3] * sc) & 0xFFFF0000u) |
                     (__float_as_uint(f[2] * sc) >> 16);
    }
    uint4* dst = reinterpret_cast<uint4*>(w_out + n * (long)K + k);
    dst[0] = uint4{o[0], o[1], o[2], o[3]};
    dst[1] = uint4{o[4], o[5], o[6], o[7]};
  }
}

namespace {

// waves per workgroup, from the shape alone: fewer waves where there are
// enough tiles to fill the CUs several times over, never more than
// chunks
inline int fw_waves_for(int N, int K) {
  const long tiles = ((long)N + FW_ROWS - 1) / FW_ROWS;
  const int kc = K / FW_KCHUNK;
  int waves = tiles >= 1024 ? 4 : tiles >= 512 ? 8 : 16;
  while (waves > 4 && waves / 2 >= kc) waves /= 2;
  return waves;
}

}  // namespace

// x [M, K] bf16, packed codes of W[N, K] (layout above), scale_exp [N]
// int8, y [M, N] bf16. 1 <= M <= 16, N >= 1, K % 64 == 0; x and packed
// 16-byte aligned, y 2-byte aligned. Anything else returns
// hipErrorInvalidValue before any launch.
extern "C" hipError_t ca_fp8w_decode_gemm_bf16(const void* x,
                                               const void* codes,
                                               const void* scale_exp, void* y,
                                               int M, int N, int K,
                                               hipStream_t stream) {
  if (M < 1 || M > FW_MAX_M || N < 1 || K < FW_KCHUNK || K % FW_KCHUNK != 0)
    return hipErrorInvalidValue;
  if (!x || !codes || !scale_exp || !y) return hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)codes) % 16 != 0 || (uintptr_t)y % 2 != 0)
    return hipErrorInvalidValue;
  const long tiles = ((long)N + FW_ROWS - 1) / FW_ROWS;
#define FW_LAUNCH(WAVES)                                                     \
  hipLaunchKernelGGL((fp8w_decode_gemm_kernel<WAVES>), dim3((uint32_t)tiles), \
                     dim3(WAVES * 64), 0, stream, (const uint16_t*)x,        \
                     (const uint8_t*)codes, (const int8_t*)scale_exp,        \
                     (uint16_t*)y, M, N, K)
  switch (fw_waves_for(N, K)) {
    case 4: FW_LAUNCH(4); break;
    case 8: FW_LAUNCH(8); break;
    default: FW_LAUNCH(16); break;
  }
#undef FW_LAUNCH
  return hipGetLastError();
}

// packed codes of W[N, K] -> w_out [N, K] bf16 = W_eff. K % 64 == 0;
// codes and w_out 16-byte aligned.
extern "C" hipError_t ca_fp8w_dequant_bf16(const void* codes,
                                           const void* scale_exp, void* w_out,
                                           int N, int K, hipStream_t stream) {
  if (N < 1 || K < FW_KCHUNK || K % FW_KCHUNK != 0)
    return hipErrorInvalidValue;
  if (!codes || !scale_exp || !w_out) return hipErrorInvalidValue;
  if (((uintptr_t)codes | (uintptr_t)w_out) % 16 != 0)
    return hipErrorInvalidValue;
  const long tiles = ((long)N + FW_ROWS - 1) / FW_ROWS;
  const long items = tiles * (K / FW_KCHUNK) * 64;
  hipLaunchKernelGGL(fp8w_dequant_kernel, dim3(ca_grid_for(items)), dim3(256),
                     0, stream, (const uint8_t*)codes,
                     (const int8_t*)scale_exp, (uint16_t*)w_out, N, K, items);
  return hipGetLastError();
}
