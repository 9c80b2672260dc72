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
// ca_fp8w_gemm_bf16: the same y for any M >= 1 (prefill chunks, decode
// batches above 16 rows), a design of its own. A workgroup of 2 x 2 waves
// owns a BM x BN tile of y with the whole K, BM = BN = 128, 64 or 32
// chosen on the host from (M, N) alone (fg_tile_for); a wave owns a
// quarter as WT x WT MFMA tiles (WT = 4, 2, 1). There is no K split: every
// accumulator sees the 64-wide chunks in ascending order, both MFMA steps
// of a chunk in order, and every variant runs the same MFMA shape. So a
// row's output bits depend only on that row of x, on (N, K) and on the
// weights: not on M, on the other rows or on the tile variant. They are
// not the decode kernel's bits, which sums in another order.
// Codes go global -> VGPR, one 16-byte lane load per 16-row tile and
// chunk, no LDS, converted once per chunk and used against the wave's WT
// column tiles. The BM x 64 chunk of x is staged through LDS, double
// buffered, and read back as B fragments by the two waves that share the
// rows. LDS rows are padded from 128 to 144 bytes: the 16 rows of a
// fragment read then start 36 dwords apart and cover all 64 banks once
// (unpadded they would start on the same bank). The loads of chunk c + 1
// (codes to registers, x to registers on its way to the other buffer) are
// issued unconditionally before chunk c is converted and multiplied; the
// last chunk is a separate tail. One barrier per chunk. The epilogue
// scales by 2^scale_exp[n], rounds RNE and stores straight from the D
// fragment, whose lane holds four consecutive n of one row of y: 8-byte
// stores (2-byte ones where N % 4 != 0), 32 WT contiguous bytes per row
// and wave. A pass through LDS for 16-byte stores was not tried.
// -Rpass-analysis=kernel-resource-usage, gfx950, tile 128 / 64 / 32:
// 124 / 59 / 44 VGPRs + 96 / 24 / 4 AGPRs, LDS 36864 / 18432 / 9216 bytes,
// scratch 0 / 0 / 0, occupancy 2 / 5 / 8 waves per SIMD.
//
// ca_fp8w_dequant_bf16: packed codes -> the bf16 bits of W_eff, row-major
// [N, K]; for the dequant route, which runs the library GEMM on it.

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

// ---------------------------------------------------------------------------
// wide GEMM (M > 16: prefill chunks, wide decode batches)
// ---------------------------------------------------------------------------

#define FG_THREADS 256  // 2 x 2 waves
#define FG_ROW_U4 9     // an LDS row of x: 8 x 16 B of data and 16 B of pad
#define FG_MIN_BLOCKS 192

namespace {

// The format-specific part of the wide kernel: one 16-byte lane load per
// 16-row tile and chunk, and the A fragment of MFMA step s from it.
__device__ __forceinline__ fw_u32x4 fg_load_codes(const fw_u32x4* p) {
  return *p;
}

__device__ __forceinline__ fw_frag_ab fg_codes_to_frag(const fw_u32x4& w,
                                                       int s) {
  return s == 0 ? fw_codes8_to_frag(w.x, w.y) : fw_codes8_to_frag(w.z, w.w);
}

// One 64-wide chunk for a wave's WT x WT MFMA tiles: per step WT B
// fragments from LDS (sx points at the wave's row r, 16-byte piece 2 q),
// WT A fragments converted once and used against all of them.
template <int WT>
__device__ __forceinline__ void fg_chunk(const fw_u32x4* sx,
                                         const fw_u32x4 (&w)[WT],
                                         fw_frag_cd (&acc)[WT][WT]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    fw_frag_u b[WT];
#pragma unroll
    for (int i = 0; i < WT; ++i) b[i].u = sx[16 * i * FG_ROW_U4 + s];
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const fw_frag_ab a = fg_codes_to_frag(w[j], s);
#pragma unroll
      for (int i = 0; i < WT; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[i].f,
                                                            acc[i][j], 0, 0, 0);
    }
  }
}

}  // namespace

// A workgroup owns the (32 WT) x (32 WT) tile (mb, nb) of y with the whole
// K; wave (wave >> 1, wave & 1) owns its (16 WT) x (16 WT) quarter as
// WT x WT MFMA tiles, weights as A (rows n), x as B (columns m).
template <int WT>
__global__ void __launch_bounds__(FG_THREADS)
fp8w_gemm_kernel(const uint16_t* __restrict__ x,
                 const uint8_t* __restrict__ packed,
                 const int8_t* __restrict__ scale_exp,
                 uint16_t* __restrict__ y, int M, int N, int K, int mblocks) {
  constexpr int BT = 32 * WT;
  __shared__ fw_u32x4 s_x[2][BT * FG_ROW_U4];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 15;
  const int q = lane >> 4;
  // the row blocks of one column block are neighbours in launch order:
  // they read the same codes
  const int m0 = (int)(blockIdx.x % mblocks) * BT;
  const int n0 = (int)(blockIdx.x / mblocks) * BT;
  const int wm0 = (wave >> 1) * 16 * WT;
  const int wn0 = (wave & 1) * 16 * WT;
  const int kc = K / FW_KCHUNK;
  const int tiles = (N + FW_ROWS - 1) / FW_ROWS;

  // staging of x: the BT x 128 B chunk is BT x 8 pieces of 16 B, WT per
  // thread, 8 consecutive threads one row. Rows >= M repeat row M - 1:
  // they feed only outputs nobody writes, and x is never read beyond its
  // last row.
  const fw_u32x4* xg[WT];
  int xs[WT];
#pragma unroll
  for (int i = 0; i < WT; ++i) {
    const int p = tid + FG_THREADS * i;
    const int row = p >> 3;
    const int gm = m0 + row < M ? m0 + row : M - 1;
    xg[i] = reinterpret_cast<const fw_u32x4*>(x + (long)gm * K) + (p & 7);
    xs[i] = row * FG_ROW_U4 + (p & 7);
  }
  // codes: 16-row tiles beyond the padded N repeat the last one, for the
  // same reason
  const fw_u32x4* wg[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    int t = (n0 + wn0) / FW_ROWS + j;
    t = t < tiles ? t : tiles - 1;
    wg[j] = reinterpret_cast<const fw_u32x4*>(packed) + (long)t * kc * 64 +
            lane;
  }

  fw_frag_cd acc[WT][WT];
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[i][j] = fw_frag_cd{0.f, 0.f, 0.f, 0.f};

  fw_u32x4 w[WT], xr[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) w[j] = fg_load_codes(wg[j]);
#pragma unroll
  for (int i = 0; i < WT; ++i) xr[i] = xg[i][0];
#pragma unroll
  for (int i = 0; i < WT; ++i) s_x[0][xs[i]] = xr[i];
  __syncthreads();

  // lane (m = r, q) reads x[m][64 c + 16 q + 8 s ...] at step s, the k of
  // the weight lane (r, q)'s bytes 8 s ...
  const int sx0 = (wm0 + r) * FG_ROW_U4 + 2 * q;
  // steady state: the loads of chunk c + 1 (codes to registers, x to
  // registers on its way to the other LDS buffer) are issued, without a
  // condition, before chunk c is converted and multiplied. One barrier
  // per chunk: the buffer written here was last read before the previous
  // barrier.
  int c = 0;
  for (; c + 1 < kc; ++c) {
    fw_u32x4 wn[WT];
#pragma unroll
    for (int j = 0; j < WT; ++j)
      wn[j] = fg_load_codes(wg[j] + (long)(c + 1) * 64);
#pragma unroll
    for (int i = 0; i < WT; ++i) xr[i] = xg[i][(long)(c + 1) * 8];
    __builtin_amdgcn_sched_barrier(0);
    fg_chunk<WT>(&s_x[c & 1][sx0], w, acc);
#pragma unroll
    for (int i = 0; i < WT; ++i) s_x[(c + 1) & 1][xs[i]] = xr[i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WT; ++j) w[j] = wn[j];
  }
  // tail: the last chunk, nothing left to load
  fg_chunk<WT>(&s_x[c & 1][sx0], w, acc);

  // D[n = 4 q + e][m = r] in acc[i][j][e]: a lane holds four consecutive n
  // of one row of y, the four q of a row 32 contiguous bytes, the WT
  // tiles of a wave 32 WT. 8-byte stores where y's rows allow them.
  const bool vec = (N & 3) == 0 && ((uintptr_t)y & 7) == 0;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    const int n = n0 + wn0 + 16 * j + 4 * q;
    float sc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      sc[e] = fw_exp2i(scale_exp[n + e < N ? n + e : N - 1]);
#pragma unroll
    for (int i = 0; i < WT; ++i) {
      const int m = m0 + wm0 + 16 * i + r;
      if (m >= M) continue;
      uint16_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = __bfloat16_as_ushort(__float2bfloat16(acc[i][j][e] * sc[e]));
      uint16_t* dst = y + (long)m * N + n;
      if (vec && n + 3 < N) {
        *reinterpret_cast<uint2*>(dst) =
            uint2{(uint32_t)o[0] | ((uint32_t)o[1] << 16),
                  (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < N) dst[e] = o[e];
      }
    }
  }
}

namespace {

// Tile edge of the wide GEMM (BM = BN = 128, 64 or 32), from (M, N)
// alone: the largest whose grid has at least FG_MIN_BLOCKS workgroups,
// about one per CU of the 256; 32 where none has. Larger tiles re-read x
// and the codes less often (each N / BN and M / BM times), smaller ones
// fill the CUs; every variant runs the same MFMAs in the same k order.
inline long fg_blocks(int M, int N, int t) {
  return (((long)M + t - 1) / t) * (((long)N + t - 1) / t);
}

inline int fg_tile_for(int M, int N) {
  for (int t = 128; t > 32; t /= 2)
    if (fg_blocks(M, N, t) >= FG_MIN_BLOCKS) return t;
  return 32;
}

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

// The tile edge ca_fp8w_gemm_bf16 uses for (M, N); 0 outside its contract.
extern "C" int ca_fp8w_gemm_tile(int M, int N) {
  return M < 1 || N < 1 ? 0 : fg_tile_for(M, N);
}

// The decode GEMM's semantics without its limit on M: x [M, K] bf16,
// packed codes of W[N, K], scale_exp [N] int8, y [M, N] bf16. M >= 1,
// N >= 1, K % 64 == 0; x and packed 16-byte aligned, y 2-byte aligned.
// Anything else returns hipErrorInvalidValue before any launch. No
// workspace, no atomics.
extern "C" hipError_t ca_fp8w_gemm_bf16(const void* x, const void* codes,
                                        const void* scale_exp, void* y, int M,
                                        int N, int K, hipStream_t stream) {
  if (M < 1 || N < 1 || K < FW_KCHUNK || K % FW_KCHUNK != 0)
    return hipErrorInvalidValue;
  if (!x || !codes || !scale_exp || !y) return hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)codes) % 16 != 0 || (uintptr_t)y % 2 != 0)
    return hipErrorInvalidValue;
  const int tile = fg_tile_for(M, N);
  const long blocks = fg_blocks(M, N, tile);
  if (blocks > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const int mblocks = (int)(((long)M + tile - 1) / tile);
#define FG_LAUNCH(WT)                                                       \
  hipLaunchKernelGGL((fp8w_gemm_kernel<WT>), dim3((uint32_t)blocks),         \
                     dim3(FG_THREADS), 0, stream, (const uint16_t*)x,       \
                     (const uint8_t*)codes, (const int8_t*)scale_exp,       \
                     (uint16_t*)y, M, N, K, mblocks)
  switch (tile) {
    case 128: FG_LAUNCH(4); break;
    case 64: FG_LAUNCH(2); break;
    default: FG_LAUNCH(1); break;
  }
#undef FG_LAUNCH
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
