// LLM prefill-chunk kernels for gfx950: RoPE + KV-cache scatter for a
// chunk of C tokens per row, and flash-style GQA attention of the chunk's
// queries over the row's cache on v_mfma_f32_32x32x16_bf16. Included from
// kernels.hip (after the decode attention, whose helpers it shares).
//
// Layouts (all contiguous): q/k/v/out [B, C, heads, d] bf16, as the
// projections produce them; caches [rows, hk, cache_len, d] bf16 bits or
// e4m3 codes; pos/row_lens/row_map [B] int64. Token c of batch row i is
// real when c < row_lens[i]; it sits at position p = pos[i] + c of cache
// row row_map[i].
//
// rope_scatter_prefill: one lane per 16 bytes (8 elements, 4 rotation
// pairs) of a q, k or v head vector. q is rotated in place and scaled,
// rotated k and copied v go to the cache (encoded to e4m3 for an fp8
// cache) with rope_rotate_pair and CastF32ToFp8, the decode kernels'
// arithmetic. A token that is not real, whose position is outside
// [0, cache_len) or whose row_map is outside [0, cache_rows) writes
// nothing at all, q included.
//
// gqa_prefill_attention: grid (query tile, kv head, row). A workgroup
// owns PA_QTILE query positions x the rep query heads of one kv head;
// these (query, head) pairs are the columns of the MFMA tiles, 32 per
// wave, in a block of 4 waves (rep <= 4) or 8. Blocks of PA_KSTAGE keys are
// staged once per workgroup in LDS (K as [key][d], V transposed to
// [d][key]; e4m3 is converted to bf16 on the way, exactly) and shared by
// the waves, which walk a block in tiles of PA_KTILE keys, the unit of
// the online softmax; the next block's global loads are in flight while
// the current one is computed.
//
// Orientation: S^T = K Q^T (A = K tile, B = Q^T), so a lane holds the 16
// scores of ONE query column for 16 keys in its accumulator registers:
// the softmax row reduction is 16 registers and one exchange with lane
// ^ 32, and the probabilities, rounded RNE to bf16, are already the B
// operand of O^T = V^T P^T (the sum runs over the accumulator's row
// index), so P never goes through LDS. m, l and O are fp32; l is summed
// from the unrounded probabilities.
//
// Keys j >= the workgroup's last visible key + 1 are not loaded (zeros
// are staged instead), so NaN patterns behind a row's own keys never
// reach an MFMA. Keys a query must not see get the score -inf by a
// select, never by arithmetic.
//
// No atomics, no workspace: the key range is not split. A query's tiles,
// their boundaries (multiples of PA_KTILE from key 0) and every reduction
// order depend on its position alone. A workgroup may walk tiles that are
// wholly invisible to one of its queries; there that query's factor is
// exp(0) = 1 and its probabilities are exact zeros, which change no bit.
// So the output bits of (row, c) do not depend on B, the row's index,
// row_map, max_len or the other rows.

#define PA_QTILE 32   // query positions per workgroup (exported to Python)
#define PA_KTILE 32   // keys per online-softmax tile (exported to Python)
#define PA_KSTAGE 128  // keys staged in LDS per barrier pair: 4 tiles

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 pa_frag_ab;
typedef __attribute__((ext_vector_type(16))) float pa_frag_cd;

union pa_frag_u {
  uint4 u;
  pa_frag_ab f;
};

inline bool pa_head_dim_ok(int d) {
  return d == 16 || d == 32 || d == 64 || d == 128;
}

// 8 stored elements -> 8 bf16 (exact for e4m3)
__device__ __forceinline__ uint4 pa_to_bf16(const uint4& w, const uint16_t*) {
  return w;
}
__device__ __forceinline__ uint4 pa_to_bf16(const uint2& w, const uint8_t*) {
  float f[16];
  ga_unpack(uint4{w.x, w.y, 0u, 0u}, f, (const uint8_t*)nullptr);
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = (__float_as_uint(f[2 * i]) >> 16) |
           (__float_as_uint(f[2 * i + 1]) & 0xFFFF0000u);
  return uint4{o[0], o[1], o[2], o[3]};
}

template <typename T>
struct pa_raw;
template <>
struct pa_raw<uint16_t> {
  typedef uint4 type;
};
template <>
struct pa_raw<uint8_t> {
  typedef uint2 type;
};

__device__ __forceinline__ void pa_zero(uint4& w) { w = uint4{0u, 0u, 0u, 0u}; }
__device__ __forceinline__ void pa_zero(uint2& w) { w = uint2{0u, 0u}; }

}  // namespace

template <bool FP8>
__global__ void __launch_bounds__(256) rope_scatter_prefill_kernel(
    uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ v, void* __restrict__ ck_,
    void* __restrict__ cv_, const float* __restrict__ cos_tab,
    const float* __restrict__ sin_tab, const long* __restrict__ pos,
    const long* __restrict__ row_lens, const long* __restrict__ row_map,
    int b, int c_len, int hq, int hk, int d, long cache_len, long cache_rows,
    float q_scale) {
  const int dch = d / 8;
  const int heads = hq + 2 * hk;
  const int half = d / 2;
  const long total = (long)b * c_len * heads * dch;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    long rem = i;
    const int e8 = (int)(rem % dch);
    rem /= dch;
    const int head = (int)(rem % heads);
    rem /= heads;
    const int c = (int)(rem % c_len);
    const int row = (int)(rem / c_len);
    if (c >= row_lens[row]) continue;
    const long p = pos[row] + c;
    const long rm = row_map[row];
    if (p < 0 || p >= cache_len || rm < 0 || rm >= cache_rows) continue;
    const long tok = (long)row * c_len + c;

    uint16_t in[8], o[8];
    if (head < hq + hk) {
      const float4 cs =
          *reinterpret_cast<const float4*>(cos_tab + p * half + 4 * e8);
      const float4 sn =
          *reinterpret_cast<const float4*>(sin_tab + p * half + 4 * e8);
      const float cc[4] = {cs.x, cs.y, cs.z, cs.w};
      const float ss[4] = {sn.x, sn.y, sn.z, sn.w};
      if (head < hq) {  // q: rotate in place (+ folded scale)
        uint16_t* src = q + (tok * hq + head) * d + 8 * e8;
        *reinterpret_cast<uint4*>(in) = *reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          rope_rotate_pair(in, o, j, cc[j], ss[j], q_scale);
        *reinterpret_cast<uint4*>(src) = *reinterpret_cast<const uint4*>(o);
        continue;
      }
      const uint16_t* src = k + (tok * hk + (head - hq)) * d + 8 * e8;
      *reinterpret_cast<uint4*>(in) = *reinterpret_cast<const uint4*>(src);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        rope_rotate_pair(in, o, j, cc[j], ss[j], 1.0f);
    } else {  // v: copied as it is
      const uint16_t* src = v + (tok * hk + (head - hq - hk)) * d + 8 * e8;
      *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(src);
    }
    const int h = (head < hq + hk) ? head - hq : head - hq - hk;
    void* cache = (head < hq + hk) ? ck_ : cv_;
    const long off = ((rm * hk + h) * cache_len + p) * d + 8 * e8;
    if constexpr (FP8) {
      uint32_t w[2] = {0u, 0u};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        w[j / 4] |= (uint32_t)CastF32ToFp8::convert(bf16_to_f32(o[j]))
                    << (8 * (j % 4));
      *reinterpret_cast<uint2*>((uint8_t*)cache + off) = uint2{w[0], w[1]};
    } else {
      *reinterpret_cast<uint4*>((uint16_t*)cache + off) =
          *reinterpret_cast<const uint4*>(o);
    }
  }
}

namespace {

hipError_t pa_rope_scatter_launch(bool fp8, void* q, const void* k,
                                  const void* v, void* ck, void* cv,
                                  const void* cos_tab, const void* sin_tab,
                                  const void* pos, const void* row_lens,
                                  const void* row_map, int b, int c_len,
                                  int hq, int hk, int d, long cache_len,
                                  long cache_rows, float q_scale,
                                  hipStream_t stream) {
  if (!pa_head_dim_ok(d) || b < 0 || c_len < 0 || hq <= 0 || hk <= 0 ||
      cache_len <= 0 || cache_rows <= 0)
    return hipErrorInvalidValue;
  // 16-byte accesses of q/k/v, the tables and a bf16 cache; 8-byte
  // stores of e4m3 codes
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)cos_tab |
       (uintptr_t)sin_tab) % 16 != 0 ||
      ((uintptr_t)ck | (uintptr_t)cv) % (fp8 ? 8 : 16) != 0)
    return hipErrorInvalidValue;
  const long total = (long)b * c_len * (hq + 2 * hk) * (d / 8);
  if (total == 0) return hipSuccess;
#define PA_RS_LAUNCH(FP8)                                                     \
  hipLaunchKernelGGL((rope_scatter_prefill_kernel<FP8>),                      \
                     dim3(ca_grid_for(total)), dim3(256), 0, stream,          \
                     (uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v,    \
                     ck, cv, (const float*)cos_tab, (const float*)sin_tab,    \
                     (const long*)pos, (const long*)row_lens,                 \
                     (const long*)row_map, b, c_len, hq, hk, d, cache_len,    \
                     cache_rows, q_scale)
  if (fp8) PA_RS_LAUNCH(true);
  else PA_RS_LAUNCH(false);
#undef PA_RS_LAUNCH
  return hipGetLastError();
}

}  // namespace

// q [b, c_len, hq, d] rotated in place; k/v [b, c_len, hk, d]; ck/cv
// [cache_rows, hk, cache_len, d] bf16
extern "C" hipError_t ca_rope_scatter_prefill_bf16(
    void* q, const void* k, const void* v, void* ck, void* cv,
    const void* cos_tab, const void* sin_tab, const void* pos,
    const void* row_lens, const void* row_map, int b, int c_len, int hq,
    int hk, int d, long cache_len, long cache_rows, float q_scale,
    hipStream_t stream) {
  return pa_rope_scatter_launch(false, q, k, v, ck, cv, cos_tab, sin_tab, pos,
                                row_lens, row_map, b, c_len, hq, hk, d,
                                cache_len, cache_rows, q_scale, stream);
}

// the same into an e4m3 cache (one code per element)
extern "C" hipError_t ca_rope_scatter_prefill_fp8kv_bf16(
    void* q, const void* k, const void* v, void* ck, void* cv,
    const void* cos_tab, const void* sin_tab, const void* pos,
    const void* row_lens, const void* row_map, int b, int c_len, int hq,
    int hk, int d, long cache_len, long cache_rows, float q_scale,
    hipStream_t stream) {
  return pa_rope_scatter_launch(true, q, k, v, ck, cv, cos_tab, sin_tab, pos,
                                row_lens, row_map, b, c_len, hq, hk, d,
                                cache_len, cache_rows, q_scale, stream);
}

template <typename T, int D, int NTHR>
__global__ void __launch_bounds__(NTHR)
gqa_prefill_attention_kernel(const uint16_t* __restrict__ q,
                             const T* __restrict__ ck,
                             const T* __restrict__ cv,
                             const long* __restrict__ pos,
                             const long* __restrict__ row_lens,
                             const long* __restrict__ row_map,
                             uint16_t* __restrict__ out, int c_len, int hq,
                             int hk, int rep, float scale, long max_len,
                             long cache_len, long cache_rows) {
  constexpr int KS = D + 8;             // K row stride in LDS (elements)
  constexpr int VS = PA_KSTAGE + 4;     // V^T row stride in LDS
  constexpr int DCH = D / 8;            // 8-element chunks of a key row
  constexpr int CHUNKS = PA_KSTAGE * DCH;
  constexpr int CH = (CHUNKS + NTHR - 1) / NTHR;  // chunks per lane
  constexpr int DT = (D + 31) / 32;     // 32-row tiles of O^T
  constexpr int KSTEPS = D / 16;        // MFMA k-steps of K Q^T
  constexpr int SUB = PA_KSTAGE / PA_KTILE;  // key tiles per staged block
  static_assert(CH >= 1 && PA_KTILE == 32 && PA_KSTAGE % PA_KTILE == 0,
                "tiling");
  typedef typename pa_raw<T>::type raw_t;

  __shared__ __attribute__((aligned(16))) uint16_t s_k[PA_KSTAGE * KS];
  __shared__ __attribute__((aligned(16))) uint16_t s_vt[D * VS];

  const int tid = threadIdx.x;
  constexpr int nthr = NTHR;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int c0 = blockIdx.x * PA_QTILE;
  const int g_kv = blockIdx.y;
  const int row = blockIdx.z;

  const long p0 = pos[row];
  long len = row_lens[row];
  if (len > c_len) len = c_len;
  const long rm = row_map[row];

  // this lane's column: query c0 + qi, head g_kv * rep + hr
  const int col = wave * 32 + lr;
  const int qi = col / rep;
  const int c = c0 + qi;
  const bool col_in = qi < PA_QTILE && c < c_len;
  const long qoff =
      (((long)row * c_len + c) * hq + (long)g_kv * rep + (col - qi * rep)) * D;

  // real queries of this tile (block-uniform)
  long last = (len < (long)c0 + PA_QTILE) ? len : (long)c0 + PA_QTILE;
  const bool row_ok = rm >= 0 && rm < cache_rows && p0 >= 0 && last > c0;
  long kv_end = p0 + last;  // one past the last real query's position
  if (kv_end > max_len) kv_end = max_len;
  if (!row_ok || kv_end <= 0) {
    if (col_in) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d0 = 32 * dt + 8 * g + 4 * lh;
          if (d0 < D)
            *reinterpret_cast<uint2*>(out + qoff + d0) = uint2{0u, 0u};
        }
    }
    return;
  }
  const bool valid = col_in && c < len;
  // last key the column's query sees; -1: none
  long pq = -1;
  if (valid) {
    pq = p0 + c;
    if (pq > max_len - 1) pq = max_len - 1;
  }
  const int nt = (int)((kv_end + PA_KTILE - 1) / PA_KTILE);

  pa_frag_u qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    if (col_in)
      qf[ks].u =
          *reinterpret_cast<const uint4*>(q + qoff + 16 * ks + 8 * lh);
    else
      qf[ks].u = uint4{0u, 0u, 0u, 0u};
  }

  const long kv_base = ((rm * hk + g_kv) * cache_len) * D;
  const T* kbase = ck + kv_base;
  const T* vbase = cv + kv_base;
  raw_t kreg[CH], vreg[CH];

  // global -> registers for staged block st; keys at or past kv_end are
  // zeros
#define PA_PREFETCH(st)                                                       \
  _Pragma("unroll") for (int n = 0; n < CH; ++n) {                            \
    const int ci = tid + n * nthr;                                            \
    if (ci < CHUNKS) {                                                        \
      const long j = (long)(st) * PA_KSTAGE + ci / DCH;                       \
      if (j < kv_end) {                                                       \
        const long o_ = j * D + (ci % DCH) * 8;                               \
        kreg[n] = *reinterpret_cast<const raw_t*>(kbase + o_);                \
        vreg[n] = *reinterpret_cast<const raw_t*>(vbase + o_);                \
      } else {                                                                \
        pa_zero(kreg[n]);                                                     \
        pa_zero(vreg[n]);                                                     \
      }                                                                       \
    }                                                                         \
  }

  float m = -INFINITY, l = 0.f;
  pa_frag_cd o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  const int nst = (nt + SUB - 1) / SUB;
  PA_PREFETCH(0)
  for (int st = 0; st < nst; ++st) {
    __syncthreads();  // the previous block's reads are done
#pragma unroll
    for (int n = 0; n < CH; ++n) {
      const int ci = tid + n * nthr;
      if (ci < CHUNKS) {
        const int key = ci / DCH;
        const int dc = ci % DCH;
        *reinterpret_cast<uint4*>(&s_k[key * KS + dc * 8]) =
            pa_to_bf16(kreg[n], (const T*)nullptr);
        const uint4 vw = pa_to_bf16(vreg[n], (const T*)nullptr);
        const uint32_t vu[4] = {vw.x, vw.y, vw.z, vw.w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          s_vt[(dc * 8 + e) * VS + key] =
              (uint16_t)(vu[e / 2] >> (16 * (e % 2)));
      }
    }
    __syncthreads();
    if (st + 1 < nst) {
      PA_PREFETCH(st + 1)
    }
    // a wave with no column (small rep) only stages
    if (wave * 32 >= PA_QTILE * rep) continue;

    for (int sub = 0; sub < SUB; ++sub) {
    const int t = st * SUB + sub;  // key tile: keys 32 t .. 32 t + 31
    if (t >= nt) break;
    const uint16_t* tk = s_k + sub * PA_KTILE * KS;
    const uint16_t* tv = s_vt + sub * PA_KTILE;
    // S^T tile: 32 keys x 32 columns
    pa_frag_cd s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      pa_frag_u a;
      a.u = *reinterpret_cast<const uint4*>(&tk[lr * KS + 16 * ks + 8 * lh]);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.f, qf[ks].f, s, 0, 0, 0);
    }
    // register r of lane (lr, lh) is key (r&3) + 8*(r>>2) + 4*lh of the tile
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long j = (long)t * PA_KTILE + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float sc = (j <= pq) ? s[r] * scale : -INFINITY;
      s[r] = sc;
      tmax = fmaxf(tmax, sc);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m, tmax);
    // a column with no visible key so far keeps m = -inf; exp(-inf - 0)
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __expf(m - m_use);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __expf(s[r] - m_use);
      s[r] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 32);
    l = l * alpha + psum;
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

    // O^T += V^T P^T: registers 8*ks .. 8*ks+7, rounded to bf16, are the B
    // fragment of k-step ks; its element j is key 16*ks + 8*(j>>2) + 4*lh
    // + (j&3), so the A fragment takes V^T from those same keys
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      pa_frag_u pb;
      uint32_t w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        w[i] = (uint32_t)f32_to_bf16_rne(s[8 * ks + 2 * i]) |
               ((uint32_t)f32_to_bf16_rne(s[8 * ks + 2 * i + 1]) << 16);
      pb.u = uint4{w[0], w[1], w[2], w[3]};
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        pa_frag_u a;
        const int dr = 32 * dt + lr;
        if (D >= 32 || dr < D) {
          const uint16_t* vp = &tv[dr * VS + 16 * ks + 4 * lh];
          const uint2 lo = *reinterpret_cast<const uint2*>(vp);
          const uint2 hi = *reinterpret_cast<const uint2*>(vp + 8);
          a.u = uint4{lo.x, lo.y, hi.x, hi.y};
        } else {
          a.u = uint4{0u, 0u, 0u, 0u};  // head dim padded to 32 rows
        }
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.f, pb.f, o[dt], 0,
                                                        0, 0);
      }
    }
    }  // sub
  }
#undef PA_PREFETCH

  // register r of o[dt] is head-dim element 32*dt + (r&3) + 8*(r>>2) + 4*lh
  if (col_in) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 32 * dt + 8 * g + 4 * lh;
        if (d0 < D) {
          uint32_t w[2] = {0u, 0u};
          if (valid) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              w[e / 2] |= (uint32_t)__bfloat16_as_ushort(__float2bfloat16(
                              o[dt][4 * g + e] / l))
                          << (16 * (e % 2));
          }
          *reinterpret_cast<uint2*>(out + qoff + d0) = uint2{w[0], w[1]};
        }
      }
  }
}

namespace {

template <typename T, int D>
hipError_t pa_attn_launch(const void* q, const void* ck, const void* cv,
                          const void* pos, const void* row_lens,
                          const void* row_map, void* out, int b, int c_len,
                          int hq, int hk, float scale, long max_len,
                          long cache_len, long cache_rows,
                          hipStream_t stream) {
  const int rep = hq / hk;
  const dim3 grid((uint32_t)((c_len + PA_QTILE - 1) / PA_QTILE), (uint32_t)hk,
                  (uint32_t)b);
  // PA_QTILE * rep columns, 32 per wave: four waves up to rep 4 (those
  // without a column help staging), eight above
#define PA_LAUNCH(NTHR)                                                       \
  hipLaunchKernelGGL((gqa_prefill_attention_kernel<T, D, NTHR>), grid,        \
                     dim3(NTHR), 0, stream, (const uint16_t*)q, (const T*)ck, \
                     (const T*)cv, (const long*)pos, (const long*)row_lens,   \
                     (const long*)row_map, (uint16_t*)out, c_len, hq, hk,     \
                     rep, scale, max_len, cache_len, cache_rows)
  static_assert(PA_QTILE * 8 <= 32 * (512 / 64), "columns of rep 8");
  if (PA_QTILE * rep <= 32 * (256 / 64)) PA_LAUNCH(256);
  else PA_LAUNCH(512);
#undef PA_LAUNCH
  return hipGetLastError();
}

template <typename T>
hipError_t pa_attn_launch_d(int d, const void* q, const void* ck,
                            const void* cv, const void* pos,
                            const void* row_lens, const void* row_map,
                            void* out, int b, int c_len, int hq, int hk,
                            float scale, long max_len, long cache_len,
                            long cache_rows, hipStream_t stream) {
#define PA_CASE(D)                                                            \
  case D:                                                                     \
    return pa_attn_launch<T, D>(q, ck, cv, pos, row_lens, row_map, out, b,    \
                                c_len, hq, hk, scale, max_len, cache_len,     \
                                cache_rows, stream)
  switch (d) {
    PA_CASE(16);
    PA_CASE(32);
    PA_CASE(64);
    PA_CASE(128);
    default:
      return hipErrorInvalidValue;
  }
#undef PA_CASE
}

}  // namespace

// bytes of workspace ca_gqa_prefill_attention needs: none, the key range
// is not split over workgroups
extern "C" long ca_gqa_prefill_attention_workspace_bytes(int b, int c_len,
                                                         int hq, int d,
                                                         long max_len) {
  (void)b; (void)c_len; (void)hq; (void)d; (void)max_len;
  return 0;
}

// q/out [b, c_len, hq, d] bf16; ck/cv [cache_rows, hk, cache_len, d] bf16
// bits, or e4m3 codes with kv_fp8; pos/row_lens/row_map [b] int64 on the
// device. ws/ws_bytes are accepted for a later split-key variant.
extern "C" hipError_t ca_gqa_prefill_attention(
    const void* q, const void* ck, const void* cv, const void* pos,
    const void* row_lens, const void* row_map, void* out, void* ws,
    long ws_bytes, int b, int c_len, int hq, int hk, int d, float scale,
    long max_len, long cache_len, long cache_rows, int kv_fp8,
    hipStream_t stream) {
  (void)ws;
  if (b < 0 || c_len < 0 || !ga_shape_ok(hq, hk, d))
    return hipErrorInvalidValue;
  if (max_len <= 0 || max_len > cache_len || cache_rows <= 0)
    return hipErrorInvalidValue;
  if (b > 65535 || hk > 65535) return hipErrorInvalidValue;  // grid y, z
  if (ws_bytes <
      ca_gqa_prefill_attention_workspace_bytes(b, c_len, hq, d, max_len))
    return hipErrorInvalidValue;
  // 16-byte q loads, 8- or 16-byte K/V chunk loads, 8-byte out stores
  if (((uintptr_t)q | (uintptr_t)out) % 16 != 0 ||
      ((uintptr_t)ck | (uintptr_t)cv) % (kv_fp8 ? 8 : 16) != 0)
    return hipErrorInvalidValue;
  if (b == 0 || c_len == 0) return hipSuccess;
  if (kv_fp8)
    return pa_attn_launch_d<uint8_t>(d, q, ck, cv, pos, row_lens, row_map,
                                     out, b, c_len, hq, hk, scale, max_len,
                                     cache_len, cache_rows, stream);
  return pa_attn_launch_d<uint16_t>(d, q, ck, cv, pos, row_lens, row_map, out,
                                    b, c_len, hq, hk, scale, max_len,
                                    cache_len, cache_rows, stream);
}
