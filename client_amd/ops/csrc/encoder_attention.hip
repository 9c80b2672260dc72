// BERT encoder self-attention for gfx950: flash-style MFMA attention of
// every query of a row over the row's own keys, with a per-row key mask,
// on v_mfma_f32_32x32x16_bf16. Included from kernels.hip after
// prefill_attention.hip, whose fragment types and helpers it shares; it is
// gqa_prefill_attention without the KV cache, e4m3, row_map, the causal
// diagonal and the head grouping.
//
// Layouts (all contiguous): qkv [B, S, 3, heads, d] bf16, the packed
// in-projection output viewed in place (q, k and v of a token are read
// where the GEMM wrote them, no head transpose); out [B, S, heads, d] bf16,
// the out-projection's input; key_mask [B, S] uint8, nonzero = the key may
// be attended to; kv_len [B] int32, one plus the index of the row's last
// nonzero mask byte (0: none).
//
// Query c < kv_len[i] of row i attends to the keys j < kv_len[i] with
// key_mask[i, j] != 0, whatever its own mask byte says. Queries
// c >= kv_len[i] are written as exact zeros and a query tile that holds
// only such queries does no work. A query with no visible key yields
// exact zeros.
//
// Grid (query tile, head, row). A workgroup owns EA_QTILE query positions
// of one head: they are the columns of the MFMA tiles, 32 per wave, so
// EA_QTILE / 32 waves compute. Up to d = 64 the block is those two waves
// (128 threads), which also stage; at d = 128 the staging registers of
// two waves would not fit, so the block has 256 threads and the other two
// waves only help staging. Blocks of EA_KSTAGE keys (and their mask bytes) are staged
// once per workgroup in LDS (K as [key][d], V transposed to [d][key]) and
// walked in tiles of EA_KTILE keys, the unit of the online softmax; the
// next block's global loads are in flight while the current one is
// computed. At the BERT-large serving shape (B 8, S 128, 16 heads) the
// grid is 2 x 16 x 8 = 256 workgroups and a row's keys are one block.
//
// Arithmetic and orientation are gqa_prefill_attention's: S^T = K Q^T, a
// lane holds the 16 scores of one query column, m, l and O are fp32, the
// probabilities are rounded RNE to bf16 as the B operand of O^T = V^T P^T
// and l is summed from the unrounded ones.
//
// Keys j >= kv_len are not loaded (zeros and a zero mask byte are staged
// instead), so NaN patterns behind a row's keys never reach an MFMA. A
// masked key gets the score -inf by a select, never by arithmetic.
//
// No atomics, no workspace: the key range is not split. The tiles
// (multiples of EA_KTILE from key 0, up to kv_len) and every reduction
// order depend on the row's kv_len and mask alone, so the output bits of
// (row, c) do not depend on B, the row's index, S or the other rows.

#define EA_QTILE 64    // query positions per workgroup (exported to Python)
#define EA_KTILE 32    // keys per online-softmax tile (exported to Python)
#define EA_KSTAGE 128  // keys staged in LDS per barrier pair: 4 tiles

template <int D, int NTHR>
__global__ void __launch_bounds__(NTHR)
encoder_attention_kernel(const uint16_t* __restrict__ qkv,
                         const uint8_t* __restrict__ key_mask,
                         const int* __restrict__ kv_len,
                         uint16_t* __restrict__ out, int s_len, int heads,
                         float scale) {
  constexpr int KS = D + 8;             // K row stride in LDS (elements)
  constexpr int VS = EA_KSTAGE + 4;     // V^T row stride in LDS
  constexpr int DCH = D / 8;            // 8-element chunks of a key row
  constexpr int CHUNKS = EA_KSTAGE * DCH;
  constexpr int CH = (CHUNKS + NTHR - 1) / NTHR;  // chunks per lane
  constexpr int DT = (D + 31) / 32;     // 32-row tiles of O^T
  constexpr int KSTEPS = D / 16;        // MFMA k-steps of K Q^T
  constexpr int SUB = EA_KSTAGE / EA_KTILE;  // key tiles per staged block
  static_assert(CH >= 1 && EA_KTILE == 32 && EA_KSTAGE % EA_KTILE == 0 &&
                    EA_QTILE % 32 == 0 && EA_QTILE / 32 <= NTHR / 64 &&
                    EA_KSTAGE <= NTHR,
                "tiling");

  __shared__ __attribute__((aligned(16))) uint16_t s_k[EA_KSTAGE * KS];
  __shared__ __attribute__((aligned(16))) uint16_t s_vt[D * VS];
  __shared__ __attribute__((aligned(16))) uint8_t s_m[EA_KSTAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lr = lane & 31;
  const int lh = lane >> 5;
  const int c0 = blockIdx.x * EA_QTILE;
  const int head = blockIdx.y;
  const int row = blockIdx.z;

  int kv_end = kv_len[row];  // keys walked, and real queries, of this row
  if (kv_end > s_len) kv_end = s_len;

  // this lane's column: query c0 + wave * 32 + lr
  const bool computes = wave * 32 < EA_QTILE;
  const int c = c0 + wave * 32 + lr;
  const bool col_in = computes && c < s_len;
  const long tok_stride = 3L * heads * D;  // elements between tokens of qkv
  const long row_base = (long)row * s_len * tok_stride + (long)head * D;
  const long ooff = (((long)row * s_len + c) * heads + head) * D;

  if (kv_end <= c0) {  // no real query in this tile (block-uniform)
    if (col_in) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d0 = 32 * dt + 8 * g + 4 * lh;
          if (d0 < D)
            *reinterpret_cast<uint2*>(out + ooff + d0) = uint2{0u, 0u};
        }
    }
    return;
  }
  const bool valid = col_in && c < kv_end;
  const int nt = (kv_end + EA_KTILE - 1) / EA_KTILE;

  pa_frag_u qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    if (valid)
      qf[ks].u = *reinterpret_cast<const uint4*>(
          qkv + row_base + (long)c * tok_stride + 16 * ks + 8 * lh);
    else
      qf[ks].u = uint4{0u, 0u, 0u, 0u};
  }

  const uint16_t* kbase = qkv + row_base + (long)heads * D;
  const uint16_t* vbase = qkv + row_base + 2L * heads * D;
  const uint8_t* mbase = key_mask + (long)row * s_len;
  uint4 kreg[CH], vreg[CH];
  uint8_t mreg = 0;

  // global -> registers for staged block st; keys at or past kv_end are
  // zeros with a zero mask byte
#define EA_PREFETCH(st)                                                       \
  _Pragma("unroll") for (int n = 0; n < CH; ++n) {                            \
    const int ci = tid + n * NTHR;                                            \
    if (ci < CHUNKS) {                                                        \
      const int j = (st) * EA_KSTAGE + ci / DCH;                              \
      if (j < kv_end) {                                                       \
        const long o_ = (long)j * tok_stride + (ci % DCH) * 8;                \
        kreg[n] = *reinterpret_cast<const uint4*>(kbase + o_);                \
        vreg[n] = *reinterpret_cast<const uint4*>(vbase + o_);                \
      } else {                                                                \
        kreg[n] = uint4{0u, 0u, 0u, 0u};                                      \
        vreg[n] = uint4{0u, 0u, 0u, 0u};                                      \
      }                                                                       \
    }                                                                         \
  }                                                                           \
  if (tid < EA_KSTAGE) {                                                      \
    const int j = (st) * EA_KSTAGE + tid;                                     \
    mreg = (j < kv_end) ? mbase[j] : (uint8_t)0;                              \
  }

  float m = -INFINITY, l = 0.f;
  pa_frag_cd o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;

  const int nst = (nt + SUB - 1) / SUB;
  EA_PREFETCH(0)
  for (int st = 0; st < nst; ++st) {
    __syncthreads();  // the previous block's reads are done
#pragma unroll
    for (int n = 0; n < CH; ++n) {
      const int ci = tid + n * NTHR;
      if (ci < CHUNKS) {
        const int key = ci / DCH;
        const int dc = ci % DCH;
        *reinterpret_cast<uint4*>(&s_k[key * KS + dc * 8]) = kreg[n];
        const uint32_t vu[4] = {vreg[n].x, vreg[n].y, vreg[n].z, vreg[n].w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          s_vt[(dc * 8 + e) * VS + key] =
              (uint16_t)(vu[e / 2] >> (16 * (e % 2)));
      }
    }
    if (tid < EA_KSTAGE) s_m[tid] = mreg;
    __syncthreads();
    if (st + 1 < nst) {
      EA_PREFETCH(st + 1)
    }
    // a wave with no column only stages
    if (!computes) continue;

    for (int sub = 0; sub < SUB; ++sub) {
    const int t = st * SUB + sub;  // key tile: keys 32 t .. 32 t + 31
    if (t >= nt) break;
    const uint16_t* tk = s_k + sub * EA_KTILE * KS;
    const uint16_t* tv = s_vt + sub * EA_KTILE;
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
    // register r of lane (lr, lh) is key (r&3) + 8*(r>>2) + 4*lh of the
    // tile; its four mask bytes per r>>2 are one aligned word
    float tmax = -INFINITY;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t mw = *reinterpret_cast<const uint32_t*>(
          &s_m[sub * EA_KTILE + 8 * g + 4 * lh]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool vis = ((mw >> (8 * e)) & 0xFFu) != 0u;
        const float sc = vis ? s[4 * g + e] * scale : -INFINITY;
        s[4 * g + e] = sc;
        tmax = fmaxf(tmax, sc);
      }
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
#undef EA_PREFETCH

  // register r of o[dt] is head-dim element 32*dt + (r&3) + 8*(r>>2) + 4*lh;
  // l == 0: the query saw no key at all
  if (col_in) {
    const bool live = valid && l > 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 32 * dt + 8 * g + 4 * lh;
        if (d0 < D) {
          uint32_t w[2] = {0u, 0u};
          if (live) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              w[e / 2] |= (uint32_t)__bfloat16_as_ushort(__float2bfloat16(
                              o[dt][4 * g + e] / l))
                          << (16 * (e % 2));
          }
          *reinterpret_cast<uint2*>(out + ooff + d0) = uint2{w[0], w[1]};
        }
      }
  }
}

// qkv [b, s, 3, heads, d] bf16; key_mask [b, s] uint8; kv_len [b] int32;
// out [b, s, heads, d] bf16, all on the device. An unsupported shape or a
// misaligned pointer is an error and nothing is launched.
extern "C" hipError_t ca_encoder_attention(const void* qkv,
                                           const void* key_mask,
                                           const void* kv_len, void* out,
                                           int b, int s, int heads, int d,
                                           float scale, hipStream_t stream) {
  if (!pa_head_dim_ok(d) || b < 0 || s < 0 || heads <= 0)
    return hipErrorInvalidValue;
  if (b > 65535 || heads > 65535) return hipErrorInvalidValue;  // grid y, z
  // 16-byte q/k/v loads, 8-byte out stores, 4-byte kv_len loads
  if ((uintptr_t)qkv % 16 != 0 || (uintptr_t)out % 8 != 0 ||
      (uintptr_t)kv_len % 4 != 0)
    return hipErrorInvalidValue;
  if (b == 0 || s == 0) return hipSuccess;
  const dim3 grid((uint32_t)((s + EA_QTILE - 1) / EA_QTILE), (uint32_t)heads,
                  (uint32_t)b);
#define EA_CASE(D, NTHR)                                                      \
  case D:                                                                     \
    hipLaunchKernelGGL((encoder_attention_kernel<D, NTHR>), grid, dim3(NTHR), \
                       0, stream, (const uint16_t*)qkv,                       \
                       (const uint8_t*)key_mask, (const int*)kv_len,          \
                       (uint16_t*)out, s, heads, scale);                      \
    break
  switch (d) {
    EA_CASE(16, 128);
    EA_CASE(32, 128);
    EA_CASE(64, 128);
    EA_CASE(128, 256);
    default:
      return hipErrorInvalidValue;
  }
#undef EA_CASE
  return hipGetLastError();
}
