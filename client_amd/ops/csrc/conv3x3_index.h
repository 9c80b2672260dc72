// Tile geometry and tile -> address arithmetic of the fused 3x3 conv
// kernel (conv3x3.hip). Plain C++ so a host program can enumerate every
// global and LDS offset the kernel forms (tests/test_conv3x3_index.py).
//
// Geometry. The conv is 3x3, pad 1, stride 1 or 2, NCHW. Output rows
// are numbered across the batch: go = n*OH + oh. A tile is R whole
// consecutive output rows (possibly spanning images) laid out as
// columns j = jr*OW + ow of a BN-wide MFMA tile; columns past R*OW, or
// past the last image, are computed on in-bounds LDS data and dropped.
//
// The input footprint of a tile is staged per channel chunk in LDS in a
// padded row space: every image has PH = H+2 padded rows (row 0 and row
// H+1 are the zero halo) of PW = W+2 pixels, numbered across the batch
// as P = n*PH + (ih+1). Output row (n, oh) reads padded rows
// n*PH + oh*stride + r, r = 0..2, so a run of output rows reads one
// contiguous range of padded rows, halo rows between images included,
// and tap (r, s) of a column is its base pixel + r*PW + s.
#pragma once

#ifndef CA_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CA_HD __host__ __device__
#else
#define CA_HD
#endif
#endif

enum {
  C3_BM = 64,         // output channels per workgroup
  C3_CK = 32,         // input channels per LDS chunk
  C3_THREADS = 256,   // 4 waves as 2 (channels) x 2 (columns)
  C3_MAXIT = 6,       // staging items (pixel x 8 channels) per thread
  C3_PIX_BYTES = 80,  // LDS bytes per staged pixel: 32 bf16 + 16 B pad
  C3_A_BYTES = 9 * C3_CK * C3_BM * 2,  // weight chunk in LDS
  C3_LDS_MAX = 64 * 1024,
};

struct Conv3x3Geom {
  int N, C, K, H, W, stride;
  int OH, OW;  // output extent
  int PH, PW;  // padded input extent
  int NT;      // 32-column MFMA tiles per wave (BN = 64 * NT)
  int R;       // output rows per tile
  int tiles;   // ceil(N*OH / R)
  int fp_max;  // largest staged footprint of any tile, in pixels
};

// first and last (inclusive) batch-wide output row of a tile
CA_HD inline int c3_tile_go0(const Conv3x3Geom& g, int tile) {
  return tile * g.R;
}
CA_HD inline int c3_tile_go1(const Conv3x3Geom& g, int tile) {
  int go1 = tile * g.R + g.R;
  const int rows = g.N * g.OH;
  return (go1 < rows ? go1 : rows) - 1;
}

// padded input row read by tap row r of batch-wide output row go
CA_HD inline int c3_prow(const Conv3x3Geom& g, int go, int r) {
  const int n = go / g.OH;
  const int oh = go - n * g.OH;
  return n * g.PH + oh * g.stride + r;
}

// staged footprint of a tile: first padded row and pixel count
CA_HD inline int c3_tile_p0(const Conv3x3Geom& g, int tile) {
  return c3_prow(g, c3_tile_go0(g, tile), 0);
}
CA_HD inline int c3_tile_fp(const Conv3x3Geom& g, int tile) {
  return (c3_prow(g, c3_tile_go1(g, tile), 2) - c3_tile_p0(g, tile) + 1) *
         g.PW;
}

// Footprint pixel pi of a tile whose first padded row is p0 -> element
// offset of that pixel in channel 0 of x (add c*H*W), or -1 for a halo
// pixel, which is staged as zero and never addressed in global memory.
CA_HD inline long c3_stage_src(const Conv3x3Geom& g, int p0, int pi) {
  const int fr = pi / g.PW;
  const int iw = pi - fr * g.PW - 1;
  const int p = p0 + fr;
  const int n = p / g.PH;
  const int ih = p - n * g.PH - 1;
  if (n >= g.N || ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) return -1;
  return ((long)n * g.C * g.H + ih) * g.W + iw;
}

// Column j of a tile -> LDS pixel of its tap (0,0) and element offset of
// its output in channel 0 of out (add k*OH*OW). Returns false for a
// padding column: lds_pix is then 0 (its nine taps stay inside the
// first three staged rows) and nothing is stored.
CA_HD inline bool c3_column(const Conv3x3Geom& g, int tile, int j,
                            int* lds_pix, long* out_off) {
  const int jr = j / g.OW;
  const int ow = j - jr * g.OW;
  const int go = c3_tile_go0(g, tile) + jr;
  *lds_pix = 0;
  *out_off = 0;
  if (jr >= g.R || go >= g.N * g.OH) return false;
  const int n = go / g.OH;
  const int oh = go - n * g.OH;
  *lds_pix = (c3_prow(g, go, 0) - c3_tile_p0(g, tile)) * g.PW + ow * g.stride;
  *out_off = ((long)n * g.K * g.OH + oh) * g.OW + ow;
  return true;
}

// LDS pixel offset of tap (r, s) relative to a column's lds_pix
CA_HD inline int c3_tap_pix(const Conv3x3Geom& g, int r, int s) {
  return r * g.PW + s;
}

inline int c3_fp_max(const Conv3x3Geom& g) {
  int m = 0;
  for (int t = 0; t < g.tiles; ++t) {
    const int fp = c3_tile_fp(g, t);
    if (fp > m) m = fp;
  }
  return m;
}

inline bool c3_try(Conv3x3Geom* g, int nt, int r) {
  g->NT = nt;
  g->R = r;
  g->tiles = (g->N * g->OH + r - 1) / r;
  g->fp_max = c3_fp_max(*g);
  return g->fp_max * 4 <= C3_MAXIT * C3_THREADS &&
         C3_A_BYTES + g->fp_max * C3_PIX_BYTES <= C3_LDS_MAX;
}

// Chooses the tiling for a shape; false when the kernel does not
// support it. 128-column tiles when they fill at least 3/4 of their
// columns and still give two workgroups per CU, otherwise 64-column
// tiles. The choice affects speed only: an output element's summation
// order does not depend on it.
inline bool c3_plan(Conv3x3Geom* g, int N, int C, int K, int H, int W,
                    int stride) {
  if (N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return false;
  if (C < C3_CK || C % C3_CK || K < C3_BM || K % C3_BM) return false;
  if ((long)N * (C > K ? C : K) * H * W >= (1L << 31)) return false;
  g->N = N, g->C = C, g->K = K, g->H = H, g->W = W, g->stride = stride;
  g->OH = (H - 1) / stride + 1;
  g->OW = (W - 1) / stride + 1;
  g->PH = H + 2;
  g->PW = W + 2;
  if (g->OW > 64) return false;
  for (int nt = 2; nt >= 1; --nt) {
    const int bn = 64 * nt;
    int r = bn / g->OW;
    if (r > g->N * g->OH) r = g->N * g->OH;
    while (r >= 1 && !c3_try(g, nt, r)) --r;
    if (r < 1) continue;
    if (nt == 1) return true;
    const long blocks = (long)g->tiles * (K / C3_BM);
    if (4 * r * g->OW >= 3 * bn && blocks >= 512) return true;
  }
  return false;
}
