// Tile geometry and tile -> address arithmetic of the two DenseNet dense-
// layer kernels (dense_layer.hip). Plain C++, like conv1x1_index.h, whose
// helpers kernel A reuses wherever the address does not depend on the
// input's image stride.
#pragma once

#include "conv1x1_index.h"

// ---------------------------------------------------------------------------
// Kernel A: BN+ReLU prologue, 1x1 conv, bias (+ReLU). The input is the
// channel prefix [0, C) of a block buffer: image n starts at element n*xs,
// xs >= C*HW. Everything else (columns j = n*HW + p, tiles, staging items,
// LDS offsets, the dense [N,K,H,W] output) is conv1x1_index.h's.
// ---------------------------------------------------------------------------

enum { DL_LDS_MAX = 64 * 1024 };

struct DenseConv1x1Geom {
  Conv1x1Geom c;  // shape and tiling; c.C is the number of channels read
  long xs;        // image stride of x, in elements
};

// Column j -> element offset of its pixel in channel 0 of x (add c*HW),
// or -1 for a column past the last image: never addressed in global
// memory.
C1_HD inline long dl_col_src(const DenseConv1x1Geom& g, int j) {
  if (j >= g.c.J) return -1;
  const int n = j / g.c.HW;
  return (long)n * g.xs + (j - n * g.c.HW);
}

// LDS: scale[C] then shift[C] (fp32, staged once), then the two staging
// buffers of conv1x1_index.h, which the exchange region reuses
C1_HD inline int dl_ss_bytes(int C) { return 2 * C * 4; }
C1_HD inline int dl_a_lds_bytes(const DenseConv1x1Geom& g) {
  return dl_ss_bytes(g.c.C) + c1_lds_bytes(g.c.NT);
}

// c1_plan's tiling. Dword loads (two pixels of a channel) need every
// image to start at an even element: with an odd xs the plan takes the
// 2-byte loads, and with them the 2-byte stores. An output element's
// summation order depends on none of this.
inline bool dl_plan_a(DenseConv1x1Geom* g, int N, int C, int K, int H, int W,
                      long xs) {
  if (!c1_plan(&g->c, N, C, K, H, W)) return false;
  if (xs < (long)C * H * W || (long)N * xs >= (1L << 31)) return false;
  g->xs = xs;
  if (xs % 2) g->c.VL = 1, g->c.VS = 0;
  return dl_a_lds_bytes(*g) <= DL_LDS_MAX;
}

// ---------------------------------------------------------------------------
// Kernel B: 3x3 conv, pad 1, stride 1, dense [N,C,H,W] in, exactly 32
// output channels stored at channel k0 of a buffer with image stride os.
//
// Output rows are numbered across the batch, go = n*H + oh. A tile is R
// whole consecutive output rows (possibly spanning images) laid out as
// columns j = jr*W + ow of a 32*NT-wide MFMA tile. The four waves of a
// workgroup split the reduction, not the tile: wave v takes the
// 32-channel chunks v, v+4, ... and stages its chunk's footprint in an LDS
// region of its own, in the padded row space of conv3x3_index.h: image n
// has PH = H+2 padded rows (row 0 and row H+1 are the zero halo) of
// PW = W+2 pixels, numbered P = n*PH + ih + 1, so tap (r, s) of a column
// is its base pixel + r*PW + s.
// ---------------------------------------------------------------------------

enum {
  DL3_K = 32,          // output channels
  DL3_CK = 32,         // input channels per chunk (one wave's share)
  DL3_THREADS = 256,   // 4 waves, one chunk each per round
  DL3_PIX_BYTES = 80,  // LDS bytes per staged pixel: 32 bf16 + 16 B pad
  DL3_WG_TARGET = 256  // workgroups wanted before tiles grow past a row
};

struct DenseConv3x3Geom {
  int N, C, H, W;
  int HW, PH, PW;
  int k0;      // first output channel in the buffer
  long os;     // image stride of the output buffer, in elements
  int NT;      // 32-column MFMA tiles per wave (1 or 2)
  int R;       // output rows per tile
  int tiles;   // ceil(N*H / R)
  int fp_max;  // largest staged footprint of any tile, in pixels
};

// first padded row a batch-wide output row reads (its tap row 0)
C1_HD inline int dl3_prow(const DenseConv3x3Geom& g, int go) {
  const int n = go / g.H;
  return n * g.PH + (go - n * g.H);
}

// staged footprint of a tile: first padded row and pixel count
C1_HD inline int dl3_tile_p0(const DenseConv3x3Geom& g, int tile) {
  return dl3_prow(g, tile * g.R);
}
C1_HD inline int dl3_tile_fp(const DenseConv3x3Geom& g, int tile) {
  int go1 = tile * g.R + g.R;
  if (go1 > g.N * g.H) go1 = g.N * g.H;
  return (dl3_prow(g, go1 - 1) + 2 - dl3_tile_p0(g, tile) + 1) * g.PW;
}

// Footprint pixel pi of a tile whose first padded row is p0 -> element
// offset of that pixel in channel 0 of x (add c*HW), or -1 for a halo
// pixel: staged as zero, never addressed in global memory.
C1_HD inline long dl3_stage_src(const DenseConv3x3Geom& g, int p0, int pi) {
  const int fr = pi / g.PW;
  const int iw = pi - fr * g.PW - 1;
  const int p = p0 + fr;
  const int n = p / g.PH;
  const int ih = p - n * g.PH - 1;
  if (n >= g.N || ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) return -1;
  return ((long)n * g.C * g.H + ih) * g.W + iw;
}

// Column j of a tile -> LDS pixel of its tap (0,0) and element offset of
// its output channel k0 in the buffer (add k*HW). False for a padding
// column: lds_pix is then 0 (its nine taps stay inside the first three
// staged rows) and nothing is stored.
C1_HD inline bool dl3_column(const DenseConv3x3Geom& g, int tile, int j,
                             int* lds_pix, long* out_off) {
  const int jr = j / g.W;
  const int ow = j - jr * g.W;
  const int go = tile * g.R + jr;
  *lds_pix = 0;
  *out_off = 0;
  if (jr >= g.R || go >= g.N * g.H) return false;
  const int n = go / g.H;
  const int oh = go - n * g.H;
  *lds_pix = (dl3_prow(g, go) - dl3_tile_p0(g, tile)) * g.PW + ow;
  *out_off = (long)n * g.os + ((long)g.k0 * g.H + oh) * g.W + ow;
  return true;
}

// element offset in the packed weights [3][3][C/16][32][16] of the A
// fragment (8 input channels 8*half.., 16-channel step c16) of output
// channel `row` at tap: one wave's 64 lanes read 1 KB contiguous
C1_HD inline long dl3_w_off(const DenseConv3x3Geom& g, int tap, int c16,
                            int row, int half) {
  return (((long)tap * (g.C / 16) + c16) * DL3_K + row) * 16 + half * 8;
}

// LDS: four footprint regions while the waves accumulate, then the four
// partial tiles as fp32 [wave][tile][register][lane]
C1_HD inline int dl3_red_off(int nt, int wave, int t, int r, int lane) {
  return (((wave * nt + t) * 16 + r) * 64 + lane) * 4;
}
C1_HD inline int dl3_lds_bytes(const DenseConv3x3Geom& g) {
  const int stage = 4 * g.fp_max * DL3_PIX_BYTES;
  const int red = dl3_red_off(g.NT, 4, 0, 0, 0);
  return stage > red ? stage : red;
}

inline void dl3_set_rows(DenseConv3x3Geom* g, int r) {
  g->R = r;
  g->NT = r * g->W > 32 ? 2 : 1;
  g->tiles = (g->N * g->H + r - 1) / r;
  g->fp_max = 0;
  for (int t = 0; t < g->tiles; ++t) {
    const int fp = dl3_tile_fp(*g, t);
    if (fp > g->fp_max) g->fp_max = fp;
  }
}

// Chooses the tiling; false when the kernel does not support the shape
// or the slot does not lie inside the buffer's image. With 32 output
// channels all the parallelism comes from pixels, so a tile takes as
// many rows as fit 64 columns only while that still leaves
// DL3_WG_TARGET workgroups; small batches and planes run one row per
// workgroup. The choice affects speed only: an output element's chain is
// the same at every R.
inline bool dl_plan_b(DenseConv3x3Geom* g, int N, int C, int H, int W,
                      int k0, long os) {
  if (N < 1 || H < 1 || W < 1 || W > 64) return false;
  if (C < DL3_CK || C % DL3_CK || k0 < 0) return false;
  const long hw = (long)H * W;
  if (os < hw || (long)k0 + DL3_K > os / hw) return false;
  if ((long)N * C * hw >= (1L << 31) || (long)N * os >= (1L << 31)) {
    return false;
  }
  g->N = N, g->C = C, g->H = H, g->W = W;
  g->HW = H * W, g->PH = H + 2, g->PW = W + 2;
  g->k0 = k0, g->os = os;
  int r = 64 / W;
  if (r > N * H) r = N * H;
  while (r > 1 && (N * H + r - 1) / r < DL3_WG_TARGET) --r;
  dl3_set_rows(g, r);
  while (g->R > 1 && dl3_lds_bytes(*g) > DL_LDS_MAX) dl3_set_rows(g, g->R - 1);
  return dl3_lds_bytes(*g) <= DL_LDS_MAX;
}
