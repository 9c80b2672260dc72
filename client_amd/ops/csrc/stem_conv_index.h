// Tile geometry and every address of the fused stem kernel
// (stem_conv.hip): 7x7 stride-2 pad-3 conv, 3 -> 64 channels, + bias +
// ReLU + 3x3 stride-2 pad-1 max-pool, NCHW bf16. Plain C++ so host code
// can form the same offsets the kernel forms.
//
// A tile is SC_TR x SC_TC pooled pixels of one image, all 64 channels.
// Pooled pixel (pr, pc) takes the maximum over conv pixels 2*pr-1..2*pr+1
// x 2*pc-1..2*pc+1, so the tile at pooled origin (pr0, pc0) needs the
// SC_CR x SC_CC conv pixels from (2*pr0-1, 2*pc0-1) on; its one halo row
// and column are recomputed, not exchanged. Conv pixel (oy, ox) reads
// input rows 2*oy-3..2*oy+3 and, with kx padded to 8, input columns
// 2*ox-3..2*ox+4, so the tile's input footprint is SC_FR rows x SC_FC
// columns from (4*pr0-5, 4*pc0-5) on.
//
// LDS, two regions:
//   x  SC_LINES lines of SC_X_PITCH bytes; line = footprint row * 3 +
//      channel, a line is SC_FC bf16 as they lie in NCHW. K group
//      g = ky*3 + c of local conv pixel (oyl, oxl) is the 16 bytes at
//      line 6*oyl + g, byte 4*oxl.
//   c  the finished conv map, bf16 [64][SC_CR][SC_C_PITCH].
#pragma once

#ifndef CA_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define CA_HD __host__ __device__
#else
#define CA_HD
#endif
#endif

enum {
  SC_K = 64,         // output channels
  SC_THREADS = 256,  // 4 waves as 2 (channel halves) x 2 (column tiles)
  SC_TR = 2,         // pooled rows per tile
  SC_TC = 28,        // pooled columns per tile
  SC_CR = 2 * SC_TR + 1,         // conv rows under a tile (5)
  SC_CC = 2 * SC_TC + 1,         // conv columns under a tile (57)
  SC_PIX = SC_CR * SC_CC,        // GEMM columns of a tile (285)
  SC_NT = (SC_PIX + 31) / 32,    // 32-column MFMA tiles (9)
  SC_FR = 2 * SC_CR + 5,         // footprint rows (15)
  SC_FC = 2 * SC_CC + 6,         // footprint columns, kx pad included (120)
  SC_LINES = SC_FR * 3,          // (row, channel) lines in LDS (45)
  SC_X_PITCH = 256,              // bytes per line
  SC_GROUPS = 21,                // real (ky, c) groups; group 21 is zero
  SC_STEPS = 11,                 // MFMA k steps: 22 groups x 8 / 16
  SC_PAIRS = SC_FC / 2 + 1,      // staged column pairs per line (61)
  SC_STAGE_ITEMS = SC_LINES * SC_PAIRS,
  SC_C_PITCH = SC_CC + 1,        // conv map row pitch, elements (even)
  SC_C_CH = SC_CR * SC_C_PITCH,  // conv map channel pitch, elements
  SC_POOL_G = SC_TC / 4,         // groups of 4 pooled columns per row
  SC_POOL_ITEMS = SC_K * SC_TR * SC_POOL_G,
  SC_X_BYTES = SC_LINES * SC_X_PITCH,
  SC_C_BYTES = SC_K * SC_C_CH * 2,
  SC_LDS_BYTES = SC_X_BYTES + SC_C_BYTES,
  SC_W_ELEMS = 2 * SC_STEPS * 64 * 8,  // packed weight, bf16 elements
  SC_MAX_GRID = 768,                   // workgroups; tiles are looped over
};

static_assert(SC_TC % 4 == 0, "pool items are 4 pooled columns");
static_assert(SC_FC * 2 <= SC_X_PITCH, "a line holds the footprint row");
static_assert(SC_C_PITCH % 2 == 0, "pool reads the conv map as dwords");
static_assert(SC_LDS_BYTES <= 64 * 1024, "static LDS");

struct StemGeom {
  int N, H, W;
  int OH, OW;  // conv map
  int PH, PW;  // pooled map
  int tiles_y, tiles_x;
  int tiles;   // N * tiles_y * tiles_x
};

// false when the kernel does not support the shape: every element
// offset of x and out must fit 31 bits
inline bool sc_plan(StemGeom* g, int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return false;
  g->N = N, g->H = H, g->W = W;
  g->OH = (H - 1) / 2 + 1;
  g->OW = (W - 1) / 2 + 1;
  g->PH = (g->OH - 1) / 2 + 1;
  g->PW = (g->OW - 1) / 2 + 1;
  if ((long)N * 3 * H * W >= (1L << 31)) return false;
  if ((long)N * SC_K * g->PH * g->PW >= (1L << 31)) return false;
  g->tiles_y = (g->PH + SC_TR - 1) / SC_TR;
  g->tiles_x = (g->PW + SC_TC - 1) / SC_TC;
  const long tiles = (long)N * g->tiles_y * g->tiles_x;
  if (tiles >= (1L << 31)) return false;
  g->tiles = (int)tiles;
  return true;
}

inline int sc_grid(const StemGeom& g) {
  return g.tiles < SC_MAX_GRID ? g.tiles : SC_MAX_GRID;
}

// tile -> image and pooled origin
CA_HD inline void sc_tile(const StemGeom& g, int tile, int* n, int* pr0,
                          int* pc0) {
  const int per = g.tiles_y * g.tiles_x;
  *n = tile / per;
  const int t = tile - *n * per;
  const int ty = t / g.tiles_x;
  *pr0 = ty * SC_TR;
  *pc0 = (t - ty * g.tiles_x) * SC_TC;
}

// first conv row/column and first input row/column under a tile
CA_HD inline int sc_conv0(int p0) { return 2 * p0 - 1; }
CA_HD inline int sc_in0(int p0) { return 4 * p0 - 5; }

// Footprint element (line, l) of the tile at (n, pr0, pc0) -> element
// offset in x, or -1 for a halo element, which is staged as zero and
// never addressed in global memory. l may be -1 or SC_FC (the far halves
// of the first and last staged pair); those are not stored in LDS.
CA_HD inline long sc_stage_src(const StemGeom& g, int n, int pr0, int pc0,
                               int line, int l) {
  const int row = line / 3;
  const int c = line - row * 3;
  const int iy = sc_in0(pr0) + row;
  const int ix = sc_in0(pc0) + l;
  if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) return -1;
  return (((long)n * 3 + c) * g.H + iy) * g.W + ix;
}

// LDS byte offset (x region) of footprint element (line, l), 0 <= l < SC_FC
CA_HD inline int sc_stage_dst(int line, int l) {
  return line * SC_X_PITCH + l * 2;
}

// GEMM column j of a tile -> local conv pixel; false for a padding column
// (j >= SC_PIX), which computes on pixel (0, 0) and is dropped
CA_HD inline bool sc_column(int j, int* oyl, int* oxl) {
  *oyl = 0, *oxl = 0;
  if (j >= SC_PIX) return false;
  *oyl = j / SC_CC;
  *oxl = j - *oyl * SC_CC;
  return true;
}

// LDS byte offset (x region) of K group grp (< SC_GROUPS) of a local conv
// pixel: 16 bytes, 4-byte aligned
CA_HD inline int sc_frag_off(int oyl, int oxl, int grp) {
  return (6 * oyl + grp) * SC_X_PITCH + 4 * oxl;
}

// element index (c region) of channel k at a local conv pixel
CA_HD inline int sc_conv_idx(int k, int oyl, int oxl) {
  return k * SC_C_CH + oyl * SC_C_PITCH + oxl;
}

// true when the tile's local conv pixel lies inside the conv map; the
// others are stored as -inf and so take no part in a maximum
CA_HD inline bool sc_conv_inside(const StemGeom& g, int pr0, int pc0,
                                 int oyl, int oxl) {
  const int oy = sc_conv0(pr0) + oyl;
  const int ox = sc_conv0(pc0) + oxl;
  return oy >= 0 && oy < g.OH && ox >= 0 && ox < g.OW;
}

// Pool item -> channel, local pooled row, group of 4 pooled columns.
// Its window rows are local conv rows 2*prl..2*prl+2, its 9 window
// columns local conv columns 8*grp..8*grp+8.
CA_HD inline void sc_pool_item(int item, int* k, int* prl, int* grp) {
  *grp = item % SC_POOL_G;
  const int r = item / SC_POOL_G;
  *prl = r % SC_TR;
  *k = r / SC_TR;
}

// element offset in out of pooled pixel (pr, pc) of channel k, image n
CA_HD inline long sc_out_off(const StemGeom& g, int n, int k, int pr,
                             int pc) {
  return (((long)n * SC_K + k) * g.PH + pr) * g.PW + pc;
}
