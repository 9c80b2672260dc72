// Tile geometry and tile -> address arithmetic of the fused 1x1 conv
// kernel (conv1x1.hip). Plain C++ so a host program can enumerate every
// global and LDS offset the kernel forms (tests/test_conv1x1_index.py).
//
// Geometry. The conv is 1x1, stride 1, NCHW. Pixels are numbered across
// the batch as columns j = n*HW + p, J = N*HW of them; column j of
// channel c lives at element (n*C + c)*HW + p of x, and its output of
// channel k at (n*K + k)*HW + p of out (and of the residual). A tile is
// BN = 64 or 128 consecutive columns, possibly spanning images; columns
// past J are staged as zeros, computed on and dropped.
//
// Workgroups are numbered with the 64-channel row fastest, so the
// K/64 workgroups that read the same input tile run next to each other.
#pragma once

// always inlined on the device: the kernels carry a target attribute, and
// a function without it that is not forced inline would become a call
#if defined(__HIPCC__) || defined(__CUDACC__)
#define C1_HD __host__ __device__ __attribute__((always_inline))
#else
#define C1_HD
#endif

enum {
  C1_BM = 64,         // output channels per workgroup
  C1_CK = 32,         // input channels per LDS chunk
  C1_THREADS = 256,   // 4 waves as 2 (channels) x 2 (columns)
  C1_PIX_BYTES = 80,  // LDS bytes per staged pixel: 32 bf16 + 16 B pad
  C1_A_BYTES = C1_CK * C1_BM * 2,  // weight chunk in LDS
  C1_EX_PAD = 8,      // bf16 elements of padding per exchange row
  C1_LDS_MAX = 64 * 1024,
};

struct Conv1x1Geom {
  int N, C, K, H, W;
  int HW;     // pixels per image
  int J;      // columns: N * HW
  int NT;     // 32-column MFMA tiles per wave (BN = 64 * NT)
  int VL;     // columns per staging load: 2 (4-byte loads) when HW is even
  int VS;     // 1: outputs leave through LDS as 16-byte stores (HW % 8 == 0)
  int tiles;  // ceil(J / BN)
  int mrows;  // K / C1_BM
};

C1_HD inline int c1_bn(const Conv1x1Geom& g) { return 64 * g.NT; }

// one of the two staging buffers: weight chunk, then BN staged pixels
C1_HD inline int c1_buf_bytes(int nt) {
  return C1_A_BYTES + 64 * nt * C1_PIX_BYTES;
}
// the exchange region [64 channels][BN + pad] bf16 reuses both buffers
C1_HD inline int c1_ex_bytes(int nt) {
  return C1_BM * (64 * nt + C1_EX_PAD) * 2;
}
C1_HD inline int c1_lds_bytes(int nt) { return 2 * c1_buf_bytes(nt); }

// workgroup -> (column tile, 64-channel row)
C1_HD inline int c1_block_tile(const Conv1x1Geom& g, int block) {
  return block / g.mrows;
}
C1_HD inline int c1_block_m0(const Conv1x1Geom& g, int block) {
  return (block % g.mrows) * C1_BM;
}

// Column j -> element offset of its pixel in channel 0 of x (add c*HW),
// or -1 for a column past the last image: staged as zero, never
// addressed in global memory.
C1_HD inline long c1_col_src(const Conv1x1Geom& g, int j) {
  if (j >= g.J) return -1;
  const int n = j / g.HW;
  return (long)n * g.C * g.HW + (j - n * g.HW);
}

// Column j -> element offset of its output in channel 0 of out and of
// the residual (add k*HW), or -1 for a padding column: nothing stored.
C1_HD inline long c1_col_out(const Conv1x1Geom& g, int j) {
  if (j >= g.J) return -1;
  const int n = j / g.HW;
  return (long)n * g.K * g.HW + (j - n * g.HW);
}

// staging item -> (8-channel group, first column in the tile); items of
// consecutive threads are consecutive column groups of one channel group
C1_HD inline int c1_items(const Conv1x1Geom& g) {
  return c1_bn(g) / g.VL * (C1_CK / 8);
}
C1_HD inline int c1_item_cg(const Conv1x1Geom& g, int item) {
  return item / (c1_bn(g) / g.VL);
}
C1_HD inline int c1_item_col(const Conv1x1Geom& g, int item) {
  return (item % (c1_bn(g) / g.VL)) * g.VL;
}

// byte offset in the staged pixels of 8-channel group cg of tile column
// col (16 bytes), for the staging store and the B-fragment read
C1_HD inline int c1_lds_pix(int col, int cg) {
  return col * C1_PIX_BYTES + cg * 16;
}

// element offset in the packed weights [C/16][K][16] of 16-byte unit v
// (0..255) of the chunk that starts at input channel c0, rows m0..m0+63;
// unit v goes to byte v*16 of the staged weight chunk
C1_HD inline long c1_w_off(const Conv1x1Geom& g, int c0, int m0, int v) {
  return (((long)(c0 >> 4) + (v >> 7)) * g.K + m0) * 16 + (long)(v & 127) * 8;
}

// byte offset of the A fragment (8 input channels 8*half.., 16-channel
// step kk) of weight row `row` (0..63) in the staged weight chunk
C1_HD inline int c1_lds_a(int kk, int row, int half) {
  return ((kk * C1_BM + row) * 16 + half * 8) * 2;
}

// byte offset of (channel row ch, tile column col) in the exchange region
C1_HD inline int c1_lds_ex(const Conv1x1Geom& g, int ch, int col) {
  return (ch * (c1_bn(g) + C1_EX_PAD) + col) * 2;
}

// Chooses the tiling for a shape; false when the kernel does not
// support it. 128-column tiles when they still give two workgroups per
// CU, otherwise 64-column tiles. Neither that choice nor the load and
// store widths change an output element's summation order.
inline bool c1_plan(Conv1x1Geom* g, int N, int C, int K, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return false;
  if (C < C1_CK || C % C1_CK || K < C1_BM || K % C1_BM) return false;
  if ((long)N * (C > K ? C : K) * H * W >= (1L << 31)) return false;
  g->N = N, g->C = C, g->K = K, g->H = H, g->W = W;
  g->HW = H * W;
  g->J = N * g->HW;
  g->VL = g->HW % 2 == 0 ? 2 : 1;
  g->VS = g->HW % 8 == 0 ? 1 : 0;
  g->mrows = K / C1_BM;
  g->NT = 2;
  g->tiles = (g->J + 127) / 128;
  if ((long)g->tiles * g->mrows < 512) {
    g->NT = 1;
    g->tiles = (g->J + 63) / 64;
  }
  return c1_lds_bytes(g->NT) <= C1_LDS_MAX &&
         c1_ex_bytes(g->NT) <= c1_lds_bytes(g->NT);
}
