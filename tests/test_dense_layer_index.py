"""Bounds of the two dense-layer kernels' addressing, checked on the CPU.

dense_layer_index.h holds, as host+device helpers, the tile -> address
arithmetic of client_amd/ops/csrc/dense_layer.hip. A small host program
walks every workgroup of a shape the way the kernel bodies do.

Kernel A (dense_conv1x1_*): everything tests/test_conv1x1_index.py checks
of conv1x1.hip, with the image stride xs of the input: every load lies in
a channel < C of the column's own image of the block buffer, a dword load
is at an even element, scale and shift sit in front of the staging
buffers and an item reads its own eight channels of each, and every
output element is stored exactly once.

Kernel B (dense_conv3x3_k32_*): the padded row space, the footprints that
span images, the four waves' staging regions, the nine tap reads of every
column (padding columns included), the split of the reduction over waves
and rounds, the packed weights, the reduction region, and the stores into
the 32-channel slot at k0 of a buffer with image stride os: every slot
element exactly once and nothing else.
"""

import subprocess
from pathlib import Path

import pytest

import dense_layer_refs as dr

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "client_amd" / "ops" / "csrc"

# DenseNet-121 at 224x224: (first C, last C, C_end, H) of each block's
# first and last dense layer, and (C, K, H) of the three transitions
BLOCKS = [(64, 224, 256, 56), (128, 480, 512, 28), (256, 992, 1024, 14),
          (512, 992, 1024, 7)]
TRANSITIONS = [(256, 128, 56), (512, 256, 28), (1024, 512, 14)]
# A: (C, K, H, W, xs); B: (C, H, W, k0, os), both without the batch
SERVED_A = ([(c, 128, h, h, ce * h * h) for c0, c1, ce, h in BLOCKS
             for c in (c0, c1)]
            + [(c, k, h, h, c * h * h) for c, k, h in TRANSITIONS])
SERVED_B = [(128, h, h, c, ce * h * h) for c0, c1, ce, h in BLOCKS
            for c in (c0, c1)]

# the cases of tests/test_dense_layer_gpu.py: A (N, C, C_buf, K, H, W),
# also with C_buf = C; B (N, C, C_buf, k0, H, W), also at the next slot of
# a wider buffer; both also one image at a time
GPU_A = [(1, 32, 64, 64, 1, 1), (3, 64, 96, 128, 7, 7),
         (2, 96, 160, 128, 4, 6), (2, 992, 1024, 128, 7, 7),
         (2, 256, 256, 128, 14, 14), (11, 64, 96, 128, 56, 56)]
GPU_B = [(1, 32, 96, 64, 1, 1), (3, 128, 160, 96, 7, 7),
         (2, 128, 96, 64, 9, 5), (1, 128, 96, 64, 56, 56),
         (2, 128, 1024, 992, 7, 7), (80, 32, 32, 0, 7, 7)]

# tests/test_dense_layer_rounding_gpu.py: the plan each case was chosen
# to reach. The 128-column cases are the smallest batches at which K =
# 2048 gives the 512 workgroups of the wide tile.
ROUNDING_A = {
    (3, 96, 64, 7, 7, 128 * 49): "NT=1 VL=1 VS=0",
    (2, 64, 128, 14, 14, 96 * 196): "NT=1 VL=2 VS=0",
    (2, 96, 64, 4, 6, 160 * 24): "NT=1 VL=2 VS=1",
    (2, 64, 64, 4, 4, 64 * 16 + 1): "NT=1 VL=1 VS=0",
    (1, 32, 64, 1, 1, 32): "NT=1 VL=1 VS=0",
    (2, 1024, 64, 7, 7, 1024 * 49): "NT=1 VL=1 VS=0",
    (40, 32, 2048, 7, 7, 64 * 49): "NT=2 VL=1 VS=0",
    (10, 32, 2048, 14, 14, 64 * 196): "NT=2 VL=2 VS=0",
    (31, 32, 2048, 8, 8, 64 * 64): "NT=2 VL=2 VS=1",
    (31, 32, 2048, 8, 8, 64 * 64 + 1): "NT=2 VL=1 VS=0",
}
# (N, C, H, W, k0, C_buf) -> NT, R
ROUNDING_B = {
    (3, 160, 7, 7, 32, 96): "NT=1 R=1",
    (2, 256, 9, 5, 0, 32): "NT=1 R=1",
    (96, 32, 8, 20, 0, 32): "NT=2 R=3",
    (128, 32, 4, 32, 0, 32): "NT=2 R=2",
    (2, 160, 3, 33, 32, 96): "NT=2 R=1",
    (1, 64, 3, 64, 0, 32): "NT=2 R=1",
    (80, 32, 7, 7, 0, 32): "NT=1 R=2",
    (1, 32, 1, 1, 0, 32): "NT=1 R=1",
}

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dense_layer_index.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAIL line %d: %s (block %d)\n", __LINE__, #cond, b);  \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static int walk_a(int N, int C, int K, int H, int W, long xs) {
  DenseConv1x1Geom dg;
  int b = -1;
  if (!dl_plan_a(&dg, N, C, K, H, W, xs)) {
    std::printf("UNSUPPORTED\n");
    return 0;
  }
  const Conv1x1Geom& g = dg.c;
  const long hw = (long)H * W;
  const long o_elems = (long)N * K * hw, w_elems = (long)C * K;
  const long x_end = (long)(N - 1) * xs + C * hw;  // end of the read prefix
  CHECK(dg.xs == xs && xs >= C * hw && (long)N * xs < (1L << 31));
  CHECK(g.HW == hw && g.J == N * hw && g.mrows * C1_BM == K && g.C == C);
  CHECK(g.NT == 1 || g.NT == 2);
  CHECK(g.VL == 1 || (g.VL == 2 && hw % 2 == 0 && xs % 2 == 0));
  CHECK(g.VS == 0 || (g.VL == 2 && hw % 8 == 0));
  const int bn = c1_bn(g);
  CHECK((long)g.tiles * bn >= g.J && (long)(g.tiles - 1) * bn < g.J);
  // LDS: scale[C], shift[C], then the two buffers
  const int ss = dl_ss_bytes(C), half = C * 4;
  const int buf = c1_buf_bytes(g.NT), x_lds = bn * C1_PIX_BYTES;
  CHECK(ss == 2 * half && ss % 16 == 0);
  CHECK(dl_a_lds_bytes(dg) == ss + 2 * buf && dl_a_lds_bytes(dg) <= DL_LDS_MAX);
  CHECK(C1_A_BYTES + x_lds == buf && buf % 16 == 0);
  CHECK(c1_ex_bytes(g.NT) <= 2 * buf);
  // the staging loop of scale and shift fills both halves once
  {
    std::vector<int> fill(2 * C, 0);
    for (int tid = 0; tid < C1_THREADS; ++tid)
      for (int i = tid; i < 2 * C; i += C1_THREADS) ++fill[i];
    for (int i = 0; i < 2 * C; ++i) CHECK(fill[i] == 1);
  }
  const int items = c1_items(g);
  const int per_thread = (items + C1_THREADS - 1) / C1_THREADS;
  CHECK(items == bn / g.VL * 4 && per_thread * C1_THREADS >= items);
  std::vector<unsigned char> written(o_elems, 0);
  std::vector<long> staged(bn);
  std::vector<unsigned char> filled(x_lds);
  long loads = 0;
  const long blocks = (long)g.tiles * g.mrows;
  for (b = 0; b < blocks; ++b) {
    const int tile = c1_block_tile(g, b), m0 = c1_block_m0(g, b);
    CHECK(tile >= 0 && tile < g.tiles && m0 >= 0 && m0 + C1_BM <= K);
    CHECK(b == tile * g.mrows + m0 / C1_BM);
    const int j0 = tile * bn;
    std::fill(filled.begin(), filled.end(), 0);
    for (int it = 0; it < items; ++it) {
      const int cg = c1_item_cg(g, it), col = c1_item_col(g, it);
      CHECK(cg >= 0 && cg < 4 && col >= 0 && col + g.VL <= bn);
      const long s = dl_col_src(dg, j0 + col);
      for (int v = 0; v < g.VL; ++v) {
        const int dst = c1_lds_pix(col, cg) + v * C1_PIX_BYTES;
        CHECK(dst >= 0 && dst % 16 == 0 && dst + 16 <= x_lds);
        for (int q = 0; q < 16; ++q) CHECK(filled[dst + q]++ == 0);
        // a 4-byte load's second pixel is the next column's pixel
        const long sv = dl_col_src(dg, j0 + col + v);
        CHECK(s < 0 ? sv < 0 : sv == s + v);
        if (cg == 0) staged[col + v] = sv;
      }
      const int ch8 = cg * 8;
      for (int c0 = 0; c0 < C; c0 += C1_CK) {
        // the item's 16-byte reads of scale and shift: ss + c0 + ch8 and
        // four floats on, and the same at + C
        for (int q = 0; q < 2; ++q) {
          const int sc = (c0 + ch8 + 4 * q) * 4;
          const int sh = (C + c0 + ch8 + 4 * q) * 4;
          CHECK(sc % 16 == 0 && sc >= 0 && sc + 16 <= half);
          CHECK(sh % 16 == 0 && sh >= half && sh + 16 <= ss);
          // float e of the read is scale / shift of channel c0+cg*8+4q+e
          CHECK(sc / 4 == c0 + cg * 8 + 4 * q && sh / 4 - C == sc / 4);
        }
        if (s < 0) continue;
        const long n = (j0 + col) / hw;
        for (int c = 0; c < 8; ++c) {
          const long ch = c0 + cg * 8 + c;
          const long off = s + ((long)cg * 8 + c0 + c) * hw;
          CHECK(ch < C && off % g.VL == 0);
          // inside channel ch of the column's own image
          CHECK(off >= n * xs + ch * hw && off + g.VL <= n * xs + (ch + 1) * hw);
          CHECK(off + g.VL <= x_end);
          CHECK(off == n * xs + ch * hw + (j0 + col) % hw);
          ++loads;
        }
      }
    }
    for (int col = 0; col < bn; ++col) {
      for (int cg = 0; cg < 4; ++cg) {
        const int rd = c1_lds_pix(col, cg);
        CHECK(rd >= 0 && rd + 16 <= x_lds && filled[rd] == 1);
      }
      const int j = j0 + col;
      const long want = j < g.J ? (long)(j / hw) * xs + j % hw : -1;
      CHECK(staged[col] == want);
    }
    // weights: global units and A-fragment reads
    for (int c0 = 0; c0 < C; c0 += C1_CK)
      for (int v = 0; v < C1_THREADS; ++v) {
        const long goff = c1_w_off(g, c0, m0, v);
        CHECK(goff >= 0 && goff % 8 == 0 && goff + 8 <= w_elems);
        CHECK(v * 16 + 16 <= C1_A_BYTES);
        const long row = m0 + (v & 127) / 2;
        const long ch = c0 + 16 * (v >> 7) + 8 * (v & 1);
        CHECK(goff == ((ch / 16) * K + row) * 16 + ch % 16);
      }
    for (int kk = 0; kk < 2; ++kk)
      for (int row = 0; row < C1_BM; ++row)
        for (int hf = 0; hf < 2; ++hf) {
          const int rd = c1_lds_a(kk, row, hf);
          CHECK(rd >= 0 && rd % 16 == 0 && rd + 16 <= C1_A_BYTES);
          CHECK(rd == (kk * 128 + row * 2 + hf) * 16);
        }
    if (g.VS) {
      for (int ch = 0; ch < C1_BM; ++ch)
        for (int col = 0; col < bn; ++col) {
          const int e = c1_lds_ex(g, ch, col);
          CHECK(e >= 0 && e + 2 <= c1_ex_bytes(g.NT));
          CHECK(col % 8 || e % 16 == 0);
        }
      const int groups = bn / 8;
      for (int tid = 0; tid < C1_THREADS; ++tid) {
        const int col = (tid % groups) * 8;
        const long o = c1_col_out(g, j0 + col);
        int rows = 0;
        for (int ch = tid / groups; ch < C1_BM; ch += C1_THREADS / groups) {
          ++rows;
          if (o < 0) continue;
          const long off = o + (long)(m0 + ch) * hw;
          CHECK(off % 8 == 0 && off >= 0 && off + 8 <= o_elems);
          for (int q = 0; q < 8; ++q) {
            const long j = j0 + col + q;
            CHECK(off + q == ((j / hw) * K + m0 + ch) * hw + j % hw);
            CHECK(written[off + q]++ == 0);
          }
        }
        CHECK(rows * (C1_THREADS / groups) == C1_BM);
      }
    } else {
      for (int col = 0; col < bn; ++col) {
        const long o = c1_col_out(g, j0 + col);
        if (o < 0) {
          CHECK(j0 + col >= g.J);
          continue;
        }
        const long j = j0 + col;
        for (int k = m0; k < m0 + C1_BM; ++k) {
          const long off = o + (long)k * hw;
          CHECK(off >= 0 && off < o_elems);
          CHECK(off == ((j / hw) * K + k) * hw + j % hw);
          CHECK(written[off]++ == 0);
        }
      }
    }
  }
  b = -1;
  for (long i = 0; i < o_elems; ++i) CHECK(written[i] == 1);
  std::printf("OK NT=%d VL=%d VS=%d tiles=%d loads=%ld\n", g.NT, g.VL, g.VS,
              g.tiles, loads);
  return 0;
}

static int walk_b(int N, int C, int H, int W, int k0, long os) {
  DenseConv3x3Geom g;
  int b = -1;
  if (!dl_plan_b(&g, N, C, H, W, k0, os)) {
    std::printf("UNSUPPORTED\n");
    return 0;
  }
  const long hw = (long)H * W;
  const long x_elems = (long)N * C * hw, w_elems = 9L * C * DL3_K;
  const int chunks = C / DL3_CK;
  CHECK(g.N == N && g.C == C && g.H == H && g.W == W && g.HW == hw);
  CHECK(g.PH == H + 2 && g.PW == W + 2 && g.k0 == k0 && g.os == os);
  CHECK(k0 >= 0 && (k0 + DL3_K) * hw <= os && (long)N * os < (1L << 31));
  CHECK((g.NT == 1 || g.NT == 2) && g.R >= 1 && g.R * W <= 32 * g.NT);
  CHECK((long)g.tiles * g.R >= (long)N * H && (long)(g.tiles - 1) * g.R < (long)N * H);
  const int lds = dl3_lds_bytes(g);
  const int region = g.fp_max * DL3_PIX_BYTES;
  CHECK(lds <= DL_LDS_MAX && region % 16 == 0);
  // the four waves' staging regions: consecutive, inside the LDS
  for (int wave = 0; wave < 4; ++wave) {
    const int lo = wave * g.fp_max * DL3_PIX_BYTES;
    CHECK(lo == wave * region && lo + region <= lds);
  }
  // every chunk is one wave's in one round
  {
    std::vector<int> taken(chunks, 0);
    int rounds = 0;
    for (int first = 0; first < chunks; first += 4, ++rounds)
      for (int wave = 0; wave < 4; ++wave)
        if (first + wave < chunks) ++taken[first + wave];
    for (int c = 0; c < chunks; ++c) CHECK(taken[c] == 1);
    CHECK(rounds == (chunks + 3) / 4);
  }
  // packed weights [3][3][C/16][32][16]
  for (int chunk = 0; chunk < chunks; ++chunk)
    for (int f = 0; f < 18; ++f)
      for (int row = 0; row < DL3_K; ++row)
        for (int hf = 0; hf < 2; ++hf) {
          const int tap = f >> 1;
          const long off = dl3_w_off(g, tap, chunk * 2 + (f & 1), row, hf);
          CHECK(off >= 0 && off % 8 == 0 && off + 8 <= w_elems);
          const long ch = chunk * 32L + (f & 1) * 16 + hf * 8;
          CHECK(off == ((((tap / 3) * 3L + tap % 3) * (C / 16) + ch / 16)
                        * DL3_K + row) * 16 + ch % 16);
        }
  // reduction region [wave][tile][register][lane], fp32
  {
    std::vector<unsigned char> seen(lds / 4, 0);
    for (int wave = 0; wave < 4; ++wave)
      for (int t = 0; t < g.NT; ++t)
        for (int r = 0; r < 16; ++r)
          for (int lane = 0; lane < 64; ++lane) {
            const int off = dl3_red_off(g.NT, wave, t, r, lane);
            CHECK(off >= 0 && off % 4 == 0 && off + 4 <= lds);
            CHECK(seen[off / 4]++ == 0);
          }
  }
  // wave v finishes registers 4v..4v+3: register r of lane half lh is
  // output channel (r&3) + 8*(r>>2) + 4*lh, each of the 32 once
  {
    int ks[DL3_K];
    std::memset(ks, 0, sizeof ks);
    for (int wave = 0; wave < 4; ++wave)
      for (int q = 0; q < 4; ++q)
        for (int lh = 0; lh < 2; ++lh) {
          const int r = wave * 4 + q, k = q + 8 * wave + 4 * lh;
          CHECK(k == (r & 3) + 8 * (r >> 2) + 4 * lh && k < DL3_K);
          ++ks[k];
        }
    for (int k = 0; k < DL3_K; ++k) CHECK(ks[k] == 1);
  }
  std::vector<unsigned char> written((long)N * DL3_K * hw, 0);
  std::vector<long> staged(g.fp_max);
  std::vector<unsigned char> filled(region);
  long loads = 0;
  for (b = 0; b < g.tiles; ++b) {
    const int tile = b;
    const int p0 = dl3_tile_p0(g, tile), fp = dl3_tile_fp(g, tile);
    CHECK(3 * g.PW <= fp && fp <= g.fp_max && fp % g.PW == 0);
    CHECK(p0 >= 0 && p0 + fp / g.PW <= N * g.PH);
    // staging: lane's items it = lane, lane + 64, ..; item = cg*fp + pi
    std::fill(filled.begin(), filled.end(), 0);
    for (int lane = 0; lane < 64; ++lane)
      for (int it = lane; it < fp * (DL3_CK / 8); it += 64) {
        const int cg = it / fp, pi = it - cg * fp;
        CHECK(cg >= 0 && cg < 4 && pi >= 0 && pi < fp);
        const int dst = pi * DL3_PIX_BYTES + cg * 16;
        CHECK(dst % 16 == 0 && dst + 16 <= fp * DL3_PIX_BYTES);
        CHECK(dst + 16 <= region);
        for (int q = 0; q < 16; ++q) CHECK(filled[dst + q]++ == 0);
        const long s = dl3_stage_src(g, p0, pi);
        // the padded pixel: row P of the batch-wide padded row space
        const int P = p0 + pi / g.PW, pc = pi % g.PW;
        const int n = P / g.PH, pr = P % g.PH;
        const bool halo = n >= N || pr == 0 || pr == H + 1 || pc == 0 ||
                          pc == W + 1;
        CHECK((s == -1) == halo);
        if (cg == 0) staged[pi] = s;
        if (halo) continue;
        CHECK(s == ((long)n * C * H + (pr - 1)) * W + (pc - 1));
        for (int chunk = 0; chunk < chunks; ++chunk)
          for (int c = 0; c < 8; ++c) {
            const long ch = chunk * 32L + cg * 8 + c;
            const long off = s + (long)chunk * DL3_CK * hw +
                             (long)cg * 8 * hw + c * hw;
            CHECK(off >= 0 && off < x_elems && off / hw == (long)n * C + ch);
            ++loads;
          }
      }
    for (int pi = 0; pi < fp; ++pi)
      for (int cg = 0; cg < 4; ++cg)
        CHECK(filled[pi * DL3_PIX_BYTES + cg * 16] == 1);
    // columns: tap reads (padding columns too) and stores
    for (int j = 0; j < 32 * g.NT; ++j) {
      int pix;
      long o;
      const bool ok = dl3_column(g, tile, j, &pix, &o);
      const int jr = j / W, ow = j % W;
      const long go = (long)tile * g.R + jr;
      CHECK(ok == (jr < g.R && go < (long)N * H));
      const int n = ok ? go / H : 0, oh = ok ? go % H : 0;
      for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s) {
          const int tp = pix + r * g.PW + s;
          for (int f = 0; f < 2; ++f)
            for (int lh = 0; lh < 2; ++lh) {
              const int rd = tp * DL3_PIX_BYTES + f * 32 + lh * 16;
              CHECK(rd >= 0 && rd % 16 == 0 && rd + 16 <= fp * DL3_PIX_BYTES);
              CHECK(filled[rd] == 1 && rd % DL3_PIX_BYTES + 16 <= 64);
            }
          if (!ok) continue;
          const int ih = oh + r - 1, iw = ow + s - 1;
          const long want = ih < 0 || ih >= H || iw < 0 || iw >= W
                                ? -1
                                : ((long)n * C * H + ih) * W + iw;
          CHECK(staged[tp] == want);
        }
      if (!ok) {
        CHECK(pix == 0);
        continue;
      }
      for (int k = 0; k < DL3_K; ++k) {
        const long off = o + k * hw;
        CHECK(off == (long)n * os + (k0 + k) * hw + (long)oh * W + ow);
        CHECK(off >= (long)n * os + k0 * hw);
        CHECK(off < (long)n * os + (k0 + DL3_K) * hw && off < (long)(n + 1) * os);
        CHECK(written[((long)n * DL3_K + k) * hw + oh * W + ow]++ == 0);
      }
    }
  }
  b = -1;
  for (size_t i = 0; i < written.size(); ++i) CHECK(written[i] == 1);
  std::printf("OK NT=%d R=%d tiles=%d fp_max=%d lds=%d loads=%ld\n", g.NT,
              g.R, g.tiles, g.fp_max, lds, loads);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  long v[6];
  for (int i = 0; i < 6; ++i) v[i] = atol(argv[i + 2]);
  if (argv[1][0] == 'a')
    return walk_a((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5]);
  return walk_b((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5]);
}
"""


def _id(case):
    return "x".join(map(str, case))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_layer_index")
    src = d / "dense_layer_index_check.cc"
    src.write_text(PROGRAM)
    exe = d / "dense_layer_index_check"
    proc = subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{CSRC}",
         str(src), "-o", str(exe)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    cache = {}

    def run(kernel, *args):
        """kernel "a": N C K H W xs; "b": N C H W k0 os."""
        key = (kernel, *args)
        if key not in cache:
            proc = subprocess.run([str(exe), kernel, *map(str, args)],
                                  capture_output=True, text=True)
            assert proc.returncode == 0, (key, proc.stdout + proc.stderr)
            cache[key] = proc.stdout.strip()
        return cache[key]

    return run


def _b_args(case):
    """(N, C, H, W, k0, C_buf) -> the walk's N C H W k0 os."""
    n, c, h, w, k0, cb = case
    return n, c, h, w, k0, cb * h * w


@pytest.mark.parametrize("shape", SERVED_A, ids=_id)
def test_a_served_shapes_in_bounds_and_written_once(checker, shape):
    for n in (8, 32):
        out = checker("a", n, *shape)
        assert out.startswith("OK"), (n, out)


@pytest.mark.parametrize("shape", SERVED_B, ids=_id)
def test_b_served_shapes_in_bounds_and_written_once(checker, shape):
    for n in (8, 32):
        out = checker("b", n, *shape)
        assert out.startswith("OK"), (n, out)


@pytest.mark.parametrize("case", GPU_A, ids=_id)
def test_a_gpu_test_shapes(checker, case):
    n, c, cb, k, h, w = case
    for batch in (n, 1):
        for stride in (cb * h * w, c * h * w):
            out = checker("a", batch, c, k, h, w, stride)
            assert out.startswith("OK"), (batch, stride, out)


@pytest.mark.parametrize("case", GPU_B, ids=_id)
def test_b_gpu_test_shapes(checker, case):
    n, c, cb, k0, h, w = case
    for batch in (n, 1):
        for slot, width in ((k0, cb), (cb, cb + 32)):
            out = checker("b", batch, c, h, w, slot, width * h * w)
            assert out.startswith("OK"), (batch, slot, out)


def test_a_rounding_shapes_reach_their_variants(checker):
    assert list(ROUNDING_A) == dr.A_SHAPES
    assert set(dr.A_INTERVAL_SHAPES + dr.A_NONFINITE_SHAPES) <= set(ROUNDING_A)
    seen = set()
    for case, variant in ROUNDING_A.items():
        out = checker("a", *case)
        assert out.split()[:4] == ["OK", *variant.split()], (case, out)
        seen.add((variant, case[5] % 2))
        # and at the strides of the invariance test
        n, c, k, h, w, _ = case
        for xs in (c * h * w, c * h * w + 2 * h * w + 2, c * h * w + 3):
            assert checker("a", n, c, k, h, w, xs).startswith("OK"), (case, xs)
    # all six kernels, and both tile widths through the odd-stride branch
    assert {v for v, odd in seen} == {
        f"NT={nt} VL={vl} VS={vs}"
        for nt in (1, 2) for vl, vs in ((1, 0), (2, 0), (2, 1))}
    assert {v for v, odd in seen if odd} == {"NT=1 VL=1 VS=0",
                                             "NT=2 VL=1 VS=0"}
    # an odd stride is what moved those two off the 16-byte-store kernels
    for case in ROUNDING_A:
        if case[5] % 2:
            n, c, k, h, w, xs = case
            assert (h * w) % 8 == 0
            assert checker("a", n, c, k, h, w, xs - 1).split()[1:4] == [
                f"NT={ROUNDING_A[case][3]}", "VL=2", "VS=1"]
    # one image fewer and the 128-column cases fall to the 64-column kernel
    for case in ROUNDING_A:
        if ROUNDING_A[case].startswith("NT=2"):
            n, c, k, h, w, xs = case
            assert n in (40, 10, 31)
            out = checker("a", n - 1, c, k, h, w, xs)
            assert out.split()[:2] == ["OK", "NT=1"], (case, out)


def test_b_rounding_shapes_reach_their_plans(checker):
    assert list(ROUNDING_B) == dr.B_SHAPES
    assert set(dr.B_INTERVAL_SHAPES) <= set(ROUNDING_B)
    kinds = set()
    for case, plan in ROUNDING_B.items():
        out = checker("b", *_b_args(case))
        assert out.split()[:3] == ["OK", *plan.split()], (case, out)
        nt, r = (int(f.split("=")[1]) for f in plan.split())
        kinds.add((nt, r > 1))
        # the other slot and stride of the invariance test
        n, c, h, w, k0, cb = case
        assert checker("b", n, c, h, w, cb, (cb + 32) * h * w + 1).split()[:3] \
            == ["OK", *plan.split()]
    assert kinds == {(1, False), (1, True), (2, False), (2, True)}
    # the case at W = 64 fills the LDS to 63,360 of 65,536 bytes
    out = checker("b", *_b_args((1, 64, 3, 64, 0, 32)))
    assert "lds=63360" in out.split(), out
    # rounds of the reduction split: C / 128, rounded up
    assert [c for (_, c, *_) in ROUNDING_B if c > 128] == [160, 256, 160]


@pytest.mark.parametrize("case", [
    ("a", 2, 48, 64, 14, 14, 48 * 196),      # C not a multiple of 32
    ("a", 2, 16, 64, 14, 14, 16 * 196),      # C below one chunk
    ("a", 2, 64, 96, 14, 14, 64 * 196),      # K not a multiple of 64
    ("a", 2, 64, 64, 14, 14, 64 * 196 - 2),  # stride inside the prefix
    ("a", 2, 64, 64, 14, 14, 1 << 30),       # N * xs = 2^31
    ("a", 0, 64, 64, 14, 14, 64 * 196),
    ("b", 2, 48, 14, 14, 0, 96 * 196),
    ("b", 2, 16, 14, 14, 0, 96 * 196),
    ("b", 2, 64, 4, 65, 0, 96 * 4 * 65),     # a row wider than a tile
    ("b", 2, 64, 14, 14, 65, 96 * 196),      # k0 + 32 > os / HW
    ("b", 2, 64, 14, 14, 0, 195),            # os < HW
    ("b", 2, 64, 14, 14, 0, 1 << 30),        # N * os = 2^31
    ("b", 0, 64, 14, 14, 0, 96 * 196),
], ids=_id)
def test_unsupported_shapes_are_rejected(checker, case):
    assert checker(*case) == "UNSUPPORTED"
    # the same shape with the one offending value mended is walked
    mended = {"a": ("a", 2, 64, 64, 14, 14, 64 * 196),
              "b": ("b", 2, 64, 14, 14, 0, 96 * 196)}[case[0]]
    assert checker(*mended).startswith("OK")
