"""Bounds of the fused 1x1 conv kernel's addressing, checked on the CPU.

conv1x1_index.h holds, as host+device helpers, all the tile -> address
arithmetic of client_amd/ops/csrc/conv1x1.hip. A small host program
walks every workgroup of a shape the way the kernel does and checks that

  - every global load (input, packed weights, residual) and every store
    lies inside its tensor, with the alignment its width needs,
  - every LDS store, fragment read and exchange access lies inside the
    region it belongs to, and the launch fits the LDS,
  - the pixel a fragment read finds in LDS for column j is the input
    pixel of that column (or a zero column past the batch),
  - every output element is stored exactly once, and its residual is the
    element at the same offset.
"""

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "client_amd" / "ops" / "csrc"

# (C, K, H, W): the stride-1 1x1 convs of a 224x224 ResNet50 forward ...
SERVED = [
    (64, 64, 56, 56), (256, 64, 56, 56), (256, 128, 56, 56),
    (512, 128, 28, 28), (512, 256, 28, 28), (1024, 256, 14, 14),
    (1024, 512, 14, 14), (2048, 512, 7, 7),
    (64, 256, 56, 56), (128, 512, 28, 28), (256, 1024, 14, 14),
    (512, 2048, 7, 7),
]
# ... and (N, C, K, H, W) of tests/test_conv1x1_gpu.py
TESTED = [
    (1, 64, 64, 7, 7), (3, 64, 64, 7, 7), (2, 64, 128, 14, 14),
    (1, 64, 64, 9, 5), (1, 32, 64, 1, 1), (2, 2048, 64, 7, 7),
    (1, 64, 256, 56, 56), (6, 64, 256, 56, 56), (2, 64, 64, 4, 6),
    (336, 64, 256, 7, 7), (42, 64, 512, 14, 14),
]
# ... and of tests/test_conv_rounding_gpu.py with the variant each was
# chosen to reach: the smallest batches at which K = 2048 gives the 512
# workgroups of the 128-column kernels
ROUNDING = {
    (3, 96, 64, 7, 7): "NT=1 VL=1 VS=0",
    (2, 64, 128, 14, 14): "NT=1 VL=2 VS=0",
    (2, 96, 64, 4, 6): "NT=1 VL=2 VS=1",
    (1, 32, 64, 1, 1): "NT=1 VL=1 VS=0",
    (2, 2048, 64, 7, 7): "NT=1 VL=1 VS=0",
    (40, 32, 2048, 7, 7): "NT=2 VL=1 VS=0",
    (10, 32, 2048, 14, 14): "NT=2 VL=2 VS=0",
    (31, 32, 2048, 8, 8): "NT=2 VL=2 VS=1",
}
TESTED += [c for c in ROUNDING if c not in TESTED]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv1x1_index.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAIL line %d: %s (block %d)\n", __LINE__, #cond, b);  \
      return 1;                                                          \
    }                                                                    \
  } while (0)

int main(int argc, char** argv) {
  const int N = atoi(argv[1]), C = atoi(argv[2]), K = atoi(argv[3]);
  const int H = atoi(argv[4]), W = atoi(argv[5]);
  Conv1x1Geom g;
  int b = -1;
  if (!c1_plan(&g, N, C, K, H, W)) {
    std::printf("UNSUPPORTED\n");
    return 0;
  }
  const long hw = (long)H * W;
  const long x_elems = (long)N * C * hw, o_elems = (long)N * K * hw;
  const long w_elems = (long)C * K;
  CHECK(g.HW == hw && g.J == N * hw && g.mrows * C1_BM == K);
  CHECK(g.NT == 1 || g.NT == 2);
  CHECK(g.VL == 1 || (g.VL == 2 && hw % 2 == 0));
  CHECK(g.VS == 0 || (g.VL == 2 && hw % 8 == 0));
  const int bn = c1_bn(g);
  CHECK((long)g.tiles * bn >= g.J && (long)(g.tiles - 1) * bn < g.J);
  const int buf = c1_buf_bytes(g.NT), x_lds = bn * C1_PIX_BYTES;
  CHECK(2 * buf == c1_lds_bytes(g.NT) && c1_lds_bytes(g.NT) <= C1_LDS_MAX);
  CHECK(C1_A_BYTES + x_lds == buf && c1_ex_bytes(g.NT) <= 2 * buf);
  const int items = c1_items(g);
  const int per_thread = (items + C1_THREADS - 1) / C1_THREADS;
  CHECK(items == bn / g.VL * 4 && per_thread * C1_THREADS >= items);
  std::vector<unsigned char> written(o_elems, 0);
  std::vector<long> staged(bn);  // column of the tile -> x offset, -1 zero
  std::vector<unsigned char> filled(x_lds);
  long loads = 0;
  const long blocks = (long)g.tiles * g.mrows;
  for (b = 0; b < blocks; ++b) {
    const int tile = c1_block_tile(g, b), m0 = c1_block_m0(g, b);
    CHECK(tile >= 0 && tile < g.tiles && m0 >= 0 && m0 + C1_BM <= K);
    CHECK(b == tile * g.mrows + m0 / C1_BM);
    const int j0 = tile * bn;
    // staging: every item, every chunk
    std::fill(filled.begin(), filled.end(), 0);
    for (int it = 0; it < items; ++it) {
      const int cg = c1_item_cg(g, it), col = c1_item_col(g, it);
      CHECK(cg >= 0 && cg < 4 && col >= 0 && col + g.VL <= bn);
      const long s = c1_col_src(g, j0 + col);
      for (int v = 0; v < g.VL; ++v) {
        const int dst = c1_lds_pix(col, cg) + v * C1_PIX_BYTES;
        CHECK(dst >= 0 && dst % 16 == 0 && dst + 16 <= x_lds);
        for (int q = 0; q < 16; ++q) CHECK(filled[dst + q]++ == 0);
        // a 4-byte load's second pixel is the next column's pixel
        const long sv = c1_col_src(g, j0 + col + v);
        CHECK(s < 0 ? sv < 0 : sv == s + v);
        if (cg == 0) staged[col + v] = sv;
      }
      if (s < 0) continue;
      for (int c0 = 0; c0 < C; c0 += C1_CK)
        for (int c = 0; c < 8; ++c) {
          const long off = s + ((long)cg * 8 + c0 + c) * hw;
          CHECK(off >= 0 && off + g.VL <= x_elems && off % g.VL == 0);
          // inside channel c0 + cg*8 + c of the column's own image
          CHECK(off / hw == (j0 + col) / hw * C + c0 + cg * 8 + c);
          ++loads;
        }
    }
    // every 16-byte group a fragment read touches was staged
    for (int col = 0; col < bn; ++col) {
      for (int cg = 0; cg < 4; ++cg) {
        const int rd = c1_lds_pix(col, cg);
        CHECK(rd >= 0 && rd + 16 <= x_lds && filled[rd] == 1);
      }
      // the pixel found there is this column's input pixel
      const int j = j0 + col;
      const long want = j < g.J ? (long)(j / hw) * C * hw + j % hw : -1;
      CHECK(staged[col] == want);
    }
    // weights: global units and A-fragment reads
    for (int c0 = 0; c0 < C; c0 += C1_CK)
      for (int v = 0; v < C1_THREADS; ++v) {
        const long goff = c1_w_off(g, c0, m0, v);
        CHECK(goff >= 0 && goff % 8 == 0 && goff + 8 <= w_elems);
        CHECK(v * 16 + 16 <= C1_A_BYTES);
        // packed [C/16][K][16]: unit v holds row m0 + (v&127)/2, input
        // channels c0 + 16*(v>>7) + 8*(v&1) ..
        const long row = m0 + (v & 127) / 2;
        const long ch = c0 + 16 * (v >> 7) + 8 * (v & 1);
        CHECK(goff == ((ch / 16) * K + row) * 16 + ch % 16);
      }
    for (int kk = 0; kk < 2; ++kk)
      for (int row = 0; row < C1_BM; ++row)
        for (int half = 0; half < 2; ++half) {
          const int rd = c1_lds_a(kk, row, half);
          CHECK(rd >= 0 && rd % 16 == 0 && rd + 16 <= C1_A_BYTES);
          // the unit staged there: v = kk*128 + row*2 + half
          CHECK(rd == (kk * 128 + row * 2 + half) * 16);
        }
    // stores (and residual loads, at the same offsets)
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
            // element q is column j0 + col + q of channel m0 + ch
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
"""


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv1x1_index")
    src = d / "conv1x1_index_check.cc"
    src.write_text(PROGRAM)
    exe = d / "conv1x1_index_check"
    proc = subprocess.run(
        ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{CSRC}",
         str(src), "-o", str(exe)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return exe


def _run(exe, n, c, k, h, w):
    proc = subprocess.run([str(exe), *map(str, (n, c, k, h, w))],
                          capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout.strip()


@pytest.mark.parametrize("shape", SERVED, ids=lambda s: "x".join(map(str, s)))
def test_served_shapes_in_bounds_and_written_once(checker, shape):
    for n in (8, 32):
        out = _run(checker, n, *shape)
        assert out.startswith("OK"), (n, out)


@pytest.mark.parametrize("case", TESTED, ids=lambda s: "x".join(map(str, s)))
def test_gpu_test_shapes_in_bounds_and_written_once(checker, case):
    out = _run(checker, *case)
    assert out.startswith("OK"), out
    # and each image of the batch alone, as the batch-invariance test runs
    assert _run(checker, 1, *case[1:]).startswith("OK")


def test_every_kernel_variant_is_walked(checker):
    seen = set()
    for case in TESTED:
        seen.add(tuple(_run(checker, *case).split()[1:4]))
    assert seen == {(f"NT={nt}", f"VL={vl}", f"VS={vs}")
                    for nt in (1, 2) for vl, vs in ((1, 0), (2, 0), (2, 1))}


def test_rounding_test_shapes_reach_their_variants(checker):
    import conv_refs as cr

    assert set(cr.CONV1X1_SHAPES) == set(ROUNDING)
    assert set(cr.CONV1X1_INTERVAL_SHAPES
               + cr.CONV1X1_NONFINITE_SHAPES) <= set(ROUNDING)
    for case, variant in ROUNDING.items():
        assert _run(checker, *case).split()[1:4] == variant.split(), case
    # one image fewer and the 128-column cases fall to the 64-column kernel
    for case in ((39, 32, 2048, 7, 7), (9, 32, 2048, 14, 14),
                 (30, 32, 2048, 8, 8)):
        assert _run(checker, *case).split()[1] == "NT=1", case


@pytest.mark.parametrize("case", [
    (2, 48, 64, 14, 14),     # C not a multiple of the 32-channel chunk
    (2, 16, 64, 14, 14),     # C below one chunk
    (2, 64, 96, 14, 14),     # K not a multiple of the 64-row tile
    (2, 64, 64, 0, 14),
    (0, 64, 64, 14, 14),
    (64, 2048, 64, 128, 128),  # offsets past 2^31
])
def test_unsupported_shapes_are_rejected(checker, case):
    assert _run(checker, *case) == "UNSUPPORTED"
