// fuse_sim3_block_check.cpp — FuseSim3Block of csrc/stage_blocks.h on the CPU (tests/test_fuse_sim3_block_cpu.py builds this with -fsanitize=address,undefined).
// Every segment's offset against the segments in front of it, the two copied ranges, and every segment filled (or read) to its declared length in a malloc'd
// block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include "block_check.h"

static void fuse(size_t K, size_t F, size_t P, size_t L, bool uv) {
  FuseSim3Block b(K, F, P, L, uv);
  Check c(b);
  c.up(b.kdesc, 32 * F, true, 16); c.up(b.pdesc, 32 * P, true, 16);
  c.up(b.rec, FSM_REC_FLOATS * K, true); c.up(b.pose, FSM_POSE_FLOATS * K, false);
  c.up(b.feat_off, K + 1, true); c.up(b.cell_off, K * (FSM_CELLS + 1), true);
  c.up(b.kxy, 2 * F, true); c.up(b.cell_idx, F, false); c.up(b.koct, F, true);
  c.up(b.scale_factors, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.normal, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  const size_t n_in = 32 * F + 32 * P + 4 * (25 * K + K + 1 + K * (FSM_CELLS + 1) + 2 * F + L + 8 * P) + words(2 * F) + words(F);
  EXPECT_EQ(c.o, n_in);
  c.zero_and_down(b.n_valid, K); c.zero_and_down(b.n_hit, K);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in + 8 * K);
  c.uploaded_bytes();
  c.down(b.table, K * P); c.down(b.uv, uv ? 2 * K * P : 0);
  const size_t n_out = 8 * K + 4 * K * P + (uv ? 8 * K * P : 0);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in + 8 * K > n_out ? n_in + 8 * K : n_out);
}

int main() {
  for (int uv = 0; uv < 2; uv++) {
    fuse(0, 0, 0, 8, uv); fuse(0, 0, 5, 8, uv); fuse(3, 1001, 0, 8, uv);
    fuse(1, 0, 1, 1, uv);                                       // a keyframe without features
    for (size_t K : {1, 2, 3, 8})
      for (size_t F : {1, 2, 3, 5, 333, 1000})
        for (size_t P : {1, 63, 64, 65, 257, 2500}) fuse(K, K * F - (K > 1), P, K == 3 ? 16 : 8, uv);   // (one keyframe of several without features' worth less)
  }
  fuse(300, 300 * 957, 40, 8, true);
  if (g_fail) { printf("fuse_sim3 block: %d failures\n", g_fail); return 1; }
  printf("fuse_sim3 block ok\n");
  return 0;
}
