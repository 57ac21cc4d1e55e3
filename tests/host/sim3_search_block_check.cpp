// sim3_search_block_check.cpp — Sim3ProjectResidentBlock and Sim3PairResidentBlock of csrc/stage_blocks.h on the CPU (tests/test_sim3_search_block_cpu.py builds this
// with -fsanitize=address,undefined).  Every segment's offset against the segments in front of it, the two copied ranges, and every segment filled (or read) to its
// declared length in a malloc'd block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include "block_check.h"

static void project(size_t K, size_t P, size_t L, size_t M, bool uv) {
  Sim3ProjectResidentBlock b(K, P, L, M, uv);
  Check c(b);
  c.up(b.pdesc, 32 * P, true, 16);
  c.up(b.slot, K, false); c.up(b.skip_off, K + 1, true);
  c.up(b.pose, FSM_POSE_FLOATS * K, false); c.up(b.scale_factors, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.normal, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  c.up(b.skip, M, true);
  const size_t n_in = 32 * P + 4 * (K + K + 1 + FSM_POSE_FLOATS * K + L + 8 * P) + words(M);
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

static void pair(size_t K, size_t P, size_t L, size_t J, size_t T, size_t N, bool uv) {
  Sim3PairResidentBlock b(K, P, L, J, T, N, uv);
  Check c(b);
  c.up(b.pdesc, 32 * P, true, 16);
  c.up(b.job, FPM_JOB_INTS * J, false, 16); c.up(b.tile, 2 * T, false); c.up(b.slot, K, false);
  c.up(b.pose, SSM_JOB_FLOATS * J, false); c.up(b.scale_factors, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  const size_t n_in = 32 * P + 4 * (FPM_JOB_INTS * J + 2 * T + K + SSM_JOB_FLOATS * J + L + 5 * P);
  EXPECT_EQ(c.o, n_in);
  c.zero_and_down(b.n_valid, J); c.zero_and_down(b.n_hit, J);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in + 8 * J);
  c.uploaded_bytes();
  c.down(b.table, N); c.down(b.uv, uv ? 2 * N : 0);
  const size_t n_out = 8 * J + 4 * N + (uv ? 8 * N : 0);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in + 8 * J > n_out ? n_in + 8 * J : n_out);
}

int main() {
  for (int uv = 0; uv < 2; uv++) {
    project(1, 1, 8, 0, uv);                                    // a keyframe without features
    for (size_t K : {1, 2, 7})
      for (size_t P : {1, 63, 64, 65, 255, 256, 257, 2500})
        for (size_t M : {1, 2, 3, 70, 300, 1001}) project(K, P, K == 2 ? 16 : 8, K * M - (K > 1), uv);   // mask lengths that are no multiple of 4
    pair(2, 1, 8, 1, 1, 1, uv);
    for (size_t P : {1, 63, 64, 65, 255, 256, 257, 1600}) {
      pair(2, P, 8, 2, 2 * ((P + FPM_TILE - 1) / FPM_TILE), 2 * P, uv);                 // two jobs on all points (overlapping ranges)
      pair(2, P, 8, 3, (P + FPM_TILE - 1) / FPM_TILE, P, uv);                           // an empty job among three
      pair(1, P, 1, 2, (P / 2 + FPM_TILE - 1) / FPM_TILE + (P - P / 2 + FPM_TILE - 1) / FPM_TILE, P, uv);
    }
  }
  if (g_fail) { printf("sim3_search blocks: %d failures\n", g_fail); return 1; }
  printf("sim3_search blocks ok\n");
  return 0;
}
