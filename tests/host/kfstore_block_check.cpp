// kfstore_block_check.cpp — KfstoreAddBlock, FuseSim3ResidentBlock and FusePoseResidentBlock of csrc/stage_blocks.h and the host side of csrc/kfstore_math.h on the
// CPU (tests/test_kfstore_block_cpu.py builds this with -fsanitize=address,undefined).  Every segment's offset against the segments in front of it, the two copied ranges, and every segment filled (or read) to
// its declared length in a malloc'd block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include "block_check.h"
#include <math.h>

static void add(size_t M, size_t F, bool grid) {
  KfstoreAddBlock b(M, F, grid);
  Check c(b);
  c.up(b.desc, 32 * F, true, 16);
  c.up(b.slot, M, false); c.up(b.feat_off, M + 1, true);
  c.up(b.rec, FSM_REC_FLOATS * M, true); c.up(b.xy, 2 * F, true);
  c.up(b.cell_off, grid ? M * (FSM_CELLS + 1) : 0, true); c.up(b.cell_idx, grid ? F : 0, false);
  c.up(b.oct, F, true);
  const size_t n_in = 32 * F + 4 * (M + M + 1 + 10 * M + 2 * F + (grid ? M * (FSM_CELLS + 1) : 0)) + (grid ? words(2 * F) : 0) + words(F);
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in);
  c.uploaded_bytes();
  c.down(b.n_in, M);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), 4 * M);
  EXPECT_EQ(b.bytes(), n_in + 4 * M);
  EXPECT_EQ(b.pin_bytes(), n_in > 4 * M ? n_in : 4 * M);
}

static void sim3(size_t K, size_t P, size_t L, bool uv) {
  FuseSim3ResidentBlock b(K, P, L, uv);
  Check c(b);
  c.up(b.pdesc, 32 * P, true, 16);
  c.up(b.slot, K, false); c.up(b.pose, FSM_POSE_FLOATS * K, false); c.up(b.scale_factors, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.normal, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  const size_t n_in = 32 * P + 4 * (16 * K + L + 8 * P);
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

static void pose(size_t K, size_t P, size_t L, size_t J, size_t T, size_t N, bool uv) {
  FusePoseResidentBlock b(K, P, L, J, T, N, uv);
  Check c(b);
  c.up(b.pdesc, 32 * P, true, 16);
  c.up(b.job, FPM_JOB_INTS * J, false, 16); c.up(b.tile, 2 * T, false); c.up(b.slot, K, false);
  c.up(b.pose, FSM_POSE_FLOATS * K, true); c.up(b.scale_factors, L, true); c.up(b.inv_sigma2, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.normal, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  const size_t n_in = 32 * P + 4 * (4 * J + 2 * T + 16 * K + 2 * L + 8 * P);
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

// kfg_build_host and kfg_check_add of csrc/kfstore_math.h on arrays of exactly the documented lengths: n keypoints (some outside the grid, NaN, Inf and huge among
// them), cell_off of 3 601 and cell_idx of n entries.  The prefix ends at the features in the grid, every index appears once and ascends inside its cell.
static void grid(int n) {
  const float rec[FSM_REC_FLOATS] = {458.f, 457.f, 367.f, 248.f, -17.f, -9.f, 752.f, 480.f, 75.f / 769.f, 48.f / 489.f};
  float* xy = (float*)malloc(n ? 2 * n * sizeof(float) : 1);
  int32_t* off = (int32_t*)malloc((FSM_CELLS + 1) * sizeof(int32_t));
  uint16_t* idx = (uint16_t*)malloc(n ? n * sizeof(uint16_t) : 1);
  unsigned r = 12345u + (unsigned)n;
  for (int i = 0; i < 2 * n; i++) { r = r * 1664525u + 1013904223u; xy[i] = (float)(r >> 8) / 16777216.f * (i % 2 ? 560.f : 900.f) - (i % 2 ? 40.f : 60.f); }   // x in [-60, 840), y in [-40, 520): about 3 in 4 in the grid
  const float odd[6] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e10f};
  for (int i = 0; i < n && i < 12; i++) xy[(7 * i) % (2 * n)] = odd[i % 6];
  const int n_in = kfg_build_host(rec, n, xy, off, idx);
  EXPECT(off[0] == 0 && off[FSM_CELLS] == n_in && n_in <= n);
  EXPECT(n < 100 || (n_in > n / 2 && n_in < n));
  std::vector<char> seen(n ? n : 1, 0);
  for (int c = 0; c < FSM_CELLS; c++) {
    EXPECT(off[c + 1] >= off[c]);
    for (int p = off[c]; p < off[c + 1]; p++) {
      int cell = -1;
      EXPECT(idx[p] < n && !seen[idx[p]] && kfg_cell_of(rec, xy[2 * idx[p]], xy[2 * idx[p] + 1], &cell) && cell == c);
      EXPECT(p == off[c] || idx[p] > idx[p - 1]);
      seen[idx[p]] = 1;
    }
  }
  // the same grid handed back as a supplied one passes the argument rules, also when it ends below n; one index out of range does not
  const int32_t feat_off[2] = {0, n};
  std::vector<int32_t> idx32(n ? n : 1, 0);
  for (int p = 0; p < n_in; p++) idx32[p] = idx[p];
  const uint8_t* bytes = (const uint8_t*)xy;   // any non-null pointer: the rules read no feature array
  EXPECT(kfg_check_add(1, n ? n : 1, rec, feat_off, xy, bytes, bytes, off, idx32.data()) == nullptr);
  EXPECT(kfg_check_add(1, n ? n : 1, rec, feat_off, xy, bytes, bytes, nullptr, nullptr) == nullptr);
  EXPECT(kfg_check_add(1, n ? n : 1, rec, feat_off, xy, bytes, bytes, off, nullptr) != nullptr);
  if (n > 1) EXPECT(kfg_check_add(1, n - 1, rec, feat_off, xy, bytes, bytes, nullptr, nullptr) != nullptr);
  if (n_in) { idx32[n_in - 1] = n; EXPECT(kfg_check_add(1, n, rec, feat_off, xy, bytes, bytes, off, idx32.data()) != nullptr); }
  free(xy); free(off); free(idx);
}

int main() {
  for (int n : {0, 1, 2, 63, 64, 65, 257, 1000, 65535}) grid(n);
  for (int grid = 0; grid < 2; grid++) {
    add(1, 0, grid); add(1, 1, grid); add(2, 3, grid); add(3, 1001, grid); add(40, 40 * 333 - 7, grid); add(1, 65535, grid);
  }
  for (int uv = 0; uv < 2; uv++) {
    sim3(1, 1, 1, uv); sim3(300, 40, 8, uv);
    for (size_t K : {1, 2, 3, 8})
      for (size_t P : {1, 63, 64, 65, 257, 2500}) sim3(K, P, K == 3 ? 16 : 8, uv);
    pose(1, 1, 1, 1, 1, 1, uv); pose(9, 7500, 8, 4, 12, 2757, uv); pose(2, 30, 8, 3, 2, 257, uv); pose(9, 4800, 8, 13, 133, 32300, uv);
    for (size_t J : {1, 2, 5})
      for (size_t n : {1, 255, 256, 257}) pose(3, 300, 8, J, J * ((n + 255) / 256), J * n, uv);
  }
  if (g_fail) { printf("kfstore blocks: %d failures\n", g_fail); return 1; }
  printf("kfstore blocks ok\n");
  return 0;
}
