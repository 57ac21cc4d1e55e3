// fuse_pose_block_check.cpp — FusePoseBlock of csrc/stage_blocks.h on the CPU (tests/test_fuse_pose_block_cpu.py builds this with -fsanitize=address,undefined).
// Every segment's offset against the segments in front of it, the two copied ranges, every segment filled (or read) to its declared length in a malloc'd block of
// exactly pin_bytes(), and the job / tile tables written from a job list as ccm_fuse_pose_eval writes them, so that an overrun is the sanitizer's to report.
#include "block_check.h"

static size_t up16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// K keyframes with F features, P points, L levels and the job list (kf, pt0, n); sizes from fpm_check_jobs as the stage takes them
static void fuse(size_t K, size_t F, size_t P, size_t L, const std::vector<int32_t>& kf, const std::vector<int32_t>& p0, const std::vector<int32_t>& n, bool uv) {
  const int J = (int)kf.size();
  int64_t total = 0, tiles = 0;
  const char* why = fpm_check_jobs(J, (int)K, (int)P, kf.data(), p0.data(), n.data(), &total, &tiles);
  EXPECT(why == nullptr);
  if (why) return;
  const size_t N = (size_t)total, T = (size_t)tiles;
  FusePoseBlock b(K, F, P, L, (size_t)J, T, N, uv);
  Check c(b);
  c.up(b.kdesc, 32 * F, true, 16); c.up(b.pdesc, 32 * P, true, 16);
  c.seg(b.job, FPM_JOB_INTS * (size_t)J, 16); c.seg(b.tile, 2 * T, 0);
  {   // the two tables as the stage writes them: within their segments, one tile per 256 pairs of a job, every pair in exactly one tile
    int32_t* hj = b.up(b.job); int32_t* ht = b.up(b.tile);
    int32_t out0 = 0; size_t t = 0;
    for (int j = 0; j < J; j++) {
      hj[4 * j] = kf[j]; hj[4 * j + 1] = p0[j]; hj[4 * j + 2] = n[j]; hj[4 * j + 3] = out0;
      for (int32_t e = 0; e < n[j]; e += FPM_TILE, t++) { EXPECT(t < T); if (t < T) { ht[2 * t] = j; ht[2 * t + 1] = e; } }
      out0 += n[j];
    }
    EXPECT_EQ(t, T); EXPECT_EQ((size_t)out0, N);
    std::vector<char> seen(N, 0);
    for (size_t i = 0; i < T; i++) {
      const int j = ht[2 * i], e0 = ht[2 * i + 1];
      EXPECT(j >= 0 && j < J && e0 >= 0 && e0 < hj[4 * j + 2] && hj[4 * j] < (int32_t)K);
      for (int e = e0; e < e0 + FPM_TILE && e < hj[4 * j + 2]; e++) {
        const size_t o = (size_t)hj[4 * j + 3] + (size_t)e;
        EXPECT(o < N && (size_t)hj[4 * j + 1] + (size_t)e < P);
        if (o < N) { EXPECT(!seen[o]); seen[o] = 1; }
      }
    }
    for (size_t i = 0; i < N; i++) if (!seen[i]) { printf("FAIL: pair %zu is in no tile\n", i); g_fail++; break; }
    memset(hj, 0xff, 16 * (size_t)J); memset(ht, 0xff, 8 * T);
    for (size_t i = 0; i < 16 * (size_t)J; i++) c.filled[b.job.off - b.up_begin() + i] = 1;
    for (size_t i = 0; i < 8 * T; i++) c.filled[b.tile.off - b.up_begin() + i] = 1;
  }
  c.up(b.rec, FSM_REC_FLOATS * K, true); c.up(b.pose, FSM_POSE_FLOATS * K, true);
  c.up(b.feat_off, K + 1, true); c.up(b.cell_off, K * (FSM_CELLS + 1), true);
  c.up(b.kxy, 2 * F, true); c.up(b.cell_idx, F, false); c.up(b.koct, F, true);
  c.up(b.scale_factors, L, true); c.up(b.inv_sigma2, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.normal, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  const size_t n_in = up16(32 * F + 32 * P) + 16 * (size_t)J + 8 * T + 4 * (25 * K + K + 1 + K * (FSM_CELLS + 1) + 2 * F + 2 * L + 8 * P) + words(2 * F) + words(F);
  EXPECT_EQ(c.o, n_in);
  c.zero_and_down(b.n_valid, (size_t)J); c.zero_and_down(b.n_hit, (size_t)J);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in + 8 * (size_t)J);
  c.uploaded_bytes();
  c.down(b.table, N); c.down(b.uv, uv ? 2 * N : 0);
  const size_t n_out = 8 * (size_t)J + 4 * N + (uv ? 8 * N : 0);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in + 8 * (size_t)J > n_out ? n_in + 8 * (size_t)J : n_out);
}

int main() {
  typedef std::vector<int32_t> V;
  for (int uv = 0; uv < 2; uv++) {
    fuse(0, 0, 0, 8, V{}, V{}, V{}, uv); fuse(0, 0, 7, 8, V{}, V{}, V{}, uv); fuse(1, 957, 41, 8, V{}, V{}, V{}, uv);
    fuse(1, 957, 41, 8, V{0}, V{40}, V{1}, uv);                               // J = 1, n = 1
    fuse(1, 0, 32, 8, V{0}, V{0}, V{32}, uv);                                  // a keyframe without features
    fuse(2, 1914, 300, 8, V{0, 1, 1}, V{40, 5, 100}, V{70, 0, 130}, uv);       // an empty job between two others
    fuse(2, 1914, 300, 8, V{1}, V{300}, V{0}, uv); fuse(1, 957, 0, 1, V{0}, V{0}, V{0}, uv);
    for (int J : {1, 2, 3})
      for (int n : {63, 64, 65, 255, 256, 257}) fuse(9, 9 * 957, 7500, J == 3 ? 16 : 8, V(J, J - 1), V(J, 40), V(J, n), uv);
    fuse(9, 9 * 957, 7500, 8, V{2, 0, 1, 0, 2}, V{50, 40, 0, 200, 100}, V{1, 257, 0, 64, 300}, uv);
    fuse(9, 9 * 957, 7500, 8, V{5, 5, 5, 1}, V{0, 0, 300, 0}, V{700, 700, 700, 10}, uv);
    {   // the SearchInNeighbors shape: 12 jobs x 2 500 points on 8 keyframes and 1 job x 6 000 points
      V kf{0, 1, 5, 6, 1, 5, 2, 7, 3, 3, 4, 6, 8}, p0(13, 0), n(13, 2500);
      p0[12] = 1500; n[12] = 6000;
      fuse(9, 9 * 957, 7500, 8, kf, p0, n, uv);
    }
    {   // 300 jobs x 40 points
      V kf, p0, n;
      for (int j = 0; j < 300; j++) { kf.push_back(j % 9); p0.push_back(30 + 7 * j); n.push_back(40); }
      fuse(9, 9 * 957, 7500, 8, kf, p0, n, uv);
    }
    fuse(23, 40, 32, 8, V{0, 22}, V{0, 0}, V{32, 32}, uv);                     // the planted scene's sizes
  }
  if (g_fail) { printf("fuse_pose block: %d failures\n", g_fail); return 1; }
  printf("fuse_pose block ok\n");
  return 0;
}
