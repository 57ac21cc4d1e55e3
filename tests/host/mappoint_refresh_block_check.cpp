// mappoint_refresh_block_check.cpp — MapPointRefreshBlock of csrc/stage_blocks.h and the lines of csrc/mappoint_math.h on the CPU
// (tests/test_mappoint_refresh_block_cpu.py builds this with -fsanitize=address,undefined).  The block: every segment's offset against the segments in front of it,
// the two copied ranges, and every segment filled (or read) to its declared length in a malloc'd block of exactly pin_bytes().  The lines: mpm_select against a
// literal sort on every row of up to six distances over {0, 1, 255, 256} at every rank, the median rank, the first-minimum key, the host evaluator on rows whose
// answer is certain.
#include <algorithm>
#include "block_check.h"

static void block(size_t K, size_t P, size_t M, size_t L, bool nd, bool want_desc) {
  MapPointRefreshBlock b(K, P, M, L, nd, want_desc);
  Check c(b);
  c.up(b.kf_center, nd ? 3 * K : 0, true);
  c.up(b.obs_off, P + 1, true); c.up(b.obs_row, M, false); c.up(b.obs_kf, nd ? M : 0, true);
  c.up(b.pos, nd ? 3 * P : 0, true);
  c.up(b.ref_row, P, false); c.up(b.ref_kf, nd ? P : 0, true);
  c.up(b.scale_factors, L, true);
  c.up(b.order, P, false);
  const size_t n_in = 4 * ((nd ? 3 * K : 0) + P + 1 + M + (nd ? M : 0) + (nd ? 3 * P : 0) + P + (nd ? P : 0) + L + P);
  EXPECT_EQ(c.o, n_in);
  // the seeded outputs: uploaded with the caller's values and downloaded; they start the download on 16 bytes
  const size_t out0 = (n_in + 15) & ~(size_t)15, n_seed = nd ? 4 * 5 * P : 0;
  c.up(b.normal, nd ? 3 * P : 0, true, 16); c.up(b.dmin, nd ? P : 0, true); c.up(b.dmax, nd ? P : 0, true);
  EXPECT_EQ(b.normal.off, out0);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), out0 + n_seed);
  c.uploaded_bytes();
  { std::vector<float> dst(3 * P + 1); b.get(b.normal, dst.data()); b.get(b.dmin, dst.data()); b.get(b.dmax, dst.data()); }
  c.down(b.best_obs, P); c.down(b.status, P);
  c.seg(b.best_desc, want_desc ? 32 * P : 0, 16);
  EXPECT((b.best_desc.off - b.down_begin()) % 16 == 0 && b.best_desc.off % 16 == 0);   // 16-byte stores on the device, and the pinned side starts at 0
  { std::vector<uint8_t> dst(32 * P + 1); b.get(b.best_desc, dst.data()); }
  EXPECT(b.best_desc.off + b.best_desc.count <= b.down_begin() + b.down_bytes());
  EXPECT_EQ(b.down_begin(), out0);
  EXPECT_EQ(b.down_bytes(), c.o - out0);
  EXPECT_EQ(b.bytes(), c.o);
  EXPECT_EQ(b.best_desc.off, (out0 + n_seed + 4 * P + words(P) + 15) & ~(size_t)15);   // the status bytes are padded to whole words
  EXPECT_EQ(b.pin_bytes(), std::max(b.up_bytes(), b.down_bytes()));
}

static void median_rule() {
  const int values[4] = {0, 1, 255, 256};
  long checked = 0;
  for (int len = 1; len <= 6; len++) {
    int total = 1;
    for (int i = 0; i < len; i++) total *= 4;
    for (int code = 0; code < total; code++) {
      int row[6], sorted[6];
      for (int i = 0, c = code; i < len; i++, c /= 4) sorted[i] = row[i] = values[c % 4];
      std::sort(sorted, sorted + len);
      const auto count_le = [&](int v) { int c = 0; for (int i = 0; i < len; i++) c += row[i] <= v; return c; };
      for (int rank = 0; rank < len; rank++) { EXPECT(mpm_select(rank, count_le) == sorted[rank]); checked++; }
      EXPECT(mpm_select(mpm_median_rank(len), count_le) == sorted[(int)(0.5 * (len - 1))]);
    }
  }
  EXPECT(checked > 20000);
  // every value 0 .. 256 alone, and beside entries that are no observation
  for (int v = 0; v <= 256; v++) {
    EXPECT(mpm_select(0, [&](int x) { return (int)(v <= x); }) == v);
    EXPECT(mpm_select(0, [&](int x) { return (int)(v <= x) + (int)(MPM_NO_DIST <= x); }) == v);
  }
  const int ranks[9] = {0, 0, 1, 1, 2, 2, 3, 3, 4};
  for (int N = 1; N <= 9; N++) EXPECT(mpm_median_rank(N) == ranks[N - 1]);
  EXPECT(mpm_median_rank(256) == 127 && mpm_median_rank(65) == 32 && mpm_median_rank(64) == 31);
  // the first minimum: an equal median at a later index is the larger key; a median of 256 stays below the no-key value
  EXPECT(mpm_key(5, 3) < mpm_key(5, 4) && mpm_key(5, 255) < mpm_key(6, 0) && mpm_key(256, 255) < MPM_NO_KEY && mpm_key_index(mpm_key(256, 255)) == 255);
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ones[8] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u}, one[8] = {0, 0, 0, 0x100, 0, 0, 0, 0};
  EXPECT(mpm_hamming(zero, ones) == 256 && mpm_hamming(zero, zero) == 0 && mpm_hamming(zero, one) == 1 && mpm_hamming(ones, one) == 255);
}

static void evaluator() {
  // one keyframe of four features: 0 and 1 complementary, 2 one bit from 0, 3 = 2; octaves 0, 1, 7, 9
  uint8_t desc[4 * 32];
  memset(desc, 0, sizeof desc); memset(desc + 32, 0xff, 32); desc[64] = 1; desc[96] = 1;
  const uint8_t oct[4] = {0, 1, 7, 9};
  const MpmKf kf[2] = {{4, desc, oct}, {4, desc, oct}};   // two keys on the same arrays
  const float centre[6] = {0, 0, 0, 0, 0, 5}, pos[3] = {0, 0, 4}, sf[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  const int32_t okf[4] = {0, 0, 0, 0};
  int32_t best; uint8_t status, bd[32]; float nrm[3], dmin, dmax;
  const auto run = [&](int N, const int32_t* feat, int ref_kf, int ref_feat) {
    memset(bd, 0xa5, 32); nrm[0] = nrm[1] = nrm[2] = -7.f; dmin = dmax = -7.f;
    mpm_point_host(kf, centre, N, okf, feat, pos, ref_kf, ref_feat, 8, sf, &best, bd, nrm, &dmin, &dmax, &status);
  };
  const int32_t pair[2] = {1, 0}, three[3] = {1, 2, 3}, four[4] = {1, 0, 2, 3};
  run(0, pair, 0, 0);   // empty: everything stays
  EXPECT(best == -1 && status == 0 && bd[0] == 0xa5 && nrm[0] == -7.f && dmin == -7.f && dmax == -7.f);
  run(2, pair, -1, 0);   // rank 0: both medians are the self-distance, index 0 wins; no normal / depth part
  EXPECT(best == 0 && status == MPM_DESC && bd[0] == 0xff && nrm[0] == -7.f && dmax == -7.f);
  run(3, three, 0, 1);   // rows {0,255,255}, {255,0,0}, {255,0,0}: medians 255, 0, 0 -> index 1; both observers 4 below the point: normal (0, 0, 1), level 1
  EXPECT(best == 1 && status == (MPM_DESC | MPM_NORMAL_DEPTH) && bd[0] == 1 && nrm[0] == 0.f && nrm[1] == 0.f && nrm[2] == 1.f && dmax == 8.f && dmin == 1.f);
  run(4, four, 1, 2);   // rank 1; rows {0,256,255,255}, {256,0,1,1}, {255,1,0,0}, {255,1,0,0}: medians 255, 1, 0, 0 -> index 2; reference centre 1 below: dist 1, level 7
  EXPECT(best == 2 && status == (MPM_DESC | MPM_NORMAL_DEPTH) && dmax == 8.f && dmin == 1.f);
  run(4, four, 0, 3);   // the reference feature's octave 9 is beyond the 8 levels: the values stay
  EXPECT(best == 2 && status == (MPM_DESC | MPM_OCTAVE_BEYOND) && nrm[2] == -7.f && dmin == -7.f && dmax == -7.f);
  // the argument rules
  bool any = false;
  const int64_t keys[1] = {5};
  const int32_t off[2] = {0, 2}, bad_off[2] = {1, 2}, ref[1] = {0}, rf[1] = {0};
  int32_t bo[1]; uint8_t st[1]; float n3[3], d1[1], d2[1];
#define ARGS(K, P, OFF, OKF, NL) mpm_check_args(K, keys, centre, P, OFF, OKF, pair, pos, ref, rf, NL, sf, bo, n3, d1, d2, st, &any)
  EXPECT(ARGS(1, 1, off, okf, 8) == nullptr && any);
  EXPECT(ARGS(1, 1, bad_off, okf, 8) != nullptr && ARGS(1, 1, off, okf, 0) != nullptr && ARGS(1, 1, off, okf, 257) != nullptr && ARGS(0, 1, off, okf, 8) != nullptr);
  EXPECT(ARGS(1, 1, off, pair, 8) != nullptr);   // obs_kf = 1 with K = 1
  EXPECT(ARGS(1, 0, nullptr, nullptr, 8) == nullptr && !any);
#undef ARGS
  const int32_t n_feat[1] = {4}, f_ok[2] = {3, 0}, f_bad[2] = {4, 0}, rf_bad[1] = {4};
  EXPECT(mpm_check_features(n_feat, 1, off, okf, f_ok, ref, rf) == nullptr && mpm_check_features(n_feat, 1, off, okf, f_bad, ref, rf) != nullptr &&
         mpm_check_features(n_feat, 1, off, okf, f_ok, ref, rf_bad) != nullptr);
}

int main() {
  for (bool nd : {false, true})
    for (bool want : {false, true}) {
      block(0, 1, 0, 1, nd, want); block(1, 1, 1, 1, nd, want); block(3, 2, 5, 8, nd, want); block(21, 1000, 2000, 8, nd, want); block(8, 37, 1003, 7, nd, want);
      for (size_t P : {1, 3, 63, 64, 65, 257}) block(5, P, 3 * P + 1, 8, nd, want);   // status lengths that are no multiple of four
    }
  median_rule();
  evaluator();
  if (g_fail) { printf("mappoint_refresh block: %d failures\n", g_fail); return 1; }
  printf("mappoint_refresh block ok\n");
  return 0;
}
