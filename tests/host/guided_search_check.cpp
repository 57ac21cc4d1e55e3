// guided_search_check.cpp — the host side of ccm_frame_guided_search on the CPU (tests/test_guided_search_cpu.py builds this with -fsanitize=address,undefined):
// GuidedSearchBlock of csrc/stage_blocks.h (every segment's offset, the two copied ranges, every segment filled or read to its declared length in a malloc'd block of
// exactly pin_bytes()), csrc/guided_search_math.h on planted points, and the sequential pass of host/guided_replay.h on planted lists in exactly-sized arrays.
#include "block_check.h"
#include "guided_search_math.h"
#include "../host/guided_replay.h"
#include <limits>

static void block(size_t P, size_t cap) {
  GuidedSearchBlock b(P, cap);
  Check c(b);
  c.up(b.desc, 32 * P, true, 16); c.up(b.pos, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true); c.up(b.skip, P, false);
  const size_t n_in = 32 * P + 20 * P + words(P);
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in);
  c.uploaded_bytes();
  c.seg(b.radius, P, 0); c.seg(b.minl, P, 0); c.seg(b.maxl, P, 0); c.seg(b.cnt, P, 0);
  const size_t out_at = n_in + 16 * P;
  c.down(b.u, P); c.down(b.v, P); c.down(b.level, P); c.down(b.cand_off, P + 1); c.down(b.status, P); c.down(b.cand_idx, cap); c.down(b.cand_dist, cap);
  EXPECT_EQ(b.u.off, out_at); EXPECT_EQ(b.desc.off % 16, 0);
  EXPECT_EQ(b.down_begin(), out_at); EXPECT_EQ(b.down_bytes(), 12 * P + 4 * (P + 1) + words(P) + 4 * cap + words(2 * cap));
  EXPECT_EQ(b.bytes(), out_at + b.down_bytes());
}

static void header() {
  const float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  float pose[GSM_POSE_FLOATS];
  gsm_pose(T, pose);
  for (int i = 12; i < 15; i++) EXPECT(pose[i] == 0.0f);
  const float Tt[12] = {0, -1, 0, 1, 1, 0, 0, 2, 0, 0, 1, 3};   // Ow = -R^T t = (-2, 1, -3)
  gsm_pose(Tt, pose);
  EXPECT(pose[12] == -2.0f && pose[13] == 1.0f && pose[14] == -3.0f);
  gsm_pose(T, pose);
  const float K[4] = {512, 512, 320, 240};
  float sf[FSM_MAX_LEVELS];
  sf[0] = 1.0f;
  for (int i = 1; i < FSM_MAX_LEVELS; i++) sf[i] = sf[i - 1] * 1.2f;
  const float logsf = logf(1.2f);
  float u, v, r; int l;
  auto gate = [&](float x, float y, float z, float dmin, float dmax, int nlevels) { const float P[3] = {x, y, z}; return gsm_gate(pose, K, 0, 640, 0, 480, P, dmin, dmax, logsf, nlevels, sf, 10.0f, u, v, l, r); };
  EXPECT(gate(-0.625f, 0, 1, 0.1f, 1.0f, 8) == GSM_SEARCHED && u == 0.0f && v == 240.0f && l == 0 && r == 10.0f);
  EXPECT(gate(nextafterf(-0.625f, -1.0f), 0, 1, 0.1f, 1.0f, 8) == GSM_OUTSIDE && u < 0.0f && r == -1.0f);
  EXPECT(gate(0.625f, 0, 1, 0.1f, 1.0f, 8) == GSM_SEARCHED && u == 640.0f);
  EXPECT(gate(0, 0, 4, 0.1f, 3.0f, 8) == GSM_RANGE);
  EXPECT(gate(0, 0, 4, 0.1f, 4.0f * 9.0f, 8) == GSM_SEARCHED && l == 7 && r == 10.0f * sf[7]);
  EXPECT(gate(0, 0, 4, 0.1f, 4.0f * 9.0f, 1) == GSM_SEARCHED && l == 0);
  EXPECT(gate(0, 0, 4, 0.1f, 4.0f * 1e9f, 16) == GSM_SEARCHED && l == 15 && r == 10.0f * sf[15]);
  EXPECT(gate(0, 0, -4, 0.1f, 4.0f, 8) == GSM_SEARCHED && u == 320.0f);                       // behind the camera, inside the image
  EXPECT(gate(1, 1, 0, 0.1f, 4.0f, 8) == GSM_OUTSIDE && std::isinf(u));
  EXPECT(gate(0, 0, 0, 0.0f, 4.0f, 8) == GSM_SEARCHED && u != u && v != v && l == 0);          // 0 * inf
  EXPECT(gate(0, 0, 0, 1.0f, 4.0f, 8) == GSM_RANGE);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  EXPECT(gate(nan, 0, 1, 0.0f, 4.0f, 8) == GSM_RANGE || l == 0);                                // whatever the status, the level stays inside the table
  for (float dmax : {nan, inf, -1.0f, 0.0f, 1e-44f})
    for (float z : {4.0f, 1e-30f, 1e30f}) { gate(0, 0, z, 0.0f, dmax, 8); EXPECT(l >= 0 && l < 8); }
}

static void replay() {
  // four slots, five features, in arrays of exactly the lists' sizes
  {
    std::vector<int32_t> off{0, 2, 4, 4, 5}, idx{1, 0, 0, 1, 4};
    std::vector<uint16_t> dist{6, 6, 2, 30, 255};
    std::vector<float> ka{10, 10, 0, 900}, fa{350, 350, 0, 0, 0};
    std::vector<int32_t> mp(5, -1);
    auto angle = [&](int i2) { return fa[i2]; };
    EXPECT(ccm_guided::replay(4, off.data(), idx.data(), dist.data(), ka.data(), angle, 5, mp.data(), 255, false) == 3);
    EXPECT(mp[1] == 0 && mp[0] == 1 && mp[4] == 3 && mp[2] == -1 && mp[3] == -1);              // the tie goes to the first in the list; slot 1 takes what is left
    mp.assign(5, -1);
    EXPECT(ccm_guided::replay(4, off.data(), idx.data(), dist.data(), ka.data(), angle, 5, mp.data(), 254, true) == 2 && mp[4] == -1);   // 255 > ORBdist
    mp.assign(5, -1);
    EXPECT(ccm_guided::replay(4, off.data(), idx.data(), dist.data(), ka.data(), angle, 5, mp.data(), 255, true) == 3);   // bins 1 (wrapped), 1, 0 (from 30)
    mp.assign(5, 7);
    EXPECT(ccm_guided::replay(4, off.data(), idx.data(), dist.data(), ka.data(), angle, 5, mp.data(), 255, true) == 0);   // every candidate claimed
    for (int bad : {-1, 256}) {
      bool thrown = false;
      try { ccm_guided::replay(4, off.data(), idx.data(), dist.data(), ka.data(), angle, 5, mp.data(), bad, true); } catch (const std::invalid_argument&) { thrown = true; }
      EXPECT(thrown);
    }
  }
  EXPECT(ccm_guided::histBin(-340.0f) == 1 && ccm_guided::histBin(900.0f) == 0 && ccm_guided::histBin(359.0f) == 12 && ccm_guided::histBin(0.0f) == 0);
  {   // an angle difference beyond the histogram is refused, not written
    ccm_guided::RotationFilter f;
    bool thrown = false;
    try { f.add(915.0f, 0); } catch (const std::invalid_argument&) { thrown = true; }
    EXPECT(thrown && ccm_guided::histBin(915.0f) == 31);
    f.add(914.0f, 0);
    EXPECT(f.hist[0].size() == 1);
  }
  {   // no slots, no features
    std::vector<int32_t> off{0};
    EXPECT(ccm_guided::replay(0, off.data(), nullptr, nullptr, nullptr, [](int) { return 0.0f; }, 0, nullptr, 100, true) == 0);
  }
}

int main() {
  for (size_t P : {0, 1, 7, 8, 9, 255, 256, 257, 1000})
    for (size_t cap : {0, 1, 2, 3, 1000}) block(P, cap);
  header();
  replay();
  if (g_fail) { printf("guided search: %d failures\n", g_fail); return 1; }
  printf("guided search ok\n");
  return 0;
}
