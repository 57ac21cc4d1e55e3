// bow_search_block_check.cpp — BowPairResidentBlock of csrc/stage_blocks.h and the lines of csrc/bow_search_math.h on the CPU (tests/test_bow_search_block_cpu.py
// builds this with -fsanitize=address,undefined).  The block: every segment's offset against the segments in front of it, the two copied ranges, and every segment
// filled (or read) to its declared length in a malloc'd block of exactly pin_bytes().  The lines: bsm_update and bsm_merge against the sequential loop on every list
// of up to five distances over {0, 1, 2, 256} and every split point, and the word packing round trip.
#include "block_check.h"

static void block(size_t J, size_t M1, size_t M2) {
  BowPairResidentBlock b(J, M1, M2);
  Check c(b);
  c.up(b.job, BSM_JOB_INTS * J, false, 16);
  c.up(b.live1, M1, true); c.up(b.live2, M2, true);
  const size_t n_in = 4 * BSM_JOB_INTS * J + words(M1) + words(M2);
  EXPECT_EQ(c.o, n_in);
  c.zero_and_down(b.table, M1); c.zero_and_down(b.n_query, J); c.zero_and_down(b.n_dist, J);
  const size_t t0 = (n_in + 7) & ~(size_t)7, n_out = 8 * M1 + 8 * J;
  EXPECT_EQ(b.table.off, t0);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), t0 + n_out);
  c.uploaded_bytes();
  EXPECT_EQ(b.down_begin(), t0); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), t0 + n_out);
  EXPECT_EQ(b.pin_bytes(), t0 + n_out);
  EXPECT(b.table.off % 8 == 0 && (size_t)((const char*)b.down(b.table) - (const char*)b.host()) % 8 == 0);   // the 64-bit words lie on 8 bytes on both sides
}

// the sequential loop of ORBmatcher.cpp:613-639 on a list of (distance, index)
static BowBest sequential(const int* dist, int i0, int i1) {
  int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
  for (int i = i0; i < i1; i++) {
    if (dist[i] < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist[i]; bestIdx2 = 100 + i; }
    else if (dist[i] < bestDist2) bestDist2 = dist[i];
  }
  return BowBest{bestDist1, bestIdx2, bestDist2};
}
static bool same(const BowBest& a, const BowBest& b) { return a.d1 == b.d1 && a.idx == b.idx && a.d2 == b.d2; }

static void lines() {
  const int values[4] = {0, 1, 2, 256};
  long checked = 0;
  for (int len = 0; len <= 5; len++) {
    int total = 1;
    for (int i = 0; i < len; i++) total *= 4;
    for (int code = 0; code < total; code++) {
      int dist[5] = {0, 0, 0, 0, 0};
      for (int i = 0, c = code; i < len; i++, c /= 4) dist[i] = values[c % 4];
      const BowBest want = sequential(dist, 0, len);
      BowBest upd = bsm_empty();
      for (int i = 0; i < len; i++) bsm_update(upd, dist[i], 100 + i);
      EXPECT(same(upd, want));
      for (int split = 0; split <= len; split++) {
        EXPECT(same(bsm_merge(sequential(dist, 0, split), sequential(dist, split, len)), want));
        for (int split2 = split; split2 <= len; split2++)   // three parts, merged in order
          EXPECT(same(bsm_merge(bsm_merge(sequential(dist, 0, split), sequential(dist, split, split2)), sequential(dist, split2, len)), want));
        checked++;
      }
    }
  }
  EXPECT(checked > 5000);
  // the properties by name: the first index of the minimum, the second smallest as a multiset, the empty sides
  const int five[2] = {5, 5};
  EXPECT(same(sequential(five, 0, 2), BowBest{5, 100, 5}));
  EXPECT(same(bsm_merge(sequential(five, 0, 1), sequential(five, 1, 2)), BowBest{5, 100, 5}));
  EXPECT(same(bsm_merge(bsm_empty(), bsm_empty()), BowBest{256, -1, 256}));
  EXPECT(same(bsm_merge(bsm_empty(), sequential(five, 0, 1)), BowBest{5, 100, 256}));
  EXPECT(same(bsm_merge(sequential(five, 0, 1), bsm_empty()), BowBest{5, 100, 256}));
}

static void packing() {
  EXPECT(bsm_pack(BSM_NOT_A_QUERY, BowBest{7, 9, 11}, 3) == 0);
  const int idxs[] = {-1, 0, 1, 255, 256, 32767, 32768, 65534}, dists[] = {0, 1, 49, 50, 255, 256}, nodes[] = {0, 1, 99, 65534};
  for (int status : {BSM_NO_CANDIDATE, BSM_EVALUATED})
    for (int idx : idxs)
      for (int d1 : dists)
        for (int d2 : dists)
          for (int node : nodes) {
            const uint64_t w = bsm_pack(status, BowBest{d1, idx, d2}, node);
            EXPECT(w != 0 && bsm_status(w) == status && same(bsm_best(w), BowBest{d1, idx, d2}) && bsm_node2(w) == node);
          }
  // the argument rules on arrays of exactly the documented lengths
  const int32_t node[3] = {3, 5, 9}, off[4] = {0, 3, 7, 10}, idx[10] = {0, 1, 8, 2, 3, 4, 10, 5, 6, 9};
  uint8_t seen[12];
  EXPECT(bsm_check_featvec(12, 3, node, off, idx, seen) == nullptr);
  EXPECT(bsm_check_featvec(11, 3, node, off, idx, seen) == nullptr);
  EXPECT(bsm_check_featvec(10, 3, node, off, idx, seen) != nullptr);    // index 10 is outside 10 features
  EXPECT(bsm_check_featvec(12, 0, nullptr, nullptr, nullptr, seen) == nullptr);
  EXPECT(bsm_check_featvec(9, 3, node, off, idx, seen) != nullptr);     // more entries than features: refused before any index is read
  EXPECT(bsm_find_node(node, 3, 3) == 0 && bsm_find_node(node, 3, 9) == 2 && bsm_find_node(node, 3, 4) == -1 && bsm_find_node(node, 3, 1) == -1 &&
         bsm_find_node(node, 3, 10) == -1 && bsm_find_node(node, 0, 3) == -1);
}

int main() {
  block(1, 0, 0); block(1, 1, 1); block(1, 3, 5); block(2, 7, 1000); block(3, 3 * 1001, 1001 + 999 + 2);
  for (size_t J : {1, 2, 8})
    for (size_t n : {1, 63, 64, 65, 257, 1000, 2001}) block(J, J * n, J * n - (J > 1));   // mask lengths that are no multiple of four or eight
  lines();
  packing();
  if (g_fail) { printf("bow_search block: %d failures\n", g_fail); return 1; }
  printf("bow_search block ok\n");
  return 0;
}
