// bow_search_block_check.cpp — BowPairResidentBlock of csrc/stage_blocks.h and the lines of csrc/bow_search_math.h on the CPU (tests/test_bow_search_block_cpu.py
// builds this with -fsanitize=address,undefined).  The block: every segment's offset against the segments in front of it, the two copied ranges, and every segment
// filled (or read) to its declared length in a malloc'd block of exactly pin_bytes().  The lines: bsm_update and bsm_merge against the sequential loop on every list
// of up to five distances over {0, 1, 2, 256} and every split point, the word packing round trip, and the host walk over a keyframe pair's common nodes
// (fv_pair_walk_host, which tri_search_math.h's evaluator shares) on one pair with an absent node, a node without a query and a query without a candidate.
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

// One keyframe pair through the shared walk, on arrays of exactly the lengths the walk may read.  Keyframe 1: node 2 {0, 1} (keyframe 2 lacks it), node 5 {2} (not
// live: a node without a query), node 7 {3, 4} (keyframe 2's node 7 holds no live feature: queries without a candidate), node 9 {5}.  Keyframe 2: node 5 {4},
// node 7 {0, 1}, node 9 {2, 3} at distances 3 and 1 from feature 5 of keyframe 1.
static void walk() {
  const int32_t node1[4] = {2, 5, 7, 9}, off1[5] = {0, 2, 3, 5, 6}, node2[3] = {5, 7, 9}, off2[4] = {0, 1, 3, 5};
  const uint16_t idx1[6] = {0, 1, 2, 3, 4, 5}, idx2[5] = {4, 0, 1, 2, 3};
  std::vector<uint8_t> desc1(6 * 32, 0), desc2(5 * 32, 0xff);
  desc2[2 * 32] = 0x07; desc2[3 * 32] = 0x01;
  for (int k = 1; k < 32; k++) desc2[2 * 32 + k] = desc2[3 * 32 + k] = 0;
  const uint8_t live1[6] = {1, 1, 0, 1, 1, 1}, live2[5] = {0, 0, 1, 1, 1};
  const BowKf k1{6, 4, node1, off1, idx1, desc1.data()}, k2{5, 3, node2, off2, idx2, desc2.data()};
  // the walk alone: the words zeroed, then the queries of the common nodes in list order with their node's position in keyframe 2
  uint32_t seen[6] = {9, 9, 9, 9, 9, 9};
  std::vector<int> order;
  fv_pair_walk_host(k1, k2, live1, true, seen, [&](int idx1_, int b) { order.push_back(10 * idx1_ + b); return (uint32_t)(100 + idx1_); });
  EXPECT((order == std::vector<int>{31, 41, 52}));
  EXPECT(seen[0] == 0 && seen[1] == 0 && seen[2] == 0 && seen[3] == 103 && seen[4] == 104 && seen[5] == 105);
  order.clear();
  fv_pair_walk_host(k1, k2, live1, false, seen, [&](int idx1_, int b) { order.push_back(10 * idx1_ + b); return 7u; });   // the other sense of the mask: feature 2 alone
  EXPECT((order == std::vector<int>{20}) && seen[2] == 7 && seen[3] == 0 && seen[5] == 0);
  // the job evaluator on it.  By hand: no candidate = status 1, (256, -1, 256), node position 1; feature 5 = status 2, (1, feature 3, 3), node position 2
  uint64_t table[6] = {9, 9, 9, 9, 9, 9};
  int32_t n_query = -1, n_dist = -1;
  bow_job_eval_host(k1, k2, live1, live2, table, &n_query, &n_dist);
  EXPECT(table[0] == 0 && table[1] == 0 && table[2] == 0);
  EXPECT(table[3] == 0x4000000601000000ull && table[4] == 0x4000000601000000ull && table[5] == 0x8000000806010004ull);
  EXPECT(n_query == 3 && n_dist == 2);
  // and as one job of a call, behind a job whose keyframe 2 has no node at all
  const BowKf bare{5, 0, node2, off2, idx2, desc2.data()}, ka[2] = {k1, k1}, kb[2] = {bare, k2};
  const int32_t o1[3] = {0, 6, 12}, o2[3] = {0, 5, 10};
  const uint8_t l1[12] = {1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1}, l2[10] = {1, 1, 1, 1, 1, 0, 0, 1, 1, 1};
  uint64_t t2[12];
  int32_t nq[2], nd[2];
  memset(t2, 0xa5, sizeof t2);
  bow_pair_eval_host(2, ka, kb, o1, l1, o2, l2, t2, nq, nd);
  for (int i = 0; i < 6; i++) EXPECT(t2[i] == 0 && t2[6 + i] == table[i]);
  EXPECT(nq[0] == 0 && nd[0] == 0 && nq[1] == 3 && nd[1] == 2);
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
  walk();
  packing();
  if (g_fail) { printf("bow_search block: %d failures\n", g_fail); return 1; }
  printf("bow_search block ok\n");
  return 0;
}
