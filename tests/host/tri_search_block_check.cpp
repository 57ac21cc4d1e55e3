// tri_search_block_check.cpp — TriSearchResidentBlock of csrc/stage_blocks.h and the lines of csrc/tri_search_math.h on the CPU (tests/test_tri_search_block_cpu.py
// builds this with -fsanitize=address,undefined).  The block: every segment's offset against the segments in front of it, the two copied ranges, and every segment
// filled (or read) to its declared length in a malloc'd block of exactly pin_bytes().  The lines: tsm_accept and tsm_merge against the sequential loop of
// ORBmatcher.cpp:753-785 on every list of up to five (distance, gate) pairs over the distances {0, 1, 50, 51}, at every split point and every pair of split points, and
// the word packing round trip; and the evaluator's walk over a keyframe pair's common nodes (bow_search_math.h's fv_pair_walk_host) on one pair with an absent node,
// a node without a query and a query without a candidate.
#include "block_check.h"

static void block(size_t J, size_t M1, size_t M2, size_t L) {
  TriSearchResidentBlock b(J, M1, M2, L);
  Check c(b);
  c.up(b.job, TSM_JOB_INTS * J, false, 16);
  c.up(b.line_thr, L, false);
  c.up(b.job_epi, TSM_EPI_FLOATS * J, true); c.up(b.scale_factors, L, true);
  c.up(b.has1, M1, true); c.up(b.has2, M2, true);
  const size_t n_in = 4 * TSM_JOB_INTS * J + 8 * L + 4 * TSM_EPI_FLOATS * J + 4 * L + words(M1) + words(M2);
  EXPECT_EQ(c.o, n_in);
  EXPECT(b.line_thr.off % 8 == 0 && (size_t)((const char*)b.up(b.line_thr) - (const char*)b.host()) % 8 == 0);   // the doubles lie on 8 bytes on both sides
  c.zero_and_down(b.table, M1); c.zero_and_down(b.n_query, J); c.zero_and_down(b.n_match, J); c.zero_and_down(b.n_dist, J);
  const size_t n_out = 4 * M1 + 12 * J;
  EXPECT_EQ(b.table.off, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in + n_out);
  c.uploaded_bytes();
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in + n_out);
}

// the sequential loop of ORBmatcher.cpp:753-785 on a list of (distance, gates passed); candidate i is feature 100 + i
static TriBest sequential(const int* dist, const bool* gate, int i0, int i1) {
  int bestDist = 50, bestIdx2 = -1;
  for (int i = i0; i < i1; i++) {
    if (dist[i] > 50 || dist[i] > bestDist) continue;
    if (!gate[i]) continue;
    bestIdx2 = 100 + i; bestDist = dist[i];
  }
  return TriBest{bestDist, bestIdx2};
}
static bool same(const TriBest& a, const TriBest& b) { return a.d == b.d && a.idx == b.idx; }
// a part as the kernel forms it: tsm_accept over the candidates that pass the gates and the threshold
static TriBest part(const int* dist, const bool* gate, int i0, int i1) {
  TriBest b = tsm_empty();
  for (int i = i0; i < i1; i++)
    if (gate[i] && dist[i] <= TSM_TH_LOW) tsm_accept(b, dist[i], 100 + i);
  return b;
}

static void lines() {
  const int values[4] = {0, 1, 50, 51};
  long checked = 0;
  for (int len = 0; len <= 5; len++) {
    int total = 1;
    for (int i = 0; i < len; i++) total *= 8;
    for (int code = 0; code < total; code++) {
      int dist[5] = {0, 0, 0, 0, 0};
      bool gate[5] = {false, false, false, false, false};
      for (int i = 0, c = code; i < len; i++, c /= 8) { dist[i] = values[c % 4]; gate[i] = (c % 8) >= 4; }
      const TriBest want = sequential(dist, gate, 0, len);
      EXPECT(same(part(dist, gate, 0, len), want));
      for (int split = 0; split <= len; split++) {
        EXPECT(same(tsm_merge(sequential(dist, gate, 0, split), sequential(dist, gate, split, len)), want));
        EXPECT(same(tsm_merge(part(dist, gate, 0, split), part(dist, gate, split, len)), want));
        for (int split2 = split; split2 <= len; split2++)   // three parts, merged in order
          EXPECT(same(tsm_merge(tsm_merge(part(dist, gate, 0, split), part(dist, gate, split, split2)), part(dist, gate, split2, len)), want));
        checked++;
      }
    }
  }
  EXPECT(checked > 100000);
  // the properties by name: the last index of the minimum, 50 accepted and 51 not, the empty sides
  const int five[2] = {5, 5}, edge[2] = {50, 51};
  const bool yes[2] = {true, true};
  EXPECT(same(sequential(five, yes, 0, 2), TriBest{5, 101}));
  EXPECT(same(tsm_merge(part(five, yes, 0, 1), part(five, yes, 1, 2)), TriBest{5, 101}));
  EXPECT(same(part(edge, yes, 0, 2), TriBest{50, 100}));
  EXPECT(same(part(edge, yes, 1, 2), TriBest{50, -1}));
  EXPECT(same(tsm_merge(tsm_empty(), tsm_empty()), TriBest{50, -1}));
  EXPECT(same(tsm_merge(tsm_empty(), part(five, yes, 0, 1)), TriBest{5, 100}));
  EXPECT(same(tsm_merge(part(five, yes, 0, 1), tsm_empty()), TriBest{5, 100}));
}

// One keyframe pair through the job evaluator, on arrays of exactly the lengths it may read.  Keyframe 1 (every keypoint on the row y = 50): node 2 {0, 1} (keyframe 2
// lacks it), node 5 {2} (it has a map point: a node without a query), node 7 {3, 4} (keyframe 2's node 7 holds only features with a map point: queries without a
// candidate), node 9 {5}.  Keyframe 2: node 5 {4}, node 7 {0, 1}, node 9 {2, 3}: feature 2 at distance 3 on the row, feature 3 at distance 1 ten rows below it.
// F12 makes the epipolar line of (x1, y1) the row y2 = y1 with den = 1; the epipole is far away.
static void walk() {
  const int32_t node1[4] = {2, 5, 7, 9}, off1[5] = {0, 2, 3, 5, 6}, node2[3] = {5, 7, 9}, off2[4] = {0, 1, 3, 5};
  const uint16_t idx1[6] = {0, 1, 2, 3, 4, 5}, idx2[5] = {4, 0, 1, 2, 3};
  std::vector<uint8_t> desc1(6 * 32, 0), desc2(5 * 32, 0);
  desc2[2 * 32] = 0x07; desc2[3 * 32] = 0x01;
  const float xy1[12] = {100, 50, 110, 50, 120, 50, 130, 50, 140, 50, 150, 50}, xy2[10] = {200, 50, 210, 50, 220, 50, 230, 60, 240, 50};
  const uint8_t oct1[6] = {0, 0, 0, 0, 0, 0}, oct2[5] = {0, 0, 0, 0, 0};
  const uint8_t has1[6] = {0, 0, 1, 0, 0, 0}, has2[5] = {1, 1, 0, 0, 0};
  const float epi[TSM_EPI_FLOATS] = {0, 0, 0, 0, 0, -1, 0, 1, 0, -1000, 240}, sf[2] = {1.0f, 1.2f}, sigma2[2] = {1.0f, 1.44f};
  const TriKf k1{BowKf{6, 4, node1, off1, idx1, desc1.data()}, xy1, oct1}, k2{BowKf{5, 3, node2, off2, idx2, desc2.data()}, xy2, oct2};
  const TriLevels lv{2, sf, sigma2};
  // by hand: no candidate = status 1, bestDist 50, no index; feature 5 = status 2, distance 3, feature 2 (the nearer feature 3 fails the line gate: 100 > 3.84)
  uint32_t table[6] = {9, 9, 9, 9, 9, 9};
  int32_t n_query = -1, n_match = -1, n_dist = -1;
  tri_job_eval_host(k1, k2, has1, has2, epi, lv, table, &n_query, &n_match, &n_dist);
  EXPECT(table[0] == 0 && table[1] == 0 && table[2] == 0);
  EXPECT(table[3] == 0x40320000u && table[4] == 0x40320000u && table[5] == 0x80030003u);
  EXPECT(n_query == 3 && n_match == 1 && n_dist == 2);
  // and as one job of a call, behind a job whose keyframe 2 has no node at all
  const TriKf bare{BowKf{5, 0, node2, off2, idx2, desc2.data()}, xy2, oct2}, ka[2] = {k1, k1}, kb[2] = {bare, k2};
  const int32_t o1[3] = {0, 6, 12}, o2[3] = {0, 5, 10};
  const uint8_t h1[12] = {0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0}, h2[10] = {0, 0, 0, 0, 0, 1, 1, 0, 0, 0};
  const float epis[2 * TSM_EPI_FLOATS] = {0, 0, 0, 0, 0, -1, 0, 1, 0, -1000, 240, 0, 0, 0, 0, 0, -1, 0, 1, 0, -1000, 240};
  uint32_t t2[12];
  int32_t nq[2], nm[2], nd[2];
  memset(t2, 0xa5, sizeof t2);
  tri_search_eval_host(2, ka, kb, o1, h1, o2, h2, epis, lv, t2, nq, nm, nd);
  for (int i = 0; i < 6; i++) EXPECT(t2[i] == 0 && t2[6 + i] == table[i]);
  EXPECT(nq[0] == 0 && nm[0] == 0 && nd[0] == 0 && nq[1] == 3 && nm[1] == 1 && nd[1] == 2);
}

static void packing() {
  EXPECT(tsm_pack(TSM_NOT_A_QUERY, TriBest{7, 9}) == 0);
  const int idxs[] = {-1, 0, 1, 255, 256, 32767, 32768, 65534}, dists[] = {0, 1, 49, 50};
  for (int status : {TSM_NO_MATCH, TSM_MATCHED})
    for (int idx : idxs)
      for (int d : dists) {
        const uint32_t w = tsm_pack(status, TriBest{d, idx});
        EXPECT(w != 0 && tsm_status(w) == status && tsm_idx(w) == idx && tsm_dist(w) == d);
      }
  // the gates on values whose answers are certain
  EXPECT(tsm_epipole_gate(0.0f, 0.0f, 6.0f, 8.0f, 1.0f) == false);    // 36 + 64 = 100 is not < 100
  EXPECT(tsm_epipole_gate(0.0f, 0.0f, 6.0f, 7.0f, 1.0f) == true);
  const float F[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};
  const TriLine l = tsm_line(3.0f, 100.0f, F);
  EXPECT(l.a == 0.0f && l.b == 1.0f && l.c == -100.0f && l.den == 1.0f);
  EXPECT(tsm_line_gate(l.a, l.b, l.c, 50.0f, 101.5f, 1.0f) == true);    // 2.25 < 3.84
  EXPECT(tsm_line_gate(l.a, l.b, l.c, 50.0f, 102.0f, 1.0f) == false);   // 4 > 3.84
  EXPECT(tsm_line_gate(0.0f, 0.0f, 1.0f, 50.0f, 100.0f, 1.0f) == false);   // den == 0
  EXPECT(tsm_check_args(1, F, 0, F, F) != nullptr && tsm_check_args(1, nullptr, 8, F, F) != nullptr && tsm_check_args(0, nullptr, 8, nullptr, nullptr) == nullptr &&
         tsm_check_args(1, F, 8, F, F) == nullptr);
}

int main() {
  block(1, 0, 0, 1); block(1, 1, 1, 1); block(1, 3, 5, 8); block(2, 7, 1000, 8); block(3, 3 * 1001, 1001 + 999 + 2, 7);
  for (size_t J : {1, 2, 20})
    for (size_t n : {1, 63, 64, 65, 257, 1000, 2001}) block(J, J * n, J * n - (J > 1), 8);   // mask lengths that are no multiple of four
  lines();
  walk();
  packing();
  if (g_fail) { printf("tri_search block: %d failures\n", g_fail); return 1; }
  printf("tri_search block ok\n");
  return 0;
}
