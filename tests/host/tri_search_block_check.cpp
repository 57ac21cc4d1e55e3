// tri_search_block_check.cpp — TriSearchResidentBlock of csrc/stage_blocks.h and the lines of csrc/tri_search_math.h on the CPU (tests/test_tri_search_block_cpu.py
// builds this with -fsanitize=address,undefined).  The block: every segment's offset against the segments in front of it, the two copied ranges, and every segment
// filled (or read) to its declared length in a malloc'd block of exactly pin_bytes().  The lines: tsm_accept and tsm_merge against the sequential loop of
// ORBmatcher.cpp:753-785 on every list of up to five (distance, gate) pairs over the distances {0, 1, 50, 51}, at every split point and every pair of split points, and
// the word packing round trip.
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
  packing();
  if (g_fail) { printf("tri_search block: %d failures\n", g_fail); return 1; }
  printf("tri_search block ok\n");
  return 0;
}
