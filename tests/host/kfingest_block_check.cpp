// kfingest_block_check.cpp — KfIngestBlock of csrc/stage_blocks.h and the host side of csrc/kfingest_math.h on the CPU (tests/test_kfingest_block_cpu.py builds this
// with -fsanitize=address,undefined).  Every segment's offset against the segments in front of it, the two copied ranges, every segment filled (or read) to its
// declared length in a malloc'd block of exactly pin_bytes(); then the evaluator on rows whose answer is certain, its outputs in arrays of exactly the documented lengths.
#include "block_check.h"
#include "kfingest_math.h"
#include <math.h>

static void block(size_t M, size_t F, bool want) {
  KfIngestBlock b(M, F, want);
  Check c(b);
  c.up(b.desc, 32 * F, true, 16);
  c.up(b.slot, M, false); c.up(b.feat_off, M + 1, true);
  c.up(b.rec, FSM_REC_FLOATS * M, true); c.up(b.xy, 2 * F, true);
  c.up(b.oct, F, true);
  const size_t n_in = 32 * F + 4 * (M + M + 1 + 10 * M + 2 * F) + words(F);
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), ((n_in + 7) & ~(size_t)7));   // the pad in front of the doubles travels with the upload
  c.uploaded_bytes();
  // device only: the weights on 8 bytes, the words and nodes when the caller does not ask for them
  c.seg(b.weight, F, 0);
  c.seg(b.work_word, want ? 0 : F, 0); c.seg(b.work_node, want ? 0 : F, 0);
  const size_t n_work = c.o;
  c.down(b.bow_value, F);
  EXPECT_EQ(b.bow_value.off % 8, 0);
  EXPECT_EQ(b.down_begin(), b.bow_value.off);
  c.down(b.n_in, M); c.down(b.bow_n, M); c.down(b.fv_nn, M);
  c.down(b.bow_word, F); c.down(b.fv_node, F); c.down(b.fv_off, F + M); c.down(b.fv_idx, F);
  c.down(b.feat_word, want ? F : 0); c.down(b.feat_node, want ? F : 0);
  const size_t n_out = 8 * F + 4 * (3 * M + 3 * F + F + M + (want ? 2 * F : 0));
  EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), ((n_work + 7) & ~(size_t)7) + n_out);
  EXPECT_EQ(b.pin_bytes(), b.up_bytes() > n_out ? b.up_bytes() : n_out);
}

// A tree of two levels with three children under the root and two under each: 0 -> 1 2 3; 1 -> 4 5; 2 -> 6 7; 3 -> 8 9.  Node i's descriptor has its first kBits[i]
// bits set, so the distance of a descriptor with its first b bits set to node i is |b - kBits[i]|.
static const int kBits[10] = {0, 10, 20, 30, 8, 12, 18, 22, 28, 32};
struct Tree {
  int32_t child_off[11] = {0, 3, 5, 7, 9, 9, 9, 9, 9, 9, 9};
  int32_t child_id[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  uint8_t node_desc[10 * 32];
  int32_t word_id[10] = {-1, -1, -1, -1, 50, 40, 30, 20, 10, 0};   // word order is not leaf order
  double weight[10] = {0, 0, 0, 0, 0.1, 2.0, 0.0, -1.0, NAN, 3.0};
  kfi_tree t;
  static void bits(uint8_t* d, int n) { memset(d, 0, 32); for (int i = 0; i < n; i++) d[i / 8] |= (uint8_t)(1u << (i % 8)); }
  Tree() { for (int i = 0; i < 10; i++) bits(node_desc + 32 * i, kBits[i]); t = {10, 2, child_off, child_id, node_desc, word_id, weight}; }
};

static void evaluator() {
  Tree T;
  // descent: level 1 picks the nearest of 10 20 30 bits, level 2 the nearest of the node's two children, the first on a tie (15: 10 before 20; 20: 18 before 22;
  // 25: 20 before 30)
  uint32_t dw[80], d[8];
  memcpy(dw, T.node_desc, sizeof dw);
  const int rows[10] = {8, 12, 15, 18, 20, 22, 28, 32, 0, 25}, want_leaf[10] = {4, 5, 5, 6, 6, 7, 8, 9, 4, 7}, want_l1[10] = {1, 1, 1, 2, 2, 2, 3, 3, 1, 2};
  for (int r = 0; r < 10; r++) {
    uint8_t bytes[32]; Tree::bits(bytes, rows[r]); memcpy(d, bytes, 32);
    int nid = -1;
    const int leaf = kfi_descend(T.child_off, T.child_id, dw, 10, d, 1, &nid);
    EXPECT(leaf == want_leaf[r] && nid == want_l1[r]);
    int nid0 = -1, nid3 = -1;
    EXPECT(kfi_descend(T.child_off, T.child_id, dw, 10, d, 0, &nid0) == leaf && nid0 == 0);    // the recorded level is the root's: 0
    EXPECT(kfi_descend(T.child_off, T.child_id, dw, 10, d, 3, &nid3) == leaf && nid3 == 0);    // a leaf lies above the recorded level: 0
    EXPECT(kfi_descend(T.child_off, T.child_id, dw, 10, d, 2, &nid3) == leaf && nid3 == leaf);
  }
  // two keyframes in one call, arrays of exactly the documented lengths.  Keyframe 0: eight features on the leaves 4 4 5 4 4 4 4 9 (six on the word of weight 0.1),
  // keyframe 1: one feature each on 6 (stopped), 7 (negative), 8 (NaN): both vectors empty.
  const int b0[8] = {8, 8, 12, 8, 8, 8, 8, 32}, b1[3] = {18, 22, 28};
  const size_t F = 11, M = 2;
  uint8_t* desc = (uint8_t*)malloc(32 * F);
  for (int i = 0; i < 8; i++) Tree::bits(desc + 32 * i, b0[i]);
  for (int i = 0; i < 3; i++) Tree::bits(desc + 32 * (8 + i), b1[i]);
  const int32_t feat_off[3] = {0, 8, 11};
  int32_t *bow_n = (int32_t*)malloc(4 * M), *fv_nn = (int32_t*)malloc(4 * M), *bow_word = (int32_t*)malloc(4 * F), *fv_node = (int32_t*)malloc(4 * F),
          *fv_off = (int32_t*)malloc(4 * (F + M)), *fv_idx = (int32_t*)malloc(4 * F), *fw = (int32_t*)malloc(4 * F), *fn = (int32_t*)malloc(4 * F);
  double* bow_value = (double*)malloc(8 * F);
  const float rec[2 * FSM_REC_FLOATS] = {0};
  const float* xy = (const float*)desc;   // any non-null pointer: the rules read no feature array
  EXPECT(kfi_check_ingest(2, 8, rec, feat_off, xy, desc, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx) == nullptr);
  EXPECT(kfi_check_ingest(2, 7, rec, feat_off, xy, desc, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx) != nullptr);   // more than max_feat
  EXPECT(kfi_check_ingest(2, 8, rec, feat_off, xy, desc, desc, bow_n, nullptr, bow_value, fv_nn, fv_node, fv_off, fv_idx) != nullptr);
  EXPECT(kfi_check_ingest(2, 8, rec, feat_off, xy, desc, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, nullptr, fv_idx) != nullptr);
  EXPECT(kfi_check_ingest(0, 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == nullptr);
  const int32_t big[2] = {0, KFI_MAX_FEAT + 1}, most[2] = {0, KFI_MAX_FEAT};
  EXPECT(kfi_check_ingest(1, 65535, rec, big, xy, desc, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx) != nullptr);
  EXPECT(kfi_check_ingest(1, 65535, rec, most, xy, desc, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx) == nullptr);
  kfi_ingest_host(T.t, 1, 2, feat_off, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx, fw, fn);
  const int32_t want_word[8] = {50, 50, 40, 50, 50, 50, 50, 0}, want_node[8] = {1, 1, 1, 1, 1, 1, 1, 3};
  for (int i = 0; i < 8; i++) EXPECT(fw[i] == want_word[i] && fn[i] == want_node[i]);
  EXPECT(fw[8] == 30 && fw[9] == 20 && fw[10] == 10 && fn[8] == 2 && fn[9] == 2 && fn[10] == 3);
  // keyframe 0: words 0 (3.0), 40 (2.0), 50 (0.1 six times, added one after the other), the norm added in that order
  const double six = 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1, norm = 3.0 + 2.0 + six;
  EXPECT(six != 6 * 0.1);
  EXPECT(bow_n[0] == 3 && bow_word[0] == 0 && bow_word[1] == 40 && bow_word[2] == 50);
  EXPECT(bow_value[0] == 3.0 / norm && bow_value[1] == 2.0 / norm && bow_value[2] == six / norm);
  EXPECT(fv_nn[0] == 2 && fv_node[0] == 1 && fv_node[1] == 3 && fv_off[0] == 0 && fv_off[1] == 7 && fv_off[2] == 8);
  for (int i = 0; i < 7; i++) EXPECT(fv_idx[i] == i);
  EXPECT(fv_idx[7] == 7);
  // keyframe 1: nothing kept, nothing divided; its offsets start at feat_off[1] + 1
  EXPECT(bow_n[1] == 0 && fv_nn[1] == 0 && fv_off[8 + 1] == 0);
  // NULL feat_word / feat_node
  kfi_ingest_host(T.t, 1, 2, feat_off, desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx, nullptr, nullptr);
  EXPECT(bow_n[0] == 3 && fv_nn[0] == 2);
  free(desc); free(bow_n); free(fv_nn); free(bow_word); free(fv_node); free(fv_off); free(fv_idx); free(fw); free(fn); free(bow_value);
}

int main() {
  for (int want = 0; want < 2; want++) {
    block(1, 0, want); block(1, 1, want); block(1, 2, want); block(2, 3, want); block(3, 1001, want); block(40, 40 * 333 - 7, want); block(1, KFI_MAX_FEAT, want);
    block(5, 0, want);
  }
  evaluator();
  if (g_fail) { printf("kfingest block: %d failures\n", g_fail); return 1; }
  printf("kfingest block ok\n");
  return 0;
}
