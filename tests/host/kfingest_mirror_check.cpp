// kfingest_mirror_check.cpp — the C++ mirror of ccm_kfstore_ingest as INTEGRATION.md §7q names it, run once without a device (tests/test_kfingest_cpu.py builds this
// against libccm_host.so): a cslam::ORBVocabulary constructed WITHOUT a context (its host copy of the flat tree alone) and
// cslam::KeyFrameStore::ingest(ctx = nullptr, voc, …, std::vector<BowVector>&, std::vector<FeatureVector>&) on a host-only store.  The per-keyframe vectors must be
// the split of kfi_ingest_host's flat outputs on the caller's own arrays, the shadows those of add + set_featvec, a refusal must leave the vectors alone.
#include "../../ccm_slam_amd/host/ccm_host.h"
#include "../../ccm_slam_amd/csrc/kfingest_math.h"
#include <stdio.h>

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)

static unsigned g_r = 2463534242u;
static unsigned rnd() { g_r = g_r * 1664525u + 1013904223u; return g_r >> 8; }

int main() {
  // a complete tree, k = 5, L = 3: 156 nodes in breadth-first order, random descriptors, one word in seven stopped, one negative weight
  const int k = 5, L = 3, n_inner = 31, n_nodes = 156;
  std::vector<int32_t> child_off(n_nodes + 1), child_id(n_inner * k), word_id(n_nodes, -1);
  std::vector<uint8_t> node_desc(32 * n_nodes);
  std::vector<double> weight(n_nodes, 0.0);
  for (int i = 0; i <= n_nodes; i++) child_off[i] = (i < n_inner ? i : n_inner) * k;
  for (int i = 0; i < n_inner * k; i++) child_id[i] = i + 1;
  for (auto& b : node_desc) b = (uint8_t)rnd();
  for (int i = n_inner; i < n_nodes; i++) { word_id[i] = n_nodes - i; weight[i] = (i % 7 == 0) ? 0.0 : 0.1 + (rnd() % 1000) / 173.0; }   // word order is not leaf order
  weight[n_inner + 1] = -2.0;
  cslam::ORBVocabulary voc(nullptr, n_nodes, L, child_off.data(), child_id.data(), node_desc.data(), word_id.data(), weight.data());
  EXPECT(voc.handle() == nullptr && voc.n_nodes() == n_nodes && voc.L() == L);
  EXPECT(voc.child_off() == child_off && voc.child_id() == child_id && voc.node_desc() == node_desc && voc.word_id() == word_id && voc.weight() == weight);
  {
    cslam::BowVector b; cslam::FeatureVector f;
    bool threw = false;
    try { voc.transform(node_desc.data(), 1, b, f); } catch (const std::exception&) { threw = true; }
    EXPECT(threw);   // no device tree: the per-keyframe transform says so, it does not fall back
  }
  // three keyframes of 300, 0 and 77 features
  const int M = 3;
  const int32_t feat_off[M + 1] = {0, 300, 300, 377};
  const int F = 377;
  const int64_t keys[M] = {11, 12, 13};
  std::vector<uint8_t> desc(32 * F), oct(F);
  std::vector<float> xy(2 * F), rec(10 * M), angle(F);
  for (auto& b : desc) b = (uint8_t)rnd();
  for (int i = 0; i < F; i++) { oct[i] = (uint8_t)(rnd() % 8); xy[2 * i] = (float)(rnd() % 752); xy[2 * i + 1] = (float)(rnd() % 480); angle[i] = (float)(rnd() % 360); }
  for (int m = 0; m < M; m++) {
    const float r[10] = {458.f, 457.f, 367.f, 248.f, 0.f, 0.f, 752.f, 480.f, 75.f / 752.f, 48.f / 480.f};
    for (int j = 0; j < 10; j++) rec[10 * m + j] = r[j];
  }
  cslam::KeyFrameStore a(nullptr, 4, 300), b(nullptr, 4, 300);
  std::vector<cslam::BowVector> bow;
  std::vector<cslam::FeatureVector> fv;
  EXPECT(a.ingest(nullptr, voc, M, keys, rec.data(), feat_off, xy.data(), oct.data(), desc.data(), angle.data(), bow, fv, 1) == CCM_OK);
  EXPECT(a.live() == 3 && bow.size() == 3 && fv.size() == 3);
  // the flat evaluator on the caller's own arrays
  std::vector<int32_t> bow_n(M), fv_nn(M), bow_word(F), fv_node(F), fv_off(F + M), fv_idx(F);
  std::vector<double> bow_value(F);
  const kfi_tree t = {n_nodes, L, child_off.data(), child_id.data(), node_desc.data(), word_id.data(), weight.data()};
  kfi_ingest_host(t, 1, M, feat_off, desc.data(), bow_n.data(), bow_word.data(), bow_value.data(), fv_nn.data(), fv_node.data(), fv_off.data(), fv_idx.data(), nullptr, nullptr);
  EXPECT(bow_n[0] > 20 && bow_n[0] < 300 && fv_nn[0] == 25 && bow_n[1] == 0 && fv_nn[1] == 0);   // 25 nodes at level 2; stopped words dropped
  for (int m = 0; m < M && bow.size() == 3; m++) {
    const int f0 = feat_off[m], nw = bow_n[m], nn = fv_nn[m];
    EXPECT((int)bow[m].word.size() == nw && (int)bow[m].value.size() == nw && (int)fv[m].node.size() == nn && (int)fv[m].off.size() == nn + 1);
    if ((int)bow[m].word.size() != nw || (int)fv[m].off.size() != nn + 1) continue;
    EXPECT(std::equal(bow[m].word.begin(), bow[m].word.end(), bow_word.begin() + f0));
    EXPECT(nw == 0 || !memcmp(bow[m].value.data(), bow_value.data() + f0, 8 * (size_t)nw));
    EXPECT(std::equal(fv[m].node.begin(), fv[m].node.end(), fv_node.begin() + f0));
    EXPECT(std::equal(fv[m].off.begin(), fv[m].off.end(), fv_off.begin() + f0 + m));
    EXPECT((int)fv[m].idx.size() == fv[m].off.back() && std::equal(fv[m].idx.begin(), fv[m].idx.end(), fv_idx.begin() + f0));
    double sum = 0.0;
    for (double x : bow[m].value) sum += x;
    EXPECT(nw == 0 || fabs(sum - 1.0) < 1e-12);
  }
  // the shadows are those of add followed by set_featvec
  EXPECT(b.add(nullptr, M, keys, rec.data(), feat_off, xy.data(), oct.data(), desc.data()) == CCM_OK);
  for (int m = 0; m < M && fv.size() == 3; m++)
    EXPECT(b.set_featvec(nullptr, keys[m], cslam::FeatureVectorView{(int)fv[m].node.size(), fv[m].node.data(), fv[m].off.data(), fv[m].idx.data()}, angle.data() + feat_off[m]) == CCM_OK);
  for (int m = 0; m < M; m++) {
    const auto x = a.shadow(keys[m]), y = b.shadow(keys[m]);
    EXPECT(x && y);
    if (!x || !y) continue;
    EXPECT(!memcmp(x->rec, y->rec, sizeof x->rec) && x->n == y->n && x->n_in == y->n_in && x->xy == y->xy && x->oct == y->oct && x->desc == y->desc);
    EXPECT(x->cell_off == y->cell_off && x->cell_idx == y->cell_idx);
    EXPECT(x->has_fv && y->has_fv && x->fv_node == y->fv_node && x->fv_off == y->fv_off && x->fv_idx == y->fv_idx && x->angle == y->angle);
    EXPECT(x->n == feat_off[m + 1] - feat_off[m]);
  }
  // refusals leave the vectors and the store alone: a live key; more features than the store's max_feat
  const std::vector<cslam::BowVector> bow0 = bow;
  EXPECT(a.ingest(nullptr, voc, 1, keys + 2, rec.data(), feat_off, xy.data(), oct.data(), desc.data(), nullptr, bow, fv, 1) == CCM_E_STATE);
  const int64_t k9 = 9; const int32_t too_many[2] = {0, 301};
  EXPECT(a.ingest(nullptr, voc, 1, &k9, rec.data(), too_many, xy.data(), oct.data(), desc.data(), nullptr, bow, fv, 1) == CCM_E_ARG);
  EXPECT(a.live() == 3 && bow.size() == 3 && bow[0].word == bow0[0].word && bow[2].value == bow0[2].value);
  // M == 0
  std::vector<cslam::BowVector> none_b; std::vector<cslam::FeatureVector> none_f;
  EXPECT(a.ingest(nullptr, voc, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, none_b, none_f) == CCM_OK && none_b.empty() && a.live() == 3);
  // the next call after the refusals is right: the first keyframe again under another key
  const int32_t one[2] = {0, 300};
  EXPECT(a.ingest(nullptr, voc, 1, &k9, rec.data(), one, xy.data(), oct.data(), desc.data(), nullptr, bow, fv, 1) == CCM_OK);
  EXPECT(bow.size() == 1 && bow[0].word == bow0[0].word && bow[0].value == bow0[0].value && a.live() == 4);
  if (g_fail) { printf("kfingest mirror: %d failures\n", g_fail); return 1; }
  printf("kfingest mirror ok\n");
  return 0;
}
