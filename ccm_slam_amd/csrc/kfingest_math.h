// kfingest_math.h — the lines of ccm_kfstore_ingest, written once: what DBoW2's TemplatedVocabulary::transform(features, BowVector, FeatureVector,
// levelsup) (TemplatedVocabulary.h:1127-1190, :1218-1260) and BowVector::addWeight / normalize (BowVector.cpp:34-84) do to one keyframe's descriptors, as
// KeyFrame::ComputeBoW calls them.  __host__ __device__ under hipcc, plain C++ under g++ (host/ccm_host.cpp, tests/host/kfingest_block_check.cpp).  The kernels of
// kfingest.hip run kfi_kept, kfi_key and kfi_key_* ; the argument rules and the sequential evaluator kfi_ingest_host are the host's.
#pragma once
#include "kfstore_math.h"
#ifndef __HIP_DEVICE_COMPILE__
#include <algorithm>
#include <vector>
#endif

#define KFI_MAX_FEAT 4096   // the most features of one keyframe of an ingest call: its keys, weights and values stay in one workgroup's LDS (128 KB of the 160)

// The kept test (TemplatedVocabulary.h:1157, "not stopped"): a zero, negative or NaN weight drops the feature from both vectors.
FSM_HD bool kfi_kept(double w) { return w > 0; }

// (id, feature) as ONE sortable key: ascending id (signed), then ascending feature.  The keys of a keyframe are unique, so every exact sort gives one order.
FSM_HD uint64_t kfi_key(int32_t id, int feat) { return ((uint64_t)((uint32_t)id ^ 0x80000000u) << 32) | (uint32_t)feat; }
FSM_HD int32_t kfi_key_id(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
FSM_HD int kfi_key_feat(uint64_t key) { return (int)(uint32_t)key; }
#define KFI_NO_KEY 0xFFFFFFFFFFFFFFFFull   // a dropped feature's place: behind every key

// FORB::distance
FSM_HD int kfi_ham256(const uint32_t* a, const uint32_t* b) {
  int d = 0;
  for (int k = 0; k < 8; k++) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// The descent for one feature on the calling thread (bow_descend_kernel's rule, vocab.h): the first minimum in child order wins; the node at level nid_level is
// recorded, 0 when that level is <= 0 or a leaf lies above it.  Returns the leaf.  n_nodes bounds the walk.
FSM_HD int kfi_descend(const int32_t* child_off, const int32_t* child_id, const uint32_t* node_desc, int n_nodes, const uint32_t* desc, int nid_level, int* nid) {
  int node = 0, level = 0;
  *nid = 0;
  for (int step = 0; step < n_nodes; step++) {
    const int c0 = child_off[node], c1 = child_off[node + 1];
    if (c1 <= c0) break;
    ++level;
    int best = 0x7FFFFFFF, best_c = c0;
    for (int c = c0; c < c1; c++) {
      const int d = kfi_ham256(desc, node_desc + 8 * (size_t)child_id[c]);
      if (d < best) { best = d; best_c = c; }
    }
    node = child_id[best_c];
    if (level == nid_level) *nid = node;
  }
  return node;
}

// The argument rules of ccm_kfstore_ingest that read the arrays alone, shared by the stage and the host evaluator: ccm_kfstore_add's without a grid, then the
// ingest's own; nullptr, or what is wrong.
FSM_HD const char* kfi_check_ingest(int M, int max_feat, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
                                    const uint8_t* feat_desc, const int32_t* bow_n, const int32_t* bow_word, const double* bow_value, const int32_t* fv_nn,
                                    const int32_t* fv_node, const int32_t* fv_off, const int32_t* fv_idx) {
  if (const char* why = kfg_check_add(M, max_feat, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, nullptr, nullptr)) return why;
  if (M == 0) return nullptr;
  for (int m = 0; m < M; m++)
    if (feat_off[m + 1] - feat_off[m] > KFI_MAX_FEAT) return "a keyframe with more than KFI_MAX_FEAT = 4096 features (add and set_featvec take it)";
  if (!bow_n || !fv_nn || !fv_off) return "null output pointers";
  if (feat_off[M] && (!bow_word || !bow_value || !fv_node || !fv_idx)) return "null output pointers";
  return nullptr;
}

#ifndef __HIP_DEVICE_COMPILE__
// The flat tree of ccm_vocab_create on the host.
struct kfi_tree {
  int n_nodes, L;
  const int32_t *child_off, *child_id;
  const uint8_t* node_desc;
  const int32_t* word_id;
  const double* weight;
};

// One keyframe's two vectors from its features' (word, weight, node), sequentially: addWeight in feature order (the first occurrence's weight, then += w per
// further occurrence), normalize (the sum of fabs over the words in ascending id, one after the other; above 0, every value divided by it), addFeature (nodes
// ascending, features ascending inside a node).  Outputs in the layout of ccm_kfstore_ingest, at the keyframe's own start: bow_word / bow_value [n], fv_node [n],
// fv_off [n + 1], fv_idx [n].
static inline void kfi_vectors_host(int n, const int32_t* word, const double* weight, const int32_t* node, int32_t* bow_n, int32_t* bow_word, double* bow_value,
                                    int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx) {
  std::vector<uint64_t> wk, nk;
  for (int i = 0; i < n; i++)
    if (kfi_kept(weight[i])) { wk.push_back(kfi_key(word[i], i)); nk.push_back(kfi_key(node[i], i)); }
  std::sort(wk.begin(), wk.end());
  std::sort(nk.begin(), nk.end());
  int nw = 0;
  for (size_t s = 0; s < wk.size();) {
    const int32_t id = kfi_key_id(wk[s]);
    double acc = weight[kfi_key_feat(wk[s])];
    for (s++; s < wk.size() && kfi_key_id(wk[s]) == id; s++) acc += weight[kfi_key_feat(wk[s])];
    bow_word[nw] = id; bow_value[nw] = acc; nw++;
  }
  double norm = 0.0;
  for (int r = 0; r < nw; r++) norm += fabs(bow_value[r]);
  if (norm > 0.0)
    for (int r = 0; r < nw; r++) bow_value[r] /= norm;
  *bow_n = nw;
  int nn = 0;
  for (size_t s = 0; s < nk.size(); s++) {
    if (s == 0 || kfi_key_id(nk[s]) != kfi_key_id(nk[s - 1])) { fv_node[nn] = kfi_key_id(nk[s]); fv_off[nn] = (int32_t)s; nn++; }
    fv_idx[s] = kfi_key_feat(nk[s]);
  }
  fv_off[nn] = (int32_t)nk.size();
  *fv_nn = nn;
  // what lies behind the counts is written as zeros, as the kernel writes it
  for (int r = nw; r < n; r++) { bow_word[r] = 0; bow_value[r] = 0.0; }
  for (int r = nn; r < n; r++) { fv_node[r] = 0; fv_off[r + 1] = 0; }
  for (int r = (int)nk.size(); r < n; r++) fv_idx[r] = 0;
}

// ccm_kfstore_ingest's vectors for M keyframes on the calling thread: the descent of every feature, then kfi_vectors_host per keyframe.  The caller has run
// kfi_check_ingest.  feat_word / feat_node are nullable.
static inline void kfi_ingest_host(const kfi_tree& t, int levelsup, int M, const int32_t* feat_off, const uint8_t* feat_desc, int32_t* bow_n, int32_t* bow_word,
                                   double* bow_value, int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node) {
  std::vector<int32_t> word, node;
  std::vector<double> w;
  std::vector<uint32_t> dw((size_t)t.n_nodes * 8);
  memcpy(dw.data(), t.node_desc, dw.size() * 4);
  for (int m = 0; m < M; m++) {
    const int32_t f0 = feat_off[m], n = feat_off[m + 1] - f0;
    word.resize((size_t)n); node.resize((size_t)n); w.resize((size_t)n);
    for (int i = 0; i < n; i++) {
      uint32_t d[8];
      memcpy(d, feat_desc + 32 * (size_t)(f0 + i), 32);
      int nid;
      const int leaf = kfi_descend(t.child_off, t.child_id, dw.data(), t.n_nodes, d, t.L - levelsup, &nid);
      word[i] = t.word_id[leaf]; w[i] = t.weight[leaf]; node[i] = nid;
      if (feat_word) feat_word[f0 + i] = word[i];
      if (feat_node) feat_node[f0 + i] = nid;
    }
    kfi_vectors_host(n, word.data(), w.data(), node.data(), bow_n + m, bow_word + f0, bow_value + f0, fv_nn + m, fv_node + f0, fv_off + f0 + m, fv_idx + f0);
  }
}
#endif
