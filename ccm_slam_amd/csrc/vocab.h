// vocab.h — the vocabulary handle (ccm_vocab_create, hamming.hip) and the wave-level descent of the DBoW2 tree, shared by hamming.hip (bow_descend_kernel of
// ccm_bow_transform) and kfingest.hip (ccm_kfstore_ingest).  The device arrays are written once by ccm_vocab_create and read in place afterwards.
#pragma once
#include "common.h"

struct ccm_vocab {
  ccm_ctx* ctx; int n_nodes, L;
  int32_t *d_child_off, *d_child_id; uint32_t* d_node_desc;
  int32_t* d_word_id; double* d_weight;   // per node, for the ingest kernels; the host copies below serve ccm_bow_transform
  std::vector<int32_t> word_id; std::vector<double> weight;
};

#ifdef __HIPCC__
// TemplatedVocabulary::transform (DBoW2/TemplatedVocabulary.h:1218-1260) for ONE feature by ONE wave, every lane active: at every level the lanes take one child
// each (64 at a time), the wave picks the child with the least FORB::distance, the FIRST minimum winning (strict '<' in child order).  a: the feature's eight
// words, wave-uniform.  The leaf is returned in every lane; *nid is the node at level nid_level, 0 when that level is <= 0 or a leaf lies above it.  n_nodes
// bounds the walk: a path of a tree is shorter, so the bound is met only by child lists that are no tree.
__device__ __forceinline__ int vocab_descend_wave(const uint32_t (&a)[8], int lane, const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_id,
                                                  const uint32_t* __restrict__ node_desc, int n_nodes, int nid_level, int* nid) {
  int node = 0, level = 0;
  *nid = 0;
  for (int step = 0; step < n_nodes; step++) {
    const int c0 = child_off[node], c1 = child_off[node + 1];
    if (c1 <= c0) break;   // leaf
    ++level;
    uint32_t best = 0xFFFFFFFFu;
    for (int base = c0; base < c1; base += 64) {
      uint32_t key = 0xFFFFFFFFu;
      if (base + lane < c1) {
        const int id = child_id[base + lane];
        const uint4* bp = reinterpret_cast<const uint4*>(node_desc + (size_t)id * 8);
        const uint4 lo = bp[0], hi = bp[1];
        const int d = __builtin_popcount(a[0] ^ lo.x) + __builtin_popcount(a[1] ^ lo.y) + __builtin_popcount(a[2] ^ lo.z) + __builtin_popcount(a[3] ^ lo.w) +
                      __builtin_popcount(a[4] ^ hi.x) + __builtin_popcount(a[5] ^ hi.y) + __builtin_popcount(a[6] ^ hi.z) + __builtin_popcount(a[7] ^ hi.w);
        key = ((uint32_t)d << 20) | (uint32_t)(base + lane - c0);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, off, 64));
      best = min(best, key);
    }
    node = child_id[c0 + (int)(best & 0xFFFFFu)];
    if (level == nid_level) *nid = node;
  }
  return node;
}
#endif
