// bow_search_math.h — the inner lines of ORBmatcher::SearchByBoW(pKF1, pKF2, ...) (cslam/src/ORBmatcher.cpp:609-639), once, for the form of bowsearch.hip and for
// the host: the update of (bestDist1, bestIdx2, bestDist2) by one distance, the merge of two such partial results, the packing of one result word,
// the argument rules of ccm_kfstore_set_featvec, the host walk over the common nodes of a keyframe pair that this search and tri_search_math.h's share
// (fv_pair_walk_host; the device's is fv_pair.h's), and the host evaluator of a whole ccm_bow_pair_eval_resident call.  Integer work throughout: host and device
// agree bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define BSM_HD __host__ __device__ inline
#else
#define BSM_HD static inline
#endif

#define BSM_NONE 256          // bestDist1 / bestDist2 before any candidate (:610, :612)
#define BSM_JOB_INTS 8        // a job on the device: slot 1, slot 2, nodes of keyframe 1, nodes of keyframe 2, first mask byte of side 1, of side 2, first work item, 0
enum { BSM_NOT_A_QUERY = 0, BSM_NO_CANDIDATE = 1, BSM_EVALUATED = 2 };

struct BowBest { int d1, idx, d2; };   // bestDist1, bestIdx2, bestDist2

BSM_HD BowBest bsm_empty() { return BowBest{BSM_NONE, -1, BSM_NONE}; }

// :631-639.  Strict '<': the FIRST candidate in list order that reaches the minimum keeps bestIdx2, and bestDist2 is the second smallest distance as a multiset.
BSM_HD void bsm_update(BowBest& b, int dist, int idx2) {
  if (dist < b.d1) { b.d2 = b.d1; b.d1 = dist; b.idx = idx2; }
  else if (dist < b.d2) b.d2 = dist;
}

// What the loop leaves after the candidates of `a` followed by those of `b`.  The two smallest of the union: on equal minima a's index stays (it came first).
BSM_HD BowBest bsm_merge(const BowBest& a, const BowBest& b) {
  if (b.d1 < a.d1) return BowBest{b.d1, b.idx, a.d1 < b.d2 ? a.d1 : b.d2};
  return BowBest{a.d1, a.idx, a.d2 < b.d1 ? a.d2 : b.d1};
}

// One result word.  bits 0-15: bestIdx2 + 1 (0: none; a feature index is below 65535), 16-24: bestDist1, 25-33: bestDist2, 34-49: the position of the query's node
// in keyframe 2's node list (what the re-evaluation rule of cslam::SearchByBoWBatch walks), 62-63: the status.  A feature that is no query has the word 0.
BSM_HD uint64_t bsm_pack(int status, const BowBest& b, int node2) {
  if (status == BSM_NOT_A_QUERY) return 0;
  return (uint64_t)(uint32_t)(b.idx + 1) | (uint64_t)(uint32_t)b.d1 << 16 | (uint64_t)(uint32_t)b.d2 << 25 | (uint64_t)(uint32_t)node2 << 34 | (uint64_t)status << 62;
}
BSM_HD int bsm_status(uint64_t w) { return (int)(w >> 62); }
BSM_HD BowBest bsm_best(uint64_t w) { return BowBest{(int)(w >> 16 & 0x1FF), (int)(w & 0xFFFF) - 1, (int)(w >> 25 & 0x1FF)}; }
BSM_HD int bsm_node2(uint64_t w) { return (int)(w >> 34 & 0xFFFF); }

BSM_HD int bsm_hamming(const uint8_t* a, const uint8_t* b) {   // ORBmatcher::DescriptorDistance (:1653-1669): the bits that differ among the 256
  int d = 0;
  for (int k = 0; k < 4; k++) {
    uint64_t x, y;
    memcpy(&x, a + 8 * k, 8); memcpy(&y, b + 8 * k, 8);   // the descriptors of a shadow lie on no particular boundary
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

// the position of `node` in the ascending list nodes[0 .. nn), or -1
BSM_HD int bsm_find_node(const int32_t* nodes, int nn, int32_t node) {
  int lo = 0, hi = nn;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nodes[mid] < node) lo = mid + 1; else hi = mid;
  }
  return lo < nn && nodes[lo] == node ? lo : -1;
}

// The argument rules of ccm_kfstore_set_featvec for a keyframe of n features; nullptr, or what is wrong.  seen: n bytes of scratch.
static inline const char* bsm_check_featvec(int n, int nn, const int32_t* node, const int32_t* off, const int32_t* idx, uint8_t* seen) {
  if (nn < 0) return "nn negative";
  if (nn == 0) return nullptr;
  if (!node || !off || !idx) return "null pointers";
  if (off[0] != 0) return "off[0] != 0";
  for (int a = 0; a < nn; a++) {
    if (node[a] < 0) return "a negative node id";
    if (a && node[a] <= node[a - 1]) return "the node ids do not ascend";
    if (off[a + 1] <= off[a]) return "an empty node (off does not increase)";
    if (off[a + 1] > n) return "more list entries than features";
  }
  for (int i = 0; i < n; i++) seen[i] = 0;
  for (int a = 0; a < nn; a++)
    for (int32_t s = off[a]; s < off[a + 1]; s++) {
      if (idx[s] < 0 || idx[s] >= n) return "a feature index out of range";
      if (s > off[a] && idx[s] <= idx[s - 1] && !seen[idx[s]]) return "the feature indices of a node do not ascend";
      if (seen[idx[s]]) return "a feature listed twice";
      seen[idx[s]] = 1;
    }
  return nullptr;
}

// The offset rules of ccm_bow_pair_eval_resident's two mask arrays; n1[j] / n2[j]: the feature counts of job j's keyframes in the store.
static inline const char* bsm_check_masks(int J, const int32_t* off, const uint8_t* mask, const int32_t* n) {
  if (!off) return "null pointers";
  if (off[0] != 0) return "a mask offset array does not start at 0";
  for (int j = 0; j < J; j++) {
    if (off[j + 1] < off[j]) return "a mask offset array decreases";
    if (off[j + 1] - off[j] != n[j]) return "a mask is not as long as its keyframe's features";
  }
  if (off[J] > 0 && !mask) return "null pointers";
  return nullptr;
}

// A keyframe as the evaluator reads it: n features, their descriptors, and the feature vector in the store's form (16-bit indices).
struct BowKf { int n, nn; const int32_t* node; const int32_t* off; const uint16_t* idx; const uint8_t* desc; };

// The reduction of one query over the live features of one node of keyframe 2 that `skip` (nullable, per feature of keyframe 2) does not exclude, in list order.
// *n_live: the candidates met; *n_dist (nullable) is advanced by as many.
static inline BowBest bsm_reduce_host(const uint8_t* qdesc, const BowKf& k2, int node2, const uint8_t* live2, const uint8_t* skip, int* n_live, int32_t* n_dist) {
  BowBest b = bsm_empty();
  int cnt = 0;
  for (int32_t s = k2.off[node2]; s < k2.off[node2 + 1]; s++) {
    const int idx2 = k2.idx[s];
    if (!live2[idx2] || (skip && skip[idx2])) continue;
    bsm_update(b, bsm_hamming(qdesc, k2.desc + 32 * (size_t)idx2), idx2);
    cnt++;
  }
  *n_live = cnt;
  if (n_dist) *n_dist = (int32_t)((uint32_t)*n_dist + (uint32_t)cnt);   // wraps as the kernel's unsigned add does
  return b;
}

// One job of a search over the common nodes of two keyframes on the calling thread, for both evaluators (tri_search_math.h's too): the k1.n words zeroed, then the
// nodes of keyframe 1 that keyframe 2 has (at position b of its list) in ascending order and, of each, the features that are queries (mask byte set, or clear, as
// query_when_set says) in list order: word(idx1, b) gives the feature's word and advances the evaluator's counters.
template <class Word, class Eval>
static inline void fv_pair_walk_host(const BowKf& k1, const BowKf& k2, const uint8_t* mask1, bool query_when_set, Word* table, Eval word) {
  for (int i = 0; i < k1.n; i++) table[i] = 0;
  for (int a = 0; a < k1.nn; a++) {
    const int b = bsm_find_node(k2.node, k2.nn, k1.node[a]);
    if (b < 0) continue;
    for (int32_t s = k1.off[a]; s < k1.off[a + 1]; s++) {
      const int idx1 = k1.idx[s];
      if ((mask1[idx1] != 0) == query_when_set) table[idx1] = word(idx1, b);
    }
  }
}

// One job of ccm_bow_pair_eval_resident on the calling thread: table (k1.n words), *n_query, *n_dist.
static inline void bow_job_eval_host(const BowKf& k1, const BowKf& k2, const uint8_t* live1, const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  *n_query = *n_dist = 0;
  fv_pair_walk_host(k1, k2, live1, true, table, [&](int idx1, int b) {
    int n_live = 0;
    const BowBest r = bsm_reduce_host(k1.desc + 32 * (size_t)idx1, k2, b, live2, nullptr, &n_live, n_dist);
    ++*n_query;
    return bsm_pack(n_live ? BSM_EVALUATED : BSM_NO_CANDIDATE, r, b);
  });
}

// A whole call: job j is (k1[j], k2[j]) under the masks live1 + live1_off[j], live2 + live2_off[j]; its words start at table + live1_off[j].
static inline void bow_pair_eval_host(int J, const BowKf* k1, const BowKf* k2, const int32_t* live1_off, const uint8_t* live1, const int32_t* live2_off, const uint8_t* live2,
                                      uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  for (int j = 0; j < J; j++)
    bow_job_eval_host(k1[j], k2[j], live1 + live1_off[j], live2 + live2_off[j], table + live1_off[j], n_query + j, n_dist + j);
}
