// covis_math.h — the rules of KeyFrame::UpdateConnections (cslam/src/KeyFrame.cpp:629-711) run over a set of keyframes in a given walk order, with the
// AddConnection / UpdateBestCovisibles calls (KeyFrame.cpp:392-426) the set's keyframes make on each other, host + device.  The kernels of covis.hip run
// these lines; the host evaluator of cslam::CovisibilityBatch (host/ccm_host.cpp) compiles them with g++.  Integers only.
//
// Keyframes 0 .. n_kf - 1 are the set in walk order, n_kf .. n_all - 1 the observers outside it; order_key[n_all] (distinct) stands for the pointer order of
// std::map<kfptr, ...> and of sort on pair<int, kfptr>.  C_i is keyframe i's own count row, E_i the keyframes it calls AddConnection on:
//   count       an entry of i's list counts iff it is not null and its point is not bad; every observer j != i of the point gets C_i[j] += 1
//   events      E_i = { j : C_i[j] >= th }, or, when that is empty, the one j of maximal count, ties to the smallest order_key (strict > in key order)
//   reach       AddConnection(i, C_j[i]) of j in E-relation with i survives in i's final state iff j is walked after i's own step, which replaces the map;
//               a keyframe with an empty C_i returns before replacing anything, so every call reaches it
//   order       descending by (weight, order_key): the ascending sort read back through push_front
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define COVIS_HD __host__ __device__ inline
#else
#define COVIS_HD inline
#endif

enum { COVIS_EMPTY = 1, COVIS_FALLBACK = 2, COVIS_CHANGED = 4 };

// pMP != nullptr && !pMP->isBad()
COVIS_HD bool covis_entry_counts(int32_t pt, uint32_t skip) { return pt >= 0 && !skip; }
// mit->first->mId == this->mId: continue
COVIS_HD bool covis_observer_counts(int32_t j, int32_t i) { return j != i; }
// `if (mit->second > nmax)` while the map is walked in key order: a later key replaces the best only with a larger count
COVIS_HD bool covis_fallback_better(uint32_t c, int32_t key, uint32_t best_c, int32_t best_key) { return c > best_c || (c == best_c && key < best_key); }
// is column `col` with count c one of the row's events; n_ge = entries of the row with count >= th, fb_col = the fallback's column when n_ge == 0
COVIS_HD bool covis_is_event(uint32_t c, int32_t col, uint32_t th, int32_t n_ge, int32_t fb_col) { return n_ge > 0 ? c >= th : col == fb_col; }
// does AddConnection from keyframe j of the set reach the final state of keyframe i of the set
COVIS_HD bool covis_reaches(int32_t j, int32_t i, bool i_empty) { return i_empty || j > i; }
// larger key = earlier in mvpOrderedConnectedKeyFrames; 0 is below every real key (weights are >= 1)
COVIS_HD uint64_t covis_sort_key(uint32_t w, int32_t order_key) { return ((uint64_t)w << 32) | (uint64_t)((uint32_t)order_key ^ 0x80000000u); }
// position of `target` in the ascending columns col[lo .. hi), -1 if absent
COVIS_HD int32_t covis_find(const int32_t* col, int32_t lo, int32_t hi, int32_t target) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    const int32_t v = col[mid];
    if (v == target) return mid;
    if (v < target) lo = mid + 1; else hi = mid;
  }
  return -1;
}
// number of columns col[lo .. hi) below `target`
COVIS_HD int32_t covis_lower(const int32_t* col, int32_t lo, int32_t hi, int32_t target) {
  const int32_t lo0 = lo;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (col[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo - lo0;
}
// size of the ordered list from the row's facts
COVIS_HD int32_t covis_ord_size(bool changed, int32_t final_size, int32_t row_size, int32_t n_ge) { return changed ? final_size : row_size == 0 ? 0 : n_ge > 0 ? n_ge : 1; }

#include <algorithm>
#include <vector>
// the argument checks shared by ccm_covis_update and the host evaluator: nullptr, or what is wrong
inline const char* covis_check_args(int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt,
                                    const int32_t* obs_off, const int32_t* obs_kf, int th, int cap) {
  if (n_kf < 1 || n_all < n_kf || n_pt < 0 || th < 1 || cap < 0 || !order_key || !list_off) return "bad args";
  if (list_off[0] != 0) return "list_off[0] != 0";
  for (int i = 0; i < n_kf; i++) if (list_off[i + 1] < list_off[i]) return "list_off decreases";
  const int32_t NL = list_off[n_kf];
  if (NL && (!list_pt || !list_skip)) return "bad args";
  if (n_pt && !obs_off) return "bad args";
  if (n_pt && obs_off[0] != 0) return "obs_off[0] != 0";
  for (int p = 0; p < n_pt; p++) if (obs_off[p + 1] < obs_off[p]) return "obs_off decreases";
  const int32_t NO = n_pt ? obs_off[n_pt] : 0;
  if (NO && !obs_kf) return "bad args";
  for (int32_t e = 0; e < NL; e++) if (list_pt[e] >= n_pt) return "point index out of range";
  for (int32_t k = 0; k < NO; k++) if (obs_kf[k] < 0 || obs_kf[k] >= n_all) return "observer out of range";
  std::vector<int32_t> keys(order_key, order_key + n_all);
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return "order_key repeats a value";
  return nullptr;
}
