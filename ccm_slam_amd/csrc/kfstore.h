// kfstore.h — the keyframe feature store's handle, shared by kfstore.hip (which fills it) and fuse.hip, bowsearch.hip, trisearch.hip and mappoint.hip (whose resident
// evaluators read it).  DESIGN.md §21, §23, §24, §25.
#pragma once
#include "common.h"
#include "kfstore_math.h"
#include <shared_mutex>
#include <unordered_map>

struct ccm_kfstore {
  int device = 0, max_kf = 0, max_feat = 0, stride = 0;   // stride: a slot's features, max_feat rounded up to KFG_FEAT_ALIGN
  std::shared_mutex mu;                                    // resident evaluators and get shared, add / erase / clear exclusive
  // device: one array per field, indexed by slot (features at slot * stride)
  float* d_rec = nullptr;          // [10 max_kf]
  int32_t* d_n = nullptr;          // [max_kf] features
  int32_t* d_n_in = nullptr;       // [max_kf] features in the grid = cell_off[FSM_CELLS]
  int32_t* d_cell_off = nullptr;   // [(FSM_CELLS + 1) max_kf]
  uint16_t* d_cell_idx = nullptr;  // [stride max_kf]
  float* d_xy = nullptr;           // [2 stride max_kf]
  uint8_t* d_oct = nullptr;        // [stride max_kf]
  uint8_t* d_desc = nullptr;       // [32 stride max_kf]
  // the keyframe's DBoW2::FeatureVector (ccm_kfstore_set_featvec), as the caller gave it: a node has at least one feature, so nn <= n
  int32_t* d_fv_node = nullptr;    // [stride max_kf] node ids, ascending
  int32_t* d_fv_off = nullptr;     // [(stride + 1) max_kf] offsets of the nodes' features
  uint16_t* d_fv_idx = nullptr;    // [stride max_kf] the features of the nodes, ascending inside a node
  // host
  std::vector<int32_t> h_n;                // [max_kf] d_n as the adds wrote it: the feature count a mask of ccm_sim3_project_eval_resident is held to
  std::vector<int32_t> h_fv_nn;            // [max_kf] the nodes of the slot's feature vector; -1: the tenant has none
  std::unordered_map<int64_t, int> live;   // key -> slot
  std::vector<int> free_slots;             // a stack: the slot freed last is taken first
};
