// kfstore.h — the keyframe feature store's handle, shared by kfstore.hip (which fills it) and fuse.hip, bowsearch.hip, trisearch.hip and mappoint.hip (whose resident
// evaluators read it).  DESIGN.md §21, §23, §24, §25.
#pragma once
#include "common.h"
#include "kfstore_math.h"
#include <algorithm>
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

// kfstore_add_kernel's arguments (kfstore.hip): the call's staged arrays, then the store's
struct KfAddArgs {
  int stride;
  const int32_t *slot, *feat_off, *cell_off_in;
  const float *rec_in, *xy_in;
  const uint16_t* cell_idx_in;
  const uint8_t *oct_in, *desc_in;
  float *rec, *xy;
  int32_t *n, *n_in, *cell_off, *n_in_out;
  uint16_t* cell_idx;
  uint8_t *oct, *desc;
};

// the grid-building form of kfstore_add_kernel on the context's stream, one workgroup per keyframe: ccm_kfstore_add without a grid, and ccm_kfstore_ingest
// (kfingest.hip).  Internal to libccm_hip.so: not exported.
__attribute__((visibility("hidden"))) void kfstore_launch_add_build(ccm_ctx* ctx, const KfAddArgs& a, int M);

// the handle and the caller's context of every store call
inline int kfstore_ctx_ok(ccm_kfstore* st, ccm_ctx* ctx, const char* what) {
  if (!ctx) return CCM_E_ARG;
  if (!st) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": NULL handle");
  if (ctx->device != st->device) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": the context is on another device than the store");
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return CCM_OK;
}

// what add and ingest ask of the call's keys under the store's exclusive lock: no key twice, none live, a free slot for each
inline int kfstore_keys_ok(ccm_kfstore* st, ccm_ctx* ctx, const char* me, int M, const int64_t* keys) {
  std::vector<int64_t> sorted(keys, keys + M);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return ccm_set_error(ctx, CCM_E_STATE, std::string(me) + "a key is repeated within the call");
  for (int m = 0; m < M; m++)
    if (st->live.count(keys[m])) return ccm_set_error(ctx, CCM_E_STATE, std::string(me) + "a key is already in the store");
  if ((size_t)M > st->free_slots.size()) return ccm_set_error(ctx, CCM_E_STATE, std::string(me) + "fewer free slots than keyframes");
  return CCM_OK;
}
