// c_vocab.cpp — C entry points of the vocabulary transform, the keyframe database, the optimisers and the f32 <-> f64 boundary (ccm_convert.h)
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include "ccm_convert.h"
#include <cstring>
#include <map>

using namespace ccmh_c;

extern "C" {
int ccmh_local_ba(int device, int n_cam, int n_pt, int n_edge, double* cam_qt, const uint8_t* cam_fixed, const double* cam_K,
                  double* pt_xyz, const int32_t* e_cam, const int32_t* e_pt, const double* e_obs, const double* e_info, uint8_t* to_erase) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    cslam::BAProblem p;
    p.cam_qt.assign(cam_qt, cam_qt + 7 * (size_t)n_cam); p.cam_fixed.assign(cam_fixed, cam_fixed + n_cam);
    p.cam_K.assign(cam_K, cam_K + 4 * (size_t)n_cam); p.pt_xyz.assign(pt_xyz, pt_xyz + 3 * (size_t)n_pt);
    p.e_cam.assign(e_cam, e_cam + n_edge); p.e_pt.assign(e_pt, e_pt + n_edge);
    p.e_obs.assign(e_obs, e_obs + 2 * (size_t)n_edge); p.e_info.assign(e_info, e_info + n_edge);
    std::vector<uint8_t> er;
    cslam::Optimizer::LocalBundleAdjustmentClient(ctx, p, nullptr, er);
    std::memcpy(cam_qt, p.cam_qt.data(), sizeof(double) * p.cam_qt.size());
    std::memcpy(pt_xyz, p.pt_xyz.data(), sizeof(double) * p.pt_xyz.size());
    std::memcpy(to_erase, er.data(), er.size());
    return 0;
  });
}

int ccmh_optimize_sim3(int device, double* sim3, int n, const double* P1c, const double* P2c, const double* obs1, const double* obs2,
                       const double* info1, const double* info2, const double* K1, const double* K2, float th2, int fix_scale, uint8_t* keep) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    std::vector<uint8_t> k;
    const int nin = cslam::Optimizer::OptimizeSim3(ctx, sim3, n, P1c, P2c, obs1, obs2, info1, info2, K1, K2, th2, fix_scale != 0, k);
    if (n) std::memcpy(keep, k.data(), k.size());
    return nin;
  });
}

int ccmh_bow_transform(int device, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc,
                       const int32_t* word_id, const double* weight, const uint8_t* desc, int N, int levelsup, int32_t* bow_ids,
                       double* bow_vals, int32_t* fv_nodes, int32_t* fv_off, int32_t* fv_idx, int32_t* sizes /* [n_bow, n_fv_nodes, n_fv_idx] */) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    cslam::ORBVocabulary voc(ctx, n_nodes, L, child_off, child_id, node_desc, word_id, weight);
    cslam::BowVector v; cslam::FeatureVector fv;
    voc.transform(desc, N, v, fv, levelsup);
    std::memcpy(bow_ids, v.word.data(), v.word.size() * 4); std::memcpy(bow_vals, v.value.data(), v.value.size() * 8);
    std::memcpy(fv_nodes, fv.node.data(), fv.node.size() * 4); std::memcpy(fv_off, fv.off.data(), fv.off.size() * 4);
    std::memcpy(fv_idx, fv.idx.data(), fv.idx.size() * 4);
    sizes[0] = (int32_t)v.word.size(); sizes[1] = (int32_t)fv.node.size(); sizes[2] = (int32_t)fv.idx.size();
    return 0;
  });
}

// KeyFrameDatabase::Detect*Candidates through the mirror on a database handle of libccm_hip.so (the Python KeyFrameDatabase's).  kind 0 = loop
// (self_key, allow / n_allow (n_allow < 0: every keyframe), exclude), 1 = map match (exclude_groups), 2 = relocalisation.  Neighbours as a table:
// nb_key[i] has the neighbours nb_list[nb_off[i] .. nb_off[i+1]); keys absent from it have none.  Returns the number of candidates (<= cap written).
int ccmh_kfdb_detect(void* db, int device, int kind, int n, const int32_t* word, const double* value, float min_score, int64_t self_key,
                     const int64_t* allow, int n_allow, const int64_t* exclude, int n_exclude, uint64_t exclude_groups, int n_nb_keys,
                     const int64_t* nb_key, const int32_t* nb_off, const int64_t* nb_list, int64_t* out, int cap) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    cslam::KeyFrameDatabase kfdb(as<ccm_kfdb>(db));
    cslam::BowVector v; v.word.assign(word, word + n); v.value.assign(value, value + n);
    std::map<int64_t, int> row;
    for (int i = 0; i < n_nb_keys; i++) row[nb_key[i]] = i;
    auto nbs = [&](int64_t k, std::vector<int64_t>& o) {
      auto it = row.find(k);
      if (it != row.end()) o.assign(nb_list + nb_off[it->second], nb_list + nb_off[it->second + 1]);
    };
    std::vector<int64_t> r;
    if (kind == 0) {
      std::vector<int64_t> ex(exclude, exclude + n_exclude), al;
      if (n_allow >= 0) al.assign(allow, allow + n_allow);
      r = kfdb.DetectLoopCandidates(ctx, self_key, v, min_score, n_allow >= 0 ? &al : nullptr, ex, nbs);
    } else if (kind == 1) {
      r = kfdb.DetectMapMatchCandidates(ctx, v, min_score, exclude_groups, nbs);
    } else {
      r = kfdb.DetectRelocalizationCandidates(ctx, v, nbs);
    }
    for (int i = 0; i < (int)r.size() && i < cap; i++) out[i] = r[i];
    return (int)r.size();
  });
}

// C entry points of the f32 <-> f64 boundary (ccm_convert.h) for the tests and for non-C++ callers

void ccmh_to_se3quat(const float* Tcw16, double* qt7) { ccmh::toSE3Quat(Tcw16, qt7); }
void ccmh_se3quat_to_cvmat(const double* qt7, float* Tcw16) { ccmh::toCvMat(qt7, Tcw16); }
void ccmh_sim3_to_cvse3(const double* s8, float* Tcw16) { ccmh::sim3ToCvSE3(s8, Tcw16); }
}  // extern "C"
