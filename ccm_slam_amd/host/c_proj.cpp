// c_proj.cpp — C entry points of the six projected searches and their host evaluators; fuse_math.h compiled for the host
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include "../csrc/fuse_math.h"
#include <cstring>

using namespace ccmh_c;

extern "C" {
// SearchAndFuseBatch through C, and fuse_math.h compiled for the host
void* ccmh_fuse_sim3_create(int device, int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                            const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th,
                            int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc) {
  return guard_ptr([&]() -> void* {
    cslam::SearchAndFuseBatch::KeyFrames kf;
    kf.K = K; kf.rec = kf_rec; kf.feat_off = feat_off; kf.feat_xy = feat_xy; kf.feat_octave = feat_octave; kf.feat_desc = feat_desc; kf.cell_off = cell_off;
    kf.cell_idx = cell_idx; kf.Scw = Scw;
    const cslam::SearchAndFuseBatch::Points pt{P, pos, normal, min_dist, max_dist, pt_desc};
    return new cslam::SearchAndFuseBatch(ctx_or_null(device), kf, pt, nlevels, scale_factors, logScaleFactor, th);
  });
}
int ccmh_fuse_sim3_table(void* h, uint32_t* table, int32_t* n_valid, int32_t* n_hit) {
  if (!h) return -1;
  const cslam::SearchAndFuseBatch& b = *as<cslam::SearchAndFuseBatch>(h);
  copy_out(table, b.table());
  if (n_valid && b.keyframes()) std::memcpy(n_valid, b.nValid().data(), (size_t)b.keyframes() * 4);
  if (n_hit && b.keyframes()) std::memcpy(n_hit, b.nHit().data(), (size_t)b.keyframes() * 4);
  return 0;
}
int ccmh_fuse_sim3_resolve(void* h, int k, const uint8_t* skip_now, const uint8_t* desc_now, int n_pts, int32_t* best_idx, int32_t* best_dist) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    std::vector<int32_t> bi, bd;
    const int n = as<cslam::SearchAndFuseBatch>(h)->resolve(k, skip_now, desc_now, bi, bd);
    return copy_best(n, n_pts, bi, bd, best_idx, best_dist);
  });
}
long long ccmh_fuse_sim3_n_reeval(void* h) { return h ? as<cslam::SearchAndFuseBatch>(h)->n_reeval() : -1; }
void ccmh_fuse_sim3_destroy(void* h) { delete as<cslam::SearchAndFuseBatch>(h); }
int ccmh_fuse_sim3_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                             const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th,
                             int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table,
                             int32_t* n_valid, int32_t* n_hit, float* uv, int32_t* n_cand) {
  return cslam::fuse_sim3_eval_host(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, Scw, nlevels, scale_factors, logScaleFactor, th, P, pos, normal,
                                    min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv, n_cand);
}
void ccmh_fuse_sim3_decompose(const float* Scw12, float* pose15) { fsm_decompose_scw(Scw12, pose15); }

// SearchInNeighborsBatch through C, and fuse_math.h compiled for the host
void* ccmh_fuse_pose_create(int device, int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                            const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
                            float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                            const uint8_t* pt_desc, int n_calls, const int32_t* target, int current, int n_current) {
  return guard_ptr([&]() -> void* {
    cslam::SearchInNeighborsBatch::KeyFrames kf;
    kf.K = K; kf.rec = kf_rec; kf.feat_off = feat_off; kf.feat_xy = feat_xy; kf.feat_octave = feat_octave; kf.feat_desc = feat_desc; kf.cell_off = cell_off;
    kf.cell_idx = cell_idx; kf.pose = pose;
    const cslam::SearchInNeighborsBatch::Points pt{P, pos, normal, min_dist, max_dist, pt_desc};
    return new cslam::SearchInNeighborsBatch(ctx_or_null(device), kf, n_calls, target, current, pt, n_current, nlevels, scale_factors,
                                             inv_level_sigma2, logScaleFactor, th);
  });
}
int ccmh_fuse_pose_table(void* h, uint32_t* table, int32_t* n_valid, int32_t* n_hit) {
  if (!h) return -1;
  const cslam::SearchInNeighborsBatch& b = *as<cslam::SearchInNeighborsBatch>(h);
  copy_out(table, b.table());
  copy_out(n_valid, b.nValid());
  copy_out(n_hit, b.nHit());
  return 0;
}
int ccmh_fuse_pose_resolve(void* h, int c, const uint8_t* skip_now, const uint8_t* desc_now, int n_pts, int32_t* best_idx, int32_t* best_dist) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    std::vector<int32_t> bi, bd;
    const int n = as<cslam::SearchInNeighborsBatch>(h)->resolve(c, skip_now, desc_now, bi, bd);
    return copy_best(n, n_pts, bi, bd, best_idx, best_dist);
  });
}
int ccmh_fuse_pose_resolve_current(void* h, int n, const int32_t* slot, const uint8_t* skip_now, const uint8_t* desc_now, const float* pos, const float* normal,
                                   const float* min_dist, const float* max_dist, const uint8_t* desc, int32_t* best_idx, int32_t* best_dist) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    const cslam::SearchInNeighborsBatch::Points fresh{n, pos, normal, min_dist, max_dist, desc};
    std::vector<int32_t> bi, bd;
    const int nf = as<cslam::SearchInNeighborsBatch>(h)->resolve_current(n, slot, skip_now, desc_now, fresh, bi, bd);
    return copy_best(nf, n, bi, bd, best_idx, best_dist);
  });
}
long long ccmh_fuse_pose_n_reeval(void* h) { return h ? as<cslam::SearchInNeighborsBatch>(h)->n_reeval() : -1; }
long long ccmh_fuse_pose_n_unpredicted(void* h) { return h ? as<cslam::SearchInNeighborsBatch>(h)->n_unpredicted() : -1; }
void ccmh_fuse_pose_destroy(void* h) { delete as<cslam::SearchInNeighborsBatch>(h); }
int ccmh_fuse_pose_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                             const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
                             float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                             const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid,
                             int32_t* n_hit, float* uv, int32_t* n_cand) {
  return cslam::fuse_pose_eval_host(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, pose, nlevels, scale_factors, inv_level_sigma2, logScaleFactor,
                                    th, P, pos, normal, min_dist, max_dist, pt_desc, J, job_kf, job_pt0, job_n, table, n_valid, n_hit, uv, n_cand);
}

int ccmh_fuse_sim3_eval_resident_host(void* store, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th,
                                      int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc,
                                      uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!store) return -1;
  return cslam::fuse_sim3_eval_resident_host(*as<cslam::KeyFrameStore>(store), K, keys, Scw, nlevels, scale_factors, logScaleFactor, th, P, pos, normal, min_dist,
                                             max_dist, pt_desc, table, n_valid, n_hit, uv);
}
int ccmh_fuse_pose_eval_resident_host(void* store, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
                                      float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                                      const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table,
                                      int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!store) return -1;
  return cslam::fuse_pose_eval_resident_host(*as<cslam::KeyFrameStore>(store), K, keys, pose, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th, P, pos,
                                             normal, min_dist, max_dist, pt_desc, J, job_kf, job_pt0, job_n, table, n_valid, n_hit, uv);
}
void* ccmh_fuse_sim3_create_resident(void* store, int device, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor,
                                     float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc) {
  if (!store) return nullptr;
  return guard_ptr([&]() -> void* {
    const cslam::SearchAndFuseBatch::Points pt{P, pos, normal, min_dist, max_dist, pt_desc};
    return new cslam::SearchAndFuseBatch(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), K, keys, Scw, pt, nlevels,
                                         scale_factors, logScaleFactor, th);
  });
}
void* ccmh_fuse_pose_create_resident(void* store, int device, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors,
                                     const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* pt_desc, int n_calls, const int32_t* target, int current, int n_current) {
  if (!store) return nullptr;
  return guard_ptr([&]() -> void* {
    const cslam::SearchInNeighborsBatch::Points pt{P, pos, normal, min_dist, max_dist, pt_desc};
    return new cslam::SearchInNeighborsBatch(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), K, keys, pose, n_calls, target,
                                             current, pt, n_current, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th);
  });
}

// the two projected searches of ComputeSim3 through C: host evaluators, ssm_derive, the two mirrors
int ccmh_sim3_project_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                                const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels,
                                const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  return cslam::sim3_project_eval_host(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, Scw, skip_off, feat_skip, nlevels, scale_factors,
                                       logScaleFactor, th, P, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv);
}
int ccmh_sim3_pair_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                             const int32_t* cell_off, const int32_t* cell_idx, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P,
                             const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4,
                             const float* job_src_pose, const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid,
                             int32_t* n_hit, float* uv) {
  return cslam::sim3_pair_eval_host(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, nlevels, scale_factors, logScaleFactor, th, P, pos, min_dist,
                                    max_dist, pt_desc, J, job_kf, job_K4, job_src_pose, job_T, job_pt0, job_n, table, n_valid, n_hit, uv);
}
int ccmh_sim3_project_eval_resident_host(void* store, int K, const int64_t* keys, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels,
                                         const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                         const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!store) return -1;
  return cslam::sim3_project_eval_resident_host(*as<cslam::KeyFrameStore>(store), K, keys, Scw, skip_off, feat_skip, nlevels, scale_factors, logScaleFactor, th, P,
                                                pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv);
}
int ccmh_sim3_pair_eval_resident_host(void* store, int K, const int64_t* keys, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P,
                                      const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf,
                                      const float* job_K4, const float* job_src_pose, const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table,
                                      int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!store) return -1;
  return cslam::sim3_pair_eval_resident_host(*as<cslam::KeyFrameStore>(store), K, keys, nlevels, scale_factors, logScaleFactor, th, P, pos, min_dist, max_dist,
                                             pt_desc, J, job_kf, job_K4, job_src_pose, job_T, job_pt0, job_n, table, n_valid, n_hit, uv);
}
void ccmh_ssm_derive(float s12, const float* R12, const float* t12, float* sR12, float* sR21, float* t21) { ssm_derive(s12, R12, t12, sR12, sR21, t21); }
void* ccmh_sim3_project_create(void* store, int device, int64_t key, const float* Scw12, const uint8_t* matched0, int nlevels, const float* scale_factors,
                               float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                               const uint8_t* pt_desc) {
  if (!store) return nullptr;
  return guard_ptr([&]() -> void* {
    const cslam::Sim3ProjectionSearch::Points pt{P, pos, normal, min_dist, max_dist, pt_desc};
    return new cslam::Sim3ProjectionSearch(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), key, Scw12, pt, matched0, nlevels,
                                           scale_factors, logScaleFactor, th);
  });
}
int ccmh_sim3_project_table(void* h, uint32_t* table, int32_t* n_valid, int32_t* n_hit) {
  if (!h) return -1;
  const cslam::Sim3ProjectionSearch& b = *as<cslam::Sim3ProjectionSearch>(h);
  copy_out(table, b.table());
  if (n_valid) *n_valid = b.nValid();
  if (n_hit) *n_hit = b.nHit();
  return 0;
}
int ccmh_sim3_project_resolve(void* h, const uint8_t* skip_now, const int32_t* existing_idx, int n_feat, int32_t* matched, int n_pts, int32_t* best_idx, int32_t* remap) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    cslam::Sim3ProjectionSearch& b = *as<cslam::Sim3ProjectionSearch>(h);
    if (n_pts != b.points() || n_feat != b.features()) return -1001;
    std::vector<int32_t> bi, rm;
    const int n = b.resolve(skip_now, existing_idx, matched, bi, rm);
    if (n_pts) { std::memcpy(best_idx, bi.data(), bi.size() * 4); std::memcpy(remap, rm.data(), rm.size() * 4); }
    return n;
  });
}
long long ccmh_sim3_project_n_reeval(void* h) { return h ? as<cslam::Sim3ProjectionSearch>(h)->n_reeval() : -1; }
void ccmh_sim3_project_destroy(void* h) { delete as<cslam::Sim3ProjectionSearch>(h); }
int ccmh_search_by_sim3_resident(void* store, int device, int64_t key1, int64_t key2, int N1, const uint8_t* live1, const float* pos1, const float* min1, const float* max1,
                                 const uint8_t* desc1, const float* pose1, int N2, const uint8_t* live2, const float* pos2, const float* min2, const float* max2,
                                 const uint8_t* desc2, const float* pose2, float s12, const float* R12, const float* t12, const int32_t* matches12_in, int nlevels,
                                 const float* scale_factors, float logScaleFactor, float th, int32_t* matches12, int32_t* vn1, int32_t* vn2, int32_t* n_valid2,
                                 int32_t* n_hit2) {
  if (!store) return -1000;
  return guard_int([&]() -> int {
    cslam::SearchBySim3Batch::Side a, b;
    a.N = N1; a.live = live1; a.pos = pos1; a.min_dist = min1; a.max_dist = max1; a.desc = desc1; a.pose = pose1;
    b.N = N2; b.live = live2; b.pos = pos2; b.min_dist = min2; b.max_dist = max2; b.desc = desc2; b.pose = pose2;
    const cslam::SearchBySim3Batch r(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), key1, key2, a, b, s12, R12, t12,
                                     matches12_in, nlevels, scale_factors, logScaleFactor, th);
    if (matches12 && N1) std::memcpy(matches12, r.matches12().data(), (size_t)N1 * 4);
    if (vn1 && N1) std::memcpy(vn1, r.vnMatch1().data(), (size_t)N1 * 4);
    if (vn2 && N2) std::memcpy(vn2, r.vnMatch2().data(), (size_t)N2 * 4);
    if (n_valid2) std::memcpy(n_valid2, r.nValid().data(), 8);
    if (n_hit2) std::memcpy(n_hit2, r.nHit().data(), 8);
    return r.nFound();
  });
}
}  // extern "C"
