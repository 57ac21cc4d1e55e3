// c_map.cpp — C entry points of Sim3MapCorrection, GbaMapUpdate, CovisibilityBatch and KeyFrameCullingBatch
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include "mirror_internal.h"
#include <cstring>

using namespace ccmh_c;

extern "C" {
// Sim3MapCorrection through C
static cslam::Sim3MapCorrection::Points mk_s3c_points(int n_pt, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const int32_t* obs_off,
                                                      const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level) {
  cslam::Sim3MapCorrection::Points p;
  if (n_pt < 0 || (n_pt > 0 && (!pos || !normal || !min_dist || !max_dist || !obs_off || !ref_kf || !ref_level))) throw cslam::infrastructure_ex("points");
  const size_t n = (size_t)n_pt;
  p.obs_off.assign(1, 0);
  if (n) {
    p.pos.assign(pos, pos + 3 * n); p.normal.assign(normal, normal + 3 * n); p.min_dist.assign(min_dist, min_dist + n); p.max_dist.assign(max_dist, max_dist + n);
    p.obs_off.assign(obs_off, obs_off + n + 1); p.ref_kf.assign(ref_kf, ref_kf + n); p.ref_level.assign(ref_level, ref_level + n);
    if (obs_off[n] < 0 || (obs_off[n] > 0 && !obs_kf)) throw cslam::infrastructure_ex("points");
    p.obs_kf.assign(obs_kf, obs_kf + obs_off[n]);
  }
  return p;
}
void* ccmh_sim3corr_create_loop(int device, int n_kf, int n_obs_kf, const float* Tiw, const float* center, int cur, const float* Twc, const double* Scw,
                                const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt, const float* pos, const float* normal,
                                const float* min_dist, const float* max_dist, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level,
                                const float* scale_factors, int n_levels) {
  return guard_ptr([&]() -> void* {
    if (n_kf < 1 || n_obs_kf < n_kf || !Tiw || !center || !Twc || !Scw || !list_off || n_levels < 1 || !scale_factors) return nullptr;
    const int ne = list_off[n_kf];
    if (ne < 0 || (ne > 0 && (!list_pt || !list_skip))) return nullptr;
    return new cslam::Sim3MapCorrection(ctx_or_null(device), n_kf, std::vector<float>(Tiw, Tiw + 12 * (size_t)n_kf),
                                        std::vector<float>(center, center + 3 * (size_t)n_obs_kf), cur, Twc, Scw, std::vector<int32_t>(list_off, list_off + n_kf + 1),
                                        std::vector<int32_t>(list_pt, list_pt + ne), std::vector<uint8_t>(list_skip, list_skip + ne),
                                        mk_s3c_points(n_pt, pos, normal, min_dist, max_dist, obs_off, obs_kf, ref_kf, ref_level),
                                        std::vector<float>(scale_factors, scale_factors + n_levels));
  });
}
void* ccmh_sim3corr_create_epilogue(int device, int n_kf, int n_obs_kf, const float* center, const double* S_non, const double* S_cor, const int32_t* pt_kf, int n_pt,
                                    const float* pos, const float* normal, const float* min_dist, const float* max_dist, const int32_t* obs_off, const int32_t* obs_kf,
                                    const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels) {
  return guard_ptr([&]() -> void* {
    if (n_kf < 1 || n_obs_kf < n_kf || !center || !S_non || !S_cor || n_pt < 0 || (n_pt > 0 && !pt_kf) || n_levels < 1 || !scale_factors) return nullptr;
    return new cslam::Sim3MapCorrection(ctx_or_null(device), n_kf, std::vector<float>(center, center + 3 * (size_t)n_obs_kf),
                                        std::vector<double>(S_non, S_non + 8 * (size_t)n_kf), std::vector<double>(S_cor, S_cor + 8 * (size_t)n_kf),
                                        std::vector<int32_t>(pt_kf, pt_kf + n_pt), mk_s3c_points(n_pt, pos, normal, min_dist, max_dist, obs_off, obs_kf, ref_kf, ref_level),
                                        std::vector<float>(scale_factors, scale_factors + n_levels));
  });
}
int ccmh_sim3corr_results(void* h, float* pos, float* normal, float* min_dist, float* max_dist, int32_t* tag, float* Tiw_new, float* center_new, double* S_non,
                          double* S_cor) {
  if (!h) return -1;
  const cslam::Sim3MapCorrection& c = *as<cslam::Sim3MapCorrection>(h);
  copy_out(pos, c.points().pos); copy_out(normal, c.points().normal); copy_out(min_dist, c.points().min_dist); copy_out(max_dist, c.points().max_dist);
  copy_out(tag, c.tag()); copy_out(Tiw_new, c.poses()); copy_out(center_new, c.centers()); copy_out(S_non, c.nonCorrectedSim3()); copy_out(S_cor, c.correctedSim3());
  return 0;
}
void ccmh_sim3corr_destroy(void* h) { delete as<cslam::Sim3MapCorrection>(h); }
int ccmh_sim3_correct_map_host(int n_kf, const float* Tiw, int cur, const float* Twc, const double* Scw, double* S_non, double* S_cor, int n_obs_kf, const float* kf_center,
                               const int32_t* kf_rank, int n_pt, const float* pos, const int32_t* owner, const int32_t* owner_rank, const int32_t* obs_off,
                               const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, float* pos_out,
                               float* normal, float* min_dist, float* max_dist, float* Tiw_new, float* center_new) {
  return cslam::sim3_correct_map_host(n_kf, Tiw, cur, Twc, Scw, S_non, S_cor, n_obs_kf, kf_center, kf_rank, n_pt, pos, owner, owner_rank, obs_off, obs_kf, ref_kf, ref_level,
                                      scale_factors, n_levels, pos_out, normal, min_dist, max_dist, Tiw_new, center_new);
}

// GbaMapUpdate through C
void* ccmh_gbaupd_create(int device, int n_kf, int n_origins, const int32_t* origins, const int32_t* child_off, const int32_t* child_kf, const int32_t* kf_cam, const float* Tcw,
                         const float* Twc, int n_pt, const float* pos, const int32_t* vert, const int32_t* ref_kf, int n_cam, const double* cam_qt, int n_lm,
                         const double* pt_xyz) {
  return guard_ptr([&]() -> void* {
    if (n_kf < 1 || n_origins < 1 || !origins || !child_off || !kf_cam || !Tcw || !Twc || n_pt < 0 || (n_pt > 0 && (!pos || !vert || !ref_kf)) || n_cam < 1 || !cam_qt ||
        n_lm < 0 || (n_lm > 0 && !pt_xyz))
      return nullptr;
    const int ne = child_off[n_kf];
    if (ne < 0 || (ne > 0 && !child_kf)) return nullptr;
    cslam::GbaMapUpdate::Graph g;
    g.origins.assign(origins, origins + n_origins); g.child_off.assign(child_off, child_off + n_kf + 1); g.child_kf.assign(child_kf, child_kf + ne);
    g.kf_cam.assign(kf_cam, kf_cam + n_kf); g.Tcw.assign(Tcw, Tcw + 12 * (size_t)n_kf); g.Twc.assign(Twc, Twc + 12 * (size_t)n_kf);
    cslam::GbaMapUpdate::Points p;
    if (n_pt) { p.pos.assign(pos, pos + 3 * (size_t)n_pt); p.vert.assign(vert, vert + n_pt); p.ref_kf.assign(ref_kf, ref_kf + n_pt); }
    return new cslam::GbaMapUpdate(ctx_or_null(device), std::move(g), std::move(p), std::vector<double>(cam_qt, cam_qt + 7 * (size_t)n_cam),
                                   n_lm ? std::vector<double>(pt_xyz, pt_xyz + 3 * (size_t)n_lm) : std::vector<double>());
  });
}
int ccmh_gbaupd_sizes(void* h, int64_t* out4) {
  if (!h || !out4) return -1;
  const cslam::GbaMapUpdate& u = *as<cslam::GbaMapUpdate>(h);
  out4[0] = (int64_t)u.order().size(); out4[1] = u.reachedTwice(); out4[2] = u.staleReferences(); out4[3] = (int64_t)u.status().size();
  return 0;
}
int ccmh_gbaupd_results(void* h, int32_t* order, int32_t* parent, float* T_new, float* Twc_new, float* pos, uint8_t* status) {
  if (!h) return -1;
  const cslam::GbaMapUpdate& u = *as<cslam::GbaMapUpdate>(h);
  copy_out(order, u.order()); copy_out(parent, u.parents()); copy_out(T_new, u.poses()); copy_out(Twc_new, u.inverses()); copy_out(pos, u.positions()); copy_out(status, u.status());
  return 0;
}
void ccmh_gbaupd_destroy(void* h) { delete as<cslam::GbaMapUpdate>(h); }
int ccmh_gba_apply_map_host(int n_kf, const int32_t* kf_parent, const int32_t* kf_cam, const float* Tcw_old, const float* Twc_old, int n_pt, const float* pos,
                            const int32_t* pt_vert, const int32_t* pt_ref, int n_cam, const double* cam_qt, int n_lm, const double* pt_xyz, float* T_new, float* Twc_new,
                            float* pos_out, uint8_t* pt_status) {
  return cslam::gba_apply_map_host(n_kf, kf_parent, kf_cam, Tcw_old, Twc_old, n_pt, pos, pt_vert, pt_ref, n_cam, cam_qt, n_lm, pt_xyz, T_new, Twc_new, pos_out, pt_status);
}

// CovisibilityBatch through C
void* ccmh_covis_create(int device, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt,
                        const int32_t* obs_off, const int32_t* obs_kf, int th) {
  return guard_ptr([&]() -> void* {
    if (n_kf < 1 || n_all < n_kf || n_pt < 0 || !order_key || !list_off || (n_pt > 0 && !obs_off)) return nullptr;
    const int ne = list_off[n_kf], no = n_pt ? obs_off[n_pt] : 0;
    if (ne < 0 || no < 0 || (ne > 0 && (!list_pt || !list_skip)) || (no > 0 && !obs_kf)) return nullptr;
    return new cslam::CovisibilityBatch(ctx_or_null(device), n_kf, std::vector<int32_t>(order_key, order_key + n_all),
                                        std::vector<int32_t>(list_off, list_off + n_kf + 1), std::vector<int32_t>(list_pt, list_pt + ne),
                                        std::vector<uint8_t>(list_skip, list_skip + ne), n_pt ? std::vector<int32_t>(obs_off, obs_off + n_pt + 1) : std::vector<int32_t>(1, 0),
                                        std::vector<int32_t>(obs_kf, obs_kf + no), th);
  });
}
int ccmh_covis_sizes(void* h, int64_t* out5) {
  if (!h || !out5) return -1;
  const cslam::CovisibilityBatch& c = *as<cslam::CovisibilityBatch>(h);
  out5[0] = c.size(); out5[1] = (int64_t)c.rowKf().size(); out5[2] = (int64_t)c.weightKf().size(); out5[3] = (int64_t)c.orderedKf().size(); out5[4] = (int64_t)c.outsideCalls().size();
  return 0;
}
int ccmh_covis_results(void* h, int32_t* flags, int32_t* row_off, int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off,
                       int32_t* ord_kf, int32_t* ord_w, int32_t* outside) {
  if (!h) return -1;
  const cslam::CovisibilityBatch& c = *as<cslam::CovisibilityBatch>(h);
  copy_out(flags, c.allFlags()); copy_out(row_off, c.rowOff()); copy_out(col, c.rowKf()); copy_out(count, c.rowCount()); copy_out(fw_off, c.weightOff()); copy_out(fw_col, c.weightKf());
  copy_out(fw_w, c.weight()); copy_out(ord_off, c.orderedOff()); copy_out(ord_kf, c.orderedKf()); copy_out(ord_w, c.orderedWeight());
  if (outside) for (size_t k = 0; k < c.outsideCalls().size(); k++) { outside[3 * k] = c.outsideCalls()[k].target; outside[3 * k + 1] = c.outsideCalls()[k].source; outside[3 * k + 2] = c.outsideCalls()[k].weight; }
  return 0;
}
int ccmh_covis_best(void* h, int i, int N, int32_t* out, int cap) {
  if (!h || i < 0 || i >= as<cslam::CovisibilityBatch>(h)->size()) return -1;
  return view(as<cslam::CovisibilityBatch>(h)->GetBestCovisibilityKeyFrames(i, N), out, cap);
}
int ccmh_covis_by_weight(void* h, int i, int w, int32_t* out, int cap) {
  if (!h || i < 0 || i >= as<cslam::CovisibilityBatch>(h)->size()) return -1;
  return view(as<cslam::CovisibilityBatch>(h)->GetCovisiblesByWeight(i, w), out, cap);
}
void ccmh_covis_destroy(void* h) { delete as<cslam::CovisibilityBatch>(h); }
int ccmh_covis_update_host(int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt,
                           const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col,
                           int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags, int32_t* needed) {
  return cslam::covis_update_host(n_kf, n_all, order_key, list_off, list_pt, list_skip, n_pt, obs_off, obs_kf, th, cap, row_off, col, count, fw_off, fw_col, fw_w, ord_off,
                                  ord_kf, ord_w, flags, needed);
}

// KeyFrameCullingBatch through C
void* ccmh_kfcull_create(int device, int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                         const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad,
                         int th_obs, double thres, int n_levels) {
  return guard_ptr([&]() -> void* {
    if (n_cand < 1 || n_pt < 0 || !cand_flags || !list_off || (n_pt > 0 && (!obs_off || !pt_nobs || !pt_bad))) return nullptr;
    const int ne = list_off[n_cand], no = n_pt ? obs_off[n_pt] : 0;
    if (ne < 0 || no < 0 || (ne > 0 && (!list_pt || !list_level)) || (no > 0 && (!obs_kf || !obs_level || !obs_bad))) return nullptr;
    return new cslam::KeyFrameCullingBatch(ctx_or_null(device), n_all, std::vector<uint8_t>(cand_flags, cand_flags + n_cand),
                                           std::vector<int32_t>(list_off, list_off + n_cand + 1), std::vector<int32_t>(list_pt, list_pt + ne),
                                           std::vector<uint8_t>(list_level, list_level + ne), std::vector<int32_t>(pt_nobs, pt_nobs + n_pt),
                                           std::vector<uint8_t>(pt_bad, pt_bad + n_pt), n_pt ? std::vector<int32_t>(obs_off, obs_off + n_pt + 1) : std::vector<int32_t>(1, 0),
                                           std::vector<int32_t>(obs_kf, obs_kf + no), std::vector<uint8_t>(obs_level, obs_level + no),
                                           std::vector<uint8_t>(obs_bad, obs_bad + no), thres, n_levels, th_obs);
  });
}
int ccmh_kfcull_results(void* h, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone, int32_t* pt_nobs, int32_t* n_reeval) {
  if (!h) return -1;
  const cslam::KeyFrameCullingBatch& c = *as<cslam::KeyFrameCullingBatch>(h);
  if (verdict) for (int k = 0; k < c.size(); k++) verdict[k] = (uint8_t)c.verdict(k);
  if (n_mps && c.size()) std::memcpy(n_mps, c.nMPs().data(), (size_t)c.size() * 4);
  if (n_red && c.size()) std::memcpy(n_red, c.nRedundant().data(), (size_t)c.size() * 4);
  copy_out(pt_gone, c.gone());
  copy_out(pt_nobs, c.observations());
  if (n_reeval) *n_reeval = c.reevaluated();
  return 0;
}
int ccmh_kfcull_culled(void* h, int32_t* out, int cap) { return h ? view(as<cslam::KeyFrameCullingBatch>(h)->culled(), out, cap) : -1; }
int ccmh_kfcull_points_gone(void* h, int32_t* out, int cap) { return h ? view(as<cslam::KeyFrameCullingBatch>(h)->pointsGone(), out, cap) : -1; }
void ccmh_kfcull_destroy(void* h) { delete as<cslam::KeyFrameCullingBatch>(h); }
int ccmh_kfcull_walk_host(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                          const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad,
                          int th_obs, double thres, int n_levels, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone, int32_t* pt_nobs_out, int32_t* n_reeval) {
  return cslam::kfcull_walk_host(n_cand, n_all, cand_flags, list_off, list_pt, list_level, n_pt, pt_nobs, pt_bad, obs_off, obs_kf, obs_level, obs_bad, th_obs, thres,
                                 n_levels, verdict, n_mps, n_red, pt_gone, pt_nobs_out, n_reeval);
}
int ccmh_kfcull_walk_mapcopy_model(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                                   const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level,
                                   const uint8_t* obs_bad, int th_obs, double thres, int n_levels, uint8_t* verdict) {
  return cslam::kfcull_walk_mapcopy_model(n_cand, n_all, cand_flags, list_off, list_pt, list_level, n_pt, pt_nobs, pt_bad, obs_off, obs_kf, obs_level, obs_bad, th_obs,
                                          thres, n_levels, verdict);
}
}  // extern "C"
