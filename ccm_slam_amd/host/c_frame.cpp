// c_frame.cpp — C entry points of the extractor, the tracking searches, the guided search and the relocalisation refine chain
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include <algorithm>
#include <cstring>

using namespace ccmh_c;

namespace {
cslam::KeyFramePoints guidedKf(int P, const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const float* angle) {
  cslam::KeyFramePoints kf;
  kf.n = P; kf.live = live; kf.pos = pos; kf.min_dist = min_dist; kf.max_dist = max_dist; kf.desc = desc; kf.angle = angle;
  return kf;
}
}  // namespace

extern "C" {
int ccmh_search_by_projection_mp(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* fdesc, int N,
                                 float minX, float minY, float maxX, float maxY, const float* scale_factors, int n_mp,
                                 const uint8_t* in_view, const float* px, const float* py, const int32_t* lvl, const float* vcos,
                                 const uint8_t* mp_desc, float th, float nnratio, int32_t* frame_mp) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    const float bounds[4] = {minX, minY, maxX, maxY};
    FlatFrame fr(mk_keys(kx, ky, oct, nullptr, N), fdesc, bounds, scale_factors, frame_mp);
    cslam::TrackedMapPoints M; M.n = n_mp; M.mbTrackInView = in_view; M.mTrackProjX = px; M.mTrackProjY = py; M.mnTrackScaleLevel = lvl;
    M.mTrackViewCos = vcos; M.mDescriptor = mp_desc;
    cslam::ORBmatcher m(ctx, nnratio, true);
    return m.SearchByProjection(fr.F, M, th);
  });
}

int ccmh_search_by_projection_last(int device, const float* kx, const float* ky, const int32_t* oct, const float* kangle,
                                   const uint8_t* fdesc, int N, float minX, float minY, float maxX, float maxY,
                                   const float* scale_factors, int n_last, const uint8_t* valid, const float* u, const float* v,
                                   const int32_t* l_oct, const float* l_angle, const uint8_t* l_desc, float th, int check_ori,
                                   int32_t* cur_mp) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    const float bounds[4] = {minX, minY, maxX, maxY};
    FlatFrame fr(mk_keys(kx, ky, oct, kangle, N), fdesc, bounds, scale_factors, cur_mp);
    cslam::LastFrameProjections L; L.n = n_last; L.valid = valid; L.u = u; L.v = v; L.octave = l_oct; L.angle = l_angle; L.mpDescriptor = l_desc;
    cslam::ORBmatcher m(ctx, 0.9f, check_ori != 0);
    return m.SearchByProjection(fr.F, L, th);
  });
}

// SearchByProjection(Frame, map points) through the device grid: raw (distorted) keypoints in, match table + undistorted xy out
int ccmh_search_by_projection_mp_dev(int device, const float* K, const float* dist, int n_dist, int w, int h, const void* kps_raw, const uint8_t* fdesc,
                                     int N, const float* scale_factors, int n_mp, const uint8_t* in_view, const float* px, const float* py,
                                     const int32_t* lvl, const float* vcos, const uint8_t* mp_desc, float th, float nnratio, int32_t* frame_mp,
                                     float* xy_un_out) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    cslam::FrameGridDev grid(ctx, K, dist, n_dist, w, h);
    std::vector<cslam::KeyPoint> keysUn;
    grid.SetKeyPoints(raw_keys(kps_raw, N), fdesc, keysUn);
    for (int i = 0; i < N; i++) { xy_un_out[2 * i] = keysUn[i].x; xy_un_out[2 * i + 1] = keysUn[i].y; }
    FlatFrame fr(std::move(keysUn), fdesc, grid, scale_factors, frame_mp);
    cslam::TrackedMapPoints mps;
    mps.n = n_mp; mps.mbTrackInView = in_view; mps.mTrackProjX = px; mps.mTrackProjY = py; mps.mnTrackScaleLevel = lvl; mps.mTrackViewCos = vcos;
    mps.mDescriptor = mp_desc;
    cslam::ORBmatcher m(ctx, nnratio, true);
    return m.SearchByProjection(grid, fr.F, mps, th);
  });
}

// SearchByProjection(Frame, LastFrame) through the device grid; keypoints given already undistorted (no distortion coefficients)
int ccmh_search_by_projection_last_dev(int device, const void* kps_un, const uint8_t* cdesc, int N, int w, int h, const float* scale_factors, int n_last,
                                       const uint8_t* valid, const float* u, const float* v, const int32_t* oct, const float* angle, const uint8_t* mp_desc,
                                       float th, int check_ori, int32_t* frame_mp) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    const float K[4] = {1.f, 1.f, 0.f, 0.f};
    cslam::FrameGridDev grid(ctx, K, nullptr, 0, w, h);
    std::vector<cslam::KeyPoint> keysUn;
    grid.SetKeyPoints(raw_keys(kps_un, N), cdesc, keysUn);
    FlatFrame fr(std::move(keysUn), cdesc, grid, scale_factors, frame_mp);
    cslam::LastFrameProjections L;
    L.n = n_last; L.valid = valid; L.u = u; L.v = v; L.octave = oct; L.angle = angle; L.mpDescriptor = mp_desc;
    cslam::ORBmatcher m(ctx, 0.9f, check_ori != 0);
    return m.SearchByProjection(grid, fr.F, L, th);
  });
}

int ccmh_orb_extract(int device, int nfeatures, const uint8_t* img, int w, int h, void* kps_out, uint8_t* desc_out, int cap) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    cslam::ORBextractor ex(ctx, nfeatures, 1.2f, 8, 20, 7);
    std::vector<cslam::KeyPoint> k; std::vector<uint8_t> d;
    ex(img, w, h, w, k, d);
    const int n = std::min<int>((int)k.size(), cap);
    std::memcpy(kps_out, k.data(), sizeof(cslam::KeyPoint) * n);
    std::memcpy(desc_out, d.data(), (size_t)n * 32);
    return n;
  });
}

// The host evaluator of ccm_frame_guided_search: its arguments after the frame, which is given as arrays; no device is touched.  0, or -1 for its CCM_E_ARG cases.
int ccmh_guided_search_host(const void* kps_un, const uint8_t* fdesc, int N, const float* bounds, const float* K, const void* pose_v, int P, const float* pos,
                            const float* min_dist, const float* max_dist, const uint8_t* desc, const uint8_t* skip, float th, uint8_t* status, float* u, float* v,
                            int32_t* level, int32_t* cand_off, int32_t* cand_idx, uint16_t* cand_dist, int64_t cap, int64_t* n_cand) {
  return guard_arg([&]() -> int {
    if (!pose_v || !bounds || !K || N < 0 || (N && (!kps_un || !fdesc)) || P < 0 || !cand_off || !n_cand || (P && (!status || !u || !v || !level)) || cap < 0 ||
        (cap && (!cand_idx || !cand_dist)))
      return -1;
    ccm_guided_pose pose;
    std::memcpy(&pose, pose_v, sizeof(pose));
    FlatFrame fr(raw_keys(kps_un, N), fdesc, bounds, pose.scaleFactors, nullptr);
    const std::vector<uint8_t> live((size_t)std::max(P, 1), 1);
    cslam::GuidedCandidates c;
    cslam::ORBmatcher::GuidedSearchHost(fr.F, K, pose, guidedKf(P, live.data(), pos, min_dist, max_dist, desc, nullptr), skip, th, c);
    *n_cand = (int64_t)c.idx.size();
    std::memcpy(cand_off, c.off.data(), sizeof(int32_t) * ((size_t)P + 1));
    if (P) {
      std::memcpy(status, c.status.data(), (size_t)P); std::memcpy(u, c.u.data(), sizeof(float) * (size_t)P); std::memcpy(v, c.v.data(), sizeof(float) * (size_t)P);
      std::memcpy(level, c.level.data(), sizeof(int32_t) * (size_t)P);
    }
    if (cap == 0) return 0;
    if (*n_cand > cap) return -1;
    if (*n_cand) { std::memcpy(cand_idx, c.idx.data(), sizeof(int32_t) * c.idx.size()); std::memcpy(cand_dist, c.dist.data(), sizeof(uint16_t) * c.dist.size()); }
    return 0;
  });
}

// ORBmatcher::SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist): the host mirror without a grid (no device is touched) and with one (a FrameGridDev
// built from the arrays).  nmatches, -1 for a bad argument, -1000 when the device path throws.  frame_mp: in/out, F.mvpMapPoints.
int ccmh_search_by_projection_kf_host(const void* kps_un, const uint8_t* fdesc, int N, const float* bounds, const float* K, const void* pose_v, int P,
                                      const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const float* angle,
                                      const uint8_t* already_found, float th, int orb_dist, int check_ori, int32_t* frame_mp) {
  return guard_arg([&]() -> int {
    if (!pose_v || !bounds || !K || N < 0 || (N && (!kps_un || !fdesc || !frame_mp)) || P < 0) return -1;
    ccm_guided_pose pose;
    std::memcpy(&pose, pose_v, sizeof(pose));
    FlatFrame fr(raw_keys(kps_un, N), fdesc, bounds, pose.scaleFactors, frame_mp);
    const cslam::KeyFramePoints kf = guidedKf(P, live, pos, min_dist, max_dist, desc, angle);
    if (orb_dist < 0 || orb_dist > 255) return -1;
    cslam::GuidedCandidates c;
    cslam::ORBmatcher::GuidedSearchHost(fr.F, K, pose, kf, already_found, th, c);
    return cslam::ORBmatcher::GuidedReplay(fr.F, kf, c, orb_dist, check_ori != 0);
  });
}
int ccmh_search_by_projection_kf_dev(int device, const float* K, int w, int h, const void* kps_un, const uint8_t* fdesc, int N, const void* pose_v, int P,
                                     const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const float* angle,
                                     const uint8_t* already_found, float th, int orb_dist, int check_ori, int32_t* frame_mp) {
  return guard_arg([&]() -> int {
    if (!pose_v || !K || N < 0 || (N && (!kps_un || !fdesc || !frame_mp)) || P < 0) return -1;
    ccm_guided_pose pose;
    std::memcpy(&pose, pose_v, sizeof(pose));
    cslam::HipContext& ctx = thread_context(device);
    cslam::FrameGridDev grid(ctx, K, nullptr, 0, w, h);
    std::vector<cslam::KeyPoint> keysUn;
    grid.SetKeyPoints(raw_keys(kps_un, N), fdesc, keysUn);
    FlatFrame fr(std::move(keysUn), fdesc, grid, pose.scaleFactors, frame_mp);
    cslam::ORBmatcher m(ctx, 0.9f, check_ori != 0);
    return m.SearchByProjection(grid, fr.F, pose, guidedKf(P, live, pos, min_dist, max_dist, desc, angle), already_found, th, orb_dist);
  });
}

// the drop-in's form: the lists are the caller's Frame::GetFeaturesInArea results (cand_off over the P slots); f_angle: the frame's mvKeysUn[].angle
int ccmh_search_by_projection_kf_cand(int device, const uint8_t* fdesc, const float* f_angle, int N, int P, const uint8_t* desc, const float* kf_angle,
                                      const int32_t* cand_off, const int32_t* cand_idx, int orb_dist, int check_ori, int32_t* frame_mp) {
  return guard_arg([&]() -> int {
    if (N < 0 || P < 0 || (N && (!fdesc || !f_angle || !frame_mp)) || !cand_off) return -1;
    cslam::HipContext& ctx = thread_context(device);
    std::vector<cslam::KeyPoint> keys((size_t)N);
    for (int i = 0; i < N; i++) keys[i] = cslam::KeyPoint{0.f, 0.f, 31.f, f_angle[i], 0.f, 0};
    FlatFrame fr(std::move(keys), fdesc, nullptr, nullptr, frame_mp);
    cslam::ORBmatcher m(ctx, 0.9f, check_ori != 0);
    return m.SearchByProjectionCandidates(fr.F, guidedKf(P, nullptr, nullptr, nullptr, nullptr, desc, kf_angle), cand_off, cand_idx, orb_dist);
  });
}

// cslam::RelocalizationRefine on flat arrays.  1 matched, 0 not, -1 for a bad argument, -1000 when the device path throws.  frame_mp [N], Tcw16, trace5 and n_good: out.
int ccmh_reloc_refine(int device, const float* K, int w, int h, const void* kps_un, const uint8_t* fdesc, int N, const float* inv_level_sigma2,
                      const void* frame_v, int P, const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc,
                      const float* angle, const int32_t* matches_f, const uint8_t* inliers, int32_t* frame_mp, float* Tcw16, int32_t* trace5, int32_t* n_good) {
  return guard_arg([&]() -> int {
    if (!frame_v || !K || N < 0 || (N && (!kps_un || !fdesc || !frame_mp)) || P < 0 || !Tcw16 || !trace5 || !n_good) return -1;
    ccm_guided_pose frame;
    std::memcpy(&frame, frame_v, sizeof(frame));
    cslam::HipContext& ctx = thread_context(device);
    cslam::FrameGridDev grid(ctx, K, nullptr, 0, w, h);
    std::vector<cslam::KeyPoint> keysUn;
    grid.SetKeyPoints(raw_keys(kps_un, N), fdesc, keysUn);
    FlatFrame fr(std::move(keysUn), fdesc, grid, frame.scaleFactors, frame_mp);
    const cslam::RelocRefineResult r = cslam::RelocalizationRefine(ctx, grid, fr.F, K, inv_level_sigma2, frame, guidedKf(P, live, pos, min_dist, max_dist, desc, angle),
                                                                   matches_f, inliers);
    std::memcpy(Tcw16, r.Tcw, sizeof(float) * 16);
    for (int i = 0; i < 5; i++) trace5[i] = r.trace[i];
    *n_good = r.nGood;
    return r.matched ? 1 : 0;
  });
}
}  // extern "C"
