// c_matcher.cpp — C entry points of the BoW / triangulation / initialisation searches, the projected window search, FuseBatch, TriangulationBatch
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include <cstring>

using namespace ccmh_c;

extern "C" {
// mode 0: SearchByBoW(KF,F) -> out[N2] ; 1: SearchByBoW(KF,KF) -> out[N1] ; 2: SearchForTriangulation -> out[N1]
int ccmh_search_bow(int device, int mode, const int32_t* n1, const int32_t* o1, const int32_t* i1, int nn1, const int32_t* n2,
                    const int32_t* o2, const int32_t* i2, int nn2, const uint8_t* has1, const uint8_t* has2, const uint8_t* d1,
                    const float* x1, const float* y1, const float* a1, int N1, const uint8_t* d2, const float* x2, const float* y2,
                    const int32_t* oct2, const float* a2, int N2, const float* F12, float ex, float ey, const float* sigma2_2,
                    const float* sf2, float nnratio, int check_ori, int32_t* out) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    auto k1 = mk_keys(x1, y1, nullptr, a1, N1), k2 = mk_keys(x2, y2, oct2, a2, N2);
    cslam::KeysView A; A.N = N1; A.keys = k1.data(); A.desc = d1; A.hasMapPoint = has1; A.fv = cslam::FeatureVectorView{nn1, n1, o1, i1};
    cslam::KeysView B; B.N = N2; B.keys = k2.data(); B.desc = d2; B.hasMapPoint = has2; B.fv = cslam::FeatureVectorView{nn2, n2, o2, i2};
    cslam::ORBmatcher m(ctx, nnratio, check_ori != 0);
    std::vector<int32_t> r; int n = 0;
    if (mode == 0) n = m.SearchByBoW(A, B, r);
    else if (mode == 1) n = m.SearchByBoW_KF(A, B, r);
    else n = m.SearchForTriangulation(A, B, F12, ex, ey, sigma2_2, sf2, r);
    std::memcpy(out, r.data(), r.size() * sizeof(int32_t));
    return n;
  });
}

// TriangulationBatch through C (shim/ORBmatcher_hip.cpp, tests): neighbour arrays as arrays of pointers, one entry per neighbour
void* ccmh_tri_batch_create(int device, float nnratio, int check_ori, const int32_t* n1, const int32_t* o1, const int32_t* i1, int nn1, const uint8_t* has1,
                            const uint8_t* d1, const float* x1, const float* y1, const float* a1, int N1, int n_nb, const int32_t* const* n2,
                            const int32_t* const* o2, const int32_t* const* i2, const int32_t* nn2, const uint8_t* const* has2, const uint8_t* const* d2,
                            const float* const* x2, const float* const* y2, const int32_t* const* oct2, const float* const* a2, const int32_t* N2) {
  return guard_ptr([&]() -> void* {
    cslam::HipContext& ctx = thread_context(device);
    auto k1 = mk_keys(x1, y1, nullptr, a1, N1);
    cslam::KeysView A; A.N = N1; A.keys = k1.data(); A.desc = d1; A.hasMapPoint = has1; A.fv = cslam::FeatureVectorView{nn1, n1, o1, i1};
    std::vector<std::vector<cslam::KeyPoint>> k2((size_t)n_nb);
    std::vector<cslam::KeysView> B((size_t)n_nb);
    for (int j = 0; j < n_nb; j++) {
      k2[j] = mk_keys(x2[j], y2[j], oct2[j], a2[j], N2[j]);
      B[j].N = N2[j]; B[j].keys = k2[j].data(); B[j].desc = d2[j]; B[j].hasMapPoint = has2[j]; B[j].fv = cslam::FeatureVectorView{nn2[j], n2[j], o2[j], i2[j]};
    }
    cslam::ORBmatcher m(ctx, nnratio, check_ori != 0);
    return new cslam::TriangulationBatch(m, A, B);
  });
}
int ccmh_tri_batch_resolve(void* h, int j, const uint8_t* has1_now, const uint8_t* has2_now, const float* F12, float ex, float ey, const float* sigma2_2,
                           const float* sf2, int32_t* matches12) {
  return guard_int([&]() -> int {
    std::vector<int32_t> r;
    const int n = as<cslam::TriangulationBatch>(h)->resolve(j, has1_now, has2_now, F12, ex, ey, sigma2_2, sf2, r);
    std::memcpy(matches12, r.data(), r.size() * sizeof(int32_t));
    return n;
  });
}
long long ccmh_tri_batch_candidates(void* h) { return h ? (long long)as<cslam::TriangulationBatch>(h)->candidates() : 0; }
void ccmh_tri_batch_destroy(void* h) { delete as<cslam::TriangulationBatch>(h); }

int ccmh_search_for_initialization(int device, const float* x1, const float* y1, const int32_t* oct1, const float* a1, const uint8_t* d1, int N1,
                                   const float* x2, const float* y2, const int32_t* oct2, const float* a2, const uint8_t* d2, int N2,
                                   float minX, float minY, float maxX, float maxY, float* prev_xy, int window, float nnratio, int check_ori,
                                   int32_t* matches12) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    auto k1 = mk_keys(x1, y1, oct1, a1, N1);
    cslam::KeysView A; A.N = N1; A.keys = k1.data(); A.desc = d1;
    const float bounds[4] = {minX, minY, maxX, maxY};
    FlatFrame fr(mk_keys(x2, y2, oct2, a2, N2), d2, bounds, nullptr, nullptr);
    fr.all_free();
    std::vector<float> prev(prev_xy, prev_xy + 2 * (size_t)N1);
    std::vector<int32_t> r;
    cslam::ORBmatcher m(ctx, nnratio, check_ori != 0);
    const int n = m.SearchForInitialization(A, fr.F, prev, r, window);
    std::memcpy(prev_xy, prev.data(), prev.size() * sizeof(float));
    std::memcpy(matches12, r.data(), r.size() * sizeof(int32_t));
    return n;
  });
}

int ccmh_projected_window_search(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, int N, float minX,
                                 float minY, float maxX, float maxY, const float* scale_factors, const float* inv_sigma2, int n_pts,
                                 const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, float th,
                                 int chi2_gate, int dist_threshold, int32_t* matched, int claim, const uint8_t* no_claim,
                                 int32_t* best_idx, int32_t* best_dist) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    const float bounds[4] = {minX, minY, maxX, maxY};
    FlatFrame fr(mk_keys(kx, ky, oct, nullptr, N), kdesc, bounds, scale_factors, nullptr);
    fr.all_free();
    cslam::ORBmatcher::ProjectedPoints P; P.n = n_pts; P.valid = valid; P.u = u; P.v = v; P.level = level; P.desc = pdesc; P.noClaim = no_claim;
    cslam::ORBmatcher m(ctx);
    std::vector<int32_t> bi, bd;
    const int n = m.ProjectedSearch(fr.F, inv_sigma2, P, th, chi2_gate != 0, dist_threshold, matched, claim != 0, bi, bd);
    return copy_best(n, n_pts, bi, bd, best_idx, best_dist);
  });
}

// the same search on candidate lists the caller obtained from its own KeyFrame::GetFeaturesInArea (CSR over the n points; th and the bounds are unused)
int ccmh_projected_window_search_cand(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, int N,
                                      const float* inv_sigma2, int n_pts, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                      const uint8_t* pdesc, const int32_t* cand_off, const int32_t* cand_idx, int chi2_gate, int dist_threshold,
                                      int32_t* matched, int claim, const uint8_t* no_claim, int32_t* best_idx, int32_t* best_dist) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    FlatFrame fr(mk_keys(kx, ky, oct, nullptr, N), kdesc, nullptr, nullptr, nullptr);
    cslam::ORBmatcher::ProjectedPoints P; P.n = n_pts; P.valid = valid; P.u = u; P.v = v; P.level = level; P.desc = pdesc; P.noClaim = no_claim;
    P.candOff = cand_off; P.candIdx = cand_idx;
    cslam::ORBmatcher m(ctx);
    std::vector<int32_t> bi, bd;
    const int n = m.ProjectedSearch(fr.F, inv_sigma2, P, 0.f, chi2_gate != 0, dist_threshold, matched, claim != 0, bi, bd);
    return copy_best(n, n_pts, bi, bd, best_idx, best_dist);
  });
}

// the same search through the device grid (bounds must be the plain image rectangle: 0, 0, maxX, maxY)
int ccmh_projected_window_search_dev(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, int N, float maxX,
                                     float maxY, const float* scale_factors, const float* inv_sigma2, int n_pts, const uint8_t* valid,
                                     const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, float th, int chi2_gate,
                                     int dist_threshold, int32_t* matched, int claim, const uint8_t* no_claim, int32_t* best_idx,
                                     int32_t* best_dist) {
  return guard_int([&]() -> int {
    cslam::HipContext& ctx = thread_context(device);
    const float K[4] = {1.f, 1.f, 0.f, 0.f};
    cslam::FrameGridDev grid(ctx, K, nullptr, 0, (int)maxX, (int)maxY);
    std::vector<cslam::KeyPoint> keysUn;
    grid.SetKeyPoints(mk_keys(kx, ky, oct, nullptr, N), kdesc, keysUn);
    FlatFrame fr(std::move(keysUn), kdesc, grid, scale_factors, nullptr);
    fr.all_free();
    cslam::ORBmatcher::ProjectedPoints P; P.n = n_pts; P.valid = valid; P.u = u; P.v = v; P.level = level; P.desc = pdesc; P.noClaim = no_claim;
    cslam::ORBmatcher m(ctx);
    std::vector<int32_t> bi, bd;
    const int n = m.ProjectedSearch(grid, fr.F, inv_sigma2, P, th, chi2_gate != 0, dist_threshold, matched, claim != 0, bi, bd);
    return copy_best(n, n_pts, bi, bd, best_idx, best_dist);
  });
}

// FuseBatch through a flat interface (tests): S targets given as concatenated arrays with offsets; every target is searched with the chi2 gate and TH_LOW like Fuse
void* ccmh_fuse_batch_create(int device, int S, const int32_t* kf_off /* [S+1] features */, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc,
                             const float* bounds4 /* [S][4] minX minY maxX maxY */, const float* scale_factors, const float* inv_sigma2,
                             const int32_t* pt_off /* [S+1] points */, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                             const uint8_t* pdesc, float th) {
  return guard_ptr([&]() -> void* {
    cslam::HipContext& ctx = thread_context(device);
    cslam::ORBmatcher m(ctx);
    std::vector<FlatFrame> fr;
    fr.reserve(S);
    std::vector<cslam::FuseBatch::Target> tg(S);
    for (int s = 0; s < S; s++) {
      const int k0 = kf_off[s], N = kf_off[s + 1] - k0, p0 = pt_off[s];
      fr.emplace_back(mk_keys(kx + k0, ky + k0, oct + k0, nullptr, N), kdesc + (size_t)k0 * 32, bounds4 + 4 * (size_t)s, scale_factors, nullptr);
      tg[s].KF = fr[s].all_free().F;
      cslam::ORBmatcher::ProjectedPoints& P = tg[s].P;
      P.n = pt_off[s + 1] - p0; P.valid = valid + p0; P.u = u + p0; P.v = v + p0; P.level = level + p0; P.desc = pdesc + (size_t)p0 * 32;
      tg[s].invLevelSigma2 = inv_sigma2; tg[s].th = th;
    }
    return new cslam::FuseBatch(m, tg);
  });
}
// the same with every target's window candidates supplied by the caller (its own KeyFrame::GetFeaturesInArea, as ccmh_projected_window_search_cand): target s owns the
// points pt_off[s] .. pt_off[s+1]; cand_off has one entry per point plus one per target (target s: entries pt_off[s] + s .. pt_off[s+1] + s, starting at 0), its
// candidate indices start at cand_base[s] in cand_idx
void* ccmh_fuse_batch_create_cand(int device, int S, const int32_t* kf_off, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc,
                                  const float* const* inv_sigma2 /* [S] */, const int32_t* pt_off, const uint8_t* valid, const float* u, const float* v,
                                  const int32_t* level, const uint8_t* pdesc, const int32_t* cand_off, const int32_t* cand_base, const int32_t* cand_idx,
                                  int chi2_gate, int dist_threshold) {
  return guard_ptr([&]() -> void* {
    cslam::HipContext& ctx = thread_context(device);
    cslam::ORBmatcher m(ctx);
    std::vector<FlatFrame> fr;
    fr.reserve(S);
    std::vector<cslam::FuseBatch::Target> tg(S);
    for (int s = 0; s < S; s++) {
      const int k0 = kf_off[s], N = kf_off[s + 1] - k0, p0 = pt_off[s];
      fr.emplace_back(mk_keys(kx + k0, ky + k0, oct + k0, nullptr, N), kdesc + (size_t)k0 * 32, nullptr, nullptr, nullptr);
      tg[s].KF = fr[s].F;
      cslam::ORBmatcher::ProjectedPoints& P = tg[s].P;
      P.n = pt_off[s + 1] - p0; P.valid = valid + p0; P.u = u + p0; P.v = v + p0; P.level = level + p0; P.desc = pdesc + (size_t)p0 * 32;
      P.candOff = cand_off + p0 + s; P.candIdx = cand_idx + cand_base[s];
      tg[s].invLevelSigma2 = inv_sigma2[s]; tg[s].th = 0.f;
    }
    return new cslam::FuseBatch(m, tg, chi2_gate != 0, dist_threshold);
  });
}
long long ccmh_fuse_batch_candidates(void* h) { return h ? (long long)as<cslam::FuseBatch>(h)->candidates() : -1; }
int ccmh_fuse_batch_resolve(void* h, int s, const uint8_t* skip_now, int n_pts, int32_t* best_idx, int32_t* best_dist) {
  return guard_int([&]() -> int {
    std::vector<int32_t> bi, bd;
    const int n = as<cslam::FuseBatch>(h)->resolve(s, skip_now, bi, bd);
    return copy_best(n, n_pts, bi, bd, best_idx, best_dist);
  });
}
void ccmh_fuse_batch_destroy(void* h) { delete as<cslam::FuseBatch>(h); }
}  // extern "C"
