// c_init.cpp — C entry points of NewMapPointBatch and TwoViewInitializer; triangulate_math.h and twoview_math.h compiled for the host
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include "mirror_internal.h"
#include "../csrc/triangulate_math.h"
#include "../csrc/twoview_math.h"
#include <cstring>

using namespace ccmh_c;

namespace {
// the two calls of a TwoViewInitializer: a device call that failed ("ccm_...") is -1000, every other complaint of the mirror -1
template <class F>
int guard_twoview(F&& f) {
  try {
    return f();
  } catch (const cslam::infrastructure_ex& e) {
    return std::strncmp(e.what(), "ccm_", 4) == 0 ? -1000 : -1;
  } catch (const std::exception&) { return -1000; }
}
}  // namespace

extern "C" {
// NewMapPointBatch through C.  cam records: 21 floats each (include/ccm_hip.h, ccm_triangulate_pairs); tables: nlevels floats each.
static cslam::LevelTables mk_tables(int nlevels, const float* s1, const float* f1, const float* s2, const float* f2) {
  cslam::LevelTables lv;
  if (nlevels < 1 || !s1 || !f1 || !s2 || !f2) throw cslam::infrastructure_ex("level tables");
  lv.nlevels = nlevels;
  lv.sigma2_1.assign(s1, s1 + nlevels); lv.sf_1.assign(f1, f1 + nlevels); lv.sigma2_2.assign(s2, s2 + nlevels); lv.sf_2.assign(f2, f2 + nlevels);
  return lv;
}
void* ccmh_newpts_create(int device, const float* cam1, int N1, const float* x1, const float* y1, const int32_t* oct1, int n_nb, const float* cam2,
                         const int32_t* N2, const float* const* x2, const float* const* y2, const int32_t* const* oct2, const int32_t* pair_off,
                         const int32_t* idx12, int nlevels, const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2,
                         float ratio_factor) {
  return guard_ptr([&]() -> void* {
    if (!cam1 || n_nb < 0 || (n_nb > 0 && (!cam2 || !N2 || !x2 || !y2 || !oct2 || !pair_off))) return nullptr;
    cslam::CamRecord c1; std::memcpy(&c1, cam1, sizeof c1);
    std::vector<cslam::NewMapPointBatch::Neighbour> nb((size_t)n_nb);
    for (int j = 0; j < n_nb; j++) {
      std::memcpy(&nb[j].cam, cam2 + 21 * (size_t)j, sizeof(cslam::CamRecord));
      nb[j].keys = mk_keys(x2[j], y2[j], oct2[j], nullptr, N2[j]);
      for (int i = pair_off[j]; i < pair_off[j + 1]; i++) nb[j].predicted.emplace_back(idx12[2 * i], idx12[2 * i + 1]);
    }
    return new cslam::NewMapPointBatch(ctx_or_null(device), c1, mk_keys(x1, y1, oct1, nullptr, N1), std::move(nb),
                                       mk_tables(nlevels, sigma2_1, sf_1, sigma2_2, sf_2), ratio_factor);
  });
}
void* ccmh_newpts_create_tri(int device, void* tri_batch, const int32_t* oct1, const float* cam1, const float* cam2, const float* F12, const float* exy,
                             int nlevels, const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2, float ratio_factor) {
  return guard_ptr([&]() -> void* {
    if (!tri_batch || !cam1 || !cam2 || !F12 || !exy) return nullptr;
    const cslam::TriangulationBatch& tb = *as<cslam::TriangulationBatch>(tri_batch);
    const int n = tb.neighbours();
    cslam::CamRecord c1; std::memcpy(&c1, cam1, sizeof c1);
    std::vector<cslam::CamRecord> c2((size_t)n);
    std::vector<cslam::NewMapPointBatch::Epipolar> ep((size_t)n);
    for (int j = 0; j < n; j++) {
      std::memcpy(&c2[j], cam2 + 21 * (size_t)j, sizeof(cslam::CamRecord));
      std::memcpy(ep[j].F12, F12 + 9 * (size_t)j, 9 * sizeof(float));
      ep[j].ex = exy[2 * j]; ep[j].ey = exy[2 * j + 1];
    }
    return new cslam::NewMapPointBatch(thread_context(device), tb, c1, c2, ep, mk_tables(nlevels, sigma2_1, sf_1, sigma2_2, sf_2), ratio_factor, oct1);
  });
}
int ccmh_newpts_points(void* h, int j, int n, const int32_t* idx12, uint8_t* status, float* x3d) {
  return guard_int([&]() -> int {
    if (!h || n < 0 || (n > 0 && (!idx12 || !status || !x3d))) return -1;
    cslam::NewMapPointBatch::Pairs p((size_t)n);
    for (int i = 0; i < n; i++) p[i] = {idx12[2 * i], idx12[2 * i + 1]};
    std::vector<uint8_t> st; std::vector<float> x;
    const int ok = as<cslam::NewMapPointBatch>(h)->points(j, p, st, x);
    if (n > 0) { std::memcpy(status, st.data(), st.size()); std::memcpy(x3d, x.data(), x.size() * sizeof(float)); }
    return ok;
  });
}
int ccmh_newpts_stats(void* h, int64_t* out3) {
  if (!h || !out3) return -1;
  const cslam::NewMapPointBatch& b = *as<cslam::NewMapPointBatch>(h);
  out3[0] = b.predicted(); out3[1] = b.hits(); out3[2] = b.misses();
  return 0;
}
void ccmh_newpts_destroy(void* h) { delete as<cslam::NewMapPointBatch>(h); }
// the arguments of ccm_triangulate_pairs through the host's tri_pair on the calling thread (what points() runs for a miss; scripts/triangulate_profile.py times it)
int ccmh_triangulate_pairs_host(const float* cam1, int S, const float* cam2, const int32_t* pair_off, const float* xy, const int32_t* oct, int nlevels,
                                const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2, float ratio_factor, uint8_t* status,
                                float* x3d, int32_t* n_accepted) {
  if (S < 1 || nlevels < 1 || !cam1 || !cam2 || !pair_off || !sigma2_1 || !sf_1 || !sigma2_2 || !sf_2 || !n_accepted || pair_off[0] != 0) return -1;
  for (int s = 0; s < S; s++) if (pair_off[s + 1] < pair_off[s]) return -1;
  const int P = pair_off[S];
  if (P > 0 && (!xy || !oct || !status || !x3d)) return -1;
  for (int i = 0; i < 2 * P; i++) if (oct[i] < 0 || oct[i] >= nlevels) return -1;
  TriCam c1; std::memcpy(&c1, cam1, sizeof c1);
  for (int s = 0; s < S; s++) {
    TriCam c2; std::memcpy(&c2, cam2 + 21 * (size_t)s, sizeof c2);
    int32_t n = 0;
    for (int i = pair_off[s]; i < pair_off[s + 1]; i++) {
      status[i] = (uint8_t)tri_pair(c1, c2, xy[4 * i], xy[4 * i + 1], oct[2 * i], xy[4 * i + 2], xy[4 * i + 3], oct[2 * i + 1], sigma2_1, sf_1, sigma2_2, sf_2,
                                    ratio_factor, x3d + 3 * (size_t)i);
      n += status[i] == TRI_OK;
    }
    n_accepted[s] = n;
  }
  return 0;
}

// TwoViewInitializer through C, and twoview_math.h compiled for the host
void* ccmh_twoview_create(int device, const float* K9, int N1, const float* keys1, float sigma) {
  return guard_ptr([&]() -> void* {
    if (!K9 || N1 < 0 || (N1 > 0 && !keys1)) return nullptr;
    return new cslam::TwoViewInitializer(ctx_or_null(device), K9, std::vector<float>(keys1, keys1 + 2 * (size_t)N1), sigma);
  });
}
int ccmh_twoview_find(void* h, int N2, const float* keys2, const int32_t* matches12, int n_sets, const int32_t* sets, float* scores3, int32_t* best2, float* H21,
                      float* F21, uint8_t* inl_h, uint8_t* inl_f) {
  if (!h || N2 < 0 || (N2 > 0 && !keys2) || !matches12 || n_sets < 1 || !sets || !scores3 || !best2 || !H21 || !F21 || !inl_h || !inl_f) return -1;
  cslam::TwoViewInitializer& tv = *as<cslam::TwoViewInitializer>(h);
  return guard_twoview([&]() -> int {
    // matches12 has one entry per keypoint of frame 1; the mirror knows how many that is from its own keys
    const cslam::TwoViewInitializer::Models m = tv.FindModels(std::vector<float>(keys2, keys2 + 2 * (size_t)N2), std::vector<int>(matches12, matches12 + tv.keys1()),
                                                              cslam::TwoViewInitializer::Sets(sets, sets + 8 * (size_t)n_sets));
    scores3[0] = m.SH; scores3[1] = m.SF; scores3[2] = m.RH;
    best2[0] = m.bestH; best2[1] = m.bestF;
    std::memcpy(H21, m.H21, sizeof m.H21); std::memcpy(F21, m.F21, sizeof m.F21);
    for (int i = 0; i < tv.matches(); i++) { inl_h[i] = m.vbMatchesInliersH[i]; inl_f[i] = m.vbMatchesInliersF[i]; }
    return tv.matches();
  });
}
int ccmh_twoview_check_rt(void* h, int n_hyp, const float* Rt, const uint8_t* inliers, float th2, int32_t* n_good, float* parallax, float* p3d, uint8_t* good,
                          uint8_t* status) {
  if (!h || n_hyp < 1 || n_hyp > 8 || !Rt || !inliers || !n_good || !parallax || !p3d || !good || !status) return -1;
  cslam::TwoViewInitializer& tv = *as<cslam::TwoViewInitializer>(h);
  return guard_twoview([&]() -> int {
    std::vector<cslam::TwoViewInitializer::Motion> hyp((size_t)n_hyp);
    for (int q = 0; q < n_hyp; q++) { std::memcpy(hyp[q].R, Rt + 12 * (size_t)q, 9 * sizeof(float)); std::memcpy(hyp[q].t, Rt + 12 * (size_t)q + 9, 3 * sizeof(float)); }
    const auto out = tv.CheckRTBatch(hyp, std::vector<bool>(inliers, inliers + tv.matches()), th2);
    const size_t N1 = (size_t)tv.keys1(), N = (size_t)tv.matches();
    for (int q = 0; q < n_hyp; q++) {
      n_good[q] = out[q].nGood; parallax[q] = out[q].parallax;
      std::memcpy(p3d + 3 * N1 * q, out[q].vP3D.data(), 3 * N1 * sizeof(float));
      for (size_t i = 0; i < N1; i++) good[N1 * q + i] = out[q].vbGood[i];
      std::memcpy(status + N * q, out[q].status.data(), N);
    }
    return 0;
  });
}
void ccmh_twoview_destroy(void* h) { delete as<cslam::TwoViewInitializer>(h); }
int ccmh_twoview_draw_sets(int N, int iterations, const int32_t* raw, int32_t* sets) {
  if (N < 8 || iterations < 0 || (iterations > 0 && (!raw || !sets))) return -1;
  size_t at = 0;
  const cslam::TwoViewInitializer::Sets s = cslam::TwoViewInitializer::DrawSets(N, iterations, [&] { return (int)raw[at++]; });
  std::memcpy(sets, s.data(), s.size() * sizeof(int32_t));
  return 0;
}
int ccmh_twoview_ransac_eval_host(int N, const float* xy1, const float* xy2, const float* pn1, const float* pn2, const float* T1, const float* T2inv, const float* T2t,
                                  float sigma, int H, const int32_t* sets, int model, float* scoreH, float* scoreF, float* H21, float* F21, uint32_t* maskH,
                                  uint32_t* maskF) {
  if (model < 0 || model > 2) return -1;
  return cslam::detail::twoview_ransac_host(N, xy1, xy2, pn1, pn2, T1, T2inv, T2t, sigma, H, sets, model, scoreH, scoreF, H21, F21, maskH, maskF);
}
int ccmh_twoview_check_rt_host(int n_hyp, const float* rec, const float* K9, int N, const float* xy1, const float* xy2, const uint32_t* inlier_mask, float th2,
                               uint8_t* status, float* x3d, float* cos_parallax) {
  return cslam::detail::twoview_check_rt_host(n_hyp, rec, K9, N, xy1, xy2, inlier_mask, th2, status, x3d, cos_parallax);
}
void ccmh_twoview_normalize(const float* xy, int n, float* pn, float* T9) { tv_normalize(xy, n, pn, T9); }
void ccmh_twoview_inv33(const float* S9, float* D9) { tv_inv33(S9, D9); }
void ccmh_twoview_prepare_rt(const float* K9, const float* R9, const float* t3, float* rec27) {
  TvMotion m;
  tv_prepare_rt(K9, R9, t3, m);
  std::memcpy(rec27, &m, sizeof m);
}
int ccmh_twoview_svd(int shape, const float* A, float* out) {
  if (!A || !out) return -1;
  if (shape == 0) tv_svd16x9_last_row(A, out);
  else if (shape == 1) { std::memcpy(out, A, 72 * sizeof(float)); tv_svd8x9_vt(out); }
  else if (shape == 2) tv_svd3x3(A, out, out + 3, out + 12);
  else return -1;
  return 0;
}
int ccmh_twoview_score_host(int model, int n_models, const float* M, int N, const float* xy1, const float* xy2, float sigma, float* score, uint32_t* mask) {
  if (model < 0 || model > 1 || n_models < 1 || N < 1 || !M || !xy1 || !xy2 || !score || !mask) return -1;
  const size_t words = ((size_t)N + 31) / 32;
  for (int h = 0; h < n_models; h++) {
    float inv[9] = {0};
    if (model == 0) tv_inv33(M + 9 * (size_t)h, inv);
    score[h] = tv_score(model == 0, M + 9 * (size_t)h, inv, N, xy1, xy2, sigma, mask + words * h);
  }
  return 0;
}
}  // extern "C"
