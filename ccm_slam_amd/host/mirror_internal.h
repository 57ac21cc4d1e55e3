// mirror_internal.h — what ccm_host.cpp defines, ccm_host.h does not declare, and a c_*.cpp unit calls.  Not installed, not for shim/.
//   cslam::detail (hidden visibility):
//     twoview_ransac_host, twoview_check_rt_host   ccm_host.cpp (TwoViewInitializer without a context), c_init.cpp (their C entry points)
//   cslam (exported as before):
//     sim3_correct_map_host                        ccm_host.cpp (Sim3MapCorrection without a context), c_map.cpp (its C entry point)
#pragma once
#include <cstdint>

namespace cslam {

int sim3_correct_map_host(int n_kf, const float* Tiw, int cur, const float* Twc, const double* Scw, double* S_non, double* S_cor, int n_obs_kf, const float* kf_center,
                          const int32_t* kf_rank, int n_pt, const float* pos, const int32_t* owner, const int32_t* owner_rank, const int32_t* obs_off,
                          const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, float* pos_out, float* normal,
                          float* min_dist, float* max_dist, float* Tiw_new, float* center_new);

namespace detail __attribute__((visibility("hidden"))) {
// twoview_math.h on the calling thread with the arguments of ccm_twoview_ransac_eval; model: 0 both, 1 the homography only, 2 the fundamental matrix only
int twoview_ransac_host(int N, const float* xy1, const float* xy2, const float* pn1, const float* pn2, const float* T1, const float* T2inv, const float* T2t,
                        float sigma, int H, const int32_t* sets, int model, float* scoreH, float* scoreF, float* H21, float* F21, uint32_t* maskH, uint32_t* maskF);
int twoview_check_rt_host(int n_hyp, const float* rec, const float* K, int N, const float* xy1, const float* xy2, const uint32_t* inl, float th2, uint8_t* status,
                          float* x3d, float* cosp);
}  // namespace detail
}  // namespace cslam
