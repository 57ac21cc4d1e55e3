// test_internal.h — entry points that exist for tests only.  They are NOT part of the C ABI (include/ccm_hip.h): C++ linkage inside namespace
// ccm_internal, defined next to the file-local kernels they exercise, and reached from tests through the `extern "C"` wrappers of
// libccm_testhooks.so (test_hooks.hip, declared in include/ccm_testhooks.h).  Nothing on a product path calls them.
#pragma once
#include "../../include/ccm_hip.h"
#include <cstddef>
#include <cstdint>
struct ccm_pg_debug_out;   // include/ccm_testhooks.h
namespace ccm_internal {
int  ba_debug_partial_reduced(ccm_ba* ba, double lambda, double* out, size_t cap, size_t* count);
int  ba_debug_coarse(ccm_ba* ba, double lambda, int* na, double* Ac, double* Ainv, double* Pm, size_t cap);
int  ba_debug_pcg_solve(ccm_ba* ba, double lambda, int coarse, double rel_tol, int max_it, double* x_out, size_t cap, int* flags);
int  comm_loopback_create(int nranks, void** group);
void comm_loopback_destroy(void* group);
int  comm_init_loopback(ccm_ctx* ctx, void* group, int rank);
int  debug_dense_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info);
int  debug_planned_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info);
int  debug_tile_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info, int* levels, int* tiles);
int  debug_dense_inverse(ccm_ctx* ctx, const double* A, int n, double* Ainv, int* info);
int  orb_debug_timing(const ccm_orb* o, double out_ms[6]);
int  orb_debug_level(ccm_orb* o, int level, uint8_t* score_out, uint8_t* blur_out);
int  orb_debug_candidates(ccm_orb* o, int level, ccm_keypoint* out, int cap, int* n_out);
int  orb_debug_octree_dev(ccm_ctx* ctx, const int32_t* x, const int32_t* y, const int32_t* response, int n, int W, int H, int N,
                          int32_t* sel_out, int cap, int* n_out, int* overflow);
int  covis_update_window(ccm_ctx* ctx, int small_window, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt,
                         const uint8_t* list_skip, int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col,
                         int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags,
                         int32_t* needed);
int  pg_debug_solve(ccm_ctx* ctx, int n_vert, const double* sim3, const uint8_t* fixed, int fix_scale, int n_edge, const int32_t* e_i, const int32_t* e_j,
                    const double* meas, double lambda, int solver, double rel_tol, int max_it, const double* r_in, ccm_pg_debug_out* out);
int  poseopt_debug_linearise(ccm_ctx* ctx, const double cam_qt[7], int n, const double* Xw, const double* obs, const double* info, const double K[4],
                             const uint8_t* level, const uint8_t* robust, double* acc_out, double* err_out, int shape[3]);
int  sim3opt_debug_linearise(ccm_ctx* ctx, const double sim3[8], int n, const double* P1c, const double* P2c, const double* obs1, const double* obs2,
                             const double* info1, const double* info2, const double K1[4], const double K2[4], double th2, int fix_scale, const uint8_t* alive,
                             double* acc_out, double* chi2_out, double* err_out, double* pert_out, double* J_out, int shape[2]);
}  // namespace ccm_internal
