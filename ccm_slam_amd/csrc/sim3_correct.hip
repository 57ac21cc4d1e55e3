// sim3_correct.hip — the Sim3 correction of a closed loop's or merged map's keyframes and map points on the device: ccm_sim3_correct_map
// (LoopFinder.cpp:543-613, MapMerger.cpp:289-395, Optimizer.cpp:1279-1330).
//
// Layout: per keyframe of the set, in walk order, three Sim3 tables of 8 doubles (S_non = Siw, S_cor = CorrectedSiw, S_swi = its
// inverse), the new pose (12 floats) and the new centre; the old centres and the ranks cover the set and the observers outside it.  Points carry their
// owner, the owner's rank, an observation list in CSR and a reference keyframe with its level.  Two kernels on the context's stream: one lane per
// keyframe, then one lane per point, 64 lanes per workgroup (a loop neighbourhood has a few thousand points: small workgroups spread them over the CUs).
// A point's lane loops over its own observation list; lanes of a wave with shorter lists idle until the longest is done (2 .. 30 entries, mean about 6).
// The rank and centre tables are a few thousand keyframes x 12 bytes and stay in L2.
#include "common.h"
#include "sim3_correct_math.h"
#include "stage_blocks.h"
#include <limits.h>

namespace {

constexpr int kS3cBlock = 64;

struct S3cArgs {
  int n_kf, n_pt, cur, n_levels;
  const float* Tiw;          // [n_kf * 12] or nullptr (epilogue form)
  const float* Twc;          // [12]
  const double* Scw;         // [8]
  double* S_non;             // [n_kf * 8]
  double* S_cor;             // [n_kf * 8]
  double* S_swi;             // [n_kf * 8]
  float* T_new;              // [n_kf * 12]
  float* c_new;              // [n_kf * 3]
  const float* c_old;        // [n_obs_kf * 3]
  const int32_t* kf_rank;    // [n_obs_kf]
  const float* scale_factors;
  const float* pos;          // [n_pt * 3]
  const int32_t* owner;      // [n_pt]
  const int32_t* owner_rank; // [n_pt]
  const int32_t* obs_off;    // [n_pt + 1]
  const int32_t* obs_kf;
  const int32_t* ref_kf;     // [n_pt]
  const int32_t* ref_level;  // [n_pt]
  const float* normal_in;    // [n_pt * 3]
  const float* dmin_in;
  const float* dmax_in;
  float* pos_out;            // [n_pt * 3]
  float* normal_out;
  float* dmin_out;
  float* dmax_out;
};

__global__ __launch_bounds__(kS3cBlock) void sim3_correct_kf_kernel(S3cArgs a) {
  const int i = blockIdx.x * kS3cBlock + threadIdx.x;
  if (i >= a.n_kf) return;
  Sim3d S_non, S_cor, S_swi;
  float T[12], O[3];
  if (a.Tiw) {
    s3c_keyframe(a.Tiw + 12 * (size_t)i, i == a.cur, a.Twc, sim3_load(a.Scw), S_non, S_cor, S_swi, T, O);
    sim3_store(a.S_non + 8 * (size_t)i, S_non);
    sim3_store(a.S_cor + 8 * (size_t)i, S_cor);
  } else {
    S_cor = sim3_load(a.S_cor + 8 * (size_t)i);
    s3c_keyframe(nullptr, false, nullptr, S_cor, S_non, S_cor, S_swi, T, O);
  }
  sim3_store(a.S_swi + 8 * (size_t)i, S_swi);
#pragma unroll
  for (int k = 0; k < 12; k++) a.T_new[12 * (size_t)i + k] = T[k];
  a.c_new[3 * (size_t)i] = O[0]; a.c_new[3 * (size_t)i + 1] = O[1]; a.c_new[3 * (size_t)i + 2] = O[2];
}

__global__ __launch_bounds__(kS3cBlock) void sim3_correct_pt_kernel(S3cArgs a) {
  const int i = blockIdx.x * kS3cBlock + threadIdx.x;
  if (i >= a.n_pt) return;
  const size_t o = (size_t)a.owner[i];
  float p[3];
  s3c_point(sim3_load(a.S_non + 8 * o), sim3_load(a.S_swi + 8 * o), a.pos + 3 * (size_t)i, p);
  float n[3] = {a.normal_in[3 * (size_t)i], a.normal_in[3 * (size_t)i + 1], a.normal_in[3 * (size_t)i + 2]};
  float dmin = a.dmin_in[i], dmax = a.dmax_in[i];
  s3c_normal_depth(p, a.obs_off[i], a.obs_off[i + 1], a.obs_kf, a.n_kf, a.kf_rank, a.owner_rank[i], a.c_old, a.c_new, a.ref_kf[i], a.ref_level[i], a.scale_factors,
                   a.n_levels, n, dmin, dmax);
  a.pos_out[3 * (size_t)i] = p[0]; a.pos_out[3 * (size_t)i + 1] = p[1]; a.pos_out[3 * (size_t)i + 2] = p[2];
  a.normal_out[3 * (size_t)i] = n[0]; a.normal_out[3 * (size_t)i + 1] = n[1]; a.normal_out[3 * (size_t)i + 2] = n[2];
  a.dmin_out[i] = dmin; a.dmax_out[i] = dmax;
}

}  // namespace

extern "C" int ccm_sim3_correct_map(ccm_ctx* ctx, int n_kf, const float* Tiw, int cur, const float* Twc, const double* Scw, double* S_non, double* S_cor,
                                    int n_obs_kf, const float* kf_center, const int32_t* kf_rank, int n_pt, const float* pos, const int32_t* owner,
                                    const int32_t* owner_rank, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level,
                                    const float* scale_factors, int n_levels, float* pos_out, float* normal, float* min_dist, float* max_dist, float* Tiw_new,
                                    float* center_new) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_sim3_correct_map: ";
  if (n_kf < 1 || n_obs_kf < n_kf || n_pt < 0 || n_levels < 1 || !S_non || !S_cor || !kf_center || !kf_rank || !scale_factors || !Tiw_new || !center_new)
    return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
  if (Tiw && (!Twc || !Scw)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "the loop form needs Twc and Scw");
  if (Tiw && (cur < 0 || cur >= n_kf)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "current keyframe outside the set");
  size_t NO = 0;
  if (n_pt > 0) {
    if (!pos || !owner || !owner_rank || !obs_off || !ref_kf || !ref_level || !pos_out || !normal || !min_dist || !max_dist)
      return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
    if (obs_off[0] != 0) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "obs_off[0] != 0");
    for (int i = 0; i < n_pt; i++) {
      if (obs_off[i + 1] < obs_off[i]) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "obs_off decreases");
      if (owner[i] < 0 || owner[i] >= n_kf) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "owner outside the set");
      if (ref_kf[i] < 0 || ref_kf[i] >= n_obs_kf) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "reference keyframe out of range");
      if (ref_level[i] < 0 || ref_level[i] >= n_levels) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "level outside [0, n_levels)");
    }
    NO = (size_t)obs_off[n_pt];
    if (NO && !obs_kf) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
    for (size_t k = 0; k < NO; k++)
      if (obs_kf[k] < 0 || obs_kf[k] >= n_obs_kf) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "observer out of range");
  }
  const size_t K = (size_t)n_kf, P = (size_t)n_pt;
  const bool loop = Tiw != nullptr;
  S3cBlock b(K, (size_t)n_obs_kf, P, (size_t)n_levels, NO, loop);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  if (loop) { b.put(b.Scw, Scw); b.put(b.Twc, Twc); }
  b.put(b.S_non_in, S_non); b.put(b.S_cor_in, S_cor); b.put(b.Tiw, Tiw);
  b.put(b.c_old, kf_center); b.put(b.scale_factors, scale_factors);
  b.put(b.pos, pos); b.put(b.normal_in, normal); b.put(b.dmin_in, min_dist); b.put(b.dmax_in, max_dist);
  b.put(b.kf_rank, kf_rank); b.put(b.owner, owner); b.put(b.owner_rank, owner_rank);
  b.put(b.obs_off, obs_off); b.put(b.obs_kf, obs_kf); b.put(b.ref_kf, ref_kf); b.put(b.ref_level, ref_level);
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  S3cArgs a;
  a.n_kf = n_kf; a.n_pt = n_pt; a.cur = cur; a.n_levels = n_levels;
  a.Tiw = loop ? b.dev(b.Tiw) : nullptr;
  a.Twc = b.dev(b.Twc); a.Scw = b.dev(b.Scw);
  // the epilogue form reads the caller's tables where the upload put them; the loop form writes them among the outputs
  a.S_non = b.dev(loop ? b.S_non : b.S_non_in); a.S_cor = b.dev(loop ? b.S_cor : b.S_cor_in); a.S_swi = b.dev(b.S_swi);
  a.T_new = b.dev(b.T_new); a.c_new = b.dev(b.c_new);
  a.pos_out = b.dev(b.pos_out); a.normal_out = b.dev(b.normal_out); a.dmin_out = b.dev(b.dmin_out); a.dmax_out = b.dev(b.dmax_out);
  a.c_old = b.dev(b.c_old); a.kf_rank = b.dev(b.kf_rank); a.scale_factors = b.dev(b.scale_factors);
  a.pos = b.dev(b.pos); a.normal_in = b.dev(b.normal_in); a.dmin_in = b.dev(b.dmin_in); a.dmax_in = b.dev(b.dmax_in);
  a.owner = b.dev(b.owner); a.owner_rank = b.dev(b.owner_rank); a.obs_off = b.dev(b.obs_off);
  a.obs_kf = b.dev(b.obs_kf); a.ref_kf = b.dev(b.ref_kf); a.ref_level = b.dev(b.ref_level);
  hipLaunchKernelGGL(sim3_correct_kf_kernel, dim3((unsigned)((K + kS3cBlock - 1) / kS3cBlock)), dim3(kS3cBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (P) {
    hipLaunchKernelGGL(sim3_correct_pt_kernel, dim3((unsigned)((P + kS3cBlock - 1) / kS3cBlock)), dim3(kS3cBlock), 0, ctx->stream, a);
    CCM_HIP_CHECK(ctx, hipGetLastError());
  }
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  if (loop) { b.get(b.S_non, S_non); b.get(b.S_cor, S_cor); }   // the epilogue form's tables are the caller's own
  b.get(b.T_new, Tiw_new); b.get(b.c_new, center_new);
  b.get(b.pos_out, pos_out); b.get(b.normal_out, normal); b.get(b.dmin_out, min_dist); b.get(b.dmax_out, max_dist);
  return CCM_OK;
}
