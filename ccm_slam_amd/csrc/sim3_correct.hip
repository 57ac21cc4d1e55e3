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
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // device block in 4-byte words, the doubles first (8-byte aligned).  inputs: [Scw 8d | S_non 8d n_kf | S_cor 8d n_kf (epilogue form only)] [Twc 12 |
  // Tiw 12 n_kf | centres 3 n_obs_kf | scale n_levels | pos 3P | normal 3P | dmin P | dmax P] [rank n_obs_kf | owner P | owner_rank P | obs_off P+1 |
  // obs_kf NO | ref_kf P | ref_level P]; outputs: [S_non 8d n_kf | S_cor 8d n_kf] [pose 12 n_kf | centre 3 n_kf | pos 3P | normal 3P | dmin P | dmax P], then
  // S_swi 8d n_kf, which stays on the device.  One H2D of the inputs, one D2H of the outputs, both through the pinned staging buffer.
  const size_t K = (size_t)n_kf, KO = (size_t)n_obs_kf, P = (size_t)n_pt, L = (size_t)n_levels;
  const bool loop = Tiw != nullptr;
  const size_t n_in_d = 8 + (loop ? 0 : 16 * K);
  const size_t n_in = (2 * n_in_d + 12 + (loop ? 12 * K : 0) + 3 * KO + L + 8 * P + KO + 2 * P + (P ? P + 1 : 0) + NO + 2 * P + 1) & ~(size_t)1;
  const size_t n_out = (2 * 16 * K + 15 * K + 8 * P + 1) & ~(size_t)1;
  void* scratch = nullptr;
  int rc = ccm_scratch(ctx, (n_in + n_out + 2 * 8 * K) * 4 + 64, &scratch);
  if (rc) return rc;
  void* pin = nullptr;
  rc = ccm_pin_scratch(ctx, (n_in > n_out ? n_in : n_out) * 4 + 64, &pin);
  if (rc) return rc;
  uint32_t* hp = (uint32_t*)pin;
  size_t o = 0;
  auto put = [&](const void* src, size_t n) { const size_t at = o; if (n) memcpy(hp + o, src, n * 4); o += n; return at; };
  auto skip = [&](size_t n) { const size_t at = o; memset(hp + o, 0, n * 4); o += n; return at; };
  const size_t o_scw = loop ? put(Scw, 16) : skip(16);
  const size_t o_snon = loop ? 0 : put(S_non, 16 * K);
  const size_t o_scor = loop ? 0 : put(S_cor, 16 * K);
  const size_t o_twc = loop ? put(Twc, 12) : skip(12);
  const size_t o_tiw = loop ? put(Tiw, 12 * K) : 0;
  const size_t o_cen = put(kf_center, 3 * KO);
  const size_t o_sf = put(scale_factors, L);
  const size_t o_pos = put(pos, 3 * P);
  const size_t o_nrm = put(normal, 3 * P);
  const size_t o_dmin = put(min_dist, P);
  const size_t o_dmax = put(max_dist, P);
  const size_t o_rank = put(kf_rank, KO);
  const size_t o_own = put(owner, P);
  const size_t o_ork = put(owner_rank, P);
  const size_t o_off = put(obs_off, P ? P + 1 : 0);
  const size_t o_okf = put(obs_kf, NO);
  const size_t o_ref = put(ref_kf, P);
  const size_t o_lvl = put(ref_level, P);
  uint32_t* d = (uint32_t*)scratch;
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(d, hp, n_in * 4, hipMemcpyHostToDevice, ctx->stream));
  uint32_t* dout = d + n_in;
  S3cArgs a;
  a.n_kf = n_kf; a.n_pt = n_pt; a.cur = cur; a.n_levels = n_levels;
  a.Tiw = loop ? (const float*)(d + o_tiw) : nullptr;
  a.Twc = (const float*)(d + o_twc); a.Scw = (const double*)(d + o_scw);
  // the epilogue form reads the caller's tables where the H2D copy put them; the loop form writes them into the output block
  a.S_non = loop ? (double*)dout : (double*)(d + o_snon);
  a.S_cor = loop ? (double*)(dout + 16 * K) : (double*)(d + o_scor);
  a.S_swi = (double*)(dout + n_out);
  a.T_new = (float*)(dout + 32 * K); a.c_new = a.T_new + 12 * K;
  a.pos_out = a.c_new + 3 * K; a.normal_out = a.pos_out + 3 * P; a.dmin_out = a.normal_out + 3 * P; a.dmax_out = a.dmin_out + P;
  a.c_old = (const float*)(d + o_cen); a.kf_rank = (const int32_t*)(d + o_rank); a.scale_factors = (const float*)(d + o_sf);
  a.pos = (const float*)(d + o_pos); a.normal_in = (const float*)(d + o_nrm); a.dmin_in = (const float*)(d + o_dmin); a.dmax_in = (const float*)(d + o_dmax);
  a.owner = (const int32_t*)(d + o_own); a.owner_rank = (const int32_t*)(d + o_ork); a.obs_off = (const int32_t*)(d + o_off);
  a.obs_kf = (const int32_t*)(d + o_okf); a.ref_kf = (const int32_t*)(d + o_ref); a.ref_level = (const int32_t*)(d + o_lvl);
  hipLaunchKernelGGL(sim3_correct_kf_kernel, dim3((unsigned)((K + kS3cBlock - 1) / kS3cBlock)), dim3(kS3cBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (P) {
    hipLaunchKernelGGL(sim3_correct_pt_kernel, dim3((unsigned)((P + kS3cBlock - 1) / kS3cBlock)), dim3(kS3cBlock), 0, ctx->stream, a);
    CCM_HIP_CHECK(ctx, hipGetLastError());
  }
  // the loop form copies the two Sim3 tables back with the rest; the epilogue form's are the caller's own and are skipped
  const size_t skip_out = loop ? 0 : 32 * K;
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(hp, dout + skip_out, (n_out - skip_out) * 4, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const uint32_t* h = hp;
  if (loop) { memcpy(S_non, h, 16 * K * 4); memcpy(S_cor, h + 16 * K, 16 * K * 4); h += 32 * K; }
  memcpy(Tiw_new, h, 12 * K * 4); h += 12 * K;
  memcpy(center_new, h, 3 * K * 4); h += 3 * K;
  if (P) {
    memcpy(pos_out, h, 3 * P * 4); h += 3 * P;
    memcpy(normal, h, 3 * P * 4); h += 3 * P;
    memcpy(min_dist, h, P * 4); h += P;
    memcpy(max_dist, h, P * 4);
  }
  return CCM_OK;
}
