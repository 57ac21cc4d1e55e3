// gba_apply.hip — a finished global BA applied to the map on the device: ccm_gba_apply_map (Optimizer.cpp:803-857, then the walk of RunGBA: Map.cpp:1441-1568,
// LoopFinder.cpp ~895-1010, MapMerger.cpp ~640-755).
//
// Layout: per keyframe of the walk, in walk order, its parent, its camera in the BA problem (-1: it was no vertex), its pose and inverse
// pose before the walk, its new pose and the [Rwc | Ow] that SetPose leaves; per point its position, its landmark (-1: none) and its reference keyframe in the
// walk (-1: none).  The optimised state is 7 doubles per camera and 3 per landmark, uploaded by the host form and read in place from a ccm_ba handle by the
// handle form.  Three kernels on the context's stream: one lane per keyframe (vertices only), ONE workgroup that takes the keyframes that were no vertices
// level by level (a child needs its parent's finished pose and f32 products do not re-associate: there is nothing to jump over), one lane per point, 64 lanes
// per workgroup (the §13 reasoning: 10^3 .. 10^5 points spread over the CUs in small workgroups).  The pose tables are a few thousand keyframes x 48 bytes and
// stay in L2.
#include "common.h"
#include "gba_apply_math.h"
#include "stage_blocks.h"
#include <vector>

struct ccm_ba;
namespace ccm_internal {
// ba.hip: the device state of a handle in the caller's numbering.  stage_points == 0 launches nothing.
int ba_gba_state(ccm_ba* ba, int stage_points, ccm_ctx** ctx, int* nranks, int* n_cam, int* n_lm, const double** d_cam_qt, const double** d_cam_raw,
                 const int** d_slot_cam, int* n_slot, const double** d_pt_xyz);
}

namespace {

constexpr int kGbaBlock = 64;
constexpr int kGbaTreeBlock = 256;

struct GbaArgs {
  int n_kf, n_pt, n_lvl;
  const double* cam_qt;        // [n_cam * 7]
  const double* cam_raw;       // handle form: [n_cam * 7] the cameras as uploaded to the handle; nullptr in the host form
  const int* slot_cam;         // handle form: [n_slot] the cameras that carry an estimate, ascending
  int n_slot;
  const double* pt_xyz;        // [n_lm * 3]
  const float* Tcw_old;        // [n_kf * 12]
  const float* Twc_old;        // [n_kf * 12]
  const float* pos;            // [n_pt * 3]
  const int32_t* kf_parent;    // [n_kf]
  const int32_t* kf_cam;       // [n_kf]
  const int32_t* pt_vert;      // [n_pt]
  const int32_t* pt_ref;       // [n_pt]
  const int32_t* tree_kf;      // [n_tree] the keyframes that were no vertices, by depth
  const int32_t* lvl_off;      // [n_lvl + 1]
  float* T_new;                // [n_kf * 12]
  float* Twc_new;              // [n_kf * 12]
  float* pos_out;              // [n_pt * 3]
  uint8_t* status;             // [n_pt]
};

__device__ inline void gba_store_pose(float* dst, const float T[12]) {
#pragma unroll
  for (int k = 0; k < 12; k++) dst[k] = T[k];
}

__global__ __launch_bounds__(kGbaBlock) void gba_apply_kf_kernel(GbaArgs a) {
  const int i = blockIdx.x * kGbaBlock + threadIdx.x;
  if (i >= a.n_kf) return;
  const int c = a.kf_cam[i];
  if (c < 0) return;   // the tree kernel's
  const double* qt = a.cam_qt + 7 * (size_t)c;
  if (a.cam_raw) {   // as ccm_ba_download: a camera that was no free vertex of the handle (fixed, or without an active edge) keeps the caller's values
    int lo = 0, hi = a.n_slot;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.slot_cam[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo >= a.n_slot || a.slot_cam[lo] != c) qt = a.cam_raw + 7 * (size_t)c;
  }
  float T[12], Twc[12];
  gba_pose_of_se3(qt, T);
  gba_twc(T, Twc);
  gba_store_pose(a.T_new + 12 * (size_t)i, T);
  gba_store_pose(a.Twc_new + 12 * (size_t)i, Twc);
}

// ONE workgroup.  Level l holds the keyframes at depth l + 1 below their nearest vertex ancestor; a parent is a vertex (written by the launch before) or sits one
// level up (written before the barrier, which orders the workgroup's global stores and loads).
__global__ __launch_bounds__(kGbaTreeBlock) void gba_apply_tree_kernel(GbaArgs a) {
  for (int l = 0; l < a.n_lvl; l++) {
    const int e = a.lvl_off[l + 1];
    for (int j = a.lvl_off[l] + (int)threadIdx.x; j < e; j += kGbaTreeBlock) {
      const size_t k = (size_t)a.tree_kf[j], p = (size_t)a.kf_parent[k];
      float Tp[12], T[12], Twc[12];
#pragma unroll
      for (int q = 0; q < 12; q++) Tp[q] = a.T_new[12 * p + q];
      gba_child_pose(a.Tcw_old + 12 * k, a.Twc_old + 12 * p, Tp, T);
      gba_twc(T, Twc);
      gba_store_pose(a.T_new + 12 * k, T);
      gba_store_pose(a.Twc_new + 12 * k, Twc);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kGbaBlock) void gba_apply_pt_kernel(GbaArgs a) {
  const int i = blockIdx.x * kGbaBlock + threadIdx.x;
  if (i >= a.n_pt) return;
  const float P[3] = {a.pos[3 * (size_t)i], a.pos[3 * (size_t)i + 1], a.pos[3 * (size_t)i + 2]};
  float out[3];
  a.status[i] = gba_point(a.pt_vert[i], a.pt_ref[i], a.pt_xyz, a.Tcw_old, a.Twc_new, P, out);
  a.pos_out[3 * (size_t)i] = out[0]; a.pos_out[3 * (size_t)i + 1] = out[1]; a.pos_out[3 * (size_t)i + 2] = out[2];
}

}  // namespace

extern "C" int ccm_gba_apply_map(ccm_ctx* ctx, int n_kf, const int32_t* kf_parent, const int32_t* kf_cam, const float* Tcw_old, const float* Twc_old, int n_pt,
                                 const float* pos, const int32_t* pt_vert, const int32_t* pt_ref, int n_cam, const double* cam_qt, int n_lm, const double* pt_xyz,
                                 ccm_ba* ba, float* T_new, float* Twc_new, float* pos_out, uint8_t* pt_status) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_gba_apply_map: ";
  if (n_kf < 1 || n_pt < 0 || !kf_parent || !kf_cam || !Tcw_old || !Twc_old || !T_new || !Twc_new) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
  if (n_pt > 0 && (!pos || !pt_vert || !pt_ref || !pos_out || !pt_status)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
  const bool handle = ba != nullptr;
  if (handle ? (cam_qt || pt_xyz) : !cam_qt) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "the optimised state comes as host arrays or as a handle, one of the two");
  if (handle) {
    ccm_ctx* bctx = nullptr; int nranks = 1;
    if (int rc = ccm_internal::ba_gba_state(ba, 0, &bctx, &nranks, &n_cam, &n_lm, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    if (bctx != ctx) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "the handle belongs to another context");
    if (nranks > 1) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "a sharded handle needs the collective download");
  }
  if (n_cam < 1 || n_lm < 0 || (!handle && n_lm > 0 && !pt_xyz)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
  std::vector<int32_t> depth((size_t)n_kf);
  int n_tree = 0, n_lvl = 0;
  if (const char* why = gba_check_walk(n_kf, kf_parent, kf_cam, n_cam, depth.data(), &n_tree, &n_lvl)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  if (const char* why = gba_check_points(n_pt, pt_vert, pt_ref, n_lm, n_kf)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  const size_t K = (size_t)n_kf, P = (size_t)n_pt;
  GbaApplyBlock b(K, P, handle ? 0 : (size_t)n_cam, handle ? 0 : (size_t)n_lm, (size_t)n_tree, (size_t)n_lvl);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  b.put(b.cam_qt, cam_qt); b.put(b.pt_xyz, pt_xyz);
  b.put(b.Tcw_old, Tcw_old); b.put(b.Twc_old, Twc_old); b.put(b.pos, pos);
  b.put(b.kf_parent, kf_parent); b.put(b.kf_cam, kf_cam); b.put(b.pt_vert, pt_vert); b.put(b.pt_ref, pt_ref);
  if (n_tree) gba_tree_levels(n_kf, depth.data(), n_lvl, b.up(b.tree_kf), b.up(b.lvl_off));
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  GbaArgs a;
  a.n_kf = n_kf; a.n_pt = n_pt; a.n_lvl = n_lvl;
  a.cam_qt = b.dev(b.cam_qt); a.pt_xyz = b.dev(b.pt_xyz); a.cam_raw = nullptr; a.slot_cam = nullptr; a.n_slot = 0;
  if (handle) {   // the handle's own buffers, landmarks brought into the caller's numbering on this stream
    ccm_ctx* bctx = nullptr; int nranks = 1;
    if (int rc = ccm_internal::ba_gba_state(ba, 1, &bctx, &nranks, &n_cam, &n_lm, &a.cam_qt, &a.cam_raw, &a.slot_cam, &a.n_slot, &a.pt_xyz)) return rc;
  }
  a.Tcw_old = b.dev(b.Tcw_old); a.Twc_old = b.dev(b.Twc_old); a.pos = b.dev(b.pos);
  a.kf_parent = b.dev(b.kf_parent); a.kf_cam = b.dev(b.kf_cam); a.pt_vert = b.dev(b.pt_vert); a.pt_ref = b.dev(b.pt_ref);
  a.tree_kf = b.dev(b.tree_kf); a.lvl_off = b.dev(b.lvl_off);
  a.T_new = b.dev(b.T_new); a.Twc_new = b.dev(b.Twc_new); a.pos_out = b.dev(b.pos_out); a.status = b.dev(b.status);
  hipLaunchKernelGGL(gba_apply_kf_kernel, dim3((unsigned)((K + kGbaBlock - 1) / kGbaBlock)), dim3(kGbaBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (n_tree) {
    hipLaunchKernelGGL(gba_apply_tree_kernel, dim3(1), dim3(kGbaTreeBlock), 0, ctx->stream, a);
    CCM_HIP_CHECK(ctx, hipGetLastError());
  }
  if (P) {
    hipLaunchKernelGGL(gba_apply_pt_kernel, dim3((unsigned)((P + kGbaBlock - 1) / kGbaBlock)), dim3(kGbaBlock), 0, ctx->stream, a);
    CCM_HIP_CHECK(ctx, hipGetLastError());
  }
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.T_new, T_new); b.get(b.Twc_new, Twc_new); b.get(b.pos_out, pos_out); b.get(b.status, pt_status);
  return CCM_OK;
}
