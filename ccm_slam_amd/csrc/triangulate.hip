// triangulate.hip — the per-match arithmetic of LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:353-448) on the device: ccm_triangulate_pairs.
//
// Layout: the new keyframe's pose record and intrinsics (TriCam, 21 floats), one TriCam per neighbour group, P matches in CSR over
// pair_off, per match the two undistorted keypoints (x1 y1 x2 y2) and their octaves, the level tables of both sides.  One lane per match, 64 lanes
// per workgroup (a keyframe has a few thousand matches: small workgroups spread them over the CUs).  Each lane runs tri_pair of triangulate_math.h;
// the 4x4 Jacobi state has fixed indices only and stays in registers.  Lanes whose match fails the parallax gate leave before the SVD.
#include "common.h"
#include "triangulate_math.h"
#include "stage_blocks.h"

namespace {

constexpr int kTriBlock = 64;

struct TriArgs {
  int P;
  const float* cam1;      // [21]
  const float* cam2;      // [S * 21]
  const float* sigma2_1;  // [nlevels] each
  const float* sf_1;
  const float* sigma2_2;
  const float* sf_2;
  const float* xy;        // [P * 4]
  const uint32_t* oct;    // [P]: oct1 | oct2 << 16
  const int32_t* grp;     // [P]
  float ratioFactor;
  float* x3d;             // [P * 3]
  uint8_t* status;        // [P]
};

__device__ inline TriCam tri_load_cam(const float* p) {
  TriCam c;
  for (int i = 0; i < 9; i++) c.Rcw[i] = p[i];
  for (int i = 0; i < 3; i++) { c.tcw[i] = p[9 + i]; c.Ow[i] = p[12 + i]; }
  c.fx = p[15]; c.fy = p[16]; c.cx = p[17]; c.cy = p[18]; c.invfx = p[19]; c.invfy = p[20];
  return c;
}

__global__ __launch_bounds__(kTriBlock) void triangulate_kernel(TriArgs a) {
  const int i = blockIdx.x * kTriBlock + threadIdx.x;
  if (i >= a.P) return;
  const TriCam c1 = tri_load_cam(a.cam1);
  const TriCam c2 = tri_load_cam(a.cam2 + (size_t)a.grp[i] * TRI_CAM_FLOATS);
  const float4 k = reinterpret_cast<const float4*>(a.xy)[i];
  const uint32_t o = a.oct[i];
  float X[3];
  const int st = tri_pair(c1, c2, k.x, k.y, (int)(o & 0xffffu), k.z, k.w, (int)(o >> 16), a.sigma2_1, a.sf_1, a.sigma2_2, a.sf_2, a.ratioFactor, X);
  a.x3d[3 * (size_t)i] = X[0]; a.x3d[3 * (size_t)i + 1] = X[1]; a.x3d[3 * (size_t)i + 2] = X[2];
  a.status[i] = (uint8_t)st;
}

}  // namespace

extern "C" int ccm_triangulate_pairs(ccm_ctx* ctx, const float* cam1, int S, const float* cam2, const int32_t* pair_off, const float* xy, const int32_t* oct,
                                     int nlevels, const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2, float ratioFactor,
                                     uint8_t* status, float* x3d, int32_t* n_accepted) {
  if (!ctx) return CCM_E_ARG;
  if (S < 1 || nlevels < 1 || nlevels > 0xffff || !cam1 || !cam2 || !pair_off || !sigma2_1 || !sf_1 || !sigma2_2 || !sf_2 || !n_accepted)
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_triangulate_pairs: bad args");
  if (pair_off[0] != 0) return ccm_set_error(ctx, CCM_E_ARG, "ccm_triangulate_pairs: pair_off[0] != 0");
  for (int s = 0; s < S; s++)
    if (pair_off[s + 1] < pair_off[s]) return ccm_set_error(ctx, CCM_E_ARG, "ccm_triangulate_pairs: pair_off decreases");
  const size_t P = (size_t)pair_off[S];
  for (int s = 0; s < S; s++) n_accepted[s] = 0;
  if (P == 0) return CCM_OK;
  if (!xy || !oct || !status || !x3d) return ccm_set_error(ctx, CCM_E_ARG, "ccm_triangulate_pairs: bad args");
  for (size_t i = 0; i < 2 * P; i++)
    if (oct[i] < 0 || oct[i] >= nlevels) return ccm_set_error(ctx, CCM_E_ARG, "ccm_triangulate_pairs: octave outside [0, nlevels)");
  TriBlock b(P, (size_t)S, (size_t)nlevels);
  if (int rc = ccm_staged_begin(ctx, b, "ccm_triangulate_pairs: ")) return rc;
  b.put(b.xy, xy); b.put(b.cam1, cam1); b.put(b.cam2, cam2);
  b.put(b.sigma2_1, sigma2_1); b.put(b.sf_1, sf_1); b.put(b.sigma2_2, sigma2_2); b.put(b.sf_2, sf_2);
  uint32_t* h_oct = b.up(b.oct);
  for (size_t i = 0; i < P; i++) h_oct[i] = (uint32_t)oct[2 * i] | ((uint32_t)oct[2 * i + 1] << 16);
  int32_t* h_grp = b.up(b.grp);
  for (int s = 0; s < S; s++)
    for (int i = pair_off[s]; i < pair_off[s + 1]; i++) h_grp[i] = s;
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  TriArgs a;
  a.P = (int)P;
  a.xy = b.dev(b.xy); a.cam1 = b.dev(b.cam1); a.cam2 = b.dev(b.cam2);
  a.sigma2_1 = b.dev(b.sigma2_1); a.sf_1 = b.dev(b.sf_1); a.sigma2_2 = b.dev(b.sigma2_2); a.sf_2 = b.dev(b.sf_2);
  a.oct = b.dev(b.oct); a.grp = b.dev(b.grp);
  a.ratioFactor = ratioFactor;
  a.x3d = b.dev(b.x3d); a.status = b.dev(b.status);
  hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)((P + kTriBlock - 1) / kTriBlock)), dim3(kTriBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.x3d, x3d); b.get(b.status, status);
  // n_accepted: counted from the status bytes that have just come back (a device count would need a zeroing pass and atomics for a few thousand bytes)
  for (int s = 0; s < S; s++) {
    int32_t n = 0;
    for (int i = pair_off[s]; i < pair_off[s + 1]; i++) n += status[i] == TRI_OK;
    n_accepted[s] = n;
  }
  return CCM_OK;
}
