// triangulate.hip — the per-match arithmetic of LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:353-448) on the device: ccm_triangulate_pairs.
//
// Layout: the new keyframe's pose record and intrinsics (TriCam, 21 floats), one TriCam per neighbour group, P matches in CSR over
// pair_off, per match the two undistorted keypoints (x1 y1 x2 y2) and their octaves, the level tables of both sides.  One lane per match, 64 lanes
// per workgroup (a keyframe has a few thousand matches: small workgroups spread them over the CUs).  Each lane runs tri_pair of triangulate_math.h;
// the 4x4 Jacobi state has fixed indices only and stays in registers.  Lanes whose match fails the parallax gate leave before the SVD.
#include "common.h"
#include "triangulate_math.h"

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
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // device block (4-byte words): inputs [xy 4P | cam1 21 | cam2 21S | four tables nlevels each | oct P | grp P], then outputs [x3d 3P | status P bytes].
  // xy comes first so that its float4 reads are 16-byte aligned.  One H2D of the inputs, one D2H of the outputs, both through the pinned staging buffer.
  const size_t L = (size_t)nlevels;
  const size_t n_in = (4 * P + TRI_CAM_FLOATS * (size_t)(S + 1) + 4 * L + 2 * P + 3) & ~(size_t)3;
  const size_t n_out = 3 * P + (P + 3) / 4;
  void* scratch = nullptr;
  int rc = ccm_scratch(ctx, (n_in + n_out) * 4 + 64, &scratch);
  if (rc) return rc;
  void* pin = nullptr;
  rc = ccm_pin_scratch(ctx, (n_in > n_out ? n_in : n_out) * 4 + 64, &pin);
  if (rc) return rc;
  uint32_t* hp = (uint32_t*)pin;
  size_t o = 0;
  auto put = [&](const void* src, size_t n) { memcpy(hp + o, src, n * 4); o += n; };
  const size_t o_xy = o; put(xy, 4 * P);
  const size_t o_c1 = o; put(cam1, TRI_CAM_FLOATS);
  const size_t o_c2 = o; put(cam2, TRI_CAM_FLOATS * (size_t)S);
  const size_t o_s1 = o; put(sigma2_1, L);
  const size_t o_f1 = o; put(sf_1, L);
  const size_t o_s2 = o; put(sigma2_2, L);
  const size_t o_f2 = o; put(sf_2, L);
  const size_t o_oc = o;
  for (size_t i = 0; i < P; i++) hp[o++] = (uint32_t)oct[2 * i] | ((uint32_t)oct[2 * i + 1] << 16);
  const size_t o_gr = o;
  for (int s = 0; s < S; s++)
    for (int i = pair_off[s]; i < pair_off[s + 1]; i++) hp[o++] = (uint32_t)s;
  uint32_t* d = (uint32_t*)scratch;
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(d, hp, n_in * 4, hipMemcpyHostToDevice, ctx->stream));
  TriArgs a;
  a.P = (int)P;
  a.xy = (const float*)(d + o_xy); a.cam1 = (const float*)(d + o_c1); a.cam2 = (const float*)(d + o_c2);
  a.sigma2_1 = (const float*)(d + o_s1); a.sf_1 = (const float*)(d + o_f1); a.sigma2_2 = (const float*)(d + o_s2); a.sf_2 = (const float*)(d + o_f2);
  a.oct = d + o_oc; a.grp = (const int32_t*)(d + o_gr);
  a.ratioFactor = ratioFactor;
  uint32_t* dout = d + n_in;
  a.x3d = (float*)dout; a.status = (uint8_t*)(dout + 3 * P);
  hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)((P + kTriBlock - 1) / kTriBlock)), dim3(kTriBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(hp, dout, n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(x3d, hp, 3 * P * 4);
  memcpy(status, hp + 3 * P, P);
  // n_accepted: counted from the status bytes that have just come back (a device count would need a zeroing pass and atomics for a few thousand bytes)
  for (int s = 0; s < S; s++) {
    int32_t n = 0;
    for (int i = pair_off[s]; i < pair_off[s + 1]; i++) n += status[i] == TRI_OK;
    n_accepted[s] = n;
  }
  return CCM_OK;
}
