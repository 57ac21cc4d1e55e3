// sim3ransac.hip — the RANSAC hypotheses of cslam::Sim3Solver (cslam/src/Sim3Solver.cpp) on the device: ccm_sim3_ransac_eval.
//
// Layout: K candidates in CSR over pt_off, per point mvX3Dc1 / mvX3Dc2 (f32 x 3) and the integer thresholds mvnMaxError1/2,
// per candidate K1 / K2 (fx fy cx cy).  H hypotheses, each a candidate and three distinct point indices (the host already mapped the random
// draws).  The wave is ransac_wave.h's (one wave64 per hypothesis, the ballot's mask words and count); this file holds its Sim3 form: lane 0's
// serial three-point solve (centroids, Horn's 4x4 matrix, Jacobi, Rodrigues, scale, translation) and the test of a point projected both ways are
// Sim3HypForm of sim3_ransac_math.h, and the two transforms reach the other lanes through the shuffles below.  The kernel declares no LDS.
#include "common.h"
#include "ransac_wave.h"
#include "sim3_ransac_math.h"
#include "stage_blocks.h"

namespace {

struct Sim3Form : Sim3HypForm {
  using Sim3HypForm::Sim3HypForm;
  __device__ void broadcast() {   // the two transforms (sR | t, sRinv | tinv) from lane 0
    for (int i = 0; i < 9; i++) { hy.sR[i] = __shfl(hy.sR[i], 0); hy.sRi[i] = __shfl(hy.sRi[i], 0); }
    for (int i = 0; i < 3; i++) { hy.t[i] = __shfl(hy.t[i], 0); hy.ti[i] = __shfl(hy.ti[i], 0); }
  }
};

__global__ __launch_bounds__(64 * kRansacWavesPerBlock) void sim3_ransac_kernel(Sim3RansacArgs a) { ransac_wave<Sim3Form>(a, nullptr); }

}  // namespace

extern "C" int ccm_sim3_ransac_eval(ccm_ctx* ctx, int K, const int32_t* pt_off, const float* X3Dc1, const float* X3Dc2, const float* K1,
                                    const float* K2, const uint32_t* max_err1, const uint32_t* max_err2, int H, const int32_t* hyp_cand,
                                    const int32_t* hyp_idx, int fix_scale, int32_t* n_inl, float* rts, int32_t* mask_off, uint32_t* mask) {
  if (!ctx) return CCM_E_ARG;
  if (K < 1 || H < 0 || !pt_off || !X3Dc1 || !X3Dc2 || !K1 || !K2 || !max_err1 || !max_err2 || !mask_off ||
      (H > 0 && (!hyp_cand || !hyp_idx || !n_inl || !rts || !mask)))
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: bad args");
  int64_t words = 0;
  if (const RansacCheck r = ransac_check_hyps<3>(K, pt_off, H, hyp_cand, hyp_idx, mask_off, &words, /*range_first=*/true))
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: " + ransac_check_text(r, 3));
  if (H == 0) return CCM_OK;
  Sim3RansacBlock b((size_t)K, (size_t)pt_off[K], (size_t)H, (size_t)words);
  if (int rc = ccm_staged_begin(ctx, b, "ccm_sim3_ransac_eval: ")) return rc;
  b.put(b.pt_off, pt_off); b.put(b.X1, X3Dc1); b.put(b.X2, X3Dc2); b.put(b.K1, K1); b.put(b.K2, K2); b.put(b.thr1, max_err1); b.put(b.thr2, max_err2);
  b.put(b.hyp_cand, hyp_cand); b.put(b.hyp_idx, hyp_idx); b.put(b.mask_off, mask_off);
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  Sim3RansacArgs a;
  a.K = K; a.H = H; a.fix_scale = fix_scale ? 1 : 0;
  a.pt_off = b.dev(b.pt_off); a.X1 = b.dev(b.X1); a.X2 = b.dev(b.X2); a.K1 = b.dev(b.K1); a.K2 = b.dev(b.K2); a.thr1 = b.dev(b.thr1); a.thr2 = b.dev(b.thr2);
  a.hyp_cand = b.dev(b.hyp_cand); a.hyp_idx = b.dev(b.hyp_idx); a.mask_off = b.dev(b.mask_off);
  a.n_inl = b.dev(b.n_inl); a.rts = b.dev(b.rts); a.mask = b.dev(b.mask);
  hipLaunchKernelGGL(sim3_ransac_kernel, dim3((H + kRansacWavesPerBlock - 1) / kRansacWavesPerBlock), dim3(64 * kRansacWavesPerBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.n_inl, n_inl); b.get(b.rts, rts); b.get(b.mask, mask);
  return CCM_OK;
}
