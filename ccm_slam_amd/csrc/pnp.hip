// pnp.hip — the RANSAC hypotheses of cslam::PnPsolver (cslam/src/PnPSolver.cpp) on the device: ccm_pnp_ransac_eval.
//
// Layout: K candidates in CSR over pt_off, per point mvP3Dw (f32 x 3), mvP2D (f32 x 2) and mvMaxError (f32), per candidate fu fv uc vc (f64).
// H hypotheses, each a candidate and four distinct point indices (the host already mapped the random draws).  One wave64 per hypothesis, kRansacWavesPerBlock waves
// per workgroup: lane 0 runs the serial EPnP compute_pose of pnp_math.h on its four correspondences and hands R and t to the wave through lane shuffles; the lanes
// then stride over the candidate's points and a ballot gives 64 inlier bits at a time (two mask words) and the count.  The solve's two large run-time indexed arrays
// (M, 8 x 12, and M' M / Ut, 12 x 12, f64) live in an LDS slice per wave: in private memory they would be scratch for all 64 lanes of a wave of which one works.
// The Jacobi sweeps stay on one lane: every sum keeps the header's sequential order, so the device equals the host evaluator bit for bit.
//
// The wave is that of ransac_wave.h, written out.  It is not ransac_wave<F>: this kernel runs at 256 VGPRs and one wave per SIMD and its time is lane 0's solve,
// and as soon as the call of pnp_compute_pose sits in a function of its own (a form's solve, force-inlined or not) the compiler forwards compute_pose's Betas
// through registers instead of scratch, which costs 156 more AGPR copies in the solve (1 172 against 1 016) at the same arithmetic.  The checks of the entry
// point, the arguments and the host walk (PnpHypForm of pnp_math.h) are the shared ones.
#include "common.h"
#include "pnp_math.h"
#include "ransac_wave.h"
#include "stage_blocks.h"

namespace {

__global__ __launch_bounds__(64 * kRansacWavesPerBlock) void pnp_ransac_kernel(PnpRansacArgs a) {
  __shared__ double s_work[kRansacWavesPerBlock][PnpHypForm::kWorkDoubles];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int h = blockIdx.x * kRansacWavesPerBlock + wave;
  if (h >= a.H) return;   // whole waves only: no barrier below
  const int c = a.hyp_cand[h];
  const int p0 = a.pt_off[c], N = a.pt_off[c + 1] - p0;
  const double cam[4] = {a.cam[4 * c], a.cam[4 * c + 1], a.cam[4 * c + 2], a.cam[4 * c + 3]};
  double R[9] = {}, t[3] = {};   // lanes 1..63 take lane 0's pose through the shuffles below
  if (lane == 0) {
    double pws[12], us[8], alphas[16], pcs[12];
    for (int j = 0; j < 4; j++) {
      const size_t i = (size_t)(p0 + a.hyp_idx[4 * h + j]);
      for (int r = 0; r < 3; r++) pws[3 * j + r] = a.P3Dw[3 * i + r];
      for (int r = 0; r < 2; r++) us[2 * j + r] = a.P2D[2 * i + r];
    }
    pnp_compute_pose(4, pws, us, cam, alphas, pcs, s_work[wave], s_work[wave] + 96, R, t, nullptr, nullptr);
    double* o = a.Rt + 12 * (size_t)h;
    for (int i = 0; i < 9; i++) o[i] = R[i];
    for (int i = 0; i < 3; i++) o[9 + i] = t[i];
  }
  for (int i = 0; i < 9; i++) R[i] = __shfl(R[i], 0);
  for (int i = 0; i < 3; i++) t[i] = __shfl(t[i], 0);
  uint32_t* m = a.mask + a.mask_off[h];
  const int n_words = (N + 31) >> 5;
  int count = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < N) {
      const size_t g = (size_t)(p0 + i);
      in = pnp_inlier(R, t, cam, a.P3Dw + 3 * g, a.P2D + 2 * g, a.max_err[g]);
    }
    const uint64_t b = __ballot(in);
    count += __popcll(b);
    const int w = base >> 5;
    if (lane == 0) m[w] = (uint32_t)b;
    if (lane == 1 && w + 1 < n_words) m[w + 1] = (uint32_t)(b >> 32);
  }
  if (lane == 0) a.n_inl[h] = count;
}

}  // namespace

extern "C" int ccm_pnp_ransac_eval(ccm_ctx* ctx, int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* max_err, const double* cam,
                                   int H, const int32_t* hyp_cand, const int32_t* hyp_idx, int32_t* n_inl, double* Rt, int32_t* mask_off, uint32_t* mask) {
  if (!ctx) return CCM_E_ARG;
  if (K < 1 || H < 0 || !pt_off || !P3Dw || !P2D || !max_err || !cam || !mask_off || (H > 0 && (!hyp_cand || !hyp_idx || !n_inl || !Rt || !mask)))
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: bad args");
  int64_t words = 0;
  if (const RansacCheck r = ransac_check_hyps<4>(K, pt_off, H, hyp_cand, hyp_idx, mask_off, &words, /*range_first=*/false))
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: " + ransac_check_text(r, 4));
  if (H == 0) return CCM_OK;
  PnpRansacBlock b((size_t)K, (size_t)pt_off[K], (size_t)H, (size_t)words);
  if (int rc = ccm_staged_begin(ctx, b, "ccm_pnp_ransac_eval: ")) return rc;
  b.put(b.cam, cam); b.put(b.pt_off, pt_off); b.put(b.P3Dw, P3Dw); b.put(b.P2D, P2D); b.put(b.max_err, max_err);
  b.put(b.hyp_cand, hyp_cand); b.put(b.hyp_idx, hyp_idx); b.put(b.mask_off, mask_off);
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  PnpRansacArgs a;
  a.K = K; a.H = H;
  a.cam = b.dev(b.cam); a.pt_off = b.dev(b.pt_off); a.P3Dw = b.dev(b.P3Dw); a.P2D = b.dev(b.P2D); a.max_err = b.dev(b.max_err);
  a.hyp_cand = b.dev(b.hyp_cand); a.hyp_idx = b.dev(b.hyp_idx); a.mask_off = b.dev(b.mask_off);
  a.Rt = b.dev(b.Rt); a.n_inl = b.dev(b.n_inl); a.mask = b.dev(b.mask);
  hipLaunchKernelGGL(pnp_ransac_kernel, dim3((H + kRansacWavesPerBlock - 1) / kRansacWavesPerBlock), dim3(64 * kRansacWavesPerBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.n_inl, n_inl); b.get(b.Rt, Rt); b.get(b.mask, mask);
  return CCM_OK;
}
