// pnp.hip — the RANSAC hypotheses of cslam::PnPsolver (cslam/src/PnPSolver.cpp) on the device: ccm_pnp_ransac_eval.
//
// Layout: K candidates in CSR over pt_off, per point mvP3Dw (f32 x 3), mvP2D (f32 x 2) and mvMaxError (f32), per candidate fu fv uc vc (f64).
// H hypotheses, each a candidate and four distinct point indices (the host already mapped the random draws).  One wave64 per hypothesis, 4 waves per workgroup,
// as in sim3ransac.hip: lane 0 runs the serial EPnP compute_pose of pnp_math.h on its four correspondences and hands R and t to the wave through lane shuffles; the
// lanes then stride over the candidate's points and a ballot gives 64 inlier bits at a time (two mask words) and the count.  The solve's two large run-time
// indexed arrays (M, 8 x 12, and M' M / Ut, 12 x 12, f64) live in an LDS slice per wave: in private memory they would be scratch for all 64 lanes of a wave of
// which one works.  The Jacobi sweeps stay on one lane: every sum keeps the header's sequential order, so the device equals the host evaluator bit for bit.
#include "common.h"
#include "pnp_math.h"
#include "stage_blocks.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kWorkDoubles = 96 + 144;   // M (2 * 4 rows of 12), then M' M / Ut

struct PnpRansacArgs {
  int K, H;
  const double* cam;       // [K * 4]
  const int32_t* pt_off;   // [K + 1]
  const float* P3Dw;       // [Ntot * 3]
  const float* P2D;        // [Ntot * 2]
  const float* max_err;    // [Ntot]
  const int32_t* hyp_cand; // [H]
  const int32_t* hyp_idx;  // [H * 4], candidate-local
  const int32_t* mask_off; // [H + 1] words
  double* Rt;              // [H * 12]: R (9), t (3)
  int32_t* n_inl;          // [H]
  uint32_t* mask;          // [mask_off[H]]
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void pnp_ransac_kernel(PnpRansacArgs a) {
  __shared__ double s_work[kWavesPerBlock][kWorkDoubles];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int h = blockIdx.x * kWavesPerBlock + wave;
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
  if (pt_off[0] != 0) return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: pt_off[0] != 0");
  for (int c = 0; c < K; c++)
    if (pt_off[c + 1] - pt_off[c] < 4) return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: a candidate with fewer than 4 points");
  // words of each hypothesis' mask, and the index checks (every index < N of its candidate, four distinct)
  int64_t words = 0;
  mask_off[0] = 0;
  for (int h = 0; h < H; h++) {
    const int c = hyp_cand[h];
    if (c < 0 || c >= K) return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: hypothesis candidate out of range");
    const int N = pt_off[c + 1] - pt_off[c];
    const int32_t* ix = hyp_idx + 4 * (size_t)h;
    for (int j = 0; j < 4; j++) {
      if (ix[j] < 0 || ix[j] >= N) return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: point index out of range");
      for (int k = 0; k < j; k++)
        if (ix[k] == ix[j]) return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: repeated point index in a hypothesis");
    }
    words += (N + 31) >> 5;
    if (words > INT32_MAX) return ccm_set_error(ctx, CCM_E_ARG, "ccm_pnp_ransac_eval: mask too large");
    mask_off[h + 1] = (int32_t)words;
  }
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
  hipLaunchKernelGGL(pnp_ransac_kernel, dim3((H + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.n_inl, n_inl); b.get(b.Rt, Rt); b.get(b.mask, mask);
  return CCM_OK;
}
