// sim3ransac.hip — the RANSAC hypotheses of cslam::Sim3Solver (cslam/src/Sim3Solver.cpp) on the device: ccm_sim3_ransac_eval.
//
// Layout: K candidates in CSR over pt_off, per point mvX3Dc1 / mvX3Dc2 (f32 x 3) and the integer thresholds mvnMaxError1/2,
// per candidate K1 / K2 (fx fy cx cy).  H hypotheses, each a candidate and three distinct point indices (the host already mapped the random
// draws).  One wave64 per hypothesis, 4 waves per workgroup: lane 0 runs the serial three-point solve (centroids, Horn's 4x4 matrix, Jacobi,
// Rodrigues, scale, translation) of sim3_ransac_math.h and hands the two transforms to the wave through lane shuffles; the lanes then stride
// over the candidate's points, each point projected both ways, and a ballot gives 64 inlier bits at a time (two mask words) and the count.
// Points are read from global memory: a candidate holds a few thousand points at most, which the hypotheses of one launch share through L2.
#include "common.h"
#include "sim3_ransac_math.h"
#include "stage_blocks.h"

namespace {

constexpr int kWavesPerBlock = 4;

struct Sim3RansacArgs {
  int K, H, fix_scale;
  const int32_t* pt_off;   // [K + 1]
  const float* X1;         // [Ntot * 3]
  const float* X2;
  const float* K1;         // [K * 4]
  const float* K2;
  const uint32_t* thr1;    // [Ntot]
  const uint32_t* thr2;
  const int32_t* hyp_cand; // [H]
  const int32_t* hyp_idx;  // [H * 3], candidate-local
  const int32_t* mask_off; // [H + 1] words
  int32_t* n_inl;          // [H]
  float* rts;              // [H * 13]: R (9), t (3), s
  uint32_t* mask;          // [mask_off[H]]
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void sim3_ransac_kernel(Sim3RansacArgs a) {
  const int lane = threadIdx.x & 63;
  const int h = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (h >= a.H) return;   // whole waves only: no barrier below
  const int c = a.hyp_cand[h];
  const int p0 = a.pt_off[c], N = a.pt_off[c + 1] - p0;
  S3Hyp hy = {};   // lanes 1..63 take lane 0's transforms through the shuffles below
  if (lane == 0) {
    float x1[3][3], x2[3][3];
    for (int j = 0; j < 3; j++) {
      const int i = p0 + a.hyp_idx[3 * h + j];
      for (int r = 0; r < 3; r++) { x1[j][r] = a.X1[3 * i + r]; x2[j][r] = a.X2[3 * i + r]; }
    }
    s3_compute_sim3(x1, x2, a.fix_scale != 0, hy);
    float* o = a.rts + 13 * (size_t)h;
    for (int i = 0; i < 9; i++) o[i] = hy.R[i];
    for (int i = 0; i < 3; i++) o[9 + i] = hy.t[i];
    o[12] = hy.s;
  }
  // broadcast the two transforms (sR | t, sRinv | tinv) from lane 0
  for (int i = 0; i < 9; i++) { hy.sR[i] = __shfl(hy.sR[i], 0); hy.sRi[i] = __shfl(hy.sRi[i], 0); }
  for (int i = 0; i < 3; i++) { hy.t[i] = __shfl(hy.t[i], 0); hy.ti[i] = __shfl(hy.ti[i], 0); }
  const float k1[4] = {a.K1[4 * c], a.K1[4 * c + 1], a.K1[4 * c + 2], a.K1[4 * c + 3]};
  const float k2[4] = {a.K2[4 * c], a.K2[4 * c + 1], a.K2[4 * c + 2], a.K2[4 * c + 3]};
  uint32_t* m = a.mask + a.mask_off[h];
  const int n_words = (N + 31) >> 5;
  int count = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < N) {
      const int g = p0 + i;
      in = s3_inlier(hy, a.X1 + 3 * (size_t)g, a.X2 + 3 * (size_t)g, k1, k2, a.thr1[g], a.thr2[g]);
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

extern "C" int ccm_sim3_ransac_eval(ccm_ctx* ctx, int K, const int32_t* pt_off, const float* X3Dc1, const float* X3Dc2, const float* K1,
                                    const float* K2, const uint32_t* max_err1, const uint32_t* max_err2, int H, const int32_t* hyp_cand,
                                    const int32_t* hyp_idx, int fix_scale, int32_t* n_inl, float* rts, int32_t* mask_off, uint32_t* mask) {
  if (!ctx) return CCM_E_ARG;
  if (K < 1 || H < 0 || !pt_off || !X3Dc1 || !X3Dc2 || !K1 || !K2 || !max_err1 || !max_err2 || !mask_off ||
      (H > 0 && (!hyp_cand || !hyp_idx || !n_inl || !rts || !mask)))
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: bad args");
  if (pt_off[0] != 0) return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: pt_off[0] != 0");
  for (int c = 0; c < K; c++)
    if (pt_off[c + 1] - pt_off[c] < 3) return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: a candidate with fewer than 3 points");
  // words of each hypothesis' mask, and the index checks (every index < N of its candidate, three distinct)
  int64_t words = 0;
  mask_off[0] = 0;
  for (int h = 0; h < H; h++) {
    const int c = hyp_cand[h];
    if (c < 0 || c >= K) return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: hypothesis candidate out of range");
    const int N = pt_off[c + 1] - pt_off[c];
    const int i0 = hyp_idx[3 * h], i1 = hyp_idx[3 * h + 1], i2 = hyp_idx[3 * h + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= N || i1 >= N || i2 >= N)
      return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: point index out of range");
    if (i0 == i1 || i0 == i2 || i1 == i2) return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: repeated point index in a hypothesis");
    words += (N + 31) >> 5;
    if (words > INT32_MAX) return ccm_set_error(ctx, CCM_E_ARG, "ccm_sim3_ransac_eval: mask too large");
    mask_off[h + 1] = (int32_t)words;
  }
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
  hipLaunchKernelGGL(sim3_ransac_kernel, dim3((H + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.n_inl, n_inl); b.get(b.rts, rts); b.get(b.mask, mask);
  return CCM_OK;
}
