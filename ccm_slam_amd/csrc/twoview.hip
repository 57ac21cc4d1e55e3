// twoview.hip — the arithmetic of cslam::Initializer (cslam/src/Initializer.cpp) on the device: ccm_twoview_ransac_eval (the 2 x H eight-point models of
// FindHomography / FindFundamental, :120-219, each scored against every match) and ccm_twoview_check_rt (every inlier under up to 8 motion hypotheses, :794-903).
//
// Layout.  RANSAC: the matches as xy1 / xy2 (mvKeysUn in match order) and pn1 / pn2 (the same points normalised), T1, T2inv, T2t, H sets of
// eight match indices.  Two launches.  The solve kernel has one lane per (hypothesis, model): blockIdx.y is the model, so a wave runs one SVD chain, not both;
// it writes H21 / H12 / F21.  The score kernel has the same mapping; a lane walks the matches in order (the order of the f32 sum is the contract), all lanes of
// a wave read the same match, and a lane writes an inlier word every 32 matches.  CheckRT: one lane per (hypothesis, match), blockIdx.y the hypothesis.
// 64 lanes per workgroup, plain loads and stores, no atomics, no waiting across workgroups; every loop is bounded by a constant or by N.
#include "common.h"
#include "twoview_math.h"
#include "stage_blocks.h"

namespace {

constexpr int kTvBlock = 64;

struct TvRansacArgs {
  int N, H, words;
  const float* xy1; const float* xy2; const float* pn1; const float* pn2;
  const float* T;         // T1, T2inv, T2t
  const int32_t* sets;    // [8 H]
  float sigma;
  float* H12;             // [9 H]
  float* scoreH; float* scoreF; float* H21; float* F21;
  uint32_t* maskH; uint32_t* maskF;   // [words H] each
};

__global__ __launch_bounds__(kTvBlock) void twoview_solve_kernel(TvRansacArgs a) {
  const int h = blockIdx.x * kTvBlock + threadIdx.x;
  if (h >= a.H) return;
  float p1[16], p2[16];
  for (int j = 0; j < 8; j++) {
    const int idx = a.sets[8 * h + j];
    p1[2 * j] = a.pn1[2 * idx]; p1[2 * j + 1] = a.pn1[2 * idx + 1];
    p2[2 * j] = a.pn2[2 * idx]; p2[2 * j + 1] = a.pn2[2 * idx + 1];
  }
  float M[9], Mi[9];
  if (blockIdx.y == 0) {
    tv_model_h(p1, p2, a.T, a.T + 9, M, Mi);
    for (int k = 0; k < 9; k++) { a.H21[9 * (size_t)h + k] = M[k]; a.H12[9 * (size_t)h + k] = Mi[k]; }
  } else {
    tv_model_f(p1, p2, a.T, a.T + 18, M);
    for (int k = 0; k < 9; k++) a.F21[9 * (size_t)h + k] = M[k];
  }
}

__global__ __launch_bounds__(kTvBlock) void twoview_score_kernel(TvRansacArgs a) {
  const int h = blockIdx.x * kTvBlock + threadIdx.x;
  if (h >= a.H) return;
  const bool hom = blockIdx.y == 0;
  float M[9], Mi[9];
  for (int k = 0; k < 9; k++) {
    M[k] = hom ? a.H21[9 * (size_t)h + k] : a.F21[9 * (size_t)h + k];
    Mi[k] = hom ? a.H12[9 * (size_t)h + k] : 0.f;
  }
  uint32_t* mask = (hom ? a.maskH : a.maskF) + (size_t)h * a.words;
  const float score = tv_score(hom, M, Mi, a.N, a.xy1, a.xy2, a.sigma, mask);
  (hom ? a.scoreH : a.scoreF)[h] = score;
}

struct TvCheckRtArgs {
  int N;
  const float* xy1; const float* xy2;
  const float* rec;       // [27 Q]
  const float* K;         // [9]
  const uint32_t* inl;    // [ceil(N / 32)]
  float th2;
  float* x3d;             // [Q N 3]
  float* cosp;            // [Q N]
  uint8_t* status;        // [Q N]
};

__global__ __launch_bounds__(kTvBlock) void twoview_check_rt_kernel(TvCheckRtArgs a) {
  const int i = blockIdx.x * kTvBlock + threadIdx.x;
  if (i >= a.N) return;
  const size_t o = (size_t)blockIdx.y * a.N + i;
  float X[3] = {NAN, NAN, NAN}, cosp = NAN;
  int st = TV_NOT_INLIER;
  if ((a.inl[i >> 5] >> (i & 31)) & 1u) {
    TvMotion m;
    const float* r = a.rec + TV_REC_FLOATS * (size_t)blockIdx.y;
    for (int k = 0; k < 12; k++) m.P2[k] = r[k];
    for (int k = 0; k < 3; k++) { m.O2[k] = r[12 + k]; m.t[k] = r[24 + k]; }
    for (int k = 0; k < 9; k++) m.R[k] = r[15 + k];
    float K[9];
    for (int k = 0; k < 9; k++) K[k] = a.K[k];
    st = tv_check_rt(K, m, a.xy1[2 * i], a.xy1[2 * i + 1], a.xy2[2 * i], a.xy2[2 * i + 1], a.th2, X, cosp);
  }
  a.x3d[3 * o] = X[0]; a.x3d[3 * o + 1] = X[1]; a.x3d[3 * o + 2] = X[2];
  a.cosp[o] = cosp;
  a.status[o] = (uint8_t)st;
}

}  // namespace

extern "C" int ccm_twoview_ransac_eval(ccm_ctx* ctx, int N, const float* xy1, const float* xy2, const float* pn1, const float* pn2, const float* T1,
                                       const float* T2inv, const float* T2t, float sigma, int H, const int32_t* sets, float* scoreH, float* scoreF,
                                       float* H21, float* F21, uint32_t* maskH, uint32_t* maskF) {
  if (!ctx) return CCM_E_ARG;
  if (N < 8 || H < 1 || !xy1 || !xy2 || !pn1 || !pn2 || !T1 || !T2inv || !T2t || !sets || !scoreH || !scoreF || !H21 || !F21 || !maskH || !maskF)
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_twoview_ransac_eval: bad args");
  if ((size_t)H * (((size_t)N + 31) / 32) > (size_t)INT32_MAX) return ccm_set_error(ctx, CCM_E_ARG, "ccm_twoview_ransac_eval: masks too large");
  for (int h = 0; h < H; h++)
    for (int j = 0; j < 8; j++) {
      const int32_t idx = sets[8 * (size_t)h + j];
      if (idx < 0 || idx >= N) return ccm_set_error(ctx, CCM_E_ARG, "ccm_twoview_ransac_eval: a set index outside [0, N)");
      for (int k = 0; k < j; k++)
        if (sets[8 * (size_t)h + k] == idx) return ccm_set_error(ctx, CCM_E_ARG, "ccm_twoview_ransac_eval: an index repeated within a set");
    }
  TwoViewRansacBlock b((size_t)N, (size_t)H);
  if (int rc = ccm_staged_begin(ctx, b, "ccm_twoview_ransac_eval: ")) return rc;
  b.put(b.xy1, xy1); b.put(b.xy2, xy2); b.put(b.pn1, pn1); b.put(b.pn2, pn2); b.put(b.sets, sets);
  float* hT = b.up(b.T);
  memcpy(hT, T1, 9 * sizeof(float)); memcpy(hT + 9, T2inv, 9 * sizeof(float)); memcpy(hT + 18, T2t, 9 * sizeof(float));
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  TvRansacArgs a;
  a.N = N; a.H = H; a.words = (int)b.words;
  a.xy1 = b.dev(b.xy1); a.xy2 = b.dev(b.xy2); a.pn1 = b.dev(b.pn1); a.pn2 = b.dev(b.pn2); a.T = b.dev(b.T); a.sets = b.dev(b.sets);
  a.sigma = sigma;
  a.H12 = b.dev(b.H12);
  a.scoreH = b.dev(b.scoreH); a.scoreF = b.dev(b.scoreF); a.H21 = b.dev(b.H21); a.F21 = b.dev(b.F21);
  a.maskH = b.dev(b.maskH); a.maskF = b.dev(b.maskF);
  const dim3 grid((unsigned)((H + kTvBlock - 1) / kTvBlock), 2);
  hipLaunchKernelGGL(twoview_solve_kernel, grid, dim3(kTvBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(twoview_score_kernel, grid, dim3(kTvBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.scoreH, scoreH); b.get(b.scoreF, scoreF); b.get(b.H21, H21); b.get(b.F21, F21); b.get(b.maskH, maskH); b.get(b.maskF, maskF);
  return CCM_OK;
}

extern "C" int ccm_twoview_check_rt(ccm_ctx* ctx, int n_hyp, const float* rec, const float* K, int N, const float* xy1, const float* xy2,
                                    const uint32_t* inlier_mask, float th2, uint8_t* status, float* x3d, float* cos_parallax) {
  if (!ctx) return CCM_E_ARG;
  if (n_hyp < 1 || n_hyp > 8 || N < 1 || !rec || !K || !xy1 || !xy2 || !inlier_mask || !status || !x3d || !cos_parallax)
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_twoview_check_rt: bad args");
  TwoViewCheckRtBlock b((size_t)N, (size_t)n_hyp);
  if (int rc = ccm_staged_begin(ctx, b, "ccm_twoview_check_rt: ")) return rc;
  b.put(b.xy1, xy1); b.put(b.xy2, xy2); b.put(b.rec, rec); b.put(b.K, K); b.put(b.inl, inlier_mask);
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  TvCheckRtArgs a;
  a.N = N;
  a.xy1 = b.dev(b.xy1); a.xy2 = b.dev(b.xy2); a.rec = b.dev(b.rec); a.K = b.dev(b.K); a.inl = b.dev(b.inl);
  a.th2 = th2;
  a.x3d = b.dev(b.x3d); a.cosp = b.dev(b.cosp); a.status = b.dev(b.status);
  hipLaunchKernelGGL(twoview_check_rt_kernel, dim3((unsigned)((N + kTvBlock - 1) / kTvBlock), (unsigned)n_hyp), dim3(kTvBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.x3d, x3d); b.get(b.cosp, cos_parallax); b.get(b.status, status);
  return CCM_OK;
}
