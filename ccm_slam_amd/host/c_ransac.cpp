// c_ransac.cpp — C entry points of the two RANSAC batches, of the Sim3 solver's iterate, and pnp_math.h compiled for the host
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include "../csrc/pnp_math.h"
#include <cstring>
#include <memory>

using namespace ccmh_c;

namespace {
// a batch behind a C handle, with the supplied draws it reads (after the thread's FIFO) where the caller gave some
template <class Batch>
struct RansacBatchHandle {
  std::vector<int32_t> draws;
  size_t cursor = 0;
  std::unique_ptr<Batch> batch;
  ccm_ransac::DrawSource source(const int32_t* d, int64_t n) {   // d == NULL: ::rand()
    if (!d) return ccm_ransac::rand_source();
    draws.assign(d, d + n);
    return [this](int& v) { if (cursor >= draws.size()) return false; v = draws[cursor++]; return true; };
  }
};
typedef RansacBatchHandle<cslam::Sim3RansacBatch> Sim3BatchHandle;
typedef RansacBatchHandle<cslam::PnPRansacBatch> PnpBatchHandle;

int pnp_pose_out(const cslam::PnPRansacBatch::Pose& p, int32_t* cand, float* Tcw16, uint8_t* inliers, int cap, int32_t* n_inliers, int32_t* flags2) {
  if (cand) *cand = p.cand;
  if (Tcw16) std::memcpy(Tcw16, p.Tcw, sizeof p.Tcw);
  if (n_inliers) *n_inliers = p.nInliers;
  if (flags2) { flags2[0] = p.refined; flags2[1] = p.bNoMore; }
  if (inliers) for (int i = 0; i < cap && i < (int)p.vbInliers.size(); i++) inliers[i] = p.vbInliers[i] ? 1 : 0;
  return 1;
}
}  // namespace

extern "C" {
// Sim3RansacBatch over flat arrays: candidate c has the correspondences pt_off[c] .. pt_off[c+1] (X3Dc1 / X3Dc2 3 per correspondence, thresholds,
// idx1 = mvnIndices1) and n1[c] = mN1, K1 / K2 4 per candidate.  draws != NULL: the raw rand() values come from draws[0 .. n_draws) (after the
// thread's FIFO) instead of ::rand().
void* ccmh_sim3_ransac_create(int device, int K, const int32_t* pt_off, const float* X3Dc1, const float* X3Dc2, const float* K1, const float* K2,
                              const uint32_t* max_err1, const uint32_t* max_err2, const int32_t* n1, const int32_t* idx1, double probability,
                              int min_inliers, int max_iterations, int solver_iterations, int fix_scale, const int32_t* draws, int64_t n_draws) {
  return guard_ptr([&]() -> void* {
    if (K < 0 || !pt_off || (K > 0 && (!n1 || !K1 || !K2)) || (draws == nullptr && n_draws != 0) || n_draws < 0 || solver_iterations < 1) return nullptr;
    std::vector<cslam::Sim3Candidate> cands(K);
    for (int c = 0; c < K; c++) {
      const int a = pt_off[c], b = pt_off[c + 1];
      if (b < a) return nullptr;
      if (b > a && (!X3Dc1 || !X3Dc2 || !max_err1 || !max_err2 || !idx1)) return nullptr;
      auto& x = cands[c];
      x.n1 = n1[c];
      x.indices1.assign(idx1 + a, idx1 + b);
      x.X3Dc1.assign(X3Dc1 + 3 * (size_t)a, X3Dc1 + 3 * (size_t)b);
      x.X3Dc2.assign(X3Dc2 + 3 * (size_t)a, X3Dc2 + 3 * (size_t)b);
      x.max_err1.assign(max_err1 + a, max_err1 + b);
      x.max_err2.assign(max_err2 + a, max_err2 + b);
      for (int k = 0; k < 4; k++) { x.K1[k] = K1[4 * c + k]; x.K2[k] = K2[4 * c + k]; }
    }
    ccm_sim3::Params p;
    p.probability = probability; p.min_inliers = min_inliers; p.max_iterations = max_iterations; p.solver_iterations = solver_iterations;
    std::unique_ptr<Sim3BatchHandle> h(new Sim3BatchHandle);
    h->batch.reset(new cslam::Sim3RansacBatch(thread_context(device), std::move(cands), p, fix_scale != 0, h->source(draws, n_draws)));
    return h.release();
  });
}
// 1: an event (inliers[0 .. min(cap, mN1)) = vbInliers), 0: every candidate discarded, -1: the supplied draws ran out, -1000: device error
int ccmh_sim3_ransac_next(void* hv, int32_t* cand, float* R9, float* t3, float* s, uint8_t* inliers, int cap, int32_t* n_inliers) {
  if (!hv) return -1000;
  return guard_int([&]() -> int {
    Sim3BatchHandle* h = as<Sim3BatchHandle>(hv);
    int c = -1, n = 0; float sc = 0; std::vector<bool> vb;
    float R[9], t[3];
    try {
      if (!h->batch->next(c, R, t, sc, vb, n)) return 0;
    } catch (const ccm_sim3::DrawsExhausted&) {
      return -1;
    }
    if (cand) *cand = c;
    if (R9) std::memcpy(R9, R, sizeof R);
    if (t3) std::memcpy(t3, t, sizeof t);
    if (s) *s = sc;
    if (n_inliers) *n_inliers = n;
    if (inliers) for (int i = 0; i < cap && i < (int)vb.size(); i++) inliers[i] = vb[i] ? 1 : 0;
    return 1;
  });
}
// [values taken from the draw source, hypotheses evaluated, passes (device calls)]
int ccmh_sim3_ransac_stats(void* hv, int64_t* out3) {
  if (!hv || !out3) return -1000;
  const auto& sc = as<Sim3BatchHandle>(hv)->batch->schedule();
  out3[0] = sc.source_draws(); out3[1] = sc.hyps_evaluated(); out3[2] = sc.passes();
  return 0;
}
void ccmh_sim3_ransac_destroy(void* hv) { delete as<Sim3BatchHandle>(hv); }
// One Sim3Solver::iterate(n_iterations) of the drop-in shim/Sim3Solver_hip.cpp: N correspondences (X3Dc1 / X3Dc2, thresholds, cameras), state = [mnIterations,
// mnBestInliers] in / out, draws from ::rand() through the calling thread's FIFO.  flags = [success, bNoMore, best moved, inliers of the best]; when the best
// moved, best_rts = R (9) t (3) s and best_mask = its inlier bits (ceil(N / 32) words).  0, or -1000 on a device error.
int ccmh_sim3_solver_iterate(int device, int N, const float* X3Dc1, const float* X3Dc2, const float* K1, const float* K2, const uint32_t* max_err1,
                             const uint32_t* max_err2, int fix_scale, int min_inliers, int max_iterations, int n_iterations, int32_t* state,
                             float* best_rts, uint32_t* best_mask, int32_t* flags) {
  return guard_int([&]() -> int {
    if (N < 0 || !state || !flags || !best_rts || (N > 0 && (!X3Dc1 || !X3Dc2 || !K1 || !K2 || !max_err1 || !max_err2 || !best_mask))) return -1000;
    cslam::Sim3RansacBatch::Eval ev;
    ev.ctx = &thread_context(device);
    ev.fix_scale = fix_scale ? 1 : 0;
    ev.add(N, X3Dc1, X3Dc2, K1, K2, max_err1, max_err2);
    ccm_sim3::SolverState st;
    st.N = N; st.max_its = max_iterations; st.min_inliers = min_inliers; st.its = state[0]; st.best = state[1];
    bool no_more = false, moved = false;
    ccm_sim3::Event best;
    const bool ok = ccm_sim3::iterate_one(ev, st, n_iterations, ccm_sim3::rand_source(), no_more, moved, best);
    state[0] = st.its; state[1] = st.best;
    flags[0] = ok; flags[1] = no_more; flags[2] = moved; flags[3] = moved ? best.n_inliers : 0;
    if (moved) {
      for (int i = 0; i < 9; i++) best_rts[i] = best.R[i];
      for (int i = 0; i < 3; i++) best_rts[9 + i] = best.t[i];
      best_rts[12] = best.s;
      std::memcpy(best_mask, best.mask.data(), best.mask.size() * 4);
    }
    return 0;
  });
}

// PnPRansacBatch over flat arrays: candidate c has the correspondences pt_off[c] .. pt_off[c+1]
void* ccmh_pnp_ransac_create(int device, int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* sigma2, const double* cam,
                             const int32_t* n_matches, const int32_t* kp_idx, double probability, int min_inliers, int max_iterations, int min_set,
                             float epsilon, float th2, int solver_iterations, const int32_t* draws, int64_t n_draws) {
  return guard_ptr([&]() -> void* {
    if (K < 0 || !pt_off || (K > 0 && (!n_matches || !cam)) || (draws == nullptr && n_draws != 0) || n_draws < 0) return nullptr;
    std::vector<cslam::PnPCandidate> cands(K);
    for (int c = 0; c < K; c++) {
      const int a = pt_off[c], b = pt_off[c + 1];
      if (b < a) return nullptr;
      if (b > a && (!P3Dw || !P2D || !sigma2 || !kp_idx)) return nullptr;
      auto& x = cands[c];
      x.n_matches = n_matches[c];
      x.keypoint_indices.assign(kp_idx + a, kp_idx + b);
      x.P3Dw.assign(P3Dw + 3 * (size_t)a, P3Dw + 3 * (size_t)b);
      x.P2D.assign(P2D + 2 * (size_t)a, P2D + 2 * (size_t)b);
      x.sigma2.assign(sigma2 + a, sigma2 + b);
      for (int k = 0; k < 4; k++) x.cam[k] = cam[4 * c + k];
    }
    ccm_pnp::Params p;
    p.probability = probability; p.min_inliers = min_inliers; p.max_iterations = max_iterations; p.min_set = min_set; p.epsilon = epsilon; p.th2 = th2;
    p.solver_iterations = solver_iterations;
    std::unique_ptr<PnpBatchHandle> h(new PnpBatchHandle);
    h->batch.reset(new cslam::PnPRansacBatch(ctx_or_null(device), std::move(cands), p, h->source(draws, n_draws)));
    return h.release();
  });
}
int ccmh_pnp_ransac_next(void* hv, int32_t* cand, float* Tcw16, uint8_t* inliers, int cap, int32_t* n_inliers, int32_t* flags2) {
  if (!hv) return -1000;
  return guard_int([&]() -> int {
    cslam::PnPRansacBatch::Pose p;
    try {
      if (!as<PnpBatchHandle>(hv)->batch->next(p)) return 0;
    } catch (const ccm_pnp::DrawsExhausted&) {
      return -1;
    }
    return pnp_pose_out(p, cand, Tcw16, inliers, cap, n_inliers, flags2);
  });
}
int ccmh_pnp_ransac_iterate(void* hv, int c, int n_iterations, float* Tcw16, uint8_t* inliers, int cap, int32_t* n_inliers, int32_t* flags2) {
  if (!hv || !flags2) return -1000;
  return guard_int([&]() -> int {
    cslam::PnPRansacBatch::Pose p;
    bool no_more = false;
    bool got;
    try {
      got = as<PnpBatchHandle>(hv)->batch->iterate(c, n_iterations, no_more, p);
    } catch (const ccm_pnp::DrawsExhausted&) {
      return -1;
    }
    flags2[0] = 0; flags2[1] = no_more;
    if (!got) return 0;
    return pnp_pose_out(p, nullptr, Tcw16, inliers, cap, n_inliers, flags2);
  });
}
// [values taken from the draw source, hypotheses evaluated, passes (evaluator calls), Refine() computations]
int ccmh_pnp_ransac_stats(void* hv, int64_t* out4) {
  if (!hv || !out4) return -1000;
  const auto& sc = as<PnpBatchHandle>(hv)->batch->schedule();
  out4[0] = sc.source_draws(); out4[1] = sc.hyps_evaluated(); out4[2] = sc.passes(); out4[3] = sc.refines();
  return 0;
}
// [mnIterations, mRansacMaxIts, mRansacMinInliers, discarded] of candidate c
int ccmh_pnp_ransac_info(void* hv, int c, int32_t* out4) {
  if (!hv || !out4) return -1000;
  const auto& sc = as<PnpBatchHandle>(hv)->batch->schedule();
  if (c < 0 || c >= (int)sc.candidates().size()) return -1;
  out4[0] = sc.iterations(c); out4[1] = sc.max_iterations(c); out4[2] = sc.min_inliers(c); out4[3] = sc.discarded(c);
  return 0;
}
void ccmh_pnp_ransac_destroy(void* hv) { delete as<PnpBatchHandle>(hv); }
// the calling thread's FIFO of drawn, unused rand() values: returns its length, copies min(length, cap) values front first
int ccmh_sim3_draws_pending(int32_t* out, int cap) {
  const auto& q = ccm_sim3::draw_fifo();
  for (int i = 0; i < cap && i < (int)q.size(); i++) out[i] = q[i];
  return (int)q.size();
}
void ccmh_sim3_draws_clear(void) { ccm_sim3::draw_fifo().clear(); }

// pnp_math.h through C: the host evaluator of ccm_pnp_ransac_eval (its arguments without the context), compute_pose and Refine for any n, and the restated primitives
int ccmh_pnp_compute_pose(int n, const double* pws, const double* us, const double* cam4, double* R9, double* t3, double* rep_errors4, int32_t* chosen) {
  if (n < 4 || !pws || !us || !cam4 || !R9 || !t3) return -1;
  std::vector<double> alphas(4 * (size_t)n), pcs(3 * (size_t)n), M(24 * (size_t)n), ut(144);
  int N = 0;
  pnp_compute_pose(n, pws, us, cam4, alphas.data(), pcs.data(), M.data(), ut.data(), R9, t3, rep_errors4, &N);
  if (chosen) *chosen = N;
  return 0;
}
int ccmh_pnp_ransac_eval_host(int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* max_err, const double* cam, int H, const int32_t* hyp_cand,
                              const int32_t* hyp_idx, int32_t* n_inl, double* Rt, int32_t* mask_off, uint32_t* mask) {
  return ccm_pnp::eval_host(K, pt_off, P3Dw, P2D, max_err, cam, H, hyp_cand, hyp_idx, n_inl, Rt, mask_off, mask);
}
int ccmh_pnp_check_inliers(int N, const float* P3Dw, const float* P2D, const float* max_err, const double* cam4, const double* Rt12, uint8_t* inliers, float* error2) {
  if (N < 0 || !P3Dw || !P2D || !max_err || !cam4 || !Rt12) return -1;
  int count = 0;
  for (int i = 0; i < N; i++) {
    const float e = pnp_error2(Rt12, Rt12 + 9, cam4, P3Dw + 3 * (size_t)i, P2D + 2 * (size_t)i);
    const bool in = e < max_err[i];
    if (error2) error2[i] = e;
    if (inliers) inliers[i] = in;
    count += in;
  }
  return count;
}
int ccmh_pnp_refine(int N, const float* P3Dw, const float* P2D, const float* max_err, const double* cam4, const uint8_t* best_inliers, double* Rt12, uint8_t* inliers) {
  if (N < 4 || !P3Dw || !P2D || !max_err || !cam4 || !best_inliers || !Rt12) return -1;
  std::vector<uint32_t> best(((size_t)N + 31) / 32, 0u), got;
  int n = 0;
  for (int i = 0; i < N; i++)
    if (best_inliers[i]) { best[i >> 5] |= 1u << (i & 31); n++; }
  if (n < 4) return -1;
  const int count = ccm_pnp::refine_host(N, P3Dw, P2D, max_err, cam4, best, Rt12, got);
  if (inliers)
    for (int i = 0; i < N; i++) inliers[i] = got[i >> 5] >> (i & 31) & 1u;
  return count;
}
int ccmh_pnp_matrices(int n, const double* pws, const double* us, const double* cam4, double* mtm144, double* pca9, double* cc9) {
  if (n < 4 || !pws || !us || !cam4 || !mtm144 || !pca9 || !cc9) return -1;
  std::vector<double> alphas(4 * (size_t)n), M(24 * (size_t)n);
  double cws[4][3];
  pnp_build_mtm(n, pws, us, cam4, cws, alphas.data(), M.data(), mtm144, pca9, cc9);
  return 0;
}
int ccmh_pnp_primitive(int which, int rows, const double* A, const double* b, double* out) {
  if (!A || !out) return -1;
  switch (which) {
    case 0: { double a[9]; std::memcpy(a, A, sizeof a); pnp_svd_ut<3>(a, out); std::memcpy(out + 3, a, sizeof a); return 0; }
    case 1: { std::vector<double> a(A, A + 144); pnp_svd_ut<12>(a.data(), out); std::memcpy(out + 12, a.data(), 144 * sizeof(double)); return 0; }
    case 2: pnp_svd_uv3(A, out, out + 3, out + 12); return 0;
    case 3: pnp_invert3_svd(A, out); return 0;
    case 4: if (!b) return -1; pnp_solve_svd<3>(A, b, out); return 0;
    case 5: if (!b) return -1; pnp_solve_svd<4>(A, b, out); return 0;
    case 6: if (!b) return -1; pnp_solve_svd<5>(A, b, out); return 0;
    case 7: if (rows < 1) return -1; pnp_mul_transposed<3>(A, rows, out); return 0;
    case 8: if (rows < 1) return -1; pnp_mul_transposed<12>(A, rows, out); return 0;
    case 9: { if (!b) return -1; double a[24], bb[6]; std::memcpy(a, A, sizeof a); std::memcpy(bb, b, sizeof bb); return pnp_qr_solve(a, bb, out) ? 1 : 0; }
  }
  return -1;
}
}  // extern "C"
