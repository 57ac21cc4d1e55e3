// pnp_schedule.h — the RANSAC state of cslam::PnPsolver (cslam/src/PnPSolver.cpp: SetRansacParameters :111-147, iterate :155-249, Refine :251-296) and a round-robin
// of iterate(n) over the candidates of a relocalisation, evaluated in passes of many hypotheses.  Header-only and templated on the evaluator, so that the host mirror
// (ccm_host.cpp: device evaluator ccm_pnp_ransac_eval, or eval_host below) and the test driver (tests/host/pnp_check.cpp) run the same lines.  The draws and the
// pass are ransac_schedule.h's; what is here is the call lengths of the round-robin, Refine and the replay of the reference's iterate().
//
// iterate() is kept literally, with its quirks: the loop runs while `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`, so a call without a success
// runs max(nIterations, mRansacMaxIts - mnIterations) hypotheses and always ends with bNoMore; N < mRansacMinInliers gives bNoMore before any draw; Refine() runs after
// every hypothesis with mnInliersi >= mRansacMinInliers, works on mvbBestInliers (not on the current mask) and succeeds on >; mBestTcw / mRefinedTcw are the f32
// conversions of the f64 pose.
//
// Why speculation is exact: the reference draws exactly four values per hypothesis (DUtils::Random::RandomInt(0, size-1) with size = N, N-1, N-2, N-3, swap-with-back
// removal from the identity mvAllIndices) and the only data-dependent event is a successful Refine, which draws nothing.  A pass therefore enumerates the rest of the
// round-robin as if no Refine succeeded, takes four raw draws per hypothesis (first from the calling thread's FIFO, ransac_schedule.h, then from the source), evaluates
// all of it in one call, and replays the reference's loop in order up to the first call that returns a pose.  The raw draws of every hypothesis after it go back to
// the FRONT of the FIFO, in order: the next pass — or the next Sim3 or PnP solver of this thread — uses exactly the values the sequential reference would have drawn.
//
// Refine()'s EPnP has a variable n and runs here, on the host, through pnp_math.h.  Its result depends on mvbBestInliers alone, so it is computed once per change of
// the best mask and kept, failed or not.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "ransac_schedule.h"
#include "../csrc/pnp_math.h"
#include "../csrc/ransac_wave.h"

namespace ccm_pnp {

using ccm_ransac::DrawSource;
using ccm_ransac::DrawsExhausted;
using ccm_ransac::draw_fifo;
using ccm_ransac::fifo_restore;
using ccm_ransac::rand_source;
using ccm_ransac::random_int;

struct Params {   // SetRansacParameters' defaults (PnPSolver.h)
  double probability = 0.99;
  int min_inliers = 8;
  int max_iterations = 300;
  int min_set = 4;   // fixed: the device solves four correspondences
  float epsilon = 0.4f;
  float th2 = 5.991f;
  int solver_iterations = 5;   // nIterations of the round-robin's iterate() calls
};

// what the constructor (:57-100) gathers for one candidate, in the order of the frame's keypoints
struct Candidate {
  std::vector<float> P3Dw, P2D, sigma2;   // mvP3Dw (3 per correspondence), mvP2D (2), mvSigma2
  double cam[4] = {0, 0, 0, 0};           // fu fv uc vc
  int N() const { return (int)sigma2.size(); }
};

// SetRansacParameters (:111-147): the adjusted mRansacMinInliers and mRansacMaxIts
struct Ransac { int min_inliers = 0, max_its = 1; };
inline Ransac set_ransac_parameters(int N, const Params& p) {
  Ransac r;
  float epsilon = p.epsilon;
  int nMinInliers = (int)(N * epsilon);
  if (nMinInliers < p.min_inliers) nMinInliers = p.min_inliers;
  if (nMinInliers < p.min_set) nMinInliers = p.min_set;
  r.min_inliers = nMinInliers;
  if (N < r.min_inliers) return r;   // iterate() returns bNoMore before it reads mRansacMaxIts
  if (epsilon < (float)r.min_inliers / N) epsilon = (float)r.min_inliers / N;
  int nIterations;
  if (r.min_inliers == N)
    nIterations = 1;
  else {
    const double v = std::ceil(std::log(1 - p.probability) / std::log(1 - std::pow(epsilon, 3)));
    nIterations = v < (double)p.max_iterations ? (int)v : p.max_iterations;   // the reference converts v itself; beyond int that is undefined
  }
  r.max_its = std::max(1, std::min(nIterations, p.max_iterations));
  return r;
}

// the arguments of ccm_pnp_ransac_eval without the context, on the calling thread: its checks (ransac_wave.h), then PnpHypForm hypothesis after hypothesis.  0, or -1
// for its CCM_E_ARG cases.
inline int eval_host(int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* max_err, const double* cam, int H, const int32_t* hyp_cand,
                     const int32_t* hyp_idx, int32_t* n_inl, double* Rt, int32_t* mask_off, uint32_t* mask) {
  if (K < 1 || H < 0 || !pt_off || !P3Dw || !P2D || !max_err || !cam || !mask_off || (H > 0 && (!hyp_cand || !hyp_idx || !n_inl || !Rt || !mask))) return -1;
  int64_t words = 0;
  if (ransac_check_hyps<4>(K, pt_off, H, hyp_cand, hyp_idx, mask_off, &words, /*range_first=*/false)) return -1;
  ransac_eval_host<PnpHypForm>(PnpRansacArgs{K, H, cam, pt_off, P3Dw, P2D, max_err, hyp_cand, hyp_idx, mask_off, Rt, n_inl, mask});
  return 0;
}

// compute_pose on the correspondences of a mask (Refine :253-275) and CheckInliers (:278) over all N; returns mnInliersi
inline int refine_host(int N, const float* P3Dw, const float* P2D, const float* max_err, const double* cam, const std::vector<uint32_t>& best_mask, double Rt[12],
                       std::vector<uint32_t>& mask_out) {
  std::vector<double> pws, us;
  for (int i = 0; i < N; i++)
    if (best_mask[i >> 5] >> (i & 31) & 1u) {
      for (int r = 0; r < 3; r++) pws.push_back(P3Dw[3 * (size_t)i + r]);
      for (int r = 0; r < 2; r++) us.push_back(P2D[2 * (size_t)i + r]);
    }
  const int n = (int)(us.size() / 2);
  std::vector<double> alphas(4 * (size_t)n), pcs(3 * (size_t)n), M(24 * (size_t)n), ut(144);
  pnp_compute_pose(n, pws.data(), us.data(), cam, alphas.data(), pcs.data(), M.data(), ut.data(), Rt, Rt + 9, nullptr, nullptr);
  mask_out.assign(((size_t)N + 31) / 32, 0u);
  int count = 0;
  for (int i = 0; i < N; i++)
    if (pnp_inlier(Rt, Rt + 9, cam, P3Dw + 3 * (size_t)i, P2D + 2 * (size_t)i, max_err[i])) { mask_out[i >> 5] |= 1u << (i & 31); count++; }
  return count;
}

// Rcw.convertTo(CV_32F), tcw.convertTo(CV_32F) into eye(4, 4, CV_32F)
inline void to_tcw(const double Rt[12], float Tcw[16]) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw[4 * r + c] = (float)Rt[3 * r + c];
    Tcw[4 * r + 3] = (float)Rt[9 + r];
  }
  Tcw[12] = Tcw[13] = Tcw[14] = 0; Tcw[15] = 1;
}

// one iterate() call that returned a pose
struct Event {
  int cand = -1;
  int n_inliers = 0;
  bool refined = false;   // mRefinedTcw (a successful Refine) or mBestTcw (the iterations ran out with mnBestInliers >= mRansacMinInliers)
  bool no_more = false;   // bNoMore of that call
  float Tcw[16];
  std::vector<uint32_t> mask;   // candidate-local inlier bits (bit i % 32 of word i / 32): mvbRefinedInliers or mvbBestInliers
};

typedef ccm_ransac::Pass<4, double> Pass;   // the model: Rt, 12 per hypothesis

// evaluator: ransac_schedule.h's, with Rt (12 per hypothesis) as the model
template <class Eval>
class Schedule : private Pass {
 public:
  Schedule(std::vector<Candidate> cands, const Params& p, DrawSource src) : c_(std::move(cands)), p_(p), src_(std::move(src)) {
    if (p_.min_set != 4) throw std::invalid_argument("PnP RANSAC: min_set must be 4");
    if (p_.solver_iterations < 1) throw std::invalid_argument("PnP RANSAC: solver_iterations < 1");
    const int K = (int)c_.size();
    st_.resize(K);
    for (int c = 0; c < K; c++) {
      const Candidate& x = c_[c];
      if (x.P3Dw.size() != 3 * x.sigma2.size() || x.P2D.size() != 2 * x.sigma2.size()) throw std::invalid_argument("PnP RANSAC: inconsistent candidate sizes");
      State& s = st_[c];
      s.r = set_ransac_parameters(x.N(), p_);
      s.max_err.resize(x.sigma2.size());
      for (size_t i = 0; i < x.sigma2.size(); i++) s.max_err[i] = pnp_max_error(x.sigma2[i], p_.th2);
    }
  }

  const std::vector<Candidate>& candidates() const { return c_; }
  const std::vector<float>& max_err(int c) const { return st_[c].max_err; }

  // the round-robin `for each candidate not discarded: iterate(solver_iterations)`: the next call that returns a pose; false when every candidate is discarded.
  // Throws DrawsExhausted when a supplied draw array runs out before the reference would stop; if the evaluator throws, the pass's draws are back in the FIFO.
  bool next(Eval& eval, Event& ev) {
    const int K = (int)c_.size();
    for (;;) {
      // the rest of the round-robin as if no Refine succeeded: every call without one ends with bNoMore, so each live candidate is called once
      std::vector<int> call_cand, call_n;
      for (int q = 0; q < K; q++) {
        const int c = (pos_ + q) % K;
        if (st_[c].discarded) continue;
        call_cand.push_back(c);
        call_n.push_back(call_length(c, p_.solver_iterations));
      }
      if (call_cand.empty()) return false;
      bool no_more = false;
      if (run(eval, call_cand, call_n, p_.solver_iterations, ev, no_more)) return true;
      pos_ = 0;
    }
  }

  // one iterate(n_iterations) of candidate c, as the drop-in calls it: true when it returns a pose (ev), no_more = bNoMore
  bool iterate(Eval& eval, int c, int n_iterations, Event& ev, bool& no_more) {
    const std::vector<int> call_cand(1, c), call_n(1, call_length(c, n_iterations));
    return run(eval, call_cand, call_n, n_iterations, ev, no_more);
  }

  using Pass::source_draws;
  using Pass::hyps_evaluated;
  using Pass::passes;
  int64_t refines() const { return refines_; }
  int iterations(int c) const { return st_[c].its; }
  int max_iterations(int c) const { return st_[c].r.max_its; }
  int min_inliers(int c) const { return st_[c].r.min_inliers; }
  bool discarded(int c) const { return st_[c].discarded; }

 private:
  struct State {
    Ransac r;
    std::vector<float> max_err;   // mvMaxError
    int its = 0, best = 0;        // mnIterations, mnBestInliers
    bool discarded = false;       // the round-robin's flag: a call returned bNoMore
    std::vector<uint32_t> best_mask;
    float best_tcw[16];
    bool refine_known = false;    // Refine() of the current best mask
    int refined = 0;
    std::vector<uint32_t> refined_mask;
    float refined_tcw[16];
  };

  // hypotheses of an iterate(n) call in which no Refine succeeds
  int call_length(int c, int n) const {
    const State& s = st_[c];
    if (c_[c].N() < s.r.min_inliers) return 0;
    return std::max(n, s.r.max_its - s.its);
  }

  bool refine(int c) {
    State& s = st_[c];
    if (!s.refine_known) {
      double Rt[12];
      s.refined = refine_host(c_[c].N(), c_[c].P3Dw.data(), c_[c].P2D.data(), s.max_err.data(), c_[c].cam, s.best_mask, Rt, s.refined_mask);
      to_tcw(Rt, s.refined_tcw);
      s.refine_known = true;
      refines_++;
    }
    return s.refined > s.r.min_inliers;
  }

  bool run(Eval& eval, const std::vector<int>& call_cand, const std::vector<int>& call_n, int n_iterations, Event& ev, bool& no_more) {
    // four raw draws per hypothesis, FIFO first; a supplied array may run out (the pass is then cut there), and one evaluation
    take(call_cand, call_n, [&](int c) { return c_[c].N(); }, src_);
    const int H = evaluate(eval);
    // the reference's iterate(), call after call, up to the first one that returns a pose
    const int K = (int)c_.size();
    int hp = 0;
    for (size_t j = 0; j < call_cand.size(); j++) {
      const int c = call_cand[j];
      State& s = st_[c];
      no_more = false;
      if (c_[c].N() < s.r.min_inliers) { no_more = true; s.discarded = true; continue; }   // bNoMore before any draw, an empty Mat
      int cur = 0;
      while (s.its < s.r.max_its || cur < n_iterations) {
        if (hp >= H) throw DrawsExhausted();
        cur++; s.its++;
        const int h = hp++;
        const int n = n_inl[h];
        if (n >= s.r.min_inliers) {
          if (n > s.best) {
            copy_mask(h, s.best_mask);
            s.best = n;
            to_tcw(&model[12 * (size_t)h], s.best_tcw);
            s.refine_known = false;
          }
          if (refine(c)) {
            restore_after(hp);
            ev.cand = c; ev.n_inliers = s.refined; ev.refined = true; ev.no_more = false;
            std::copy(s.refined_tcw, s.refined_tcw + 16, ev.Tcw);
            ev.mask = s.refined_mask;
            pos_ = (c + 1) % K;
            return true;
          }
        }
      }
      no_more = true;   // mnIterations >= mRansacMaxIts holds whenever the loop ends
      s.discarded = true;
      if (s.best >= s.r.min_inliers) {
        restore_after(hp);
        ev.cand = c; ev.n_inliers = s.best; ev.refined = false; ev.no_more = true;
        std::copy(s.best_tcw, s.best_tcw + 16, ev.Tcw);
        ev.mask = s.best_mask;
        pos_ = (c + 1) % K;
        return true;
      }
    }
    return false;
  }

  std::vector<Candidate> c_;
  Params p_;
  DrawSource src_;
  std::vector<State> st_;
  int pos_ = 0;
  int64_t refines_ = 0;
};

}  // namespace ccm_pnp
