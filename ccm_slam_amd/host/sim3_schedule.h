// sim3_schedule.h — the RANSAC state of cslam::Sim3Solver (cslam/src/Sim3Solver.cpp:94-197) and the round-robin of LoopFinder::ComputeSim3
// (cslam/src/LoopFinder.cpp:288-346; MapMatcher::ComputeSim3 has the same loop), evaluated in passes of many hypotheses.  Header-only and
// templated on the evaluator, so that the host mirror (ccm_host.cpp, device evaluator ccm_sim3_ransac_eval) and the test driver
// (tests/host/sim3_schedule_check.cpp, CPU evaluator) run the same lines.  The draws and the pass are ransac_schedule.h's; what is here is the
// enumeration of the round-robin and the replay of the reference's loop.
//
// Why speculation is exact: the reference draws exactly three values per hypothesis (DUtils::Random::RandomInt(0, size-1) with size = N, N-1,
// N-2, swap-with-back removal from the identity mvAllIndices) and the only data-dependent event is a success (mnInliersi >= mnBestInliers &&
// mnInliersi > mRansacMinInliers, :167-182).  A pass therefore enumerates the remaining schedule as if no success came, takes three raw draws
// per hypothesis (first from the calling thread's FIFO, then from the source), evaluates all of it in one call, and replays the reference's
// loop in schedule order up to the first success.  The raw draws of every hypothesis after that success go back to the FRONT of the FIFO, in
// order: the next pass (or the next Sim3Solver of this thread) uses exactly the values the sequential reference would have drawn next.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>
#include "ransac_schedule.h"

namespace ccm_sim3 {

// the draw helpers both RANSAC schedules of a thread share (ransac_schedule.h)
using ccm_ransac::DrawSource;
using ccm_ransac::DrawsExhausted;
using ccm_ransac::draw_fifo;
using ccm_ransac::fifo_restore;
using ccm_ransac::rand_source;
using ccm_ransac::random_int;
inline void draws_to_indices(const int* raw, int N, int* idx) { ccm_ransac::draws_to_indices<3>(raw, N, idx); }

struct Params {
  double probability = 0.99;   // SetRansacParameters defaults (Sim3Solver.h), the values conf/config.yaml gives LoopFinder / MapMatcher
  int min_inliers = 6;
  int max_iterations = 300;
  int solver_iterations = 5;   // params::opt::mSolverIterations: hypotheses per iterate() call of the round-robin
};

// SetRansacParameters (:94-118): mRansacMaxIts.  (A candidate with N < minInliers never draws: iterate() returns bNoMore first.)
inline int ransac_max_iterations(int N, double probability, int min_inliers, int max_iterations) {
  if (N < min_inliers || N <= 0) return 1;
  const float epsilon = (float)min_inliers / N;
  int n_it;
  if (min_inliers == N)
    n_it = 1;
  else
    n_it = (int)std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
  return std::max(1, std::min(n_it, max_iterations));
}

struct Event {
  int cand = -1;
  int n_inliers = 0;
  float R[9], t[3], s;
  std::vector<uint32_t> mask;   // candidate-local inlier bits (bit i % 32 of word i / 32)
};

typedef ccm_ransac::Pass<3, float> Pass;   // the model: rts, 13 per hypothesis

// hypothesis h of a pass as an event of candidate c
inline void set_event(const Pass& p, int h, int c, Event& ev) {
  ev.cand = c; ev.n_inliers = p.n_inl[h];
  const float* o = &p.model[13 * (size_t)h];
  for (int i = 0; i < 9; i++) ev.R[i] = o[i];
  for (int i = 0; i < 3; i++) ev.t[i] = o[9 + i];
  ev.s = o[12];
  p.copy_mask(h, ev.mask);
}

// evaluator: ransac_schedule.h's, with rts (13 per hypothesis) as the model
template <class Eval>
class Schedule : private Pass {
 public:
  Schedule(const std::vector<int>& N, const Params& p, DrawSource src) : N_(N), p_(p), src_(std::move(src)) {
    const int K = (int)N_.size();
    max_its_.resize(K); n_its_.assign(K, 0); best_.assign(K, 0); discarded_.assign(K, 0);
    for (int c = 0; c < K; c++) {
      if (N_[c] < p_.min_inliers) continue;
      if (N_[c] < 3) throw std::invalid_argument("Sim3 RANSAC: a candidate with fewer than 3 correspondences and minInliers <= N");
      max_its_[c] = ransac_max_iterations(N_[c], p_.probability, p_.min_inliers, p_.max_iterations);
    }
  }

  // the next success event in the reference's order; false when every candidate is discarded.  Throws DrawsExhausted when a supplied
  // draw array runs out before the reference would stop; if the evaluator throws, the pass's draws are back in the FIFO and the state is unchanged.
  bool next(Eval& eval, Event& ev) {
    const int K = (int)N_.size();
    for (;;) {
      bool live = false;
      for (int c = 0; c < K; c++) live |= !discarded_[c];
      if (!live) return false;
      // 1. enumerate the rest of the schedule as if no success came: calls (candidate, hypotheses) in round-robin order from pos_
      std::vector<int> call_cand, call_n;
      {
        std::vector<int> its = n_its_;
        std::vector<char> disc = discarded_;
        int left = 0;
        for (int c = 0; c < K; c++) left += !disc[c];
        for (int c = pos_; left > 0; c = (c + 1) % K) {
          if (disc[c]) continue;
          int k = 0;
          if (N_[c] >= p_.min_inliers) k = std::max(0, std::min(p_.solver_iterations, max_its_[c] - its[c]));
          call_cand.push_back(c); call_n.push_back(k);
          its[c] += k;
          if (N_[c] < p_.min_inliers || its[c] >= max_its_[c]) { disc[c] = 1; left--; }
        }
      }
      // 2. three raw draws per hypothesis, FIFO first; a supplied array may run out (the pass is then cut there), and one evaluation
      take(call_cand, call_n, [&](int c) { return N_[c]; }, src_);
      const int H = evaluate(eval);
      // 3. the reference's loop over those calls, up to the first success
      int hp = 0;
      for (size_t j = 0; j < call_cand.size(); j++) {
        const int c = call_cand[j];
        if (N_[c] < p_.min_inliers) { discarded_[c] = 1; continue; }   // iterate(): N < mRansacMinInliers -> bNoMore, no draw
        int cur = 0;
        while (n_its_[c] < max_its_[c] && cur < p_.solver_iterations) {
          if (hp >= H) throw DrawsExhausted();
          cur++; n_its_[c]++;
          const int n = n_inl[hp];
          const int h = hp++;
          if (n >= best_[c]) {   // the best estimate moves on >=, with or without a success
            best_[c] = n;
            if (n > p_.min_inliers) {
              restore_after(hp);
              set_event(*this, h, c, ev);
              pos_ = (c + 1) % K;   // the for loop of ComputeSim3 goes on with the next candidate
              return true;
            }
          }
        }
        if (n_its_[c] >= max_its_[c]) discarded_[c] = 1;   // bNoMore
      }
      pos_ = 0;
    }
  }

  using Pass::source_draws;
  using Pass::hyps_evaluated;
  using Pass::passes;
  int iterations(int c) const { return n_its_[c]; }
  int max_iterations(int c) const { return max_its_[c]; }

 private:
  std::vector<int> N_;
  Params p_;
  DrawSource src_;
  std::vector<int> max_its_, n_its_, best_;
  std::vector<char> discarded_;
  int pos_ = 0;
};

// One Sim3Solver::iterate(nIterations) call (Sim3Solver.cpp:120-191) on a single candidate: its at most nIterations hypotheses in one evaluation,
// draws from the thread's FIFO first, the values of hypotheses after a success given back to it.  st.its / st.best = mnIterations /
// mnBestInliers (in / out).  Returns true on a success; no_more = bNoMore; best_updated: a hypothesis moved the best estimate (>=), which is
// then in `best` (the last such hypothesis).
struct SolverState { int N = 0, max_its = 1, min_inliers = 6, its = 0, best = 0; };
template <class Eval>
bool iterate_one(Eval& eval, SolverState& st, int n_iterations, const DrawSource& src, bool& no_more, bool& best_updated, Event& best) {
  no_more = false; best_updated = false;
  if (st.N < st.min_inliers) { no_more = true; return false; }
  const int k = std::max(0, std::min(n_iterations, st.max_its - st.its));
  Pass p;
  if (!p.take(std::vector<int>(1, 0), std::vector<int>(1, k), [&](int) { return st.N; }, src)) {
    p.restore_after(0);   // nothing is evaluated: every value taken goes back, in order
    throw DrawsExhausted();
  }
  p.evaluate(eval);
  for (int h = 0; h < k; h++) {
    st.its++;
    const int n = p.n_inl[h];
    if (n >= st.best) {
      st.best = n;
      best_updated = true;
      set_event(p, h, 0, best);
      if (n > st.min_inliers) {
        p.restore_after(h + 1);
        return true;
      }
    }
  }
  if (st.its >= st.max_its) no_more = true;
  return false;
}

}  // namespace ccm_sim3
