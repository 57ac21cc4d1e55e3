// sim3_schedule.h — the RANSAC state of cslam::Sim3Solver (cslam/src/Sim3Solver.cpp:94-197) and the round-robin of LoopFinder::ComputeSim3
// (cslam/src/LoopFinder.cpp:288-346; MapMatcher::ComputeSim3 has the same loop), evaluated in passes of many hypotheses.  Header-only and
// templated on the evaluator, so that the host mirror (ccm_host.cpp, device evaluator ccm_sim3_ransac_eval) and the test driver
// (tests/host/sim3_schedule_check.cpp, CPU evaluator) run the same lines.
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
#include <cstdlib>
#include <deque>
#include <functional>
#include <stdexcept>
#include <vector>
#include "ransac_draws.h"

namespace ccm_sim3 {

// the draw helpers both RANSAC schedules of a thread share (ransac_draws.h)
using ccm_ransac::DrawSource;
using ccm_ransac::DrawsExhausted;
using ccm_ransac::draw_fifo;
using ccm_ransac::fifo_restore;
using ccm_ransac::rand_source;
using ccm_ransac::random_int;

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

// three raw draws -> the sample's indices: vAvailableIndices = identity of N, randi = RandomInt(0, size-1), idx = avail[randi],
// avail[randi] = avail.back(), pop_back (:146-160).  Only the at most three changed slots are kept.
inline void draws_to_indices(const int raw[3], int N, int idx[3]) {
  int pos[3], val[3], nm = 0;
  auto get = [&](int p) { for (int j = nm - 1; j >= 0; j--) if (pos[j] == p) return val[j]; return p; };
  for (int j = 0; j < 3; j++) {
    const int size = N - j;
    const int r = random_int(raw[j], size);
    idx[j] = get(r);
    const int back = get(size - 1);
    pos[nm] = r; val[nm] = back; nm++;
  }
}

// evaluate; if the evaluator throws, this pass's raw draws go back to the front of the FIFO first, so that the thread's sequence is kept
template <class Eval>
void eval_or_restore(Eval& eval, const std::vector<int>& raws, const std::vector<int32_t>& hc, const std::vector<int32_t>& hi, std::vector<int32_t>& n_inl,
                     std::vector<float>& rts, std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask) {
  try {
    eval(hc, hi, n_inl, rts, mask_off, mask);
  } catch (...) {
    fifo_restore(raws.data(), raws.size());
    throw;
  }
}

struct Event {
  int cand = -1;
  int n_inliers = 0;
  float R[9], t[3], s;
  std::vector<uint32_t> mask;   // candidate-local inlier bits (bit i % 32 of word i / 32)
};

// evaluator: void(const std::vector<int32_t>& hyp_cand, const std::vector<int32_t>& hyp_idx, std::vector<int32_t>& n_inl,
//                 std::vector<float>& rts /* 13 per hypothesis */, std::vector<int32_t>& mask_off /* H + 1 */, std::vector<uint32_t>& mask)
template <class Eval>
class Schedule {
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
      // 2. three raw draws per hypothesis, FIFO first; a supplied array may run out (the pass is then cut there)
      std::deque<int>& fifo = draw_fifo();
      std::vector<int> raws;
      hyp_cand_.clear(); hyp_idx_.clear();
      bool cut = false;
      for (size_t j = 0; j < call_cand.size() && !cut; j++)
        for (int q = 0; q < call_n[j] && !cut; q++) {
          int r[3];
          for (int u = 0; u < 3; u++) {
            if (!fifo.empty()) { r[u] = fifo.front(); fifo.pop_front(); }
            else if (src_(r[u])) { source_draws_++; }
            else { cut = true; for (int w = u - 1; w >= 0; w--) fifo.push_front(r[w]); break; }
          }
          if (cut) break;
          raws.insert(raws.end(), r, r + 3);
          int idx[3];
          draws_to_indices(r, N_[call_cand[j]], idx);
          hyp_cand_.push_back(call_cand[j]);
          hyp_idx_.insert(hyp_idx_.end(), idx, idx + 3);
        }
      const int H = (int)hyp_cand_.size();
      if (H > 0) {
        eval_or_restore(eval, raws, hyp_cand_, hyp_idx_, n_inl_, rts_, mask_off_, mask_);
        hyps_evaluated_ += H;
        passes_++;
      }
      // 3. the reference's loop over those calls, up to the first success
      int hp = 0;
      for (size_t j = 0; j < call_cand.size(); j++) {
        const int c = call_cand[j];
        if (N_[c] < p_.min_inliers) { discarded_[c] = 1; continue; }   // iterate(): N < mRansacMinInliers -> bNoMore, no draw
        int cur = 0;
        while (n_its_[c] < max_its_[c] && cur < p_.solver_iterations) {
          if (hp >= H) throw DrawsExhausted();
          cur++; n_its_[c]++;
          const int n = n_inl_[hp];
          const int h = hp++;
          if (n >= best_[c]) {   // the best estimate moves on >=, with or without a success
            best_[c] = n;
            if (n > p_.min_inliers) {
              fifo_restore(raws.data() + 3 * (size_t)hp, raws.size() - 3 * (size_t)hp);
              ev.cand = c; ev.n_inliers = n;
              const float* o = &rts_[13 * (size_t)h];
              for (int i = 0; i < 9; i++) ev.R[i] = o[i];
              for (int i = 0; i < 3; i++) ev.t[i] = o[9 + i];
              ev.s = o[12];
              ev.mask.assign(mask_.begin() + mask_off_[h], mask_.begin() + mask_off_[h + 1]);
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

  int64_t source_draws() const { return source_draws_; }
  int64_t hyps_evaluated() const { return hyps_evaluated_; }
  int passes() const { return passes_; }
  int iterations(int c) const { return n_its_[c]; }
  int max_iterations(int c) const { return max_its_[c]; }

 private:
  std::vector<int> N_;
  Params p_;
  DrawSource src_;
  std::vector<int> max_its_, n_its_, best_;
  std::vector<char> discarded_;
  int pos_ = 0;
  int64_t source_draws_ = 0, hyps_evaluated_ = 0;
  int passes_ = 0;
  std::vector<int32_t> hyp_cand_, hyp_idx_, n_inl_, mask_off_;
  std::vector<float> rts_;
  std::vector<uint32_t> mask_;
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
  std::deque<int>& fifo = draw_fifo();
  std::vector<int> raws;
  std::vector<int32_t> hc, hi, n_inl, mask_off;
  std::vector<float> rts;
  std::vector<uint32_t> mask;
  for (int q = 0; q < k; q++) {
    int r[3];
    for (int u = 0; u < 3; u++) {
      if (!fifo.empty()) { r[u] = fifo.front(); fifo.pop_front(); continue; }
      if (src(r[u])) continue;
      raws.insert(raws.end(), r, r + u);   // nothing is evaluated: every value taken goes back, in order
      fifo_restore(raws.data(), raws.size());
      throw DrawsExhausted();
    }
    raws.insert(raws.end(), r, r + 3);
    int idx[3];
    draws_to_indices(r, st.N, idx);
    hc.push_back(0);
    hi.insert(hi.end(), idx, idx + 3);
  }
  if (k > 0) eval_or_restore(eval, raws, hc, hi, n_inl, rts, mask_off, mask);
  for (int h = 0; h < k; h++) {
    st.its++;
    const int n = n_inl[h];
    if (n >= st.best) {
      st.best = n;
      best_updated = true;
      best.cand = 0; best.n_inliers = n;
      for (int i = 0; i < 9; i++) best.R[i] = rts[13 * h + i];
      for (int i = 0; i < 3; i++) best.t[i] = rts[13 * h + 9 + i];
      best.s = rts[13 * h + 12];
      best.mask.assign(mask.begin() + mask_off[h], mask.begin() + mask_off[h + 1]);
      if (n > st.min_inliers) {
        fifo_restore(raws.data() + 3 * (size_t)(h + 1), raws.size() - 3 * (size_t)(h + 1));
        return true;
      }
    }
  }
  if (st.its >= st.max_its) no_more = true;
  return false;
}

}  // namespace ccm_sim3
