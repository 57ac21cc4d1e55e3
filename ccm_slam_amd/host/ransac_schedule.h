// ransac_schedule.h — what the RANSAC schedules of a thread (sim3_schedule.h, pnp_schedule.h) share: the raw random draws and one pass of speculated hypotheses.
//
// The draws.  Sim3Solver and PnPsolver both consume ::rand() through DUtils::Random::RandomInt, so the schedules of one thread share ONE FIFO of values that were
// drawn for speculated hypotheses and not used: whichever solver draws next takes them first, in order, exactly as the sequential reference would have drawn them.
//
// The pass (Pass<S, Real>).  A schedule enumerates the calls (candidate, hypotheses) that the reference would make if no data-dependent event came; take() draws S
// raw values per hypothesis, FIFO first, then the source, and maps them to the sample's indices; evaluate() runs the evaluator on all of it, or puts the draws back
// if the evaluator throws; the schedule then replays the reference's loop over the results and, at its event, restore_after() gives the draws of every later
// hypothesis back to the FRONT of the FIFO, in order.  The replay loops, which are what differs, are in the two schedule headers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <functional>
#include <stdexcept>
#include <vector>

namespace ccm_ransac {

// DUtils::Random::RandomInt(0, d - 1) on one raw rand() value
inline int random_int(int raw, int d) { return int(((double)raw / ((double)RAND_MAX + 1.0)) * d) + 0; }

// the calling thread's FIFO of raw draws taken but not used (shared by every batch and drop-in solver of the thread)
inline std::deque<int>& draw_fifo() {
  thread_local std::deque<int> q;
  return q;
}

// a draw source: returns false when exhausted (a supplied array); the default is ::rand()
using DrawSource = std::function<bool(int&)>;
inline DrawSource rand_source() { return [](int& v) { v = ::rand(); return true; }; }

// a supplied draw array ran out before the reference would stop drawing
struct DrawsExhausted : std::runtime_error {
  DrawsExhausted() : std::runtime_error("RANSAC: the supplied draws ran out") {}
};

// put values back at the front of the thread's FIFO so that it then starts with v[0], v[1], ...
inline void fifo_restore(const int* v, size_t n) {
  std::deque<int>& fifo = draw_fifo();
  for (size_t w = n; w-- > 0;) fifo.push_front(v[w]);
}

// S raw draws -> the sample's indices: vAvailableIndices = identity of N, randi = RandomInt(0, size-1), idx = avail[randi], avail[randi] = avail.back(), pop_back
// (Sim3Solver.cpp:146-160, PnPSolver.cpp:178-192).  Only the at most S changed slots are kept.
template <int S>
inline void draws_to_indices(const int* raw, int N, int* idx) {
  int pos[S], val[S], nm = 0;
  auto get = [&](int p) { for (int j = nm - 1; j >= 0; j--) if (pos[j] == p) return val[j]; return p; };
  for (int j = 0; j < S; j++) {
    const int size = N - j;
    const int r = random_int(raw[j], size);
    idx[j] = get(r);
    const int back = get(size - 1);
    pos[nm] = r; val[nm] = back; nm++;
  }
}

// One pass of hypotheses with S draws each and a model of Real values, and the counters over a schedule's passes.
// evaluator: void(const std::vector<int32_t>& hyp_cand, const std::vector<int32_t>& hyp_idx /* S per hypothesis */, std::vector<int32_t>& n_inl,
//                 std::vector<Real>& model, std::vector<int32_t>& mask_off /* H + 1 */, std::vector<uint32_t>& mask)
template <int S, class Real>
struct Pass {
  std::vector<int> raws;   // S per hypothesis taken, in order
  std::vector<int32_t> hyp_cand, hyp_idx, n_inl, mask_off;
  std::vector<Real> model;
  std::vector<uint32_t> mask;   // candidate-local inlier bits (bit i % 32 of word i / 32) from mask_off[h]
  int64_t source_draws_ = 0, hyps_evaluated_ = 0;
  int passes_ = 0;
  int64_t source_draws() const { return source_draws_; }       // values taken from the draw source
  int64_t hyps_evaluated() const { return hyps_evaluated_; }
  int passes() const { return passes_; }                       // evaluator calls

  // the draws and samples of call_n[j] hypotheses of candidate call_cand[j] (n_points(c) correspondences), call after call.  A supplied array may run out: the
  // pass is then cut there (false), the complete hypotheses stay and the partial one's values are back at the front of the FIFO, in order.
  template <class NPoints>
  bool take(const std::vector<int>& call_cand, const std::vector<int>& call_n, NPoints n_points, const DrawSource& src) {
    std::deque<int>& fifo = draw_fifo();
    raws.clear(); hyp_cand.clear(); hyp_idx.clear();
    size_t total = 0;
    for (int n : call_n) total += (size_t)std::max(n, 0);
    // a hint only (the vectors grow past it): without it the three vectors regrow a dozen times per pass, a fifth of a 4 800-hypothesis pass's host time
    total = std::min(total, (size_t)1 << 16);
    raws.reserve(S * total); hyp_cand.reserve(total); hyp_idx.reserve(S * total);
    for (size_t j = 0; j < call_cand.size(); j++)
      for (int q = 0; q < call_n[j]; q++) {
        int r[S], idx[S];
        for (int u = 0; u < S; u++) {
          if (!fifo.empty()) { r[u] = fifo.front(); fifo.pop_front(); }
          else if (src(r[u])) { source_draws_++; }
          else { fifo_restore(r, (size_t)u); return false; }
        }
        raws.insert(raws.end(), r, r + S);
        draws_to_indices<S>(r, n_points(call_cand[j]), idx);
        hyp_cand.push_back(call_cand[j]);
        hyp_idx.insert(hyp_idx.end(), idx, idx + S);
      }
    return true;
  }

  // evaluate what take() left and return the number of hypotheses; if the evaluator throws, this pass's raw draws go back to the front of the FIFO first, so that
  // the thread's sequence is kept
  template <class Eval>
  int evaluate(Eval& eval) {
    const int H = (int)hyp_cand.size();
    if (H == 0) return 0;
    try {
      eval(hyp_cand, hyp_idx, n_inl, model, mask_off, mask);
    } catch (...) {
      restore_after(0);
      throw;
    }
    hyps_evaluated_ += H;
    passes_++;
    return H;
  }

  // the draws of every hypothesis from `hp` on go back to the front of the FIFO
  void restore_after(int hp) const { fifo_restore(raws.data() + S * (size_t)hp, raws.size() - S * (size_t)hp); }

  void copy_mask(int h, std::vector<uint32_t>& out) const { out.assign(mask.begin() + mask_off[h], mask.begin() + mask_off[h + 1]); }
};

}  // namespace ccm_ransac
