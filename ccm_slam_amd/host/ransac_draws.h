// ransac_draws.h — the raw random draws of the RANSAC schedules (sim3_schedule.h, pnp_schedule.h).  Sim3Solver and PnPsolver both consume ::rand() through
// DUtils::Random::RandomInt, so the schedules of one thread share ONE FIFO of values that were drawn for speculated hypotheses and not used: whichever solver draws
// next takes them first, in order, exactly as the sequential reference would have drawn them.
#pragma once
#include <cstdlib>
#include <deque>
#include <functional>
#include <stdexcept>

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
  DrawsExhausted() : std::runtime_error("Sim3 RANSAC: the supplied draws ran out") {}
};

// put values back at the front of the thread's FIFO so that it then starts with v[0], v[1], ...
inline void fifo_restore(const int* v, size_t n) {
  std::deque<int>& fifo = draw_fifo();
  for (size_t w = n; w-- > 0;) fifo.push_front(v[w]);
}

}  // namespace ccm_ransac
