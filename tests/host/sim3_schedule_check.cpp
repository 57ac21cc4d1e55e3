// sim3_schedule_check.cpp — ccm_slam_amd/host/sim3_schedule.h (batched passes, per-thread FIFO) against a literal restatement of
// Sim3Solver::iterate (cslam/src/Sim3Solver.cpp:120-191) inside the round-robin of LoopFinder::ComputeSim3 (LoopFinder.cpp:288-346), both on
// the same array of raw rand() values and the same CPU evaluator.  A verifier rejects the first `reject` events (SearchBySim3 + OptimizeSim3
// failing), so the loop goes on after a success.  Two schedules run back to back per seed, so the FIFO carries values from one to the next.
// Built and run by tests/test_sim3_ransac_cpu.py; prints "sim3 schedule ok: <seeds> seeds, <events> events, <hyps> hypotheses".
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sim3_schedule.h"

namespace {

uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}

// a CPU evaluator: inlier count, "R/t/s" and mask derived from (seed, candidate, sample) so that successes come at data-dependent places
struct CpuEval {
  uint32_t salt;
  std::vector<int> N;
  int min_inliers;
  int count(int c, const int* idx) const {
    const uint32_t h = mix(salt ^ mix(c * 7919u + idx[0] * 31u + idx[1] * 131071u + idx[2] * 524287u));
    if (h % 97 < 3) return min_inliers + 1 + (int)(h / 97 % 6);   // a success (or a tie / miss against a better earlier best)
    return (int)(h / 97 % (unsigned)(min_inliers + 1));
  }
  void operator()(const std::vector<int32_t>& hc, const std::vector<int32_t>& hi, std::vector<int32_t>& n_inl, std::vector<float>& rts,
                  std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask) {
    const int H = (int)hc.size();
    n_inl.resize(H); rts.assign(13 * (size_t)H, 0.f); mask_off.assign(H + 1, 0); mask.clear();
    for (int h = 0; h < H; h++) {
      n_inl[h] = count(hc[h], &hi[3 * h]);
      for (int j = 0; j < 3; j++) rts[13 * h + j] = (float)hi[3 * h + j];
      rts[13 * h + 12] = (float)hc[h];
      const int w = (N[hc[h]] + 31) / 32;
      for (int k = 0; k < w; k++) mask.push_back(mix(hi[3 * h] * 3u + k));
      mask_off[h + 1] = mask_off[h] + w;
    }
  }
};

struct Ev { int cand, n, i0, i1, i2; uint32_t m0; };

// the literal reference: one Sim3Solver per candidate, iterate(nIterations) round-robin
struct LiteralSolver {
  int N, minInl, maxIts, its = 0, best = 0;
  bool fixed_discard = false;
};

std::vector<Ev> literal(const CpuEval& ev, const std::vector<int>& N, const ccm_sim3::Params& p, int reject, const std::vector<int>& draws, size_t& cur) {
  const int K = (int)N.size();
  std::vector<LiteralSolver> s(K);
  std::vector<char> discarded(K, 0);
  int nCandidates = 0;
  for (int c = 0; c < K; c++) {
    s[c].N = N[c]; s[c].minInl = p.min_inliers;
    s[c].maxIts = ccm_sim3::ransac_max_iterations(N[c], p.probability, p.min_inliers, p.max_iterations);
    nCandidates++;
  }
  std::vector<Ev> out;
  bool bMatch = false;
  while (nCandidates > 0 && !bMatch) {
    for (int i = 0; i < K; i++) {
      if (discarded[i]) continue;
      LiteralSolver& S = s[i];
      bool bNoMore = false, got = false;
      Ev e{};
      if (S.N < S.minInl) {
        bNoMore = true;
      } else {
        int nCurrent = 0;
        while (S.its < S.maxIts && nCurrent < p.solver_iterations) {
          nCurrent++; S.its++;
          std::vector<int> avail(S.N);
          for (int k = 0; k < S.N; k++) avail[k] = k;
          int idx[3];
          for (int j = 0; j < 3; j++) {
            const int raw = draws.at(cur++);
            const int randi = ccm_sim3::random_int(raw, (int)avail.size());
            idx[j] = avail[randi];
            avail[randi] = avail.back();
            avail.pop_back();
          }
          const int n = ev.count(i, idx);
          if (n >= S.best) {
            S.best = n;
            if (n > S.minInl) { got = true; e = Ev{i, n, idx[0], idx[1], idx[2], mix(idx[0] * 3u)}; break; }
          }
        }
        if (!got && S.its >= S.maxIts) bNoMore = true;
      }
      if (bNoMore) { discarded[i] = 1; nCandidates--; }
      if (got) {
        out.push_back(e);
        if ((int)out.size() > reject) { bMatch = true; break; }
      }
    }
  }
  return out;
}

}  // namespace

int main() {
  int n_events = 0;
  long long n_hyps = 0;
  const int n_seeds = 200;
  for (int seed = 0; seed < n_seeds; seed++) {
    uint32_t st = mix(seed + 1);
    auto rnd = [&]() { st = mix(st + 0x9e3779b9U); return st; };
    std::vector<int> draws(60000);
    for (auto& d : draws) d = (int)(rnd() & 0x7fffffff);   // RAND_MAX = 2^31 - 1 on glibc
    ccm_sim3::draw_fifo().clear();
    size_t lit_cur = 0, src_cur = 0;
    for (int run = 0; run < 2; run++) {
      ccm_sim3::Params p;
      p.max_iterations = (rnd() % 3 == 0) ? 300 : 20 + (int)(rnd() % 40);   // short schedules too, so that failures run out
      const int K = 1 + (int)(rnd() % 10);
      std::vector<int> N(K);
      for (int c = 0; c < K; c++) {
        const uint32_t r = rnd() % 10;
        N[c] = r == 0 ? (int)(rnd() % 6) : r == 1 ? 6 : 7 + (int)(rnd() % 60);   // some below MinInliers, some equal to it
      }
      const int reject = (int)(rnd() % 3 == 0 ? 0 : rnd() % 3 == 0 ? 1 : 3);
      CpuEval ev{rnd(), N, p.min_inliers};
      const std::vector<Ev> want = literal(ev, N, p, reject, draws, lit_cur);
      ccm_sim3::Schedule<CpuEval> sc(N, p, [&](int& v) { if (src_cur >= draws.size()) return false; v = draws[src_cur++]; return true; });
      std::vector<Ev> got;
      ccm_sim3::Event e;
      while ((int)got.size() <= reject && sc.next(ev, e)) {
        if (e.s != (float)e.cand) { std::printf("MISMATCH seed %d: the event carries another hypothesis' results\n", seed); return 1; }
        got.push_back(Ev{e.cand, e.n_inliers, (int)e.R[0], (int)e.R[1], (int)e.R[2], e.mask.empty() ? 0u : e.mask[0]});
      }
      n_hyps += sc.hyps_evaluated();
      bool ok = got.size() == want.size();
      for (size_t i = 0; ok && i < got.size(); i++)
        ok = got[i].cand == want[i].cand && got[i].n == want[i].n && got[i].i0 == want[i].i0 && got[i].i1 == want[i].i1 && got[i].i2 == want[i].i2 &&
             got[i].m0 == want[i].m0;
      // the values the sequential reference consumed are exactly those taken from the source minus what waits in the FIFO, and the FIFO holds the next ones in order
      const auto& q = ccm_sim3::draw_fifo();
      ok = ok && src_cur - q.size() == lit_cur;
      for (size_t i = 0; ok && i < q.size(); i++) ok = q[i] == draws[lit_cur + i];
      if (!ok) {
        std::printf("MISMATCH seed %d run %d: %zu events, literal %zu; consumed %zu (source %zu, fifo %zu), literal %zu\n", seed, run, got.size(), want.size(),
                    src_cur - q.size(), src_cur, q.size(), lit_cur);
        for (size_t i = 0; i < want.size() || i < got.size(); i++)
          std::printf("  %zu: got %d/%d (%d %d %d)  want %d/%d (%d %d %d)\n", i, i < got.size() ? got[i].cand : -1, i < got.size() ? got[i].n : -1,
                      i < got.size() ? got[i].i0 : -1, i < got.size() ? got[i].i1 : -1, i < got.size() ? got[i].i2 : -1, i < want.size() ? want[i].cand : -1,
                      i < want.size() ? want[i].n : -1, i < want.size() ? want[i].i0 : -1, i < want.size() ? want[i].i1 : -1, i < want.size() ? want[i].i2 : -1);
        return 1;
      }
      n_events += (int)got.size();
    }
  }
  std::printf("sim3 schedule ok: %d seeds, %d events, %lld hypotheses\n", n_seeds, n_events, n_hyps);
  return 0;
}
