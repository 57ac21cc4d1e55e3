// pnp_check.cpp — ccm_slam_amd/host/pnp_schedule.h (batched passes, cached Refine, per-thread FIFO) against a literal restatement of PnPsolver::iterate and
// Refine (cslam/src/PnPSolver.cpp:155-296) inside the round-robin `for each candidate not discarded: iterate(n)`, both on the same array of raw rand() values and
// on csrc/pnp_math.h.  tests/test_pnp_cpu.py builds this with -fsanitize=address,undefined as a stand-alone program: every array of the EPnP solve, of Refine's
// variable n and of the schedule is walked under the sanitizers, on regular scenes and on degenerate samples (a repeated 3D point, coplanar points, a point on the
// camera plane).  A Sim3 schedule runs after each PnP one on the same thread, so the FIFO hands values from one solver to the other.  The pieces both schedules
// take from ransac_schedule.h are checked on their own: draws_to_indices<S> against the literal removal, and a pass cut where a supplied array ends.
// Prints "pnp schedule ok: <seeds> seeds, <events> events, <hyps> hypotheses".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pnp_schedule.h"
#include "sim3_schedule.h"

namespace {

int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)

uint64_t g_rng = 1;
double uni() {   // [0, 1)
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}

ccm_pnp::Candidate scene(int n_true, int n_out, double fu) {
  ccm_pnp::Candidate c;
  c.cam[0] = fu; c.cam[1] = fu + 7; c.cam[2] = 320; c.cam[3] = 240;
  const double a = 0.2 * uni() - 0.1, ca = cos(a), sa = sin(a);
  const double R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca}, t[3] = {0.2 * uni(), -0.1 * uni(), 0.3 * uni()};
  for (int i = 0; i < n_true + n_out; i++) {
    const float X[3] = {(float)(3 * uni() - 1.5), (float)(3 * uni() - 1.5), (float)(4 + 2 * uni())};
    double Xc[3];
    for (int r = 0; r < 3; r++) Xc[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
    double u = c.cam[2] + c.cam[0] * Xc[0] / Xc[2], v = c.cam[3] + c.cam[1] * Xc[1] / Xc[2];
    if (i >= n_true) { u += 30 + 40 * uni(); v -= 30 + 40 * uni(); }
    c.P3Dw.insert(c.P3Dw.end(), X, X + 3);
    c.P2D.push_back((float)u); c.P2D.push_back((float)v);
    c.sigma2.push_back(i % 3 == 0 ? 1.44f : 1.0f);
  }
  return c;
}

struct HostEval {
  std::vector<int32_t> pt_off;
  std::vector<float> P3Dw, P2D, max_err;
  std::vector<double> cam;
  void operator()(const std::vector<int32_t>& hc, const std::vector<int32_t>& hi, std::vector<int32_t>& n_inl, std::vector<double>& Rt,
                  std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask) {
    const int H = (int)hc.size();
    size_t words = 0;
    for (int h = 0; h < H; h++) words += (pt_off[hc[h] + 1] - pt_off[hc[h]] + 31) / 32;
    n_inl.resize(H); Rt.resize(12 * (size_t)H); mask_off.resize(H + 1); mask.resize(words);
    const int rc = ccm_pnp::eval_host((int)pt_off.size() - 1, pt_off.data(), P3Dw.data(), P2D.data(), max_err.data(), cam.data(), H, hc.data(), hi.data(),
                                      n_inl.data(), Rt.data(), mask_off.data(), mask.data());
    EXPECT(rc == 0);
  }
};

struct Ev {
  int cand, n; bool refined, no_more; float Tcw[16]; std::vector<uint32_t> mask;
  bool operator==(const Ev& o) const {
    return cand == o.cand && n == o.n && refined == o.refined && no_more == o.no_more && !memcmp(Tcw, o.Tcw, sizeof Tcw) && mask == o.mask;
  }
};

// the literal reference: one PnPsolver per candidate
struct Literal {
  const ccm_pnp::Candidate* c;
  std::vector<float> max_err;
  int N, minInl, maxIts, its = 0, best = 0;
  std::vector<uint32_t> best_mask;
  float best_tcw[16];
  // iterate(nIterations): true when a pose comes back
  bool iterate(int nIterations, const std::vector<int>& draws, size_t& cur, bool& bNoMore, Ev& ev) {
    bNoMore = false;
    if (N < minInl) { bNoMore = true; return false; }
    int nCurrent = 0;
    while (its < maxIts || nCurrent < nIterations) {
      nCurrent++; its++;
      std::vector<int> avail(N);
      for (int i = 0; i < N; i++) avail[i] = i;
      int32_t idx[4];
      for (int i = 0; i < 4; i++) {
        const int randi = ccm_ransac::random_int(draws.at(cur++), (int)avail.size());
        idx[i] = avail[randi];
        avail[randi] = avail.back();
        avail.pop_back();
      }
      const int32_t pt_off[2] = {0, N}, hc = 0;
      int32_t n_inl = 0, mask_off[2];
      double Rt[12];
      std::vector<uint32_t> mask((N + 31) / 32);
      EXPECT(ccm_pnp::eval_host(1, pt_off, c->P3Dw.data(), c->P2D.data(), max_err.data(), c->cam, 1, &hc, idx, &n_inl, Rt, mask_off, mask.data()) == 0);
      if (n_inl >= minInl) {
        if (n_inl > best) { best_mask = mask; best = n_inl; ccm_pnp::to_tcw(Rt, best_tcw); }
        // Refine(), computed every time
        double rRt[12];
        std::vector<uint32_t> rmask;
        const int nr = ccm_pnp::refine_host(N, c->P3Dw.data(), c->P2D.data(), max_err.data(), c->cam, best_mask, rRt, rmask);
        if (nr > minInl) {
          ev.n = nr; ev.refined = true; ev.no_more = false; ev.mask = rmask;
          ccm_pnp::to_tcw(rRt, ev.Tcw);
          return true;
        }
      }
    }
    if (its >= maxIts) {
      bNoMore = true;
      if (best >= minInl) {
        ev.n = best; ev.refined = false; ev.no_more = true; ev.mask = best_mask;
        memcpy(ev.Tcw, best_tcw, sizeof best_tcw);
        return true;
      }
    }
    return false;
  }
};

std::vector<Ev> literal(const std::vector<ccm_pnp::Candidate>& cands, const ccm_pnp::Params& p, int max_events, const std::vector<int>& draws, size_t& cur) {
  const int K = (int)cands.size();
  std::vector<Literal> s(K);
  std::vector<char> discarded(K, 0);
  int live = K;
  for (int c = 0; c < K; c++) {
    s[c].c = &cands[c]; s[c].N = cands[c].N();
    const ccm_pnp::Ransac r = ccm_pnp::set_ransac_parameters(s[c].N, p);
    s[c].minInl = r.min_inliers; s[c].maxIts = r.max_its;
    for (float v : cands[c].sigma2) s[c].max_err.push_back(v * p.th2);
  }
  std::vector<Ev> out;
  while (live > 0)
    for (int c = 0; c < K; c++) {
      if (discarded[c]) continue;
      bool bNoMore = false;
      Ev ev;
      const bool got = s[c].iterate(p.solver_iterations, draws, cur, bNoMore, ev);
      if (bNoMore) { discarded[c] = 1; live--; }
      if (got) {
        ev.cand = c;
        out.push_back(ev);
        if ((int)out.size() >= max_events) return out;
      }
    }
  return out;
}

// a Sim3 evaluator that needs no data: the Sim3 schedule is only the FIFO's next consumer here
struct Sim3Eval {
  std::vector<int32_t> seen;   // every sample index, in order
  void operator()(const std::vector<int32_t>& hc, const std::vector<int32_t>& hi, std::vector<int32_t>& n_inl, std::vector<float>& rts, std::vector<int32_t>& mask_off,
                  std::vector<uint32_t>& mask) {
    const int H = (int)hc.size();
    n_inl.assign(H, 0); rts.assign(13 * (size_t)H, 0.f); mask_off.assign(H + 1, 0); mask.clear();
    for (int h = 0; h < H; h++) { mask.push_back(0); mask_off[h + 1] = h + 1; }
    seen.insert(seen.end(), hi.begin(), hi.end());
  }
};

void degenerate_samples() {
  // four points with a repeated one, four coplanar points, a point on the camera plane, a point behind the camera: nothing is trapped, every array stays in bounds
  ccm_pnp::Candidate c = scene(12, 0, 500);
  for (int r = 0; r < 3; r++) c.P3Dw[3 * 1 + r] = c.P3Dw[r];              // point 1 = point 0
  for (int i = 4; i < 8; i++) c.P3Dw[3 * i + 2] = 5.f;                    // points 4..7 on the plane z = 5
  c.P3Dw[3 * 8 + 2] = 0.f; c.P3Dw[3 * 9 + 2] = -3.f;
  std::vector<float> max_err(12, 5.991f);
  const int32_t pt_off[2] = {0, 12};
  const int32_t hc[4] = {0, 0, 0, 0}, hi[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 2, 3, 10, 9, 2, 3, 11};
  int32_t n_inl[4], mask_off[5];
  double Rt[48];
  uint32_t mask[4];
  EXPECT(ccm_pnp::eval_host(1, pt_off, c.P3Dw.data(), c.P2D.data(), max_err.data(), c.cam, 4, hc, hi, n_inl, Rt, mask_off, mask) == 0);
  for (int h = 0; h < 4; h++) EXPECT(n_inl[h] >= 0 && n_inl[h] <= 12 && mask[h] >> 12 == 0);
  const int32_t bad[4] = {0, 1, 2, 2};
  EXPECT(ccm_pnp::eval_host(1, pt_off, c.P3Dw.data(), c.P2D.data(), max_err.data(), c.cam, 1, hc, bad, n_inl, Rt, mask_off, mask) == -1);
}

// ransac_schedule.h's draws_to_indices<S> against the literal "identity vector, swap with back, pop" of the reference, for every N from S to S + 6 and N = 1000:
// every pattern of 0 and RAND_MAX over the S slots (slot 0 each time, the back each time, and the mixes), then drawn values
template <int S>
void indices_against_the_literal() {
  for (int k = 0; k <= 7; k++)
    for (int rep = 0; rep < (1 << S) + 50; rep++) {
      const int N = k < 7 ? S + k : 1000;
      int raw[S], idx[S];
      for (int j = 0; j < S; j++) raw[j] = rep < (1 << S) ? (rep >> j & 1 ? RAND_MAX : 0) : (int)(uni() * 2147483648.0);
      std::vector<int> avail(N);
      for (int i = 0; i < N; i++) avail[i] = i;
      ccm_ransac::draws_to_indices<S>(raw, N, idx);
      for (int j = 0; j < S; j++) {
        const int randi = ccm_ransac::random_int(raw[j], (int)avail.size());
        EXPECT(idx[j] == avail[randi]);
        avail[randi] = avail.back();
        avail.pop_back();
      }
    }
}

// a supplied array that ends in the middle of a hypothesis: the pass is cut there, evaluates the complete hypotheses only, and the FIFO then begins with exactly the
// partial hypothesis's values, in order; Sim3's single-solver call evaluates nothing and gives back every value it took
void cut_in_the_middle_of_a_hypothesis() {
  std::vector<int> draws(14);
  for (int& d : draws) d = (int)(uni() * 2147483647.0);
  std::deque<int>& fifo = ccm_ransac::draw_fifo();
  fifo.clear();
  {   // the pass itself: three complete hypotheses of four draws and two values of a fourth
    size_t at = 0;
    ccm_ransac::Pass<4, double> p;
    const ccm_ransac::DrawSource src = [&](int& v) { if (at >= draws.size()) return false; v = draws[at++]; return true; };
    const bool whole = p.take(std::vector<int>(1, 0), std::vector<int>(1, 6), [](int) { return 30; }, src);
    EXPECT(!whole && at == 14 && p.source_draws() == 14);
    EXPECT(p.hyp_cand.size() == 3 && p.hyp_idx.size() == 12 && p.raws == std::vector<int>(draws.begin(), draws.begin() + 12));
    EXPECT(fifo.size() == 2 && fifo[0] == draws[12] && fifo[1] == draws[13]);
    fifo.clear();
  }
  {   // the schedule on a candidate that never reaches the threshold: the three hypotheses are evaluated, then the replay finds the draws exhausted
    std::vector<ccm_pnp::Candidate> cands(1, scene(0, 30, 480));
    size_t at = 0;
    ccm_pnp::Schedule<HostEval> sched(cands, ccm_pnp::Params(), [&](int& v) { if (at >= draws.size()) return false; v = draws[at++]; return true; });
    HostEval he;
    he.pt_off = {0, 30}; he.P3Dw = cands[0].P3Dw; he.P2D = cands[0].P2D; he.max_err = sched.max_err(0);
    he.cam.assign(cands[0].cam, cands[0].cam + 4);
    ccm_pnp::Event e;
    bool exhausted = false;
    try { sched.next(he, e); } catch (const ccm_ransac::DrawsExhausted&) { exhausted = true; }
    EXPECT(exhausted && sched.hyps_evaluated() == 3 && sched.passes() == 1 && sched.source_draws() == 14);
    EXPECT(fifo.size() == 2 && fifo[0] == draws[12] && fifo[1] == draws[13]);
    fifo.clear();
  }
  {   // Sim3Solver::iterate(5) on seven values: two complete samples and one value
    size_t at = 0;
    Sim3Eval se;
    ccm_sim3::SolverState st;
    st.N = 50; st.max_its = 100;
    bool no_more = false, moved = false, exhausted = false;
    ccm_sim3::Event best;
    try {
      ccm_sim3::iterate_one(se, st, 5, [&](int& v) { if (at >= 7) return false; v = draws[at++]; return true; }, no_more, moved, best);
    } catch (const ccm_ransac::DrawsExhausted&) { exhausted = true; }
    EXPECT(exhausted && se.seen.empty() && st.its == 0 && fifo.size() == 7);
    for (size_t i = 0; i < fifo.size() && i < 7; i++) EXPECT(fifo[i] == draws[i]);
    fifo.clear();
  }
}

}  // namespace

int main() {
  degenerate_samples();
  indices_against_the_literal<3>();
  indices_against_the_literal<4>();
  cut_in_the_middle_of_a_hypothesis();
  long n_events = 0, n_hyps = 0;
  const int seeds = 6;
  for (int seed = 0; seed < seeds; seed++) {
    g_rng = 1000 + seed;
    std::vector<ccm_pnp::Candidate> cands;
    cands.push_back(scene(40, 20 + 5 * seed, 480));
    cands.push_back(scene(5, 1, 500));              // N < mRansacMinInliers: discarded before any draw
    cands.push_back(scene(30, 45, 520));
    if (seed & 1) cands.push_back(scene(9, 60, 500));   // hardly ever reaches the threshold: runs to max(mRansacMaxIts, n)
    ccm_pnp::Params p;
    p.max_iterations = 60 + 40 * seed;
    std::vector<int> draws(400000);
    for (int& d : draws) d = (int)(uni() * 2147483647.0);
    for (int max_events : {1, 2, 1000}) {
      size_t cur = 0;
      const std::vector<Ev> want = literal(cands, p, max_events, draws, cur);
      // the schedule on the same values
      ccm_ransac::draw_fifo().clear();
      size_t at = 0;
      ccm_pnp::Schedule<HostEval> sched(cands, p, [&](int& v) { if (at >= draws.size()) return false; v = draws[at++]; return true; });
      HostEval he;
      he.pt_off.push_back(0);
      std::vector<int32_t> remap;
      for (size_t c = 0; c < cands.size(); c++) {
        he.pt_off.push_back(he.pt_off.back() + cands[c].N());
        he.P3Dw.insert(he.P3Dw.end(), cands[c].P3Dw.begin(), cands[c].P3Dw.end());
        he.P2D.insert(he.P2D.end(), cands[c].P2D.begin(), cands[c].P2D.end());
        he.max_err.insert(he.max_err.end(), sched.max_err((int)c).begin(), sched.max_err((int)c).end());
        he.cam.insert(he.cam.end(), cands[c].cam, cands[c].cam + 4);
      }
      std::vector<Ev> got;
      ccm_pnp::Event e;
      while ((int)got.size() < max_events && sched.next(he, e)) {
        Ev g; g.cand = e.cand; g.n = e.n_inliers; g.refined = e.refined; g.no_more = e.no_more; g.mask = e.mask;
        memcpy(g.Tcw, e.Tcw, sizeof g.Tcw);
        got.push_back(g);
      }
      EXPECT(got.size() == want.size());
      for (size_t i = 0; i < got.size() && i < want.size(); i++) EXPECT(got[i] == want[i]);
      if (max_events == 1000) {
        bool refined = false, discarded_small = sched.discarded(1) && sched.iterations(1) == 0;
        for (const Ev& g : got) refined |= g.refined;
        EXPECT(refined); EXPECT(discarded_small);
        EXPECT(sched.refines() <= sched.hyps_evaluated());
      }
      // values taken = values the literal loop used + what waits in the FIFO, and the FIFO holds exactly the values the literal loop would draw next
      const std::deque<int>& fifo = ccm_ransac::draw_fifo();
      EXPECT(at == cur + fifo.size());
      for (size_t i = 0; i < fifo.size(); i++) EXPECT(fifo[i] == draws[cur + i]);
      // the next consumer of the thread is a Sim3 schedule: its samples are those of the values from `cur` on
      const size_t pending = fifo.size();
      {
        ccm_sim3::Params sp; sp.max_iterations = 7; sp.solver_iterations = 5;
        Sim3Eval se;
        ccm_sim3::Schedule<Sim3Eval> s3(std::vector<int>(1, 50), sp, [&](int& v) { if (at >= draws.size()) return false; v = draws[at++]; return true; });
        ccm_sim3::Event s3e;
        EXPECT(!s3.next(se, s3e));
        EXPECT(se.seen.size() == 3u * s3.max_iterations(0));
        for (size_t h = 0; 3 * h < se.seen.size(); h++) {
          int idx[3];
          ccm_sim3::draws_to_indices(&draws[cur + 3 * h], 50, idx);
          EXPECT(idx[0] == se.seen[3 * h] && idx[1] == se.seen[3 * h + 1] && idx[2] == se.seen[3 * h + 2]);
        }
        EXPECT(s3.source_draws() == (int64_t)(se.seen.size() > pending ? se.seen.size() - pending : 0));
      }
      n_events += (long)got.size(); n_hyps += (long)sched.hyps_evaluated();
      ccm_ransac::draw_fifo().clear();
    }
  }
  // min_set other than 4 is an error
  bool threw = false;
  try {
    ccm_pnp::Params p; p.min_set = 5;
    ccm_pnp::Schedule<HostEval> s(std::vector<ccm_pnp::Candidate>(), p, ccm_pnp::rand_source());
  } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);
  if (g_fail) { printf("pnp schedule: %d failures\n", g_fail); return 1; }
  printf("pnp schedule ok: %d seeds, %ld events, %ld hypotheses\n", seeds, n_events, n_hyps);
  return 0;
}
