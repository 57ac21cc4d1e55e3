// ransac_wave.h — what the minimal-sample RANSACs over candidates in CSR share: the wave over a form (ransac_wave<F>: sim3_ransac_kernel
// of sim3ransac.hip; pnp_ransac_kernel of pnp.hip is the same wave written out, for the reason its header gives); the same walk without lanes for the host
// (ransac_eval_host<F>: the host evaluator of pnp_schedule.h and tests/host/sim3_hyp_check.cpp); and the checks of the hypotheses that the two entry points and
// the host evaluator make before anything is evaluated.
//
// The wave.  One wave64 per hypothesis, kRansacWavesPerBlock waves per workgroup that share nothing, so a wave past the last hypothesis simply leaves.  Lane 0 runs the
// form's serial minimal solve and writes the model out; the form hands the model to the other lanes through lane shuffles; the lanes then stride 64 over the
// candidate's points and a ballot gives 64 inlier bits at a time: two mask words, written by lanes 0 and 1 (the second only where the candidate has that word, so
// no bit at or beyond N is ever set and every word of the hypothesis is written), and the count.  Points are read from global memory: the hypotheses of one
// launch share a candidate's points through L2.
//
// A form F supplies (every member inlines away):
//   Args                          the kernel's arguments: at least H, pt_off, hyp_cand, hyp_idx, mask_off, n_inl, mask
//   S, kWorkDoubles               the sample size; the doubles of work space the solve wants (0: none)
//   F(a, c)                       every lane: what the solve and the test need of candidate c, the model zeroed
//   solve(a, h, p0, work)         lane 0 only: the model of hypothesis h (sample a.hyp_idx[S h ..], points from p0) into the form and into the model output
//   broadcast()                   device only, every lane: lane 0's model
//   prepare(a)                    every lane, once the model is there: what only the test needs (kept out of the registers that live across the solve)
//   inlier(a, g) -> bool          point g (global index) under the model
// The first four and the last two are host + device (the *_math.h headers hold them), so g++ compiles the same lines.
#pragma once
#include <stdint.h>
#include <string>

constexpr int kRansacWavesPerBlock = 4;

#if defined(__HIPCC__)
// work: this wave's kWorkDoubles doubles (the kernel's LDS slice), or nullptr where the form wants none
template <class F>
__device__ __forceinline__ void ransac_wave(const typename F::Args& a, double* work) {
  const int lane = threadIdx.x & 63;
  const int h = blockIdx.x * kRansacWavesPerBlock + (threadIdx.x >> 6);
  if (h >= a.H) return;   // whole waves only: no barrier below
  const int c = a.hyp_cand[h];
  const int p0 = a.pt_off[c], N = a.pt_off[c + 1] - p0;
  F f(a, c);   // lanes 1..63 take lane 0's model through the shuffles below
  if (lane == 0) f.solve(a, h, p0, work);
  f.broadcast();
  f.prepare(a);
  uint32_t* m = a.mask + a.mask_off[h];
  const int n_words = (N + 31) >> 5;
  int count = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < N) in = f.inlier(a, p0 + i);
    const uint64_t b = __ballot(in);
    count += __popcll(b);
    const int w = base >> 5;
    if (lane == 0) m[w] = (uint32_t)b;
    if (lane == 1 && w + 1 < n_words) m[w + 1] = (uint32_t)(b >> 32);
  }
  if (lane == 0) a.n_inl[h] = count;
}
#endif

// The same hypotheses on the calling thread: the outputs of the kernel, every mask word zeroed before its bits are set.
template <class F>
inline void ransac_eval_host(const typename F::Args& a) {
  double work[F::kWorkDoubles + 1];
  for (int h = 0; h < a.H; h++) {
    const int c = a.hyp_cand[h];
    const int p0 = a.pt_off[c], N = a.pt_off[c + 1] - p0;
    F f(a, c);
    f.solve(a, h, p0, work);
    f.prepare(a);
    uint32_t* m = a.mask + a.mask_off[h];
    for (int w = 0; w < (N + 31) >> 5; w++) m[w] = 0;
    int count = 0;
    for (int i = 0; i < N; i++)
      if (f.inlier(a, p0 + i)) { m[i >> 5] |= 1u << (i & 31); count++; }
    a.n_inl[h] = count;
  }
}

// The checks of a call's candidates and hypotheses, in this order: pt_off[0] == 0; at least S points per candidate; per hypothesis its candidate < K, every
// index within its candidate, S distinct indices, and the running sum of mask words within int32.  Fills mask_off[0 .. H] as far as the checks pass and, at
// RANSAC_OK, *words = mask_off[H].  The two entry points always differed in what a sample with BOTH defects reports, and each keeps its answer: range_first
// (ccm_sim3_ransac_eval) looks at the range of all S indices before any repeat; otherwise (ccm_pnp_ransac_eval) index j is compared with the earlier ones as soon
// as it is in range, so (5, 5, 99, 0) is a repeated index there.
enum RansacCheck { RANSAC_OK = 0, RANSAC_PT_OFF0, RANSAC_FEW_POINTS, RANSAC_CAND_RANGE, RANSAC_IDX_RANGE, RANSAC_IDX_REPEATED, RANSAC_MASK_SIZE };

template <int S>
inline RansacCheck ransac_check_hyps(int K, const int32_t* pt_off, int H, const int32_t* hyp_cand, const int32_t* hyp_idx, int32_t* mask_off, int64_t* words_out,
                                     bool range_first) {
  if (pt_off[0] != 0) return RANSAC_PT_OFF0;
  for (int c = 0; c < K; c++)
    if (pt_off[c + 1] - pt_off[c] < S) return RANSAC_FEW_POINTS;
  int64_t words = 0;
  mask_off[0] = 0;
  for (int h = 0; h < H; h++) {
    const int c = hyp_cand[h];
    if (c < 0 || c >= K) return RANSAC_CAND_RANGE;
    const int N = pt_off[c + 1] - pt_off[c];
    const int32_t* ix = hyp_idx + S * (size_t)h;
    for (int pass = range_first ? 0 : 1; pass < 2; pass++)   // pass 0: ranges only; pass 1: ranges (again, or for the first time) with the repeats
      for (int j = 0; j < S; j++) {
        if (ix[j] < 0 || ix[j] >= N) return RANSAC_IDX_RANGE;
        for (int k = 0; pass == 1 && k < j; k++)
          if (ix[k] == ix[j]) return RANSAC_IDX_REPEATED;
      }
    words += (N + 31) >> 5;
    if (words > INT32_MAX) return RANSAC_MASK_SIZE;
    mask_off[h + 1] = (int32_t)words;
  }
  *words_out = words;
  return RANSAC_OK;
}

// what an entry point reports behind its own name
inline std::string ransac_check_text(RansacCheck r, int S) {
  switch (r) {
    case RANSAC_PT_OFF0: return "pt_off[0] != 0";
    case RANSAC_FEW_POINTS: return "a candidate with fewer than " + std::to_string(S) + " points";
    case RANSAC_CAND_RANGE: return "hypothesis candidate out of range";
    case RANSAC_IDX_RANGE: return "point index out of range";
    case RANSAC_IDX_REPEATED: return "repeated point index in a hypothesis";
    case RANSAC_MASK_SIZE: return "mask too large";
    default: return "";
  }
}
