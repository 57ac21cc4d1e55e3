// kfcull.hip — the server's keyframe culling walk on the device: ccm_kfcull_walk, LocalMapping::KeyFrameCullingV3 (Mapping.cpp:804-862) over the candidates in walk
// order with what KeyFrame::SetBadFlag (KeyFrame.cpp:990-997) does to the points of a culled keyframe.  The rules are kfcull_math.h.
//
// Layout: two launches.
//   eval   every (candidate, slot) on the INITIAL state, 256 slots per workgroup, up to kKcMaxChunks workgroups per candidate (longer lists stride).  A lane walks
//          its slot's observers when the point has at most 64 of them; points with more are handed to the whole wave, one after the other, 64 observers per step
//          with a ballot count.  The switch is the length of the point's observer list read from obs_off.  Each slot leaves one byte (counted, redundant, volatile =
//          the point lists an earlier candidate that can be erased); the candidate's sums of the volatile and the other slots are reduced per wave by ballot and
//          popcount, per workgroup through LDS, and added to global integers (integer sums do not depend on arrival order).
//   walk   ONE workgroup of 1024 lanes takes the candidates in order.  Until the first erasure, and for a candidate without volatile slots, the sums of eval are the
//          answer.  Otherwise its volatile slots are counted again against the current state (erased bitmask, n(p), gone(p) in global scratch; a lane per slot, the
//          early break at th_obs keeps long observer lists short here).  An erasure sets the candidate's bit, then the lanes stride over its slots: the first lane to
//          stamp a point with the candidate's number lowers n(p) and decides gone(p), so a point listed twice is erased once.
// Nothing waits on another workgroup: the ordered part is one workgroup, and the kernel boundary orders eval before walk.
#include "common.h"
#include "kfcull_math.h"
#include "stage_blocks.h"
#include <algorithm>

namespace {

constexpr int kKcBlock = 256;
constexpr int kKcWaves = kKcBlock / 64;
constexpr int kKcMaxChunks = 8;        // workgroups per candidate in eval: lists beyond 2048 slots stride
constexpr int kKcLaneMax = 64;         // observers one lane walks alone; beyond, the wave takes the slot
constexpr int kKcWalkBlock = 1024;
constexpr int kKcWalkWaves = kKcWalkBlock / 64;

struct KfcullArgs {
  int n_cand, chunks, th_obs;
  double thres;
  const int32_t *cand_flags, *list_off, *list_pt, *obs_off, *obs_kf;
  const uint8_t *list_level, *obs_level, *obs_bad;
  uint8_t* slot;          // one byte per list entry
  int32_t* sums;          // [4][n_cand]: nMPs / nRed of the non-volatile slots, nMPs / nRed of the volatile ones, all on the initial state
  uint32_t* erased;       // one bit per candidate
  int32_t* stamp;         // [n_pt]: 1 + the candidate whose erasure touched the point last
  int32_t *hdr, *verdict, *n_mps, *n_red, *gone, *nobs;   // output block; gone / nobs start as the caller's pt_bad / pt_nobs
};

__global__ __launch_bounds__(kKcBlock) void kfcull_eval_kernel(KfcullArgs a) {
  __shared__ int32_t part[kKcWaves][4];
  const int k = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.cand_flags[k] & KFCULL_SKIP) return;
  const int32_t e0 = a.list_off[k], e1 = a.list_off[k + 1];
  int32_t s_nv_mps = 0, s_nv_red = 0, s_v_mps = 0, s_v_red = 0;     // wave totals, the same in every lane
  for (int32_t base = e0 + chunk * kKcBlock; base < e1; base += a.chunks * kKcBlock) {   // base < e1 is workgroup-uniform
    const int32_t e = base + tid;
    int32_t p = -1, level = 0;
    uint32_t byte = 0;
    bool wide = false;
    if (e < e1) {
      p = a.list_pt[e];
      if (p >= 0 && kfcull_slot_counts(p, a.gone[p])) {
        byte = KFCULL_SLOT_COUNTED;
        level = a.list_level[e];
        const int32_t o0 = a.obs_off[p], o1 = a.obs_off[p + 1];
        if (o1 - o0 > kKcLaneMax) {
          wide = true;
        } else {
          const bool checked = kfcull_point_is_checked(a.nobs[p], a.th_obs);
          int32_t n = 0;
          bool vol = false;
          for (int32_t o = o0; o < o1; o++) {      // no early break: the volatile flag needs every observer
            const int32_t kf = a.obs_kf[o];
            vol |= kfcull_observer_is_volatile(kf, k, a.cand_flags);
            n += checked && kfcull_observer_counts(kf, a.obs_bad[o] != 0, false, k, a.obs_level[o], level);
          }
          if (n >= a.th_obs) byte |= KFCULL_SLOT_REDUNDANT;
          if (vol) byte |= KFCULL_SLOT_VOLATILE;
        }
      }
    }
    // the slots of points with long observer lists: the wave takes them one by one
    unsigned long long todo = __ballot(wide);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t sp = __shfl(p, src, 64), sl = __shfl(level, src, 64);
      const int32_t o0 = a.obs_off[sp], o1 = a.obs_off[sp + 1];
      const bool checked = kfcull_point_is_checked(a.nobs[sp], a.th_obs);
      int32_t n = 0;
      bool vol = false;
      for (int32_t ob = o0; ob < o1; ob += 64) {
        const int32_t o = ob + lane;
        bool c = false, v = false;
        if (o < o1) {
          const int32_t kf = a.obs_kf[o];
          v = kfcull_observer_is_volatile(kf, k, a.cand_flags);
          c = checked && kfcull_observer_counts(kf, a.obs_bad[o] != 0, false, k, a.obs_level[o], sl);
        }
        n += (int32_t)__popcll(__ballot(c));
        vol |= __ballot(v) != 0;
      }
      if (lane == src) byte |= (n >= a.th_obs ? KFCULL_SLOT_REDUNDANT : 0) | (vol ? KFCULL_SLOT_VOLATILE : 0);
    }
    if (e < e1) a.slot[e] = (uint8_t)byte;
    const bool counted = (byte & KFCULL_SLOT_COUNTED) != 0, red = (byte & KFCULL_SLOT_REDUNDANT) != 0, vol = (byte & KFCULL_SLOT_VOLATILE) != 0;
    s_nv_mps += (int32_t)__popcll(__ballot(counted && !vol));
    s_nv_red += (int32_t)__popcll(__ballot(red && !vol));
    s_v_mps += (int32_t)__popcll(__ballot(counted && vol));
    s_v_red += (int32_t)__popcll(__ballot(red && vol));
  }
  if (lane == 0) { part[wave][0] = s_nv_mps; part[wave][1] = s_nv_red; part[wave][2] = s_v_mps; part[wave][3] = s_v_red; }
  __syncthreads();
  if (tid < 4) {
    int32_t s = 0;
#pragma unroll
    for (int q = 0; q < kKcWaves; q++) s += part[q][tid];
    if (s) atomicAdd(&a.sums[(size_t)tid * a.n_cand + k], s);
  }
}

__global__ __launch_bounds__(kKcWalkBlock) void kfcull_walk_kernel(KfcullArgs a) {
  __shared__ int32_t part[2][kKcWalkWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t K = (size_t)a.n_cand;
  bool erased_before = false;     // workgroup-uniform, like everything that steers the loop
  int32_t n_reeval = 0;
  int phase = 0;
  for (int k = 0; k < a.n_cand; k++) {
    const int32_t flags = a.cand_flags[k];
    if (flags & KFCULL_SKIP) {
      if (tid == 0) { a.verdict[k] = KFCULL_SKIPPED; a.n_mps[k] = 0; a.n_red[k] = 0; }
      continue;
    }
    const int32_t e0 = a.list_off[k], e1 = a.list_off[k + 1];
    int32_t n_mps = a.sums[k], n_red = a.sums[K + k];
    const int32_t v_mps = a.sums[2 * K + k];
    if (kfcull_reevaluated(erased_before, v_mps)) {
      // the volatile slots again, against the current state
      int32_t m = 0, r = 0;
      for (int32_t e = e0 + tid; e < e1; e += kKcWalkBlock) {
        if (!(a.slot[e] & KFCULL_SLOT_VOLATILE)) continue;
        const int32_t p = a.list_pt[e];
        if (!kfcull_slot_counts(p, a.gone[p])) continue;
        m++;
        if (kfcull_point_is_checked(a.nobs[p], a.th_obs))
          r += kfcull_count_observers(a.obs_kf, a.obs_level, a.obs_bad, a.obs_off[p], a.obs_off[p + 1], a.erased, a.n_cand, k, a.list_level[e], a.th_obs) >= a.th_obs;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) { m += __shfl_xor(m, off, 64); r += __shfl_xor(r, off, 64); }
      if (lane == 0) { part[phase][wave][0] = m; part[phase][wave][1] = r; }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kKcWalkWaves; q++) { n_mps += part[phase][q][0]; n_red += part[phase][q][1]; }
      phase ^= 1;                 // the next reduction writes the other half: one barrier per reduction
      n_reeval++;
    } else {
      n_mps += v_mps; n_red += a.sums[3 * K + k];
    }
    const int32_t verdict = kfcull_verdict(kfcull_redundant(n_red, n_mps, a.thres), flags);
    if (tid == 0) { a.verdict[k] = verdict; a.n_mps[k] = n_mps; a.n_red[k] = n_red; }
    if (verdict != KFCULL_CULLED) continue;
    // KeyFrame::SetBadFlag: the candidate joins the erased set first, so that it is no live observer of its own points
    if (tid == 0) a.erased[k >> 5] |= 1u << (k & 31);
    __syncthreads();
    for (int32_t e = e0 + tid; e < e1; e += kKcWalkBlock) {
      const int32_t p = a.list_pt[e];
      if (p < 0 || a.gone[p]) continue;
      bool lists_back = false, live = false;
      const int32_t o1 = a.obs_off[p + 1];
      for (int32_t o = a.obs_off[p]; o < o1; o++) {
        const int32_t kf = a.obs_kf[o];
        lists_back |= kf == k;
        live |= !a.obs_bad[o] && !kfcull_erased(a.erased, a.n_cand, kf);
      }
      if (!lists_back) continue;                         // a stale slot: mObservations.count(pKF) == 0
      if (atomicExch(&a.stamp[p], k + 1) == k + 1) continue;   // the point's other slot in this list was here first
      const int32_t n = a.nobs[p] - 1;
      a.nobs[p] = n;
      if (kfcull_point_goes(n, live)) a.gone[p] = 1;
    }
    __syncthreads();
    erased_before = true;
  }
  if (tid == 0) { a.hdr[0] = n_reeval; a.hdr[1] = 0; a.hdr[2] = 0; a.hdr[3] = 0; }
}

}  // namespace

extern "C" int ccm_kfcull_walk(ccm_ctx* ctx, int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level,
                               int n_pt, const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level,
                               const uint8_t* obs_bad, int th_obs, double thres, int n_levels, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone,
                               int32_t* pt_nobs_out, int32_t* n_reeval) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_kfcull_walk: ";
  if (!verdict || !n_mps || !n_red || !n_reeval || (n_pt > 0 && (!pt_gone || !pt_nobs_out))) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
  if (const char* why = kfcull_check_args(n_cand, n_all, cand_flags, list_off, list_pt, list_level, n_pt, pt_nobs, pt_bad, obs_off, obs_kf, obs_level, obs_bad, th_obs,
                                          thres, n_levels))
    return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  const size_t K = (size_t)n_cand, P = (size_t)n_pt, NL = (size_t)list_off[n_cand];
  KfcullBlock b(K, P, NL, n_pt ? (size_t)obs_off[n_pt] : 0);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  int32_t* h_gone = b.up(b.gone);
  for (size_t p = 0; p < P; p++) h_gone[p] = pt_bad[p] != 0;
  b.put(b.nobs, pt_nobs);
  int32_t* h_flags = b.up(b.cand_flags);
  for (size_t k = 0; k < K; k++) h_flags[k] = cand_flags[k] & (KFCULL_SKIP | KFCULL_NOT_ERASE);
  b.put(b.list_off, list_off); b.put(b.list_pt, list_pt);
  if (n_pt) b.put(b.obs_off, obs_off);
  b.put(b.obs_kf, obs_kf); b.put(b.list_level, list_level); b.put(b.obs_level, obs_level); b.put(b.obs_bad, obs_bad);
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  KfcullArgs a;
  a.n_cand = n_cand; a.th_obs = th_obs; a.thres = thres;
  a.hdr = b.dev(b.hdr); a.verdict = b.dev(b.verdict); a.n_mps = b.dev(b.n_mps); a.n_red = b.dev(b.n_red); a.gone = b.dev(b.gone); a.nobs = b.dev(b.nobs);
  a.sums = b.dev(b.sums); a.erased = b.dev(b.erased); a.stamp = b.dev(b.stamp);
  a.cand_flags = b.dev(b.cand_flags); a.list_off = b.dev(b.list_off); a.list_pt = b.dev(b.list_pt); a.obs_off = b.dev(b.obs_off); a.obs_kf = b.dev(b.obs_kf);
  a.list_level = b.dev(b.list_level); a.obs_level = b.dev(b.obs_level); a.obs_bad = b.dev(b.obs_bad); a.slot = b.dev(b.slot);
  int32_t longest = 0;
  for (int k = 0; k < n_cand; k++) longest = std::max(longest, list_off[k + 1] - list_off[k]);
  a.chunks = std::min(kKcMaxChunks, std::max(1, (longest + kKcBlock - 1) / kKcBlock));
  // the grid is n_cand * chunks workgroups: fold the chunks when that would pass the grid limit
  while (a.chunks > 1 && K * (size_t)a.chunks > (size_t)INT32_MAX) a.chunks >>= 1;
  if (NL) hipLaunchKernelGGL(kfcull_eval_kernel, dim3((unsigned)(K * (size_t)a.chunks)), dim3(kKcBlock), 0, ctx->stream, a);
  hipLaunchKernelGGL(kfcull_walk_kernel, dim3(1), dim3(kKcWalkBlock), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  *n_reeval = b.down(b.hdr)[0];
  const int32_t *h_verdict = b.down(b.verdict), *h_gone_out = b.down(b.gone);
  for (size_t k = 0; k < K; k++) verdict[k] = (uint8_t)h_verdict[k];
  b.get(b.n_mps, n_mps); b.get(b.n_red, n_red);
  for (size_t p = 0; p < P; p++) pt_gone[p] = (uint8_t)h_gone_out[p];
  b.get(b.nobs, pt_nobs_out);
  return CCM_OK;
}
