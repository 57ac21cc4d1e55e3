// bowsearch.hip — ORBmatcher::SearchByBoW(pKF1, pKF2, ...) (cslam/src/ORBmatcher.cpp:565-698) of ComputeSim3 for all candidates on keyframes of the keyframe store:
// ccm_bow_pair_eval_resident (include/ccm_hip.h).  The descriptors and the feature vectors are the store's (kfstore.hip, ccm_kfstore_set_featvec);
// the call uploads the slot pairs, the offsets and the mask bytes, launches ONE kernel and downloads the table and the counters (stage_blocks.h
// BowPairResidentBlock).  The lines are bow_search_math.h's.
//
// One wave per (job, node of keyframe 1); a workgroup is four waves that share nothing.  The wave finds its job by a search over the jobs' first work items and its
// node in keyframe 2's ascending node list by a binary search: both read wave-uniform addresses, so they run on the scalar unit.  A node that keyframe 2 does not
// have ends the wave: its features stay at the zero word the upload carries.  Otherwise the wave takes its keyframe-1 segment 64 queries at a time (lane t keeps query
// t's feature index, live byte and running result) and, per chunk, keyframe 2's segment 64 candidates at a time: lane t loads candidate t's descriptor with two
// 16-byte loads and keeps it in registers while the wave walks the chunk's live queries.  A query's descriptor is wave-uniform (its index comes out of the holding
// lane by a lane read), so its eight words arrive through the scalar cache and the distance is 8 x (xor with a scalar operand + bit count), hamming.hip's inner step.
// The pass's best and second best are two butterfly minima (row swaps and DPP moves, no LDS) of the key (distance << 16 | list position), the second over the
// keys without the winner (keys are unique: the position bits); the holding lane merges them behind what the earlier passes left (bsm_merge: strict '<', so the
// first position keeps the index).
// After the last pass every lane writes its query's word: each word is written once, by one lane, and no atomic touches the table.  The counters take one integer
// atomic add per wave.  Every loop is bounded by a count the host validated (set_featvec's rules, the mask lengths).
#include "kfstore.h"
#include "lane_xor.h"
#include "stage_blocks.h"

#include <chrono>

namespace {

constexpr int kWave = 64, kBowThreads = 256, kBowWaves = kBowThreads / kWave;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

struct BowArgs {
  int W, J, stride;                 // work items, jobs, the store's slot stride
  const int32_t* job;               // BSM_JOB_INTS per job
  const uint8_t *live1, *live2;
  const int32_t *fv_node, *fv_off;  // the store's
  const uint16_t* fv_idx;
  const uint8_t* desc;
  uint64_t* table;
  uint32_t *n_query, *n_dist;
};

using lanex::wave_min_u32;   // the butterfly minimum without the LDS pipe (lane_xor.h); every lane of the wave must be active

__global__ __launch_bounds__(kBowThreads) void bow_pair_kernel(BowArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kBowWaves + (threadIdx.x >> 6)));
  if (w >= a.W) return;   // the last workgroup's idle waves; nothing below waits on another wave
  // the job: the last one whose first work item is <= w (a job without nodes shares its first item with the next one and is never met)
  int j = 0;
  for (int hi = a.J - 1; j < hi;) {
    const int mid = (j + hi + 1) >> 1;
    if (a.job[BSM_JOB_INTS * mid + 6] <= w) j = mid; else hi = mid - 1;
  }
  const int32_t* job = a.job + BSM_JOB_INTS * j;
  const int s1 = job[0], s2 = job[1], nn2 = job[3], na = w - job[6];
  const size_t g1 = (size_t)s1 * (size_t)a.stride, g2 = (size_t)s2 * (size_t)a.stride;
  const int nb = bsm_find_node(a.fv_node + g2, nn2, a.fv_node[g1 + na]);
  if (nb < 0) return;
  const int32_t* off1 = a.fv_off + g1 + s1;   // a slot's offsets: stride + 1 entries
  const int32_t* off2 = a.fv_off + g2 + s2;
  const int q0 = off1[na], q1 = off1[na + 1], c0 = off2[nb], c1 = off2[nb + 1];
  const uint16_t* idx1 = a.fv_idx + g1;
  const uint16_t* idx2 = a.fv_idx + g2;
  const uint8_t* live1 = a.live1 + job[4];
  const uint8_t* live2 = a.live2 + job[5];
  const uint32_t* desc1 = reinterpret_cast<const uint32_t*>(a.desc + 32 * g1);
  const uint8_t* desc2 = a.desc + 32 * g2;
  uint64_t* table = a.table + job[4];
  uint32_t n_live1 = 0, n_live2 = 0;
  for (int qb = q0; qb < q1; qb += kWave) {
    int my_idx1 = 0;
    bool my_live = false;
    if (qb + lane < q1) { my_idx1 = idx1[qb + lane]; my_live = live1[my_idx1] != 0; }
    const unsigned long long queries = __ballot(my_live);
    n_live1 += (uint32_t)__popcll(queries);
    BowBest part = bsm_empty();
    uint32_t cands = 0;
    for (int cb = c0; cb < c1; cb += kWave) {
      int my_idx2 = 0;
      bool c_live = false;
      if (cb + lane < c1) { my_idx2 = idx2[cb + lane]; c_live = live2[my_idx2] != 0; }
      uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
      if (c_live) {
        const uint4* tp = reinterpret_cast<const uint4*>(desc2 + 32 * (size_t)my_idx2);
        lo = tp[0]; hi = tp[1];
      }
      const unsigned long long cmask = __ballot(c_live);
      cands += (uint32_t)__popcll(cmask);
      if (!cmask) continue;   // wave-uniform: a pass without a live candidate leaves every result as it is
      const uint32_t pos = (uint32_t)(cb - c0 + lane);
      for (unsigned long long m = queries; m; m &= m - 1) {
        const int q = __ffsll((long long)m) - 1;
        const uint32_t* qp = desc1 + 8 * (size_t)__builtin_amdgcn_readlane(my_idx1, q);   // wave-uniform: the scalar path
        uint32_t key = kNoKey;
        if (c_live) {
          const int d = __builtin_popcount(qp[0] ^ lo.x) + __builtin_popcount(qp[1] ^ lo.y) + __builtin_popcount(qp[2] ^ lo.z) + __builtin_popcount(qp[3] ^ lo.w) +
                        __builtin_popcount(qp[4] ^ hi.x) + __builtin_popcount(qp[5] ^ hi.y) + __builtin_popcount(qp[6] ^ hi.z) + __builtin_popcount(qp[7] ^ hi.w);
          key = (uint32_t)d << 16 | pos;
        }
        const uint32_t m1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_min_u32(key));   // below kNoKey: the pass has a live candidate
        const uint32_t m2 = wave_min_u32(key == m1 ? kNoKey : key);
        BowBest r;
        r.d1 = (int)(m1 >> 16);
        r.d2 = m2 == kNoKey ? BSM_NONE : (int)(m2 >> 16);
        // a candidate at distance 256 is no best candidate (:631 is a strict '<' against 256)
        r.idx = r.d1 < BSM_NONE ? __builtin_amdgcn_readlane(my_idx2, (int)(m1 & 0xFFFFu) - (cb - c0)) : -1;
        if (lane == q) part = bsm_merge(part, r);
      }
    }
    n_live2 = cands;   // the same for every chunk of queries
    if (my_live) table[my_idx1] = bsm_pack(cands ? BSM_EVALUATED : BSM_NO_CANDIDATE, part, nb);
  }
  if (lane == 0 && n_live1) {
    atomicAdd(a.n_query + j, n_live1);
    if (n_live2) atomicAdd(a.n_dist + j, n_live1 * n_live2);
  }
}

typedef std::chrono::steady_clock Clock;
double us_between(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); }

#define BOW_REFUSE(why) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + (why))

}  // namespace

extern "C" int ccm_bow_pair_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int J, const int64_t* key1, const int64_t* key2, const int32_t* live1_off, const uint8_t* live1,
                                          const int32_t* live2_off, const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_bow_pair_eval_resident: ";
  if (!st) BOW_REFUSE("NULL store");
  if (st->device != ctx->device) BOW_REFUSE("the context is on another device than the store");
  if (J < 0) BOW_REFUSE("J negative");
  if (J == 0) return CCM_OK;
  if (!key1 || !key2 || !live1_off || !live2_off || !n_query || !n_dist) BOW_REFUSE("null pointers");
  std::shared_lock<std::shared_mutex> lk(st->mu);   // from the key lookup to the end of the download: no slot read here is reused or rewritten meanwhile
  std::vector<int32_t> slot1((size_t)J), slot2((size_t)J), n1((size_t)J), n2((size_t)J);
  int64_t W = 0;
  for (int j = 0; j < J; j++) {
    auto i1 = st->live.find(key1[j]), i2 = st->live.find(key2[j]);
    if (i1 == st->live.end() || i2 == st->live.end()) BOW_REFUSE("a key is not in the store");
    slot1[j] = i1->second; slot2[j] = i2->second;
    if (st->h_fv_nn[(size_t)slot1[j]] < 0 || st->h_fv_nn[(size_t)slot2[j]] < 0) BOW_REFUSE("a key without a feature vector");
    n1[j] = st->h_n[(size_t)slot1[j]]; n2[j] = st->h_n[(size_t)slot2[j]];
    W += st->h_fv_nn[(size_t)slot1[j]];
  }
  if (const char* why = bsm_check_masks(J, live1_off, live1, n1.data())) BOW_REFUSE(why);
  if (const char* why = bsm_check_masks(J, live2_off, live2, n2.data())) BOW_REFUSE(why);
  const size_t M1 = (size_t)live1_off[J], M2 = (size_t)live2_off[J];
  if (M1 > 0 && !table) BOW_REFUSE("null pointers");
  if (W > (int64_t)INT32_MAX - kBowWaves) BOW_REFUSE("too many work items");
  for (int j = 0; j < J; j++) n_query[j] = n_dist[j] = 0;
  if (M1) std::memset(table, 0, M1 * sizeof(uint64_t));
  if (W == 0) return CCM_OK;   // no keyframe 1 has a node: nothing is a query
  BowPairResidentBlock b((size_t)J, M1, M2);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  const Clock::time_point t0 = Clock::now();
  int32_t* h_job = b.up(b.job);
  int32_t item0 = 0;
  for (int j = 0; j < J; j++) {
    int32_t* r = h_job + BSM_JOB_INTS * (size_t)j;
    r[0] = slot1[j]; r[1] = slot2[j]; r[2] = st->h_fv_nn[(size_t)slot1[j]]; r[3] = st->h_fv_nn[(size_t)slot2[j]];
    r[4] = live1_off[j]; r[5] = live2_off[j]; r[6] = item0; r[7] = 0;
    item0 += r[2];
  }
  b.put(b.live1, live1); b.put(b.live2, live2);
  const Clock::time_point t1 = Clock::now();
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  BowArgs a = {};
  a.W = (int)W; a.J = J; a.stride = st->stride;
  a.job = b.dev(b.job); a.live1 = b.dev(b.live1); a.live2 = b.dev(b.live2);
  a.fv_node = st->d_fv_node; a.fv_off = st->d_fv_off; a.fv_idx = st->d_fv_idx; a.desc = st->d_desc;
  a.table = b.dev(b.table); a.n_query = (uint32_t*)b.dev(b.n_query); a.n_dist = (uint32_t*)b.dev(b.n_dist);
  hipLaunchKernelGGL(bow_pair_kernel, dim3((unsigned)((W + kBowWaves - 1) / kBowWaves)), dim3(kBowThreads), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  const Clock::time_point t2 = Clock::now();
  b.get(b.table, table); b.get(b.n_query, n_query); b.get(b.n_dist, n_dist);
  if (ccm_dbg("bow"))   // scripts/bow_search_profile.py reads this line
    fprintf(stderr, "[bow_pair] J=%d W=%lld pack_us=%.1f device_us=%.1f unpack_us=%.1f up_bytes=%zu down_bytes=%zu\n", J, (long long)W, us_between(t0, t1),
            us_between(t1, t2), us_between(t2, Clock::now()), b.up_bytes(), b.down_bytes());
  return CCM_OK;
}
