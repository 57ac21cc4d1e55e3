// fv_pair.h — what the searches over the common vocabulary nodes of two keyframes of the keyframe store share: the wave's walk of bow_pair_kernel
// (bowsearch.hip) and tri_search_kernel (trisearch.hip), written once over a form, and the host stage of their two entry points, written once over the block type.
//
// The walk.  One wave per (job, node of keyframe 1); a workgroup is four waves that share nothing.  The wave finds its job by a search over the jobs' first work items
// and its node in keyframe 2's ascending node list by a binary search: both read wave-uniform addresses, so they run on the scalar unit.  A node that keyframe 2 does not
// have ends the wave: its features stay at the zero word the upload carries.  Otherwise the wave takes its keyframe-1 segment 64 queries at a time (lane t keeps query
// t's feature index, the form's per-query state and the running result) and, per chunk, keyframe 2's segment 64 candidates at a time: lane t keeps candidate t's
// per-candidate state and, where the form can use the candidate, its descriptor (two 16-byte loads) in registers while the wave walks the chunk's queries.  A query's
// descriptor is wave-uniform (its index comes out of the holding lane by a lane read), so its eight words arrive through the scalar cache and the distance is
// 8 x (xor with a scalar operand + bit count), hamming.hip's inner step; the form turns the distance into a key (the no-key value where it rejects the pair) and
// reduces the wave's keys to the pass's result by butterfly minima (lane_xor.h: row swaps and DPP moves, no LDS), which the holding lane merges behind what the
// earlier passes left.  After the last pass every lane writes its query's word: each word is written once, by one lane, and no atomic touches the table.  The counters
// take one integer atomic add per wave each.  Every loop is bounded by a count the host validated (set_featvec's rules, the mask lengths).  With more than 64 queries
// AND more than 64 candidates in a node the candidate passes are loaded again per query chunk.
//
// A form F supplies (every member inlines away; the kernels' registers are those of the two hand-written bodies):
//   Args, Best, Query, Cand                    the kernel's arguments (FvPairArgs<Word> or more), the running result, the per-query and per-candidate lane state
//   F(a, job, g1, g2)                          the wave's own pointers and counters
//   is_query(byte of side 1), is_counted(byte of side 2)
//   query(is it one, idx1) -> Query            by the holding lane, once per chunk
//   lane_read(Query, q) -> Query               the wave's copy of lane q's
//   candidate(is it counted, idx2, &Cand)      -> is it usable; once per pass: what does not depend on the query
//   key(d, pos, Query, Cand) -> uint32_t       of a usable candidate at list position pos; kNoKey where the form rejects the pair
//   empty() -> Best
//   reduce(key, my_idx2, pos0, holds, &Best)   every lane active: the pass's result from the wave's keys, merged behind the running result where `holds`
//   word(is it a query, Best, counted, nb)     -> Word; called by every lane (it may ballot)
//   add_counters(a, j)                         by lane 0 of a wave with a query, between n_query and n_dist
#pragma once
#include "kfstore.h"
#include "lane_xor.h"
#include "stage_blocks.h"

#include <chrono>

namespace fvp {

constexpr int kWave = 64, kThreads = 256, kWaves = kThreads / kWave;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

template <class Word>
struct FvPairArgs {
  int W, J, stride;                 // work items, jobs, the store's slot stride
  const int32_t* job;               // BSM_JOB_INTS per job
  const uint8_t *mask1, *mask2;
  const int32_t *fv_node, *fv_off;  // the store's
  const uint16_t* fv_idx;
  const uint8_t* desc;
  Word* table;
  uint32_t *n_query, *n_dist;
};

template <class F>
__device__ __forceinline__ void fv_pair_wave(const typename F::Args& a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + (threadIdx.x >> 6)));
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
  const uint8_t* mask1 = a.mask1 + job[4];
  const uint8_t* mask2 = a.mask2 + job[5];
  const uint32_t* desc1 = reinterpret_cast<const uint32_t*>(a.desc + 32 * g1);
  const uint8_t* desc2 = a.desc + 32 * g2;
  auto* table = a.table + job[4];
  F f(a, job, g1, g2);
  uint32_t n_q = 0, n_c = 0;
  for (int qb = q0; qb < q1; qb += kWave) {
    int my_idx1 = 0;
    bool my_query = false;
    if (qb + lane < q1) { my_idx1 = idx1[qb + lane]; my_query = F::is_query(mask1[my_idx1]); }
    const unsigned long long queries = __ballot(my_query);
    n_q += (uint32_t)__popcll(queries);
    const typename F::Query my_q = f.query(my_query, my_idx1);
    typename F::Best part = F::empty();
    uint32_t cands = 0;
    for (int cb = c0; cb < c1; cb += kWave) {
      int my_idx2 = 0;
      bool counted = false;
      if (cb + lane < c1) { my_idx2 = idx2[cb + lane]; counted = F::is_counted(mask2[my_idx2]); }
      typename F::Cand c;
      const bool usable = f.candidate(counted, my_idx2, c);
      uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
      if (usable) {
        const uint4* tp = reinterpret_cast<const uint4*>(desc2 + 32 * (size_t)my_idx2);
        lo = tp[0]; hi = tp[1];
      }
      cands += (uint32_t)__popcll(__ballot(counted));
      if (!__ballot(usable)) continue;   // wave-uniform: a pass without a usable candidate leaves every result as it is
      const uint32_t pos = (uint32_t)(cb - c0 + lane);
      for (unsigned long long m = queries; m; m &= m - 1) {
        const int q = __ffsll((long long)m) - 1;
        const uint32_t* qp = desc1 + 8 * (size_t)__builtin_amdgcn_readlane(my_idx1, q);   // wave-uniform: the scalar path
        const typename F::Query uq = F::lane_read(my_q, q);
        uint32_t key = kNoKey;
        if (usable) {
          const int d = __builtin_popcount(qp[0] ^ lo.x) + __builtin_popcount(qp[1] ^ lo.y) + __builtin_popcount(qp[2] ^ lo.z) + __builtin_popcount(qp[3] ^ lo.w) +
                        __builtin_popcount(qp[4] ^ hi.x) + __builtin_popcount(qp[5] ^ hi.y) + __builtin_popcount(qp[6] ^ hi.z) + __builtin_popcount(qp[7] ^ hi.w);
          key = F::key(d, pos, uq, c);
        }
        F::reduce(key, my_idx2, cb - c0, lane == q, part);
      }
    }
    n_c = cands;   // the same for every chunk of queries
    const auto word = f.word(my_query, part, cands, nb);
    if (my_query) table[my_idx1] = word;
  }
  if (lane == 0 && n_q) {
    atomicAdd(a.n_query + j, n_q);
    f.add_counters(a, j);
    if (n_c) atomicAdd(a.n_dist + j, n_q * n_c);
  }
}

typedef std::chrono::steady_clock Clock;
inline double us_between(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); }

// What the two entry points receive alike, and what names the form: its refusals' prefix, its CCM_DBG topic and line tag, its own two refusals (nullptr, or what is
// wrong) in the place they take among the shared ones, the block's two mask segments and, where the form has a third counter, that one.
template <class Block>
struct FvPairCall {
  const char *me, *topic, *tag;
  const char* scalar_why;   // reported behind "J negative", before J == 0 returns
  const char* limit_why;    // reported behind "too many work items"
  int J;
  const int64_t *key1, *key2;
  const int32_t* off1; const uint8_t* mask1; StagedSeg<uint8_t> Block::*seg1;
  const int32_t* off2; const uint8_t* mask2; StagedSeg<uint8_t> Block::*seg2;
  void* table;              // one word of the block's table per mask byte of side 1
  int32_t *n_query, *n_dist;
  int32_t* n_match; StagedSeg<int32_t> Block::*seg_match;   // seg_match == nullptr: the form has none
};

// One call: the checks in the entries' order, the store's reader lock from the key lookup to the end of the download, the outputs zeroed and nothing launched where no
// keyframe 1 has a node; otherwise begin, the job records (r[7] = job_word7 * j: the job's first float, 0 where the form has none), pack (the form's own segments),
// upload, the shared kernel arguments and fill (the form's), one wave per work item, download, the caller's outputs and the CCM_DBG line.  extra: what the block's
// constructor takes behind (J, M1, M2).
template <class Block, class Args, class Pack, class Fill, class... Extra>
int fv_pair_stage(ccm_ctx* ctx, ccm_kfstore* st, const FvPairCall<Block>& c, void (*kernel)(Args), int job_word7, Pack pack, Fill fill, Extra... extra) {
#define FVP_REFUSE(why) return ccm_set_error(ctx, CCM_E_ARG, std::string(c.me) + (why))
  const int J = c.J;
  if (!st) FVP_REFUSE("NULL store");
  if (st->device != ctx->device) FVP_REFUSE("the context is on another device than the store");
  if (J < 0) FVP_REFUSE("J negative");
  if (c.scalar_why) FVP_REFUSE(c.scalar_why);
  if (J == 0) return CCM_OK;
  if (!c.key1 || !c.key2 || !c.off1 || !c.off2 || !c.n_query || (c.seg_match && !c.n_match) || !c.n_dist) FVP_REFUSE("null pointers");
  std::shared_lock<std::shared_mutex> lk(st->mu);   // from the key lookup to the end of the download: no slot read here is reused or rewritten meanwhile
  std::vector<int32_t> slot1((size_t)J), slot2((size_t)J), n1((size_t)J), n2((size_t)J);
  int64_t W = 0;
  for (int j = 0; j < J; j++) {
    auto i1 = st->live.find(c.key1[j]), i2 = st->live.find(c.key2[j]);
    if (i1 == st->live.end() || i2 == st->live.end()) FVP_REFUSE("a key is not in the store");
    slot1[j] = i1->second; slot2[j] = i2->second;
    if (st->h_fv_nn[(size_t)slot1[j]] < 0 || st->h_fv_nn[(size_t)slot2[j]] < 0) FVP_REFUSE("a key without a feature vector");
    n1[j] = st->h_n[(size_t)slot1[j]]; n2[j] = st->h_n[(size_t)slot2[j]];
    W += st->h_fv_nn[(size_t)slot1[j]];
  }
  if (const char* why = bsm_check_masks(J, c.off1, c.mask1, n1.data())) FVP_REFUSE(why);
  if (const char* why = bsm_check_masks(J, c.off2, c.mask2, n2.data())) FVP_REFUSE(why);
  const size_t M1 = (size_t)c.off1[J], M2 = (size_t)c.off2[J];
  if (M1 > 0 && !c.table) FVP_REFUSE("null pointers");
  if (W > (int64_t)INT32_MAX - kWaves) FVP_REFUSE("too many work items");
  if (c.limit_why) FVP_REFUSE(c.limit_why);
#undef FVP_REFUSE
  for (int j = 0; j < J; j++) {
    c.n_query[j] = c.n_dist[j] = 0;
    if (c.seg_match) c.n_match[j] = 0;
  }
  if (M1) std::memset(c.table, 0, M1 * sizeof(*Args().table));
  if (W == 0) return CCM_OK;   // no keyframe 1 has a node: nothing is a query
  Block b((size_t)J, M1, M2, extra...);
  if (int rc = ccm_staged_begin(ctx, b, c.me)) return rc;
  const Clock::time_point t0 = Clock::now();
  int32_t* h_job = b.up(b.job);
  int32_t item0 = 0;
  for (int j = 0; j < J; j++) {
    int32_t* r = h_job + BSM_JOB_INTS * (size_t)j;
    r[0] = slot1[j]; r[1] = slot2[j]; r[2] = st->h_fv_nn[(size_t)slot1[j]]; r[3] = st->h_fv_nn[(size_t)slot2[j]];
    r[4] = c.off1[j]; r[5] = c.off2[j]; r[6] = item0; r[7] = job_word7 * j;
    item0 += r[2];
  }
  b.put(b.*c.seg1, c.mask1); b.put(b.*c.seg2, c.mask2);
  pack(b);
  const Clock::time_point t1 = Clock::now();
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  Args a = {};
  a.W = (int)W; a.J = J; a.stride = st->stride;
  a.job = b.dev(b.job); a.mask1 = b.dev(b.*c.seg1); a.mask2 = b.dev(b.*c.seg2);
  a.fv_node = st->d_fv_node; a.fv_off = st->d_fv_off; a.fv_idx = st->d_fv_idx; a.desc = st->d_desc;
  a.table = b.dev(b.table); a.n_query = (uint32_t*)b.dev(b.n_query); a.n_dist = (uint32_t*)b.dev(b.n_dist);
  fill(b, a);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((W + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  const Clock::time_point t2 = Clock::now();
  b.get(b.table, c.table); b.get(b.n_query, c.n_query);
  if (c.seg_match) b.get(b.*c.seg_match, c.n_match);
  b.get(b.n_dist, c.n_dist);
  if (ccm_dbg(c.topic))   // scripts/bow_search_profile.py and tri_search_profile.py read this line
    fprintf(stderr, "[%s] J=%d W=%lld pack_us=%.1f device_us=%.1f unpack_us=%.1f up_bytes=%zu down_bytes=%zu\n", c.tag, J, (long long)W, us_between(t0, t1),
            us_between(t1, t2), us_between(t2, Clock::now()), b.up_bytes(), b.down_bytes());
  return CCM_OK;
}

}  // namespace fvp
