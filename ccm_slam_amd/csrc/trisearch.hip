// trisearch.hip — ORBmatcher::SearchForTriangulation (cslam/src/ORBmatcher.cpp:700-852) of LocalMapping::CreateNewMapPoints for all neighbours on keyframes of the
// keyframe store: ccm_tri_search_eval_resident (include/ccm_hip.h).  Descriptors, mvKeysUn, octaves and feature vectors are the store's; the call uploads
// the slot pairs, the offsets, 11 floats per job, the level tables and the map-point bytes, launches ONE kernel and downloads one 32-bit word per feature of every
// job's keyframe 1 and three counters per job (stage_blocks.h TriSearchResidentBlock).  The lines are tri_search_math.h's.
//
// The mapping is bowsearch.hip's: one wave per (job, node of keyframe 1), four waves per workgroup that share nothing; the job by a search over the jobs' first work
// items and the node of keyframe 2 by a binary search, both on wave-uniform addresses.  The wave takes its keyframe-1 segment 64 queries at a time: lane t keeps query
// t's feature index, its epipolar line (a, b, c, den of :162-168, computed once) and its running result.  Per chunk it takes keyframe 2's segment 64 candidates at a
// time: lane t loads candidate t's map-point byte, octave, keypoint, line threshold and descriptor (two 16-byte loads) and evaluates the epipole gate, which does not
// depend on the query, once per pass.  A query's descriptor is wave-uniform and arrives through the scalar cache; its line reaches the wave by four lane reads.  The
// line gate (one correctly rounded f32 division, one comparison in double) runs only in lanes whose distance is at most TH_LOW.  The pass's winner is ONE butterfly
// minimum of the key (distance << 16 | 0xFFFF - list position): the smallest distance, and among equals the LARGEST position, as :770's `dist > bestDist` leaves
// it; a lane whose candidate fails any test holds the no-key value.  The holding lane merges with '<=' (tsm_merge), so a later pass wins ties.
// After the last pass every lane writes its query's word: each word is written once, by one lane; no atomic touches the table and there is no LDS.  The counters take
// one integer atomic add per wave each.  Every loop is bounded by a count the host validated (set_featvec's rules, the mask lengths).
#include "kfstore.h"
#include "lane_xor.h"
#include "stage_blocks.h"

#include <chrono>

namespace {

constexpr int kWave = 64, kTriThreads = 256, kTriWaves = kTriThreads / kWave;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

struct TriArgs {
  int W, J, stride, nlevels;        // work items, jobs, the store's slot stride, the levels of the two tables
  const int32_t* job;               // TSM_JOB_INTS per job
  const float *epi, *sf;            // TSM_EPI_FLOATS per job; scale_factors[nlevels]
  const double* thr;                // 3.84 * (double)level_sigma2[l]
  const uint8_t *has1, *has2;
  const int32_t *fv_node, *fv_off;  // the store's
  const uint16_t* fv_idx;
  const uint8_t *desc, *oct;
  const float* xy;
  uint32_t* table;
  uint32_t *n_query, *n_match, *n_dist;
};

__device__ __forceinline__ float lane_read(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(kTriThreads) void tri_search_kernel(TriArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTriWaves + (threadIdx.x >> 6)));
  if (w >= a.W) return;   // the last workgroup's idle waves; nothing below waits on another wave
  // the job: the last one whose first work item is <= w (a job without nodes shares its first item with the next one and is never met)
  int j = 0;
  for (int hi = a.J - 1; j < hi;) {
    const int mid = (j + hi + 1) >> 1;
    if (a.job[TSM_JOB_INTS * mid + 6] <= w) j = mid; else hi = mid - 1;
  }
  const int32_t* job = a.job + TSM_JOB_INTS * j;
  const int s1 = job[0], s2 = job[1], nn2 = job[3], na = w - job[6];
  const size_t g1 = (size_t)s1 * (size_t)a.stride, g2 = (size_t)s2 * (size_t)a.stride;
  const int nb = bsm_find_node(a.fv_node + g2, nn2, a.fv_node[g1 + na]);
  if (nb < 0) return;
  const int32_t* off1 = a.fv_off + g1 + s1;   // a slot's offsets: stride + 1 entries
  const int32_t* off2 = a.fv_off + g2 + s2;
  const int q0 = off1[na], q1 = off1[na + 1], c0 = off2[nb], c1 = off2[nb + 1];
  const uint16_t* idx1 = a.fv_idx + g1;
  const uint16_t* idx2 = a.fv_idx + g2;
  const uint8_t* has1 = a.has1 + job[4];
  const uint8_t* has2 = a.has2 + job[5];
  const float* epi = a.epi + job[7];
  const float ex = epi[9], ey = epi[10];
  const uint32_t* desc1 = reinterpret_cast<const uint32_t*>(a.desc + 32 * g1);
  const uint8_t* desc2 = a.desc + 32 * g2;
  const float2* xy1 = reinterpret_cast<const float2*>(a.xy + 2 * g1);
  const float2* xy2 = reinterpret_cast<const float2*>(a.xy + 2 * g2);
  const uint8_t* oct2 = a.oct + g2;
  uint32_t* table = a.table + job[4];
  uint32_t n_q = 0, n_m = 0, n_free2 = 0;
  for (int qb = q0; qb < q1; qb += kWave) {
    int my_idx1 = 0;
    bool my_query = false;
    if (qb + lane < q1) { my_idx1 = idx1[qb + lane]; my_query = has1[my_idx1] == 0; }
    const unsigned long long queries = __ballot(my_query);
    n_q += (uint32_t)__popcll(queries);
    TriLine my_l = {0.0f, 0.0f, 0.0f, 0.0f};
    if (my_query) { const float2 p = xy1[my_idx1]; my_l = tsm_line(p.x, p.y, epi); }
    TriBest part = tsm_empty();
    uint32_t free2 = 0;
    for (int cb = c0; cb < c1; cb += kWave) {
      int my_idx2 = 0;
      bool c_free = false, c_ok = false;
      float x2 = 0.0f, y2 = 0.0f;
      double thr = 0.0;
      uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
      if (cb + lane < c1) { my_idx2 = idx2[cb + lane]; c_free = has2[my_idx2] == 0; }
      if (c_free) {
        const int o = oct2[my_idx2];
        if (o < a.nlevels) {   // an octave the tables do not have: no candidate, and neither table is read
          const float2 p = xy2[my_idx2];
          x2 = p.x; y2 = p.y;
          c_ok = !tsm_epipole_gate(ex, ey, x2, y2, a.sf[o]);
          thr = a.thr[o];
        }
        if (c_ok) {
          const uint4* tp = reinterpret_cast<const uint4*>(desc2 + 32 * (size_t)my_idx2);
          lo = tp[0]; hi = tp[1];
        }
      }
      free2 += (uint32_t)__popcll(__ballot(c_free));
      if (!__ballot(c_ok)) continue;   // wave-uniform: a pass without a candidate leaves every result as it is
      const uint32_t rpos = 0xFFFFu - (uint32_t)(cb - c0 + lane);
      for (unsigned long long m = queries; m; m &= m - 1) {
        const int q = __ffsll((long long)m) - 1;
        const uint32_t* qp = desc1 + 8 * (size_t)__builtin_amdgcn_readlane(my_idx1, q);   // wave-uniform: the scalar path
        const float la = lane_read(my_l.a, q), lb = lane_read(my_l.b, q), lc = lane_read(my_l.c, q), lden = lane_read(my_l.den, q);
        uint32_t key = kNoKey;
        if (c_ok) {
          const int d = __builtin_popcount(qp[0] ^ lo.x) + __builtin_popcount(qp[1] ^ lo.y) + __builtin_popcount(qp[2] ^ lo.z) + __builtin_popcount(qp[3] ^ lo.w) +
                        __builtin_popcount(qp[4] ^ hi.x) + __builtin_popcount(qp[5] ^ hi.y) + __builtin_popcount(qp[6] ^ hi.z) + __builtin_popcount(qp[7] ^ hi.w);
          if (d <= TSM_TH_LOW && tsm_line_gate_thr(la, lb, lc, lden, x2, y2, thr)) key = (uint32_t)d << 16 | rpos;
        }
        const uint32_t m1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lanex::wave_min_u32(key));   // every lane is active here
        if (m1 != kNoKey) {   // wave-uniform
          TriBest r;
          r.d = (int)(m1 >> 16);
          r.idx = __builtin_amdgcn_readlane(my_idx2, (int)(0xFFFFu - (m1 & 0xFFFFu)) - (cb - c0));
          if (lane == q) part = tsm_merge(part, r);
        }
      }
    }
    n_free2 = free2;   // the same for every chunk of queries
    const bool matched = my_query && part.idx >= 0;
    n_m += (uint32_t)__popcll(__ballot(matched));
    if (my_query) table[my_idx1] = tsm_pack(matched ? TSM_MATCHED : TSM_NO_MATCH, part);
  }
  if (lane == 0 && n_q) {
    atomicAdd(a.n_query + j, n_q);
    if (n_m) atomicAdd(a.n_match + j, n_m);
    if (n_free2) atomicAdd(a.n_dist + j, n_q * n_free2);
  }
}

typedef std::chrono::steady_clock Clock;
double us_between(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); }

#define TRI_REFUSE(why) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + (why))

}  // namespace

extern "C" int ccm_tri_search_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int J, const int64_t* key1, const int64_t* key2, const int32_t* has1_off, const uint8_t* has1,
                                            const int32_t* has2_off, const uint8_t* has2, const float* job_epi, int nlevels, const float* scale_factors,
                                            const float* level_sigma2, uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_tri_search_eval_resident: ";
  if (!st) TRI_REFUSE("NULL store");
  if (st->device != ctx->device) TRI_REFUSE("the context is on another device than the store");
  if (J < 0) TRI_REFUSE("J negative");
  if (const char* why = tsm_check_args(J, job_epi, nlevels, scale_factors, level_sigma2)) TRI_REFUSE(why);
  if (J == 0) return CCM_OK;
  if (!key1 || !key2 || !has1_off || !has2_off || !n_query || !n_match || !n_dist) TRI_REFUSE("null pointers");
  std::shared_lock<std::shared_mutex> lk(st->mu);   // from the key lookup to the end of the download: no slot read here is reused or rewritten meanwhile
  std::vector<int32_t> slot1((size_t)J), slot2((size_t)J), n1((size_t)J), n2((size_t)J);
  int64_t W = 0;
  for (int j = 0; j < J; j++) {
    auto i1 = st->live.find(key1[j]), i2 = st->live.find(key2[j]);
    if (i1 == st->live.end() || i2 == st->live.end()) TRI_REFUSE("a key is not in the store");
    slot1[j] = i1->second; slot2[j] = i2->second;
    if (st->h_fv_nn[(size_t)slot1[j]] < 0 || st->h_fv_nn[(size_t)slot2[j]] < 0) TRI_REFUSE("a key without a feature vector");
    n1[j] = st->h_n[(size_t)slot1[j]]; n2[j] = st->h_n[(size_t)slot2[j]];
    W += st->h_fv_nn[(size_t)slot1[j]];
  }
  if (const char* why = bsm_check_masks(J, has1_off, has1, n1.data())) TRI_REFUSE(why);
  if (const char* why = bsm_check_masks(J, has2_off, has2, n2.data())) TRI_REFUSE(why);
  const size_t M1 = (size_t)has1_off[J], M2 = (size_t)has2_off[J];
  if (M1 > 0 && !table) TRI_REFUSE("null pointers");
  if (W > (int64_t)INT32_MAX - kTriWaves) TRI_REFUSE("too many work items");
  if ((int64_t)J * TSM_EPI_FLOATS > (int64_t)INT32_MAX) TRI_REFUSE("too many jobs");
  for (int j = 0; j < J; j++) n_query[j] = n_match[j] = n_dist[j] = 0;
  if (M1) std::memset(table, 0, M1 * sizeof(uint32_t));
  if (W == 0) return CCM_OK;   // no keyframe 1 has a node: nothing is a query
  TriSearchResidentBlock b((size_t)J, M1, M2, (size_t)nlevels);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  const Clock::time_point t0 = Clock::now();
  int32_t* h_job = b.up(b.job);
  int32_t item0 = 0;
  for (int j = 0; j < J; j++) {
    int32_t* r = h_job + TSM_JOB_INTS * (size_t)j;
    r[0] = slot1[j]; r[1] = slot2[j]; r[2] = st->h_fv_nn[(size_t)slot1[j]]; r[3] = st->h_fv_nn[(size_t)slot2[j]];
    r[4] = has1_off[j]; r[5] = has2_off[j]; r[6] = item0; r[7] = TSM_EPI_FLOATS * j;
    item0 += r[2];
  }
  double* h_thr = b.up(b.line_thr);
  for (int l = 0; l < nlevels; l++) h_thr[l] = tsm_line_thr(level_sigma2[l]);
  b.put(b.job_epi, job_epi); b.put(b.scale_factors, scale_factors);
  b.put(b.has1, has1); b.put(b.has2, has2);
  const Clock::time_point t1 = Clock::now();
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  TriArgs a = {};
  a.W = (int)W; a.J = J; a.stride = st->stride; a.nlevels = nlevels;
  a.job = b.dev(b.job); a.epi = b.dev(b.job_epi); a.sf = b.dev(b.scale_factors); a.thr = b.dev(b.line_thr);
  a.has1 = b.dev(b.has1); a.has2 = b.dev(b.has2);
  a.fv_node = st->d_fv_node; a.fv_off = st->d_fv_off; a.fv_idx = st->d_fv_idx; a.desc = st->d_desc; a.oct = st->d_oct; a.xy = st->d_xy;
  a.table = b.dev(b.table); a.n_query = (uint32_t*)b.dev(b.n_query); a.n_match = (uint32_t*)b.dev(b.n_match); a.n_dist = (uint32_t*)b.dev(b.n_dist);
  hipLaunchKernelGGL(tri_search_kernel, dim3((unsigned)((W + kTriWaves - 1) / kTriWaves)), dim3(kTriThreads), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  const Clock::time_point t2 = Clock::now();
  b.get(b.table, table); b.get(b.n_query, n_query); b.get(b.n_match, n_match); b.get(b.n_dist, n_dist);
  if (ccm_dbg("tri"))   // scripts/tri_search_profile.py reads this line
    fprintf(stderr, "[tri_search] J=%d W=%lld pack_us=%.1f device_us=%.1f unpack_us=%.1f up_bytes=%zu down_bytes=%zu\n", J, (long long)W, us_between(t0, t1),
            us_between(t1, t2), us_between(t2, Clock::now()), b.up_bytes(), b.down_bytes());
  return CCM_OK;
}
