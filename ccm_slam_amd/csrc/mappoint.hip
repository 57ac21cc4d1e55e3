// mappoint.hip — MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) for a batch of map points
// whose observers are keyframes of the keyframe store: ccm_mappoint_refresh_resident (include/ccm_hip.h).  Descriptors and octaves are the store's; the
// call uploads one row index per observation, the observers' centre indices, the centres, the positions and the seeded outputs, launches ONE kernel and downloads the
// winners, their descriptors, the three values and one status byte per point (stage_blocks.h MapPointRefreshBlock).  The lines are mappoint_math.h's.
//
// The stage sorts the points into four size classes while it validates, and a workgroup of four waves works on one class:
//   N <= 8, <= 16, <= 32   a group of 8, 16 or 32 lanes per point, so a wave carries 8, 4 or 2 points.  Lane i of a group owns observation i: it loads its descriptor
//                          in place (two 16-byte loads), meets the group's descriptors one after the other (the row index comes from the owning lane, the 32 bytes
//                          from the cache) and keeps its row of distances in registers, indexed by unrolled constants only.  The median is mpm_select on compares over
//                          those registers; the winner is one butterfly minimum of mpm_key inside the group (DPP moves, one row swap for 32 lanes).
//   33 .. 256              the whole workgroup on one point.  Lane t keeps the descriptors of the COLUMNS t, t + 64, t + 128, t + 192; wave w takes the ROWS w, w + 4, ...
//                          A row's descriptor is wave-uniform and arrives through the scalar cache; its four distances per lane are counted by ballots, so the bisection
//                          runs on scalars.  The four waves' best keys meet in 16 bytes of LDS, the only LDS of the kernel.
// No lane keeps an array it indexes dynamically, nothing is sized by the cap of 256, and there is no scratch.
// The normal: lane i computes observer i's three products (the difference, the norm in double, the reciprocal, the products), then the sums are formed in LIST order
// from the lanes' values (a group shuffle per observer; lane reads in the whole-workgroup class), so the bits are the sequential loop's.  No float atomics.
// Every output is stored once by one lane: best_obs, status and the three values by the group's first lane, the winner's descriptor by the lane that owns it (two
// lanes of wave 0 copy it in the whole-workgroup class).  Every index is one the host validated.
#include "kfstore.h"
#include "lane_xor.h"
#include "stage_blocks.h"

#include <chrono>

namespace {

constexpr int kWave = 64, kMprThreads = 256, kMprWaves = kMprThreads / kWave;
constexpr int kMprClasses = 4;
constexpr int kMprGroup[kMprClasses - 1] = {8, 16, 32};   // lanes per point of the group classes; a point above the last one takes a workgroup

struct MprArgs {
  int blk0[kMprClasses + 1];   // the first workgroup of every class
  int pt0[kMprClasses + 1];    // the first entry of `order` of every class
  int nlevels;
  const int32_t *obs_off, *obs_row, *obs_kf, *ref_row, *ref_kf, *order;
  const float *kf_center, *pos, *sf;
  const uint8_t *desc, *oct;   // the store's
  int32_t* best_obs;
  uint8_t* best_desc;          // nullptr: not asked for
  float *normal, *dmin, *dmax;
  uint8_t* status;
};

__device__ __forceinline__ float lane_read(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__device__ __forceinline__ void load_desc(const uint8_t* desc, int row, uint32_t w[8]) {
  const uint4* dp = reinterpret_cast<const uint4*>(desc + 32 * (size_t)row);
  const uint4 lo = dp[0], hi = dp[1];
  w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}

// the minimum of a key over each group of G consecutive lanes, in every lane of the group; every lane of the wave must be active
template <int G>
__device__ __forceinline__ uint32_t group_min_u32(uint32_t v) {
  using lanex::dpp_u32;
  if constexpr (G >= 32) { const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false); v = min((uint32_t)p[0], (uint32_t)p[1]); }
  if constexpr (G >= 16) v = min(v, dpp_u32<0x128>(v));   // row_ror:8
  v = min(v, dpp_u32<0x1B>(dpp_u32<0x141>(v)));           // lane ^ 4
  v = min(v, dpp_u32<0x4E>(v));                           // lane ^ 2
  v = min(v, dpp_u32<0xB1>(v));                           // lane ^ 1
  return v;
}

// the finish of the normal / depth part by the one lane that stores it
__device__ __forceinline__ void store_normal_depth(const MprArgs& a, int p, const float P3[3], const float sum[3], int N, int oct) {
  float dmin, dmax, nrm[3];
  mpm_depth(P3, a.kf_center + 3 * (size_t)a.ref_kf[p], a.sf[oct], a.sf[a.nlevels - 1], dmin, dmax);
  mpm_mean(sum, N, nrm);
  a.normal[3 * (size_t)p] = nrm[0]; a.normal[3 * (size_t)p + 1] = nrm[1]; a.normal[3 * (size_t)p + 2] = nrm[2];
  a.dmin[p] = dmin; a.dmax[p] = dmax;
}

// A class of groups: G lanes per point, N <= G.  No lane leaves early: the shuffles and the butterfly read every lane.
template <int G>
__device__ __forceinline__ void refresh_groups(const MprArgs& a, int cls) {
  const int gl = threadIdx.x & (G - 1);
  const int li = ((int)blockIdx.x - a.blk0[cls]) * (kMprThreads / G) + (int)threadIdx.x / G;
  const bool valid = li < a.pt0[cls + 1] - a.pt0[cls];   // the last workgroup's idle groups
  int p = 0, o0 = 0, N = 0;
  if (valid) { p = a.order[a.pt0[cls] + li]; o0 = a.obs_off[p]; N = a.obs_off[p + 1] - o0; }
  const bool mine = gl < N;
  int row = 0;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mine) { row = a.obs_row[o0 + gl]; load_desc(a.desc, row, w); }
  int d[G];
#pragma unroll
  for (int j = 0; j < G; j++) d[j] = MPM_NO_DIST;
#pragma unroll
  for (int j = 0; j < G; j++) {
    if (!__ballot(j < N)) break;   // wave-uniform: no group of this wave has an observation j
    const int rj = __shfl(row, j, G);
    if (j < N) { uint32_t wj[8]; load_desc(a.desc, rj, wj); d[j] = mpm_hamming(w, wj); }
  }
  const int median = mpm_select(mpm_median_rank(N), [&](int v) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < G; j++) c += d[j] <= v;
    return c;
  });
  const int best = mpm_key_index(group_min_u32<G>(mine ? mpm_key(median, gl) : MPM_NO_KEY));
  if (valid && gl == 0) a.best_obs[p] = N ? best : -1;
  if (mine && gl == best && a.best_desc) {
    uint4* bp = reinterpret_cast<uint4*>(a.best_desc + 32 * (size_t)p);
    bp[0] = make_uint4(w[0], w[1], w[2], w[3]); bp[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
  int st = N ? MPM_DESC : 0, oct = 0;
  bool nd = false;
  const int rr = N ? a.ref_row[p] : -1;
  if (rr >= 0) { oct = a.oct[rr]; if (oct >= a.nlevels) st |= MPM_OCTAVE_BEYOND; else nd = true; }
  if (__ballot(nd)) {   // wave-uniform
    float P3[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f}, sum[3] = {0.f, 0.f, 0.f};
    if (nd) { P3[0] = a.pos[3 * (size_t)p]; P3[1] = a.pos[3 * (size_t)p + 1]; P3[2] = a.pos[3 * (size_t)p + 2]; }
    if (nd && mine) mpm_term(P3, a.kf_center + 3 * (size_t)a.obs_kf[o0 + gl], t);
#pragma unroll
    for (int j = 0; j < G; j++) {   // list order: every lane of the group forms the same sums
      if (!__ballot(nd && j < N)) break;
      const float t0 = __shfl(t[0], j, G), t1 = __shfl(t[1], j, G), t2 = __shfl(t[2], j, G);
      if (j < N) { sum[0] = sum[0] + t0; sum[1] = sum[1] + t1; sum[2] = sum[2] + t2; }
    }
    if (nd && gl == 0) { store_normal_depth(a, p, P3, sum, N, oct); st |= MPM_NORMAL_DEPTH; }
  }
  if (valid && gl == 0) a.status[p] = (uint8_t)st;
}

// The class above the groups: the workgroup on one point of 33 .. 256 observations.
__device__ __forceinline__ void refresh_point(const MprArgs& a, uint32_t* s_key) {
  constexpr int R = MPM_MAX_OBS / kWave;   // columns per lane
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int p = a.order[a.pt0[kMprClasses - 1] + ((int)blockIdx.x - a.blk0[kMprClasses - 1])];
  const int o0 = a.obs_off[p], N = a.obs_off[p + 1] - o0;
  uint32_t w[R][8];
#pragma unroll
  for (int r = 0; r < R; r++) {
#pragma unroll
    for (int k = 0; k < 8; k++) w[r][k] = 0;
    if (lane + kWave * r < N) load_desc(a.desc, a.obs_row[o0 + lane + kWave * r], w[r]);
  }
  const int rank = mpm_median_rank(N);
  uint32_t best = MPM_NO_KEY;
  for (int i = wave; i < N; i += kMprWaves) {   // wave-uniform
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a.desc + 32 * (size_t)a.obs_row[o0 + i]);
    uint32_t wi[8];
#pragma unroll
    for (int k = 0; k < 8; k++) wi[k] = q[k];
    int d[R];
#pragma unroll
    for (int r = 0; r < R; r++) d[r] = lane + kWave * r < N ? mpm_hamming(w[r], wi) : MPM_NO_DIST;
    const int median = mpm_select(rank, [&](int v) {
      int c = 0;
#pragma unroll
      for (int r = 0; r < R; r++) c += __popcll(__ballot(d[r] <= v));
      return c;
    });
    best = min(best, mpm_key(median, i));
  }
  if (lane == 0) s_key[wave] = best;
  __syncthreads();
  if (wave != 0) return;
  const int bi = mpm_key_index(min(min(s_key[0], s_key[1]), min(s_key[2], s_key[3])));
  if (lane == 0) a.best_obs[p] = bi;
  if (a.best_desc && lane < 2)
    reinterpret_cast<uint4*>(a.best_desc + 32 * (size_t)p)[lane] = reinterpret_cast<const uint4*>(a.desc + 32 * (size_t)a.obs_row[o0 + bi])[lane];
  int st = MPM_DESC;
  const int rr = a.ref_row[p];
  if (rr >= 0) {   // wave-uniform
    const int oct = a.oct[rr];
    if (oct >= a.nlevels) st |= MPM_OCTAVE_BEYOND;
    else {
      const float P3[3] = {a.pos[3 * (size_t)p], a.pos[3 * (size_t)p + 1], a.pos[3 * (size_t)p + 2]};
      float sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < R; r++) {
        float t[3] = {0.f, 0.f, 0.f};
        if (lane + kWave * r < N) mpm_term(P3, a.kf_center + 3 * (size_t)a.obs_kf[o0 + lane + kWave * r], t);
        const int n_r = min(kWave, N - kWave * r);
        for (int j = 0; j < n_r; j++) {   // list order
          sum[0] = sum[0] + lane_read(t[0], j); sum[1] = sum[1] + lane_read(t[1], j); sum[2] = sum[2] + lane_read(t[2], j);
        }
      }
      if (lane == 0) store_normal_depth(a, p, P3, sum, N, oct);
      st |= MPM_NORMAL_DEPTH;
    }
  }
  if (lane == 0) a.status[p] = (uint8_t)st;
}

__global__ __launch_bounds__(kMprThreads) void mappoint_refresh_kernel(MprArgs a) {
  __shared__ uint32_t s_key[kMprWaves];
  const int b = blockIdx.x;   // the class is the workgroup's
  if (b < a.blk0[1]) refresh_groups<kMprGroup[0]>(a, 0);
  else if (b < a.blk0[2]) refresh_groups<kMprGroup[1]>(a, 1);
  else if (b < a.blk0[3]) refresh_groups<kMprGroup[2]>(a, 2);
  else refresh_point(a, s_key);
}

int mpr_class(int N) {
  for (int c = 0; c < kMprClasses - 1; c++)
    if (N <= kMprGroup[c]) return c;
  return kMprClasses - 1;
}

typedef std::chrono::steady_clock Clock;
double us_between(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); }

#define MPR_REFUSE(why) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + (why))

}  // namespace

extern "C" int ccm_mappoint_refresh_resident(ccm_ctx* ctx, ccm_kfstore* st, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off,
                                             const int32_t* obs_kf, const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels,
                                             const float* scale_factors, int32_t* best_obs, uint8_t* best_desc, float* normal, float* min_dist, float* max_dist,
                                             uint8_t* status) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_mappoint_refresh_resident: ";
  if (!st) MPR_REFUSE("NULL store");
  if (st->device != ctx->device) MPR_REFUSE("the context is on another device than the store");
  bool nd = false;
  if (const char* why = mpm_check_args(K, keys, kf_center, P, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, nlevels, scale_factors, best_obs, normal, min_dist, max_dist,
                                       status, &nd))
    MPR_REFUSE(why);
  std::shared_lock<std::shared_mutex> lk(st->mu);   // from the key lookup to the end of the download: no slot read here is reused or rewritten meanwhile
  std::vector<int32_t> slot((size_t)K), kf_n((size_t)K);
  for (int k = 0; k < K; k++) {
    auto it = st->live.find(keys[k]);
    if (it == st->live.end()) MPR_REFUSE("a key is not in the store");
    slot[k] = it->second; kf_n[k] = st->h_n[(size_t)slot[k]];
  }
  if (const char* why = mpm_check_features(kf_n.data(), P, obs_off, obs_kf, obs_feat, ref_kf, ref_feat)) MPR_REFUSE(why);
  if (P == 0) return CCM_OK;
  if ((int64_t)st->max_kf * (int64_t)st->stride > (int64_t)INT32_MAX) MPR_REFUSE("the store has more feature rows than an int holds");
  const int M = obs_off[P];
  MapPointRefreshBlock b((size_t)K, (size_t)P, (size_t)M, (size_t)nlevels, nd, best_desc != nullptr);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  const Clock::time_point t0 = Clock::now();
  MprArgs a = {};
  // the classes: counted, then the points placed in input order inside their class
  int n_cls[kMprClasses] = {0, 0, 0, 0}, at[kMprClasses];
  for (int p = 0; p < P; p++) n_cls[mpr_class(obs_off[p + 1] - obs_off[p])]++;
  int64_t blocks = 0;
  for (int c = 0; c < kMprClasses; c++) {
    a.pt0[c + 1] = a.pt0[c] + n_cls[c];
    blocks += c < kMprClasses - 1 ? ccm_div_up(n_cls[c], kMprThreads / kMprGroup[c]) : n_cls[c];
    a.blk0[c + 1] = (int)blocks;
    at[c] = a.pt0[c];
  }
  int32_t *h_order = b.up(b.order), *h_row = b.up(b.obs_row), *h_ref = b.up(b.ref_row);
  for (int p = 0; p < P; p++) {
    h_order[at[mpr_class(obs_off[p + 1] - obs_off[p])]++] = p;
    h_ref[p] = ref_kf[p] < 0 ? -1 : slot[ref_kf[p]] * st->stride + ref_feat[p];
  }
  for (int o = 0; o < M; o++) h_row[o] = slot[obs_kf[o]] * st->stride + obs_feat[o];
  b.put(b.kf_center, kf_center); b.put(b.obs_off, obs_off); b.put(b.obs_kf, obs_kf); b.put(b.pos, pos); b.put(b.ref_kf, ref_kf); b.put(b.scale_factors, scale_factors);
  b.put(b.normal, normal); b.put(b.dmin, min_dist); b.put(b.dmax, max_dist);   // a point whose normal / depth part does not run keeps the caller's values
  const Clock::time_point t1 = Clock::now();
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  a.nlevels = nlevels;
  a.obs_off = b.dev(b.obs_off); a.obs_row = b.dev(b.obs_row); a.obs_kf = b.dev(b.obs_kf); a.ref_row = b.dev(b.ref_row); a.ref_kf = b.dev(b.ref_kf); a.order = b.dev(b.order);
  a.kf_center = b.dev(b.kf_center); a.pos = b.dev(b.pos); a.sf = b.dev(b.scale_factors);
  a.desc = st->d_desc; a.oct = st->d_oct;
  a.best_obs = b.dev(b.best_obs); a.best_desc = best_desc ? b.dev(b.best_desc) : nullptr;
  a.normal = b.dev(b.normal); a.dmin = b.dev(b.dmin); a.dmax = b.dev(b.dmax); a.status = b.dev(b.status);
  hipLaunchKernelGGL(mappoint_refresh_kernel, dim3((unsigned)blocks), dim3(kMprThreads), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  const Clock::time_point t2 = Clock::now();
  b.get(b.best_obs, best_obs); b.get(b.status, status);
  b.get(b.normal, normal); b.get(b.dmin, min_dist); b.get(b.dmax, max_dist);
  if (best_desc) {   // a point without observations has no winner: its row of the caller's array stays
    const uint8_t* h_desc = b.down(b.best_desc);
    for (int p = 0; p < P; p++)
      if (obs_off[p + 1] > obs_off[p]) memcpy(best_desc + 32 * (size_t)p, h_desc + 32 * (size_t)p, 32);
  }
  if (ccm_dbg("mappoint"))   // scripts/mappoint_refresh_profile.py reads this line
    fprintf(stderr, "[mappoint_refresh] P=%d M=%d blocks=%lld pack_us=%.1f device_us=%.1f unpack_us=%.1f up_bytes=%zu down_bytes=%zu\n", P, M, (long long)blocks,
            us_between(t0, t1), us_between(t1, t2), us_between(t2, Clock::now()), b.up_bytes(), b.down_bytes());
  return CCM_OK;
}
