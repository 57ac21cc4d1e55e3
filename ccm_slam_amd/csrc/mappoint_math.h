// mappoint_math.h — the lines of MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823), once, for the
// kernel of mappoint.hip and for the host: the Hamming distance, the median rule, the first-minimum key, the status bits, the normal / depth lines,
// the argument rules and the host evaluator of a whole ccm_mappoint_refresh_resident call.  The f32 expressions keep the reference's operand order; compile with
// -ffp-contract=off (a product and a sum are two roundings).  The normal / depth lines restate sim3_correct_math.h's s3c_normal_depth operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define MPM_HD __host__ __device__ inline
#else
#define MPM_HD static inline
#endif

#define MPM_MAX_OBS 256       // observations per point: ccm_distinctive_descriptors' limit
#define MPM_MAX_LEVELS 256    // an octave is one byte
#define MPM_NO_DIST 0x200     // above every distance (0 .. 256): an entry that is no observation is never counted
#define MPM_NO_KEY 0xFFFFFFFFu
// status[p]
enum { MPM_DESC = 1,          // the descriptor part ran: best_obs[p] >= 0
       MPM_NORMAL_DEPTH = 2,  // normal, min_dist and max_dist were written
       MPM_OCTAVE_BEYOND = 4  // the reference feature's octave in the store is >= nlevels: the three values are kept
};

// ORBmatcher::DescriptorDistance on the eight words of two descriptors
MPM_HD int mpm_hamming(const uint32_t a[8], const uint32_t b[8]) {
  int d = 0;
  for (int k = 0; k < 8; k++) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// :977-979.  The rank of the median in a sorted row of N distances, the self-distance included.
MPM_HD int mpm_median_rank(int N) { return (int)(0.5 * (N - 1)); }

// Element `rank` of the sorted row, by bisection over the value: the smallest v in 0 .. 256 with at least rank + 1 entries <= v.  count_le(v) counts the row's
// entries <= v: a loop over an array on the host, compares on registers or a ballot in the kernel.  Nine rounds whatever the row holds (257 values).
template <class CountLE>
MPM_HD int mpm_select(int rank, CountLE count_le) {
  int lo = 0, hi = 256;
  for (int it = 0; it < 9; it++) {
    const int mid = (lo + hi) >> 1;
    if (count_le(mid) > rank) hi = mid; else lo = mid + 1;   // once lo == hi, mid is the answer and stays
  }
  return lo;
}

// :981-985: `median < BestMedian` in list order keeps the FIRST observation with the least median.  The minimum of this key over the observations is that one.
MPM_HD uint32_t mpm_key(int median, int i) { return (uint32_t)median << 16 | (uint32_t)i; }
MPM_HD int mpm_key_index(uint32_t key) { return (int)(key & 0xFFFFu); }

// :799-805 for one observer: normali = mWorldPos - Owi; normal + normali / cv::norm(normali).  cv::norm accumulates the squares in double; the division is a
// product with (float)(1. / norm).  t: the three products, which the caller adds to its running sums in list order.
MPM_HD void mpm_term(const float p[3], const float O[3], float t[3]) {
  const float d0 = p[0] - O[0], d1 = p[1] - O[1], d2 = p[2] - O[2];
  double s = 0;
  s += (double)d0 * (double)d0; s += (double)d1 * (double)d1; s += (double)d2 * (double)d2;
  const float a = (float)(1. / sqrt(s));
  t[0] = d0 * a; t[1] = d1 * a; t[2] = d2 * a;
}

// :807-815: PC = Pos - pRefKF->GetCameraCenter(); mfMaxDistance = dist * levelScaleFactor; mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1]
MPM_HD void mpm_depth(const float p[3], const float Or[3], float sf_level, float sf_last, float& dmin, float& dmax) {
  const float c0 = p[0] - Or[0], c1 = p[1] - Or[1], c2 = p[2] - Or[2];
  double s = 0;
  s += (double)c0 * (double)c0; s += (double)c1 * (double)c1; s += (double)c2 * (double)c2;
  const float dist = (float)sqrt(s);
  dmax = dist * sf_level;
  dmin = dmax / sf_last;
}

// :816: mNormalVector = normal / n
MPM_HD void mpm_mean(const float sum[3], int N, float normal[3]) {
  const float an = (float)(1. / (double)N);
  normal[0] = sum[0] * an; normal[1] = sum[1] * an; normal[2] = sum[2] * an;
}

// A keyframe as the evaluator reads it: its feature count, descriptors and octaves
struct MpmKf { int n; const uint8_t* desc; const uint8_t* oct; };

// The rules of ccm_mappoint_refresh_resident that do not need the store; nullptr, or what is wrong.  *any_ref: some point asks for the normal / depth part.
static inline const char* mpm_check_args(int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_feat,
                                         const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels, const float* scale_factors, const int32_t* best_obs,
                                         const float* normal, const float* min_dist, const float* max_dist, const uint8_t* status, bool* any_ref) {
  *any_ref = false;
  if (K < 0 || P < 0) return "K or P negative";
  if (nlevels < 1 || nlevels > MPM_MAX_LEVELS) return "nlevels outside 1 .. 256";
  if (K > 0 && !keys) return "null keys";
  if (P == 0) return nullptr;
  if (!obs_off || !ref_kf || !ref_feat || !scale_factors || !best_obs || !normal || !min_dist || !max_dist || !status) return "null pointers";
  if (obs_off[0] != 0) return "obs_off does not start at 0";
  for (int p = 0; p < P; p++) {
    if (obs_off[p + 1] < obs_off[p]) return "obs_off decreases";
    if (obs_off[p + 1] - obs_off[p] > MPM_MAX_OBS) return "a map point has more than 256 observations";
    if (ref_kf[p] < -1 || ref_kf[p] >= K) return "ref_kf outside -1 .. K - 1";
    if (ref_kf[p] >= 0) *any_ref = true;
  }
  const int M = obs_off[P];
  if (M > 0 && (!obs_kf || !obs_feat)) return "null observation lists";
  for (int o = 0; o < M; o++)
    if (obs_kf[o] < 0 || obs_kf[o] >= K) return "obs_kf outside 0 .. K - 1";
  if (*any_ref && (!pos || !kf_center)) return "null pos or kf_center while a point has a reference keyframe";
  return nullptr;
}

// The feature indices against the keys' feature counts kf_n[K]
static inline const char* mpm_check_features(const int32_t* kf_n, int P, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_feat, const int32_t* ref_kf,
                                             const int32_t* ref_feat) {
  const int M = P > 0 ? obs_off[P] : 0;
  for (int o = 0; o < M; o++)
    if (obs_feat[o] < 0 || obs_feat[o] >= kf_n[obs_kf[o]]) return "obs_feat outside the key's features";
  for (int p = 0; p < P; p++)
    if (ref_kf[p] >= 0 && (ref_feat[p] < 0 || ref_feat[p] >= kf_n[ref_kf[p]])) return "ref_feat outside the key's features";
  return nullptr;
}

// One point on the calling thread: its N observations (obs_kf, obs_feat), copied into words first (the descriptors of a shadow lie on no particular boundary).
static inline void mpm_point_host(const MpmKf* kf, const float* kf_center, int N, const int32_t* obs_kf, const int32_t* obs_feat, const float* pos, int ref_kf, int ref_feat,
                                  int nlevels, const float* scale_factors, int32_t* best_obs, uint8_t* best_desc, float normal[3], float* min_dist, float* max_dist,
                                  uint8_t* status) {
  *best_obs = -1; *status = 0;
  if (N == 0) return;   // :794-795, :944-945: nothing changes
  uint32_t w[MPM_MAX_OBS][8];
  for (int i = 0; i < N; i++) memcpy(w[i], kf[obs_kf[i]].desc + 32 * (size_t)obs_feat[i], 32);
  const int rank = mpm_median_rank(N);
  uint32_t best = MPM_NO_KEY;
  for (int i = 0; i < N; i++) {
    int row[MPM_MAX_OBS];
    for (int j = 0; j < N; j++) row[j] = mpm_hamming(w[i], w[j]);
    const int median = mpm_select(rank, [&](int v) { int c = 0; for (int j = 0; j < N; j++) c += row[j] <= v; return c; });
    const uint32_t key = mpm_key(median, i);
    if (key < best) best = key;
  }
  *best_obs = mpm_key_index(best);
  *status |= MPM_DESC;
  if (best_desc) memcpy(best_desc, w[*best_obs], 32);
  if (ref_kf < 0) return;
  const int o = kf[ref_kf].oct[ref_feat];
  if (o >= nlevels) { *status |= MPM_OCTAVE_BEYOND; return; }   // neither table entry is read
  float sum[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < N; i++) {
    float t[3];
    mpm_term(pos, kf_center + 3 * (size_t)obs_kf[i], t);
    sum[0] = sum[0] + t[0]; sum[1] = sum[1] + t[1]; sum[2] = sum[2] + t[2];
  }
  mpm_depth(pos, kf_center + 3 * (size_t)ref_kf, scale_factors[o], scale_factors[nlevels - 1], *min_dist, *max_dist);
  mpm_mean(sum, N, normal);
  *status |= MPM_NORMAL_DEPTH;
}

// A whole call, already validated, point after point
static inline void mappoint_refresh_eval_host(const MpmKf* kf, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_feat,
                                              const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels, const float* scale_factors, int32_t* best_obs,
                                              uint8_t* best_desc, float* normal, float* min_dist, float* max_dist, uint8_t* status) {
  for (int p = 0; p < P; p++) {
    const int o0 = obs_off[p];
    mpm_point_host(kf, kf_center, obs_off[p + 1] - o0, obs_kf + o0, obs_feat + o0, pos ? pos + 3 * (size_t)p : nullptr, ref_kf[p], ref_feat[p], nlevels, scale_factors,
                   best_obs + p, best_desc ? best_desc + 32 * (size_t)p : nullptr, normal + 3 * (size_t)p, min_dist + p, max_dist + p, status + p);
  }
}
