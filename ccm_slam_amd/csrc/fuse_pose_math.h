// fuse_pose_math.h — one (keyframe, point) pair of ORBmatcher::Fuse(pKF, vpMapPoints, th) (cslam/src/ORBmatcher.cpp:854-993), host + device.  The projection, its four
// gates, MapPoint::PredictScale and the window of KeyFrame::GetFeaturesInArea are fuse_sim3_math.h's lines unchanged (fsm_gate takes Rcw, tcw and Ow, not Scw); what
// this header adds is the candidate loop of :933-962 with its chi-square gate, and the argument rules of ccm_fuse_pose_eval's job arrays.
// The kernel of fuse_pose.hip runs these lines; cslam::SearchInNeighborsBatch (host/ccm_host.cpp) compiles them with g++.  Compile with -ffp-contract=off.
#pragma once
#include "fuse_sim3_math.h"

#define FPM_CHI2 5.99         // ORBmatcher.cpp:950, a double literal
#define FPM_JOB_INTS 4        // a job's record in the staged block: keyframe, first point, points, first table word
#define FPM_TILE 256          // pairs per workgroup

// One candidate of the window, in the order of ORBmatcher.cpp:941-955: the level filter, ex / ey / e2 in f32 (two products and one sum, never fused), the gate
// `e2 * mvInvLevelSigma2[kpLevel] > 5.99` (an f32 product widened to double for the comparison, so a NaN passes as it does there), then the distance.
// in_window: the feature is one of vIndices (KeyFrame.cpp:1190-1195).  Returns the distance, or -1.  o <= level < nlevels bounds the read of inv_sigma2.
FSM_HD int fpm_candidate(const float* xy, const uint8_t* oct, const uint8_t* desc, int f, float u, float v, float r, int level, const float* inv_sigma2,
                         const uint32_t q[8], bool& in_window) {
  const float kpx = xy[2 * f], kpy = xy[2 * f + 1];
  const float distx = kpx - u, disty = kpy - v;
  in_window = fabsf(distx) < r && fabsf(disty) < r;
  if (!in_window) return -1;
  const int o = oct[f];
  if (o < level - 1 || o > level) return -1;
  const float ex = u - kpx, ey = v - kpy;
  const float exx = ex * ex, eyy = ey * ey;
  const float e2 = exx + eyy;
  const float g = e2 * inv_sigma2[o];
  if ((double)g > FPM_CHI2) return -1;
  uint32_t d[8];
  fsm_load_desc(desc + 32 * (size_t)f, d);
  return fsm_hamming(q, d);
}

// ORBmatcher.cpp:920-989 for one pair that passed the gates, one candidate after the other in the reference's order (ascending CSR position); the answer is
// fsm_finish's: the minimum of dist << 16 | position is the reference's first strict minimum.  n_cand (nullable): the size of vIndices.
FSM_HD uint32_t fpm_window_best(const float rec[FSM_REC_FLOATS], const int32_t* cell_off, const uint16_t* cell_idx, const float* xy, const uint8_t* oct,
                                const uint8_t* desc, float u, float v, int level, float th, const float* scale_factors, const float* inv_sigma2, const uint32_t q[8],
                                int* n_cand) {
  const float r = th * scale_factors[level];
  int x0, x1, y0, y1;
  bool any = false;
  uint32_t key = ~0u;
  int n = 0;
  if (fsm_cell_range(rec, u, v, r, x0, x1, y0, y1)) {
    for (int ix = x0; ix <= x1; ix++) {
      const int a = cell_off[ix * FSM_GRID_ROWS + y0], b = cell_off[ix * FSM_GRID_ROWS + y1 + 1];
      for (int pos = a; pos < b; pos++) {
        bool in;
        const int d = fpm_candidate(xy, oct, desc, cell_idx[pos], u, v, r, level, inv_sigma2, q, in);
        any |= in; n += in;
        if (d >= 0) { const uint32_t k = ((uint32_t)d << 16) | (uint32_t)pos; if (k < key) key = k; }
      }
    }
  }
  if (n_cand) *n_cand = n;
  return fsm_finish(level, any, key, cell_idx);
}

// The argument rules of ccm_fuse_pose_eval's job arrays; nullptr, or what is wrong.  total: the table's words, the sum of job_n; tiles: the workgroups.
FSM_HD const char* fpm_check_jobs(int J, int K, int P, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, int64_t* total, int64_t* tiles) {
  *total = 0; *tiles = 0;
  if (J < 0) return "J negative";
  if (J == 0) return nullptr;
  if (!job_kf || !job_pt0 || !job_n) return "null job arrays";
  int64_t sum = 0, t = 0;
  for (int j = 0; j < J; j++) {
    if (job_kf[j] < 0 || job_kf[j] >= K) return "job_kf outside the keyframes";
    if (job_n[j] < 0 || job_pt0[j] < 0) return "a negative job_n or job_pt0";
    if ((int64_t)job_pt0[j] + (int64_t)job_n[j] > (int64_t)P) return "a job's points end beyond P";
    sum += job_n[j];
    t += ((int64_t)job_n[j] + FPM_TILE - 1) / FPM_TILE;
    if (sum > (int64_t)INT32_MAX) return "more than INT32_MAX pairs";
  }
  if (t > (int64_t)INT32_MAX) return "too many workgroups";
  *total = sum; *tiles = t;
  return nullptr;
}
