// fuse_math.h — one (keyframe, point) pair of ORBmatcher::Fuse, host + device, in both of its forms: Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
// (cslam/src/ORBmatcher.cpp:995-1122, the Sim3 form) and Fuse(pKF, vpMapPoints, th) (:854-993, the pose form).  The Sim3 decomposition, the projection and its four
// gates, MapPoint::PredictScale, the window of KeyFrame::GetFeaturesInArea and the Hamming arg-min.  The two forms differ in the candidate loop alone: the pose form
// has a chi-square gate (:941-955) where the Sim3 form has none, so the candidate and the window walk are templates on `bool kChi2` (fsm_gate takes Rcw, tcw and Ow
// in both forms).  The argument rules of the two entry points follow.
// The kernels of fuse.hip run these lines; cslam::SearchAndFuseBatch and cslam::SearchInNeighborsBatch (host/ccm_host.cpp) compile them with g++.
//
// Every cv::Mat expression is evaluated as OpenCV 4.2 does in a baseline build (no FMA), by the rules oracle/ref_shim/opencv2/mini_cv.h declares
// (gemm_eval, Mat::dot, norm, Mat / s); DESIGN.md §19 lists them.  Compile with -ffp-contract=off: no product may fuse into an FMA.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "orb_math.h"

#if defined(__HIPCC__)
#define FSM_HD __host__ __device__ inline
#else
#define FSM_HD static inline
#endif

enum {
  FSM_BEHIND = 0,      // p3Dc(2) < 0
  FSM_OUTSIDE = 1,     // !pKF->IsInImage(u, v)
  FSM_RANGE = 2,       // dist3D outside [0.8 mfMinDistance, 1.2 mfMaxDistance]
  FSM_ANGLE = 3,       // PO.dot(Pn) < 0.5 dist3D
  FSM_EMPTY = 4,       // GetFeaturesInArea returned nothing
  FSM_NO_LEVEL = 5,    // no candidate at nPredictedLevel - 1 .. nPredictedLevel
  FSM_FAR = 6,         // bestDist > TH_LOW
  FSM_HIT = 7
};
#define FSM_TH_LOW 50
#define FSM_TH_HIGH 100       // ORBmatcher::TH_HIGH, the threshold of SearchBySim3
#define FSM_NO_IDX 0xFFFFu
#define FSM_NO_DIST 511u
#define FSM_MAX_LEVELS 16
#define FSM_GRID_COLS 75      // FRAME_GRID_COLS / ROWS (cslam/include/cslam/Frame.h:51-52); KeyFrame::mnGridCols / Rows
#define FSM_GRID_ROWS 48
#define FSM_CELLS (FSM_GRID_COLS * FSM_GRID_ROWS)
#define FSM_REC_FLOATS 10     // fx fy cx cy, mnMinX mnMinY mnMaxX mnMaxY (the floats of the ints), mfGridElementWidthInv, mfGridElementHeightInv
#define FSM_POSE_FLOATS 15    // Rcw (9, row-major), tcw (3), Ow (3)
#define FSM_WIDE 64           // a window whose cells hold more features than this is the whole wave's
#define FPM_CHI2 5.99         // ORBmatcher.cpp:950, a double literal
#define FPM_JOB_INTS 4        // a job's record in the staged block: keyframe, first point, points, first table word
#define FPM_TILE 256          // pairs per workgroup
#define SSM_JOB_FLOATS 28     // a SearchBySim3 job's floats in the staged block: fx fy cx cy, R_aw (9, row-major), t_aw (3), sR_ba (9), t_ba (3)

FSM_HD uint32_t fsm_pack(int status, int level, uint32_t dist, uint32_t idx) {
  return ((uint32_t)status << 29) | ((uint32_t)level << 25) | (dist << 16) | idx;
}

// ORBmatcher.cpp:1004-1008 [EXT].  S = rows 0..2 of Scw (3x4, row-major).  Mat::dot accumulates in double; scw is a float; Mat / s is Mat * (1. / s) with the
// scalar rounded to float and the product formed in float; -Rcw.t() * tcw is ONE gemm with a transposed operand: a double accumulator, alpha = -1, stored to float.
FSM_HD void fsm_decompose_scw(const float S[12], float pose[FSM_POSE_FLOATS]) {
  double d = 0;
  for (int c = 0; c < 3; c++) d += (double)S[c] * (double)S[c];
  const float scw = (float)sqrt(d);
  const float inv = (float)(1. / (double)scw);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose[3 * r + c] = S[4 * r + c] * inv;
    pose[9 + r] = S[4 * r + 3] * inv;
  }
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)pose[3 * k + r] * (double)pose[9 + k];
    pose[12 + r] = (float)(s * -1.0 + 0.0);
  }
}

// MapPoint::PredictScale(dist, pKF) (MapPoint.cpp:837-852): log(float) is logf, ceil(float) is ceilf.  The conversion to int of a value no int holds is the x86
// cvttss2si's "integer indefinite" INT_MIN, which the clamp turns into 0; stated here so that host and device agree on NaN and Inf.
FSM_HD int fsm_predict_scale(float mfMaxDistance, float dist, float logScaleFactor, int nlevels) {
  const float ratio = mfMaxDistance / dist;
  const float c = ceilf(orbm::logf_glibc(ratio) / logScaleFactor);
  if (!(c >= 0.0f) || c >= 2147483648.0f) return 0;
  if (c >= (float)nlevels) return nlevels - 1;
  return (int)c;
}

// ORBmatcher.cpp:1030-1068.  Returns the first gate that fails (FSM_BEHIND .. FSM_ANGLE) or FSM_EMPTY when the pair goes on to the window.  u, v are written from
// FSM_OUTSIDE on (0 for FSM_BEHIND), level only when the pair goes on.  NaN and Inf fall through the comparisons as the source's do.
FSM_HD int fsm_gate(const float rec[FSM_REC_FLOATS], const float pose[FSM_POSE_FLOATS], const float P[3], const float Pn[3], float mfMinDistance, float mfMaxDistance,
                    int nlevels, float logScaleFactor, float& u, float& v, int& level) {
  float Pc[3];
  for (int i = 0; i < 3; i++) {   // Rcw * p3Dw + tcw: the small-matrix gemm (frame_math.h:81-86)
    const float t = pose[3 * i] * P[0] + pose[3 * i + 1] * P[1] + pose[3 * i + 2] * P[2];
    Pc[i] = (float)((double)t * 1.0 + (double)pose[9 + i] * 1.0);
  }
  u = 0.0f; v = 0.0f; level = 0;
  if (Pc[2] < 0.0f) return FSM_BEHIND;
  const float invz = (float)(1.0 / (double)Pc[2]);
  const float x = Pc[0] * invz, y = Pc[1] * invz;
  u = rec[0] * x + rec[2];
  v = rec[1] * y + rec[3];
  if (!(u >= rec[4] && u < rec[6] && v >= rec[5] && v < rec[7])) return FSM_OUTSIDE;   // KeyFrame::IsInImage (KeyFrame.cpp:1203-1206)
  const float maxDistance = 1.2f * mfMaxDistance, minDistance = 0.8f * mfMinDistance;   // MapPoint.cpp:825-835
  const float PO[3] = {P[0] - pose[12], P[1] - pose[13], P[2] - pose[14]};
  double s2 = 0;
  for (int i = 0; i < 3; i++) s2 += (double)PO[i] * (double)PO[i];
  const float dist3D = (float)sqrt(s2);
  if (dist3D < minDistance || dist3D > maxDistance) return FSM_RANGE;
  double dot = 0;
  for (int i = 0; i < 3; i++) dot += (double)PO[i] * (double)Pn[i];
  if (dot < 0.5 * (double)dist3D) return FSM_ANGLE;
  level = fsm_predict_scale(mfMaxDistance, dist3D, logScaleFactor, nlevels);
  return FSM_EMPTY;
}

// the cell range of KeyFrame::GetFeaturesInArea (KeyFrame.cpp:1167-1181) on the keyframe's int bounds; false when the window misses the grid.  The float is clamped
// before the conversion (x86 turns a float no int holds, NaN included, into INT_MIN, and that is what the clamps restate).
FSM_HD int fsm_cell_lo(float f, int n) { return !(f > 0.0f) ? 0 : f >= (float)n ? n : (int)f; }              // max(0, (int)floor(.)); n: the caller returns
FSM_HD int fsm_cell_hi(float c, int n) { return (!(c >= 0.0f) || c >= 2147483648.0f) ? -1 : c >= (float)(n - 1) ? n - 1 : (int)c; }   // min(n - 1, (int)ceil(.))
FSM_HD bool fsm_cell_range(const float rec[FSM_REC_FLOATS], float x, float y, float r, int& x0, int& x1, int& y0, int& y1) {
  x0 = fsm_cell_lo(floorf((x - rec[4] - r) * rec[8]), FSM_GRID_COLS);
  if (x0 >= FSM_GRID_COLS) return false;
  x1 = fsm_cell_hi(ceilf((x - rec[4] + r) * rec[8]), FSM_GRID_COLS);
  if (x1 < 0) return false;
  y0 = fsm_cell_lo(floorf((y - rec[5] - r) * rec[9]), FSM_GRID_ROWS);
  if (y0 >= FSM_GRID_ROWS) return false;
  y1 = fsm_cell_hi(ceilf((y - rec[5] + r) * rec[9]), FSM_GRID_ROWS);
  if (y1 < 0) return false;
  return true;
}

// 32 descriptor bytes as 8 words.  On the device the descriptors lie on 16 bytes in the staged block.
FSM_HD void fsm_load_desc(const uint8_t* d, uint32_t q[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 a = reinterpret_cast<const uint4*>(d)[0], b = reinterpret_cast<const uint4*>(d)[1];
  q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w;
#else
  memcpy(q, d, 32);
#endif
}
FSM_HD int fsm_hamming(const uint32_t a[8], const uint32_t b[8]) {   // ORBmatcher::DescriptorDistance: a population count over 256 bits
  int n = 0;
  for (int i = 0; i < 8; i++) n += __builtin_popcount(a[i] ^ b[i]);
  return n;
}

// One candidate of the window: feature f of the keyframe (xy, octave, descriptor of ITS arrays).  in_window: the feature is one of vIndices (KeyFrame.cpp:1190-1195).
// Returns its distance, or -1 when it is not in the window or not at the level (ORBmatcher.cpp:1089).
// kChi2: the pose form, in the order of ORBmatcher.cpp:941-955: the level filter, ex / ey / e2 in f32 (two products and one sum, never fused), the gate
// `e2 * mvInvLevelSigma2[kpLevel] > 5.99` (an f32 product widened to double for the comparison, so a NaN passes as it does there), then the distance.
// o <= level < nlevels bounds the read of inv_sigma2, which the Sim3 form does not read.
// kMask: SearchByProjection(pKF, Scw, ...)'s `if(vpMatched[idx]) continue;` (ORBmatcher.cpp:393), tested before the level filter: skip[f] != 0 makes feature f no
// candidate, but it stays one of vIndices (the reference tests vIndices.empty() before its loop).  Without the flag skip is not read.
template <bool kChi2, bool kMask = false>
FSM_HD int fsm_candidate(const float* xy, const uint8_t* oct, const uint8_t* desc, int f, float u, float v, float r, int level, const float* inv_sigma2,
                         const uint32_t q[8], bool& in_window, const uint8_t* skip = nullptr) {
  const float kpx = xy[2 * f], kpy = xy[2 * f + 1];
  const float distx = kpx - u, disty = kpy - v;
  in_window = fabsf(distx) < r && fabsf(disty) < r;
  if (!in_window) return -1;
  if (kMask && skip[f]) return -1;
  const int o = oct[f];
  if (o < level - 1 || o > level) return -1;
  if (kChi2) {
    const float ex = u - kpx, ey = v - kpy;
    const float exx = ex * ex, eyy = ey * ey;
    const float e2 = exx + eyy;
    const float g = e2 * inv_sigma2[o];
    if ((double)g > FPM_CHI2) return -1;
  }
  uint32_t d[8];
  fsm_load_desc(desc + 32 * (size_t)f, d);
  return fsm_hamming(q, d);
}

// the features a window's cells hold: the cells iy = y0 .. y1 of one ix are neighbours in the x-major CSR
FSM_HD int fsm_window_count(const int32_t* cell_off, int x0, int x1, int y0, int y1) {
  int n = 0;
  for (int ix = x0; ix <= x1; ix++) n += cell_off[ix * FSM_GRID_ROWS + y1 + 1] - cell_off[ix * FSM_GRID_ROWS + y0];
  return n;
}

// the packed answer of a pair that passed the gates, from the best key (dist << 16 | CSR position, ~0u: no candidate at the level, or every one masked) and whether
// the window was empty.  dist_th: TH_LOW for Fuse and SearchByProjection, TH_HIGH for SearchBySim3.
FSM_HD uint32_t fsm_finish(int level, bool any, uint32_t key, const uint16_t* cell_idx, uint32_t dist_th) {
  if (!any) return fsm_pack(FSM_EMPTY, level, FSM_NO_DIST, FSM_NO_IDX);
  if (key == ~0u) return fsm_pack(FSM_NO_LEVEL, level, FSM_NO_DIST, FSM_NO_IDX);
  const uint32_t dist = key >> 16, idx = cell_idx[key & 0xFFFFu];
  return fsm_pack(dist <= dist_th ? FSM_HIT : FSM_FAR, level, dist, idx);
}

// ORBmatcher.cpp:1071-1118 (kChi2: :920-989) for one pair that passed the gates, one candidate after the other in the reference's order: ix, then iy, then the
// position in the cell — ascending CSR position, so the first strict minimum is the lowest position among the minima.  All arrays are the keyframe's own (cell_idx:
// local feature indices).  n_cand (nullable): the size of vIndices.  kMask, skip: fsm_candidate's; dist_th: fsm_finish's.
template <bool kChi2, bool kMask = false>
FSM_HD uint32_t fsm_window_best(const float rec[FSM_REC_FLOATS], const int32_t* cell_off, const uint16_t* cell_idx, const float* xy, const uint8_t* oct,
                                const uint8_t* desc, float u, float v, int level, float th, const float* scale_factors, const float* inv_sigma2, const uint32_t q[8],
                                int* n_cand, const uint8_t* skip = nullptr, uint32_t dist_th = FSM_TH_LOW) {
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
        const int d = fsm_candidate<kChi2, kMask>(xy, oct, desc, cell_idx[pos], u, v, r, level, inv_sigma2, q, in, skip);
        any |= in; n += in;
        if (d >= 0) { const uint32_t k = ((uint32_t)d << 16) | (uint32_t)pos; if (k < key) key = k; }   // pos ascends: an equal distance later is no less
      }
    }
  }
  if (n_cand) *n_cand = n;
  return fsm_finish(level, any, key, cell_idx, dist_th);
}

// ---- SearchBySim3 (ORBmatcher.cpp:1124-1348) -----------------------------------------------------------------------------------------------------------------
// :1141-1143.  sR12 = s12 * R12: Mat * s, the product formed in float.  sR21 = (1.0 / s12) * R12.t(): a MatTExpr with alpha = 1.0 / (double)s12, materialised as the
// transpose times alpha ROUNDED TO FLOAT (alpha == 1 multiplies nothing, which leaves the same bits).  t21 = -sR21 * t12: the negated matrix first (unary minus on
// a Mat), then the small-matrix gemm without an addend: a float accumulator summed left to right, stored as (float)(t * 1.0 + 0.0).
FSM_HD void ssm_derive(float s12, const float R12[9], const float t12[3], float sR12[9], float sR21[9], float t21[3]) {
  for (int i = 0; i < 9; i++) sR12[i] = R12[i] * s12;
  const double alpha = 1.0 / (double)s12;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) sR21[3 * r + c] = alpha != 1 ? R12[3 * c + r] * (float)alpha : R12[3 * c + r];
  for (int r = 0; r < 3; r++) {
    const float n0 = -sR21[3 * r], n1 = -sR21[3 * r + 1], n2 = -sR21[3 * r + 2];
    const float t = n0 * t12[0] + n1 * t12[1] + n2 * t12[2];
    t21[r] = (float)((double)t * 1.0 + 0.0);
  }
}

// One direction's gate, :1180-1208 (a = 1, b = 2) and :1260-1288 (a = 2, b = 1): p3Dc_a = R_aw * p3Dw + t_aw and p3Dc_b = sR_ba * p3Dc_a + t_ba, two small-matrix
// gemms with an addend; depth; the projection with job[0..3]; the TARGET's IsInImage (rec[4..7]); dist3D = the float of the double norm of p3Dc_b; the range;
// PredictScale.  job: SSM_JOB_FLOATS.  job[0..3] are pKF1's intrinsics in BOTH directions (:1127-1130 reads them once, :1192 and :1272 use them), whatever the
// target's record says.  There is no viewing-angle gate: FSM_ANGLE does not occur.  Returns and outputs as fsm_gate.
FSM_HD int ssm_gate(const float rec[FSM_REC_FLOATS], const float job[SSM_JOB_FLOATS], const float P[3], float mfMinDistance, float mfMaxDistance, int nlevels,
                    float logScaleFactor, float& u, float& v, int& level) {
  const float *Raw = job + 4, *taw = job + 13, *sR = job + 16, *tba = job + 25;
  float Pa[3], Pb[3];
  for (int i = 0; i < 3; i++) {
    const float t = Raw[3 * i] * P[0] + Raw[3 * i + 1] * P[1] + Raw[3 * i + 2] * P[2];
    Pa[i] = (float)((double)t * 1.0 + (double)taw[i] * 1.0);
  }
  for (int i = 0; i < 3; i++) {
    const float t = sR[3 * i] * Pa[0] + sR[3 * i + 1] * Pa[1] + sR[3 * i + 2] * Pa[2];
    Pb[i] = (float)((double)t * 1.0 + (double)tba[i] * 1.0);
  }
  u = 0.0f; v = 0.0f; level = 0;
  if (Pb[2] < 0.0f) return FSM_BEHIND;
  const float invz = (float)(1.0 / (double)Pb[2]);
  const float x = Pb[0] * invz, y = Pb[1] * invz;
  u = job[0] * x + job[2];
  v = job[1] * y + job[3];
  if (!(u >= rec[4] && u < rec[6] && v >= rec[5] && v < rec[7])) return FSM_OUTSIDE;
  const float maxDistance = 1.2f * mfMaxDistance, minDistance = 0.8f * mfMinDistance;
  double s2 = 0;
  for (int i = 0; i < 3; i++) s2 += (double)Pb[i] * (double)Pb[i];
  const float dist3D = (float)sqrt(s2);
  if (dist3D < minDistance || dist3D > maxDistance) return FSM_RANGE;
  level = fsm_predict_scale(mfMaxDistance, dist3D, logScaleFactor, nlevels);
  return FSM_EMPTY;
}

// the jobs' SSM_JOB_FLOATS from the caller's three arrays: K4 (4), the source pose (12), the transform (12) per job
FSM_HD void ssm_pack_jobs(int J, const float* job_K4, const float* job_src_pose, const float* job_T, float* out) {
  for (int j = 0; j < J; j++) {
    float* r = out + SSM_JOB_FLOATS * (size_t)j;
    memcpy(r, job_K4 + 4 * (size_t)j, 4 * sizeof(float)); memcpy(r + 4, job_src_pose + 12 * (size_t)j, 12 * sizeof(float));
    memcpy(r + 16, job_T + 12 * (size_t)j, 12 * sizeof(float));
  }
}

// The argument rules of ccm_fuse_sim3_eval; nullptr, or what is wrong.  The scalar rules come first and read no array.  cell_idx: int32 as the caller passes it.
// (fsm_check_scalars: the scalar rules alone, which are all the resident forms share with it: their keyframes are the store's, validated when they were added.)
FSM_HD const char* fsm_check_scalars(int K, int P, int nlevels, float th) {
  if (K < 0 || P < 0) return "K or P negative";
  if ((int64_t)K * (int64_t)P > (int64_t)INT32_MAX) return "K * P beyond INT32_MAX";
  if (nlevels < 1 || nlevels > FSM_MAX_LEVELS) return "nlevels outside 1 .. 16";
  if (!(th > 0.0f) || !(th <= 3.402823466e+38f)) return "th not finite and positive";
  return nullptr;
}
FSM_HD const char* fsm_check_args(int K, int P, const int32_t* feat_off, const int32_t* cell_off, const int32_t* cell_idx, int nlevels, float th) {
  if (const char* why = fsm_check_scalars(K, P, nlevels, th)) return why;
  if (K == 0) return nullptr;
  if (!feat_off || !cell_off) return "null pointers";
  if (feat_off[0] != 0) return "feat_off[0] != 0";
  for (int k = 0; k < K; k++) {
    const int64_t n = (int64_t)feat_off[k + 1] - feat_off[k];
    if (n < 0) return "feat_off decreases";
    if (n > 65535) return "more than 65535 features in a keyframe";
    const int32_t* co = cell_off + (size_t)k * (FSM_CELLS + 1);
    if (co[0] != 0) return "cell_off does not start at 0";
    for (int c = 0; c < FSM_CELLS; c++)
      if (co[c + 1] < co[c]) return "cell_off decreases";
    if (co[FSM_CELLS] != (int32_t)n) return "cell_off does not end at the keyframe's feature count";
    if (n && !cell_idx) return "null pointers";
    const int32_t* ci = cell_idx + feat_off[k];
    for (int64_t j = 0; j < n; j++)
      if (ci[j] < 0 || ci[j] >= n) return "cell_idx out of range";
  }
  return nullptr;
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

// The mask rules of ccm_sim3_project_eval_resident; nullptr, or what is wrong.  kf_n[k]: the feature count of key k in the store.
FSM_HD const char* fsm_check_skip(int K, const int32_t* skip_off, const uint8_t* feat_skip, const int32_t* kf_n) {
  if (K <= 0) return nullptr;
  if (!skip_off) return "null pointers";
  if (skip_off[0] != 0) return "skip_off[0] != 0";
  for (int k = 0; k < K; k++) {
    if (skip_off[k + 1] < skip_off[k]) return "skip_off decreases";
    if (skip_off[k + 1] - skip_off[k] != kf_n[k]) return "a mask is not as long as its keyframe's features";
  }
  if (skip_off[K] > 0 && !feat_skip) return "null pointers";
  return nullptr;
}
// the null-pointer rules of ccm_sim3_pair_eval_resident's per-job floats (the index arrays are fpm_check_jobs')
FSM_HD const char* fsm_check_pair_jobs(int J, const float* job_K4, const float* job_src_pose, const float* job_T) {
  if (J > 0 && (!job_K4 || !job_src_pose || !job_T)) return "null job arrays";
  return nullptr;
}

// The null-pointer rules of the six entry points after their context (and store), which the host evaluators (host/ccm_host.cpp) share with them; nullptr, or
// "null pointers".  kf: the keyframes' records, or the keys of a store.  feats: fsm_feats_ok for the flat forms, true for the resident ones.
FSM_HD bool fsm_feats_ok(size_t F, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc) { return !F || (feat_xy && feat_octave && feat_desc); }
// the keyframe-major forms: ccm_fuse_sim3_eval, ccm_fuse_sim3_eval_resident, ccm_sim3_project_eval_resident
FSM_HD const char* fsm_check_kf_pointers(int K, int P, const void* kf, const float* Scw, const float* scale_factors, const float* pos, const float* normal,
                                         const float* min_dist, const float* max_dist, const uint8_t* pt_desc, const uint32_t* table, const int32_t* n_valid,
                                         const int32_t* n_hit, bool feats) {
  if (!scale_factors || (K > 0 && (!kf || !Scw || !n_valid || !n_hit)) || (P > 0 && (!pos || !normal || !min_dist || !max_dist || !pt_desc)) ||
      (K > 0 && P > 0 && !table) || !feats)
    return "null pointers";
  return nullptr;
}
// the job forms.  fuse: ccm_fuse_pose_eval and its resident form, which read a pose per keyframe, inv_level_sigma2 and the normals; ccm_sim3_pair_eval_resident
// reads none of the three (its per-job floats are fsm_check_pair_jobs').  total: fpm_check_jobs'.
FSM_HD const char* fsm_check_job_pointers(int K, int P, int J, int64_t total, bool fuse, const void* kf, const float* pose, const float* scale_factors,
                                          const float* inv_level_sigma2, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                                          const uint8_t* pt_desc, const uint32_t* table, const int32_t* n_valid, const int32_t* n_hit, bool feats) {
  if (!scale_factors || (fuse && !inv_level_sigma2) || (K > 0 && (!kf || (fuse && !pose))) || (J > 0 && (!n_valid || !n_hit)) ||
      (P > 0 && (!pos || (fuse && !normal) || !min_dist || !max_dist || !pt_desc)) || (total > 0 && !table) || !feats)
    return "null pointers";
  return nullptr;
}
