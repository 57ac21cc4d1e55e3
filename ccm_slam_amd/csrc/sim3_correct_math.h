// sim3_correct_math.h — the Sim3 correction of a closed loop's or merged map's keyframes and map points, host + device: the per-keyframe and per-point
// arithmetic of LoopFinder::CorrectLoop (cslam/src/LoopFinder.cpp:543-613), MapMerger::MergeMaps (cslam/src/MapMerger.cpp:289-395) and the tail of the
// essential-graph optimisers (cslam/src/Optimizer.cpp:1279-1330), with KeyFrame::SetPose's camera centre (KeyFrame.cpp:298-302) and
// MapPoint::UpdateNormalAndDepth (MapPoint.cpp:794-822).  The kernels of sim3_correct.hip run these lines; cslam::Sim3MapCorrection (host/ccm_host.cpp)
// compiles them with g++.
//
// g2o::Sim3 is sim3_math.h (sim3_mul / sim3_inv / sim3_map), Eigen::Quaterniond(R) and toRotationMatrix are ba_math.h (ba_R_to_q / ba_q_to_R); the Converter
// functions are casts (host/ccm_convert.h states the same ones for the host).  The cv::Mat steps are evaluated as OpenCV 4.2 does in a baseline build (no
// FMA), with the rules oracle/ref_shim/opencv2/mini_cv.h declares.  They are restated from OpenCV's published sources and are NOT pinned against an OpenCV
// build in this tree (scripts/pin_opencv.py compares them on a machine that has cv2):
//   Tiw * Twc            4x4 f32 gemm, small-matrix path: f32 accumulator, the four products added left to right, (float)(t * 1.0 + 0.0)
//   -Rcw.t() * tcw       3x3 by 3x1 small-matrix gemm with alpha = -1: f32 accumulator left to right, (float)((double)t * -1.0 + 0.0)
//   a - b                f32, elementwise
//   cv::norm(v)          the squares summed in double, left to right, sqrt in double (`const float dist = cv::norm(PC)` rounds that to float)
//   m / s                convertTo with alpha = 1. / s: every element times (float)alpha, in f32
//   normal + v           f32, elementwise
// Compile with -ffp-contract=off: no product may fuse into an FMA.  DESIGN.md §13 states the ownership / rank rule the callers apply.
#pragma once
#include <stdint.h>
#include "sim3_math.h"

#define S3C_HD BA_HD

// rows 0..2 of Tic = Tiw * Twc; both operands are rows 0..2 of a 4x4 whose last row is 0 0 0 1 (12 floats, row-major)
S3C_HD void s3c_tic(const float* Tiw, const float* Twc, float Tic[12]) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float t = Tiw[4 * r] * Twc[c];
      t = t + Tiw[4 * r + 1] * Twc[4 + c];
      t = t + Tiw[4 * r + 2] * Twc[8 + c];
      t = t + Tiw[4 * r + 3] * (c == 3 ? 1.0f : 0.0f);
      Tic[4 * r + c] = t;
    }
}

// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of a 12-float pose: Quaterniond(R), not normalised
S3C_HD Sim3d s3c_sim3_of_pose(const float* T) {
  const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
  BaPose q;
  ba_R_to_q(R, q);
  return Sim3d{q.qx, q.qy, q.qz, q.qw, (double)T[3], (double)T[7], (double)T[11], 1.0};
}

// Converter::toCvSE3(S.rotation().toRotationMatrix(), S.translation() * (1. / S.scale())), rows 0..2
S3C_HD void s3c_pose_of_sim3(const Sim3d& S, float T[12]) {
  const BaPose q{S.qx, S.qy, S.qz, S.qw, 0, 0, 0};
  double R[9];
  ba_q_to_R(q, R);
  const double k = 1. / S.s;
  T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2]; T[3] = (float)(S.tx * k);
  T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5]; T[7] = (float)(S.ty * k);
  T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8]; T[11] = (float)(S.tz * k);
}

// Ow = -Rcw.t() * tcw of KeyFrame::SetPose
S3C_HD void s3c_center(const float* T, float O[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    float t = T[r] * T[3];
    t = t + T[4 + r] * T[7];
    t = t + T[8 + r] * T[11];
    O[r] = (float)((double)t * -1.0 + 0.0);
  }
}

// One keyframe of the walk.  loop form (Tiw != nullptr): S_non = Sim3(Riw, tiw, 1), S_cor = Sim3(Ric, tic, 1) * Scw, or Scw itself for the current
// keyframe.  epilogue form (Tiw == nullptr): S_non and S_cor are the caller's.  Both: S_swi = S_cor.inverse(), the new pose [R | t / s] and its centre.
S3C_HD void s3c_keyframe(const float* Tiw, bool is_current, const float* Twc, const Sim3d& Scw, Sim3d& S_non, Sim3d& S_cor, Sim3d& S_swi, float T_new[12],
                         float O_new[3]) {
  if (Tiw) {
    if (is_current) {
      S_cor = Scw;
    } else {
      float Tic[12];
      s3c_tic(Tiw, Twc, Tic);
      S_cor = sim3_mul(s3c_sim3_of_pose(Tic), Scw);
    }
    S_non = s3c_sim3_of_pose(Tiw);
  }
  S_swi = sim3_inv(S_cor);
  s3c_pose_of_sim3(S_cor, T_new);
  s3c_center(T_new, O_new);
}

// toCvMat(S_swi.map(S_non.map(toVector3d(P)))): two maps, never one composed transform
S3C_HD void s3c_point(const Sim3d& S_non, const Sim3d& S_swi, const float* P, float out[3]) {
  const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
  double a[3], b[3];
  sim3_map(S_non, X, a);
  sim3_map(S_swi, a, b);
  out[0] = (float)b[0]; out[1] = (float)b[1]; out[2] = (float)b[2];
}

// the camera centre keyframe k shows to a point whose owner has rank owner_rank: the corrected one iff k belongs to the set and was walked before the owner
S3C_HD const float* s3c_seen_center(int k, int n_kf, const int32_t* kf_rank, int32_t owner_rank, const float* c_old, const float* c_new) {
  return (k < n_kf && kf_rank[k] < owner_rank) ? c_new + 3 * (size_t)k : c_old + 3 * (size_t)k;
}

// MapPoint::UpdateNormalAndDepth on position p with the observers obs_kf[o0 .. o1) in list order; an empty list leaves normal / dmin / dmax as they are
S3C_HD void s3c_normal_depth(const float p[3], int o0, int o1, const int32_t* obs_kf, int n_kf, const int32_t* kf_rank, int32_t owner_rank, const float* c_old,
                             const float* c_new, int ref_kf, int ref_level, const float* scale_factors, int n_levels, float normal[3], float& dmin, float& dmax) {
  if (o1 == o0) return;
  float n0 = 0.f, n1 = 0.f, n2 = 0.f;
  for (int o = o0; o < o1; o++) {
    const float* O = s3c_seen_center(obs_kf[o], n_kf, kf_rank, owner_rank, c_old, c_new);
    const float d0 = p[0] - O[0], d1 = p[1] - O[1], d2 = p[2] - O[2];
    double s = 0;
    s += (double)d0 * (double)d0; s += (double)d1 * (double)d1; s += (double)d2 * (double)d2;
    const float a = (float)(1. / sqrt(s));
    n0 = n0 + d0 * a; n1 = n1 + d1 * a; n2 = n2 + d2 * a;
  }
  const float* Or = s3c_seen_center(ref_kf, n_kf, kf_rank, owner_rank, c_old, c_new);
  const float c0 = p[0] - Or[0], c1 = p[1] - Or[1], c2 = p[2] - Or[2];
  double s = 0;
  s += (double)c0 * (double)c0; s += (double)c1 * (double)c1; s += (double)c2 * (double)c2;
  const float dist = (float)sqrt(s);
  dmax = dist * scale_factors[ref_level];
  dmin = dmax / scale_factors[n_levels - 1];
  const float an = (float)(1. / (double)(o1 - o0));
  normal[0] = n0 * an; normal[1] = n1 * an; normal[2] = n2 * an;
}
