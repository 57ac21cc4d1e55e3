// guided_search_math.h — one map point of ORBmatcher::SearchByProjection(Frame&, kfptr, const set<mpptr>&, th, ORBdist) (cslam/src/ORBmatcher.cpp:1482-1532),
// host + device: the camera centre of the frame's pose, the projection, the image test on the Frame's float bounds, the distance gate, MapPoint::PredictScale
// and the window the point asks Frame::GetFeaturesInArea for.  The kernel of frame.hip runs these lines; the host evaluator (host/ccm_host.cpp) compiles them
// with g++.
//
// Every cv::Mat expression is evaluated as OpenCV 4.2 does in a baseline build (no FMA), by the rules fuse_math.h and frame_math.h state.
// Compile with -ffp-contract=off: no product may fuse into an FMA.
#pragma once
#include "fuse_math.h"

enum {
  GSM_SKIPPED = 0,    // no live map point in the slot, or the point is in sAlreadyFound
  GSM_OUTSIDE = 1,    // u or v beyond the Frame's bounds (:1513-1516); a NaN passes, as in the source
  GSM_RANGE = 2,      // dist3D outside [0.8 mfMinDistance, 1.2 mfMaxDistance] (:1526)
  GSM_SEARCHED = 3    // the point goes on to GetFeaturesInArea
};
#define GSM_POSE_FLOATS 15   // Rcw (9, row-major), tcw (3), Ow (3): fuse_math.h's pose record

// :1482-1484.  Tcw = rows 0..2 of mTcw (3x4, row-major).  Ow = -Rcw.t() * tcw is ONE gemm with a transposed operand: the last loop of fsm_decompose_scw, a double
// accumulator, alpha = -1, stored to float.  (KeyFrame::SetPose's centre, which materialises Rwc and sums in f32, is another value: the caller never passes mOw.)
FSM_HD void gsm_pose(const float Tcw[12], float pose[GSM_POSE_FLOATS]) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose[3 * r + c] = Tcw[4 * r + c];
    pose[9 + r] = Tcw[4 * r + 3];
  }
  for (int r = 0; r < 3; r++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)pose[3 * k + r] * (double)pose[9 + k];
    pose[12 + r] = (float)(s * -1.0 + 0.0);
  }
}

// :1503-1532 for one point.  K = fx fy cx cy and b = the Frame's bounds, both f32.  There is no depth test: a point behind the camera goes on when it projects
// inside the image, and z == 0 gives inf or NaN, which fall through the comparisons as the source's do.  u, v are written from GSM_OUTSIDE on; level and radius only
// for GSM_SEARCHED (0 and -1 otherwise: a negative radius is an empty window by frame_cell_range).  The window's levels are level - 1 .. level + 1.
FSM_HD int gsm_gate(const float pose[GSM_POSE_FLOATS], const float K[4], float minX, float maxX, float minY, float maxY, const float P[3], float mfMinDistance,
                    float mfMaxDistance, float logScaleFactor, int nlevels, const float* scaleFactors, float th, float& u, float& v, int& level, float& radius) {
  float Pc[3];
  for (int i = 0; i < 3; i++) {   // Rcw * x3Dw + tcw: the small-matrix gemm (frame_math.h)
    const float t = pose[3 * i] * P[0] + pose[3 * i + 1] * P[1] + pose[3 * i + 2] * P[2];
    Pc[i] = (float)((double)t * 1.0 + (double)pose[9 + i] * 1.0);
  }
  level = 0; radius = -1.0f;
  const float invzc = (float)(1.0 / (double)Pc[2]);
  u = K[0] * Pc[0] * invzc + K[2];
  v = K[1] * Pc[1] * invzc + K[3];
  if (u < minX || u > maxX) return GSM_OUTSIDE;
  if (v < minY || v > maxY) return GSM_OUTSIDE;
  const float PO[3] = {P[0] - pose[12], P[1] - pose[13], P[2] - pose[14]};
  double s2 = 0;
  for (int i = 0; i < 3; i++) s2 += (double)PO[i] * (double)PO[i];
  const float dist3D = (float)sqrt(s2);
  const float maxDistance = 1.2f * mfMaxDistance, minDistance = 0.8f * mfMinDistance;   // MapPoint.cpp:825-835
  if (dist3D < minDistance || dist3D > maxDistance) return GSM_RANGE;
  // MapPoint.cpp:854-869.  logf_glibc restates the library's logf for positive normal finite arguments; for every other ratio (dist3D == 0 gives inf or NaN; zero,
  // negative, subnormal) the source's quotient is -inf, +inf, NaN or below -87, which its conversion to int and its clamp turn into level 0 (frame_math.h).
  const float ratio = mfMaxDistance / dist3D;
  if (ratio >= 1.17549435e-38f && ratio <= 3.40282347e+38f) level = fsm_predict_scale(mfMaxDistance, dist3D, logScaleFactor, nlevels);
  radius = th * scaleFactors[level];
  return GSM_SEARCHED;
}
