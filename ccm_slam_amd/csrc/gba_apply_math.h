// gba_apply_math.h — what follows a finished global BA, host + device: the recovery of the f64 estimates into f32 (cslam/src/Optimizer.cpp:803-857,
// Converter.cc:52-74) and the map walk of RunGBA, which the reference carries three times (Map.cpp:1441-1568, LoopFinder.cpp ~895-1010, MapMerger.cpp
// ~640-755).  The kernels of gba_apply.hip run these lines; cslam::GbaMapUpdate (host/ccm_host.cpp) compiles them with g++.
//
// Converter::toCvMat(SE3Quat) is to_homogeneous_matrix() — the rotation of the quaternion AS IT IS (ba_q_to_R of ba_math.h, not normalised, as upstream) and
// the translation — with every element cast to f32; Converter::toCvMat(Vector3d) is three casts.  KeyFrame::SetPose's Rwc = Rcw.t() and Ow = -Rwc * tcw is
// s3c_center of sim3_correct_math.h.  The cv::Mat steps are evaluated as OpenCV 4.2 does in a baseline build (no FMA), with the rules
// oracle/ref_shim/opencv2/mini_cv.h declares.  They are restated from OpenCV's published sources and are NOT pinned against an OpenCV build in this tree:
//   (Tcw_child * Twc_parent) * mTcwGBA_parent   two 4x4 f32 gemms, small-matrix path, each evaluated as s3c_tic: f32 accumulator, the four products added
//                                               left to right, last row 0 0 0 1.  The parenthesisation is the reference's; the three are never composed.
//   Rcw * X + tcw,  Rwc * Xc + twc              ONE cv::gemm(A, B, 1, C, 1) each (frame_math.h:65-66): t = a0*b0 + a1*b1 + a2*b2 in f32 left to right, then
//                                               (float)((double)t * 1.0 + (double)c * 1.0)
// Compile with -ffp-contract=off: no product may fuse into an FMA.  DESIGN.md §17 states the walk's rule.
#pragma once
#include <stdint.h>
#include "sim3_correct_math.h"

#define GBA_HD BA_HD

enum : uint8_t { GBA_PT_UNTOUCHED = 0, GBA_PT_OPTIMISED = 1, GBA_PT_MOVED = 2 };

// Converter::toCvMat(SE3Quat), rows 0..2: mTcwGBA of a keyframe that was a vertex; qt = qx qy qz qw tx ty tz
GBA_HD void gba_pose_of_se3(const double* qt, float T[12]) {
  const BaPose q = ba_load_pose(qt);
  double R[9];
  ba_q_to_R(q, R);
  T[0] = (float)R[0]; T[1] = (float)R[1]; T[2] = (float)R[2]; T[3] = (float)q.tx;
  T[4] = (float)R[3]; T[5] = (float)R[4]; T[6] = (float)R[5]; T[7] = (float)q.ty;
  T[8] = (float)R[6]; T[9] = (float)R[7]; T[10] = (float)R[8]; T[11] = (float)q.tz;
}

// rows 0..2 of the Twc that KeyFrame::SetPose(T) leaves: [Rcw.t() | Ow]
GBA_HD void gba_twc(const float* T, float Twc[12]) {
  float O[3];
  s3c_center(T, O);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    Twc[4 * r] = T[r]; Twc[4 * r + 1] = T[4 + r]; Twc[4 * r + 2] = T[8 + r]; Twc[4 * r + 3] = O[r];
  }
}

// mTcwGBA of a child that was no vertex: Tchildc = GetPose() * Twc of the parent (both before the walk), then Tchildc * the parent's finished mTcwGBA
GBA_HD void gba_child_pose(const float* Tcw_child_old, const float* Twc_parent_old, const float* T_parent_new, float T[12]) {
  float Tchildc[12];
  s3c_tic(Tcw_child_old, Twc_parent_old, Tchildc);
  s3c_tic(Tchildc, T_parent_new, T);
}

// d = A * x + c as one cv::gemm(A, x, 1, c, 1); M holds rows 0..2 of a 4x4: A = M(0..2, 0..2), c = M(0..2, 3)
GBA_HD void gba_gemm_rt(const float* M, const float x[3], float d[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    float t = M[4 * r] * x[0];
    t = t + M[4 * r + 1] * x[1];
    t = t + M[4 * r + 2] * x[2];
    d[r] = (float)((double)t * 1.0 + (double)M[4 * r + 3] * 1.0);
  }
}

// a point that was no vertex moves with its reference keyframe: Xc through mTcwBefGBA, back through the Twc that SetPose left
GBA_HD void gba_move_point(const float* Tcw_ref_old, const float* Twc_ref_new, const float P[3], float out[3]) {
  float Xc[3];
  gba_gemm_rt(Tcw_ref_old, P, Xc);
  gba_gemm_rt(Twc_ref_new, Xc, out);
}

// one point of the walk; the three kinds of the point loop.  Returns the status byte.
GBA_HD uint8_t gba_point(int32_t vert, int32_t ref, const double* pt_xyz, const float* Tcw_old, const float* Twc_new, const float P[3], float out[3]) {
  if (vert >= 0) {
    const double* X = pt_xyz + 3 * (size_t)vert;
    out[0] = (float)X[0]; out[1] = (float)X[1]; out[2] = (float)X[2];
    return GBA_PT_OPTIMISED;
  }
  if (ref >= 0) {
    gba_move_point(Tcw_old + 12 * (size_t)ref, Twc_new + 12 * (size_t)ref, P, out);
    return GBA_PT_MOVED;
  }
  out[0] = P[0]; out[1] = P[1]; out[2] = P[2];
  return GBA_PT_UNTOUCHED;
}

// The checks and the level order shared by ccm_gba_apply_map and its host evaluator.  depth[k]: 0 for a keyframe that was a vertex, else one more than its
// parent's, so a keyframe's depth is its distance below its nearest vertex ancestor.  Returns nullptr, or what is wrong.  An origin that was no vertex has no
// mTcwGBA at all (the reference would set a stale or empty matrix as its pose): it is refused.
inline const char* gba_check_walk(int n_kf, const int32_t* kf_parent, const int32_t* kf_cam, int n_cam, int32_t* depth, int* n_tree, int* max_depth) {
  *n_tree = 0; *max_depth = 0;
  for (int k = 0; k < n_kf; k++) {
    if (kf_parent[k] >= k || kf_parent[k] < -1) return "a parent at or behind its child in the walk";
    if (kf_cam[k] >= n_cam) return "camera index out of range";
    if (kf_cam[k] >= 0) { depth[k] = 0; continue; }
    if (kf_parent[k] < 0) return "an origin that was no vertex";
    depth[k] = depth[kf_parent[k]] + 1;
    if (depth[k] > *max_depth) *max_depth = depth[k];
    ++*n_tree;
  }
  return nullptr;
}

// the keyframes that were no vertices, by depth (walk order inside a level): tree_kf[n_tree], lvl_off[max_depth + 1]
inline void gba_tree_levels(int n_kf, const int32_t* depth, int max_depth, int32_t* tree_kf, int32_t* lvl_off) {
  for (int l = 0; l <= max_depth; l++) lvl_off[l] = 0;
  for (int k = 0; k < n_kf; k++) if (depth[k] > 0) lvl_off[depth[k]]++;   // lvl_off[d] = count of depth d, d >= 1
  int at = 0;
  for (int l = 1; l <= max_depth; l++) { const int c = lvl_off[l]; lvl_off[l - 1] = at; at += c; }
  lvl_off[max_depth] = at;
  // lvl_off[d - 1] is now the start of depth d; fill with a running cursor per level
  int32_t* cur = lvl_off;
  for (int k = 0; k < n_kf; k++) if (depth[k] > 0) tree_kf[cur[depth[k] - 1]++] = k;
  // every cursor ended at the start of the next level: shift back
  for (int l = max_depth; l >= 1; l--) lvl_off[l] = lvl_off[l - 1];
  lvl_off[0] = 0;
}

inline const char* gba_check_points(int n_pt, const int32_t* pt_vert, const int32_t* pt_ref, int n_lm, int n_kf) {
  for (int i = 0; i < n_pt; i++) {
    if (pt_vert[i] >= n_lm) return "landmark index out of range";
    if (pt_ref[i] >= n_kf) return "reference keyframe out of range";
  }
  return nullptr;
}
