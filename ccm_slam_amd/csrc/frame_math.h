// frame_math.h — per-frame geometry of cslam::Frame restated for host + device (cslam/src/Frame.cpp:139-330).
// cv::undistortPoints is [EXT] (OpenCV 4.2.0, imgproc/src/undistort.dispatch.cpp, cvUndistortPointsInternal): the call
// at Frame.cpp:298 / :323 passes K (CV_32F, widened to f64), D = (k1 k2 p1 p2 [k3]), R = empty, P = K and the default
// TermCriteria(MAX_ITER, 5, 0.01) => exactly five fixed-point iterations in f64, no epsilon test, result cast to f32.
// The host mirror (host/ccm_host.cpp) compiles this file with g++: its FrameGrid takes frame_cell_range from here.
#pragma once
#include <cmath>
#include "orb_math.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FR_HD __host__ __device__ __forceinline__
#else
#define FR_HD static inline
#endif

constexpr int kGridCols = 75, kGridRows = 48;   // FRAME_GRID_COLS / ROWS (cslam/include/cslam/Frame.h:51-52)

struct FrameCam {
  double fx, fy, cx, cy;      // mK (f32 values widened)
  double k1, k2, p1, p2, k3;  // mDistCoef
};

// one point of cv::undistortPoints(src, dst, K, D, noArray(), K)
FR_HD void frame_undistort_point(const FrameCam& c, float xin, float yin, float& xout, float& yout) {
  const double u = xin, v = yin;
  const double ifx = 1. / c.fx, ify = 1. / c.fy;
  double x = (u - c.cx) * ifx, y = (v - c.cy) * ify;
  const double x0 = x, y0 = y;
  for (int j = 0; j < 5; j++) {
    const double r2 = x * x + y * y;
    // k[5..7] = 0 (rational model unused): numerator is exactly 1
    const double icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
    if (icdist < 0) { x = (u - c.cx) * ifx; y = (v - c.cy) * ify; break; }
    const double deltaX = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + 0 * r2 + 0 * r2 * r2;
    const double deltaY = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + 0 * r2 + 0 * r2 * r2;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  // RR = P * R = K: xx = fx x + 0 y + cx, ww = 1 / (0 x + 0 y + 1)
  const double xx = c.fx * x + 0 * y + c.cx, yy = 0 * x + c.fy * y + c.cy, ww = 1. / (0 * x + 0 * y + 1);
  xout = (float)(xx * ww);
  yout = (float)(yy * ww);
}

struct FrameBounds { float minX, minY, maxX, maxY, wInv, hInv; };

// Frame::PosInGrid (Frame.cpp:254-265): f32 arithmetic, round half away from zero
// A product that no int holds (NaN, Inf, beyond the int range) is undefined in the source; x86 gives INT_MIN, which is < 0, while the device would turn a NaN
// into 0: stated here as "not in the grid" (as kfstore_math.h kfg_cell_of does).  roundf of anything outside (-1, 75) x (-1, 48) is outside the grid anyway.
FR_HD int frame_cell_of(const FrameBounds& b, float x, float y) {
  const float tx = (x - b.minX) * b.wInv, ty = (y - b.minY) * b.hInv;
  if (!(tx > -1.0f && tx < (float)kGridCols) || !(ty > -1.0f && ty < (float)kGridRows)) return -1;
  const int posX = (int)roundf(tx);
  const int posY = (int)roundf(ty);
  if (posX < 0 || posX >= kGridCols || posY < 0 || posY >= kGridRows) return -1;
  return posX * kGridRows + posY;   // mGrid[x][y]: x-major
}

// cell range of Frame::GetFeaturesInArea (Frame.cpp:205-219); returns false when the window misses the grid.
// The source converts floor / ceil of four f32 products to int unchecked, which is undefined for a product no int holds (the device saturates, x86 gives
// INT_MIN), and with r < 0 it can leave x1 < x0 or y1 < y0.  The rule here is total, and the same on host and device:
//  * false (an empty window) when r is NaN or r < 0, and when a product is NaN: a NaN x or y, or inf - inf;
//  * otherwise every product is clamped to [-1, 76] before the conversion.  Both ends lie outside the grid on either axis, so every window whose products an
//    int holds keeps the range the source gives it, and a window that runs beyond the grid, up to +-inf, ends at the grid's rim.
// With r >= 0 and positive wInv, hInv the range returned has x0 <= x1 and y0 <= y1 (subtraction, addition, product, clamp, floor and ceil are monotone).
FR_HD float frame_clamp_cell(float t) { return t < -1.0f ? -1.0f : t > 76.0f ? 76.0f : t; }
FR_HD bool frame_cell_range(const FrameBounds& b, float x, float y, float r, int& x0, int& x1, int& y0, int& y1) {
  const float tx0 = (x - b.minX - r) * b.wInv, tx1 = (x - b.minX + r) * b.wInv;
  const float ty0 = (y - b.minY - r) * b.hInv, ty1 = (y - b.minY + r) * b.hInv;
  if (!(r >= 0.0f)) return false;                                            // NaN or negative radius
  if (tx0 != tx0 || tx1 != tx1 || ty0 != ty0 || ty1 != ty1) return false;    // NaN x or y, inf - inf
  x0 = (int)floorf(frame_clamp_cell(tx0));
  if (x0 < 0) x0 = 0;
  if (x0 >= kGridCols) return false;
  x1 = (int)ceilf(frame_clamp_cell(tx1));
  if (x1 > kGridCols - 1) x1 = kGridCols - 1;
  if (x1 < 0) return false;
  y0 = (int)floorf(frame_clamp_cell(ty0));
  if (y0 < 0) y0 = 0;
  if (y0 >= kGridRows) return false;
  y1 = (int)ceilf(frame_clamp_cell(ty1));
  if (y1 > kGridRows - 1) y1 = kGridRows - 1;
  if (y1 < 0) return false;
  return true;
}

// Frame::isInFrustum (Frame.cpp:139-198) for one map point, [EXT] cv::Mat arithmetic restated:
//  * mRcw*P+mtcw is one cv::gemm(A 3x3, B 3x1, alpha 1, C, beta 1): OpenCV's small-matrix path (core/src/matmul.simd.hpp,
//    case len == 3) forms t = a0*b0 + a1*b1 + a2*b2 in f32, left to right, then d = (float)(t*alpha + c*beta) in f64;
//    the baseline (non-FMA) build is restated — an AVX2-dispatched OpenCV may contract the f32 sum (parity unpinned);
//  * P - mOw in f32; cv::norm (NORM_L2, CV_32F) accumulates v*v in f64 and returns sqrt in f64, stored to a float;
//  * Mat::dot accumulates in f64; viewCos = (float)(dot / (double)dist);
//  * PredictScale: ceil(logf(mfMaxDistance / dist) / mfLogScaleFactor) clamped to [0, nLevels) (MapPoint.cpp:854-869).
struct FrustumFrame {
  float Rcw[9], tcw[3], Ow[3];
  float fx, fy, cx, cy;
  float minX, maxX, minY, maxY;
  float logScaleFactor;
  int nScaleLevels;
};

FR_HD bool frame_in_frustum(const FrustumFrame& f, const float P[3], const float Pn[3], float mfMinDistance, float mfMaxDistance,
                            float viewingCosLimit, float& u_out, float& v_out, int& level_out, float& cos_out) {
  float Pc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float t = f.Rcw[3 * i] * P[0] + f.Rcw[3 * i + 1] * P[1] + f.Rcw[3 * i + 2] * P[2];
    Pc[i] = (float)((double)t * 1.0 + (double)f.tcw[i] * 1.0);
  }
  if (Pc[2] < 0.0f) return false;
  const float invz = 1.0f / Pc[2];
  const float u = f.fx * Pc[0] * invz + f.cx;
  const float v = f.fy * Pc[1] * invz + f.cy;
  if (u < f.minX || u > f.maxX) return false;
  if (v < f.minY || v > f.maxY) return false;
  const float maxDistance = 1.2f * mfMaxDistance, minDistance = 0.8f * mfMinDistance;   // MapPoint.cpp:825-835
  const float PO[3] = {P[0] - f.Ow[0], P[1] - f.Ow[1], P[2] - f.Ow[2]};
  double s2 = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) s2 += (double)PO[i] * PO[i];
  const float dist = (float)sqrt(s2);
  if (dist < minDistance || dist > maxDistance) return false;
  double dot = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) dot += (double)PO[i] * Pn[i];
  const float viewCos = (float)(dot / dist);
  if (viewCos < viewingCosLimit) return false;
  const float ratio = mfMaxDistance / dist;
  // logf_glibc restates the library's logf for positive normal finite arguments only.  Outside them (dist == 0 gives x / 0 = inf or 0 / 0 = NaN; a zero,
  // negative or subnormal ratio) the library returns +-inf, NaN or a value below -87, and the x86 build converts ceil() of the quotient to INT_MIN for the
  // first three and to a negative int for the last: the clamp below turns each into level 0.  (The device's own conversion would saturate inf to INT_MAX.)
  int nScale = 0;
  if (ratio >= 1.17549435e-38f && ratio <= 3.40282347e+38f) nScale = (int)ceilf(orbm::logf_glibc(ratio) / f.logScaleFactor);
  if (nScale < 0) nScale = 0;
  else if (nScale >= f.nScaleLevels) nScale = f.nScaleLevels - 1;
  u_out = u; v_out = v; level_out = nScale; cos_out = viewCos;
  return true;
}
