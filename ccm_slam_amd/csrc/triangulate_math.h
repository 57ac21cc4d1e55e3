// triangulate_math.h — one match of LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:353-448): ray-parallax gate, linear triangulation
// through cv::SVD::compute on a 4x4 f32 matrix, the two depth tests, the two chi2 reprojection gates and the scale-consistency gate, host + device.
// The kernel of triangulate.hip runs these lines; cslam::NewMapPointBatch (host/ccm_host.cpp) and tests/host/triangulate_check.cpp compile them with g++.
//
// Every step is the reference's cv::Mat expression evaluated as OpenCV 4.2 does in a baseline build (no FMA), with the rules that
// oracle/ref_shim/opencv2/mini_cv.h declares where it declares one (gemm_eval, Mat::dot, norm, Mat / s).  DESIGN.md §12 lists them; the numpy
// checker of tests/test_triangulate_cpu.py restates them independently.  Compile with -ffp-contract=off: no product may fuse into an FMA.
//
// The 4x4 Jacobi keeps At, Vt and W in named scalars of fixed index (the six (i, j) rotations and the sort are written out): nothing is indexed
// dynamically, so on the device the whole state stays in registers (no private segment).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRI_HD __host__ __device__ inline
#else
#define TRI_HD static inline
#endif

enum {
  TRI_OK = 0,          // accepted
  TRI_PARALLAX = 1,    // !(cos > 0 && cos < 0.9998)
  TRI_W_ZERO = 2,      // x3D(3) == 0
  TRI_Z1 = 3,          // z1 <= 0
  TRI_Z2 = 4,          // z2 <= 0
  TRI_REPROJ1 = 5,     // reprojection in KF1
  TRI_REPROJ2 = 6,     // reprojection in KF2
  TRI_DIST_ZERO = 7,   // dist1 == 0 || dist2 == 0
  TRI_SCALE = 8        // scale ratio
};

#define TRI_CAM_FLOATS 21
struct TriCam {
  float Rcw[9];   // GetRotation(), row-major
  float tcw[3];   // GetTranslation()
  float Ow[3];    // GetCameraCenter()
  float fx, fy, cx, cy, invfx, invfy;
};

// hypot of lapack.cpp (template, double here): the scaled form
TRI_HD double tri_hypot(double a, double b) {
  a = fabs(a);
  b = fabs(b);
  if (a > b) {
    b /= a;
    return a * sqrt(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * sqrt(1 + a * a);
  }
  return 0;
}

// double sum of squares / double dot of two rows of four floats, left to right
TRI_HD double tri_sq4(const float* r) {
  double s = 0;
  s += (double)r[0] * r[0]; s += (double)r[1] * r[1]; s += (double)r[2] * r[2]; s += (double)r[3] * r[3];
  return s;
}
TRI_HD double tri_dot4(const float* a, const float* b) {
  double s = 0;
  s += (double)a[0] * b[0]; s += (double)a[1] * b[1]; s += (double)a[2] * b[2]; s += (double)a[3] * b[3];
  return s;
}

// one (i, j) step of a sweep of JacobiSVDImpl_<float> (lapack.cpp), m = n = 4, eps = 2 * FLT_EPSILON.  Ai / Aj: rows of At, Vi / Vj: rows of Vt.
TRI_HD bool tri_rotate(float* Ai, float* Aj, float* Vi, float* Vj, double& Wi, double& Wj) {
  const float eps = FLT_EPSILON * 2;
  double a = Wi, b = Wj;
  double p = tri_dot4(Ai, Aj);
  if (fabs(p) <= eps * sqrt(a * b)) return false;
  p *= 2;
  const double beta = a - b, gamma = tri_hypot(p, beta);
  float c, s;
  if (beta < 0) {
    const double delta = (gamma - beta) * 0.5;
    s = (float)sqrt(delta / gamma);
    c = (float)(p / (gamma * s * 2));
  } else {
    c = (float)sqrt((gamma + beta) / (gamma * 2));
    s = (float)(p / (gamma * c * 2));
  }
  a = b = 0;
#define TRI_GIVENS(k, acc)                          \
  {                                                 \
    const float t0 = c * Ai[k] + s * Aj[k];         \
    const float t1 = -s * Ai[k] + c * Aj[k];        \
    Ai[k] = t0; Aj[k] = t1;                         \
    if (acc) { a += (double)t0 * t0; b += (double)t1 * t1; } \
  }
  TRI_GIVENS(0, true) TRI_GIVENS(1, true) TRI_GIVENS(2, true) TRI_GIVENS(3, true)
  Wi = a; Wj = b;
  {
    float* Ai = Vi; float* Aj = Vj;   // the same rotation on Vt
    TRI_GIVENS(0, false) TRI_GIVENS(1, false) TRI_GIVENS(2, false) TRI_GIVENS(3, false)
  }
#undef TRI_GIVENS
  return true;
}

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 f32 A (row-major): vt.row(3) -> v.  JacobiSVDImpl_<float> on At = A' with Vt = I;
// U's normalisation and completion do not touch Vt and are left out.
TRI_HD void tri_svd4_last_row(const float* A, float v[4]) {
  float At0[4] = {A[0], A[4], A[8], A[12]}, At1[4] = {A[1], A[5], A[9], A[13]}, At2[4] = {A[2], A[6], A[10], A[14]}, At3[4] = {A[3], A[7], A[11], A[15]};
  float Vt0[4] = {1, 0, 0, 0}, Vt1[4] = {0, 1, 0, 0}, Vt2[4] = {0, 0, 1, 0}, Vt3[4] = {0, 0, 0, 1};
  double W0 = tri_sq4(At0), W1 = tri_sq4(At1), W2 = tri_sq4(At2), W3 = tri_sq4(At3);
  for (int iter = 0; iter < 30; iter++) {   // max(m, 30)
    bool changed = false;
    changed |= tri_rotate(At0, At1, Vt0, Vt1, W0, W1);
    changed |= tri_rotate(At0, At2, Vt0, Vt2, W0, W2);
    changed |= tri_rotate(At0, At3, Vt0, Vt3, W0, W3);
    changed |= tri_rotate(At1, At2, Vt1, Vt2, W1, W2);
    changed |= tri_rotate(At1, At3, Vt1, Vt3, W1, W3);
    changed |= tri_rotate(At2, At3, Vt2, Vt3, W2, W3);
    if (!changed) break;
  }
  W0 = sqrt(tri_sq4(At0)); W1 = sqrt(tri_sq4(At1)); W2 = sqrt(tri_sq4(At2)); W3 = sqrt(tri_sq4(At3));
  // selection sort, descending, strict <: equal singular values keep their order.  Only W and Vt are read afterwards, so At's rows stay put.
#define TRI_SWAP(Wa, Va, Wb, Vb)                                                                \
  {                                                                                             \
    const double tw = Wa; Wa = Wb; Wb = tw;                                                     \
    float tv;                                                                                   \
    tv = Va[0]; Va[0] = Vb[0]; Vb[0] = tv; tv = Va[1]; Va[1] = Vb[1]; Vb[1] = tv;               \
    tv = Va[2]; Va[2] = Vb[2]; Vb[2] = tv; tv = Va[3]; Va[3] = Vb[3]; Vb[3] = tv;               \
  }
  {
    int j = 0; double wj = W0;
    if (wj < W1) { j = 1; wj = W1; }
    if (wj < W2) { j = 2; wj = W2; }
    if (wj < W3) { j = 3; wj = W3; }
    if (j == 1) TRI_SWAP(W0, Vt0, W1, Vt1) else if (j == 2) TRI_SWAP(W0, Vt0, W2, Vt2) else if (j == 3) TRI_SWAP(W0, Vt0, W3, Vt3)
  }
  {
    int j = 1; double wj = W1;
    if (wj < W2) { j = 2; wj = W2; }
    if (wj < W3) { j = 3; wj = W3; }
    if (j == 2) TRI_SWAP(W1, Vt1, W2, Vt2) else if (j == 3) TRI_SWAP(W1, Vt1, W3, Vt3)
  }
  if (W2 < W3) TRI_SWAP(W2, Vt2, W3, Vt3)
#undef TRI_SWAP
  v[0] = Vt3[0]; v[1] = Vt3[1]; v[2] = Vt3[2]; v[3] = Vt3[3];
}

// Rcw.row(r).dot(x3Dt) + tcw(r): Mat::dot in double, a double add, then the float
TRI_HD float tri_row(const float* R, float t, const float* X) {
  double d = 0;
  d += (double)R[0] * X[0]; d += (double)R[1] * X[1]; d += (double)R[2] * X[2];
  return (float)(d + (double)t);
}

// cv::norm(x3D - Ow): f32 difference, normL2Sqr in double, sqrt, the float
TRI_HD float tri_dist(const float* X, const float* O) {
  const float d0 = X[0] - O[0], d1 = X[1] - O[1], d2 = X[2] - O[2];
  double s = 0;
  s += (double)d0 * d0; s += (double)d1 * d1; s += (double)d2 * d2;
  return (float)sqrt(s);
}

// squared reprojection error of x3D in a keyframe whose depth z is known, compared as the reference does: float sum > 5.991 * sigma2 in double
TRI_HD bool tri_reproj_fails(const TriCam& c, const float* X, float z, float kx, float ky, float sigma2) {
  const float x = tri_row(c.Rcw + 0, c.tcw[0], X);
  const float y = tri_row(c.Rcw + 3, c.tcw[1], X);
  const float invz = (float)(1.0 / (double)z);
  const float u = c.fx * x * invz + c.cx;
  const float v = c.fy * y * invz + c.cy;
  const float ex = u - kx, ey = v - ky;
  return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
}

// One match.  Returns the first gate of the reference at which the pair leaves the loop (TRI_*); x3D: the value reached so far (NaN before the SVD,
// vt.row(3)'s first three entries when its fourth is zero, the Euclidean point afterwards).
TRI_HD int tri_pair(const TriCam& c1, const TriCam& c2, float kx1, float ky1, int oct1, float kx2, float ky2, int oct2, const float* sigma2_1,
                    const float* sf_1, const float* sigma2_2, const float* sf_2, float ratioFactor, float x3D[3]) {
  // xn = ((x - cx) * invfx, (y - cy) * invfy, 1)
  const float a1 = (kx1 - c1.cx) * c1.invfx, b1 = (ky1 - c1.cy) * c1.invfy;
  const float a2 = (kx2 - c2.cx) * c2.invfx, b2 = (ky2 - c2.cy) * c2.invfy;
  // ray = Rwc * xn, Rwc = Rcw.t() materialised: small-matrix gemm, f32 accumulator left to right
  float r1[3], r2[3];
  r1[0] = c1.Rcw[0] * a1 + c1.Rcw[3] * b1 + c1.Rcw[6] * 1.0f;
  r1[1] = c1.Rcw[1] * a1 + c1.Rcw[4] * b1 + c1.Rcw[7] * 1.0f;
  r1[2] = c1.Rcw[2] * a1 + c1.Rcw[5] * b1 + c1.Rcw[8] * 1.0f;
  r2[0] = c2.Rcw[0] * a2 + c2.Rcw[3] * b2 + c2.Rcw[6] * 1.0f;
  r2[1] = c2.Rcw[1] * a2 + c2.Rcw[4] * b2 + c2.Rcw[7] * 1.0f;
  r2[2] = c2.Rcw[2] * a2 + c2.Rcw[5] * b2 + c2.Rcw[8] * 1.0f;
  double dot = 0, n1 = 0, n2 = 0;
  dot += (double)r1[0] * r2[0]; dot += (double)r1[1] * r2[1]; dot += (double)r1[2] * r2[2];
  n1 += (double)r1[0] * r1[0]; n1 += (double)r1[1] * r1[1]; n1 += (double)r1[2] * r1[2];
  n2 += (double)r2[0] * r2[0]; n2 += (double)r2[1] * r2[1]; n2 += (double)r2[2] * r2[2];
  const float cosParallaxRays = (float)(dot / (sqrt(n1) * sqrt(n2)));
  const float cosParallaxStereo = cosParallaxRays + 1;
  if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && ((double)cosParallaxRays < 0.9998))) {
    x3D[0] = x3D[1] = x3D[2] = NAN;
    return TRI_PARALLAX;
  }
  // A.row = xn(k) * Tcw.row(2) - Tcw.row(k): f32 multiply, f32 subtract
  float A[16];
  A[0] = a1 * c1.Rcw[6] - c1.Rcw[0]; A[1] = a1 * c1.Rcw[7] - c1.Rcw[1]; A[2] = a1 * c1.Rcw[8] - c1.Rcw[2]; A[3] = a1 * c1.tcw[2] - c1.tcw[0];
  A[4] = b1 * c1.Rcw[6] - c1.Rcw[3]; A[5] = b1 * c1.Rcw[7] - c1.Rcw[4]; A[6] = b1 * c1.Rcw[8] - c1.Rcw[5]; A[7] = b1 * c1.tcw[2] - c1.tcw[1];
  A[8] = a2 * c2.Rcw[6] - c2.Rcw[0]; A[9] = a2 * c2.Rcw[7] - c2.Rcw[1]; A[10] = a2 * c2.Rcw[8] - c2.Rcw[2]; A[11] = a2 * c2.tcw[2] - c2.tcw[0];
  A[12] = b2 * c2.Rcw[6] - c2.Rcw[3]; A[13] = b2 * c2.Rcw[7] - c2.Rcw[4]; A[14] = b2 * c2.Rcw[8] - c2.Rcw[5]; A[15] = b2 * c2.tcw[2] - c2.tcw[1];
  float v[4];
  tri_svd4_last_row(A, v);
  if (v[3] == 0) {
    x3D[0] = v[0]; x3D[1] = v[1]; x3D[2] = v[2];
    return TRI_W_ZERO;
  }
  // x3D.rowRange(0, 3) / w: convertTo with alpha = 1. / w, x * (float)alpha + 0.f
  const float inv = (float)(1. / (double)v[3]);
  x3D[0] = v[0] * inv + 0.0f; x3D[1] = v[1] * inv + 0.0f; x3D[2] = v[2] * inv + 0.0f;
  const float z1 = tri_row(c1.Rcw + 6, c1.tcw[2], x3D);
  if (z1 <= 0) return TRI_Z1;
  const float z2 = tri_row(c2.Rcw + 6, c2.tcw[2], x3D);
  if (z2 <= 0) return TRI_Z2;
  if (tri_reproj_fails(c1, x3D, z1, kx1, ky1, sigma2_1[oct1])) return TRI_REPROJ1;
  if (tri_reproj_fails(c2, x3D, z2, kx2, ky2, sigma2_2[oct2])) return TRI_REPROJ2;
  const float dist1 = tri_dist(x3D, c1.Ow), dist2 = tri_dist(x3D, c2.Ow);
  if (dist1 == 0 || dist2 == 0) return TRI_DIST_ZERO;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = sf_1[oct1] / sf_2[oct2];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return TRI_SCALE;
  return TRI_OK;
}
