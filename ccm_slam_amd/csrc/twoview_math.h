// twoview_math.h — the arithmetic of cslam::Initializer (cslam/src/Initializer.cpp) between SearchForInitialization and the accept / reject logic of
// ReconstructF / ReconstructH, host + device: Normalize (:745-791), ComputeH21 / ComputeF21 (:222-299) with the products around them (:155-157, :206-208),
// CheckHomography / CheckFundamental (:301-464) and one match of CheckRT (:794-903).  The kernels of twoview.hip run these lines; cslam::TwoViewInitializer
// (host/ccm_host.cpp) compiles them with g++.
//
// Every step is the reference's expression evaluated as OpenCV 4.2 does in a baseline build (no FMA), with the rules of triangulate_math.h where one applies
// (tri_svd4_last_row, cv::norm, Mat::dot, the one-gemm R * X + t) and of oracle/ref_shim/opencv2/mini_cv.h (gemm_eval).  DESIGN.md §18 lists what is restated
// here: cv::SVDecomp(A, w, u, vt, MODIFY_A | FULL_UV) for 16x9, 8x9 and 3x3 f32 matrices (JacobiSVDImpl_<float> with the normalisation of At's rows and the
// RNG completion of the rows without a singular value) and Mat::inv() of a 3x3 f32.  Both were written from memory of OpenCV 4.2.  Compile with
// -ffp-contract=off: no product may fuse into an FMA.
//
// Every loop has a fixed bound (30 sweeps, 100 completion tries, the number of matches).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "triangulate_math.h"

#define TV_HD TRI_HD

enum {
  TV_NOT_INLIER = 0,   // the mask bit is clear
  TV_NONFINITE = 1,    // !isfinite(p3dC1)
  TV_DEPTH1 = 2,       // p3dC1(2) <= 0 && cosParallax < 0.99998
  TV_DEPTH2 = 3,       // p3dC2(2) <= 0 && cosParallax < 0.99998
  TV_REPROJ1 = 4,      // squareError1 > th2
  TV_REPROJ2 = 5,      // squareError2 > th2
  TV_COUNTED = 6,      // nGood++, vbGood stays false (cosParallax >= 0.99998)
  TV_GOOD = 7          // nGood++ and vbGood
};

// one motion hypothesis of CheckRT (:810-822), from tv_prepare_rt
#define TV_REC_FLOATS 27
struct TvMotion {
  float P2[12];   // K * [R | t], row-major 3x4
  float O2[3];    // -R.t() * t
  float R[9];
  float t[3];
};

// ---- 3x3 helpers ------------------------------------------------------------------------------------------------------------------------------
// C = A * B for 3x3 f32: the small-matrix path of cv::gemm (len 3): f32 accumulator, the three products added left to right, (float)(t * 1.0 + 0.0)
TV_HD void tv_mul33(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      const float t = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
      C[3 * r + c] = (float)((double)t * 1.0 + 0.0);
    }
}

// Mat::inv() (DECOMP_LU) of a 3x3 f32: determinant and cofactors in double, (float)(cofactor * (1. / det)); all zeros when det == 0
TV_HD void tv_inv33(const float* S, float* D) {
#define TV_S(r, c) ((double)S[3 * (r) + (c)])
  double d = TV_S(0, 0) * (TV_S(1, 1) * TV_S(2, 2) - TV_S(1, 2) * TV_S(2, 1)) - TV_S(0, 1) * (TV_S(1, 0) * TV_S(2, 2) - TV_S(1, 2) * TV_S(2, 0)) +
             TV_S(0, 2) * (TV_S(1, 0) * TV_S(2, 1) - TV_S(1, 1) * TV_S(2, 0));
  if (d != 0.) {
    d = 1. / d;
    D[0] = (float)((TV_S(1, 1) * TV_S(2, 2) - TV_S(1, 2) * TV_S(2, 1)) * d);
    D[1] = (float)((TV_S(0, 2) * TV_S(2, 1) - TV_S(0, 1) * TV_S(2, 2)) * d);
    D[2] = (float)((TV_S(0, 1) * TV_S(1, 2) - TV_S(0, 2) * TV_S(1, 1)) * d);
    D[3] = (float)((TV_S(1, 2) * TV_S(2, 0) - TV_S(1, 0) * TV_S(2, 2)) * d);
    D[4] = (float)((TV_S(0, 0) * TV_S(2, 2) - TV_S(0, 2) * TV_S(2, 0)) * d);
    D[5] = (float)((TV_S(0, 2) * TV_S(1, 0) - TV_S(0, 0) * TV_S(1, 2)) * d);
    D[6] = (float)((TV_S(1, 0) * TV_S(2, 1) - TV_S(1, 1) * TV_S(2, 0)) * d);
    D[7] = (float)((TV_S(0, 1) * TV_S(2, 0) - TV_S(0, 0) * TV_S(2, 1)) * d);
    D[8] = (float)((TV_S(0, 0) * TV_S(1, 1) - TV_S(0, 1) * TV_S(1, 0)) * d);
  } else {
    for (int i = 0; i < 9; i++) D[i] = 0.f;
  }
#undef TV_S
}

// ---- Normalize (:745-791) ---------------------------------------------------------------------------------------------------------------------
// xy: the n undistorted keypoints of a frame (x y pairs), all of them; pn: n normalised points; T: 3x3 row-major.  The f32 sums run left to right.
TV_HD void tv_normalize(const float* xy, int n, float* pn, float* T) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
  meanX = meanX / (float)n; meanY = meanY / (float)n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    pn[2 * i] = xy[2 * i] - meanX; pn[2 * i + 1] = xy[2 * i + 1] - meanY;
    meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
  }
  meanDevX = meanDevX / (float)n; meanDevY = meanDevY / (float)n;
  const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
  for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
  T[0] = sX; T[1] = 0; T[2] = -meanX * sX;
  T[3] = 0; T[4] = sY; T[5] = -meanY * sY;
  T[6] = 0; T[7] = 0; T[8] = 1;
}

// ---- JacobiSVDImpl_<float> (lapack.cpp) ---------------------------------------------------------------------------------------------------------
// At: NR rows of M floats, the first N of them the rows of the problem (NR = max(N, n1)); Vt: N x N or nullptr where nobody reads it (the rows of At are
// still swapped by the sort, as they are when OpenCV has a Vt); w: N singular values or nullptr; n1: rows of At that are normalised / completed (0: none —
// neither touches Vt).  minval = FLT_MIN, eps = 2 * FLT_EPSILON.  The body is OpenCV's template on the element type T: pnp_math.h runs it on doubles.
TV_HD float tv_svd_eps(const float*) { return FLT_EPSILON * 2; }
TV_HD double tv_svd_eps(const double*) { return DBL_EPSILON * 10; }   // JacobiSVDImpl_<double>: 10 * DBL_EPSILON, minval = DBL_MIN
TV_HD double tv_svd_minval(const float*) { return FLT_MIN; }
TV_HD double tv_svd_minval(const double*) { return DBL_MIN; }
TV_HD float tv_abs(float x) { return fabsf(x); }
TV_HD double tv_abs(double x) { return fabs(x); }

template <typename T, int M, int N, int NR>
TV_HD void tv_jacobi_svd_t(T* At, T* Vt, T* w, int n1) {
  const T eps = tv_svd_eps((const T*)nullptr);
  const double minval = tv_svd_minval((const T*)nullptr);
  double W[N];
  for (int i = 0; i < N; i++) {
    double sd = 0;
    for (int k = 0; k < M; k++) { const T t = At[i * M + k]; sd += (double)t * t; }
    W[i] = sd;
    if (Vt) {
      for (int k = 0; k < N; k++) Vt[i * N + k] = 0;
      Vt[i * N + i] = 1;
    }
  }
  for (int iter = 0; iter < 30; iter++) {   // max(m, 30) with m <= 16
    bool changed = false;
    int i = 0, j = 0;
    for (int ij = 0; ij < N * (N - 1) / 2; ij++) {   // the pairs i < j in the reference's order, as one loop
      if (++j == N) { i++; j = i + 1; }
      T* Ai = At + i * M;
      T* Aj = At + j * M;
      double a = W[i], p = 0, b = W[j];
      for (int k = 0; k < M; k++) p += (double)Ai[k] * Aj[k];
      if (fabs(p) <= eps * sqrt(a * b)) continue;
      p *= 2;
      const double beta = a - b, gamma = tri_hypot(p, beta);
      T c, s;
      if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = (T)sqrt(delta / gamma);
        c = (T)(p / (gamma * s * 2));
      } else {
        c = (T)sqrt((gamma + beta) / (gamma * 2));
        s = (T)(p / (gamma * c * 2));
      }
      a = b = 0;
      for (int k = 0; k < M; k++) {
        const T t0 = c * Ai[k] + s * Aj[k];
        const T t1 = -s * Ai[k] + c * Aj[k];
        Ai[k] = t0; Aj[k] = t1;
        a += (double)t0 * t0; b += (double)t1 * t1;
      }
      W[i] = a; W[j] = b;
      changed = true;
      if (Vt) {
        T* Vi = Vt + i * N;
        T* Vj = Vt + j * N;
        for (int k = 0; k < N; k++) {
          const T t0 = c * Vi[k] + s * Vj[k];
          const T t1 = -s * Vi[k] + c * Vj[k];
          Vi[k] = t0; Vj[k] = t1;
        }
      }
    }
    if (!changed) break;
  }
  for (int i = 0; i < N; i++) {
    double sd = 0;
    for (int k = 0; k < M; k++) { const T t = At[i * M + k]; sd += (double)t * t; }
    W[i] = sqrt(sd);
  }
  // selection sort, descending, strict <: equal singular values keep their order
  for (int i = 0; i < N - 1; i++) {
    int j = i;
    for (int k = i + 1; k < N; k++)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      const double tw = W[i]; W[i] = W[j]; W[j] = tw;
      for (int k = 0; k < M; k++) { const T t = At[i * M + k]; At[i * M + k] = At[j * M + k]; At[j * M + k] = t; }
      if (Vt)
        for (int k = 0; k < N; k++) { const T t = Vt[i * N + k]; Vt[i * N + k] = Vt[j * N + k]; Vt[j * N + k] = t; }
    }
  }
  if (w)
    for (int i = 0; i < N; i++) w[i] = (T)W[i];
  // the rows of At become the left singular vectors: normalised, and completed where the singular value is not above FLT_MIN (all rows i >= N)
  uint64_t rng = 0x12345678u;   // cv::RNG(0x12345678), fresh for each decomposition
  for (int i = 0; i < n1 && i < NR; i++) {
    T* Ai = At + i * M;
    double sd = i < N ? W[i] : 0;
    for (int ii = 0; ii < 100 && sd <= minval; ii++) {
      const T val0 = (T)(1. / M);
      for (int k = 0; k < M; k++) {
        rng = (uint64_t)(uint32_t)rng * 4164903690u + (uint32_t)(rng >> 32);
        Ai[k] = ((uint32_t)rng & 256u) != 0 ? val0 : -val0;
      }
      for (int pass = 0; pass < 2; pass++)
        for (int j = 0; j < i; j++) {
          const T* Aj = At + j * M;
          sd = 0;
          for (int k = 0; k < M; k++) sd += Ai[k] * Aj[k];   // a T product added to a double
          T asum = 0;
          for (int k = 0; k < M; k++) {
            const T t = (T)((double)Ai[k] - sd * (double)Aj[k]);
            Ai[k] = t;
            asum += tv_abs(t);
          }
          asum = asum > eps * 100 ? 1 / asum : 0;
          for (int k = 0; k < M; k++) Ai[k] *= asum;
        }
      sd = 0;
      for (int k = 0; k < M; k++) { const T t = Ai[k]; sd += (double)t * t; }
      sd = sqrt(sd);
    }
    const T s = (T)(sd > minval ? 1 / sd : 0.);
    for (int k = 0; k < M; k++) Ai[k] *= s;
  }
}

template <int M, int N, int NR>
TV_HD void tv_jacobi_svd(float* At, float* Vt, float* w, int n1) { tv_jacobi_svd_t<float, M, N, NR>(At, Vt, w, n1); }

// cv::SVDecomp(A, w, u, vt, MODIFY_A | FULL_UV) on a 16x9 f32 A (row-major): vt.row(8) -> v.  At = A' (9 rows of 16), Vt = I; the normalisation and
// completion of U's rows do not touch Vt and are left out.
TV_HD void tv_svd16x9_last_row(const float* A, float v[9]) {
  float At[9 * 16], Vt[81];
  for (int i = 0; i < 9; i++)
    for (int k = 0; k < 16; k++) At[i * 16 + k] = A[k * 9 + i];
  tv_jacobi_svd<16, 9, 9>(At, Vt, nullptr, 0);
  for (int k = 0; k < 9; k++) v[k] = Vt[72 + k];
}

// the same on an 8x9 f32 A: m < n, so OpenCV runs the 9x8 problem on A's rows themselves (m = 9, n = 8, n1 = 9); vt is the completed U' and vt.row(8) the
// completed ninth row.  vt (81 floats) is A's storage with one more row.
TV_HD void tv_svd8x9_vt(float* vt /* rows 0..7 = A on entry */) {
  for (int k = 0; k < 9; k++) vt[72 + k] = 0;
  tv_jacobi_svd<9, 8, 9>(vt, nullptr, nullptr, 9);
}

// the same on a 3x3 f32 A: w, u (row-major) and vt
TV_HD void tv_svd3x3(const float* A, float w[3], float u[9], float vt[9]) {
  float At[9];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
  tv_jacobi_svd<3, 3, 3>(At, vt, w, 3);
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) u[i * 3 + k] = At[k * 3 + i];
}

// ---- ComputeH21 / ComputeF21 (:222-299) and the products of :155-157 / :206-208 -----------------------------------------------------------------------
// p1 / p2: the eight normalised points of the set (x y pairs)
TV_HD void tv_compute_h21(const float* p1, const float* p2, float Hn[9]) {
  float A[16 * 9];
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    float* r = A + 18 * i;
    r[0] = 0; r[1] = 0; r[2] = 0; r[3] = -u1; r[4] = -v1; r[5] = -1; r[6] = v2 * u1; r[7] = v2 * v1; r[8] = v2;
    r[9] = u1; r[10] = v1; r[11] = 1; r[12] = 0; r[13] = 0; r[14] = 0; r[15] = -u2 * u1; r[16] = -u2 * v1; r[17] = -u2;
  }
  tv_svd16x9_last_row(A, Hn);
}

TV_HD void tv_compute_f21(const float* p1, const float* p2, float Fn[9]) {
  float vt[81];
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    float* r = vt + 9 * i;
    r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1;
  }
  tv_svd8x9_vt(vt);
  float w[3], u[9], vt3[9];
  tv_svd3x3(vt + 72, w, u, vt3);
  w[2] = 0;
  // (u * diag(w)) * vt: two small-matrix gemms, diag(w) a full 3x3 with its zeros
  const float D[9] = {w[0], 0, 0, 0, w[1], 0, 0, 0, w[2]};
  float uD[9];
  tv_mul33(u, D, uD);
  tv_mul33(uD, vt3, Fn);
}

// H21i = (T2inv * Hn) * T1, H12i = H21i.inv()
TV_HD void tv_model_h(const float* p1, const float* p2, const float* T1, const float* T2inv, float H21[9], float H12[9]) {
  float Hn[9], tmp[9];
  tv_compute_h21(p1, p2, Hn);
  tv_mul33(T2inv, Hn, tmp);
  tv_mul33(tmp, T1, H21);
  tv_inv33(H21, H12);
}

// F21i = (T2t * Fn) * T1
TV_HD void tv_model_f(const float* p1, const float* p2, const float* T1, const float* T2t, float F21[9]) {
  float Fn[9], tmp[9];
  tv_compute_f21(p1, p2, Fn);
  tv_mul33(T2t, Fn, tmp);
  tv_mul33(tmp, T1, F21);
}

// ---- CheckHomography / CheckFundamental (:301-464): one match ---------------------------------------------------------------------------------------
// invSigmaSquare = 1.0 / (sigma * sigma): a float product, a double quotient, the float
TV_HD float tv_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// adds the match's two terms to score in the reference's order; returns bIn
TV_HD bool tv_check_h(const float* h, const float* hi, float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
  const float th = 5.991f;
  bool bIn = true;
  const float w2in1inv = (float)(1.0 / (double)(hi[6] * u2 + hi[7] * v2 + hi[8]));
  const float u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
  const float v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else score += th - chiSquare1;
  const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
  const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
  const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else score += th - chiSquare2;
  return bIn;
}

TV_HD bool tv_check_f(const float* f, float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float a2 = f[0] * u1 + f[1] * v1 + f[2];
  const float b2 = f[3] * u1 + f[4] * v1 + f[5];
  const float c2 = f[6] * u1 + f[7] * v1 + f[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else score += thScore - chiSquare1;
  const float a1 = f[0] * u2 + f[3] * v2 + f[6];
  const float b1 = f[1] * u2 + f[4] * v2 + f[7];
  const float c1 = f[2] * u2 + f[5] * v2 + f[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else score += thScore - chiSquare2;
  return bIn;
}

// The whole walk of one model over the N matches: the sequential f32 score and one inlier bit per match (bit i % 32 of word i / 32; mask holds
// ceil(N / 32) words).  hi is read for the homography only.
TV_HD float tv_score(bool homography, const float* m, const float* hi, int N, const float* xy1, const float* xy2, float sigma, uint32_t* mask) {
  const float inv = tv_inv_sigma2(sigma);
  float score = 0;
  uint32_t word = 0;
  for (int i = 0; i < N; i++) {
    const float u1 = xy1[2 * i], v1 = xy1[2 * i + 1], u2 = xy2[2 * i], v2 = xy2[2 * i + 1];
    const bool in = homography ? tv_check_h(m, hi, u1, v1, u2, v2, inv, score) : tv_check_f(m, u1, v1, u2, v2, inv, score);
    word |= (uint32_t)in << (i & 31);
    if ((i & 31) == 31 || i == N - 1) { mask[i >> 5] = word; word = 0; }
  }
  return score;
}

// ---- CheckRT (:794-903) -------------------------------------------------------------------------------------------------------------------------
// P2 = K * [R | t] (small-matrix gemm, f32 accumulator left to right); O2 = -R.t() * t (one gemm with a transposed operand: double accumulator left to
// right, times alpha = -1, the float).  K, R: 3x3 row-major.
TV_HD void tv_prepare_rt(const float* K, const float* R, const float* t, TvMotion& m) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
      const float s = K[3 * r] * b0 + K[3 * r + 1] * b1 + K[3 * r + 2] * b2;
      m.P2[4 * r + c] = (float)((double)s * 1.0 + 0.0);
    }
  for (int r = 0; r < 3; r++) {
    double s = 0;
    s += (double)R[r] * (double)t[0]; s += (double)R[3 + r] * (double)t[1]; s += (double)R[6 + r] * (double)t[2];
    m.O2[r] = (float)(s * -1.0 + 0.0);
  }
  for (int i = 0; i < 9; i++) m.R[i] = R[i];
  for (int i = 0; i < 3; i++) m.t[i] = t[i];
}

// One inlier match under one hypothesis.  Returns the first gate at which the reference's loop `continue`s (TV_NONFINITE .. TV_GOOD); x3D: the point of
// Triangulate (:730-743); cosParallax: NaN for TV_NONFINITE.  K: 3x3 row-major (P1 = K * [I | 0] holds its entries and zeros).
TV_HD int tv_check_rt(const float* K, const TvMotion& m, float x1, float y1, float x2, float y2, float th2, float x3D[3], float& cosParallax) {
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  // A.row = pt * P.row(2) - P.row(k): f32 multiply, f32 subtract
  float A[16];
  for (int c = 0; c < 4; c++) {
    const float p0 = c < 3 ? K[c] : 0.f, p1 = c < 3 ? K[3 + c] : 0.f, p2 = c < 3 ? K[6 + c] : 0.f;
    A[c] = x1 * p2 - p0;
    A[4 + c] = y1 * p2 - p1;
    A[8 + c] = x2 * m.P2[8 + c] - m.P2[c];
    A[12 + c] = y2 * m.P2[8 + c] - m.P2[4 + c];
  }
  float v[4];
  tri_svd4_last_row(A, v);
  // x3D.rowRange(0, 3) / x3D(3): convertTo with alpha = 1. / w, x * (float)alpha + 0.f
  const float inv = (float)(1. / (double)v[3]);
  x3D[0] = v[0] * inv + 0.0f; x3D[1] = v[1] * inv + 0.0f; x3D[2] = v[2] * inv + 0.0f;
  if (!isfinite(x3D[0]) || !isfinite(x3D[1]) || !isfinite(x3D[2])) {
    cosParallax = NAN;
    return TV_NONFINITE;
  }
  // normal1 = p3dC1 - O1 with O1 = 0, normal2 = p3dC1 - O2 in f32; cv::norm and Mat::dot in double; dist1 * dist2 is a float product
  const float O1[3] = {0.f, 0.f, 0.f};
  const float n1[3] = {x3D[0] - O1[0], x3D[1] - O1[1], x3D[2] - O1[2]};
  const float n2[3] = {x3D[0] - m.O2[0], x3D[1] - m.O2[1], x3D[2] - m.O2[2]};
  const float dist1 = tri_dist(x3D, O1), dist2 = tri_dist(x3D, m.O2);
  double dot = 0;
  dot += (double)n1[0] * n2[0]; dot += (double)n1[1] * n2[1]; dot += (double)n1[2] * n2[2];
  cosParallax = (float)(dot / (double)(dist1 * dist2));
  const bool low = !((double)cosParallax < 0.99998);
  if (x3D[2] <= 0 && !low) return TV_DEPTH1;
  // p3dC2 = R * p3dC1 + t: one gemm with C = t
  float X2[3];
  for (int r = 0; r < 3; r++) {
    const float s = m.R[3 * r] * x3D[0] + m.R[3 * r + 1] * x3D[1] + m.R[3 * r + 2] * x3D[2];
    X2[r] = (float)((double)s * 1.0 + (double)m.t[r] * 1.0);
  }
  if (X2[2] <= 0 && !low) return TV_DEPTH2;
  const float invZ1 = (float)(1.0 / (double)x3D[2]);
  const float im1x = fx * x3D[0] * invZ1 + cx, im1y = fy * x3D[1] * invZ1 + cy;
  const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (squareError1 > th2) return TV_REPROJ1;
  const float invZ2 = (float)(1.0 / (double)X2[2]);
  const float im2x = fx * X2[0] * invZ2 + cx, im2y = fy * X2[1] * invZ2 + cy;
  const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (squareError2 > th2) return TV_REPROJ2;
  return low ? TV_COUNTED : TV_GOOD;
}
