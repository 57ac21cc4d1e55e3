// sim3_ransac_math.h — one hypothesis of cslam::Sim3Solver (cslam/src/Sim3Solver.cpp): ComputeCentroid / ComputeSim3 (:199-321) on three
// correspondences and the per-point test of CheckInliers with Project / FromCameraToImage (:324-348, :366-407), host + device, and at the end the
// two as the host + device members of a form of ransac_wave.h.  The kernel of sim3ransac.hip runs these lines; tests/host/sim3_hyp_check.cpp
// walks them with g++.
//
// Every step is the reference's cv::Mat expression evaluated as OpenCV 4.2 does in a baseline build (no HAVE_EIGEN, no FMA), with the
// product rules that oracle/ref_shim/opencv2/mini_cv.h declares (gemm_eval, Mat::dot, convertTo).  DESIGN.md §11 lists them; the numpy
// checker of tests/test_sim3_ransac_gpu.py restates them independently.  Compile with -ffp-contract=off: no product may fuse into an FMA.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define S3_HD __host__ __device__ inline
#define S3_HDM __host__ __device__
#else
#define S3_HD static inline
#define S3_HDM
#endif

struct S3Hyp {
  float R[9];      // mR12i (row-major)
  float t[3];      // mt12i
  float s;         // ms12i
  float sR[9];     // mT12i rows 0..2, cols 0..2 = ms12i * mR12i
  float sRi[9];    // mT21i rows 0..2, cols 0..2 = (1.0 / ms12i) * mR12i.t()
  float ti[3];     // mT21i col 3 = -sRinv * mt12i
};

// cv::hypot of lapack.cpp (template, float here): the Jacobi rotation's hypot
S3_HD float s3_hypot(float a, float b) {
  a = fabsf(a);
  b = fabsf(b);
  if (a > b) {
    b /= a;
    return a * sqrtf(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * sqrtf(1 + a * a);
  }
  return 0;
}

// hal::Jacobi -> JacobiImpl_<float> (lapack.cpp) on a 4x4 symmetric A (row-major, upper triangle used, destroyed): W = eigenvalues, V = eigenvectors
// as rows, both sorted by descending eigenvalue.  eps = FLT_EPSILON, at most n*n*30 rotations.
S3_HD void s3_jacobi4(float* A, float* W, float* V) {
  const int n = 4;
  const float eps = FLT_EPSILON;
  int indR[4], indC[4];
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) V[i * n + j] = 0.f;
    V[i * n + i] = 1.f;
  }
  int i, k, m, l;
  float mv = 0.f;
  for (k = 0; k < n; k++) {
    W[k] = A[(n + 1) * k];
    if (k < n - 1) {
      for (m = k + 1, mv = fabsf(A[n * k + m]), i = k + 2; i < n; i++) {
        float val = fabsf(A[n * k + i]);
        if (mv < val) mv = val, m = i;
      }
      indR[k] = m;
    }
    if (k > 0) {
      for (m = 0, mv = fabsf(A[k]), i = 1; i < k; i++) {
        float val = fabsf(A[n * i + k]);
        if (mv < val) mv = val, m = i;
      }
      indC[k] = m;
    }
  }
  for (int iters = 0; iters < n * n * 30; iters++) {
    for (k = 0, mv = fabsf(A[indR[0]]), i = 1; i < n - 1; i++) {
      float val = fabsf(A[n * i + indR[i]]);
      if (mv < val) mv = val, k = i;
    }
    l = indR[k];
    for (i = 1; i < n; i++) {
      float val = fabsf(A[n * indC[i] + i]);
      if (mv < val) mv = val, k = indC[i], l = i;
    }
    float p = A[n * k + l];
    if (fabsf(p) <= eps) break;
    float y = (float)((double)(W[l] - W[k]) * 0.5);
    float t = fabsf(y) + s3_hypot(p, y);
    float s = s3_hypot(p, t);
    float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) s = -s, t = -t;
    A[n * k + l] = 0;
    W[k] -= t;
    W[l] += t;
    float a0, b0;
#define S3_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
    for (i = 0; i < k; i++) S3_ROT(A[n * i + k], A[n * i + l]);
    for (i = k + 1; i < l; i++) S3_ROT(A[n * k + i], A[n * i + l]);
    for (i = l + 1; i < n; i++) S3_ROT(A[n * k + i], A[n * l + i]);
    for (i = 0; i < n; i++) S3_ROT(V[n * k + i], V[n * l + i]);
#undef S3_ROT
    for (int j = 0; j < 2; j++) {
      int idx = j == 0 ? k : l;
      if (idx < n - 1) {
        for (m = idx + 1, mv = fabsf(A[n * idx + m]), i = idx + 2; i < n; i++) {
          float val = fabsf(A[n * idx + i]);
          if (mv < val) mv = val, m = i;
        }
        indR[idx] = m;
      }
      if (idx > 0) {
        for (m = 0, mv = fabsf(A[idx]), i = 1; i < idx; i++) {
          float val = fabsf(A[n * i + idx]);
          if (mv < val) mv = val, m = i;
        }
        indC[idx] = m;
      }
    }
  }
  for (k = 0; k < n - 1; k++) {   // selection sort, descending, strict <: equal eigenvalues keep their order
    m = k;
    for (i = k + 1; i < n; i++)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      float tw = W[m]; W[m] = W[k]; W[k] = tw;
      for (i = 0; i < n; i++) { float tv = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = tv; }
    }
  }
}

// small-matrix path of cv::gemm for a 3x3 float times a 3-vector (matmul.simd.hpp gemmImpl, len 3): float accumulator, then (float)(t*alpha + c*beta)
S3_HD float s3_gemm3(const float* a_row, float b0, float b1, float b2, double alpha, double c) {
  float t = a_row[0] * b0 + a_row[1] * b1 + a_row[2] * b2;
  return (float)((double)t * alpha + c);
}

S3_HD void s3_transforms(S3Hyp& h);

// ComputeSim3(P1, P2) for three correspondences: x1[j], x2[j] = mvX3Dc1 / mvX3Dc2 of sample j (3 floats each).
S3_HD void s3_compute_sim3(const float x1[3][3], const float x2[3][3], bool fix_scale, S3Hyp& h) {
  float Pr1[9], Pr2[9], O1[3], O2[3];   // Pr[r*3 + j]: row r (coordinate), column j (sample)
  for (int r = 0; r < 3; r++) {
    // cv::reduce(P, C, 1, REDUCE_SUM): reduceC_<float, float, OpAdd<float>>, two accumulators a0 = s0, a1 = s1; a0 += s2; a0 += a1
    float c1 = (x1[0][r] + x1[2][r]) + x1[1][r];
    float c2 = (x2[0][r] + x2[2][r]) + x2[1][r];
    // C = C / P.cols: MatExpr scale, convertTo(alpha = 1./3) -> cvt_32f: x * (float)alpha + (float)0
    const float third = (float)(1.0 / 3);
    O1[r] = c1 * third + 0.0f;
    O2[r] = c2 * third + 0.0f;
    for (int j = 0; j < 3; j++) {
      Pr1[r * 3 + j] = x1[j][r] - O1[r];
      Pr2[r * 3 + j] = x2[j][r] - O2[r];
    }
  }
  // M = Pr2 * Pr1.t(): gemm with GEMM_2_T -> GEMMSingleMul<float, double>
  float M[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double acc = 0;
      for (int k = 0; k < 3; k++) acc += (double)Pr2[r * 3 + k] * (double)Pr1[c * 3 + k];
      M[r * 3 + c] = (float)acc;
    }
  // N11 .. N44: float sums of M.at<float> (stored through double, exact)
  const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
  const float N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
  const float N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
  float A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
  float W[4], V[16];
  s3_jacobi4(A, W, V);   // cv::eigen(N, eval, evec)
  // vec = evec.row(0).colRange(1, 4); ang = atan2(norm(vec), evec(0, 0)); vec = 2*ang*vec/norm(vec)
  float vec[3] = {V[1], V[2], V[3]};
  const double nrm = sqrt((double)vec[0] * vec[0] + (double)vec[1] * vec[1] + (double)vec[2] * vec[2]);   // normL2Sqr<float, double>
  const double ang = atan2(nrm, (double)V[0]);
  const float alpha = (float)((2 * ang) * (1. / nrm));   // MatOp_AddEx: alpha = 2*ang, then *= 1./norm; convertTo with (float)alpha
  for (int j = 0; j < 3; j++) vec[j] = vec[j] * alpha + 0.0f;
  // cv::Rodrigues (cvRodrigues2, calibration.cpp): double, identity below DBL_EPSILON, R = c*I + c1*r*r' + s*[r]x, converted to float
  {
    double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
      for (int i = 0; i < 9; i++) h.R[i] = (i % 4 == 0) ? 1.f : 0.f;
    } else {
      const double c = cos(theta), s = sin(theta), c1 = 1. - c;
      const double itheta = theta ? 1. / theta : 0.;
      rx *= itheta; ry *= itheta; rz *= itheta;
      const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
      const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
      for (int i = 0; i < 9; i++) h.R[i] = (float)((((i % 4 == 0) ? 1.0 : 0.0) * c + c1 * rrt[i]) + s * r_x[i]);
    }
  }
  // P3 = mR12i * Pr2 (small path, alpha 1)
  float P3[9];
  for (int r = 0; r < 3; r++)
    for (int j = 0; j < 3; j++) P3[r * 3 + j] = s3_gemm3(&h.R[r * 3], Pr2[j], Pr2[3 + j], Pr2[6 + j], 1.0, 0.0);
  if (!fix_scale) {
    double nom = 0;   // Pr1.dot(P3): double accumulation in row-major order (mini_cv.h Mat::dot)
    for (int i = 0; i < 9; i++) nom += (double)Pr1[i] * (double)P3[i];
    double den = 0;   // cv::pow(P3, 2) in float, then the reference's double loop
    for (int i = 0; i < 9; i++) den += (double)(P3[i] * P3[i]);
    h.s = (float)(nom / den);
  } else {
    h.s = 1.0f;
  }
  // mt12i = O1 - ms12i*mR12i*O2: one gemm, alpha = -(double)ms12i, C = O1, beta = 1
  for (int r = 0; r < 3; r++) h.t[r] = s3_gemm3(&h.R[r * 3], O2[0], O2[1], O2[2], -(double)h.s, (double)O1[r]);
  s3_transforms(h);
}

// Step 8 of ComputeSim3 from h.R, h.t, h.s: mT12i = [sR | t], mT21i = [sRinv | tinv]
S3_HD void s3_transforms(S3Hyp& h) {
  // sR = ms12i*mR12i (convertTo, x*s + 0); sRinv = (1.0/ms12i)*mR12i.t() (MatOp_T: transpose, then convertTo unless alpha == 1)
  const double ainv = 1.0 / (double)h.s;
  const float ainvf = (float)ainv;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      h.sR[r * 3 + c] = h.R[r * 3 + c] * h.s + 0.0f;
      h.sRi[r * 3 + c] = ainv == 1.0 ? h.R[c * 3 + r] : h.R[c * 3 + r] * ainvf + 0.0f;
    }
  // tinv = -sRinv*mt12i: gemm with alpha = -1
  for (int r = 0; r < 3; r++) h.ti[r] = s3_gemm3(&h.sRi[r * 3], h.t[0], h.t[1], h.t[2], -1.0, 0.0);
}

// FromCameraToImage / Project: u = fx * (X * (1/Z)) + cx in float
S3_HD void s3_to_image(float X, float Y, float Z, const float K[4], float& u, float& v) {
  const float invz = 1 / Z;
  const float x = X * invz, y = Y * invz;
  u = K[0] * x + K[2];
  v = K[1] * y + K[3];
}

// Rcw*X + tcw: gemm with C = tcw, alpha = beta = 1 (small path)
S3_HD void s3_transform(const float* Rm, const float* tv, const float* X, float out[3]) {
  for (int r = 0; r < 3; r++) out[r] = s3_gemm3(&Rm[r * 3], X[0], X[1], X[2], 1.0, (double)tv[r]);
}

// squared reprojection error of dist = a - b as the float of the double dot (Mat::dot of a 2x1 float Mat)
S3_HD float s3_err(float au, float av, float bu, float bv) {
  const float d0 = au - bu, d1 = av - bv;
  return (float)((double)d0 * d0 + (double)d1 * d1);
}

// CheckInliers for one point: err1 < mvnMaxError1[i] && err2 < mvnMaxError2[i], the size_t thresholds converted to float (NaN -> false)
S3_HD bool s3_inlier(const S3Hyp& h, const float* X1, const float* X2, const float K1[4], const float K2[4], uint32_t thr1, uint32_t thr2) {
  float p1u, p1v, p2u, p2v, q[3], u21, v21, u12, v12;
  s3_to_image(X1[0], X1[1], X1[2], K1, p1u, p1v);   // mvP1im1
  s3_to_image(X2[0], X2[1], X2[2], K2, p2u, p2v);   // mvP2im2
  s3_transform(h.sR, h.t, X2, q);                   // vP2im1 = Project(mvX3Dc2, mT12i, mK1)
  s3_to_image(q[0], q[1], q[2], K1, u21, v21);
  s3_transform(h.sRi, h.ti, X1, q);                 // vP1im2 = Project(mvX3Dc1, mT21i, mK2)
  s3_to_image(q[0], q[1], q[2], K2, u12, v12);
  const float err1 = s3_err(p1u, p1v, u21, v21);
  const float err2 = s3_err(u12, v12, p2u, p2v);
  return err1 < (float)thr1 && err2 < (float)thr2;
}

// ---- one hypothesis over the arguments of ccm_sim3_ransac_eval: the host + device members of a form of ransac_wave.h -----------------
struct Sim3RansacArgs {
  int K, H, fix_scale;
  const int32_t* pt_off;   // [K + 1]
  const float* X1;         // [Ntot * 3]
  const float* X2;
  const float* K1;         // [K * 4]
  const float* K2;
  const uint32_t* thr1;    // [Ntot]
  const uint32_t* thr2;
  const int32_t* hyp_cand; // [H]
  const int32_t* hyp_idx;  // [H * 3], candidate-local
  const int32_t* mask_off; // [H + 1] words
  int32_t* n_inl;          // [H]
  float* rts;              // [H * 13]: R (9), t (3), s
  uint32_t* mask;          // [mask_off[H]]
};

struct Sim3HypForm {
  typedef Sim3RansacArgs Args;
  static constexpr int S = 3, kWorkDoubles = 0;
  S3Hyp hy;
  int c;
  float k1[4], k2[4];
  S3_HDM Sim3HypForm(const Args&, int cand) : hy{}, c(cand) {}
  S3_HDM void solve(const Args& a, int h, int p0, double*) {
    float x1[3][3], x2[3][3];
    for (int j = 0; j < 3; j++) {
      const int i = p0 + a.hyp_idx[3 * h + j];
      for (int r = 0; r < 3; r++) { x1[j][r] = a.X1[3 * i + r]; x2[j][r] = a.X2[3 * i + r]; }
    }
    s3_compute_sim3(x1, x2, a.fix_scale != 0, hy);
    float* o = a.rts + 13 * (size_t)h;
    for (int i = 0; i < 9; i++) o[i] = hy.R[i];
    for (int i = 0; i < 3; i++) o[9 + i] = hy.t[i];
    o[12] = hy.s;
  }
  S3_HDM void prepare(const Args& a) {   // the two cameras: loaded behind the solve, whose registers they would otherwise share
    for (int i = 0; i < 4; i++) { k1[i] = a.K1[4 * c + i]; k2[i] = a.K2[4 * c + i]; }
  }
  S3_HDM bool inlier(const Args& a, int g) const {
    return s3_inlier(hy, a.X1 + 3 * (size_t)g, a.X2 + 3 * (size_t)g, k1, k2, a.thr1[g], a.thr2[g]);
  }
};
