// pnp_math.h — the arithmetic of cslam::PnPsolver (cslam/src/PnPSolver.cpp), host + device: EPnP's compute_pose (:468-516) with everything it calls, and one
// point of CheckInliers (:299-330).  The kernel of pnp.hip runs these lines on four correspondences; the host evaluator and Refine (host/ccm_host.cpp) compile
// them with g++ for any n >= 4.
//
// Every step is the reference's expression in its own order of operations, f64 except where the reference rounds to float.  The legacy C-API calls are restated
// for f64 at the sizes used, from memory of OpenCV 4.2's baseline build (no FMA):
//   cvMulTransposed(A, D, 1)                 MulTransposedR: every entry of the upper triangle a double sum over A's rows in row order, the lower mirrored
//   cvSVD(A, W, Ut, 0, MODIFY_A | U_T)       JacobiSVDImpl_<double> on At = A' (tv_jacobi_svd_t of twoview_math.h: eps = 10 DBL_EPSILON, minval = DBL_MIN, 30 sweeps,
//                                            lapack.cpp's hypot, descending selection sort, rows normalised / completed); Ut = the rows of At
//   cvSVD(A, W, U, V, MODIFY_A)              the same with U = At', V = Vt'
//   cvInvert(A, Ainv, CV_SVD)                SVD::compute + SVBkSb without a right-hand side: threshold = 2 DBL_EPSILON * sum(w), values at or below it skipped
//   cvSolve(A, b, x, CV_SVD)                 JacobiSVD of the 6 x nc system on At = A', then SVBkSb with one right-hand side
// Compile with -ffp-contract=off.  Every loop is bounded by a constant or by n.
//
// Decisions the reference leaves open: qr_solve's singular exit leaves x as it is, and gauss_newton's x starts at zero (the reference's is an uninitialised stack
// array); nothing is printed.  Non-finite values are not trapped: they flow through as IEEE says, and a hypothesis with a non-finite pose has no inliers.
#pragma once
#include "twoview_math.h"

#define PNP_HD TV_HD
#if defined(__HIPCC__)
#define PNP_HDM __host__ __device__
#else
#define PNP_HDM
#endif

// ---- the restated C-API calls -------------------------------------------------------------------------------------------------------------------
// cvMulTransposed(A, D, 1) for a rows x C matrix A: D = A' A (C x C)
template <int C>
PNP_HD void pnp_mul_transposed(const double* A, int rows, double* D) {
  for (int i = 0; i < C; i++)
    for (int j = i; j < C; j++) {
      double s = 0;
      for (int k = 0; k < rows; k++) s += A[k * C + i] * A[k * C + j];
      D[i * C + j] = s;
    }
  for (int i = 0; i < C; i++)
    for (int j = i + 1; j < C; j++) D[j * C + i] = D[i * C + j];
}

template <int N>
PNP_HD void pnp_transpose(double* A) {
  for (int i = 0; i < N; i++)
    for (int j = i + 1; j < N; j++) { const double t = A[i * N + j]; A[i * N + j] = A[j * N + i]; A[j * N + i] = t; }
}

// cvSVD(A, W, Ut, 0, MODIFY_A | U_T) on an N x N matrix: A becomes Ut; w (nullable) the singular values.  OpenCV rotates a Vt beside At; nothing of At depends on
// it, so it is left out.
template <int N>
PNP_HD void pnp_svd_ut(double* A, double* w) {
  pnp_transpose<N>(A);
  tv_jacobi_svd_t<double, N, N, N>(A, nullptr, w, N);
}

// cvSVD(A, W, U, V, MODIFY_A) on a 3x3: u and v row-major
PNP_HD void pnp_svd_uv3(const double* A, double w[3], double u[9], double v[9]) {
  double At[9], Vt[9];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
  tv_jacobi_svd_t<double, 3, 3, 3>(At, Vt, w, 3);
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) { u[i * 3 + k] = At[k * 3 + i]; v[i * 3 + k] = Vt[k * 3 + i]; }
}

// cvInvert(A, X, CV_SVD) on a 3x3
PNP_HD void pnp_invert3_svd(const double* A, double* X) {
  double At[9], Vt[9], w[3];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
  tv_jacobi_svd_t<double, 3, 3, 3>(At, Vt, w, 3);
  for (int i = 0; i < 9; i++) X[i] = 0;
  double threshold = 0;
  for (int i = 0; i < 3; i++) threshold += w[i];
  threshold *= DBL_EPSILON * 2;
  for (int i = 0; i < 3; i++) {
    double wi = w[i];
    if (fabs(wi) <= threshold) continue;
    wi = 1 / wi;
    double buffer[3];
    for (int j = 0; j < 3; j++) buffer[j] = At[i * 3 + j] * wi;   // column i of u
    for (int r = 0; r < 3; r++) {
      const double s = Vt[i * 3 + r];
      for (int j = 0; j < 3; j++) X[r * 3 + j] = X[r * 3 + j] + s * buffer[j];
    }
  }
}

// cvSolve(A, b, x, CV_SVD) on a 6 x NC system, A row-major
template <int NC>
PNP_HD void pnp_solve_svd(const double* A, const double* b, double* x) {
  double At[NC * 6], Vt[NC * NC], w[NC];
  for (int i = 0; i < NC; i++)
    for (int k = 0; k < 6; k++) At[i * 6 + k] = A[k * NC + i];
  tv_jacobi_svd_t<double, 6, NC, NC>(At, Vt, w, NC);
  for (int i = 0; i < NC; i++) x[i] = 0;
  double threshold = 0;
  for (int i = 0; i < NC; i++) threshold += w[i];
  threshold *= DBL_EPSILON * 2;
  for (int i = 0; i < NC; i++) {
    double wi = w[i];
    if (fabs(wi) <= threshold) continue;
    wi = 1 / wi;
    double s = 0;
    for (int j = 0; j < 6; j++) s += At[i * 6 + j] * b[j];
    s *= wi;
    for (int j = 0; j < NC; j++) x[j] = x[j] + s * Vt[i * NC + j];
  }
}

// ---- PnPsolver's own lines ------------------------------------------------------------------------------------------------------------------------
PNP_HD double pnp_dist2(const double* p1, const double* p2) {
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

PNP_HD double pnp_dot(const double* v1, const double* v2) { return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]; }

// choose_control_points (:366-400): cws[4][3]; pca (nullable) receives PW0' PW0 before the decomposition
PNP_HD void pnp_choose_control_points(int n, const double* pws, double cws[4][3], double* pca) {
  cws[0][0] = cws[0][1] = cws[0][2] = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++) cws[0][j] += pws[3 * i + j];
  for (int j = 0; j < 3; j++) cws[0][j] /= n;
  double pw0tpw0[9], dc[3];
  // PW0(i, j) = pws[3 i + j] - cws[0][j] is not stored: the same difference is formed where cvMulTransposed reads it
  for (int i = 0; i < 3; i++)
    for (int j = i; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < n; k++) s += (pws[3 * k + i] - cws[0][i]) * (pws[3 * k + j] - cws[0][j]);
      pw0tpw0[i * 3 + j] = s;
    }
  for (int i = 0; i < 3; i++)
    for (int j = i + 1; j < 3; j++) pw0tpw0[j * 3 + i] = pw0tpw0[i * 3 + j];
  if (pca)
    for (int i = 0; i < 9; i++) pca[i] = pw0tpw0[i];
  pnp_svd_ut<3>(pw0tpw0, dc);
  const double* uct = pw0tpw0;
  for (int i = 1; i < 4; i++) {
    const double k = sqrt(dc[i - 1] / n);
    for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * uct[3 * (i - 1) + j];
  }
}

// compute_barycentric_coordinates (:402-425); cc_out (nullable) receives CC
PNP_HD void pnp_compute_barycentric_coordinates(int n, const double* pws, const double cws[4][3], double* alphas, double* cc_out) {
  double cc[9], cc_inv[9];
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
  if (cc_out)
    for (int i = 0; i < 9; i++) cc_out[i] = cc[i];
  pnp_invert3_svd(cc, cc_inv);
  const double* ci = cc_inv;
  for (int i = 0; i < n; i++) {
    const double* pi = pws + 3 * i;
    double* a = alphas + 4 * i;
    for (int j = 0; j < 3; j++)
      a[1 + j] = ci[3 * j] * (pi[0] - cws[0][0]) + ci[3 * j + 1] * (pi[1] - cws[0][1]) + ci[3 * j + 2] * (pi[2] - cws[0][2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
  }
}

// fill_M (:427-442); cam = fu fv uc vc
PNP_HD void pnp_fill_M(double* M, int row, const double* as, double u, double v, const double* cam) {
  double* M1 = M + row * 12;
  double* M2 = M1 + 12;
  for (int i = 0; i < 4; i++) {
    M1[3 * i] = as[i] * cam[0];
    M1[3 * i + 1] = 0.0;
    M1[3 * i + 2] = as[i] * (cam[2] - u);
    M2[3 * i] = 0.0;
    M2[3 * i + 1] = as[i] * cam[1];
    M2[3 * i + 2] = as[i] * (cam[3] - v);
  }
}

// compute_L_6x10 (:751-791)
PNP_HD void pnp_compute_L_6x10(const double* ut, double* l_6x10) {
  const double* v[4] = {ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8};
  double dv[4][6][3];
  for (int i = 0; i < 4; i++) {
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
      dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
      dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
      dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
      b++;
      if (b > 3) { a++; b = a + 1; }
    }
  }
  for (int i = 0; i < 6; i++) {
    double* row = l_6x10 + 10 * i;
    row[0] = pnp_dot(dv[0][i], dv[0][i]);
    row[1] = 2.0f * pnp_dot(dv[0][i], dv[1][i]);
    row[2] = pnp_dot(dv[1][i], dv[1][i]);
    row[3] = 2.0f * pnp_dot(dv[0][i], dv[2][i]);
    row[4] = 2.0f * pnp_dot(dv[1][i], dv[2][i]);
    row[5] = pnp_dot(dv[2][i], dv[2][i]);
    row[6] = 2.0f * pnp_dot(dv[0][i], dv[3][i]);
    row[7] = 2.0f * pnp_dot(dv[1][i], dv[3][i]);
    row[8] = 2.0f * pnp_dot(dv[2][i], dv[3][i]);
    row[9] = pnp_dot(dv[3][i], dv[3][i]);
  }
}

// compute_rho (:793-801)
PNP_HD void pnp_compute_rho(const double cws[4][3], double* rho) {
  rho[0] = pnp_dist2(cws[0], cws[1]);
  rho[1] = pnp_dist2(cws[0], cws[2]);
  rho[2] = pnp_dist2(cws[0], cws[3]);
  rho[3] = pnp_dist2(cws[1], cws[2]);
  rho[4] = pnp_dist2(cws[1], cws[3]);
  rho[5] = pnp_dist2(cws[2], cws[3]);
}

// find_betas_approx_1 (:658-685): betas10 = [B11 B12 B22 B13 B23 B33 B14 B24 B34 B44], approx_1 = [B11 B12 B13 B14]
PNP_HD void pnp_find_betas_approx_1(const double* l_6x10, const double* rho, double* betas) {
  double l_6x4[6 * 4], b4[4];
  for (int i = 0; i < 6; i++) {
    l_6x4[4 * i] = l_6x10[10 * i];
    l_6x4[4 * i + 1] = l_6x10[10 * i + 1];
    l_6x4[4 * i + 2] = l_6x10[10 * i + 3];
    l_6x4[4 * i + 3] = l_6x10[10 * i + 6];
  }
  pnp_solve_svd<4>(l_6x4, rho, b4);
  if (b4[0] < 0) {
    betas[0] = sqrt(-b4[0]);
    betas[1] = -b4[1] / betas[0];
    betas[2] = -b4[2] / betas[0];
    betas[3] = -b4[3] / betas[0];
  } else {
    betas[0] = sqrt(b4[0]);
    betas[1] = b4[1] / betas[0];
    betas[2] = b4[2] / betas[0];
    betas[3] = b4[3] / betas[0];
  }
}

// find_betas_approx_2 (:690-717): approx_2 = [B11 B12 B22]
PNP_HD void pnp_find_betas_approx_2(const double* l_6x10, const double* rho, double* betas) {
  double l_6x3[6 * 3], b3[3];
  for (int i = 0; i < 6; i++) {
    l_6x3[3 * i] = l_6x10[10 * i];
    l_6x3[3 * i + 1] = l_6x10[10 * i + 1];
    l_6x3[3 * i + 2] = l_6x10[10 * i + 2];
  }
  pnp_solve_svd<3>(l_6x3, rho, b3);
  if (b3[0] < 0) {
    betas[0] = sqrt(-b3[0]);
    betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
  } else {
    betas[0] = sqrt(b3[0]);
    betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
  }
  if (b3[1] < 0) betas[0] = -betas[0];
  betas[2] = 0.0;
  betas[3] = 0.0;
}

// find_betas_approx_3 (:722-749): approx_3 = [B11 B12 B22 B13 B23]
PNP_HD void pnp_find_betas_approx_3(const double* l_6x10, const double* rho, double* betas) {
  double l_6x5[6 * 5], b5[5];
  for (int i = 0; i < 6; i++) {
    l_6x5[5 * i] = l_6x10[10 * i];
    l_6x5[5 * i + 1] = l_6x10[10 * i + 1];
    l_6x5[5 * i + 2] = l_6x10[10 * i + 2];
    l_6x5[5 * i + 3] = l_6x10[10 * i + 3];
    l_6x5[5 * i + 4] = l_6x10[10 * i + 4];
  }
  pnp_solve_svd<5>(l_6x5, rho, b5);
  if (b5[0] < 0) {
    betas[0] = sqrt(-b5[0]);
    betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
  } else {
    betas[0] = sqrt(b5[0]);
    betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
  }
  if (b5[1] < 0) betas[0] = -betas[0];
  betas[2] = b5[3] / betas[0];
  betas[3] = 0.0;
}

// compute_A_and_b_gauss_newton (:803-829)
PNP_HD void pnp_compute_A_and_b_gauss_newton(const double* l_6x10, const double* rho, const double betas[4], double* A, double* b) {
  for (int i = 0; i < 6; i++) {
    const double* rowL = l_6x10 + i * 10;
    double* rowA = A + i * 4;
    rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
    rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
    rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
    rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
    b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                     rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                     rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
  }
}

// qr_solve (:851-941) of a 6 x 4 system: A and b are overwritten.  Returns false at the singular exit, with X untouched.
PNP_HD bool pnp_qr_solve(double* pA, double* pb, double* pX) {
  const int nr = 6, nc = 4;
  double A1[nr], A2[nr];
  double* ppAkk = pA;
  for (int k = 0; k < nc; k++) {
    double* ppAik = ppAkk;
    double eta = fabs(*ppAik);
    for (int i = k + 1; i < nr; i++) {
      const double elt = fabs(*ppAik);
      if (eta < elt) eta = elt;
      ppAik += nc;
    }
    if (eta == 0) {
      A1[k] = A2[k] = 0.0;
      return false;
    } else {
      double* ppAik = ppAkk;
      double sum = 0.0;
      const double inv_eta = 1. / eta;
      for (int i = k; i < nr; i++) {
        *ppAik *= inv_eta;
        sum += *ppAik * *ppAik;
        ppAik += nc;
      }
      double sigma = sqrt(sum);
      if (*ppAkk < 0) sigma = -sigma;
      *ppAkk += sigma;
      A1[k] = sigma * *ppAkk;
      A2[k] = -eta * sigma;
      for (int j = k + 1; j < nc; j++) {
        double* ppAik = ppAkk;
        double sum = 0;
        for (int i = k; i < nr; i++) {
          sum += *ppAik * ppAik[j - k];
          ppAik += nc;
        }
        const double tau = sum / A1[k];
        ppAik = ppAkk;
        for (int i = k; i < nr; i++) {
          ppAik[j - k] -= tau * *ppAik;
          ppAik += nc;
        }
      }
    }
    ppAkk += nc + 1;
  }
  // b <- Qt b
  double* ppAjj = pA;
  for (int j = 0; j < nc; j++) {
    double* ppAij = ppAjj;
    double tau = 0;
    for (int i = j; i < nr; i++) {
      tau += *ppAij * pb[i];
      ppAij += nc;
    }
    tau /= A1[j];
    ppAij = ppAjj;
    for (int i = j; i < nr; i++) {
      pb[i] -= tau * *ppAij;
      ppAij += nc;
    }
    ppAjj += nc + 1;
  }
  // X = R-1 b
  pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; i--) {
    const double* ppAij = pA + i * nc + (i + 1);
    double sum = 0;
    for (int j = i + 1; j < nc; j++) {
      sum += *ppAij * pX[j];
      ppAij++;
    }
    pX[i] = (pb[i] - sum) / A2[i];
  }
  return true;
}

// gauss_newton (:831-849)
PNP_HD void pnp_gauss_newton(const double* l_6x10, const double* rho, double betas[4]) {
  double a[6 * 4], b[6], x[4] = {0, 0, 0, 0};
  for (int k = 0; k < 5; k++) {
    pnp_compute_A_and_b_gauss_newton(l_6x10, rho, betas, a, b);
    pnp_qr_solve(a, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

// compute_ccs (:444-455)
PNP_HD void pnp_compute_ccs(const double* betas, const double* ut, double ccs[4][3]) {
  for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0f;
  for (int i = 0; i < 4; i++) {
    const double* v = ut + 12 * (11 - i);
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[3 * j + k];
  }
}

// compute_pcs (:457-466)
PNP_HD void pnp_compute_pcs(int n, const double* alphas, const double ccs[4][3], double* pcs) {
  for (int i = 0; i < n; i++) {
    const double* a = alphas + 4 * i;
    double* pc = pcs + 3 * i;
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
  }
}

// solve_for_sign (:627-640)
PNP_HD void pnp_solve_for_sign(int n, double ccs[4][3], double* pcs) {
  if (pcs[2] < 0.0) {
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 3; j++) ccs[i][j] = -ccs[i][j];
    for (int i = 0; i < n; i++) {
      pcs[3 * i] = -pcs[3 * i];
      pcs[3 * i + 1] = -pcs[3 * i + 1];
      pcs[3 * i + 2] = -pcs[3 * i + 2];
    }
  }
}

// estimate_R_and_t (:560-618); R row-major
PNP_HD void pnp_estimate_R_and_t(int n, const double* pws, const double* pcs, double R[9], double t[3]) {
  double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < n; i++) {
    const double* pc = pcs + 3 * i;
    const double* pw = pws + 3 * i;
    for (int j = 0; j < 3; j++) {
      pc0[j] += pc[j];
      pw0[j] += pw[j];
    }
  }
  for (int j = 0; j < 3; j++) {
    pc0[j] /= n;
    pw0[j] /= n;
  }
  double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, abt_d[3], abt_u[9], abt_v[9];
  for (int i = 0; i < n; i++) {
    const double* pc = pcs + 3 * i;
    const double* pw = pws + 3 * i;
    for (int j = 0; j < 3; j++) {
      abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
      abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
      abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
    }
  }
  pnp_svd_uv3(abt, abt_d, abt_u, abt_v);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = pnp_dot(abt_u + 3 * i, abt_v + 3 * j);
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  t[0] = pc0[0] - pnp_dot(R, pw0);
  t[1] = pc0[1] - pnp_dot(R + 3, pw0);
  t[2] = pc0[2] - pnp_dot(R + 6, pw0);
}

// reprojection_error (:541-558)
PNP_HD double pnp_reprojection_error(int n, const double* pws, const double* us, const double* cam, const double R[9], const double t[3]) {
  double sum2 = 0.0;
  for (int i = 0; i < n; i++) {
    const double* pw = pws + 3 * i;
    const double Xc = pnp_dot(R, pw) + t[0];
    const double Yc = pnp_dot(R + 3, pw) + t[1];
    const double inv_Zc = 1.0 / (pnp_dot(R + 6, pw) + t[2]);
    const double ue = cam[2] + cam[0] * Xc * inv_Zc;
    const double ve = cam[3] + cam[1] * Yc * inv_Zc;
    const double u = us[2 * i], v = us[2 * i + 1];
    sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
  }
  return sum2 / n;
}

// compute_R_and_t (:642-653)
PNP_HD double pnp_compute_R_and_t(int n, const double* pws, const double* us, const double* cam, const double* alphas, double* pcs, const double* ut,
                                  const double* betas, double R[9], double t[3]) {
  double ccs[4][3];
  pnp_compute_ccs(betas, ut, ccs);
  pnp_compute_pcs(n, alphas, ccs, pcs);
  pnp_solve_for_sign(n, ccs, pcs);
  pnp_estimate_R_and_t(n, pws, pcs, R, t);
  return pnp_reprojection_error(n, pws, us, cam, R, t);
}

// compute_pose (:468-516), first half: control points, barycentric coordinates, M and M' M.  cws comes back for compute_rho; mtm: 144 doubles; M: 24 n doubles;
// alphas: 4 n.  pca / cc (nullable): the two 3x3 matrices that are decomposed on the way.
PNP_HD void pnp_build_mtm(int n, const double* pws, const double* us, const double* cam, double cws[4][3], double* alphas, double* M, double* mtm, double* pca,
                          double* cc) {
  pnp_choose_control_points(n, pws, cws, pca);
  pnp_compute_barycentric_coordinates(n, pws, cws, alphas, cc);
  for (int i = 0; i < n; i++) pnp_fill_M(M, 2 * i, alphas + 4 * i, us[2 * i], us[2 * i + 1], cam);
  pnp_mul_transposed<12>(M, 2 * n, mtm);
}

// compute_pose (:468-516) on n correspondences: pws (3 n) and us (2 n) as add_correspondence stores them, cam = fu fv uc vc.  Work arrays of the caller: alphas (4 n),
// pcs (3 n), M (24 n), ut (144; on return Ut of M' M).  R (row-major) and t of the chosen solution; rep_errors[1..3] and the chosen N when asked for.  Returns
// rep_errors[N].
PNP_HD double pnp_compute_pose(int n, const double* pws, const double* us, const double* cam, double* alphas, double* pcs, double* M, double* ut, double R[9],
                               double t[3], double* rep_errors_out, int* chosen) {
  double cws[4][3];
  pnp_build_mtm(n, pws, us, cam, cws, alphas, M, ut, nullptr, nullptr);
  pnp_svd_ut<12>(ut, nullptr);
  double l_6x10[6 * 10], rho[6];
  pnp_compute_L_6x10(ut, l_6x10);
  pnp_compute_rho(cws, rho);
  double Betas[4][4], rep_errors[4] = {0, 0, 0, 0};
  double Rs[4][9], ts[4][3];
  for (int s = 1; s <= 3; s++) {   // the reference's three blocks, as one loop: the refinement and the pose recovery are instantiated once
    if (s == 1) pnp_find_betas_approx_1(l_6x10, rho, Betas[s]);
    else if (s == 2) pnp_find_betas_approx_2(l_6x10, rho, Betas[s]);
    else pnp_find_betas_approx_3(l_6x10, rho, Betas[s]);
    pnp_gauss_newton(l_6x10, rho, Betas[s]);
    rep_errors[s] = pnp_compute_R_and_t(n, pws, us, cam, alphas, pcs, ut, Betas[s], Rs[s], ts[s]);
  }
  int N = 1;
  if (rep_errors[2] < rep_errors[1]) N = 2;
  if (rep_errors[3] < rep_errors[N]) N = 3;
  for (int i = 0; i < 9; i++) R[i] = Rs[N][i];
  for (int i = 0; i < 3; i++) t[i] = ts[N][i];
  if (rep_errors_out)
    for (int i = 0; i < 4; i++) rep_errors_out[i] = rep_errors[i];
  if (chosen) *chosen = N;
  return rep_errors[N];
}

// ---- CheckInliers (:299-330), one point -------------------------------------------------------------------------------------------------------------
// P = mvP3Dw[i], p2d = mvP2D[i], max_err = mvMaxError[i]; the reference's mixed rounding: float Xc / Yc / invZc from double sums, double ue / ve, float distances,
// float error2, strict <.
PNP_HD float pnp_error2(const double R[9], const double t[3], const double* cam, const float* P, const float* p2d) {
  const float Xc = (float)(R[0] * P[0] + R[1] * P[1] + R[2] * P[2] + t[0]);
  const float Yc = (float)(R[3] * P[0] + R[4] * P[1] + R[5] * P[2] + t[1]);
  const float invZc = (float)(1 / (R[6] * P[0] + R[7] * P[1] + R[8] * P[2] + t[2]));
  const double ue = cam[2] + cam[0] * Xc * invZc;
  const double ve = cam[3] + cam[1] * Yc * invZc;
  const float distX = (float)(p2d[0] - ue);
  const float distY = (float)(p2d[1] - ve);
  return distX * distX + distY * distY;
}

PNP_HD bool pnp_inlier(const double R[9], const double t[3], const double* cam, const float* P, const float* p2d, float max_err) {
  return pnp_error2(R, t, cam, P, p2d) < max_err;
}

// mvMaxError[i] = mvSigma2[i] * th2 (:146): a float product
PNP_HD float pnp_max_error(float sigma2, float th2) { return sigma2 * th2; }

// ---- one hypothesis over the arguments of ccm_pnp_ransac_eval: the host + device members of a form of ransac_wave.h -------------------------------------------
struct PnpRansacArgs {
  int K, H;
  const double* cam;       // [K * 4]
  const int32_t* pt_off;   // [K + 1]
  const float* P3Dw;       // [Ntot * 3]
  const float* P2D;        // [Ntot * 2]
  const float* max_err;    // [Ntot]
  const int32_t* hyp_cand; // [H]
  const int32_t* hyp_idx;  // [H * 4], candidate-local
  const int32_t* mask_off; // [H + 1] words
  double* Rt;              // [H * 12]: R (9), t (3)
  int32_t* n_inl;          // [H]
  uint32_t* mask;          // [mask_off[H]]
};

struct PnpHypForm {
  typedef PnpRansacArgs Args;
  static constexpr int S = 4, kWorkDoubles = 96 + 144;   // the solve's run-time indexed arrays: M (2 * 4 rows of 12), then M' M / Ut
  double cam[4], R[9], t[3];
  PNP_HDM PnpHypForm(const Args& a, int c) : cam{a.cam[4 * c], a.cam[4 * c + 1], a.cam[4 * c + 2], a.cam[4 * c + 3]}, R{}, t{} {}
  PNP_HDM void solve(const Args& a, int h, int p0, double* work) {
    double pws[12], us[8], alphas[16], pcs[12];
    for (int j = 0; j < 4; j++) {
      const size_t i = (size_t)(p0 + a.hyp_idx[4 * h + j]);
      for (int r = 0; r < 3; r++) pws[3 * j + r] = a.P3Dw[3 * i + r];
      for (int r = 0; r < 2; r++) us[2 * j + r] = a.P2D[2 * i + r];
    }
    pnp_compute_pose(4, pws, us, cam, alphas, pcs, work, work + 96, R, t, nullptr, nullptr);
    double* o = a.Rt + 12 * (size_t)h;
    for (int i = 0; i < 9; i++) o[i] = R[i];
    for (int i = 0; i < 3; i++) o[9 + i] = t[i];
  }
  PNP_HDM void prepare(const Args&) {}
  PNP_HDM bool inlier(const Args& a, int g) const {
    const size_t i = (size_t)g;
    return pnp_inlier(R, t, cam, a.P3Dw + 3 * i, a.P2D + 2 * i, a.max_err[i]);
  }
};
