// Sim3Solver_hip.cpp — DROP-IN replacement for the translation unit cslam/src/Sim3Solver.cpp of the reference, compiled against the reference's
// own Sim3Solver.h: the Sim3 RANSAC that LoopFinder::ComputeSim3 and MapMatcher::ComputeSim3 run round-robin over their candidates.
//
// The constructor gathers the correspondences on the object graph as the reference does (null / bad map points and negative
// GetIndexInKeyFrame skipped, mvnMaxError as size_t, X3Dc = Rcw*X + tcw).  iterate(n) evaluates its at most n hypotheses in ONE device launch
// through libccm_host.so (ccmh_sim3_solver_iterate -> ccm_sim3_ransac_eval); the three random values per hypothesis come from ::rand() through
// the calling thread's FIFO that cslam::Sim3RansacBatch shares, and the values of hypotheses after a success go back to it.  The unmodified
// LoopFinder / MapMatcher therefore see the sample sequence, inlier sets and estimates of the reference (contract in include/ccm_hip.h).
// The batched fast path over all candidates at once is cslam::Sim3RansacBatch.
//
// ComputeSim3 / CheckInliers are protected and called by no one but the reference's own iterate(); they are defined with the same lines the
// kernel runs (ccm_slam_amd/csrc/sim3_ransac_math.h) so that the class keeps every member.  There is no CPU path for iterate(): if the device
// call fails the method throws estd::infrastructure_ex.
#include <cslam/Sim3Solver.h>

#include <cstdint>
#include <cstdlib>

#include "../ccm_slam_amd/host/ccm_host_c.h"
#include "../ccm_slam_amd/csrc/sim3_ransac_math.h"

namespace cslam {

namespace {
int device() { static const int d = std::getenv("CCM_DEVICE") ? std::atoi(std::getenv("CCM_DEVICE")) : 0; return d; }

void fail(const char* what) {
  cout << COUTFATAL << "Sim3Solver::" << what << ": the MI355X path failed" << endl;
  throw estd::infrastructure_ex();
}

void camera(const cv::Mat& K, float out[4]) {
  out[0] = K.at<float>(0, 0); out[1] = K.at<float>(1, 1); out[2] = K.at<float>(0, 2); out[3] = K.at<float>(1, 2);
}

// S3Hyp -> the reference's members (mR12i 3x3, mt12i 3x1, mT12i / mT21i 4x4, all CV_32F)
void to_mats(const S3Hyp& h, cv::Mat& R, cv::Mat& t, cv::Mat& T12, cv::Mat& T21) {
  R.create(3, 3, CV_32F); t.create(3, 1, CV_32F);
  T12 = cv::Mat::eye(4, 4, CV_32F); T21 = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      R.at<float>(r, c) = h.R[3 * r + c];
      T12.at<float>(r, c) = h.sR[3 * r + c];
      T21.at<float>(r, c) = h.sRi[3 * r + c];
    }
    t.at<float>(r) = h.t[r];
    T12.at<float>(r, 3) = h.t[r];
    T21.at<float>(r, 3) = h.ti[r];
  }
}

S3Hyp from_mats(const cv::Mat& T12, const cv::Mat& T21) {
  S3Hyp h;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) { h.sR[3 * r + c] = T12.at<float>(r, c); h.sRi[3 * r + c] = T21.at<float>(r, c); }
    h.t[r] = T12.at<float>(r, 3);
    h.ti[r] = T21.at<float>(r, 3);
  }
  return h;
}
}  // namespace

Sim3Solver::Sim3Solver(kfptr pKF1, kfptr pKF2, const vector<mpptr>& vpMatched12, const bool bFixScale)
    : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale) {
  mpKF1 = pKF1;
  mpKF2 = pKF2;
  vector<mpptr> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  mN1 = vpMatched12.size();
  mvpMapPoints1.reserve(mN1);
  mvpMapPoints2.reserve(mN1);
  mvpMatches12 = vpMatched12;
  mvnIndices1.reserve(mN1);
  mvX3Dc1.reserve(mN1);
  mvX3Dc2.reserve(mN1);
  cv::Mat Rcw1 = pKF1->GetRotation();
  cv::Mat tcw1 = pKF1->GetTranslation();
  cv::Mat Rcw2 = pKF2->GetRotation();
  cv::Mat tcw2 = pKF2->GetTranslation();
  mvAllIndices.reserve(mN1);
  size_t idx = 0;
  for (int i1 = 0; i1 < mN1; i1++) {
    if (!vpMatched12[i1]) continue;
    mpptr pMP1 = vpKeyFrameMP1[i1];
    mpptr pMP2 = vpMatched12[i1];
    if (!pMP1) {
      cout << "!pMP1" << endl;
      continue;
    }
    if (pMP1->isBad() || pMP2->isBad()) continue;
    const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
    const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
    const cv::KeyPoint& kp2 = pKF2->mvKeysUn[indexKF2];
    const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
    const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
    mvnMaxError1.push_back(9.210 * sigmaSquare1);   // size_t: truncated, as the reference stores it
    mvnMaxError2.push_back(9.210 * sigmaSquare2);
    mvpMapPoints1.push_back(pMP1);
    mvpMapPoints2.push_back(pMP2);
    mvnIndices1.push_back(i1);
    cv::Mat X3D1w = pMP1->GetWorldPos();
    mvX3Dc1.push_back(Rcw1 * X3D1w + tcw1);
    cv::Mat X3D2w = pMP2->GetWorldPos();
    mvX3Dc2.push_back(Rcw2 * X3D2w + tcw2);
    mvAllIndices.push_back(idx);
    idx++;
  }
  mK1 = pKF1->mK;
  mK2 = pKF2->mK;
  FromCameraToImage(mvX3Dc1, mvP1im1, mK1);
  FromCameraToImage(mvX3Dc2, mvP2im2, mK2);
  SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  mRansacMaxIts = maxIterations;
  N = mvpMapPoints1.size();
  mvbInliersi.resize(N);
  float epsilon = (float)mRansacMinInliers / N;
  int nIterations;
  if (mRansacMinInliers == N)
    nIterations = 1;
  else
    nIterations = ceil(log(1 - mRansacProb) / log(1 - pow(epsilon, 3)));
  mRansacMaxIts = max(1, min(nIterations, mRansacMaxIts));
  mnIterations = 0;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers = vector<bool>(mN1, false);
  nInliers = 0;
  if (N < mRansacMinInliers) {
    bNoMore = true;
    return cv::Mat();
  }
  std::vector<float> X1(3 * (size_t)N), X2(3 * (size_t)N);
  std::vector<uint32_t> t1(N), t2(N);
  for (int i = 0; i < N; i++) {
    for (int r = 0; r < 3; r++) { X1[3 * i + r] = mvX3Dc1[i].at<float>(r); X2[3 * i + r] = mvX3Dc2[i].at<float>(r); }
    t1[i] = (uint32_t)mvnMaxError1[i];
    t2[i] = (uint32_t)mvnMaxError2[i];
  }
  float K1[4], K2[4];
  camera(mK1, K1);
  camera(mK2, K2);
  int32_t state[2] = {mnIterations, mnBestInliers}, flags[4] = {0, 0, 0, 0};
  float rts[13];
  std::vector<uint32_t> mask((N + 31) / 32 + 1);
  if (ccmh_sim3_solver_iterate(device(), N, X1.data(), X2.data(), K1, K2, t1.data(), t2.data(), mbFixScale ? 1 : 0, mRansacMinInliers, mRansacMaxIts,
                               nIterations, state, rts, mask.data(), flags) != 0)
    fail("iterate");
  mnIterations = state[0];
  mnBestInliers = state[1];
  if (flags[2]) {   // the last hypothesis with mnInliersi >= mnBestInliers: the reference's mBest* and current-hypothesis members
    S3Hyp h;
    for (int i = 0; i < 9; i++) h.R[i] = rts[i];
    for (int i = 0; i < 3; i++) h.t[i] = rts[9 + i];
    h.s = rts[12];
    s3_transforms(h);
    to_mats(h, mR12i, mt12i, mT12i, mT21i);
    ms12i = h.s;
    mnInliersi = flags[3];
    for (int i = 0; i < N; i++) mvbInliersi[i] = (mask[i >> 5] >> (i & 31)) & 1u;
    mvbBestInliers = mvbInliersi;
    mBestT12 = mT12i.clone();
    mBestRotation = mR12i.clone();
    mBestTranslation = mt12i.clone();
    mBestScale = ms12i;
  }
  if (flags[0]) {
    nInliers = mnInliersi;
    for (int i = 0; i < N; i++)
      if (mvbInliersi[i]) vbInliers[mvnIndices1[i]] = true;
    return mBestT12;
  }
  if (flags[1]) bNoMore = true;
  return cv::Mat();
}

cv::Mat Sim3Solver::find(vector<bool>& vbInliers12, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

// cv::reduce(P, C, 1, REDUCE_SUM) as reduceC_<float, float, OpAdd<float>> (two accumulators, unrolled by 4), then C / P.cols as x * (float)(1./cols)
void Sim3Solver::ComputeCentroid(cv::Mat& P, cv::Mat& Pr, cv::Mat& C) {
  const int w = P.cols;
  const float sc = (float)(1. / w);
  C.create(P.rows, 1, CV_32F);
  for (int r = 0; r < P.rows; r++) {
    float a0 = P.at<float>(r, 0);
    if (w > 1) {
      float a1 = P.at<float>(r, 1);
      int i = 2;
      for (; i <= w - 4; i += 4) {
        a0 = a0 + P.at<float>(r, i); a1 = a1 + P.at<float>(r, i + 1);
        a0 = a0 + P.at<float>(r, i + 2); a1 = a1 + P.at<float>(r, i + 3);
      }
      for (; i < w; i++) a0 = a0 + P.at<float>(r, i);
      a0 = a0 + a1;
    }
    C.at<float>(r) = a0 * sc + 0.0f;
  }
  for (int i = 0; i < w; i++)
    for (int r = 0; r < P.rows; r++) Pr.at<float>(r, i) = P.at<float>(r, i) - C.at<float>(r);
}

void Sim3Solver::ComputeSim3(cv::Mat& P1, cv::Mat& P2) {
  float x1[3][3], x2[3][3];
  for (int j = 0; j < 3; j++)
    for (int r = 0; r < 3; r++) { x1[j][r] = P1.at<float>(r, j); x2[j][r] = P2.at<float>(r, j); }
  S3Hyp h;
  s3_compute_sim3(x1, x2, mbFixScale, h);
  to_mats(h, mR12i, mt12i, mT12i, mT21i);
  ms12i = h.s;
}

void Sim3Solver::CheckInliers() {
  const S3Hyp h = from_mats(mT12i, mT21i);
  float K1[4], K2[4];
  camera(mK1, K1);
  camera(mK2, K2);
  mnInliersi = 0;
  for (size_t i = 0; i < mvP1im1.size(); i++) {
    float X1[3], X2[3];
    for (int r = 0; r < 3; r++) { X1[r] = mvX3Dc1[i].at<float>(r); X2[r] = mvX3Dc2[i].at<float>(r); }
    mvbInliersi[i] = s3_inlier(h, X1, X2, K1, K2, (uint32_t)mvnMaxError1[i], (uint32_t)mvnMaxError2[i]);
    if (mvbInliersi[i]) mnInliersi++;
  }
}

cv::Mat Sim3Solver::GetEstimatedRotation() { return mBestRotation.clone(); }

cv::Mat Sim3Solver::GetEstimatedTranslation() { return mBestTranslation.clone(); }

float Sim3Solver::GetEstimatedScale() { return mBestScale; }

void Sim3Solver::Project(const vector<cv::Mat>& vP3Dw, vector<cv::Mat>& vP2D, cv::Mat Tcw, cv::Mat K) {
  float Kc[4], Rm[9], tv[3];
  camera(K, Kc);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Rm[3 * r + c] = Tcw.at<float>(r, c);
    tv[r] = Tcw.at<float>(r, 3);
  }
  vP2D.clear();
  vP2D.reserve(vP3Dw.size());
  for (size_t i = 0; i < vP3Dw.size(); i++) {
    float X[3] = {vP3Dw[i].at<float>(0), vP3Dw[i].at<float>(1), vP3Dw[i].at<float>(2)}, P[3], u, v;
    s3_transform(Rm, tv, X, P);
    s3_to_image(P[0], P[1], P[2], Kc, u, v);
    vP2D.push_back((cv::Mat_<float>(2, 1) << u, v));
  }
}

void Sim3Solver::FromCameraToImage(const vector<cv::Mat>& vP3Dc, vector<cv::Mat>& vP2D, cv::Mat K) {
  float Kc[4];
  camera(K, Kc);
  vP2D.clear();
  vP2D.reserve(vP3Dc.size());
  for (size_t i = 0; i < vP3Dc.size(); i++) {
    float u, v;
    s3_to_image(vP3Dc[i].at<float>(0), vP3Dc[i].at<float>(1), vP3Dc[i].at<float>(2), Kc, u, v);
    vP2D.push_back((cv::Mat_<float>(2, 1) << u, v));
  }
}

}  // namespace cslam
