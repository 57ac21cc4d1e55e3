// PnPsolver_hip.cpp — DROP-IN replacement for the translation unit cslam/src/PnPSolver.cpp of the reference, compiled against the reference's own
// PnPSolver.h: the EPnP RANSAC a Relocalization() runs round-robin over its candidate keyframes.
//
// The constructor gathers the correspondences as the reference does (null and bad map points skipped, mvP2D from mvKeysUn, mvSigma2 from the keypoint's
// octave, fu fv uc vc from the frame).  iterate(n) is one call of a single-candidate cslam::PnPRansacBatch in libccm_host.so (ccmh_pnp_ransac_iterate ->
// ccm_pnp_ransac_eval): all hypotheses the call can run are evaluated in ONE device launch, Refine's EPnP runs on the host, and the four random values per
// hypothesis come from ::rand() through the calling thread's FIFO (the one the Sim3 solvers use); the values of hypotheses after a successful Refine go back
// to it.  The caller therefore sees the sample sequence, the poses and the inlier sets of the reference.  The batched fast path over all
// candidates at once is cslam::PnPRansacBatch itself.
//
// The class has no member for the batch; it is kept beside the object, keyed by its address, and released by the destructor.  SetRansacParameters releases
// it as well: the reference keeps mnIterations across a second SetRansacParameters, here the RANSAC state starts again — every caller sets the parameters
// once, before the first iterate().  The private EPnP members (compute_pose and what it calls, CheckInliers, Refine) are called by no one but the reference's
// own iterate() and stay undefined: their lines are ccm_slam_amd/csrc/pnp_math.h.  There is no CPU path: if the device call fails, iterate() throws
// estd::infrastructure_ex.
#include <cslam/PnPSolver.h>

#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>

#include "../ccm_slam_amd/host/ccm_host_c.h"

namespace cslam {

namespace {
int device() { static const int d = std::getenv("CCM_DEVICE") ? std::atoi(std::getenv("CCM_DEVICE")) : 0; return d; }

void fail(const char* what) {
  cout << COUTFATAL << "PnPsolver::" << what << ": the MI355X path failed" << endl;
  throw estd::infrastructure_ex();
}

std::mutex g_mutex;
std::map<const PnPsolver*, void*> g_batch;

void release(const PnPsolver* s) {
  std::lock_guard<std::mutex> lock(g_mutex);
  auto it = g_batch.find(s);
  if (it == g_batch.end()) return;
  ccmh_pnp_ransac_destroy(it->second);
  g_batch.erase(it);
}
}  // namespace

PnPsolver::PnPsolver(const Frame& F, const vector<mpptr>& vpMapPointMatches)
    : pws(0), us(0), alphas(0), pcs(0), maximum_number_of_correspondences(0), number_of_correspondences(0), mnInliersi(0), mnIterations(0), mnBestInliers(0), N(0) {
  mvpMapPointMatches = vpMapPointMatches;
  mvP2D.reserve(F.mvpMapPoints.size());
  mvSigma2.reserve(F.mvpMapPoints.size());
  mvP3Dw.reserve(F.mvpMapPoints.size());
  mvKeyPointIndices.reserve(F.mvpMapPoints.size());
  mvAllIndices.reserve(F.mvpMapPoints.size());
  int idx = 0;
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
    mpptr pMP = vpMapPointMatches[i];
    if (!pMP) continue;
    if (pMP->isBad()) continue;
    const cv::KeyPoint& kp = F.mvKeysUn[i];
    mvP2D.push_back(kp.pt);
    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
    cv::Mat Pos = pMP->GetWorldPos();
    mvP3Dw.push_back(cv::Point3f(Pos.at<float>(0), Pos.at<float>(1), Pos.at<float>(2)));
    mvKeyPointIndices.push_back(i);
    mvAllIndices.push_back(idx);
    idx++;
  }
  fu = F.fx;
  fv = F.fy;
  uc = F.cx;
  vc = F.cy;
  SetRansacParameters();
}

PnPsolver::~PnPsolver() { release(this); }

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
  release(this);
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  mRansacMaxIts = maxIterations;
  mRansacEpsilon = epsilon;
  mRansacMinSet = minSet;
  mRansacTh = th2;
  N = mvP2D.size();
  mvbInliersi.resize(N);
  int nMinInliers = N * mRansacEpsilon;
  if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  mRansacMinInliers = nMinInliers;
  mvMaxError.resize(mvSigma2.size());
  for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
  if (N < mRansacMinInliers) return;   // iterate() returns bNoMore before it reads the iteration limit
  if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
  int nIterations;
  if (mRansacMinInliers == N)
    nIterations = 1;
  else
    nIterations = ceil(log(1 - mRansacProb) / log(1 - pow(mRansacEpsilon, 3)));
  mRansacMaxIts = max(1, min(nIterations, mRansacMaxIts));
}

cv::Mat PnPsolver::find(vector<bool>& vbInliers, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers.clear();
  nInliers = 0;
  if (N < mRansacMinInliers) {
    bNoMore = true;
    return cv::Mat();
  }
  if (mRansacMinSet != 4) fail("iterate (minSet must be 4)");
  void* h = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_batch.find(this);
    if (it != g_batch.end()) h = it->second;
  }
  const int n_matches = (int)mvpMapPointMatches.size();
  if (!h) {
    // the adjusted members reproduce themselves under SetRansacParameters' lines, so they stand for the caller's arguments
    std::vector<float> P3(3 * (size_t)N), P2(2 * (size_t)N);
    std::vector<int32_t> kp(N);
    for (int i = 0; i < N; i++) {
      P3[3 * i] = mvP3Dw[i].x; P3[3 * i + 1] = mvP3Dw[i].y; P3[3 * i + 2] = mvP3Dw[i].z;
      P2[2 * i] = mvP2D[i].x; P2[2 * i + 1] = mvP2D[i].y;
      kp[i] = (int32_t)mvKeyPointIndices[i];
    }
    const int32_t pt_off[2] = {0, N};
    const double cam[4] = {fu, fv, uc, vc};
    h = ccmh_pnp_ransac_create(device(), 1, pt_off, P3.data(), P2.data(), mvSigma2.data(), cam, &n_matches, kp.data(), mRansacProb, mRansacMinInliers, mRansacMaxIts,
                               mRansacMinSet, mRansacEpsilon, mRansacTh, 5, nullptr, 0);
    if (!h) fail("iterate (no batch)");
    std::lock_guard<std::mutex> lock(g_mutex);
    g_batch[this] = h;
  }
  float Tcw[16];
  std::vector<uint8_t> inl(n_matches + 1);
  int32_t n = 0, flags[2] = {0, 0}, info[4] = {0, 0, 0, 0};
  const int rc = ccmh_pnp_ransac_iterate(h, 0, nIterations, Tcw, inl.data(), n_matches, &n, flags);
  if (rc < 0) fail("iterate");
  if (ccmh_pnp_ransac_info(h, 0, info) == 0) mnIterations = info[0];
  bNoMore = flags[1] != 0;
  if (rc != 1) return cv::Mat();
  nInliers = n;
  vbInliers = vector<bool>(mvpMapPointMatches.size(), false);
  for (int i = 0; i < n_matches; i++)
    if (inl[i]) vbInliers[i] = true;
  cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) T.at<float>(r, c) = Tcw[4 * r + c];
  if (flags[0]) {
    mRefinedTcw = T;
    mnRefinedInliers = n;
  } else {
    mBestTcw = T;
    mnBestInliers = n;
  }
  return T.clone();
}

}  // namespace cslam
