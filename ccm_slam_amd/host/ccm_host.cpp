// ccm_host.cpp — implementation of the host-side mirror's classes (see ccm_host.h; their C entry points are in c_*.cpp).  Plain C++17, no HIP headers:
// everything device-side goes through the C ABI.
#include "ccm_host.h"
#include "mirror_internal.h"
#include "kfdb_resolve.h"
#include "../csrc/triangulate_math.h"
#include "../csrc/twoview_math.h"
#include "../csrc/pnp_math.h"
#include "../csrc/sim3_correct_math.h"
#include "../csrc/gba_apply_math.h"
#include "../csrc/covis_math.h"
#include "../csrc/kfcull_math.h"
#include "../csrc/fuse_math.h"
#include "../csrc/kfstore_math.h"
#include "../csrc/kfingest_math.h"
#include "../csrc/bow_search_math.h"
#include "../csrc/tri_search_math.h"
#include "../csrc/mappoint_math.h"
#include "../csrc/frame_math.h"
#include "../csrc/guided_search_math.h"
#include "ccm_convert.h"
#include "guided_replay.h"
#include <climits>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

namespace cslam {

static void check(int rc, ccm_ctx* ctx, const char* what) {
  if (rc != CCM_OK) throw infrastructure_ex(std::string(what) + ": " + ccm_last_error(ctx));
}

HipContext::HipContext(int device) { check(ccm_ctx_create(device, &ctx_), nullptr, "ccm_ctx_create"); }
HipContext::~HipContext() { ccm_ctx_destroy(ctx_); }

// ---- ORBextractor ----------------------------------------------------------------------------------
ORBextractor::ORBextractor(HipContext& ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
    : nlevels_(nlevels), scaleFactor_(scaleFactor) {
  check(ccm_orb_create(ctx.get(), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, &orb_), ctx.get(), "ccm_orb_create");
}
ORBextractor::~ORBextractor() { ccm_orb_destroy(orb_); }

std::vector<float> ORBextractor::table(int which) const {
  std::vector<float> t(nlevels_);
  ccm_orb_get_table(orb_, which, t.data(), nlevels_);
  return t;
}

void ORBextractor::operator()(const uint8_t* image, int cols, int rows, int step, std::vector<KeyPoint>& keypoints,
                              std::vector<uint8_t>& descriptors) {
  if (!image || cols <= 0 || rows <= 0) { keypoints.clear(); descriptors.clear(); return; }   // if(_image.empty()) return; (:1219)
  const int cap = ccm_orb_max_keypoints(orb_);
  static_assert(sizeof(KeyPoint) == sizeof(ccm_keypoint), "KeyPoint must match ccm_keypoint");
  keypoints.resize(cap);
  descriptors.resize((size_t)cap * 32);
  std::vector<uint8_t*> pyr;
  if (keepPyramid) {
    mvImagePyramid.resize(nlevels_);
    pyr.resize(nlevels_);
    for (int l = 0; l < nlevels_; l++) {
      Level& L = mvImagePyramid[l];
      ccm_orb_level_size(orb_, cols, rows, l, &L.cols, &L.rows);
      L.data.resize((size_t)L.cols * L.rows);
      pyr[l] = L.data.data();
    }
  }
  int n = 0;
  const int rc = ccm_orb_extract(orb_, image, cols, rows, step, reinterpret_cast<ccm_keypoint*>(keypoints.data()), descriptors.data(),
                                 cap, &n, keepPyramid ? pyr.data() : nullptr);
  if (rc != CCM_OK) throw infrastructure_ex(std::string("ccm_orb_extract: ") + ccm_last_error(nullptr));
  keypoints.resize(n);
  descriptors.resize((size_t)n * 32);
}

// ---- Frame grid (Frame.cpp:87-88, 103-118, 200-265), FRAME_GRID_COLS 75 x ROWS 48 -------------------
namespace {
struct FrameGrid {
  const FrameView& F;
  float wInv, hInv;
  std::vector<int> start;   // CSR over cells (column-major: cell = ix * rows + iy), insertion order kept
  std::vector<int> items;
  explicit FrameGrid(const FrameView& f) : F(f) {
    wInv = static_cast<float>(kGridCols) / static_cast<float>(F.mnMaxX - F.mnMinX);
    hInv = static_cast<float>(kGridRows) / static_cast<float>(F.mnMaxY - F.mnMinY);
    std::vector<int> cellOf(F.N, -1);
    start.assign(kGridCols * kGridRows + 1, 0);
    for (int i = 0; i < F.N; i++) {
      const int px = (int)std::round((F.mvKeysUn[i].x - F.mnMinX) * wInv);   // PosInGrid uses round()
      const int py = (int)std::round((F.mvKeysUn[i].y - F.mnMinY) * hInv);
      if (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) continue;
      cellOf[i] = px * kGridRows + py;
      start[cellOf[i] + 1]++;
    }
    for (size_t c = 1; c < start.size(); c++) start[c] += start[c - 1];
    items.resize(start.back());
    std::vector<int> pos(start.begin(), start.end() - 1);
    for (int i = 0; i < F.N; i++) if (cellOf[i] >= 0) items[pos[cellOf[i]]++] = i;
  }
  // appends the candidate indices in the reference's order (ix-major, iy, insertion)
  void featuresInArea(float x, float y, float r, int minLevel, int maxLevel, std::vector<int32_t>& out) const {
    // the cell range by the device's own lines: total for any x, y, r (csrc/frame_math.h)
    const FrameBounds b{F.mnMinX, F.mnMinY, F.mnMaxX, F.mnMaxY, wInv, hInv};
    int nMinCellX, nMaxCellX, nMinCellY, nMaxCellY;
    if (!frame_cell_range(b, x, y, r, nMinCellX, nMaxCellX, nMinCellY, nMaxCellY)) return;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
      for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
        const int c = ix * kGridRows + iy;
        for (int s = start[c]; s < start[c + 1]; s++) {
          const int k = items[s];
          const KeyPoint& kp = F.mvKeysUn[k];
          if (bCheckLevels) {
            if (kp.octave < minLevel) continue;
            if (maxLevel >= 0 && kp.octave > maxLevel) continue;
          }
          if (std::fabs(kp.x - x) < r && std::fabs(kp.y - y) < r) out.push_back(k);
        }
      }
  }
};

// the rotation-consistency filter every search ends in: guided_replay.h
using ccm_guided::RotationFilter;
}  // namespace

int ORBmatcher::DescriptorDistance(const uint8_t* a, const uint8_t* b) {
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    uint32_t x, y;
    std::memcpy(&x, a + 4 * i, 4); std::memcpy(&y, b + 4 * i, 4);
    dist += __builtin_popcount(x ^ y);
  }
  return dist;
}

// Device does every Hamming distance of every (map point, window candidate) pair in one launch; the host then
// replays the reference's loop over the map points IN ORDER on the precomputed distances, so that features
// claimed by an earlier map point are skipped by later ones exactly as ORBmatcher.cpp:113-115 does.
int ORBmatcher::SearchByProjection(FrameView& F, const TrackedMapPoints& mps, float th) {
  FrameGrid grid(F);
  const bool bFactor = th != 1.0;
  std::vector<int32_t> q_of;        // compact query -> map point index
  std::vector<int32_t> off(1, 0), idx;
  std::vector<uint8_t> qdesc;
  for (int i = 0; i < mps.n; i++) {
    if (!mps.mbTrackInView[i]) continue;
    const int lvl = mps.mnTrackScaleLevel[i];
    float r = (mps.mTrackViewCos[i] > 0.998) ? 2.5f : 4.0f;   // RadiusByViewingCos (:150-156)
    if (bFactor) r *= th;
    const size_t before = idx.size();
    grid.featuresInArea(mps.mTrackProjX[i], mps.mTrackProjY[i], r * F.mvScaleFactors[lvl], lvl - 1, lvl, idx);
    if (idx.size() == before) continue;   // vIndices.empty()
    q_of.push_back(i);
    off.push_back((int32_t)idx.size());
    qdesc.insert(qdesc.end(), mps.mDescriptor + (size_t)i * 32, mps.mDescriptor + (size_t)i * 32 + 32);
  }
  const int Q = (int)q_of.size();
  if (Q == 0) return 0;
  std::vector<uint16_t> dist(idx.size());
  check(ccm_hamming_csr(ctx_.get(), qdesc.data(), Q, F.mDescriptors, F.N, off.data(), idx.data(), dist.data(), nullptr, nullptr, nullptr),
        ctx_.get(), "ccm_hamming_csr");
  int nmatches = 0;
  for (int q = 0; q < Q; q++) {
    int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int k = idx[s];
      if (F.mvpMapPoints[k] >= 0) continue;   // F.mvpMapPoints[idx] && Observations() > 0
      const int d = dist[s];
      if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestLevel2 = bestLevel; bestLevel = F.mvKeysUn[k].octave; bestIdx = k; }
      else if (d < bestDist2) { bestLevel2 = F.mvKeysUn[k].octave; bestDist2 = d; }
    }
    if (bestDist <= TH_HIGH) {
      if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue;
      F.mvpMapPoints[bestIdx] = q_of[q];
      nmatches++;
    }
  }
  return nmatches;
}

FrameGridDev::FrameGridDev(HipContext& ctx, const float K[4], const float* distCoef, int nDist, int width, int height) : ctx_(ctx) {
  check(ccm_frame_create(ctx.get(), K, distCoef, nDist, width, height, &f_), ctx.get(), "ccm_frame_create");
  float b[4];
  ccm_frame_bounds(f_, b);
  mnMinX = b[0]; mnMinY = b[1]; mnMaxX = b[2]; mnMaxY = b[3];
}
FrameGridDev::~FrameGridDev() { ccm_frame_destroy(f_); }

void FrameGridDev::SetKeyPoints(const std::vector<KeyPoint>& mvKeys, const uint8_t* mDescriptors, std::vector<KeyPoint>& mvKeysUn) {
  static_assert(sizeof(KeyPoint) == sizeof(ccm_keypoint), "KeyPoint must mirror ccm_keypoint");
  const int n = (int)mvKeys.size();
  check(ccm_frame_set_keypoints(f_, reinterpret_cast<const ccm_keypoint*>(mvKeys.data()), mDescriptors, n), ctx_.get(), "ccm_frame_set_keypoints");
  std::vector<float> xy(2 * (size_t)std::max(n, 1));
  check(ccm_frame_get(f_, xy.data(), nullptr, nullptr), ctx_.get(), "ccm_frame_get");
  mvKeysUn = mvKeys;                                                  // kp = mvKeys[i]; kp.pt = undistorted (Frame.cpp:304-311)
  for (int i = 0; i < n; i++) { mvKeysUn[i].x = xy[2 * i]; mvKeysUn[i].y = xy[2 * i + 1]; }
}

// every candidate list (GetFeaturesInArea order) and Hamming distance of a batch of window queries in one device call
void ORBmatcher::deviceWindows(FrameGridDev& grid, const std::vector<float>& u, const std::vector<float>& v, const std::vector<float>& r,
                               const std::vector<int32_t>& minl, const std::vector<int32_t>& maxl, const std::vector<uint8_t>& qdesc,
                               std::vector<int32_t>& off, std::vector<int32_t>& idx, std::vector<uint16_t>& dist) {
  const int Q = (int)u.size();
  off.assign(Q + 1, 0);
  int64_t n = 0;
  idx.resize((size_t)Q * 16 + 1024); dist.resize(idx.size());   // typical lists hold a handful of features; grow once if short
  int rc = ccm_frame_window_search(grid.get(), Q, u.data(), v.data(), r.data(), minl.data(), maxl.data(), qdesc.data(), off.data(), idx.data(),
                                   dist.data(), (int64_t)idx.size(), &n);
  if (rc == CCM_E_ARG && n > (int64_t)idx.size()) {
    idx.resize((size_t)n); dist.resize((size_t)n);
    rc = ccm_frame_window_search(grid.get(), Q, u.data(), v.data(), r.data(), minl.data(), maxl.data(), qdesc.data(), off.data(), idx.data(),
                                 dist.data(), n, &n);
  }
  check(rc, ctx_.get(), "ccm_frame_window_search");
  idx.resize((size_t)n); dist.resize((size_t)n);
}

// SearchByProjection(Frame&, vector<mpptr>&, th) with the device grid: ONE ccm_frame_window_search call produces every
// candidate list (GetFeaturesInArea order) and distance; the ordered claim replay below is unchanged.
int ORBmatcher::SearchByProjection(FrameGridDev& grid, FrameView& F, const TrackedMapPoints& mps, float th) {
  const bool bFactor = th != 1.0;
  std::vector<int32_t> q_of, minl, maxl;
  std::vector<float> u, v, r;
  std::vector<uint8_t> qdesc;
  for (int i = 0; i < mps.n; i++) {
    if (!mps.mbTrackInView[i]) continue;
    const int lvl = mps.mnTrackScaleLevel[i];
    float rad = (mps.mTrackViewCos[i] > 0.998) ? 2.5f : 4.0f;   // RadiusByViewingCos (:150-156)
    if (bFactor) rad *= th;
    q_of.push_back(i);
    u.push_back(mps.mTrackProjX[i]); v.push_back(mps.mTrackProjY[i]); r.push_back(rad * F.mvScaleFactors[lvl]);
    minl.push_back(lvl - 1); maxl.push_back(lvl);
    qdesc.insert(qdesc.end(), mps.mDescriptor + (size_t)i * 32, mps.mDescriptor + (size_t)i * 32 + 32);
  }
  const int Q = (int)q_of.size();
  if (Q == 0) return 0;
  std::vector<int32_t> off, idx;
  std::vector<uint16_t> dist;
  deviceWindows(grid, u, v, r, minl, maxl, qdesc, off, idx, dist);
  int nmatches = 0;
  for (int q = 0; q < Q; q++) {
    int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int k = idx[s];
      if (F.mvpMapPoints[k] >= 0) continue;   // F.mvpMapPoints[idx] && Observations() > 0
      const int d = dist[s];
      if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestLevel2 = bestLevel; bestLevel = F.mvKeysUn[k].octave; bestIdx = k; }
      else if (d < bestDist2) { bestLevel2 = F.mvKeysUn[k].octave; bestDist2 = d; }
    }
    if (bestDist <= TH_HIGH) {
      if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue;
      F.mvpMapPoints[bestIdx] = q_of[q];
      nmatches++;
    }
  }
  return nmatches;
}

int ORBmatcher::SearchByProjection(FrameView& C, const LastFrameProjections& last, float th) {
  FrameGrid grid(C);
  std::vector<int32_t> q_of, off(1, 0), idx;
  std::vector<uint8_t> qdesc;
  for (int i = 0; i < last.n; i++) {
    if (!last.valid[i]) continue;
    const int oct = last.octave[i];
    const size_t before = idx.size();
    grid.featuresInArea(last.u[i], last.v[i], th * C.mvScaleFactors[oct], oct - 1, oct + 1, idx);
    if (idx.size() == before) continue;
    q_of.push_back(i);
    off.push_back((int32_t)idx.size());
    qdesc.insert(qdesc.end(), last.mpDescriptor + (size_t)i * 32, last.mpDescriptor + (size_t)i * 32 + 32);
  }
  const int Q = (int)q_of.size();
  int nmatches = 0;
  RotationFilter rot;
  if (Q > 0) {
    std::vector<uint16_t> dist(idx.size());
    check(ccm_hamming_csr(ctx_.get(), qdesc.data(), Q, C.mDescriptors, C.N, off.data(), idx.data(), dist.data(), nullptr, nullptr, nullptr),
          ctx_.get(), "ccm_hamming_csr");
    for (int q = 0; q < Q; q++) {
      int bestDist = 256, bestIdx2 = -1;
      for (int s = off[q]; s < off[q + 1]; s++) {
        const int k = idx[s];
        if (C.mvpMapPoints[k] >= 0) continue;
        if (dist[s] < bestDist) { bestDist = dist[s]; bestIdx2 = k; }
      }
      if (bestDist <= TH_HIGH) {
        C.mvpMapPoints[bestIdx2] = q_of[q];
        nmatches++;
        if (mbCheckOrientation) rot.add(last.angle[q_of[q]] - C.mvKeysUn[bestIdx2].angle, bestIdx2);
      }
    }
  }
  if (mbCheckOrientation) rot.reject_outliers([&](int k) { C.mvpMapPoints[k] = -1; nmatches--; });
  return nmatches;
}

// SearchByProjection(Frame&, const Frame& LastFrame, th) with the device grid (ORBmatcher.cpp:1350-1476)
int ORBmatcher::SearchByProjection(FrameGridDev& grid, FrameView& C, const LastFrameProjections& last, float th) {
  std::vector<int32_t> q_of, minl, maxl;
  std::vector<float> u, v, r;
  std::vector<uint8_t> qdesc;
  for (int i = 0; i < last.n; i++) {
    if (!last.valid[i]) continue;
    const int oct = last.octave[i];
    q_of.push_back(i);
    u.push_back(last.u[i]); v.push_back(last.v[i]); r.push_back(th * C.mvScaleFactors[oct]);
    minl.push_back(oct - 1); maxl.push_back(oct + 1);
    qdesc.insert(qdesc.end(), last.mpDescriptor + (size_t)i * 32, last.mpDescriptor + (size_t)i * 32 + 32);
  }
  const int Q = (int)q_of.size();
  int nmatches = 0;
  RotationFilter rot;
  if (Q > 0) {
    std::vector<int32_t> off, idx;
    std::vector<uint16_t> dist;
    deviceWindows(grid, u, v, r, minl, maxl, qdesc, off, idx, dist);
    for (int q = 0; q < Q; q++) {
      int bestDist = 256, bestIdx2 = -1;
      for (int s = off[q]; s < off[q + 1]; s++) {
        const int k = idx[s];
        if (C.mvpMapPoints[k] >= 0) continue;
        if (dist[s] < bestDist) { bestDist = dist[s]; bestIdx2 = k; }
      }
      if (bestDist <= TH_HIGH) {
        C.mvpMapPoints[bestIdx2] = q_of[q];
        nmatches++;
        if (mbCheckOrientation) rot.add(last.angle[q_of[q]] - C.mvKeysUn[bestIdx2].angle, bestIdx2);
      }
    }
  }
  if (mbCheckOrientation) rot.reject_outliers([&](int k) { C.mvpMapPoints[k] = -1; nmatches--; });
  return nmatches;
}

// ---- SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1478-1604) ------------------------------------------------
namespace {
void guidedCheck(const ccm_guided_pose& pose, const KeyFramePoints& kf, float th) {
  if (kf.n < 0 || (kf.n && (!kf.live || !kf.pos || !kf.min_dist || !kf.max_dist || !kf.desc))) throw std::invalid_argument("SearchByProjection: null keyframe arrays");
  if (pose.nScaleLevels < 1 || pose.nScaleLevels > FSM_MAX_LEVELS) throw std::invalid_argument("SearchByProjection: nScaleLevels must be 1 .. 16");
  if (!(th >= 0.0f) || !(th <= 3.40282347e+38f)) throw std::invalid_argument("SearchByProjection: th must be finite and not negative");
}
std::vector<uint8_t> guidedSkip(const KeyFramePoints& kf, const uint8_t* alreadyFound) {   // :1498-1500
  std::vector<uint8_t> skip((size_t)std::max(kf.n, 1));
  for (int i = 0; i < kf.n; i++) skip[i] = (!kf.live[i] || (alreadyFound && alreadyFound[i])) ? 1 : 0;
  return skip;
}
}  // namespace

void ORBmatcher::GuidedSearchHost(const FrameView& F, const float K[4], const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th,
                                  GuidedCandidates& c) {
  guidedCheck(pose, kf, th);
  const std::vector<uint8_t> skip = guidedSkip(kf, alreadyFound);
  const int P = kf.n;
  c.status.assign(P, GSM_SKIPPED); c.u.assign(P, 0.0f); c.v.assign(P, 0.0f); c.level.assign(P, 0); c.off.assign(P + 1, 0); c.idx.clear(); c.dist.clear();
  float rec[GSM_POSE_FLOATS];
  gsm_pose(pose.Tcw, rec);
  FrameGrid grid(F);
  for (int i = 0; i < P; i++) {
    if (!skip[i]) {
      float r;
      c.status[i] = (uint8_t)gsm_gate(rec, K, F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY, kf.pos + 3 * (size_t)i, kf.min_dist[i], kf.max_dist[i], pose.logScaleFactor,
                                      pose.nScaleLevels, pose.scaleFactors, th, c.u[i], c.v[i], c.level[i], r);
      if (c.status[i] == GSM_SEARCHED) {
        const size_t before = c.idx.size();
        grid.featuresInArea(c.u[i], c.v[i], r, c.level[i] - 1, c.level[i] + 1, c.idx);
        for (size_t s = before; s < c.idx.size(); s++) c.dist.push_back((uint16_t)DescriptorDistance(kf.desc + 32 * (size_t)i, F.mDescriptors + 32 * (size_t)c.idx[s]));
      }
    }
    c.off[i + 1] = (int32_t)c.idx.size();
  }
}

void ORBmatcher::GuidedSearchDevice(HipContext& ctx, FrameGridDev& grid, const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th,
                                    GuidedCandidates& c) {
  guidedCheck(pose, kf, th);
  const std::vector<uint8_t> skip = guidedSkip(kf, alreadyFound);
  const int P = kf.n;
  const size_t n1 = (size_t)std::max(P, 1);
  c.status.assign(n1, 0); c.u.assign(n1, 0.0f); c.v.assign(n1, 0.0f); c.level.assign(n1, 0); c.off.assign((size_t)P + 1, 0);
  int64_t n = 0;
  c.idx.resize((size_t)P * 16 + 1024); c.dist.resize(c.idx.size());   // as deviceWindows: grow once if short
  auto call = [&](int64_t cap) {
    return ccm_frame_guided_search(grid.get(), &pose, P, kf.pos, kf.min_dist, kf.max_dist, kf.desc, skip.data(), th, c.status.data(), c.u.data(), c.v.data(),
                                   c.level.data(), c.off.data(), c.idx.data(), c.dist.data(), cap, &n);
  };
  int rc = call((int64_t)c.idx.size());
  if (rc == CCM_E_ARG && n > (int64_t)c.idx.size()) {
    c.idx.resize((size_t)n); c.dist.resize((size_t)n);
    rc = call(n);
  }
  check(rc, ctx.get(), "ccm_frame_guided_search");
  c.status.resize(P); c.u.resize(P); c.v.resize(P); c.level.resize(P);
  c.idx.resize((size_t)n); c.dist.resize((size_t)n);
}

// The sequential pass (:1494-1602) on the candidate lists: the points in slot order; a feature that holds anything is skipped; the first of equal distances wins;
// a match claims its feature for the points behind it; the rotation histogram takes the keyframe slot's angle minus the frame feature's.
int ORBmatcher::GuidedReplay(FrameView& F, const KeyFramePoints& kf, const GuidedCandidates& c, int ORBdist, bool checkOrientation) {
  if ((int)c.off.size() != kf.n + 1) throw std::invalid_argument("SearchByProjection: the candidate lists are not the keyframe's");
  return ccm_guided::replay(kf.n, c.off.data(), c.idx.data(), c.dist.data(), kf.angle, [&](int i2) { return F.mvKeysUn[i2].angle; }, F.N, F.mvpMapPoints, ORBdist,
                            checkOrientation);
}

int ORBmatcher::SearchByProjection(FrameGridDev& grid, FrameView& F, const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th,
                                   int ORBdist) {
  if (ORBdist < 0 || ORBdist > 255) throw std::invalid_argument("SearchByProjection: ORBdist must be 0 .. 255");
  GuidedCandidates c;
  GuidedSearchDevice(ctx_, grid, pose, kf, alreadyFound, th, c);
  return GuidedReplay(F, kf, c, ORBdist, mbCheckOrientation);
}
int ORBmatcher::SearchByProjection(FrameView& F, const float K[4], const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th,
                                   int ORBdist) {
  if (ORBdist < 0 || ORBdist > 255) throw std::invalid_argument("SearchByProjection: ORBdist must be 0 .. 255");
  GuidedCandidates c;
  GuidedSearchHost(F, K, pose, kf, alreadyFound, th, c);
  return GuidedReplay(F, kf, c, ORBdist, mbCheckOrientation);
}

int ORBmatcher::SearchByProjectionCandidates(FrameView& F, const KeyFramePoints& kf, const int32_t* candOff, const int32_t* candIdx, int ORBdist) {
  if (ORBdist < 0 || ORBdist > 255) throw std::invalid_argument("SearchByProjection: ORBdist must be 0 .. 255");
  if (kf.n < 0 || !candOff || (kf.n && !kf.desc) || candOff[0] != 0) throw std::invalid_argument("SearchByProjection: bad candidate lists");
  for (int i = 0; i < kf.n; i++) if (candOff[i + 1] < candOff[i]) throw std::invalid_argument("SearchByProjection: bad candidate lists");
  GuidedCandidates c;
  c.off.assign(candOff, candOff + kf.n + 1);
  const int n = kf.n ? candOff[kf.n] : 0;
  if (n && !candIdx) throw std::invalid_argument("SearchByProjection: bad candidate lists");
  c.idx.assign(candIdx, candIdx + n);
  for (int32_t k : c.idx) if (k < 0 || k >= F.N) throw std::invalid_argument("SearchByProjection: a candidate the frame does not have");
  const std::vector<uint8_t> qdesc(kf.desc, kf.desc + 32 * (size_t)kf.n);
  distances(qdesc, kf.n, F.mDescriptors, F.N, c.off, c.idx, c.dist);
  return GuidedReplay(F, kf, c, ORBdist, mbCheckOrientation);
}

// ---- BoW-bucketed / triangulation / initialisation searches ---------------------------------------------
namespace {
// common node ids of two ordered FeatureVectors, ascending (the merge-join with lower_bound jumps, ORBmatcher.cpp:199-283)
std::vector<std::pair<int, int>> commonNodes(const FeatureVectorView& a, const FeatureVectorView& b) {
  std::vector<std::pair<int, int>> r;
  int i = 0, j = 0;
  while (i < a.nn && j < b.nn) {
    if (a.node[i] == b.node[j]) { r.emplace_back(i, j); i++; j++; }
    else if (a.node[i] < b.node[j]) i = (int)(std::lower_bound(a.node, a.node + a.nn, b.node[j]) - a.node);
    else j = (int)(std::lower_bound(b.node, b.node + b.nn, a.node[i]) - b.node);
  }
  return r;
}
// queries = features of `a` in bucket order that pass `keep`; candidate list of each = the whole bucket of `b`
template <typename Keep>
void bucketQueries(const KeysView& a, const KeysView& b, Keep keep, std::vector<int32_t>& q_of, std::vector<int32_t>& off,
                   std::vector<int32_t>& idx, std::vector<uint8_t>& qdesc) {
  off.assign(1, 0);
  for (auto pr : commonNodes(a.fv, b.fv))
    for (int s1 = a.fv.off[pr.first]; s1 < a.fv.off[pr.first + 1]; s1++) {
      const int i1 = a.fv.idx[s1];
      if (!keep(i1)) continue;
      q_of.push_back(i1);
      idx.insert(idx.end(), b.fv.idx + b.fv.off[pr.second], b.fv.idx + b.fv.off[pr.second + 1]);
      off.push_back((int32_t)idx.size());
      qdesc.insert(qdesc.end(), a.desc + (size_t)i1 * 32, a.desc + (size_t)i1 * 32 + 32);
    }
}
}  // namespace

void ORBmatcher::distances(const std::vector<uint8_t>& qdesc, int Q, const uint8_t* tdesc, int T, const std::vector<int32_t>& off,
                           const std::vector<int32_t>& idx, std::vector<uint16_t>& dist) {
  dist.assign(std::max<size_t>(idx.size(), 1), 0);
  if (Q == 0 || idx.empty()) return;
  check(ccm_hamming_csr(ctx_.get(), qdesc.data(), Q, tdesc, T, off.data(), idx.data(), dist.data(), nullptr, nullptr, nullptr), ctx_.get(),
        "ccm_hamming_csr");
}

int ORBmatcher::SearchByBoW(const KeysView& KF, const KeysView& F, std::vector<int32_t>& matchesF) {
  matchesF.assign(F.N, -1);
  std::vector<int32_t> q_of, off, idx; std::vector<uint8_t> qdesc; std::vector<uint16_t> dist;
  bucketQueries(KF, F, [&](int i) { return KF.hasMapPoint[i] != 0; }, q_of, off, idx, qdesc);
  distances(qdesc, (int)q_of.size(), F.desc, F.N, off, idx, dist);
  RotationFilter rot;
  int nmatches = 0;
  for (size_t q = 0; q < q_of.size(); q++) {
    int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int realIdxF = idx[s];
      if (matchesF[realIdxF] >= 0) continue;
      const int d = dist[s];
      if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = realIdxF; }
      else if (d < bestDist2) bestDist2 = d;
    }
    if (bestDist1 <= TH_LOW && static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2)) {
      matchesF[bestIdxF] = q_of[q];
      if (mbCheckOrientation) rot.add(KF.keys[q_of[q]].angle - F.keys[bestIdxF].angle, bestIdxF);
      nmatches++;
    }
  }
  if (mbCheckOrientation) rot.reject_outliers([&](int k) { matchesF[k] = -1; nmatches--; });
  return nmatches;
}

int ORBmatcher::SearchByBoW_KF(const KeysView& K1, const KeysView& K2, std::vector<int32_t>& matches12) {
  matches12.assign(K1.N, -1);
  std::vector<int32_t> q_of, off, idx; std::vector<uint8_t> qdesc; std::vector<uint16_t> dist;
  bucketQueries(K1, K2, [&](int i) { return K1.hasMapPoint[i] != 0; }, q_of, off, idx, qdesc);
  distances(qdesc, (int)q_of.size(), K2.desc, K2.N, off, idx, dist);
  std::vector<char> vbMatched2(K2.N, 0);
  RotationFilter rot;
  int nmatches = 0;
  for (size_t q = 0; q < q_of.size(); q++) {
    int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int idx2 = idx[s];
      if (vbMatched2[idx2] || !K2.hasMapPoint[idx2]) continue;
      const int d = dist[s];
      if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = idx2; }
      else if (d < bestDist2) bestDist2 = d;
    }
    if (bestDist1 < TH_LOW && static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2)) {   // strict '<' here (:641)
      matches12[q_of[q]] = bestIdx2;
      vbMatched2[bestIdx2] = 1;
      if (mbCheckOrientation) rot.add(K1.keys[q_of[q]].angle - K2.keys[bestIdx2].angle, q_of[q]);
      nmatches++;
    }
  }
  if (mbCheckOrientation) rot.reject_outliers([&](int k) { matches12[k] = -1; nmatches--; });
  return nmatches;
}

namespace {
// the sequential part of SearchForTriangulation (ORBmatcher.cpp:745-845) from the distances of every (query, candidate) slot: queries in bucket order, the
// candidate list of each = the whole vocabulary node of keyframe 2.  has1 / has2: the map-point flags at the time of the call (a query whose feature has a map
// point by now is skipped like the reference's `if(pMP1) continue`, a candidate with one like `if(vbMatched2[idx2] || pMP2) continue`).
int resolveTriangulation(const KeyPoint* keys1, int N1, const uint8_t* has1, const KeyPoint* keys2, const uint8_t* has2, const std::vector<int32_t>& q_of,
                         const std::vector<int32_t>& off, const std::vector<int32_t>& idx, const uint16_t* dist, const float F12[9], float ex, float ey,
                         const float* sigma2_2, const float* sf2, bool checkOrientation, std::vector<int32_t>& matches12) {
  const int TH_LOW = ORBmatcher::TH_LOW;
  matches12.assign(N1, -1);
  RotationFilter rot;
  int nmatches = 0;
  for (size_t q = 0; q < q_of.size(); q++) {
    if (has1 && has1[q_of[q]]) continue;
    const KeyPoint& kp1 = keys1[q_of[q]];
    int bestDist = TH_LOW, bestIdx2 = -1;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int idx2 = idx[s];
      if (has2[idx2]) continue;          // vbMatched2 is never set by the reference (:761,:789)
      const int d = dist[s];
      if (d > TH_LOW || d > bestDist) continue;
      const KeyPoint& kp2 = keys2[idx2];
      const float distex = ex - kp2.x, distey = ey - kp2.y;
      if (distex * distex + distey * distey < 100 * sf2[kp2.octave]) continue;
      // CheckDistEpipolarLine (:159-176)
      const float a = kp1.x * F12[0] + kp1.y * F12[3] + F12[6];
      const float b = kp1.x * F12[1] + kp1.y * F12[4] + F12[7];
      const float c = kp1.x * F12[2] + kp1.y * F12[5] + F12[8];
      const float num = a * kp2.x + b * kp2.y + c;
      const float den = a * a + b * b;
      if (den == 0) continue;
      const float dsqr = num * num / den;
      if (dsqr < 3.84 * sigma2_2[kp2.octave]) { bestIdx2 = idx2; bestDist = d; }
    }
    if (bestIdx2 >= 0) {
      matches12[q_of[q]] = bestIdx2;
      nmatches++;
      if (checkOrientation) rot.add(kp1.angle - keys2[bestIdx2].angle, q_of[q]);
    }
  }
  if (checkOrientation) rot.reject_outliers([&](int k) { matches12[k] = -1; nmatches--; });
  return nmatches;
}
}  // namespace

int ORBmatcher::SearchForTriangulation(const KeysView& K1, const KeysView& K2, const float F12[9], float ex, float ey, const float* sigma2_2,
                                       const float* sf2, std::vector<int32_t>& matches12) {
  std::vector<int32_t> q_of, off, idx; std::vector<uint8_t> qdesc; std::vector<uint16_t> dist;
  bucketQueries(K1, K2, [&](int i) { return K1.hasMapPoint[i] == 0; }, q_of, off, idx, qdesc);   // only features WITHOUT a map point (:745-749)
  distances(qdesc, (int)q_of.size(), K2.desc, K2.N, off, idx, dist);
  return resolveTriangulation(K1.keys, K1.N, nullptr, K2.keys, K2.hasMapPoint, q_of, off, idx, dist.data(), F12, ex, ey, sigma2_2, sf2, mbCheckOrientation, matches12);
}

TriangulationBatch::TriangulationBatch(ORBmatcher& m, const KeysView& K1, const std::vector<KeysView>& K2) : check_ori_(m.mbCheckOrientation) {
  keys1_.assign(K1.keys, K1.keys + K1.N);
  has1_.assign(K1.hasMapPoint, K1.hasMapPoint + K1.N);
  nb_.resize(K2.size());
  // the queries of all neighbours back to back; candidate indices stay local to the neighbour's own descriptor set
  std::vector<uint8_t> qdesc, tdesc;
  std::vector<int32_t> q_off(1, 0), t_off(1, 0), off_all(1, 0), idx_all;
  for (size_t j = 0; j < K2.size(); j++) {
    Nb& nb = nb_[j];
    nb.keys.assign(K2[j].keys, K2[j].keys + K2[j].N);
    nb.has.assign(K2[j].hasMapPoint, K2[j].hasMapPoint + K2[j].N);
    std::vector<uint8_t> qd;
    bucketQueries(K1, K2[j], [&](int i) { return K1.hasMapPoint[i] == 0; }, nb.q_of, nb.off, nb.idx, qd);
    qdesc.insert(qdesc.end(), qd.begin(), qd.end());
    tdesc.insert(tdesc.end(), K2[j].desc, K2[j].desc + (size_t)K2[j].N * 32);
    const int32_t base = off_all.back();
    for (size_t q = 1; q < nb.off.size(); q++) off_all.push_back(base + nb.off[q]);
    idx_all.insert(idx_all.end(), nb.idx.begin(), nb.idx.end());
    q_off.push_back((int32_t)(qdesc.size() / 32));
    t_off.push_back((int32_t)(tdesc.size() / 32));
  }
  n_cand_ = (int64_t)idx_all.size();
  std::vector<uint16_t> dist_all(std::max<size_t>(idx_all.size(), 1), 0);
  if (!idx_all.empty())
    check(ccm_hamming_csr_multi(m.ctx_.get(), (int)K2.size(), qdesc.data(), q_off.data(), tdesc.data(), t_off.data(), off_all.data(), idx_all.data(), dist_all.data(),
                                nullptr, nullptr, nullptr), m.ctx_.get(), "ccm_hamming_csr_multi");
  size_t at = 0;
  for (Nb& nb : nb_) { nb.dist.assign(dist_all.begin() + at, dist_all.begin() + at + nb.idx.size()); at += nb.idx.size(); }
}

int TriangulationBatch::resolve(int j, const uint8_t* has1_now, const uint8_t* has2_now, const float F12[9], float ex, float ey, const float* sigma2_2, const float* sf2,
                                std::vector<int32_t>& matches12) const {
  const Nb& nb = nb_.at((size_t)j);
  // (the queries were chosen with the flags of the build; a feature that has gained a map point since is skipped, one that had one then cannot lose it here:
  // LocalMapping only adds points to the new keyframe between these calls)
  return resolveTriangulation(keys1_.data(), (int)keys1_.size(), has1_now ? has1_now : nullptr, nb.keys.data(), has2_now ? has2_now : nb.has.data(), nb.q_of, nb.off, nb.idx,
                              nb.dist.data(), F12, ex, ey, sigma2_2, sf2, check_ori_, matches12);
}

int ORBmatcher::SearchForInitialization(const KeysView& F1, const FrameView& F2, std::vector<float>& prev, std::vector<int32_t>& vnMatches12, int windowSize) {
  vnMatches12.assign(F1.N, -1);
  FrameGrid grid(F2);
  std::vector<int32_t> q_of, off(1, 0), idx; std::vector<uint8_t> qdesc; std::vector<uint16_t> dist;
  for (int i1 = 0; i1 < F1.N; i1++) {
    const int level1 = F1.keys[i1].octave;
    if (level1 > 0) continue;
    const size_t before = idx.size();
    grid.featuresInArea(prev[2 * i1], prev[2 * i1 + 1], (float)windowSize, level1, level1, idx);
    if (idx.size() == before) continue;
    q_of.push_back(i1); off.push_back((int32_t)idx.size());
    qdesc.insert(qdesc.end(), F1.desc + (size_t)i1 * 32, F1.desc + (size_t)i1 * 32 + 32);
  }
  distances(qdesc, (int)q_of.size(), F2.mDescriptors, F2.N, off, idx, dist);
  RotationFilter rot;
  std::vector<int> vMatchedDistance(F2.N, INT32_MAX), vnMatches21(F2.N, -1);
  int nmatches = 0;
  for (size_t q = 0; q < q_of.size(); q++) {
    const int i1 = q_of[q];
    int bestDist = INT32_MAX, bestDist2 = INT32_MAX, bestIdx2 = -1;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int i2 = idx[s];
      const int d = dist[s];
      if (vMatchedDistance[i2] <= d) continue;
      if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = i2; }
      else if (d < bestDist2) bestDist2 = d;
    }
    if (bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio) {
      if (vnMatches21[bestIdx2] >= 0) { vnMatches12[vnMatches21[bestIdx2]] = -1; nmatches--; }   // steal-back (:506-510)
      vnMatches12[i1] = bestIdx2;
      vnMatches21[bestIdx2] = i1;
      vMatchedDistance[bestIdx2] = bestDist;
      nmatches++;
      if (mbCheckOrientation) rot.add(F1.keys[i1].angle - F2.mvKeysUn[bestIdx2].angle, i1);
    }
  }
  if (mbCheckOrientation) rot.reject_outliers([&](int idx1) { if (vnMatches12[idx1] >= 0) { vnMatches12[idx1] = -1; nmatches--; } });
  for (int i1 = 0; i1 < F1.N; i1++)
    if (vnMatches12[i1] >= 0) { prev[2 * i1] = F2.mvKeysUn[vnMatches12[i1]].x; prev[2 * i1 + 1] = F2.mvKeysUn[vnMatches12[i1]].y; }
  return nmatches;
}

int ORBmatcher::ProjectedSearch(const FrameView& KF, const float* invLevelSigma2, const ProjectedPoints& P, float th, bool chi2Gate,
                                int distThreshold, int32_t* matched, bool claim, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
  bestIdx.assign(P.n, -1); bestDist.assign(P.n, INT32_MAX);
  std::unique_ptr<FrameGrid> grid;
  if (!P.candOff) grid.reset(new FrameGrid(KF));
  std::vector<int32_t> q_of, off(1, 0), idx; std::vector<uint8_t> qdesc; std::vector<uint16_t> dist;
  for (int i = 0; i < P.n; i++) {
    if (!P.valid[i]) continue;
    const int lvl = P.level[i];
    const size_t before = idx.size();
    std::vector<int32_t> win;
    if (P.candOff) win.assign(P.candIdx + P.candOff[i], P.candIdx + P.candOff[i + 1]);
    else grid->featuresInArea(P.u[i], P.v[i], th * KF.mvScaleFactors[lvl], -1, -1, win);   // KeyFrame::GetFeaturesInArea: no level filter
    for (int k : win) {
      const int kpLevel = KF.mvKeysUn[k].octave;
      if (kpLevel < lvl - 1 || kpLevel > lvl) continue;
      if (chi2Gate) {
        const float ex = P.u[i] - KF.mvKeysUn[k].x, ey = P.v[i] - KF.mvKeysUn[k].y;
        const float e2 = ex * ex + ey * ey;
        if (e2 * invLevelSigma2[kpLevel] > 5.99) continue;
      }
      idx.push_back(k);
    }
    if (idx.size() == before) continue;
    q_of.push_back(i); off.push_back((int32_t)idx.size());
    qdesc.insert(qdesc.end(), P.desc + (size_t)i * 32, P.desc + (size_t)i * 32 + 32);
  }
  distances(qdesc, (int)q_of.size(), KF.mDescriptors, KF.N, off, idx, dist);
  int nacc = 0;
  for (size_t q = 0; q < q_of.size(); q++) {
    const int i = q_of[q];
    int bd = INT32_MAX, bi = -1;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int k = idx[s];
      if (matched && matched[k] >= 0) continue;     // claims made earlier in this loop are honoured
      if (dist[s] < bd) { bd = dist[s]; bi = k; }
    }
    if (bd <= distThreshold) {
      bestIdx[i] = bi; bestDist[i] = bd;
      if (matched && claim && !(P.noClaim && P.noClaim[i])) matched[bi] = i;
      nacc++;
    }
  }
  return nacc;
}

// ProjectedSearch with the keyframe's grid, candidate lists and distances produced on the device: the level window
// [lvl-1, lvl] is applied by the window kernel, the chi2 gate (Fuse, :930-938) during the ordered resolution
int ORBmatcher::ProjectedSearch(FrameGridDev& grid, const FrameView& KF, const float* invLevelSigma2, const ProjectedPoints& P, float th, bool chi2Gate,
                                int distThreshold, int32_t* matched, bool claim, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
  bestIdx.assign(P.n, -1); bestDist.assign(P.n, INT32_MAX);
  std::vector<int32_t> q_of, minl, maxl;
  std::vector<float> u, v, r;
  std::vector<uint8_t> qdesc;
  for (int i = 0; i < P.n; i++) {
    if (!P.valid[i]) continue;
    const int lvl = P.level[i];
    q_of.push_back(i);
    u.push_back(P.u[i]); v.push_back(P.v[i]); r.push_back(th * KF.mvScaleFactors[lvl]);
    minl.push_back(lvl - 1); maxl.push_back(lvl);
    qdesc.insert(qdesc.end(), P.desc + (size_t)i * 32, P.desc + (size_t)i * 32 + 32);
  }
  if (q_of.empty()) return 0;
  std::vector<int32_t> off, idx;
  std::vector<uint16_t> dist;
  deviceWindows(grid, u, v, r, minl, maxl, qdesc, off, idx, dist);
  int nacc = 0;
  for (size_t q = 0; q < q_of.size(); q++) {
    const int i = q_of[q];
    int bd = INT32_MAX, bi = -1;
    for (int s = off[q]; s < off[q + 1]; s++) {
      const int k = idx[s];
      if (chi2Gate) {
        const float ex = P.u[i] - KF.mvKeysUn[k].x, ey = P.v[i] - KF.mvKeysUn[k].y;
        const float e2 = ex * ex + ey * ey;
        if (e2 * invLevelSigma2[KF.mvKeysUn[k].octave] > 5.99) continue;
      }
      if (matched && matched[k] >= 0) continue;     // claims made earlier in this loop are honoured
      if (dist[s] < bd) { bd = dist[s]; bi = k; }
    }
    if (bd <= distThreshold) {
      bestIdx[i] = bi; bestDist[i] = bd;
      if (matched && claim && !(P.noClaim && P.noClaim[i])) matched[bi] = i;
      nacc++;
    }
  }
  return nacc;
}

// ---- FuseBatch: the projected window searches of many target keyframes, Hamming work in one launch ----
FuseBatch::FuseBatch(ORBmatcher& m, const std::vector<Target>& targets, bool chi2Gate, int distThreshold) : tg_(targets.size()), dist_threshold_(distThreshold) {
  const int S = (int)targets.size();
  std::vector<int32_t> q_off(S + 1, 0), t_off(S + 1, 0), cand_off(1, 0), cand_idx;
  std::vector<uint8_t> qdesc, tdesc;
  for (int s = 0; s < S; s++) {
    const Target& T = targets[s];
    const FrameView& KF = T.KF; const ORBmatcher::ProjectedPoints& P = T.P;
    Tg& g = tg_[s];
    g.n_pts = P.n; g.off.assign(1, 0);
    std::unique_ptr<FrameGrid> grid;
    if (!P.candOff) grid.reset(new FrameGrid(KF));
    std::vector<int32_t> win;
    for (int i = 0; i < P.n; i++) {          // candidate lists exactly as ProjectedSearch builds them (window, level window [lvl - 1, lvl], chi2 gate)
      if (!P.valid[i]) continue;
      const int lvl = P.level[i];
      const size_t before = g.idx.size();
      win.clear();
      if (P.candOff) win.assign(P.candIdx + P.candOff[i], P.candIdx + P.candOff[i + 1]);
      else grid->featuresInArea(P.u[i], P.v[i], T.th * KF.mvScaleFactors[lvl], -1, -1, win);
      for (int k : win) {
        const int kpLevel = KF.mvKeysUn[k].octave;
        if (kpLevel < lvl - 1 || kpLevel > lvl) continue;
        if (chi2Gate) {
          const float ex = P.u[i] - KF.mvKeysUn[k].x, ey = P.v[i] - KF.mvKeysUn[k].y;
          const float e2 = ex * ex + ey * ey;
          if (e2 * T.invLevelSigma2[kpLevel] > 5.99) continue;
        }
        g.idx.push_back(k);
      }
      if (g.idx.size() == before) continue;
      g.q_of.push_back(i); g.off.push_back((int32_t)g.idx.size());
      qdesc.insert(qdesc.end(), P.desc + (size_t)i * 32, P.desc + (size_t)i * 32 + 32);
    }
    q_off[s + 1] = q_off[s] + (int32_t)g.q_of.size();
    t_off[s + 1] = t_off[s] + KF.N;
    tdesc.insert(tdesc.end(), KF.mDescriptors, KF.mDescriptors + (size_t)KF.N * 32);
    const int32_t base = cand_off.back();
    for (size_t q = 1; q < g.off.size(); q++) cand_off.push_back(base + g.off[q]);
    cand_idx.insert(cand_idx.end(), g.idx.begin(), g.idx.end());
  }
  n_cand_ = (int64_t)cand_idx.size();
  if (!n_cand_) return;
  std::vector<uint16_t> dist(cand_idx.size());
  check(ccm_hamming_csr_multi(m.ctx_.get(), S, qdesc.data(), q_off.data(), tdesc.data(), t_off.data(), cand_off.data(), cand_idx.data(), dist.data(),
                              nullptr, nullptr, nullptr), m.ctx_.get(), "ccm_hamming_csr_multi");
  size_t at = 0;
  for (int s = 0; s < S; s++) { Tg& g = tg_[s]; g.dist.assign(dist.begin() + at, dist.begin() + at + g.idx.size()); at += g.idx.size(); }
}

int FuseBatch::resolve(int s, const uint8_t* skip_now, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) const {
  const Tg& g = tg_.at(s);
  bestIdx.assign(g.n_pts, -1); bestDist.assign(g.n_pts, INT32_MAX);
  int nacc = 0;
  for (size_t q = 0; q < g.q_of.size(); q++) {
    const int i = g.q_of[q];
    if (skip_now && skip_now[i]) continue;
    int bd = INT32_MAX, bi = -1;
    for (int c = g.off[q]; c < g.off[q + 1]; c++) if (g.dist[c] < bd) { bd = g.dist[c]; bi = g.idx[c]; }   // first minimum wins (:941-945)
    if (bd <= dist_threshold_) { bestIdx[i] = bi; bestDist[i] = bd; nacc++; }
  }
  return nacc;
}

int ORBmatcher::MutualAgreement(const std::vector<int32_t>& vnMatch1, const std::vector<int32_t>& vnMatch2, std::vector<int32_t>& matches12) {
  int nFound = 0;
  matches12.assign(vnMatch1.size(), -1);
  for (size_t i1 = 0; i1 < vnMatch1.size(); i1++) {
    const int idx2 = vnMatch1[i1];
    if (idx2 >= 0 && vnMatch2[idx2] == (int)i1) { matches12[i1] = idx2; nFound++; }
  }
  return nFound;
}

// ---- vocabulary transform / distinctive descriptors ------------------------------------------------------------
ORBVocabulary::ORBVocabulary(HipContext& ctx, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc,
                             const int32_t* word_id, const double* weight) {
  check(ccm_vocab_create(ctx.get(), n_nodes, L, child_off, child_id, node_desc, word_id, weight, &voc_), ctx.get(), "ccm_vocab_create");
  keep(n_nodes, L, child_off, child_id, node_desc, word_id, weight);
}
ORBVocabulary::ORBVocabulary(HipContext* ctx, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id,
                             const double* weight) {
  if (ctx) check(ccm_vocab_create(ctx->get(), n_nodes, L, child_off, child_id, node_desc, word_id, weight, &voc_), ctx->get(), "ccm_vocab_create");
  else if (n_nodes <= 0 || L <= 0 || !child_off || !node_desc || !word_id || !weight || child_off[n_nodes] < 0 || (child_off[n_nodes] && !child_id))
    throw infrastructure_ex("ORBVocabulary: bad args");
  keep(n_nodes, L, child_off, child_id, node_desc, word_id, weight);
}
ORBVocabulary::~ORBVocabulary() { ccm_vocab_destroy(voc_); }
void ORBVocabulary::keep(int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id, const double* weight) {
  n_nodes_ = n_nodes; L_ = L;
  child_off_.assign(child_off, child_off + n_nodes + 1);
  child_id_.assign(child_id, child_id + (child_off[n_nodes] > 0 ? child_off[n_nodes] : 0));
  node_desc_.assign(node_desc, node_desc + 32 * (size_t)n_nodes);
  word_id_.assign(word_id, word_id + n_nodes);
  weight_.assign(weight, weight + n_nodes);
}

void ORBVocabulary::transform(const uint8_t* descriptors, int N, BowVector& v, FeatureVector& fv, int levelsup) const {
  v.word.clear(); v.value.clear(); fv.node.clear(); fv.off.assign(1, 0); fv.idx.clear();
  if (N <= 0) return;
  if (!voc_) throw infrastructure_ex("ORBVocabulary::transform: a vocabulary without a context has no device tree");
  std::vector<int32_t> word(N), node(N); std::vector<double> w(N);
  if (ccm_bow_transform(voc_, descriptors, N, levelsup, word.data(), w.data(), node.data()) != CCM_OK)
    throw infrastructure_ex(std::string("ccm_bow_transform: ") + ccm_last_error(nullptr));
  // TF_IDF weighting + L1 norm (ORBvoc): BowVector::addWeight in feature order, FeatureVector::addFeature, then normalize — the lines of csrc/kfingest_math.h
  std::vector<int32_t> bw(N), fn(N), fo((size_t)N + 1), fi(N);
  std::vector<double> bv(N);
  int32_t nw = 0, nn = 0;
  kfi_vectors_host(N, word.data(), w.data(), node.data(), &nw, bw.data(), bv.data(), &nn, fn.data(), fo.data(), fi.data());
  v.word.assign(bw.begin(), bw.begin() + nw); v.value.assign(bv.begin(), bv.begin() + nw);
  fv.node.assign(fn.begin(), fn.begin() + nn); fv.off.assign(fo.begin(), fo.begin() + nn + 1); fv.idx.assign(fi.begin(), fi.begin() + fo[nn]);
}

std::vector<int32_t> ComputeDistinctiveDescriptors(HipContext& ctx, const uint8_t* desc, const std::vector<int32_t>& off) {
  std::vector<int32_t> best(off.empty() ? 0 : off.size() - 1);
  if (!best.empty()) check(ccm_distinctive_descriptors(ctx.get(), desc, off.data(), (int)best.size(), best.data()), ctx.get(), "ccm_distinctive_descriptors");
  return best;
}

// ---- KeyFrameDatabase --------------------------------------------------------------------------------
KeyFrameDatabase::KeyFrameDatabase(HipContext& ctx, int n_words, int log_capacity) {
  check(ccm_kfdb_create(ctx.get(), n_words, log_capacity, &db_), ctx.get(), "ccm_kfdb_create");
}
KeyFrameDatabase::KeyFrameDatabase(ccm_kfdb* borrowed) : db_(borrowed), owned_(false) {}
KeyFrameDatabase::~KeyFrameDatabase() { if (owned_) ccm_kfdb_destroy(db_); }
void KeyFrameDatabase::add(HipContext& ctx, int64_t key, int32_t client, const BowVector& v) {
  check(ccm_kfdb_add(db_, ctx.get(), key, client, (int)v.word.size(), v.word.data(), v.value.data()), ctx.get(), "ccm_kfdb_add");
}
void KeyFrameDatabase::erase(HipContext& ctx, int64_t key) { check(ccm_kfdb_erase(db_, ctx.get(), key), ctx.get(), "ccm_kfdb_erase"); }
void KeyFrameDatabase::clear(HipContext& ctx) { check(ccm_kfdb_clear(db_, ctx.get()), ctx.get(), "ccm_kfdb_clear"); }

std::vector<int64_t> KeyFrameDatabase::detect(HipContext& ctx, const BowVector& v, float minScore, const ccm_kfdb_filter* f, const Neighbours& neighbours) {
  std::vector<int64_t> key(64); std::vector<int32_t> cnt(64); std::vector<float> si(64); std::vector<double> s64(64);
  int n = 0;
  for (;;) {   // the table rarely outgrows the first guess; then once more with its size
    check(ccm_kfdb_query(db_, ctx.get(), (int)v.word.size(), v.word.data(), v.value.data(), f, (int)key.size(), key.data(), cnt.data(), si.data(), s64.data(),
                         &n, nullptr, nullptr, nullptr), ctx.get(), "ccm_kfdb_query");
    if (n <= (int)key.size()) break;
    key.resize(n); cnt.resize(n); si.resize(n); s64.resize(n);
  }
  key.resize(n); si.resize(n);
  return kfdb::resolve(key, si, minScore, neighbours);
}
std::vector<int64_t> KeyFrameDatabase::DetectLoopCandidates(HipContext& ctx, int64_t key, const BowVector& v, float minScore, const std::vector<int64_t>* map_keys,
                                                            const std::vector<int64_t>& connected, const Neighbours& neighbours) {
  ccm_kfdb_filter f{key, map_keys ? map_keys->data() : nullptr, map_keys ? (int)map_keys->size() : 0, connected.data(), (int)connected.size(), 0};
  static const int64_t none = 0;
  if (map_keys && map_keys->empty()) f.allow = &none;   // an empty map admits nothing
  return detect(ctx, v, minScore, &f, neighbours);
}
std::vector<int64_t> KeyFrameDatabase::DetectMapMatchCandidates(HipContext& ctx, const BowVector& v, float minScore, uint64_t ass_clients, const Neighbours& neighbours) {
  ccm_kfdb_filter f{-1, nullptr, 0, nullptr, 0, ass_clients};
  return detect(ctx, v, minScore, &f, neighbours);
}
std::vector<int64_t> KeyFrameDatabase::DetectRelocalizationCandidates(HipContext& ctx, const BowVector& v, const Neighbours& neighbours) {
  return detect(ctx, v, 0.0f, nullptr, neighbours);   // kfdb_resolve.h: relocalisation = the same phase 2 with minScore 0
}

// ---- Optimizer ---------------------------------------------------------------------------------------
int Optimizer::PoseOptimizationClient(HipContext& ctx, double cam_qt[7], int n, const double* Xw, const double* obs,
                                      const double* invSigma2, const double K[4], std::vector<uint8_t>& outlier) {
  outlier.assign(std::max(n, 1), 0);
  int ninl = 0;
  check(ccm_pose_optimize(ctx.get(), cam_qt, n, Xw, obs, invSigma2, K, outlier.data(), &ninl), ctx.get(), "ccm_pose_optimize");
  outlier.resize(n);
  return ninl;
}

// ---- RelocalizationRefine ------------------------------------------------------------------------------------------------------
namespace {
// Optimizer::PoseOptimizationClient(Frame&) on the views: the correspondences in ascending feature order, the conversions of ccm_convert.h.  Fewer than three
// correspondences return 0 and leave the pose.
int relocPoseOptimization(HipContext& ctx, const FrameView& F, const float K[4], const float* invLevelSigma2, const KeyFramePoints& kf, float Tcw[16],
                          std::vector<uint8_t>& mvbOutlier) {
  double cam_qt[7];
  ccmh::toSE3Quat(Tcw, cam_qt);
  std::vector<double> Xw, obs, info;
  std::vector<int> slot;
  for (int i = 0; i < F.N; i++) {
    const int32_t s = F.mvpMapPoints[i];
    if (s < 0) continue;
    mvbOutlier[i] = 0;
    const KeyPoint& kp = F.mvKeysUn[i];
    obs.insert(obs.end(), {(double)kp.x, (double)kp.y});
    info.push_back((double)invLevelSigma2[kp.octave]);
    Xw.insert(Xw.end(), {(double)kf.pos[3 * (size_t)s], (double)kf.pos[3 * (size_t)s + 1], (double)kf.pos[3 * (size_t)s + 2]});
    slot.push_back(i);
  }
  if (slot.size() < 3) return 0;
  const double Kd[4] = {(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  std::vector<uint8_t> outlier;
  const int nInliers = Optimizer::PoseOptimizationClient(ctx, cam_qt, (int)slot.size(), Xw.data(), obs.data(), info.data(), Kd, outlier);
  for (size_t e = 0; e < slot.size(); e++) mvbOutlier[slot[e]] = outlier[e] != 0;
  ccmh::toCvMat(cam_qt, Tcw);
  return nInliers;
}
}  // namespace

RelocRefineResult RelocalizationRefine(HipContext& ctx, FrameGridDev& grid, FrameView& F, const float K[4], const float* mvInvLevelSigma2,
                                       const ccm_guided_pose& frame, const KeyFramePoints& kf, const int32_t* matchesF, const uint8_t* vbInliers) {
  if (F.N < 0 || (F.N && (!F.mvpMapPoints || !F.mvKeysUn || !matchesF || !vbInliers || !mvInvLevelSigma2)) || !K) throw std::invalid_argument("RelocalizationRefine: null arguments");
  RelocRefineResult res;
  ORBmatcher matcher2(ctx, 0.9f, true);
  std::vector<uint8_t> found((size_t)std::max(kf.n, 1), 0), mvbOutlier((size_t)std::max(F.N, 1), 0);
  for (int j = 0; j < F.N; j++) {   // the seed
    const int32_t s = vbInliers[j] ? matchesF[j] : -1;
    if (s >= kf.n) throw std::invalid_argument("RelocalizationRefine: matchesF names a slot the keyframe does not have");
    F.mvpMapPoints[j] = s < 0 ? -1 : s;
    if (s >= 0) found[s] = 1;
  }
  ccm_guided_pose pose = frame;
  float* Tcw = res.Tcw;
  memcpy(Tcw, frame.Tcw, sizeof(float) * 12);
  Tcw[12] = 0.f; Tcw[13] = 0.f; Tcw[14] = 0.f; Tcw[15] = 1.f;
  auto optimise = [&] { return relocPoseOptimization(ctx, F, K, mvInvLevelSigma2, kf, Tcw, mvbOutlier); };
  auto clearOutliers = [&] { for (int j = 0; j < F.N; j++) if (mvbOutlier[j]) F.mvpMapPoints[j] = -1; };
  auto search = [&](float th, int ORBdist) {
    memcpy(pose.Tcw, Tcw, sizeof(float) * 12);
    return matcher2.SearchByProjection(grid, F, pose, kf, found.data(), th, ORBdist);
  };
  int nGood = res.trace[0] = optimise();
  if (nGood >= 10) {
    clearOutliers();
    if (nGood < 50) {
      const int nadditional = res.trace[1] = search(10.0f, 100);
      if (nadditional + nGood >= 50) {
        nGood = res.trace[2] = optimise();
        if (nGood > 30 && nGood < 50) {   // many inliers but still not enough: a narrower window, the pose being better (the outliers stay in the set)
          std::fill(found.begin(), found.end(), 0);
          for (int j = 0; j < F.N; j++) if (F.mvpMapPoints[j] >= 0) found[F.mvpMapPoints[j]] = 1;
          const int nadd2 = res.trace[3] = search(3.0f, 64);
          if (nGood + nadd2 >= 50) {
            nGood = res.trace[4] = optimise();
            clearOutliers();
          }
        }
      }
    }
  }
  res.nGood = nGood;
  res.matched = nGood >= 50;
  return res;
}

int Optimizer::OptimizeSim3(HipContext& ctx, double g2oS12[8], int n, const double* P1c, const double* P2c, const double* obs1,
                            const double* obs2, const double* invSigma2_1, const double* invSigma2_2, const double K1[4],
                            const double K2[4], float th2, bool bFixScale, std::vector<uint8_t>& keep) {
  keep.assign(std::max(n, 1), 0);
  int nin = 0;
  check(ccm_sim3_optimize(ctx.get(), g2oS12, n, P1c, P2c, obs1, obs2, invSigma2_1, invSigma2_2, K1, K2, (double)th2,
                          bFixScale ? 1 : 0, keep.data(), &nin), ctx.get(), "ccm_sim3_optimize");
  keep.resize(n);
  return nin;
}

void Optimizer::OptimizeEssentialGraph(HipContext& ctx, std::vector<double>& vScw, const std::vector<uint8_t>& fixed, bool bFixScale,
                                       const std::vector<int32_t>& e_i, const std::vector<int32_t>& e_j, const std::vector<double>& Sji,
                                       ccm_pg_stats* stats) {
  const int n_vert = (int)fixed.size(), n_edge = (int)e_i.size();
  if ((int)vScw.size() != 8 * n_vert || (int)e_j.size() != n_edge || (int)Sji.size() != 8 * n_edge) throw infrastructure_ex("OptimizeEssentialGraph: inconsistent sizes");
  check(ccm_pose_graph_optimize(ctx.get(), n_vert, vScw.data(), fixed.data(), bFixScale ? 1 : 0, n_edge, e_i.data(), e_j.data(), Sji.data(), 20, 1e-16,
                                nullptr, stats), ctx.get(), "ccm_pose_graph_optimize");
}

static ccm_ba_problem make_problem(BAProblem& p, const uint8_t* level, double huber) {
  ccm_ba_problem c{};
  c.n_cam = p.n_cam(); c.n_pt = p.n_pt(); c.n_edge = p.n_edge();
  c.cam_qt = p.cam_qt.data(); c.cam_fixed = p.cam_fixed.data(); c.cam_K = p.cam_K.data(); c.pt_xyz = p.pt_xyz.data();
  c.e_cam = p.e_cam.data(); c.e_pt = p.e_pt.data(); c.e_obs = p.e_obs.data(); c.e_info = p.e_info.data();
  c.e_level = level; c.huber_delta = huber;
  return c;
}

void Optimizer::LocalBundleAdjustmentClient(HipContext& ctx, BAProblem& p, bool* pbStopFlag, std::vector<uint8_t>& to_erase) {
  const int ne = p.n_edge();
  to_erase.assign(ne, 0);
  if (pbStopFlag && *pbStopFlag) return;   // :532-534
  const double thHuberMono = (double)(float)std::sqrt(5.991);   // const float thHuberMono = sqrt(5.991) (:468)
  std::vector<uint8_t> level(ne, 0), dpos(ne, 1);
  std::vector<double> chi2(ne, 0.0);
  ccm_ba_options opt{}; opt.max_iters = 5;
  ccm_ba_problem c = make_problem(p, level.data(), thHuberMono);
  const volatile unsigned char* stop = reinterpret_cast<const volatile unsigned char*>(pbStopFlag);
  check(ccm_ba_optimize(ctx.get(), &c, &opt, stop, chi2.data(), dpos.data(), nullptr), ctx.get(), "ccm_ba_optimize");
  bool bDoMore = !(pbStopFlag && *pbStopFlag);
  if (bDoMore) {
    for (int e = 0; e < ne; e++) if (chi2[e] > 5.991 || !dpos[e]) level[e] = 1;   // setLevel(1); kernel dropped for all (:548-560)
    opt.max_iters = 10;
    c = make_problem(p, level.data(), 0.0);
    check(ccm_ba_optimize(ctx.get(), &c, &opt, stop, chi2.data(), dpos.data(), nullptr), ctx.get(), "ccm_ba_optimize");
  }
  for (int e = 0; e < ne; e++) to_erase[e] = (chi2[e] > 5.991 || !dpos[e]) ? 1 : 0;   // :574-586
}

void Optimizer::GlobalBundleAdjustment(HipContext& ctx, BAProblem& p, int nIterations, bool* pbStopFlag, bool bRobust, ccm_ba_stats* stats) {
  const double thHuber2D = (double)(float)std::sqrt(5.99);   // :759
  ccm_ba_options opt{}; opt.max_iters = nIterations;
  ccm_ba_problem c = make_problem(p, nullptr, bRobust ? thHuber2D : 0.0);
  check(ccm_ba_optimize(ctx.get(), &c, &opt, reinterpret_cast<const volatile unsigned char*>(pbStopFlag), nullptr, nullptr, stats),
        ctx.get(), "ccm_ba_optimize");
}

// ---- what the two RANSAC batches share --------------------------------------------------------------
bool RansacCsr::append(int N, int S) {
  if (N < S) { remap.push_back(-1); return false; }   // never evaluated (N < minInliers, checked by the schedule)
  remap.push_back(K());
  pt_off.push_back(pt_off.back() + N);
  return true;
}

size_t RansacCsr::rows(const std::vector<int32_t>& hyp_cand) {
  cand_buf.resize(hyp_cand.size());
  size_t words = 0;
  for (size_t h = 0; h < hyp_cand.size(); h++) {
    const int r = remap[hyp_cand[h]];
    if (r < 0) throw std::invalid_argument("RANSAC batch: a hypothesis of a candidate with fewer points than a sample");
    cand_buf[h] = r;
    words += (pt_off[r + 1] - pt_off[r] + 31) / 32;
  }
  return words;
}

// a candidate's inlier bits -> vbInliers (n flags) through its index list
static void mask_to_inliers(const std::vector<uint32_t>& mask, const std::vector<int32_t>& idx, int n, std::vector<bool>& vbInliers) {
  vbInliers.assign(n, false);
  for (size_t i = 0; i < idx.size(); i++)
    if (mask[i >> 5] >> (i & 31) & 1u) vbInliers[idx[i]] = true;
}

// ---- Sim3RansacBatch ------------------------------------------------------------------------------
static std::vector<int> sim3_sizes(const std::vector<Sim3Candidate>& c) {
  std::vector<int> n;
  for (const auto& x : c) {
    if (x.X3Dc1.size() != 3 * x.indices1.size() || x.X3Dc2.size() != x.X3Dc1.size() || x.max_err1.size() != x.indices1.size() ||
        x.max_err2.size() != x.indices1.size())
      throw std::invalid_argument("Sim3Candidate: inconsistent sizes");
    for (int32_t i : x.indices1)
      if (i < 0 || i >= x.n1) throw std::invalid_argument("Sim3Candidate: mvnIndices1 outside [0, mN1)");
    n.push_back((int)x.indices1.size());
  }
  return n;
}

Sim3RansacBatch::Sim3RansacBatch(HipContext& ctx, std::vector<Sim3Candidate> cands, const ccm_sim3::Params& p, bool fix_scale, ccm_sim3::DrawSource src)
    : cands_(std::move(cands)), sched_(sim3_sizes(cands_), p, std::move(src)) {
  eval_.ctx = &ctx;
  eval_.fix_scale = fix_scale ? 1 : 0;
  for (const auto& c : cands_)
    eval_.add((int)c.indices1.size(), c.X3Dc1.data(), c.X3Dc2.data(), c.K1, c.K2, c.max_err1.data(), c.max_err2.data());
}

void Sim3RansacBatch::Eval::add(int N, const float* x1, const float* x2, const float* k1, const float* k2, const uint32_t* thr1, const uint32_t* thr2) {
  if (!append(N, 3)) return;
  X1.insert(X1.end(), x1, x1 + 3 * (size_t)N); X2.insert(X2.end(), x2, x2 + 3 * (size_t)N);
  K1.insert(K1.end(), k1, k1 + 4); K2.insert(K2.end(), k2, k2 + 4);
  t1.insert(t1.end(), thr1, thr1 + N); t2.insert(t2.end(), thr2, thr2 + N);
}

void Sim3RansacBatch::Eval::operator()(const std::vector<int32_t>& hyp_cand, const std::vector<int32_t>& hyp_idx, std::vector<int32_t>& n_inl,
                                       std::vector<float>& rts, std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask) {
  const int H = (int)hyp_cand.size();
  const size_t words = rows(hyp_cand);
  n_inl.resize(H); rts.resize(13 * (size_t)H); mask_off.resize(H + 1); mask.resize(words);
  check(ccm_sim3_ransac_eval(ctx->get(), K(), pt_off.data(), X1.data(), X2.data(), K1.data(), K2.data(), t1.data(), t2.data(), H, cand_buf.data(),
                             hyp_idx.data(), fix_scale, n_inl.data(), rts.data(), mask_off.data(), mask.data()),
        ctx->get(), "ccm_sim3_ransac_eval");
}

bool Sim3RansacBatch::next(int& cand, float R[9], float t[3], float& s, std::vector<bool>& vbInliers, int& nInliers) {
  ccm_sim3::Event ev;
  if (!sched_.next(eval_, ev)) return false;
  const Sim3Candidate& c = cands_[ev.cand];
  cand = ev.cand;
  for (int i = 0; i < 9; i++) R[i] = ev.R[i];
  for (int i = 0; i < 3; i++) t[i] = ev.t[i];
  s = ev.s;
  nInliers = ev.n_inliers;
  mask_to_inliers(ev.mask, c.indices1, c.n1, vbInliers);
  return true;
}

// ---- PnPRansacBatch -------------------------------------------------------------------------------
static std::vector<ccm_pnp::Candidate> pnp_base(const std::vector<PnPCandidate>& c) {
  std::vector<ccm_pnp::Candidate> b;
  for (const auto& x : c) {
    if (x.keypoint_indices.size() != x.sigma2.size()) throw std::invalid_argument("PnPCandidate: inconsistent sizes");
    for (int32_t i : x.keypoint_indices)
      if (i < 0 || i >= x.n_matches) throw std::invalid_argument("PnPCandidate: mvKeyPointIndices outside the matches");
    b.push_back(x);
  }
  return b;
}

PnPRansacBatch::PnPRansacBatch(HipContext* ctx, std::vector<PnPCandidate> cands, const ccm_pnp::Params& p, ccm_pnp::DrawSource src)
    : sched_(pnp_base(cands), p, std::move(src)) {
  eval_.ctx = ctx;
  for (size_t c = 0; c < cands.size(); c++) {
    const PnPCandidate& x = cands[c];
    n_matches_.push_back(x.n_matches);
    kp_idx_.push_back(x.keypoint_indices);
    if (!eval_.append(x.N(), 4)) continue;
    eval_.P3Dw.insert(eval_.P3Dw.end(), x.P3Dw.begin(), x.P3Dw.end());
    eval_.P2D.insert(eval_.P2D.end(), x.P2D.begin(), x.P2D.end());
    const std::vector<float>& me = sched_.max_err((int)c);
    eval_.max_err.insert(eval_.max_err.end(), me.begin(), me.end());
    eval_.cam.insert(eval_.cam.end(), x.cam, x.cam + 4);
  }
}

void PnPRansacBatch::Eval::operator()(const std::vector<int32_t>& hyp_cand, const std::vector<int32_t>& hyp_idx, std::vector<int32_t>& n_inl,
                                      std::vector<double>& Rt, std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask) {
  const int H = (int)hyp_cand.size(), K = this->K();
  const size_t words = rows(hyp_cand);
  n_inl.resize(H); Rt.resize(12 * (size_t)H); mask_off.resize(H + 1); mask.resize(words);
  if (!ctx) {
    if (ccm_pnp::eval_host(K, pt_off.data(), P3Dw.data(), P2D.data(), max_err.data(), cam.data(), H, cand_buf.data(), hyp_idx.data(), n_inl.data(), Rt.data(),
                           mask_off.data(), mask.data()))
      throw std::invalid_argument("PnPRansacBatch: bad hypotheses");
    return;
  }
  check(ccm_pnp_ransac_eval(ctx->get(), K, pt_off.data(), P3Dw.data(), P2D.data(), max_err.data(), cam.data(), H, cand_buf.data(), hyp_idx.data(), n_inl.data(),
                            Rt.data(), mask_off.data(), mask.data()),
        ctx->get(), "ccm_pnp_ransac_eval");
}

void PnPRansacBatch::fill(const ccm_pnp::Event& ev, Pose& out) const {
  out.cand = ev.cand; out.nInliers = ev.n_inliers; out.refined = ev.refined; out.bNoMore = ev.no_more;
  std::copy(ev.Tcw, ev.Tcw + 16, out.Tcw);
  mask_to_inliers(ev.mask, kp_idx_[ev.cand], n_matches_[ev.cand], out.vbInliers);
}

bool PnPRansacBatch::next(Pose& out) {
  ccm_pnp::Event ev;
  if (!sched_.next(eval_, ev)) return false;
  fill(ev, out);
  return true;
}

bool PnPRansacBatch::iterate(int c, int nIterations, bool& bNoMore, Pose& out) {
  if (c < 0 || c >= (int)kp_idx_.size()) throw std::invalid_argument("PnPRansacBatch::iterate: no such candidate");
  ccm_pnp::Event ev;
  if (!sched_.iterate(eval_, c, nIterations, ev, bNoMore)) return false;
  fill(ev, out);
  return true;
}

// ---- TwoViewInitializer -------------------------------------------------------------------------------
// twoview_math.h on the calling thread with the arguments of ccm_twoview_ransac_eval; model: 0 both, 1 the homography only, 2 the fundamental matrix only
int detail::twoview_ransac_host(int N, const float* xy1, const float* xy2, const float* pn1, const float* pn2, const float* T1, const float* T2inv, const float* T2t,
                               float sigma, int H, const int32_t* sets, int model, float* scoreH, float* scoreF, float* H21, float* F21, uint32_t* maskH,
                               uint32_t* maskF) {
  if (N < 8 || H < 1 || !xy1 || !xy2 || !pn1 || !pn2 || !T1 || !T2inv || !T2t || !sets) return -1;
  if (model != 2 && (!scoreH || !H21 || !maskH)) return -1;
  if (model != 1 && (!scoreF || !F21 || !maskF)) return -1;
  const size_t words = ((size_t)N + 31) / 32;
  for (int h = 0; h < H; h++) {
    float p1[16], p2[16];
    for (int j = 0; j < 8; j++) {
      const int32_t idx = sets[8 * (size_t)h + j];
      if (idx < 0 || idx >= N) return -1;
      for (int k = 0; k < j; k++) if (sets[8 * (size_t)h + k] == idx) return -1;
      p1[2 * j] = pn1[2 * idx]; p1[2 * j + 1] = pn1[2 * idx + 1]; p2[2 * j] = pn2[2 * idx]; p2[2 * j + 1] = pn2[2 * idx + 1];
    }
    if (model != 2) {
      float H12[9];
      tv_model_h(p1, p2, T1, T2inv, H21 + 9 * (size_t)h, H12);
      scoreH[h] = tv_score(true, H21 + 9 * (size_t)h, H12, N, xy1, xy2, sigma, maskH + words * h);
    }
    if (model != 1) {
      tv_model_f(p1, p2, T1, T2t, F21 + 9 * (size_t)h);
      scoreF[h] = tv_score(false, F21 + 9 * (size_t)h, nullptr, N, xy1, xy2, sigma, maskF + words * h);
    }
  }
  return 0;
}

int detail::twoview_check_rt_host(int n_hyp, const float* rec, const float* K, int N, const float* xy1, const float* xy2, const uint32_t* inl, float th2,
                                 uint8_t* status, float* x3d, float* cosp) {
  if (n_hyp < 1 || n_hyp > 8 || N < 1 || !rec || !K || !xy1 || !xy2 || !inl || !status || !x3d || !cosp) return -1;
  for (int q = 0; q < n_hyp; q++) {
    TvMotion m;
    std::memcpy(&m, rec + TV_REC_FLOATS * (size_t)q, sizeof m);
    for (int i = 0; i < N; i++) {
      const size_t o = (size_t)q * N + i;
      x3d[3 * o] = x3d[3 * o + 1] = x3d[3 * o + 2] = cosp[o] = NAN;
      status[o] = TV_NOT_INLIER;
      if ((inl[i >> 5] >> (i & 31)) & 1u) status[o] = (uint8_t)tv_check_rt(K, m, xy1[2 * i], xy1[2 * i + 1], xy2[2 * i], xy2[2 * i + 1], th2, x3d + 3 * o, cosp[o]);
    }
  }
  return 0;
}

TwoViewInitializer::TwoViewInitializer(HipContext* ctx, const float K[9], std::vector<float> keys1, float sigma) : ctx_(ctx), sigma_(sigma), keys1_(std::move(keys1)) {
  if (!K || keys1_.size() % 2) throw infrastructure_ex("TwoViewInitializer: K and x y pairs");
  std::memcpy(K_, K, sizeof K_);
}

TwoViewInitializer::Sets TwoViewInitializer::DrawSets(int N, int iterations, const std::function<int()>& rand) {
  if (N < 8 || iterations < 0) throw infrastructure_ex("TwoViewInitializer::DrawSets: fewer than 8 matches");
  Sets sets((size_t)iterations * 8, 0);
  std::vector<int32_t> all((size_t)N), avail;
  for (int i = 0; i < N; i++) all[i] = i;
  for (int it = 0; it < iterations; it++) {
    avail = all;
    for (int j = 0; j < 8; j++) {
      const int randi = ccm_sim3::random_int(rand(), (int)avail.size());   // DUtils::Random::RandomInt(0, size - 1)
      sets[8 * (size_t)it + j] = avail[randi];
      avail[randi] = avail.back();
      avail.pop_back();
    }
  }
  return sets;
}

TwoViewInitializer::Models TwoViewInitializer::FindModels(std::vector<float> keys2, const std::vector<int>& vMatches12, const Sets& sets) {
  if (keys2.size() % 2 || vMatches12.size() > keys1_.size() / 2 || sets.empty() || sets.size() % 8) throw infrastructure_ex("TwoViewInitializer::FindModels: bad arguments");
  keys2_ = std::move(keys2);
  first_.clear(); xy1_.clear(); xy2_.clear();
  const int N1 = (int)(keys1_.size() / 2), N2 = (int)(keys2_.size() / 2);
  // Normalize runs over ALL keypoints of each frame; the matched ones are then picked in match order
  std::vector<float> n1(keys1_.size()), n2(keys2_.size()), pn1, pn2;
  float T1[9], T2[9], T2inv[9], T2t[9];
  tv_normalize(keys1_.data(), N1, n1.data(), T1);
  tv_normalize(keys2_.data(), N2, n2.data(), T2);
  tv_inv33(T2, T2inv);
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) T2t[3 * r + c] = T2[3 * c + r];
  for (size_t i = 0; i < vMatches12.size(); i++) {
    const int j = vMatches12[i];
    if (j < 0) continue;
    if (j >= N2) throw infrastructure_ex("TwoViewInitializer::FindModels: match out of range");
    first_.push_back((int32_t)i);
    xy1_.insert(xy1_.end(), {keys1_[2 * i], keys1_[2 * i + 1]}); xy2_.insert(xy2_.end(), {keys2_[2 * j], keys2_[2 * j + 1]});
    pn1.insert(pn1.end(), {n1[2 * i], n1[2 * i + 1]}); pn2.insert(pn2.end(), {n2[2 * j], n2[2 * j + 1]});
  }
  const int N = (int)first_.size(), H = (int)(sets.size() / 8);
  if (N < 8) throw infrastructure_ex("TwoViewInitializer::FindModels: fewer than 8 matches");
  const size_t words = ((size_t)N + 31) / 32;
  std::vector<float> sH((size_t)H), sF((size_t)H), H21(9 * (size_t)H), F21(9 * (size_t)H);
  std::vector<uint32_t> mH(words * H), mF(words * H);
  if (ctx_) {
    const int rc = ccm_twoview_ransac_eval(ctx_->get(), N, xy1_.data(), xy2_.data(), pn1.data(), pn2.data(), T1, T2inv, T2t, sigma_, H, sets.data(), sH.data(), sF.data(),
                                           H21.data(), F21.data(), mH.data(), mF.data());
    if (rc != CCM_OK) throw infrastructure_ex(std::string("ccm_twoview_ransac_eval: ") + ccm_last_error(ctx_->get()));
  } else if (detail::twoview_ransac_host(N, xy1_.data(), xy2_.data(), pn1.data(), pn2.data(), T1, T2inv, T2t, sigma_, H, sets.data(), 0, sH.data(), sF.data(), H21.data(),
                                 F21.data(), mH.data(), mF.data()) != 0) {
    throw infrastructure_ex("TwoViewInitializer::FindModels: a set index out of range or repeated");
  }
  // `if(currentScore>score)` from score = 0, in order: the first strictly greater score wins; a NaN or zero score never does
  Models m;
  m.vbMatchesInliersH.assign((size_t)N, false); m.vbMatchesInliersF.assign((size_t)N, false);
  for (int h = 0; h < H; h++) {
    if (sH[h] > m.SH) { m.SH = sH[h]; m.bestH = h; }
    if (sF[h] > m.SF) { m.SF = sF[h]; m.bestF = h; }
  }
  if (m.bestH >= 0) {
    std::memcpy(m.H21, &H21[9 * (size_t)m.bestH], sizeof m.H21);
    for (int i = 0; i < N; i++) m.vbMatchesInliersH[i] = (mH[words * m.bestH + (i >> 5)] >> (i & 31)) & 1u;
  }
  if (m.bestF >= 0) {
    std::memcpy(m.F21, &F21[9 * (size_t)m.bestF], sizeof m.F21);
    for (int i = 0; i < N; i++) m.vbMatchesInliersF[i] = (mF[words * m.bestF + (i >> 5)] >> (i & 31)) & 1u;
  }
  m.RH = m.SH / (m.SH + m.SF);
  return m;
}

std::vector<TwoViewInitializer::Reconstruction> TwoViewInitializer::CheckRTBatch(const std::vector<Motion>& hyp, const std::vector<bool>& inliers, float th2) {
  const int N = (int)first_.size(), Q = (int)hyp.size();
  if (N < 1 || Q < 1 || Q > 8 || (int)inliers.size() != N) throw infrastructure_ex("TwoViewInitializer::CheckRTBatch: 1 to 8 hypotheses, one inlier flag per match");
  std::vector<float> rec((size_t)TV_REC_FLOATS * Q);
  for (int q = 0; q < Q; q++) {
    TvMotion m;
    tv_prepare_rt(K_, hyp[q].R, hyp[q].t, m);
    std::memcpy(&rec[(size_t)TV_REC_FLOATS * q], &m, sizeof m);
  }
  std::vector<uint32_t> mask(((size_t)N + 31) / 32, 0u);
  for (int i = 0; i < N; i++) if (inliers[i]) mask[i >> 5] |= 1u << (i & 31);
  std::vector<uint8_t> status((size_t)N * Q);
  std::vector<float> x3d(3 * (size_t)N * Q), cosp((size_t)N * Q);
  if (ctx_) {
    const int rc = ccm_twoview_check_rt(ctx_->get(), Q, rec.data(), K_, N, xy1_.data(), xy2_.data(), mask.data(), th2, status.data(), x3d.data(), cosp.data());
    if (rc != CCM_OK) throw infrastructure_ex(std::string("ccm_twoview_check_rt: ") + ccm_last_error(ctx_->get()));
  } else {
    detail::twoview_check_rt_host(Q, rec.data(), K_, N, xy1_.data(), xy2_.data(), mask.data(), th2, status.data(), x3d.data(), cosp.data());
  }
  std::vector<Reconstruction> out((size_t)Q);
  const size_t N1 = keys1_.size() / 2;
  for (int q = 0; q < Q; q++) {
    Reconstruction& r = out[q];
    r.vP3D.assign(3 * N1, 0.f); r.vbGood.assign(N1, false);
    r.status.assign(status.begin() + (size_t)q * N, status.begin() + (size_t)(q + 1) * N);
    std::vector<float> vCosParallax;
    for (int i = 0; i < N; i++) {
      const size_t o = (size_t)q * N + i;
      if (status[o] < TV_COUNTED) continue;
      vCosParallax.push_back(cosp[o]);
      for (int k = 0; k < 3; k++) r.vP3D[3 * (size_t)first_[i] + k] = x3d[3 * o + k];
      r.nGood++;
      if (status[o] == TV_GOOD) r.vbGood[first_[i]] = true;
    }
    if (r.nGood > 0) {
      std::sort(vCosParallax.begin(), vCosParallax.end());
      const size_t idx = std::min(50, int(vCosParallax.size() - 1));
      r.parallax = (float)((double)(acosf(vCosParallax[idx]) * 180) / 3.1415926535897932384626433832795);   // acos(...) * 180 / CV_PI
    }
  }
  return out;
}

// ---- NewMapPointBatch ---------------------------------------------------------------------------------
static_assert(sizeof(CamRecord) == sizeof(TriCam) && sizeof(TriCam) == TRI_CAM_FLOATS * sizeof(float), "camera record layout");

static TriCam to_tricam(const CamRecord& c) { TriCam t; std::memcpy(&t, &c, sizeof t); return t; }

NewMapPointBatch::NewMapPointBatch(HipContext* ctx, const CamRecord& cam1, std::vector<KeyPoint> keys1, std::vector<Neighbour> nb, LevelTables lv, float ratioFactor)
    : cam1_(cam1), keys1_(std::move(keys1)), lv_(std::move(lv)), ratio_(ratioFactor) {
  nb_.resize(nb.size());
  for (size_t j = 0; j < nb.size(); j++) { nb_[j].cam = nb[j].cam; nb_[j].keys = std::move(nb[j].keys); nb_[j].pred = std::move(nb[j].predicted); }
  build(ctx);
}

NewMapPointBatch::NewMapPointBatch(HipContext& ctx, const TriangulationBatch& tb, const CamRecord& cam1, const std::vector<CamRecord>& cam2,
                                   const std::vector<Epipolar>& ep, LevelTables lv, float ratioFactor, const int32_t* octave1)
    : cam1_(cam1), keys1_(tb.keys1()), lv_(std::move(lv)), ratio_(ratioFactor) {
  if ((int)cam2.size() != tb.neighbours() || (int)ep.size() != tb.neighbours()) throw infrastructure_ex("NewMapPointBatch: one camera and one F12 per neighbour");
  if (octave1) for (size_t i = 0; i < keys1_.size(); i++) keys1_[i].octave = octave1[i];
  nb_.resize(cam2.size());
  std::vector<int32_t> m12;
  for (size_t j = 0; j < nb_.size(); j++) {
    nb_[j].cam = cam2[j];
    nb_[j].keys = tb.keys2((int)j);
    tb.resolve((int)j, nullptr, nullptr, ep[j].F12, ep[j].ex, ep[j].ey, lv_.sigma2_2.data(), lv_.sf_2.data(), m12);
    for (size_t i = 0; i < m12.size(); i++)   // vMatchedIndices: ascending idx1 (ORBmatcher.cpp:842-849)
      if (m12[i] >= 0) nb_[j].pred.emplace_back((int32_t)i, m12[i]);
  }
  build(&ctx);
}

void NewMapPointBatch::build(HipContext* ctx) {
  const size_t L = (size_t)lv_.nlevels;
  if (lv_.nlevels < 1 || lv_.sigma2_1.size() != L || lv_.sf_1.size() != L || lv_.sigma2_2.size() != L || lv_.sf_2.size() != L)
    throw infrastructure_ex("NewMapPointBatch: level tables");
  std::vector<int32_t> off(1, 0), oct;
  std::vector<float> xy, cam2;
  for (Nb& nb : nb_) {
    for (const auto& pr : nb.pred) {
      if (pr.first < 0 || pr.first >= (int)keys1_.size() || pr.second < 0 || pr.second >= (int)nb.keys.size()) throw infrastructure_ex("NewMapPointBatch: feature index out of range");
      const KeyPoint& k1 = keys1_[pr.first]; const KeyPoint& k2 = nb.keys[pr.second];
      if (k1.octave < 0 || k1.octave >= lv_.nlevels || k2.octave < 0 || k2.octave >= lv_.nlevels) throw infrastructure_ex("NewMapPointBatch: octave outside the level tables");
      xy.insert(xy.end(), {k1.x, k1.y, k2.x, k2.y});
      oct.push_back(k1.octave); oct.push_back(k2.octave);
    }
    off.push_back((int32_t)(oct.size() / 2));
    const float* c = reinterpret_cast<const float*>(&nb.cam);
    cam2.insert(cam2.end(), c, c + TRI_CAM_FLOATS);
    nb.order.resize(nb.pred.size());
    for (size_t i = 0; i < nb.order.size(); i++) nb.order[i] = (int32_t)i;
    std::sort(nb.order.begin(), nb.order.end(), [&](int32_t a, int32_t b) { return nb.pred[a] < nb.pred[b]; });
  }
  const size_t P = oct.size() / 2;
  n_pred_ = (int64_t)P;
  std::vector<uint8_t> status(std::max<size_t>(P, 1));
  std::vector<float> x3d(std::max<size_t>(3 * P, 1));
  if (P > 0 && ctx) {
    std::vector<int32_t> nacc(nb_.size());
    check(ccm_triangulate_pairs(ctx->get(), reinterpret_cast<const float*>(&cam1_), (int)nb_.size(), cam2.data(), off.data(), xy.data(), oct.data(), lv_.nlevels,
                                lv_.sigma2_1.data(), lv_.sf_1.data(), lv_.sigma2_2.data(), lv_.sf_2.data(), ratio_, status.data(), x3d.data(), nacc.data()),
          ctx->get(), "ccm_triangulate_pairs");
  } else if (P > 0) {
    const TriCam c1 = to_tricam(cam1_);
    for (size_t j = 0; j < nb_.size(); j++) {
      const TriCam c2 = to_tricam(nb_[j].cam);
      for (int i = off[j]; i < off[j + 1]; i++)
        status[i] = (uint8_t)tri_pair(c1, c2, xy[4 * i], xy[4 * i + 1], oct[2 * i], xy[4 * i + 2], xy[4 * i + 3], oct[2 * i + 1], lv_.sigma2_1.data(), lv_.sf_1.data(),
                                      lv_.sigma2_2.data(), lv_.sf_2.data(), ratio_, &x3d[3 * (size_t)i]);
    }
  }
  for (size_t j = 0; j < nb_.size(); j++) {
    nb_[j].status.assign(status.begin() + off[j], status.begin() + off[j + 1]);
    nb_[j].x3d.assign(x3d.begin() + 3 * (size_t)off[j], x3d.begin() + 3 * (size_t)off[j + 1]);
  }
}

int NewMapPointBatch::points(int j, const Pairs& pairs_now, std::vector<uint8_t>& status, std::vector<float>& x3d) {
  Nb& nb = nb_.at((size_t)j);
  status.assign(pairs_now.size(), 0);
  x3d.assign(3 * pairs_now.size(), 0.f);
  const TriCam c1 = to_tricam(cam1_), c2 = to_tricam(nb.cam);
  int n_ok = 0;
  for (size_t i = 0; i < pairs_now.size(); i++) {
    const auto& pr = pairs_now[i];
    auto it = std::lower_bound(nb.order.begin(), nb.order.end(), pr, [&](int32_t a, const std::pair<int32_t, int32_t>& v) { return nb.pred[a] < v; });
    if (it != nb.order.end() && nb.pred[*it] == pr) {
      status[i] = nb.status[*it];
      std::memcpy(&x3d[3 * i], &nb.x3d[3 * (size_t)*it], 3 * sizeof(float));
      n_hit_++;
    } else {
      if (pr.first < 0 || pr.first >= (int)keys1_.size() || pr.second < 0 || pr.second >= (int)nb.keys.size()) throw infrastructure_ex("NewMapPointBatch: feature index out of range");
      const KeyPoint& k1 = keys1_[pr.first]; const KeyPoint& k2 = nb.keys[pr.second];
      if (k1.octave < 0 || k1.octave >= lv_.nlevels || k2.octave < 0 || k2.octave >= lv_.nlevels) throw infrastructure_ex("NewMapPointBatch: octave outside the level tables");
      status[i] = (uint8_t)tri_pair(c1, c2, k1.x, k1.y, k1.octave, k2.x, k2.y, k2.octave, lv_.sigma2_1.data(), lv_.sf_1.data(), lv_.sigma2_2.data(), lv_.sf_2.data(),
                                    ratio_, &x3d[3 * i]);
      n_miss_++;
    }
    n_ok += status[i] == TRI_OK;
  }
  return n_ok;
}

// ---- Sim3MapCorrection ----------------------------------------------------------------------------------
// ccm_sim3_correct_map's arguments after the context through csrc/sim3_correct_math.h on the calling thread: same checks, same lines, same order of work
// (every keyframe first, then every point).  -1 where the device entry returns CCM_E_ARG.
int sim3_correct_map_host(int n_kf, const float* Tiw, int cur, const float* Twc, const double* Scw, double* S_non, double* S_cor, int n_obs_kf, const float* kf_center,
                          const int32_t* kf_rank, int n_pt, const float* pos, const int32_t* owner, const int32_t* owner_rank, const int32_t* obs_off,
                          const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, float* pos_out, float* normal,
                          float* min_dist, float* max_dist, float* Tiw_new, float* center_new) {
  if (n_kf < 1 || n_obs_kf < n_kf || n_pt < 0 || n_levels < 1 || !S_non || !S_cor || !kf_center || !kf_rank || !scale_factors || !Tiw_new || !center_new) return -1;
  if (Tiw && (!Twc || !Scw || cur < 0 || cur >= n_kf)) return -1;
  if (n_pt > 0) {
    if (!pos || !owner || !owner_rank || !obs_off || !ref_kf || !ref_level || !pos_out || !normal || !min_dist || !max_dist || obs_off[0] != 0) return -1;
    for (int i = 0; i < n_pt; i++)
      if (obs_off[i + 1] < obs_off[i] || owner[i] < 0 || owner[i] >= n_kf || ref_kf[i] < 0 || ref_kf[i] >= n_obs_kf || ref_level[i] < 0 || ref_level[i] >= n_levels) return -1;
    if (obs_off[n_pt] && !obs_kf) return -1;
    for (int k = 0; k < obs_off[n_pt]; k++) if (obs_kf[k] < 0 || obs_kf[k] >= n_obs_kf) return -1;
  }
  std::vector<Sim3d> swi((size_t)n_kf);
  const Sim3d scw = Tiw ? sim3_load(Scw) : Sim3d{0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < n_kf; i++) {
    Sim3d non = sim3_load(S_non + 8 * (size_t)i), cor = sim3_load(S_cor + 8 * (size_t)i);
    s3c_keyframe(Tiw ? Tiw + 12 * (size_t)i : nullptr, i == cur, Twc, scw, non, cor, swi[i], Tiw_new + 12 * (size_t)i, center_new + 3 * (size_t)i);
    if (Tiw) { sim3_store(S_non + 8 * (size_t)i, non); sim3_store(S_cor + 8 * (size_t)i, cor); }
  }
  for (int i = 0; i < n_pt; i++) {
    float p[3];
    s3c_point(sim3_load(S_non + 8 * (size_t)owner[i]), swi[owner[i]], pos + 3 * (size_t)i, p);
    s3c_normal_depth(p, obs_off[i], obs_off[i + 1], obs_kf, n_kf, kf_rank, owner_rank[i], kf_center, center_new, ref_kf[i], ref_level[i], scale_factors, n_levels,
                     normal + 3 * (size_t)i, min_dist[i], max_dist[i]);
    pos_out[3 * (size_t)i] = p[0]; pos_out[3 * (size_t)i + 1] = p[1]; pos_out[3 * (size_t)i + 2] = p[2];
  }
  return 0;
}

static void s3c_check_points(const Sim3MapCorrection::Points& p) {
  const size_t n = p.min_dist.size();
  if (p.pos.size() != 3 * n || p.normal.size() != 3 * n || p.max_dist.size() != n || p.ref_kf.size() != n || p.ref_level.size() != n || p.obs_off.size() != n + 1 ||
      p.obs_off[0] != 0 || (size_t)p.obs_off[n] != p.obs_kf.size())
    throw infrastructure_ex("Sim3MapCorrection: point arrays");
}

Sim3MapCorrection::Sim3MapCorrection(HipContext* ctx, int n_kf, std::vector<float> Tiw, std::vector<float> center, int cur, const float Twc[12], const double Scw[8],
                                     const std::vector<int32_t>& list_off, const std::vector<int32_t>& list_pt, const std::vector<uint8_t>& list_skip, Points pts,
                                     std::vector<float> scale_factors)
    : n_kf_(n_kf), pts_(std::move(pts)), sf_(std::move(scale_factors)) {
  s3c_check_points(pts_);
  if (n_kf < 1 || Tiw.size() != 12 * (size_t)n_kf || center.size() < 3 * (size_t)n_kf || center.size() % 3 || list_off.size() != (size_t)n_kf + 1 || list_off[0] != 0 ||
      (size_t)list_off[n_kf] != list_pt.size() || list_skip.size() != list_pt.size() || !Twc || !Scw)
    throw infrastructure_ex("Sim3MapCorrection: keyframe arrays");
  // the walk: a point belongs to the first keyframe that lists it through an entry that is not skipped (a second entry of the same keyframe finds it tagged)
  tag_.assign(pts_.min_dist.size(), -1);
  for (int i = 0; i < n_kf; i++) {
    if (list_off[i + 1] < list_off[i]) throw infrastructure_ex("Sim3MapCorrection: list_off decreases");
    for (int e = list_off[i]; e < list_off[i + 1]; e++) {
      const int32_t p = list_pt[e];
      if (p < 0 || list_skip[e]) continue;
      if ((size_t)p >= tag_.size()) throw infrastructure_ex("Sim3MapCorrection: point index out of range");
      if (tag_[p] < 0) tag_[p] = i;
    }
  }
  run(ctx, Tiw.data(), cur, Twc, Scw, center, -1);
}

Sim3MapCorrection::Sim3MapCorrection(HipContext* ctx, int n_kf, std::vector<float> center, std::vector<double> S_non, std::vector<double> S_cor,
                                     const std::vector<int32_t>& pt_kf, Points pts, std::vector<float> scale_factors)
    : n_kf_(n_kf), pts_(std::move(pts)), sf_(std::move(scale_factors)), S_non_(std::move(S_non)), S_cor_(std::move(S_cor)) {
  s3c_check_points(pts_);
  if (n_kf < 1 || center.size() < 3 * (size_t)n_kf || center.size() % 3 || S_non_.size() != 8 * (size_t)n_kf || S_cor_.size() != 8 * (size_t)n_kf ||
      pt_kf.size() != pts_.min_dist.size())
    throw infrastructure_ex("Sim3MapCorrection: keyframe arrays");
  tag_.assign(pt_kf.begin(), pt_kf.end());
  for (int32_t& t : tag_) { if (t >= n_kf) throw infrastructure_ex("Sim3MapCorrection: keyframe index out of range"); if (t < 0) t = -1; }
  run(ctx, nullptr, 0, nullptr, nullptr, center, INT32_MAX);
}

// epilogue_rank < 0: loop form, a point's rank is its owner's
void Sim3MapCorrection::run(HipContext* ctx, const float* Tiw, int cur, const float* Twc, const double* Scw, const std::vector<float>& center, int32_t epilogue_rank) {
  const int n_obs_kf = (int)(center.size() / 3);
  std::vector<int32_t> rank((size_t)n_obs_kf, INT32_MAX);
  for (int i = 0; i < n_kf_; i++) rank[i] = i;
  // the owned points, compacted in point order
  std::vector<int32_t> sel, owner, owner_rank, off(1, 0), okf, ref, lvl;
  std::vector<float> pos, nrm, dmin, dmax;
  for (size_t p = 0; p < tag_.size(); p++) {
    if (tag_[p] < 0) continue;
    sel.push_back((int32_t)p);
    owner.push_back(tag_[p]); owner_rank.push_back(epilogue_rank < 0 ? rank[tag_[p]] : epilogue_rank);
    if (pts_.obs_off[p + 1] < pts_.obs_off[p]) throw infrastructure_ex("Sim3MapCorrection: obs_off decreases");
    okf.insert(okf.end(), pts_.obs_kf.begin() + pts_.obs_off[p], pts_.obs_kf.begin() + pts_.obs_off[p + 1]);
    off.push_back((int32_t)okf.size());
    ref.push_back(pts_.ref_kf[p]); lvl.push_back(pts_.ref_level[p]);
    pos.insert(pos.end(), pts_.pos.begin() + 3 * p, pts_.pos.begin() + 3 * p + 3);
    nrm.insert(nrm.end(), pts_.normal.begin() + 3 * p, pts_.normal.begin() + 3 * p + 3);
    dmin.push_back(pts_.min_dist[p]); dmax.push_back(pts_.max_dist[p]);
  }
  const int n = (int)sel.size();
  S_non_.resize(8 * (size_t)n_kf_); S_cor_.resize(8 * (size_t)n_kf_);
  Tiw_new_.assign(12 * (size_t)n_kf_, 0.f); center_new_.assign(3 * (size_t)n_kf_, 0.f);
  if (ctx) {
    check(ccm_sim3_correct_map(ctx->get(), n_kf_, Tiw, cur, Twc, Scw, S_non_.data(), S_cor_.data(), n_obs_kf, center.data(), rank.data(), n, pos.data(), owner.data(),
                               owner_rank.data(), off.data(), okf.data(), ref.data(), lvl.data(), sf_.data(), (int)sf_.size(), pos.data(), nrm.data(), dmin.data(),
                               dmax.data(), Tiw_new_.data(), center_new_.data()),
          ctx->get(), "ccm_sim3_correct_map");
  } else if (sim3_correct_map_host(n_kf_, Tiw, cur, Twc, Scw, S_non_.data(), S_cor_.data(), n_obs_kf, center.data(), rank.data(), n, pos.data(), owner.data(),
                                   owner_rank.data(), off.data(), okf.data(), ref.data(), lvl.data(), sf_.data(), (int)sf_.size(), pos.data(), nrm.data(), dmin.data(),
                                   dmax.data(), Tiw_new_.data(), center_new_.data())) {
    throw infrastructure_ex("Sim3MapCorrection: bad arguments");
  }
  for (int i = 0; i < n; i++) {
    const size_t p = (size_t)sel[i];
    std::memcpy(&pts_.pos[3 * p], &pos[3 * (size_t)i], 12); std::memcpy(&pts_.normal[3 * p], &nrm[3 * (size_t)i], 12);
    pts_.min_dist[p] = dmin[i]; pts_.max_dist[p] = dmax[i];
  }
}

// ---- GbaMapUpdate ---------------------------------------------------------------------------------------
// ccm_gba_apply_map's host form after the context through csrc/gba_apply_math.h on the calling thread: same checks, same lines.  The keyframes are taken in walk
// order, which finishes every parent before its child.
int gba_apply_map_host(int n_kf, const int32_t* kf_parent, const int32_t* kf_cam, const float* Tcw_old, const float* Twc_old, int n_pt, const float* pos,
                       const int32_t* pt_vert, const int32_t* pt_ref, int n_cam, const double* cam_qt, int n_lm, const double* pt_xyz, float* T_new, float* Twc_new,
                       float* pos_out, uint8_t* pt_status) {
  if (n_kf < 1 || n_pt < 0 || !kf_parent || !kf_cam || !Tcw_old || !Twc_old || !T_new || !Twc_new || !cam_qt || n_cam < 1 || n_lm < 0 || (n_lm > 0 && !pt_xyz)) return -1;
  if (n_pt > 0 && (!pos || !pt_vert || !pt_ref || !pos_out || !pt_status)) return -1;
  std::vector<int32_t> depth((size_t)n_kf);
  int n_tree = 0, n_lvl = 0;
  if (gba_check_walk(n_kf, kf_parent, kf_cam, n_cam, depth.data(), &n_tree, &n_lvl) || gba_check_points(n_pt, pt_vert, pt_ref, n_lm, n_kf)) return -1;
  for (int k = 0; k < n_kf; k++) {
    float* T = T_new + 12 * (size_t)k;
    if (kf_cam[k] >= 0) gba_pose_of_se3(cam_qt + 7 * (size_t)kf_cam[k], T);
    else gba_child_pose(Tcw_old + 12 * (size_t)k, Twc_old + 12 * (size_t)kf_parent[k], T_new + 12 * (size_t)kf_parent[k], T);
    gba_twc(T, Twc_new + 12 * (size_t)k);
  }
  for (int i = 0; i < n_pt; i++) {
    const float P[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
    float out[3];
    pt_status[i] = gba_point(pt_vert[i], pt_ref[i], pt_xyz, Tcw_old, Twc_new, P, out);
    pos_out[3 * (size_t)i] = out[0]; pos_out[3 * (size_t)i + 1] = out[1]; pos_out[3 * (size_t)i + 2] = out[2];
  }
  return 0;
}

GbaMapUpdate::GbaMapUpdate(HipContext* ctx, Graph g, Points p, const std::vector<double>& cam_qt, const std::vector<double>& pt_xyz) : pts_(std::move(p)) {
  const size_t n = g.kf_cam.size(), np = pts_.vert.size();
  if (!n || g.origins.empty() || g.child_off.size() != n + 1 || g.child_off[0] != 0 || (size_t)g.child_off[n] != g.child_kf.size() || g.Tcw.size() != 12 * n ||
      g.Twc.size() != 12 * n || pts_.pos.size() != 3 * np || pts_.ref_kf.size() != np || cam_qt.empty() || cam_qt.size() % 7 || pt_xyz.size() % 3)
    throw infrastructure_ex("GbaMapUpdate: arrays");
  // the list walk: a keyframe's position is the order in which it is pushed, which is the order in which it is popped
  std::vector<int32_t> at(n, -1);
  auto push = [&](int32_t kf, int32_t parent) {
    if (kf < 0 || (size_t)kf >= n) throw infrastructure_ex("GbaMapUpdate: keyframe id out of range");
    if (at[kf] >= 0) { n_twice_++; return; }
    at[kf] = (int32_t)order_.size(); order_.push_back(kf); parent_.push_back(parent);
  };
  for (int32_t o : g.origins) push(o, -1);
  for (size_t head = 0; head < order_.size(); head++) {
    const int32_t kf = order_[head];
    if (g.child_off[kf + 1] < g.child_off[kf]) throw infrastructure_ex("GbaMapUpdate: child_off decreases");
    for (int32_t e = g.child_off[kf]; e < g.child_off[kf + 1]; e++) push(g.child_kf[e], (int32_t)head);
  }
  status_.assign(np, 0);
  if (n_twice_) return;
  const size_t K = order_.size();
  std::vector<int32_t> cam(K), ref(np);
  std::vector<float> Tcw(12 * K), Twc(12 * K);
  for (size_t k = 0; k < K; k++) {
    cam[k] = g.kf_cam[order_[k]];
    std::memcpy(&Tcw[12 * k], &g.Tcw[12 * (size_t)order_[k]], 48); std::memcpy(&Twc[12 * k], &g.Twc[12 * (size_t)order_[k]], 48);
  }
  for (size_t i = 0; i < np; i++) {
    const int32_t r = pts_.ref_kf[i];
    if (r >= 0 && (size_t)r >= n) throw infrastructure_ex("GbaMapUpdate: reference keyframe out of range");
    ref[i] = r < 0 ? -1 : at[r];   // reached: tagged, as a vertex or by the walk
    if (r >= 0 && at[r] < 0 && g.kf_cam[r] >= 0 && pts_.vert[i] < 0) n_stale_++;
  }
  T_new_.assign(12 * K, 0.f); Twc_new_.assign(12 * K, 0.f);
  const int n_cam = (int)(cam_qt.size() / 7), n_lm = (int)(pt_xyz.size() / 3);
  if (ctx) {
    check(ccm_gba_apply_map(ctx->get(), (int)K, parent_.data(), cam.data(), Tcw.data(), Twc.data(), (int)np, pts_.pos.data(), pts_.vert.data(), ref.data(), n_cam,
                            cam_qt.data(), n_lm, pt_xyz.data(), nullptr, T_new_.data(), Twc_new_.data(), pts_.pos.data(), status_.data()),
          ctx->get(), "ccm_gba_apply_map");
  } else if (gba_apply_map_host((int)K, parent_.data(), cam.data(), Tcw.data(), Twc.data(), (int)np, pts_.pos.data(), pts_.vert.data(), ref.data(), n_cam, cam_qt.data(),
                                n_lm, pt_xyz.data(), T_new_.data(), Twc_new_.data(), pts_.pos.data(), status_.data())) {
    throw infrastructure_ex("GbaMapUpdate: bad arguments");
  }
}

// ---- CovisibilityBatch ----------------------------------------------------------------------------------
// ccm_covis_update on the calling thread: the same checks and the rules of csrc/covis_math.h, one keyframe after the other
int covis_update_host(int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt,
                      const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col,
                      int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags, int32_t* needed) {
  if (!row_off || !fw_off || !ord_off || !flags || !needed || (cap > 0 && (!col || !count || !fw_col || !fw_w || !ord_kf || !ord_w))) return -1;
  if (covis_check_args(n_kf, n_all, order_key, list_off, list_pt, list_skip, n_pt, obs_off, obs_kf, th, cap)) return -1;
  const uint32_t uth = (uint32_t)th;
  // own counts: a dense counter over the keyframe indices and the list of those touched
  std::vector<uint32_t> cnt((size_t)n_all, 0);
  std::vector<int32_t> touched, roff((size_t)n_kf + 1, 0), rcol, rcnt, nge((size_t)n_kf, 0), fb((size_t)n_kf, -1), fl((size_t)n_kf, 0);
  for (int i = 0; i < n_kf; i++) {
    touched.clear();
    for (int32_t e = list_off[i]; e < list_off[i + 1]; e++) {
      if (!covis_entry_counts(list_pt[e], list_skip[e])) continue;
      for (int32_t o = obs_off[list_pt[e]]; o < obs_off[list_pt[e] + 1]; o++) {
        const int32_t j = obs_kf[o];
        if (!covis_observer_counts(j, i)) continue;
        if (cnt[j]++ == 0) touched.push_back(j);
      }
    }
    std::sort(touched.begin(), touched.end());
    uint32_t best_c = 0; int32_t best_key = 0, best_col = -1;
    for (int32_t j : touched) {
      const uint32_t c = cnt[j];
      rcol.push_back(j); rcnt.push_back((int32_t)c);
      if (c >= uth) nge[i]++;
      if (best_col < 0 || covis_fallback_better(c, order_key[j], best_c, best_key)) { best_c = c; best_key = order_key[j]; best_col = j; }
      cnt[j] = 0;
    }
    roff[i + 1] = (int32_t)rcol.size();
    fb[i] = nge[i] > 0 ? -1 : best_col;
    fl[i] = touched.empty() ? COVIS_EMPTY : nge[i] == 0 ? COVIS_FALLBACK : 0;
  }
  // the calls that reach a keyframe whose own row lacks the caller, and the rows whose list is rebuilt
  std::vector<std::vector<std::pair<int32_t, int32_t>>> extra((size_t)n_kf);
  for (int i = 0; i < n_kf; i++)
    for (int32_t e = roff[i]; e < roff[i + 1]; e++) {
      const int32_t t = rcol[e];
      if (t >= n_kf) continue;
      const uint32_t c = (uint32_t)rcnt[e];
      const int32_t pos = covis_find(rcol.data(), roff[t], roff[t + 1], i);
      if (pos < 0 && covis_is_event(c, t, uth, nge[i], fb[i]) && covis_reaches(i, t, roff[t + 1] == roff[t])) extra[t].push_back({i, (int32_t)c});
      if (pos >= 0 && covis_reaches(t, i, false) && (uint32_t)rcnt[pos] != c && covis_is_event((uint32_t)rcnt[pos], i, uth, nge[t], fb[t])) fl[i] |= COVIS_CHANGED;
    }
  std::vector<int32_t> foff((size_t)n_kf + 1, 0), fcol, fw, ooff((size_t)n_kf + 1, 0), okf, ow;
  std::vector<std::pair<uint64_t, int32_t>> keys;
  for (int i = 0; i < n_kf; i++) {
    if (!extra[i].empty()) fl[i] |= COVIS_CHANGED;
    const bool changed = (fl[i] & COVIS_CHANGED) != 0;
    // final weights: the row with the weights that reached it, merged with the extras (already ascending: their sources were walked in order)
    size_t x = 0;
    for (int32_t e = roff[i]; e <= roff[i + 1]; e++) {
      const int32_t c = e < roff[i + 1] ? rcol[e] : INT32_MAX;
      while (x < extra[i].size() && extra[i][x].first < c) { fcol.push_back(extra[i][x].first); fw.push_back(extra[i][x].second); x++; }
      if (e == roff[i + 1]) break;
      int32_t w = rcnt[e];
      if (c < n_kf && covis_reaches(c, i, false)) {
        const int32_t pos = covis_find(rcol.data(), roff[c], roff[c + 1], i);
        if (pos >= 0 && covis_is_event((uint32_t)rcnt[pos], i, uth, nge[c], fb[c])) w = rcnt[pos];
      }
      fcol.push_back(c); fw.push_back(w);
    }
    foff[i + 1] = (int32_t)fcol.size();
    keys.clear();
    for (int32_t e = foff[i]; e < foff[i + 1]; e++)
      if (changed || covis_is_event((uint32_t)fw[e], fcol[e], uth, nge[i], fb[i])) keys.push_back({covis_sort_key((uint32_t)fw[e], order_key[fcol[e]]), e});
    std::sort(keys.begin(), keys.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (const auto& k : keys) { okf.push_back(fcol[k.second]); ow.push_back(fw[k.second]); }
    ooff[i + 1] = (int32_t)okf.size();
  }
  needed[0] = (int32_t)rcol.size(); needed[1] = (int32_t)fcol.size(); needed[2] = (int32_t)okf.size();
  if (needed[0] > cap || needed[1] > cap || needed[2] > cap) return 0;
  auto out = [](int32_t* dst, const std::vector<int32_t>& v) { if (!v.empty()) std::memcpy(dst, v.data(), v.size() * 4); };
  out(flags, fl); out(row_off, roff); out(col, rcol); out(count, rcnt); out(fw_off, foff); out(fw_col, fcol); out(fw_w, fw); out(ord_off, ooff); out(ord_kf, okf); out(ord_w, ow);
  return 0;
}

CovisibilityBatch::CovisibilityBatch(HipContext* ctx, int n_kf, std::vector<int32_t> order_key, const std::vector<int32_t>& list_off, const std::vector<int32_t>& list_pt,
                                     const std::vector<uint8_t>& list_skip, const std::vector<int32_t>& obs_off, const std::vector<int32_t>& obs_kf, int th)
    : n_kf_(n_kf), key_(std::move(order_key)) {
  const int n_all = (int)key_.size();
  if (n_kf < 1 || n_all < n_kf || list_off.size() != (size_t)n_kf + 1 || list_off[0] != 0 || list_off[n_kf] < 0 || (size_t)list_off[n_kf] != list_pt.size() ||
      list_skip.size() != list_pt.size() || obs_off.empty() || obs_off[0] != 0 || obs_off.back() < 0 || (size_t)obs_off.back() != obs_kf.size())
    throw infrastructure_ex("CovisibilityBatch: arrays");
  const int n_pt = (int)obs_off.size() - 1;
  flags_.assign((size_t)n_kf, 0); row_off_.assign((size_t)n_kf + 1, 0); fw_off_ = row_off_; ord_off_ = row_off_;
  // capacity: a first guess from the set's size, then what the call says it needs
  int cap = std::max(4096, 96 * n_kf);
  for (int attempt = 0;; attempt++) {
    col_.assign((size_t)cap, 0); count_ = col_; fw_col_ = col_; fw_w_ = col_; ord_kf_ = col_; ord_w_ = col_;
    int32_t needed[3] = {0, 0, 0};
    if (ctx) {
      check(ccm_covis_update(ctx->get(), n_kf, n_all, key_.data(), list_off.data(), list_pt.data(), list_skip.data(), n_pt, obs_off.data(), obs_kf.data(), th, cap,
                             row_off_.data(), col_.data(), count_.data(), fw_off_.data(), fw_col_.data(), fw_w_.data(), ord_off_.data(), ord_kf_.data(), ord_w_.data(),
                             flags_.data(), needed),
            ctx->get(), "ccm_covis_update");
    } else if (covis_update_host(n_kf, n_all, key_.data(), list_off.data(), list_pt.data(), list_skip.data(), n_pt, obs_off.data(), obs_kf.data(), th, cap, row_off_.data(),
                                 col_.data(), count_.data(), fw_off_.data(), fw_col_.data(), fw_w_.data(), ord_off_.data(), ord_kf_.data(), ord_w_.data(), flags_.data(),
                                 needed)) {
      throw infrastructure_ex("CovisibilityBatch: bad arguments");
    }
    const int most = std::max(needed[0], std::max(needed[1], needed[2]));
    if (most <= cap) {
      col_.resize((size_t)needed[0]); count_.resize((size_t)needed[0]); fw_col_.resize((size_t)needed[1]); fw_w_.resize((size_t)needed[1]);
      ord_kf_.resize((size_t)needed[2]); ord_w_.resize((size_t)needed[2]);
      break;
    }
    if (attempt >= 3 || most > INT32_MAX / 2) throw infrastructure_ex("CovisibilityBatch: capacity");
    cap = 2 * most;   // the final rows are at most twice the count rows
  }
  // AddConnection calls on keyframes outside the set: walk order, then the map's key order.  The events of an unchanged row are its ordered list; a rebuilt
  // list holds the whole map, so there the row's own counts decide (a FALLBACK row's single event is then its best entry under covis_fallback_better)
  for (int i = 0; i < n_kf; i++) {
    const size_t first = outside_.size();
    if (!(flags_[i] & COVIS_CHANGED)) {
      for (int32_t e = ord_off_[i]; e < ord_off_[i + 1]; e++)
        if (ord_kf_[e] >= n_kf) outside_.push_back({ord_kf_[e], i, ord_w_[e]});
    } else if (flags_[i] & COVIS_FALLBACK) {
      int32_t best = -1;
      for (int32_t e = row_off_[i]; e < row_off_[i + 1]; e++)
        if (best < 0 || covis_fallback_better((uint32_t)count_[e], key_[col_[e]], (uint32_t)count_[best], key_[col_[best]])) best = e;
      if (best >= 0 && col_[best] >= n_kf) outside_.push_back({col_[best], i, count_[best]});
    } else {
      for (int32_t e = row_off_[i]; e < row_off_[i + 1]; e++)
        if (col_[e] >= n_kf && count_[e] >= th) outside_.push_back({col_[e], i, count_[e]});
    }
    std::sort(outside_.begin() + first, outside_.end(), [&](const AddCall& a, const AddCall& b) { return key_[a.target] < key_[b.target]; });
  }
}

std::map<int32_t, int> CovisibilityBatch::GetConnectedKeyFrameWeights(int i) const {
  std::map<int32_t, int> m;
  for (int32_t e = fw_off_[i]; e < fw_off_[i + 1]; e++) m[fw_col_[e]] = fw_w_[e];
  return m;
}
std::vector<int32_t> CovisibilityBatch::GetBestCovisibilityKeyFrames(int i, int N) const {
  const int n = ord_off_[i + 1] - ord_off_[i];
  return std::vector<int32_t>(ord_kf_.begin() + ord_off_[i], ord_kf_.begin() + ord_off_[i] + (n < N ? n : std::max(N, 0)));
}
std::vector<int32_t> CovisibilityBatch::GetCovisiblesByWeight(int i, int w) const {
  const auto b = ord_w_.begin() + ord_off_[i], e = ord_w_.begin() + ord_off_[i + 1];
  if (b == e) return {};
  const auto it = std::upper_bound(b, e, w, [](int a, int c) { return a > c; });
  if (it == e) return {};
  return std::vector<int32_t>(ord_kf_.begin() + ord_off_[i], ord_kf_.begin() + ord_off_[i] + (it - b));
}

// ---- KeyFrameCullingBatch -------------------------------------------------------------------------------
// ccm_kfcull_walk on the calling thread: the same checks and the rules of csrc/kfcull_math.h, one candidate after the other, every slot counted against the
// current state (no volatile / non-volatile split: that is the device's shortcut, and n_reeval reports when it would have had to count again)
int kfcull_walk_host(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                     const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad,
                     int th_obs, double thres, int n_levels, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone, int32_t* pt_nobs_out, int32_t* n_reeval) {
  if (!verdict || !n_mps || !n_red || !n_reeval || (n_pt > 0 && (!pt_gone || !pt_nobs_out))) return -1;
  if (kfcull_check_args(n_cand, n_all, cand_flags, list_off, list_pt, list_level, n_pt, pt_nobs, pt_bad, obs_off, obs_kf, obs_level, obs_bad, th_obs, thres, n_levels)) return -1;
  std::vector<int32_t> flags((size_t)n_cand), n(pt_nobs, pt_nobs + n_pt), gone((size_t)n_pt), stamp((size_t)n_pt, 0);
  for (int k = 0; k < n_cand; k++) flags[k] = cand_flags[k] & (KFCULL_SKIP | KFCULL_NOT_ERASE);
  for (int p = 0; p < n_pt; p++) gone[p] = pt_bad[p] != 0;
  std::vector<uint32_t> erased(((size_t)n_cand + 31) / 32, 0u);
  bool erased_before = false;
  *n_reeval = 0;
  for (int k = 0; k < n_cand; k++) {
    if (flags[k] & KFCULL_SKIP) { verdict[k] = KFCULL_SKIPPED; n_mps[k] = 0; n_red[k] = 0; continue; }
    int32_t m = 0, r = 0, n_vol = 0;
    for (int32_t e = list_off[k]; e < list_off[k + 1]; e++) {
      const int32_t p = list_pt[e];
      if (p < 0) continue;
      if (!pt_bad[p]) {
        bool vol = false;
        for (int32_t o = obs_off[p]; o < obs_off[p + 1] && !vol; o++) vol = kfcull_observer_is_volatile(obs_kf[o], k, flags.data());
        n_vol += vol;
      }
      if (!kfcull_slot_counts(p, gone[p])) continue;
      m++;
      if (kfcull_point_is_checked(n[p], th_obs))
        r += kfcull_count_observers(obs_kf, obs_level, obs_bad, obs_off[p], obs_off[p + 1], erased.data(), n_cand, k, list_level[e], th_obs) >= th_obs;
    }
    if (kfcull_reevaluated(erased_before, n_vol)) ++*n_reeval;
    n_mps[k] = m; n_red[k] = r;
    verdict[k] = (uint8_t)kfcull_verdict(kfcull_redundant(r, m, thres), flags[k]);
    if (verdict[k] != KFCULL_CULLED) continue;
    erased[k >> 5] |= 1u << (k & 31);
    erased_before = true;
    for (int32_t e = list_off[k]; e < list_off[k + 1]; e++) {
      const int32_t p = list_pt[e];
      if (p < 0 || gone[p] || stamp[p] == k + 1) continue;
      bool lists_back = false, live = false;
      for (int32_t o = obs_off[p]; o < obs_off[p + 1]; o++) {
        lists_back |= obs_kf[o] == k;
        live |= !obs_bad[o] && !kfcull_erased(erased.data(), n_cand, obs_kf[o]);
      }
      if (!lists_back) continue;
      stamp[p] = k + 1;
      if (kfcull_point_goes(--n[p], live)) gone[p] = 1;
    }
  }
  for (int p = 0; p < n_pt; p++) { pt_gone[p] = (uint8_t)gone[p]; pt_nobs_out[p] = n[p]; }
  return 0;
}

// The walk the way the reference's data structures make it: a std::map of observations per point that GetObservations() copies for every checked slot of every
// candidate (Mapping.cpp:829), keyframe bad flags behind a pointer, EraseObservation / SetBadFlag on the maps.  A MODEL of the reference's cost for
// scripts/kfcull_profile.py (no mutexes, no shared_ptr counts, no graph updates), not the reference; its verdicts equal the evaluator's.
int kfcull_walk_mapcopy_model(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                              const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level,
                              const uint8_t* obs_bad, int th_obs, double thres, int n_levels, uint8_t* verdict) {
  if (!verdict) return -1;
  if (kfcull_check_args(n_cand, n_all, cand_flags, list_off, list_pt, list_level, n_pt, pt_nobs, pt_bad, obs_off, obs_kf, obs_level, obs_bad, th_obs, thres, n_levels)) return -1;
  struct Kf { bool bad = false; };
  struct Pt { std::map<Kf*, size_t> obs; int n = 0; bool bad = false; };
  std::vector<Kf> kfs((size_t)n_all);
  std::vector<Pt> pts((size_t)n_pt);
  for (int p = 0; p < n_pt; p++) {
    pts[p].n = pt_nobs[p]; pts[p].bad = pt_bad[p] != 0;
    for (int32_t o = obs_off[p]; o < obs_off[p + 1]; o++) { pts[p].obs[&kfs[obs_kf[o]]] = obs_level[o]; if (obs_bad[o]) kfs[obs_kf[o]].bad = true; }
  }
  for (int k = 0; k < n_cand; k++) {
    if (cand_flags[k] & KFCULL_SKIP) { verdict[k] = KFCULL_SKIPPED; continue; }
    Kf* const me = &kfs[k];
    int n_red = 0, n_mps = 0;
    for (int32_t e = list_off[k]; e < list_off[k + 1]; e++) {
      if (list_pt[e] < 0) continue;
      Pt& pt = pts[list_pt[e]];
      if (pt.bad) continue;
      n_mps++;
      if (pt.n <= th_obs) continue;
      const std::map<Kf*, size_t> observations = pt.obs;      // the copy of GetObservations()
      int n = 0;
      for (const auto& ob : observations) {
        if (ob.first->bad || ob.first == me) continue;
        if ((int)ob.second <= (int)list_level[e] + 1 && ++n >= th_obs) break;
      }
      n_red += n >= th_obs;
    }
    verdict[k] = (uint8_t)kfcull_verdict(kfcull_redundant(n_red, n_mps, thres), cand_flags[k]);
    if (verdict[k] != KFCULL_CULLED) continue;
    for (int32_t e = list_off[k]; e < list_off[k + 1]; e++) {
      if (list_pt[e] < 0) continue;
      Pt& pt = pts[list_pt[e]];
      if (pt.bad || !pt.obs.erase(me)) continue;
      pt.n--;
      bool live = false;
      for (const auto& ob : pt.obs) live |= !ob.first->bad;
      if (kfcull_point_goes(pt.n, live)) { pt.bad = true; pt.obs.clear(); }
    }
    me->bad = true;
  }
  return 0;
}

KeyFrameCullingBatch::KeyFrameCullingBatch(HipContext* ctx, int n_all, const std::vector<uint8_t>& cand_flags, const std::vector<int32_t>& list_off,
                                           const std::vector<int32_t>& list_pt, const std::vector<uint8_t>& list_level, const std::vector<int32_t>& pt_nobs,
                                           const std::vector<uint8_t>& pt_bad, const std::vector<int32_t>& obs_off, const std::vector<int32_t>& obs_kf,
                                           const std::vector<uint8_t>& obs_level, const std::vector<uint8_t>& obs_bad, double thres, int n_levels, int th_obs)
    : bad_before_(pt_bad) {
  const int n_cand = (int)cand_flags.size(), n_pt = (int)pt_nobs.size();
  if (n_cand < 1 || list_off.size() != (size_t)n_cand + 1 || list_off[0] != 0 || list_off[n_cand] < 0 || (size_t)list_off[n_cand] != list_pt.size() ||
      list_level.size() != list_pt.size() || pt_bad.size() != (size_t)n_pt || obs_off.size() != (size_t)n_pt + 1 || obs_off[0] != 0 || obs_off.back() < 0 ||
      (size_t)obs_off.back() != obs_kf.size() || obs_level.size() != obs_kf.size() || obs_bad.size() != obs_kf.size())
    throw infrastructure_ex("KeyFrameCullingBatch: arrays");
  verdict_.assign((size_t)n_cand, 0); n_mps_.assign((size_t)n_cand, 0); n_red_.assign((size_t)n_cand, 0);
  gone_.assign((size_t)n_pt, 0); n_obs_.assign((size_t)n_pt, 0);
  if (ctx) {
    check(ccm_kfcull_walk(ctx->get(), n_cand, n_all, cand_flags.data(), list_off.data(), list_pt.data(), list_level.data(), n_pt, pt_nobs.data(), pt_bad.data(),
                          obs_off.data(), obs_kf.data(), obs_level.data(), obs_bad.data(), th_obs, thres, n_levels, verdict_.data(), n_mps_.data(), n_red_.data(),
                          gone_.data(), n_obs_.data(), &n_reeval_),
          ctx->get(), "ccm_kfcull_walk");
  } else if (kfcull_walk_host(n_cand, n_all, cand_flags.data(), list_off.data(), list_pt.data(), list_level.data(), n_pt, pt_nobs.data(), pt_bad.data(), obs_off.data(),
                              obs_kf.data(), obs_level.data(), obs_bad.data(), th_obs, thres, n_levels, verdict_.data(), n_mps_.data(), n_red_.data(), gone_.data(),
                              n_obs_.data(), &n_reeval_)) {
    throw infrastructure_ex("KeyFrameCullingBatch: bad arguments");
  }
}

std::vector<int32_t> KeyFrameCullingBatch::culled() const {
  std::vector<int32_t> v;
  for (size_t k = 0; k < verdict_.size(); k++)
    if (verdict_[k] == KFCULL_CULLED || verdict_[k] == KFCULL_REDUNDANT_NOT_ERASED) v.push_back((int32_t)k);
  return v;
}
std::vector<int32_t> KeyFrameCullingBatch::pointsGone() const {
  std::vector<int32_t> v;
  for (size_t p = 0; p < gone_.size(); p++)
    if (gone_[p] && !bad_before_[p]) v.push_back((int32_t)p);
  return v;
}

// ---- the six projected searches on the host: one pair, one walker, and the batches built on them ------------------------------
// one keyframe's own arrays, wherever they live: in the caller's flat arrays, or in a shadow of the keyframe store
struct FuseKf { const float* rec; const int32_t* cell_off; const uint16_t* cell_idx; const float* kxy; const uint8_t* koct; const uint8_t* kdesc; };
static FuseKf fuse_kf(const KfShadow& kf) { return {kf.rec, kf.cell_off.data(), kf.cell_idx.data(), kf.xy.data(), kf.oct.data(), kf.desc.data()}; }

// The two keyframe sources of a walk, k -> FuseKf.  The flat arrays of the device entries, whose int32 cell_idx is narrowed to 16 bits here (or is 16-bit already,
// as a FuseScene keeps it) ...
struct FlatKfs {
  const float* rec; const int32_t* feat_off; const float* xy; const uint8_t* oct; const uint8_t* desc; const int32_t* cell_off; const uint16_t* idx16;
  std::vector<uint16_t> narrowed;
  FlatKfs(int K, const float* kf_rec, const int32_t* feat_off_, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off_,
          const int32_t* cell_idx)
      : rec(kf_rec), feat_off(feat_off_), xy(feat_xy), oct(feat_octave), desc(feat_desc), cell_off(cell_off_), narrowed(K ? (size_t)feat_off_[K] : 0) {
    for (size_t f = 0; f < narrowed.size(); f++) narrowed[f] = (uint16_t)cell_idx[f];
    idx16 = narrowed.data();
  }
  FlatKfs(const float* kf_rec, const int32_t* feat_off_, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off_,
          const uint16_t* cell_idx16)
      : rec(kf_rec), feat_off(feat_off_), xy(feat_xy), oct(feat_octave), desc(feat_desc), cell_off(cell_off_), idx16(cell_idx16) {}
  FlatKfs(const FlatKfs&) = delete;
  FuseKf operator()(int k) const {
    const int32_t f0 = feat_off[k];
    return FuseKf{rec + FSM_REC_FLOATS * (size_t)k, cell_off + (size_t)k * (FSM_CELLS + 1), idx16 + f0, xy + 2 * (size_t)f0, oct + f0, desc + 32 * (size_t)f0};
  }
};
// ... and the shadows of a store's keys
typedef std::vector<std::shared_ptr<const KfShadow>> Shadows;
struct ShadowKfs {
  const Shadows& kfs;
  FuseKf operator()(int k) const { return fuse_kf(*kfs[k]); }
};

// a call's level tables and scalars (isig: the pose form's alone) and its points
struct ProjLevels { int nlevels; const float *sf, *isig; float logsf, th; };
typedef SearchAndFuseBatch::Points ProjPoints;

// One (keyframe, point) pair through csrc/fuse_math.h, with the template parameters of the device's fuse_pair (csrc/fuse.hip).  kChi2: the pose form of Fuse with its
// chi-square gate, which reads isig.  kMask: SearchByProjection(pKF, Scw, ...), which reads skip (one byte per feature of the keyframe).  kPair: SearchBySim3:
// pose_or_job is the job's SSM_JOB_FLOATS instead of the keyframe's 15, Pn is not read, TH_HIGH.  n_cand (nullable): the size of vIndices, 0 short of the window.
template <bool kChi2, bool kMask, bool kPair>
static uint32_t proj_pair_host(const FuseKf& kf, const float* pose_or_job, const uint8_t* skip, const ProjLevels& lv, const float* P3, const float* Pn, float dmin,
                               float dmax, const uint8_t* pdesc, float* uv, int32_t* n_cand) {
  float u, v; int level;
  const int st = kPair ? ssm_gate(kf.rec, pose_or_job, P3, dmin, dmax, lv.nlevels, lv.logsf, u, v, level)
                       : fsm_gate(kf.rec, pose_or_job, P3, Pn, dmin, dmax, lv.nlevels, lv.logsf, u, v, level);
  if (uv) { uv[0] = u; uv[1] = v; }
  if (n_cand) *n_cand = 0;
  if (st != FSM_EMPTY) return fsm_pack(st, 0, FSM_NO_DIST, FSM_NO_IDX);
  uint32_t q[8];
  fsm_load_desc(pdesc, q);
  return fsm_window_best<kChi2, kMask>(kf.rec, kf.cell_off, kf.cell_idx, kf.kxy, kf.koct, kf.kdesc, u, v, level, lv.th, lv.sf, lv.isig, q, n_cand, skip,
                                       kPair ? FSM_TH_HIGH : FSM_TH_LOW);
}

// Every pair of a list of jobs (keyframe job_kf[j] x points job_pt0[j] .. + job_n[j]), the jobs' words one after the other; the arguments are valid.  kf_of(k):
// keyframe k's arrays.  pose: 15 floats per keyframe, with kPair SSM_JOB_FLOATS per JOB.  kMask: keyframe k's mask starts at feat_skip + skip_off[k].
template <bool kChi2, bool kMask, bool kPair, class KfOf>
static void proj_jobs_host(const KfOf& kf_of, const float* pose, const int32_t* skip_off, const uint8_t* feat_skip, const ProjLevels& lv, const ProjPoints& pt, int J,
                           const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv,
                           int32_t* n_cand) {
  size_t e = 0;
  for (int j = 0; j < J; j++) {
    n_valid[j] = n_hit[j] = 0;
    const int k = job_kf[j];
    const FuseKf kf = kf_of(k);
    const float* pj = pose + (kPair ? SSM_JOB_FLOATS * (size_t)j : FSM_POSE_FLOATS * (size_t)k);
    const uint8_t* skip = kMask ? feat_skip + skip_off[k] : nullptr;
    for (int i = job_pt0[j]; i < job_pt0[j] + job_n[j]; i++, e++) {
      const uint32_t w = proj_pair_host<kChi2, kMask, kPair>(kf, pj, skip, lv, pt.pos + 3 * (size_t)i, kPair ? nullptr : pt.normal + 3 * (size_t)i, pt.min_dist[i],
                                                             pt.max_dist[i], pt.desc + 32 * (size_t)i, uv ? uv + 2 * e : nullptr, n_cand ? n_cand + e : nullptr);
      table[e] = w;
      n_valid[j] += (w >> 29) >= FSM_EMPTY;
      n_hit[j] += (w >> 29) == FSM_HIT;
    }
  }
}

// The keyframe-major forms (Fuse with a Sim3, SearchByProjection) are the jobs (k, 0, P): every keyframe against all points, with the pose its Scw decomposes into
template <bool kMask, class KfOf>
static void proj_kf_major_host(const KfOf& kf_of, int K, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, const ProjLevels& lv, const ProjPoints& pt,
                               uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv, int32_t* n_cand) {
  std::vector<float> pose(FSM_POSE_FLOATS * (size_t)K);
  std::vector<int32_t> jk((size_t)K), j0((size_t)K, 0), jn((size_t)K, pt.P);
  for (int k = 0; k < K; k++) { jk[k] = k; fsm_decompose_scw(Scw + 12 * (size_t)k, pose.data() + FSM_POSE_FLOATS * (size_t)k); }
  proj_jobs_host<false, kMask, false>(kf_of, pose.data(), skip_off, feat_skip, lv, pt, K, jk.data(), j0.data(), jn.data(), table, n_valid, n_hit, uv, n_cand);
}

// a packed answer as a Fuse call leaves bestIdx / bestDist (untouched where the pair has no candidate)
static inline void sin_answer(uint32_t w, int32_t& bestIdx, int32_t& bestDist, int& nFused) {
  const int st = (int)(w >> 29);
  if (st >= FSM_FAR) bestDist = (int32_t)((w >> 16) & 0x1FFu);
  if (st == FSM_HIT) { bestIdx = (int32_t)(w & 0xFFFFu); nFused++; }
}

template <class KFs, class Pts>
void FuseScene::copy(const KFs& kfs, const float* pose15, const Pts& pts, int nlevels_, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor,
                     float th_) {
  nlevels = nlevels_; logsf = logScaleFactor; th = th_;
  sf.assign(scale_factors, scale_factors + nlevels);
  if (inv_level_sigma2) isig.assign(inv_level_sigma2, inv_level_sigma2 + nlevels);
  const int K = kfs.K, P = pts.P;
  if (K > 0) {
    const size_t F = (size_t)kfs.feat_off[K];
    rec.assign(kfs.rec, kfs.rec + FSM_REC_FLOATS * (size_t)K);
    pose.assign(pose15, pose15 + FSM_POSE_FLOATS * (size_t)K);
    feat_off.assign(kfs.feat_off, kfs.feat_off + K + 1);
    cell_off.assign(kfs.cell_off, kfs.cell_off + (size_t)K * (FSM_CELLS + 1));
    cell_idx.resize(F);
    for (size_t f = 0; f < F; f++) cell_idx[f] = (uint16_t)kfs.cell_idx[f];
    if (F) { kxy.assign(kfs.feat_xy, kfs.feat_xy + 2 * F); koct.assign(kfs.feat_octave, kfs.feat_octave + F); kdesc.assign(kfs.feat_desc, kfs.feat_desc + 32 * F); }
  }
  if (P > 0) {
    pos.assign(pts.pos, pts.pos + 3 * (size_t)P); normal.assign(pts.normal, pts.normal + 3 * (size_t)P);
    dmin.assign(pts.min_dist, pts.min_dist + P); dmax.assign(pts.max_dist, pts.max_dist + P);
    pdesc.assign(pts.desc, pts.desc + 32 * (size_t)P);
  }
}

static ProjLevels scene_levels(const FuseScene& s) { return {s.nlevels, s.sf.data(), s.isig.data(), s.logsf, s.th}; }

uint32_t FuseScene::eval(int k, const float* P3, const float* Pn, float dmin_, float dmax_, const uint8_t* desc) const {
  const FuseKf kf = shadow.empty() ? FlatKfs(rec.data(), feat_off.data(), kxy.data(), koct.data(), kdesc.data(), cell_off.data(), cell_idx.data())(k) : fuse_kf(*shadow[k]);
  return (isig.empty() ? proj_pair_host<false, false, false> : proj_pair_host<true, false, false>)(kf, pose.data() + FSM_POSE_FLOATS * (size_t)k, nullptr, scene_levels(*this),
                                                                                                 P3, Pn, dmin_, dmax_, desc, nullptr, nullptr);
}

// One point of a Fuse call whose answer the table predicts: word w of keyframe k and the snapshot's point g, whose descriptor is desc (nullable) by now.  The gates
// read nothing a Fuse call changes; a pair that reached the window and whose descriptor has changed is evaluated again.
static void fuse_resolve_point(const FuseScene& s, uint32_t w, int k, size_t g, const uint8_t* desc, long long& n_reeval, int32_t& bestIdx, int32_t& bestDist, int& nFused) {
  if ((w >> 29) < FSM_EMPTY) return;
  if (desc && std::memcmp(desc, s.pdesc.data() + 32 * g, 32) != 0) {
    w = s.eval(k, s.pos.data() + 3 * g, s.normal.data() + 3 * g, s.dmin[g], s.dmax[g], desc);
    n_reeval++;
  }
  sin_answer(w, bestIdx, bestDist, nFused);
}

// ---- the host evaluators: the device entry's checks (csrc/fuse_math.h), a keyframe source, one walk; -1 where the entry returns CCM_E_ARG --------------------
int fuse_sim3_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                        const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P,
                        const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid,
                        int32_t* n_hit, float* uv, int32_t* n_cand) {
  if (fsm_check_args(K, P, feat_off, cell_off, cell_idx, nlevels, th)) return -1;
  if (fsm_check_kf_pointers(K, P, kf_rec, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit,
                            fsm_feats_ok(K ? (size_t)feat_off[K] : 0, feat_xy, feat_octave, feat_desc)))
    return -1;
  proj_kf_major_host<false>(FlatKfs(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx), K, Scw, nullptr, nullptr,
                            {nlevels, scale_factors, nullptr, logScaleFactor, th}, {P, pos, normal, min_dist, max_dist, pt_desc}, table, n_valid, n_hit, uv, n_cand);
  return 0;
}

int fuse_pose_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                        const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
                        float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc,
                        int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv,
                        int32_t* n_cand) {
  if (fsm_check_args(K, P, feat_off, cell_off, cell_idx, nlevels, th)) return -1;
  int64_t total = 0, tiles = 0;
  if (fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles)) return -1;
  if (fsm_check_job_pointers(K, P, J, total, true, kf_rec, pose, scale_factors, inv_level_sigma2, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit,
                             fsm_feats_ok(K ? (size_t)feat_off[K] : 0, feat_xy, feat_octave, feat_desc)))
    return -1;
  proj_jobs_host<true, false, false>(FlatKfs(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx), pose, nullptr, nullptr,
                                     {nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th}, {P, pos, normal, min_dist, max_dist, pt_desc}, J, job_kf, job_pt0,
                                     job_n, table, n_valid, n_hit, uv, n_cand);
  return 0;
}

int sim3_project_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                           const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels,
                           const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                           const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (fsm_check_args(K, P, feat_off, cell_off, cell_idx, nlevels, th)) return -1;
  if (fsm_check_kf_pointers(K, P, kf_rec, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit,
                            fsm_feats_ok(K ? (size_t)feat_off[K] : 0, feat_xy, feat_octave, feat_desc)))
    return -1;
  std::vector<int32_t> kf_n((size_t)K);
  for (int k = 0; k < K; k++) kf_n[k] = feat_off[k + 1] - feat_off[k];
  if (fsm_check_skip(K, skip_off, feat_skip, kf_n.data())) return -1;
  proj_kf_major_host<true>(FlatKfs(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx), K, Scw, skip_off, feat_skip,
                           {nlevels, scale_factors, nullptr, logScaleFactor, th}, {P, pos, normal, min_dist, max_dist, pt_desc}, table, n_valid, n_hit, uv, nullptr);
  return 0;
}

// the pair form's walk on either source, from its validated arguments
template <class KfOf>
static void sim3_pair_walk(const KfOf& kf_of, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* min_dist,
                           const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4, const float* job_src_pose, const float* job_T,
                           const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  std::vector<float> jobs(SSM_JOB_FLOATS * (size_t)J);
  ssm_pack_jobs(J, job_K4, job_src_pose, job_T, jobs.data());
  proj_jobs_host<false, false, true>(kf_of, jobs.data(), nullptr, nullptr, {nlevels, scale_factors, nullptr, logScaleFactor, th},
                                     {P, pos, nullptr, min_dist, max_dist, pt_desc}, J, job_kf, job_pt0, job_n, table, n_valid, n_hit, uv, nullptr);
}

int sim3_pair_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                        const int32_t* cell_off, const int32_t* cell_idx, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos,
                        const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4, const float* job_src_pose,
                        const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (fsm_check_args(K, P, feat_off, cell_off, cell_idx, nlevels, th)) return -1;
  int64_t total = 0, tiles = 0;
  if (fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles) || fsm_check_pair_jobs(J, job_K4, job_src_pose, job_T)) return -1;
  if (fsm_check_job_pointers(K, P, J, total, false, kf_rec, nullptr, scale_factors, nullptr, pos, nullptr, min_dist, max_dist, pt_desc, table, n_valid, n_hit,
                             fsm_feats_ok(K ? (size_t)feat_off[K] : 0, feat_xy, feat_octave, feat_desc)))
    return -1;
  sim3_pair_walk(FlatKfs(K, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx), nlevels, scale_factors, logScaleFactor, th, P, pos, min_dist, max_dist,
                 pt_desc, J, job_kf, job_K4, job_src_pose, job_T, job_pt0, job_n, table, n_valid, n_hit, uv);
  return 0;
}

// ---- KeyFrameStore and the batches built on it ----------------------------------------------------------
KeyFrameStore::KeyFrameStore(HipContext* ctx, int max_kf, int max_feat) : max_kf_(max_kf), max_feat_(max_feat) {
  if (max_kf < 1 || !kfg_stride(max_feat) || (int64_t)max_kf * kfg_stride(max_feat) > (int64_t)INT32_MAX) throw infrastructure_ex("KeyFrameStore: bad capacity");
  if (ctx) check(ccm_kfstore_create(ctx->get(), max_kf, max_feat, &h_), ctx->get(), "ccm_kfstore_create");
}

KeyFrameStore::~KeyFrameStore() { ccm_kfstore_destroy(h_); }

// the host-only store's key rules: no key twice within the call, none live, a free slot for each
bool KeyFrameStore::keys_ok(int M, const int64_t* keys) const {
  std::vector<int64_t> sorted(keys, keys + (M > 0 ? M : 0));
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return false;
  for (int m = 0; m < M; m++)
    if (live_.count(keys[m])) return false;
  return (size_t)(M > 0 ? M : 0) <= (size_t)max_kf_ - live_.size();
}

int KeyFrameStore::add(HipContext* ctx, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
                       const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx) {
  if (h_ && !ctx) throw infrastructure_ex("KeyFrameStore::add: a device store needs the calling thread's context");
  std::unique_lock<std::shared_mutex> lk(mu_);
  if (h_) {   // the device store decides, by the same rules in the same order, and the shadows follow it
    const int rc = ccm_kfstore_add(h_, ctx->get(), M, keys, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx);
    if (rc == CCM_E_ARG || rc == CCM_E_STATE) return rc;
    check(rc, ctx->get(), "ccm_kfstore_add");
  } else {
    if ((M > 0 && !keys) || kfg_check_add(M, max_feat_, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx)) return CCM_E_ARG;
    if (!keys_ok(M, keys)) return CCM_E_STATE;
  }
  for (int m = 0; m < M; m++) {
    auto kf = std::make_shared<KfShadow>();
    const int32_t f0 = feat_off[m], n = feat_off[m + 1] - f0;
    std::memcpy(kf->rec, kf_rec + FSM_REC_FLOATS * (size_t)m, sizeof kf->rec);
    kf->n = n;
    if (n) {
      kf->xy.assign(feat_xy + 2 * (size_t)f0, feat_xy + 2 * (size_t)(f0 + n));
      kf->oct.assign(feat_octave + f0, feat_octave + f0 + n);
      kf->desc.assign(feat_desc + 32 * (size_t)f0, feat_desc + 32 * (size_t)(f0 + n));
    }
    kf->cell_off.resize(FSM_CELLS + 1);
    if (cell_off) {
      const int32_t* co = cell_off + (size_t)m * (FSM_CELLS + 1);
      kf->cell_off.assign(co, co + FSM_CELLS + 1);
      kf->n_in = co[FSM_CELLS];
      kf->cell_idx.resize((size_t)kf->n_in);
      for (int32_t j = 0; j < kf->n_in; j++) kf->cell_idx[j] = (uint16_t)cell_idx[f0 + j];
    } else {
      kf->cell_idx.resize((size_t)n);
      kf->n_in = kfg_build_host(kf->rec, n, kf->xy.data(), kf->cell_off.data(), kf->cell_idx.data());
      kf->cell_idx.resize((size_t)kf->n_in);
    }
    live_[keys[m]] = std::move(kf);
  }
  return CCM_OK;
}

int KeyFrameStore::set_featvec(HipContext* ctx, int64_t key, const FeatureVectorView& fv, const float* angle) {
  if (h_ && !ctx) throw infrastructure_ex("KeyFrameStore::set_featvec: a device store needs the calling thread's context");
  std::unique_lock<std::shared_mutex> lk(mu_);
  auto it = live_.find(key);
  if (it == live_.end()) return CCM_E_ARG;
  const int n = it->second->n;
  if (h_) {   // the device store decides, by the same rules
    const int rc = ccm_kfstore_set_featvec(h_, ctx->get(), key, fv.nn, fv.node, fv.off, fv.idx);
    if (rc == CCM_E_ARG) return rc;
    check(rc, ctx->get(), "ccm_kfstore_set_featvec");
  } else {
    std::vector<uint8_t> seen((size_t)n + 1);
    if (bsm_check_featvec(n, fv.nn, fv.node, fv.off, fv.idx, seen.data())) return CCM_E_ARG;
  }
  // batches hold the shadow they were built on: the key gets a copy with the vector
  auto kf = std::make_shared<KfShadow>(*it->second);
  kf->has_fv = true;
  kf->fv_node.assign(fv.node, fv.node + (fv.nn > 0 ? fv.nn : 0));
  kf->fv_off.assign(1, 0);
  kf->fv_idx.clear();
  if (fv.nn > 0) {
    kf->fv_off.assign(fv.off, fv.off + fv.nn + 1);
    kf->fv_idx.resize((size_t)fv.off[fv.nn]);
    for (size_t i = 0; i < kf->fv_idx.size(); i++) kf->fv_idx[i] = (uint16_t)fv.idx[i];
  }
  if (angle) kf->angle.assign(angle, angle + n); else kf->angle.assign((size_t)n, 0.0f);
  it->second = std::move(kf);
  return CCM_OK;
}

int KeyFrameStore::ingest_flat(HipContext* ctx, const ccm_vocab* dvoc, const ::kfi_tree* tree, int levelsup, int M, const int64_t* keys, const float* kf_rec,
                               const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, int32_t* bow_n,
                               int32_t* bow_word, double* bow_value, int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word,
                               int32_t* feat_node) {
  if (h_ && !ctx) throw infrastructure_ex("KeyFrameStore::ingest: a device store needs the calling thread's context");
  std::unique_lock<std::shared_mutex> lk(mu_);
  if (h_) {   // the device store decides, by the same rules in the same order, and the shadows follow it
    const int rc = ccm_kfstore_ingest(h_, ctx->get(), dvoc, levelsup, M, keys, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, bow_n, bow_word, bow_value, fv_nn, fv_node,
                                      fv_off, fv_idx, feat_word, feat_node);
    if (rc == CCM_E_ARG || rc == CCM_E_STATE) return rc;
    check(rc, ctx->get(), "ccm_kfstore_ingest");
  } else {
    if (!tree || (M > 0 && !keys) ||
        kfi_check_ingest(M, max_feat_, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx) ||
        (feat_word == nullptr) != (feat_node == nullptr))
      return CCM_E_ARG;
    if (!keys_ok(M, keys)) return CCM_E_STATE;
    kfi_ingest_host(*tree, levelsup, M, feat_off, feat_desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx, feat_word, feat_node);
  }
  for (int m = 0; m < M; m++) {   // the shadow of add without a grid, then of set_featvec
    auto kf = std::make_shared<KfShadow>();
    const int32_t f0 = feat_off[m], n = feat_off[m + 1] - f0;
    std::memcpy(kf->rec, kf_rec + FSM_REC_FLOATS * (size_t)m, sizeof kf->rec);
    kf->n = n;
    if (n) {
      kf->xy.assign(feat_xy + 2 * (size_t)f0, feat_xy + 2 * (size_t)(f0 + n));
      kf->oct.assign(feat_octave + f0, feat_octave + f0 + n);
      kf->desc.assign(feat_desc + 32 * (size_t)f0, feat_desc + 32 * (size_t)(f0 + n));
    }
    kf->cell_off.resize(FSM_CELLS + 1);
    kf->cell_idx.resize((size_t)n);
    kf->n_in = kfg_build_host(kf->rec, n, kf->xy.data(), kf->cell_off.data(), kf->cell_idx.data());
    kf->cell_idx.resize((size_t)kf->n_in);
    const int nn = fv_nn[m];
    const int32_t* off = fv_off + f0 + m;
    kf->has_fv = true;
    kf->fv_node.assign(fv_node + f0, fv_node + f0 + nn);
    kf->fv_off.assign(1, 0);
    if (nn > 0) {
      kf->fv_off.assign(off, off + nn + 1);
      kf->fv_idx.resize((size_t)off[nn]);
      for (size_t i = 0; i < kf->fv_idx.size(); i++) kf->fv_idx[i] = (uint16_t)fv_idx[f0 + i];
    }
    if (angle) kf->angle.assign(angle + f0, angle + f0 + n); else kf->angle.assign((size_t)n, 0.0f);
    live_[keys[m]] = std::move(kf);
  }
  return CCM_OK;
}

int KeyFrameStore::ingest(HipContext* ctx, const ORBVocabulary& voc, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
                          const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, std::vector<BowVector>& bow, std::vector<FeatureVector>& fv,
                          int levelsup) {
  if (M < 0 || (M > 0 && !feat_off)) return CCM_E_ARG;
  const size_t F = M > 0 && feat_off[M] > 0 ? (size_t)feat_off[M] : 0, Mu = (size_t)M;
  std::vector<int32_t> bow_n(Mu + 1), bow_word(F + 1), fv_nn(Mu + 1), fv_node(F + 1), fv_off(F + Mu + 1), fv_idx(F + 1);
  std::vector<double> bow_value(F + 1);
  const ::kfi_tree tree = {voc.n_nodes(), voc.L(), voc.child_off().data(), voc.child_id().data(), voc.node_desc().data(), voc.word_id().data(), voc.weight().data()};
  const int rc = ingest_flat(ctx, voc.handle(), &tree, levelsup, M, keys, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, angle, bow_n.data(), bow_word.data(),
                             bow_value.data(), fv_nn.data(), fv_node.data(), fv_off.data(), fv_idx.data(), nullptr, nullptr);
  if (rc != CCM_OK) return rc;
  bow.assign(Mu, BowVector()); fv.assign(Mu, FeatureVector());
  for (int m = 0; m < M; m++) {
    const int32_t f0 = feat_off[m];
    bow[m].word.assign(bow_word.begin() + f0, bow_word.begin() + f0 + bow_n[m]);
    bow[m].value.assign(bow_value.begin() + f0, bow_value.begin() + f0 + bow_n[m]);
    fv[m].node.assign(fv_node.begin() + f0, fv_node.begin() + f0 + fv_nn[m]);
    fv[m].off.assign(fv_off.begin() + f0 + m, fv_off.begin() + f0 + m + fv_nn[m] + 1);
    fv[m].idx.assign(fv_idx.begin() + f0, fv_idx.begin() + f0 + fv[m].off.back());
  }
  return CCM_OK;
}

void KeyFrameStore::erase(HipContext* ctx, int64_t key) {
  if (h_ && !ctx) throw infrastructure_ex("KeyFrameStore::erase: a device store needs the calling thread's context");
  std::unique_lock<std::shared_mutex> lk(mu_);
  if (h_) check(ccm_kfstore_erase(h_, ctx->get(), key), ctx->get(), "ccm_kfstore_erase");
  live_.erase(key);
}

void KeyFrameStore::clear(HipContext* ctx) {
  if (h_ && !ctx) throw infrastructure_ex("KeyFrameStore::clear: a device store needs the calling thread's context");
  std::unique_lock<std::shared_mutex> lk(mu_);
  if (h_) check(ccm_kfstore_clear(h_, ctx->get()), ctx->get(), "ccm_kfstore_clear");
  live_.clear();
}

int KeyFrameStore::live() const { std::shared_lock<std::shared_mutex> lk(mu_); return (int)live_.size(); }
int KeyFrameStore::free_slots() const { std::shared_lock<std::shared_mutex> lk(mu_); return max_kf_ - (int)live_.size(); }

std::shared_ptr<const KfShadow> KeyFrameStore::shadow(int64_t key) const {
  std::shared_lock<std::shared_mutex> lk(mu_);
  auto it = live_.find(key);
  return it == live_.end() ? nullptr : it->second;
}

bool KeyFrameStore::get(HipContext* ctx, int64_t key, int* n, int* n_in, int32_t* cell_off, int32_t* cell_idx) const {
  const std::shared_ptr<const KfShadow> kf = shadow(key);
  if (!kf) return false;
  if (h_ && ctx) {
    check(ccm_kfstore_get(h_, ctx->get(), key, n, n_in, cell_off, cell_idx), ctx->get(), "ccm_kfstore_get");
    return true;
  }
  if (n) *n = kf->n;
  if (n_in) *n_in = kf->n_in;
  if (cell_off) std::memcpy(cell_off, kf->cell_off.data(), (FSM_CELLS + 1) * sizeof(int32_t));
  if (cell_idx)
    for (int j = 0; j < kf->n_in; j++) cell_idx[j] = kf->cell_idx[j];
  return true;
}

template <class Pts>
void FuseScene::hold(std::vector<std::shared_ptr<const KfShadow>> kfs, const float* pose15, const Pts& pts, int nlevels_, const float* scale_factors,
                     const float* inv_level_sigma2, float logScaleFactor, float th_) {
  const SearchAndFuseBatch::KeyFrames none;   // K = 0
  copy(none, nullptr, pts, nlevels_, scale_factors, inv_level_sigma2, logScaleFactor, th_);   // the points and the call's values
  if (!kfs.empty()) pose.assign(pose15, pose15 + FSM_POSE_FLOATS * kfs.size());
  shadow = std::move(kfs);
}

// the shadows of keys[0 .. K); false when one is not live
static bool store_shadows(const KeyFrameStore& store, int K, const int64_t* keys, Shadows& out) {
  out.resize((size_t)(K > 0 ? K : 0));
  for (int k = 0; k < K; k++)
    if (!(out[k] = store.shadow(keys[k]))) return false;
  return true;
}


int fuse_sim3_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor,
                                 float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc,
                                 uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (fsm_check_scalars(K, P, nlevels, th)) return -1;
  if (fsm_check_kf_pointers(K, P, keys, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, true)) return -1;
  Shadows kfs;
  if (!store_shadows(store, K, keys, kfs)) return -1;
  proj_kf_major_host<false>(ShadowKfs{kfs}, K, Scw, nullptr, nullptr, {nlevels, scale_factors, nullptr, logScaleFactor, th}, {P, pos, normal, min_dist, max_dist, pt_desc},
                            table, n_valid, n_hit, uv, nullptr);
  return 0;
}

int fuse_pose_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors,
                                 const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                 const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n,
                                 uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (fsm_check_scalars(K, P, nlevels, th)) return -1;
  int64_t total = 0, tiles = 0;
  if (fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles)) return -1;
  if (fsm_check_job_pointers(K, P, J, total, true, keys, pose, scale_factors, inv_level_sigma2, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, true))
    return -1;
  Shadows kfs;
  if (!store_shadows(store, K, keys, kfs)) return -1;
  proj_jobs_host<true, false, false>(ShadowKfs{kfs}, pose, nullptr, nullptr, {nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th},
                                     {P, pos, normal, min_dist, max_dist, pt_desc}, J, job_kf, job_pt0, job_n, table, n_valid, n_hit, uv, nullptr);
  return 0;
}

int sim3_project_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels,
                                    const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                    const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (fsm_check_scalars(K, P, nlevels, th)) return -1;
  if (fsm_check_kf_pointers(K, P, keys, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, true)) return -1;
  Shadows kfs;
  if (!store_shadows(store, K, keys, kfs)) return -1;
  std::vector<int32_t> kf_n((size_t)K);
  for (int k = 0; k < K; k++) kf_n[k] = kfs[k]->n;
  if (fsm_check_skip(K, skip_off, feat_skip, kf_n.data())) return -1;
  proj_kf_major_host<true>(ShadowKfs{kfs}, K, Scw, skip_off, feat_skip, {nlevels, scale_factors, nullptr, logScaleFactor, th}, {P, pos, normal, min_dist, max_dist, pt_desc},
                           table, n_valid, n_hit, uv, nullptr);
  return 0;
}

int sim3_pair_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P,
                                 const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4,
                                 const float* job_src_pose, const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid,
                                 int32_t* n_hit, float* uv) {
  if (fsm_check_scalars(K, P, nlevels, th)) return -1;
  int64_t total = 0, tiles = 0;
  if (fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles) || fsm_check_pair_jobs(J, job_K4, job_src_pose, job_T)) return -1;
  if (fsm_check_job_pointers(K, P, J, total, false, keys, nullptr, scale_factors, nullptr, pos, nullptr, min_dist, max_dist, pt_desc, table, n_valid, n_hit, true)) return -1;
  Shadows kfs;
  if (!store_shadows(store, K, keys, kfs)) return -1;
  sim3_pair_walk(ShadowKfs{kfs}, nlevels, scale_factors, logScaleFactor, th, P, pos, min_dist, max_dist, pt_desc, J, job_kf, job_K4, job_src_pose, job_T, job_pt0, job_n,
                 table, n_valid, n_hit, uv);
  return 0;
}

// ---- SearchAndFuseBatch, SearchInNeighborsBatch: the keyframes are the caller's flat arrays (flat) or live keys of a store -----------------------
SearchAndFuseBatch::SearchAndFuseBatch(HipContext* ctx, const KeyFrames& kfs, const Points& pts, int nlevels, const float* scale_factors, float logScaleFactor, float th)
    : K_(kfs.K), P_(pts.P) {
  init(&kfs, nullptr, nullptr, kfs.Scw, ctx, pts, nlevels, scale_factors, logScaleFactor, th);
}
SearchAndFuseBatch::SearchAndFuseBatch(KeyFrameStore& store, HipContext* ctx, int K, const int64_t* keys, const float* Scw, const Points& pts, int nlevels,
                                       const float* scale_factors, float logScaleFactor, float th)
    : K_(K), P_(pts.P) {
  init(nullptr, &store, keys, Scw, ctx, pts, nlevels, scale_factors, logScaleFactor, th);
}

void SearchAndFuseBatch::init(const KeyFrames* flat, KeyFrameStore* store, const int64_t* keys, const float* Scw, HipContext* ctx, const Points& pts, int nlevels,
                              const float* scale_factors, float logScaleFactor, float th) {
  const int K = K_, P = P_;
  if (K < 0 || P < 0 || !scale_factors || nlevels < 1 || nlevels > FSM_MAX_LEVELS || (store && K > 0 && (!keys || !Scw)))
    throw infrastructure_ex("SearchAndFuseBatch: bad arguments");
  // the shadows first: what is held here stays valid whatever the store does from now on
  Shadows shadows;
  if (store && !store->host_only() && !ctx) throw infrastructure_ex("SearchAndFuseBatch: a device store needs the calling thread's context");
  if (store && !store_shadows(*store, K, keys, shadows)) throw infrastructure_ex("SearchAndFuseBatch: a key is not in the store");
  table_.assign((size_t)K * (size_t)P, 0); n_valid_.assign((size_t)K, 0); n_hit_.assign((size_t)K, 0);
  if (store && !store->host_only()) {
    check(ccm_fuse_sim3_eval_resident(ctx->get(), store->handle(), K, keys, Scw, nlevels, scale_factors, logScaleFactor, th, P, pts.pos, pts.normal, pts.min_dist,
                                      pts.max_dist, pts.desc, table_.data(), n_valid_.data(), n_hit_.data(), nullptr),
          ctx->get(), "ccm_fuse_sim3_eval_resident");
  } else if (store) {
    if (fsm_check_scalars(K, P, nlevels, th) || (P > 0 && (!pts.pos || !pts.normal || !pts.min_dist || !pts.max_dist || !pts.desc)))
      throw infrastructure_ex("SearchAndFuseBatch: bad arguments");
    proj_kf_major_host<false>(ShadowKfs{shadows}, K, Scw, nullptr, nullptr, {nlevels, scale_factors, nullptr, logScaleFactor, th}, pts, table_.data(), n_valid_.data(),
                              n_hit_.data(), nullptr, nullptr);
  } else if (ctx) {
    check(ccm_fuse_sim3_eval(ctx->get(), K, flat->rec, flat->feat_off, flat->feat_xy, flat->feat_octave, flat->feat_desc, flat->cell_off, flat->cell_idx, Scw, nlevels,
                             scale_factors, logScaleFactor, th, P, pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc, table_.data(), n_valid_.data(),
                             n_hit_.data(), nullptr),
          ctx->get(), "ccm_fuse_sim3_eval");
  } else if (fuse_sim3_eval_host(K, flat->rec, flat->feat_off, flat->feat_xy, flat->feat_octave, flat->feat_desc, flat->cell_off, flat->cell_idx, Scw, nlevels, scale_factors,
                                 logScaleFactor, th, P, pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc, table_.data(), n_valid_.data(), n_hit_.data(), nullptr,
                                 nullptr)) {
    throw infrastructure_ex("SearchAndFuseBatch: bad arguments");
  }
  // the arguments are valid from here on: what resolve may have to evaluate again
  std::vector<float> pose(FSM_POSE_FLOATS * (size_t)K);
  for (int k = 0; k < K; k++) fsm_decompose_scw(Scw + 12 * (size_t)k, pose.data() + FSM_POSE_FLOATS * (size_t)k);
  if (store) scene_.hold(std::move(shadows), pose.data(), pts, nlevels, scale_factors, nullptr, logScaleFactor, th);
  else scene_.copy(*flat, pose.data(), pts, nlevels, scale_factors, nullptr, logScaleFactor, th);
}

int SearchAndFuseBatch::resolve(int k, const uint8_t* skip_now, const uint8_t* desc_now, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
  if (k < 0 || k >= K_) throw infrastructure_ex("SearchAndFuseBatch::resolve: keyframe out of range");
  bestIdx.assign((size_t)P_, -1); bestDist.assign((size_t)P_, INT_MAX);
  int nFused = 0;
  for (int i = 0; i < P_; i++) {
    if (skip_now && skip_now[i]) continue;
    fuse_resolve_point(scene_, table_[(size_t)k * P_ + i], k, (size_t)i, desc_now ? desc_now + 32 * (size_t)i : nullptr, n_reeval_, bestIdx[i], bestDist[i], nFused);
  }
  return nFused;
}

SearchInNeighborsBatch::SearchInNeighborsBatch(HipContext* ctx, const KeyFrames& kfs, int n_calls, const int32_t* target, int current, const Points& pts, int n_current,
                                               int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th)
    : K_(kfs.K), C_(n_calls), cur_(current), P1_(n_current), P2_(pts.P - n_current) {
  init(&kfs, nullptr, nullptr, kfs.pose, ctx, target, pts, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th);
}
SearchInNeighborsBatch::SearchInNeighborsBatch(KeyFrameStore& store, HipContext* ctx, int K, const int64_t* keys, const float* pose, int n_calls, const int32_t* target,
                                               int current, const Points& pts, int n_current, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
                                               float logScaleFactor, float th)
    : K_(K), C_(n_calls), cur_(current), P1_(n_current), P2_(pts.P - n_current) {
  init(nullptr, &store, keys, pose, ctx, target, pts, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th);
}

void SearchInNeighborsBatch::init(const KeyFrames* flat, KeyFrameStore* store, const int64_t* keys, const float* pose, HipContext* ctx, const int32_t* target,
                                  const Points& pts, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th) {
  const int K = K_, P = pts.P, C = C_;
  if (K < 0 || P < 0 || C < 0 || P1_ < 0 || P1_ > P || (C > 0 && !target) || !scale_factors || !inv_level_sigma2 || nlevels < 1 || nlevels > FSM_MAX_LEVELS ||
      (int64_t)C * P1_ + P2_ > (int64_t)INT32_MAX || (store && K > 0 && (!keys || !pose)))
    throw infrastructure_ex("SearchInNeighborsBatch: bad arguments");
  if (store && !store->host_only() && !ctx) throw infrastructure_ex("SearchInNeighborsBatch: a device store needs the calling thread's context");
  // C jobs (target of call c, the current keyframe's points) and one (current keyframe, the predicted candidates); without a current keyframe the last job is left out
  std::vector<int32_t> jk, j0, jn;
  for (int c = 0; c < C; c++) { jk.push_back(target[c]); j0.push_back(0); jn.push_back(P1_); }
  if (cur_ >= 0) { jk.push_back(cur_); j0.push_back(P1_); jn.push_back(P2_); }
  else if (P2_ > 0) throw infrastructure_ex("SearchInNeighborsBatch: candidates without a current keyframe");
  const int J = (int)jk.size();
  Shadows shadows;
  if (store && !store_shadows(*store, K, keys, shadows)) throw infrastructure_ex("SearchInNeighborsBatch: a key is not in the store");
  table_.assign((size_t)C * (size_t)P1_ + (size_t)P2_, 0); n_valid_.assign((size_t)J, 0); n_hit_.assign((size_t)J, 0);
  if (store && !store->host_only()) {
    check(ccm_fuse_pose_eval_resident(ctx->get(), store->handle(), K, keys, pose, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th, P, pts.pos, pts.normal,
                                      pts.min_dist, pts.max_dist, pts.desc, J, jk.data(), j0.data(), jn.data(), table_.data(), n_valid_.data(), n_hit_.data(), nullptr),
          ctx->get(), "ccm_fuse_pose_eval_resident");
  } else if (store) {
    int64_t total = 0, tiles = 0;
    if (fsm_check_scalars(K, P, nlevels, th) || fpm_check_jobs(J, K, P, jk.data(), j0.data(), jn.data(), &total, &tiles) ||
        (P > 0 && (!pts.pos || !pts.normal || !pts.min_dist || !pts.max_dist || !pts.desc)))
      throw infrastructure_ex("SearchInNeighborsBatch: bad arguments");
    proj_jobs_host<true, false, false>(ShadowKfs{shadows}, pose, nullptr, nullptr, {nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th},
                                       {P, pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc}, J, jk.data(), j0.data(), jn.data(), table_.data(), n_valid_.data(),
                                       n_hit_.data(), nullptr, nullptr);
  } else if (ctx) {
    check(ccm_fuse_pose_eval(ctx->get(), K, flat->rec, flat->feat_off, flat->feat_xy, flat->feat_octave, flat->feat_desc, flat->cell_off, flat->cell_idx, pose, nlevels,
                             scale_factors, inv_level_sigma2, logScaleFactor, th, P, pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc, J, jk.data(), j0.data(),
                             jn.data(), table_.data(), n_valid_.data(), n_hit_.data(), nullptr),
          ctx->get(), "ccm_fuse_pose_eval");
  } else if (fuse_pose_eval_host(K, flat->rec, flat->feat_off, flat->feat_xy, flat->feat_octave, flat->feat_desc, flat->cell_off, flat->cell_idx, pose, nlevels, scale_factors,
                                 inv_level_sigma2, logScaleFactor, th, P, pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc, J, jk.data(), j0.data(), jn.data(),
                                 table_.data(), n_valid_.data(), n_hit_.data(), nullptr, nullptr)) {
    throw infrastructure_ex("SearchInNeighborsBatch: bad arguments");
  }
  // the arguments are valid from here on: what the resolves may have to evaluate again
  target_.assign(jk.begin(), jk.begin() + C);
  if (store) scene_.hold(std::move(shadows), pose, pts, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th);
  else scene_.copy(*flat, pose, pts, nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th);
}

int SearchInNeighborsBatch::resolve(int c, const uint8_t* skip_now, const uint8_t* desc_now, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
  if (c < 0 || c >= C_) throw infrastructure_ex("SearchInNeighborsBatch::resolve: call out of range");
  bestIdx.assign((size_t)P1_, -1); bestDist.assign((size_t)P1_, 256);
  int nFused = 0;
  for (int i = 0; i < P1_; i++) {
    if (skip_now && skip_now[i]) continue;
    fuse_resolve_point(scene_, table_[(size_t)c * P1_ + i], target_[c], (size_t)i, desc_now ? desc_now + 32 * (size_t)i : nullptr, n_reeval_, bestIdx[i], bestDist[i], nFused);
  }
  return nFused;
}

int SearchInNeighborsBatch::resolve_current(int n, const int32_t* slot, const uint8_t* skip_now, const uint8_t* desc_now, const Points& fresh,
                                            std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
  if (n < 0 || (n > 0 && !slot) || cur_ < 0) throw infrastructure_ex("SearchInNeighborsBatch::resolve_current: bad arguments");
  bestIdx.assign((size_t)n, -1); bestDist.assign((size_t)n, 256);
  int nFused = 0;
  for (int i = 0; i < n; i++) {
    if (skip_now && skip_now[i]) continue;
    const int s = slot[i];
    if (s >= P2_ || s < -1) throw infrastructure_ex("SearchInNeighborsBatch::resolve_current: slot out of range");
    if (s < 0) {                                                 // a candidate the build did not predict: from what the caller passes for it
      if (!fresh.pos || !fresh.normal || !fresh.min_dist || !fresh.max_dist || !fresh.desc || fresh.P < n)
        throw infrastructure_ex("SearchInNeighborsBatch::resolve_current: an unpredicted candidate without fresh data");
      const uint32_t w = scene_.eval(cur_, fresh.pos + 3 * (size_t)i, fresh.normal + 3 * (size_t)i, fresh.min_dist[i], fresh.max_dist[i],
                                     desc_now ? desc_now + 32 * (size_t)i : fresh.desc + 32 * (size_t)i);
      n_unpredicted_++;
      sin_answer(w, bestIdx[i], bestDist[i], nFused);
    } else {
      fuse_resolve_point(scene_, table_[(size_t)C_ * P1_ + s], cur_, (size_t)P1_ + (size_t)s, desc_now ? desc_now + 32 * (size_t)i : nullptr, n_reeval_, bestIdx[i],
                         bestDist[i], nFused);
    }
  }
  return nFused;
}

// ---- ComputeSim3's two projected searches: Sim3ProjectionSearch, SearchBySim3Batch ------------------------------
Sim3ProjectionSearch::Sim3ProjectionSearch(KeyFrameStore& store, HipContext* ctx, int64_t key, const float* Scw12, const Points& pts, const uint8_t* matched0, int nlevels,
                                           const float* scale_factors, float logScaleFactor, float th)
    : P_(pts.P) {
  const int P = P_;
  if (P < 0 || !Scw12 || !scale_factors || nlevels < 1 || nlevels > FSM_MAX_LEVELS) throw infrastructure_ex("Sim3ProjectionSearch: bad arguments");
  std::vector<std::shared_ptr<const KfShadow>> kfs;
  if (!store_shadows(store, 1, &key, kfs)) throw infrastructure_ex("Sim3ProjectionSearch: the key is not in the store");
  N_ = kfs[0]->n;
  if (N_ > 0 && !matched0) throw infrastructure_ex("Sim3ProjectionSearch: bad arguments");
  const int32_t skip_off[2] = {0, N_};
  table_.assign((size_t)P, 0);
  if (!store.host_only() && ctx) {
    check(ccm_sim3_project_eval_resident(ctx->get(), store.handle(), 1, &key, Scw12, skip_off, matched0, nlevels, scale_factors, logScaleFactor, th, P, pts.pos,
                                         pts.normal, pts.min_dist, pts.max_dist, pts.desc, table_.data(), &n_valid_, &n_hit_, nullptr),
          ctx->get(), "ccm_sim3_project_eval_resident");
  } else if (sim3_project_eval_resident_host(store, 1, &key, Scw12, skip_off, matched0, nlevels, scale_factors, logScaleFactor, th, P, pts.pos, pts.normal, pts.min_dist,
                                             pts.max_dist, pts.desc, table_.data(), &n_valid_, &n_hit_, nullptr)) {
    throw infrastructure_ex("Sim3ProjectionSearch: bad arguments");
  }
  float pose[FSM_POSE_FLOATS];
  fsm_decompose_scw(Scw12, pose);
  scene_.hold(std::move(kfs), pose, pts, nlevels, scale_factors, nullptr, logScaleFactor, th);
}

int Sim3ProjectionSearch::resolve(const uint8_t* skip_now, const int32_t* existing_idx, int32_t* matched, std::vector<int32_t>& bestIdx, std::vector<int32_t>& remap) {
  bestIdx.assign((size_t)P_, -1); remap.assign((size_t)P_, -1);
  if (N_ > 0 && !matched) throw infrastructure_ex("Sim3ProjectionSearch::resolve: bad arguments");
  const FuseScene& s = scene_;
  const FuseKf kf = fuse_kf(*s.shadow[0]);
  std::vector<uint8_t> claimed((size_t)N_, 0), mask;   // mask: vpMatched as it is now, made when the first point needs it
  int nmatches = 0;
  for (int i = 0; i < P_; i++) {
    if (skip_now && skip_now[i]) continue;
    uint32_t w = table_[(size_t)i];
    if ((w >> 29) != FSM_HIT) continue;
    if (claimed[w & 0xFFFFu]) {
      if (mask.empty()) {
        mask.resize((size_t)N_);
        for (int f = 0; f < N_; f++) mask[f] = matched[f] >= 0;
      }
      w = proj_pair_host<false, true, false>(kf, s.pose.data(), mask.data(), scene_levels(s), s.pos.data() + 3 * (size_t)i, s.normal.data() + 3 * (size_t)i, s.dmin[i],
                                             s.dmax[i], s.pdesc.data() + 32 * (size_t)i, nullptr, nullptr);
      n_reeval_++;
      if ((w >> 29) != FSM_HIT) continue;
    }
    const int32_t f = (int32_t)(w & 0xFFFFu);
    if (existing_idx && existing_idx[i] >= 0) { remap[i] = f; continue; }   // :415-434: the caller's GetMapPoint / RemapMapPointMatch; no claim, not counted
    matched[f] = i; claimed[f] = 1;
    if (!mask.empty()) mask[f] = 1;
    bestIdx[i] = f;
    nmatches++;
  }
  return nmatches;
}

SearchBySim3Batch::SearchBySim3Batch(KeyFrameStore& store, HipContext* ctx, int64_t key1, int64_t key2, const Side& kf1, const Side& kf2, float s12, const float* R12,
                                     const float* t12, const int32_t* matches12_in, int nlevels, const float* scale_factors, float logScaleFactor, float th) {
  const int N1 = kf1.N, N2 = kf2.N;
  auto side_ok = [](const Side& sd) { return sd.N >= 0 && sd.pose && (sd.N == 0 || (sd.live && sd.pos && sd.min_dist && sd.max_dist && sd.desc)); };
  if (!side_ok(kf1) || !side_ok(kf2) || !R12 || !t12 || (N1 > 0 && !matches12_in) || !scale_factors || nlevels < 1 || nlevels > FSM_MAX_LEVELS)
    throw infrastructure_ex("SearchBySim3Batch: bad arguments");
  const int64_t keys[2] = {key1, key2};
  std::vector<std::shared_ptr<const KfShadow>> kfs;
  if (!store_shadows(store, 2, keys, kfs)) throw infrastructure_ex("SearchBySim3Batch: a key is not in the store");
  if (kfs[0]->n != N1 || kfs[1]->n != N2) throw infrastructure_ex("SearchBySim3Batch: a side is not as long as its keyframe's features");
  // :1151-1164
  std::vector<uint8_t> already1((size_t)N1, 0), already2((size_t)N2, 0);
  for (int i = 0; i < N1; i++)
    if (matches12_in[i] != -1) {
      already1[i] = 1;
      if (matches12_in[i] >= 0 && matches12_in[i] < N2) already2[matches12_in[i]] = 1;
    }
  // the live unmatched points of keyframe 1, then those of keyframe 2: job 0 searches keyframe 2 (index 1 of keys), job 1 keyframe 1
  std::vector<int32_t> src;   // the feature slot of every packed point
  std::vector<float> pos, dmin, dmax;
  std::vector<uint8_t> desc;
  auto pack = [&](const Side& sd, const std::vector<uint8_t>& already) {
    int n = 0;
    for (int i = 0; i < sd.N; i++) {
      if (!sd.live[i] || already[i]) continue;
      src.push_back(i); n++;
      pos.insert(pos.end(), sd.pos + 3 * (size_t)i, sd.pos + 3 * (size_t)i + 3);
      dmin.push_back(sd.min_dist[i]); dmax.push_back(sd.max_dist[i]);
      desc.insert(desc.end(), sd.desc + 32 * (size_t)i, sd.desc + 32 * (size_t)i + 32);
    }
    return n;
  };
  const int n1 = pack(kf1, already1), n2 = pack(kf2, already2);
  const int P = n1 + n2;
  float sR12[9], sR21[9], t21[3];
  ssm_derive(s12, R12, t12, sR12, sR21, t21);
  const int32_t job_kf[2] = {1, 0}, job_pt0[2] = {0, n1}, job_n[2] = {n1, n2};
  float job_K4[8], job_src[24], job_T[24];
  for (int j = 0; j < 2; j++) std::memcpy(job_K4 + 4 * j, kfs[0]->rec, 4 * sizeof(float));   // pKF1's fx fy cx cy in both directions (:1127-1130)
  std::memcpy(job_src, kf1.pose, 12 * sizeof(float)); std::memcpy(job_src + 12, kf2.pose, 12 * sizeof(float));
  std::memcpy(job_T, sR21, 9 * sizeof(float)); std::memcpy(job_T + 9, t21, 3 * sizeof(float));
  std::memcpy(job_T + 12, sR12, 9 * sizeof(float)); std::memcpy(job_T + 21, t12, 3 * sizeof(float));
  std::vector<uint32_t> table((size_t)P, 0);
  n_valid_.assign(2, 0); n_hit_.assign(2, 0);
  if (!store.host_only() && ctx) {
    check(ccm_sim3_pair_eval_resident(ctx->get(), store.handle(), 2, keys, nlevels, scale_factors, logScaleFactor, th, P, pos.data(), dmin.data(), dmax.data(), desc.data(),
                                      2, job_kf, job_K4, job_src, job_T, job_pt0, job_n, table.data(), n_valid_.data(), n_hit_.data(), nullptr),
          ctx->get(), "ccm_sim3_pair_eval_resident");
  } else if (sim3_pair_eval_resident_host(store, 2, keys, nlevels, scale_factors, logScaleFactor, th, P, pos.data(), dmin.data(), dmax.data(), desc.data(), 2, job_kf,
                                          job_K4, job_src, job_T, job_pt0, job_n, table.data(), n_valid_.data(), n_hit_.data(), nullptr)) {
    throw infrastructure_ex("SearchBySim3Batch: bad arguments");
  }
  vn1_.assign((size_t)N1, -1); vn2_.assign((size_t)N2, -1);
  for (int e = 0; e < P; e++)
    if ((table[e] >> 29) == FSM_HIT) (e < n1 ? vn1_ : vn2_)[src[e]] = (int32_t)(table[e] & 0xFFFFu);
  std::vector<int32_t> agreed;
  n_found_ = ORBmatcher::MutualAgreement(vn1_, vn2_, agreed);
  matches12_.assign(matches12_in, matches12_in + N1);
  for (int i = 0; i < N1; i++)
    if (agreed[i] >= 0) matches12_[i] = agreed[i];
}

// ---- ComputeSim3's SearchByBoW for all candidates: the host evaluator on the shadows, SearchByBoWBatch ---------------------------------
static BowKf bow_kf(const KfShadow& kf) { return {kf.n, (int)kf.fv_node.size(), kf.fv_node.data(), kf.fv_off.data(), kf.fv_idx.data(), kf.desc.data()}; }

// What bow_pair_eval_resident_host and tri_search_eval_resident_host check alike behind their own scalar rules, in the order and with the rules of the device stage
// (csrc/fv_pair.h): the pointers, both key lists' shadows (a, b), the feature vectors, the two mask arrays against the shadows' feature counts, the table.  false
// where the entry returns CCM_E_ARG.
static bool fv_pair_front_host(const KeyFrameStore& store, int J, const int64_t* key1, const int64_t* key2, const int32_t* off1, const uint8_t* mask1, const int32_t* off2,
                               const uint8_t* mask2, const void* table, bool counters, Shadows& a, Shadows& b) {
  if (!key1 || !key2 || !off1 || !off2 || !counters) return false;
  if (!store_shadows(store, J, key1, a) || !store_shadows(store, J, key2, b)) return false;
  std::vector<int32_t> n1((size_t)J), n2((size_t)J);
  for (int j = 0; j < J; j++) {
    if (!a[j]->has_fv || !b[j]->has_fv) return false;
    n1[j] = a[j]->n; n2[j] = b[j]->n;
  }
  if (bsm_check_masks(J, off1, mask1, n1.data()) || bsm_check_masks(J, off2, mask2, n2.data())) return false;
  return off1[J] == 0 || table;
}

// What SearchByBoWBatch and SearchForTriangulationBatch build alike for their one call: key1 and its mask once per candidate, the candidates' own masks one after the
// other, and the offsets of both.  Throws for a key without a feature vector and for a missing mask.
struct FvPairMasks { std::vector<int64_t> k1; std::vector<int32_t> off1, off2; std::vector<uint8_t> m1, m2; };
static FvPairMasks fv_pair_masks(const std::string& who, int64_t key1, const KfShadow& K1, int C, const Shadows& kfs2, const uint8_t* mask1, const uint8_t* const* mask2) {
  if (!K1.has_fv) throw infrastructure_ex(who + ": a key without a feature vector");
  const int N1 = K1.n;
  if (N1 > 0 && !mask1) throw infrastructure_ex(who + ": bad arguments");
  FvPairMasks m{std::vector<int64_t>((size_t)C, key1), std::vector<int32_t>((size_t)C + 1, 0), std::vector<int32_t>((size_t)C + 1, 0), {}, {}};
  for (int j = 0; j < C; j++) {
    if (!kfs2[j]->has_fv) throw infrastructure_ex(who + ": a key without a feature vector");
    if (kfs2[j]->n > 0 && !mask2[j]) throw infrastructure_ex(who + ": bad arguments");
    m.off1[j + 1] = m.off1[j] + N1; m.off2[j + 1] = m.off2[j] + kfs2[j]->n;
  }
  m.m1.resize((size_t)m.off1[C]); m.m2.resize((size_t)m.off2[C]);
  for (int j = 0; j < C; j++) {
    if (N1) std::memcpy(m.m1.data() + m.off1[j], mask1, (size_t)N1);
    if (kfs2[j]->n) std::memcpy(m.m2.data() + m.off2[j], mask2[j], (size_t)kfs2[j]->n);
  }
  return m;
}

int bow_pair_eval_resident_host(const KeyFrameStore& store, int J, const int64_t* key1, const int64_t* key2, const int32_t* live1_off, const uint8_t* live1,
                                const int32_t* live2_off, const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  if (J < 0) return -1;
  if (J == 0) return 0;
  Shadows a, b;
  if (!fv_pair_front_host(store, J, key1, key2, live1_off, live1, live2_off, live2, table, n_query && n_dist, a, b)) return -1;
  std::vector<BowKf> k1((size_t)J), k2((size_t)J);
  for (int j = 0; j < J; j++) { k1[j] = bow_kf(*a[j]); k2[j] = bow_kf(*b[j]); }
  bow_pair_eval_host(J, k1.data(), k2.data(), live1_off, live1, live2_off, live2, table, n_query, n_dist);
  return 0;
}

SearchByBoWBatch::SearchByBoWBatch(KeyFrameStore& store, HipContext* ctx, int64_t key1, int C, const int64_t* keys2, const uint8_t* live1, const uint8_t* const* live2,
                                   float nnratio, bool checkOrientation) {
  if (C < 0 || (C > 0 && (!keys2 || !live2))) throw infrastructure_ex("SearchByBoWBatch: bad arguments");
  Shadows kf1, kfs2;
  if (!store_shadows(store, 1, &key1, kf1) || !store_shadows(store, C, keys2, kfs2)) throw infrastructure_ex("SearchByBoWBatch: a key is not in the store");
  const KfShadow& K1 = *kf1[0];
  const FvPairMasks m = fv_pair_masks("SearchByBoWBatch", key1, K1, C, kfs2, live1, live2);   // live1 once per candidate, the candidates' own one after the other
  const int N1 = K1.n;
  table_.assign((size_t)m.off1[C], 0); n_query_.assign((size_t)C, 0); n_dist_.assign((size_t)C, 0);
  if (C > 0 && !store.host_only() && ctx) {
    check(ccm_bow_pair_eval_resident(ctx->get(), store.handle(), C, m.k1.data(), keys2, m.off1.data(), m.m1.data(), m.off2.data(), m.m2.data(), table_.data(), n_query_.data(),
                                     n_dist_.data()),
          ctx->get(), "ccm_bow_pair_eval_resident");
  } else if (bow_pair_eval_resident_host(store, C, m.k1.data(), keys2, m.off1.data(), m.m1.data(), m.off2.data(), m.m2.data(), table_.data(), n_query_.data(), n_dist_.data())) {
    throw infrastructure_ex("SearchByBoWBatch: bad arguments");
  }
  // the reference's loop per candidate (:585-698) on the words
  const int TH_LOW = ORBmatcher::TH_LOW;
  nmatches_.assign((size_t)C, 0); matches12_.resize((size_t)C);
  std::vector<int> claimed;   // the features of keyframe 2 claimed so far in the node at hand
  for (int j = 0; j < C; j++) {
    const KfShadow& K2 = *kfs2[j];
    const BowKf b2 = bow_kf(K2);
    const uint64_t* words = table_.data() + m.off1[j];
    const uint8_t* l2 = m.m2.data() + m.off2[j];
    std::vector<int32_t>& matches12 = matches12_[(size_t)j];
    matches12.assign((size_t)N1, -1);
    std::vector<uint8_t> vbMatched2((size_t)K2.n, 0);
    RotationFilter rot;
    int nmatches = 0;
    for (size_t a = 0; a < K1.fv_node.size(); a++) {   // ascending nodes of keyframe 1; those keyframe 2 lacks hold no query
      claimed.clear();
      for (int32_t s1 = K1.fv_off[a]; s1 < K1.fv_off[a + 1]; s1++) {
        const int idx1 = K1.fv_idx[(size_t)s1];
        const uint64_t w = words[idx1];
        if (bsm_status(w) != BSM_EVALUATED) continue;   // not live, no common node, or no live candidate: bestDist1 stays 256
        BowBest r = bsm_best(w);
        if (r.d1 >= TH_LOW) continue;                   // stands whatever was claimed
        const uint8_t* qd = K1.desc.data() + 32 * (size_t)idx1;
        bool again = false;
        for (int c : claimed)
          if (bsm_hamming(qd, K2.desc.data() + 32 * (size_t)c) <= r.d2) { again = true; break; }
        if (again) {
          int n_live = 0;
          r = bsm_reduce_host(qd, b2, bsm_node2(w), l2, vbMatched2.data(), &n_live, nullptr);
          n_reeval_++;
        }
        if (r.d1 < TH_LOW && static_cast<float>(r.d1) < nnratio * static_cast<float>(r.d2)) {   // :641, strict
          matches12[(size_t)idx1] = r.idx;
          vbMatched2[(size_t)r.idx] = 1;
          claimed.push_back(r.idx);
          if (checkOrientation) rot.add(K1.angle[(size_t)idx1] - K2.angle[(size_t)r.idx], idx1);
          nmatches++;
        }
      }
    }
    if (checkOrientation) rot.reject_outliers([&](int k) { matches12[(size_t)k] = -1; nmatches--; });
    nmatches_[(size_t)j] = nmatches;
  }
}

// ---- CreateNewMapPoints' SearchForTriangulation for all neighbours: the host evaluator on the shadows, SearchForTriangulationBatch -------
static TriKf tri_kf(const KfShadow& kf) { return {bow_kf(kf), kf.xy.data(), kf.oct.data()}; }

int tri_search_eval_resident_host(const KeyFrameStore& store, int J, const int64_t* key1, const int64_t* key2, const int32_t* has1_off, const uint8_t* has1,
                                  const int32_t* has2_off, const uint8_t* has2, const float* job_epi, int nlevels, const float* scale_factors, const float* level_sigma2,
                                  uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  if (J < 0 || tsm_check_args(J, job_epi, nlevels, scale_factors, level_sigma2)) return -1;
  if (J == 0) return 0;
  Shadows a, b;
  if (!fv_pair_front_host(store, J, key1, key2, has1_off, has1, has2_off, has2, table, n_query && n_match && n_dist, a, b)) return -1;
  std::vector<TriKf> k1((size_t)J), k2((size_t)J);
  for (int j = 0; j < J; j++) { k1[j] = tri_kf(*a[j]); k2[j] = tri_kf(*b[j]); }
  tri_search_eval_host(J, k1.data(), k2.data(), has1_off, has1, has2_off, has2, job_epi, TriLevels{nlevels, scale_factors, level_sigma2}, table, n_query, n_match, n_dist);
  return 0;
}

SearchForTriangulationBatch::SearchForTriangulationBatch(KeyFrameStore& store, HipContext* ctx, int64_t key1, int C, const int64_t* keys2, const uint8_t* has1,
                                                         const uint8_t* const* has2, const Epipolar* ep, const float* sigma2_2, const float* sf2, int nlevels,
                                                         bool checkOrientation)
    : nlevels_(nlevels), check_ori_(checkOrientation) {
  const char* const bad = "SearchForTriangulationBatch: bad arguments";
  if (C < 0 || (C > 0 && (!keys2 || !has2 || !ep)) || nlevels < 1 || nlevels > TSM_MAX_LEVELS || !sigma2_2 || !sf2) throw infrastructure_ex(bad);
  Shadows kf1;
  if (!store_shadows(store, 1, &key1, kf1) || !store_shadows(store, C, keys2, kfs2_)) throw infrastructure_ex("SearchForTriangulationBatch: a key is not in the store");
  kf1_ = kf1[0];
  FvPairMasks m = fv_pair_masks("SearchForTriangulationBatch", key1, *kf1_, C, kfs2_, has1, has2);   // has1 once per neighbour, the neighbours' own one after the other
  sigma2_.assign(sigma2_2, sigma2_2 + nlevels); sf_.assign(sf2, sf2 + nlevels);
  has1_.assign(has1, has1 + kf1_->n);
  off1_ = std::move(m.off1); off2_ = std::move(m.off2); has2_ = std::move(m.m2);
  epi_.resize((size_t)TSM_EPI_FLOATS * (size_t)C);
  for (int j = 0; j < C; j++) {
    std::memcpy(epi_.data() + TSM_EPI_FLOATS * (size_t)j, ep[j].F12, 9 * sizeof(float));
    epi_[TSM_EPI_FLOATS * (size_t)j + 9] = ep[j].ex; epi_[TSM_EPI_FLOATS * (size_t)j + 10] = ep[j].ey;
  }
  table_.assign((size_t)off1_[C], 0); n_query_.assign((size_t)C, 0); n_match_.assign((size_t)C, 0); n_dist_.assign((size_t)C, 0);
  if (C > 0 && !store.host_only() && ctx) {
    check(ccm_tri_search_eval_resident(ctx->get(), store.handle(), C, m.k1.data(), keys2, off1_.data(), m.m1.data(), off2_.data(), has2_.data(), epi_.data(), nlevels,
                                       sf_.data(), sigma2_.data(), table_.data(), n_query_.data(), n_match_.data(), n_dist_.data()),
          ctx->get(), "ccm_tri_search_eval_resident");
  } else if (tri_search_eval_resident_host(store, C, m.k1.data(), keys2, off1_.data(), m.m1.data(), off2_.data(), has2_.data(), epi_.data(), nlevels, sf_.data(),
                                           sigma2_.data(), table_.data(), n_query_.data(), n_match_.data(), n_dist_.data())) {
    throw infrastructure_ex(bad);
  }
}

int SearchForTriangulationBatch::resolve(int j, const uint8_t* has1_now, const uint8_t* has2_now, std::vector<int32_t>& matches12) {
  const KfShadow& K1 = *kf1_;
  const KfShadow& K2 = *kfs2_.at((size_t)j);
  const TriKf t1 = tri_kf(K1), t2 = tri_kf(K2);
  const TriLevels lv{nlevels_, sf_.data(), sigma2_.data()};
  const uint32_t* words = table_.data() + off1_[(size_t)j];
  const uint8_t* h2_build = has2_.data() + off2_[(size_t)j];
  const uint8_t* h1 = has1_now ? has1_now : has1_.data();
  const uint8_t* h2 = has2_now ? has2_now : h2_build;
  const float* epi = epi_.data() + TSM_EPI_FLOATS * (size_t)j;
  matches12.assign((size_t)K1.n, -1);
  RotationFilter rot;
  int nmatches = 0;
  for (size_t a = 0; a < K1.fv_node.size(); a++) {   // ascending nodes of keyframe 1; those keyframe 2 lacks hold no query
    const int b = bsm_find_node(t2.k.node, t2.k.nn, K1.fv_node[a]);
    if (b < 0) continue;
    bool lost = false;   // a feature of the node's segment of keyframe 2 had a map point at the build and has none now: it is a candidate no word has seen
    if (has2_now)
      for (int32_t s = K2.fv_off[(size_t)b]; s < K2.fv_off[(size_t)b + 1] && !lost; s++) lost = h2_build[K2.fv_idx[(size_t)s]] && !h2[K2.fv_idx[(size_t)s]];
    for (int32_t s1 = K1.fv_off[a]; s1 < K1.fv_off[a + 1]; s1++) {
      const int idx1 = K1.fv_idx[(size_t)s1];
      if (h1[idx1]) continue;   // :745-747 with the flags of this call
      TriBest r;
      int n_free = 0;
      if (has1_[(size_t)idx1]) {   // had a map point at the build: it has no word
        r = tsm_reduce_host(t1, idx1, t2, b, h2, epi, lv, &n_free);
      } else {
        r = TriBest{tsm_dist(words[idx1]), tsm_idx(words[idx1])};
        if (has2_now && (lost || (r.idx >= 0 && h2[r.idx]))) {   // a candidate that gains a map point and is not the winner leaves the winner as it is
          r = tsm_reduce_host(t1, idx1, t2, b, h2, epi, lv, &n_free);
          n_reeval_++;
        }
      }
      if (r.idx >= 0) {   // :787-804
        matches12[(size_t)idx1] = r.idx;
        nmatches++;
        if (check_ori_) rot.add(K1.angle[(size_t)idx1] - K2.angle[(size_t)r.idx], idx1);
      }
    }
  }
  if (check_ori_) rot.reject_outliers([&](int k) { matches12[(size_t)k] = -1; nmatches--; });
  return nmatches;
}

// ---- the refresh of map points after a map stage: the host evaluator on the shadows, MapPointRefresh -------------------------------------
int mappoint_refresh_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf,
                                        const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels, const float* scale_factors,
                                        int32_t* best_obs, uint8_t* best_desc, float* normal, float* min_dist, float* max_dist, uint8_t* status) {
  bool nd = false;
  if (mpm_check_args(K, keys, kf_center, P, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, nlevels, scale_factors, best_obs, normal, min_dist, max_dist, status, &nd))
    return -1;
  Shadows kfs;
  if (!store_shadows(store, K, keys, kfs)) return -1;
  std::vector<int32_t> kf_n((size_t)(K > 0 ? K : 0));
  std::vector<MpmKf> kf(kf_n.size());
  for (int k = 0; k < K; k++) { kf_n[k] = kfs[k]->n; kf[k] = MpmKf{kfs[k]->n, kfs[k]->desc.data(), kfs[k]->oct.data()}; }
  if (mpm_check_features(kf_n.data(), P, obs_off, obs_kf, obs_feat, ref_kf, ref_feat)) return -1;
  mappoint_refresh_eval_host(kf.data(), kf_center, P, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, nlevels, scale_factors, best_obs, best_desc, normal, min_dist,
                             max_dist, status);
  return 0;
}

MapPointRefresh::MapPointRefresh(KeyFrameStore& store, HipContext* ctx, int K, const int64_t* keys, const float* kf_center, const Lists& l, const Refs& r, int nlevels,
                                 const float* scale_factors) {
  const char* const bad = "MapPointRefresh: bad arguments or a key that is not in the store";
  const int P = l.P;
  if (P < 0 || (P > 0 && (!r.normal || !r.min_dist || !r.max_dist))) throw infrastructure_ex(bad);
  const size_t n = (size_t)P;
  best_.assign(n, -1); desc_.assign(32 * n, 0); status_.assign(n, 0);
  if (P > 0) { normal_.assign(r.normal, r.normal + 3 * n); dmin_.assign(r.min_dist, r.min_dist + n); dmax_.assign(r.max_dist, r.max_dist + n); }
  if (!store.host_only() && ctx) {
    const int rc = ccm_mappoint_refresh_resident(ctx->get(), store.handle(), K, keys, kf_center, P, l.obs_off, l.obs_kf, l.obs_feat, r.pos, r.ref_kf, r.ref_feat, nlevels,
                                                 scale_factors, best_.data(), desc_.data(), normal_.data(), dmin_.data(), dmax_.data(), status_.data());
    if (rc == CCM_E_ARG) throw infrastructure_ex(bad);
    check(rc, ctx->get(), "ccm_mappoint_refresh_resident");
  } else if (mappoint_refresh_eval_resident_host(store, K, keys, kf_center, P, l.obs_off, l.obs_kf, l.obs_feat, r.pos, r.ref_kf, r.ref_feat, nlevels, scale_factors,
                                                 best_.data(), desc_.data(), normal_.data(), dmin_.data(), dmax_.data(), status_.data())) {
    throw infrastructure_ex(bad);
  }
}

NewMapPointBatch::Pairs SearchForTriangulationBatch::predicted(int j) {
  std::vector<int32_t> m;
  resolve(j, nullptr, nullptr, m);
  NewMapPointBatch::Pairs out;
  for (size_t i = 0; i < m.size(); i++)   // :844-849
    if (m[i] >= 0) out.emplace_back((int32_t)i, m[i]);
  return out;
}

}  // namespace cslam
