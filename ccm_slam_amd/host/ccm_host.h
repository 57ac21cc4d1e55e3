// ccm_host.h — host-side C++ mirror of the reference's class API for the hot path, on top of the C ABI
// (include/ccm_hip.h).  This is what replaces the three reference translation units
//   cslam/src/ORBextractor.cpp, cslam/src/ORBmatcher.cpp, cslam/src/Optimizer.cpp
// in a drop-in build (INTEGRATION.md shows the glue that walks the reference's shared_ptr graph).
//
// The reference's data model (Frame / KeyFrame / MapPoint / Map, OpenCV types) is OUT OF SCOPE and not
// available in this image, so the classes below take *views*: plain structs of pointers into the caller's
// arrays, holding exactly the fields the reference methods read.  With CCM_HAVE_OPENCV defined the
// ORBextractor additionally offers the cv::InputArray / cv::OutputArray operator() of the reference.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/ccm_hip.h"
#include "sim3_schedule.h"
#include "pnp_schedule.h"
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>

struct kfi_tree;   // csrc/kfingest_math.h: the flat vocabulary tree on the host

namespace cslam {

// thrown where the reference throws estd::infrastructure_ex (cslam/include/cslam/estd.h:74-81)
struct infrastructure_ex : std::runtime_error { using std::runtime_error::runtime_error; };

// one device context per calling thread (SURVEY §8b threading)
class HipContext {
 public:
  explicit HipContext(int device = 0);
  ~HipContext();
  ccm_ctx* get() const { return ctx_; }
 private:
  ccm_ctx* ctx_ = nullptr;
};

// ---------------------------------------------------------------------------------------------------
// ORBextractor — cslam/include/cslam/ORBextractor.h:103-138
// ---------------------------------------------------------------------------------------------------
struct KeyPoint { float x, y, size, angle, response; int octave; };   // cv::KeyPoint minus class_id

class ORBextractor {
 public:
  ORBextractor(HipContext& ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST);
  ~ORBextractor();
  // operator()(image, mask /*ignored, as in the reference*/, keypoints, descriptors): 8-bit single-channel image
  void operator()(const uint8_t* image, int cols, int rows, int step, std::vector<KeyPoint>& keypoints,
                  std::vector<uint8_t>& descriptors /* N x 32, row-major like cv::Mat CV_8U */);
  int GetLevels() const { return nlevels_; }
  float GetScaleFactor() const { return scaleFactor_; }
  std::vector<float> GetScaleFactors() const { return table(0); }
  std::vector<float> GetInverseScaleFactors() const { return table(1); }
  std::vector<float> GetScaleSigmaSquares() const { return table(2); }
  std::vector<float> GetInverseScaleSigmaSquares() const { return table(3); }
  // mvImagePyramid (public member of the reference): un-bordered levels of the last frame
  struct Level { int cols, rows; std::vector<uint8_t> data; };
  std::vector<Level> mvImagePyramid;
  bool keepPyramid = false;   // fill mvImagePyramid on every call (costs a D2H of ~1.1 MB)
 private:
  std::vector<float> table(int which) const;
  ccm_orb* orb_ = nullptr;
  int nlevels_; float scaleFactor_;
};

// ---------------------------------------------------------------------------------------------------
// ORBmatcher — cslam/include/cslam/ORBmatcher.h:100-139
// ---------------------------------------------------------------------------------------------------
// What SearchByProjection reads from a Frame (cslam/include/cslam/Frame.h:131-152)
struct FrameView {
  int N = 0;
  const KeyPoint* mvKeysUn = nullptr;       // undistorted keypoints (x, y, octave, angle)
  const uint8_t* mDescriptors = nullptr;    // N x 32
  float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
  const float* mvScaleFactors = nullptr;    // nlevels
  // mvpMapPoints as indices: -1 = no map point; >= 0 = a map point with Observations() > 0 ("claimed")
  int32_t* mvpMapPoints = nullptr;          // in/out, length N
};
// What the loop reads from each candidate map point (MapPoint.h:224-228,289)
struct TrackedMapPoints {
  int n = 0;
  const uint8_t* mbTrackInView = nullptr;   // && !isBad()
  const float* mTrackProjX = nullptr; const float* mTrackProjY = nullptr;
  const int32_t* mnTrackScaleLevel = nullptr;
  const float* mTrackViewCos = nullptr;
  const uint8_t* mDescriptor = nullptr;     // n x 32
};
// Last-frame side of SearchByProjection(Frame&, const Frame&, th): projections are computed by the caller
// (f32, ORBmatcher.cpp:1381-1397) — valid[i] = has map point && !outlier && in front && inside the image
struct LastFrameProjections {
  int n = 0;
  const uint8_t* valid = nullptr; const float* u = nullptr; const float* v = nullptr;
  const int32_t* octave = nullptr;          // LastFrame.mvKeys[i].octave
  const float* angle = nullptr;             // LastFrame.mvKeysUn[i].angle
  const uint8_t* mpDescriptor = nullptr;    // n x 32, pMP->GetDescriptor()
};

// DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) flattened: ascending node ids + CSR of feature indices
struct FeatureVectorView { int nn = 0; const int32_t* node = nullptr; const int32_t* off = nullptr; const int32_t* idx = nullptr; };
// What the BoW / triangulation / initialisation searches read from a KeyFrame or Frame
struct KeysView {
  int N = 0;
  const KeyPoint* keys = nullptr;           // mvKeysUn
  const uint8_t* desc = nullptr;            // N x 32
  const uint8_t* hasMapPoint = nullptr;     // vpMapPoints[i] && !isBad()
  FeatureVectorView fv;
};

// Device-resident grid of one Frame / KeyFrame (ccm_frame_*): undistorted keypoints, bounds, 75x48 cells, descriptors.
// Replaces Frame::UndistortKeyPoints / ComputeImageBounds / AssignFeaturesToGrid (Frame.cpp:103-118, 284-347) and serves
// batched GetFeaturesInArea + Hamming queries to the matcher.
class FrameGridDev {
 public:
  FrameGridDev(HipContext& ctx, const float K[4], const float* distCoef, int nDist, int width, int height);
  ~FrameGridDev();
  FrameGridDev(const FrameGridDev&) = delete;
  FrameGridDev& operator=(const FrameGridDev&) = delete;
  // mvKeys + mDescriptors in; mvKeysUn out (same order), bounds available afterwards
  void SetKeyPoints(const std::vector<KeyPoint>& mvKeys, const uint8_t* mDescriptors, std::vector<KeyPoint>& mvKeysUn);
  float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
  ccm_frame* get() const { return f_; }
 private:
  HipContext& ctx_;
  ccm_frame* f_ = nullptr;
};

// What SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist) reads from the candidate keyframe, per feature slot (ORBmatcher.cpp:1492-1539, :1568)
struct KeyFramePoints {
  int n = 0;
  const uint8_t* live = nullptr;            // pMP && !pMP->isBad()
  const float* pos = nullptr; const float* min_dist = nullptr; const float* max_dist = nullptr;   // GetWorldPos (n x 3), mfMinDistance, mfMaxDistance
  const uint8_t* desc = nullptr;            // n x 32, pMP->GetDescriptor()
  const float* angle = nullptr;             // pKF->mvKeysUn[i].angle
};
// What ccm_frame_guided_search returns for the n slots: the gates' outcome and every searched point's window candidates with their distances
struct GuidedCandidates {
  std::vector<uint8_t> status; std::vector<float> u, v; std::vector<int32_t> level, off, idx; std::vector<uint16_t> dist;
};

class ORBmatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
  // SearchByProjection(Frame&, kfptr, const set<mpptr>&, th, ORBdist) — ORBmatcher.cpp:1478-1604, the guided search of relocalisation.  pose.Tcw is the frame's
  // pose (the camera centre is derived from it, never passed); alreadyFound[slot] != 0: the slot's point is in sAlreadyFound (nullable: none).  On a match
  // F.mvpMapPoints[i2] = the keyframe's slot.  Returns nmatches; ORBdist outside 0 .. 255 throws.  With a grid, the gates, the windows and the distances of all
  // slots are ONE ccm_frame_guided_search call; without one, the host evaluator (the same header, a host grid, no device) produces the same arrays.  Both end in
  // GuidedReplay, the sequential pass of :1494-1602.
  int SearchByProjection(FrameGridDev& grid, FrameView& F, const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th, int ORBdist);
  int SearchByProjection(FrameView& F, const float K[4], const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th, int ORBdist);
  static void GuidedSearchDevice(HipContext& ctx, FrameGridDev& grid, const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th,
                                 GuidedCandidates& out);
  static void GuidedSearchHost(const FrameView& F, const float K[4], const ccm_guided_pose& pose, const KeyFramePoints& kf, const uint8_t* alreadyFound, float th,
                               GuidedCandidates& out);
  static int GuidedReplay(FrameView& F, const KeyFramePoints& kf, const GuidedCandidates& c, int ORBdist, bool checkOrientation);
  // the drop-in's form (shim/ORBmatcher_hip.cpp): the gates were the caller's own cv::Mat expressions and the lists its Frame::GetFeaturesInArea returned (CSR over
  // the kf.n slots, empty where a slot did not reach it; kf needs desc and angle only); ONE ccm_hamming_csr launch, then GuidedReplay
  int SearchByProjectionCandidates(FrameView& F, const KeyFramePoints& kf, const int32_t* candOff, const int32_t* candIdx, int ORBdist);
  ORBmatcher(HipContext& ctx, float nnratio = 0.6f, bool checkOri = true) : ctx_(ctx), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
  // ORBmatcher.cpp:1653-1669 (host popcount; the batched form is ccm_hamming_*)
  static int DescriptorDistance(const uint8_t* a, const uint8_t* b);
  // ORBmatcher.cpp:71-148.  Returns nmatches; F.mvpMapPoints[idx] = index of the matched map point.
  int SearchByProjection(FrameView& F, const TrackedMapPoints& mps, float th);
  // same, with the candidate lists and distances produced on the device from the frame's resident grid (no host grid walk)
  int SearchByProjection(FrameGridDev& grid, FrameView& F, const TrackedMapPoints& mps, float th);
  int SearchByProjection(FrameGridDev& grid, FrameView& CurrentFrame, const LastFrameProjections& last, float th);
  // ORBmatcher.cpp:1350-1476.
  int SearchByProjection(FrameView& CurrentFrame, const LastFrameProjections& last, float th);
  // SearchByBoW(kfptr pKF, Frame& F, ...) — ORBmatcher.cpp:178-306.  matchesF[F.N]: KF feature whose map point goes to F[i], or -1
  int SearchByBoW(const KeysView& KF, const KeysView& F, std::vector<int32_t>& matchesF);
  // SearchByBoW(kfptr, kfptr, ...) — ORBmatcher.cpp:565-698.  matches12[KF1.N]: feature of KF2 or -1
  int SearchByBoW_KF(const KeysView& KF1, const KeysView& KF2, std::vector<int32_t>& matches12);
  // SearchForTriangulation — ORBmatcher.cpp:700-852.  F12 row-major 3x3 f32; (ex,ey) epipole in image 2 (:708-714)
  int SearchForTriangulation(const KeysView& KF1, const KeysView& KF2, const float F12[9], float ex, float ey, const float* sigma2_2,
                             const float* scaleFactors2, std::vector<int32_t>& matches12);
  // SearchForInitialization — ORBmatcher.cpp:448-563.  F2 needs the grid bounds; prevMatched (x,y pairs) is updated in place
  int SearchForInitialization(const KeysView& F1, const FrameView& F2, std::vector<float>& vbPrevMatched, std::vector<int32_t>& vnMatches12,
                              int windowSize = 10);
  // The projected window search shared by Fuse (:854-993, chi2 gate), Fuse with Sim3 (:995-1122), SearchByProjection(kfptr,
  // Scw, ...) (:308-446, skips and claims vpMatched) and both directions of SearchBySim3 (:1124-1348, TH_HIGH).  The caller
  // supplies the outcome of the f32 projection / depth / viewing-angle tests (valid, u, v, predicted level) and applies the
  // map mutations (Replace / AddObservation / RemapMapPointMatch) in order from bestIdx, as the reference does after its loop.
  struct ProjectedPoints { int n = 0; const uint8_t* valid = nullptr; const float* u = nullptr; const float* v = nullptr;
                           const int32_t* level = nullptr; const uint8_t* desc = nullptr; const uint8_t* noClaim = nullptr;
                           // optional: the window candidates of every point as the caller's KeyFrame::GetFeaturesInArea returned them (CSR over the n points,
                           // unfiltered, in that order).  A drop-in build has the reference's KeyFrame.cpp, whose grid was filled with the Frame's float
                           // bounds but is read with the keyframe's int-truncated ones (KeyFrame.cpp:54-61, 1167-1171): only its own lookup has that order.
                           const int32_t* candOff = nullptr; const int32_t* candIdx = nullptr; };
  int ProjectedSearch(const FrameView& KF, const float* invLevelSigma2, const ProjectedPoints& P, float th, bool chi2Gate, int distThreshold,
                      int32_t* matched /* nullable in/out [KF.N] */, bool claim, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist);
  int ProjectedSearch(FrameGridDev& grid, const FrameView& KF, const float* invLevelSigma2, const ProjectedPoints& P, float th, bool chi2Gate,
                      int distThreshold, int32_t* matched, bool claim, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist);
  // SearchBySim3's agreement step (:1318-1345) on the two directional results
  static int MutualAgreement(const std::vector<int32_t>& vnMatch1, const std::vector<int32_t>& vnMatch2, std::vector<int32_t>& matches12);
  friend class TriangulationBatch;
  friend class FuseBatch;
 private:
  void deviceWindows(FrameGridDev& grid, const std::vector<float>& u, const std::vector<float>& v, const std::vector<float>& r,
                     const std::vector<int32_t>& minl, const std::vector<int32_t>& maxl, const std::vector<uint8_t>& qdesc,
                     std::vector<int32_t>& off, std::vector<int32_t>& idx, std::vector<uint16_t>& dist);
  // distances of every (query, candidate) slot in one device launch
  void distances(const std::vector<uint8_t>& qdesc, int Q, const uint8_t* tdesc, int T, const std::vector<int32_t>& off,
                 const std::vector<int32_t>& idx, std::vector<uint16_t>& dist);
  HipContext& ctx_;
  float mfNNratio; bool mbCheckOrientation;
};

// The per-keyframe fan-out of LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:277-470): SearchForTriangulation(pKF1, pKF2_j, F12_j, ...) for up to 20
// covisible neighbours j of the new keyframe.  The Hamming work of ALL of them — every (feature of KF1 without a map point, feature of neighbour j in the same
// vocabulary node) pair — goes to the device as ONE ccm_hamming_csr_multi launch with one read-back when the batch is built; resolve(j, ...) then replays the
// reference's sequential rules of the call against neighbour j (epipole distance, epipolar line, first-best claim, rotation histogram) from the stored distances.
// Between two calls of the reference's loop the keyframes GAIN map points (the triangulated matches of the previous neighbour): resolve() takes the map-point flags
// as they are at ITS call and skips what the reference would skip then (:745-749, :763), so the sequence of resolve() calls returns exactly what the sequence
// of SearchForTriangulation calls returns.  Everything the batch needs is copied at build time (the views may go away).
class TriangulationBatch {
 public:
  TriangulationBatch(ORBmatcher& m, const KeysView& KF1, const std::vector<KeysView>& KF2);
  int neighbours() const { return (int)nb_.size(); }
  int64_t candidates() const { return n_cand_; }
  // has1_now / has2_now: nullptr = the flags of the build
  int resolve(int j, const uint8_t* has1_now, const uint8_t* has2_now, const float F12[9], float ex, float ey, const float* sigma2_2, const float* scaleFactors2,
              std::vector<int32_t>& matches12) const;
  const std::vector<KeyPoint>& keys1() const { return keys1_; }
  const std::vector<KeyPoint>& keys2(int j) const { return nb_.at((size_t)j).keys; }
 private:
  struct Nb { std::vector<KeyPoint> keys; std::vector<uint8_t> has; std::vector<int32_t> q_of, off, idx; std::vector<uint16_t> dist; };
  std::vector<KeyPoint> keys1_; std::vector<uint8_t> has1_;
  std::vector<Nb> nb_;
  int64_t n_cand_ = 0;
  bool check_ori_;
};

// The fan-out of LocalMapping::SearchInNeighbors (cslam/src/Mapping.cpp:497-503): matcher.Fuse(pKFi, vpMapPointMatches) for every target keyframe — up to 20 covisible
// neighbours and 5 second neighbours of each — and the projected window searches of the same shape elsewhere (Fuse with Sim3 per loop keyframe, MapMatcher / LoopFinder).
// Fuse never claims features inside its loop (ORBmatcher.cpp:854-993: the best candidate of a point depends on that point alone), and what the calls change between
// each other — a point Replace()d by an earlier call is bad, a point has meanwhile been added to the keyframe — only makes a later call SKIP points (:884-888).  So the
// Hamming work of ALL targets goes to the device as ONE ccm_hamming_csr_multi launch when the batch is built (each target = one search against its own descriptor set),
// and resolve(s, skip_now) replays call s from the stored distances: bit for bit what ProjectedSearch(KF_s, ..., chi2Gate, distThreshold, matched = nullptr) returns
// for the points that are not skipped at that moment.  Everything the batch needs is copied at build time.
class FuseBatch {
 public:
  struct Target { FrameView KF; const float* invLevelSigma2 = nullptr; ORBmatcher::ProjectedPoints P; float th = 3.0f; };
  FuseBatch(ORBmatcher& m, const std::vector<Target>& targets, bool chi2Gate = true, int distThreshold = ORBmatcher::TH_LOW);
  int targets() const { return (int)tg_.size(); }
  int64_t candidates() const { return n_cand_; }
  // skip_now: nullable [P.n of target s]; != 0: the reference's loop would `continue` for this point now (isBad() / IsInKeyFrame(pKF) turned true since the build)
  int resolve(int s, const uint8_t* skip_now, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) const;
 private:
  struct Tg { int n_pts = 0; std::vector<int32_t> q_of, off, idx; std::vector<uint16_t> dist; };
  std::vector<Tg> tg_;
  int64_t n_cand_ = 0;
  int dist_threshold_;
};

// The arithmetic between SearchForTriangulation and `new MapPoint` in LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:353-448): per match the ray-parallax
// gate, the linear triangulation (cv::SVD::compute on a 4x4 f32 matrix), two depth tests, two chi2 reprojection gates and the scale-consistency gate.  The reference's
// loop is sequential across neighbours — a match accepted for neighbour j gives feature idx1 a map point, which changes the matches of neighbour j + 1 — so the batch
// predicts, then answers exactly, as FuseBatch does: at build time the matches of EVERY neighbour (as the flags of that moment give them) go to the device as ONE
// ccm_triangulate_pairs launch; points(j, pairs_now) then takes the matches the caller's real, sequential resolve(j, ...) returned, answers those that are in the table
// (key (j, idx1, idx2)) from it and computes the others on the host with the same tri_pair (csrc/triangulate_math.h compiled by g++).  tri_pair is a pure function of
// the match, so the answers equal the per-neighbour sequence bit for bit.  Everything the batch needs is copied at build time.
struct CamRecord { float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, invfx, invfy; };   // GetRotation / GetTranslation / GetCameraCenter (row-major) and the intrinsics
struct LevelTables { int nlevels = 0; std::vector<float> sigma2_1, sf_1, sigma2_2, sf_2; };   // mvLevelSigma2 / mvScaleFactors of the new keyframe (1) and the neighbours (2)
class NewMapPointBatch {
 public:
  using Pairs = std::vector<std::pair<int32_t, int32_t>>;   // vMatchedIndices: (idx1, idx2)
  struct Neighbour { CamRecord cam; std::vector<KeyPoint> keys; Pairs predicted; };
  struct Epipolar { float F12[9]; float ex, ey; };
  // ctx == nullptr asks for the host evaluator by name (a machine without a device, the CPU tests): the predicted matches are then computed by the host's tri_pair.
  // With a context, a device error throws — there is no fall-back.
  NewMapPointBatch(HipContext* ctx, const CamRecord& cam1, std::vector<KeyPoint> keys1, std::vector<Neighbour> nb, LevelTables lv, float ratioFactor);
  // the prediction taken from a TriangulationBatch: resolve(j, flags of the build, ...) of every neighbour.  octave1 (nullable, [N1]): the octaves of the new
  // keyframe's features where the batch's keys carry none (a batch created through ccmh_tri_batch_create)
  NewMapPointBatch(HipContext& ctx, const TriangulationBatch& tb, const CamRecord& cam1, const std::vector<CamRecord>& cam2, const std::vector<Epipolar>& ep,
                   LevelTables lv, float ratioFactor, const int32_t* octave1 = nullptr);
  int neighbours() const { return (int)nb_.size(); }
  // status[n] / x3d[3n] of the matches of neighbour j as they are NOW (codes of ccm_triangulate_pairs); returns the number accepted
  int points(int j, const Pairs& pairs_now, std::vector<uint8_t>& status, std::vector<float>& x3d);
  int64_t predicted() const { return n_pred_; }
  int64_t hits() const { return n_hit_; }
  int64_t misses() const { return n_miss_; }
 private:
  void build(HipContext* ctx);
  struct Nb { CamRecord cam; std::vector<KeyPoint> keys; Pairs pred; std::vector<uint8_t> status; std::vector<float> x3d; std::vector<int32_t> order; };
  CamRecord cam1_; std::vector<KeyPoint> keys1_;
  std::vector<Nb> nb_;
  LevelTables lv_; float ratio_;
  int64_t n_pred_ = 0, n_hit_ = 0, n_miss_ = 0;
};

// The Sim3 correction of a closed loop's or merged map's keyframes and map points (LoopFinder.cpp:543-613, MapMerger.cpp:289-395) and the write-back of the
// essential-graph optimisers (Optimizer.cpp:1279-1330) as ONE ccm_sim3_correct_map call.  The reference's loop is sequential: keyframe i of the walk corrects
// the points it lists that no earlier keyframe corrected, each point updating its normal and depth at once, and only then takes its new pose.  So a point is
// OWNED by the first keyframe of the walk that lists it (entry not null, not bad, not tagged already), and the camera centre keyframe k shows to that point's
// normal is the corrected one iff rank(k) < rank(owner).  The class flattens the caller's lists into owners and ranks; the graph calls
// (SetWorldPos, the tags, SetPose, UpdateConnections) stay the caller's.  The walk order is the caller's: the reference walks a std::map keyed by pointer.
// ctx == nullptr asks for the host evaluator by name (csrc/sim3_correct_math.h compiled by g++); with a context, a device error throws — there is no fall-back.
class Sim3MapCorrection {
 public:
  struct Points {                                    // every map point the lists name, by id 0 .. n - 1
    std::vector<float> pos, normal, min_dist, max_dist;          // GetWorldPos (3 n), GetNormal (3 n), mfMinDistance, mfMaxDistance
    std::vector<int32_t> obs_off, obs_kf, ref_kf, ref_level;     // non-bad observers in CSR (keyframe indices), reference keyframe and the feature's octave in it
  };
  // loop / merge form.  Keyframes 0 .. n_kf - 1 are the set in walk order (Tiw: 12 floats each), center holds theirs and then those of the observers outside
  // the set.  Keyframe i lists the points list_pt[list_off[i] .. list_off[i + 1]) (GetMapPointMatches; an entry < 0 is a null pointer), list_skip[e] != 0 marks an
  // entry whose point is bad or carries this loop's tag already.
  Sim3MapCorrection(HipContext* ctx, int n_kf, std::vector<float> Tiw, std::vector<float> center, int cur, const float Twc[12], const double Scw[8],
                    const std::vector<int32_t>& list_off, const std::vector<int32_t>& list_pt, const std::vector<uint8_t>& list_skip, Points pts,
                    std::vector<float> scale_factors);
  // essential-graph epilogue: S_non = vScw, S_cor = the optimised Sim3 per keyframe (8 doubles each); pt_kf[p] = index of the keyframe whose pair moves point p
  // (its reference keyframe, or mCorrectedReference_LC), < 0 for a bad point.  Every pose is set before any point moves, so every observer of the set shows its
  // new centre.
  Sim3MapCorrection(HipContext* ctx, int n_kf, std::vector<float> center, std::vector<double> S_non, std::vector<double> S_cor, const std::vector<int32_t>& pt_kf,
                    Points pts, std::vector<float> scale_factors);
  const Points& points() const { return pts_; }                      // pos / normal / bounds after the correction (points nobody owns: as passed in)
  const std::vector<int32_t>& tag() const { return tag_; }           // per point: the keyframe (index in the set) that corrected it, -1 none
  const std::vector<float>& poses() const { return Tiw_new_; }       // 12 n_kf
  const std::vector<float>& centers() const { return center_new_; }  // 3 n_kf
  const std::vector<double>& nonCorrectedSim3() const { return S_non_; }
  const std::vector<double>& correctedSim3() const { return S_cor_; }
 private:
  void run(HipContext* ctx, const float* Tiw, int cur, const float* Twc, const double* Scw, const std::vector<float>& center, int32_t epilogue_rank);
  int n_kf_;
  Points pts_;
  std::vector<float> sf_, Tiw_new_, center_new_;
  std::vector<double> S_non_, S_cor_;
  std::vector<int32_t> tag_;
};

// A finished global BA applied to the map (Optimizer.cpp:803-857, then the walk of RunGBA: Map.cpp:1441-1568, LoopFinder.cpp ~895-1010, MapMerger.cpp ~640-755) as
// ONE ccm_gba_apply_map call.  The reference walks a list from mvpKeyFrameOrigins, pushing every child behind its parent; a child that was no vertex of the BA
// takes (GetPose() * Twc_parent) * mTcwGBA_parent, f32 products that do not re-associate, so it needs its parent's finished pose.  The class
// flattens the graph into that walk order.  A keyframe reached twice (a child in two child sets, or a cycle) would be visited twice by the reference, the second
// time with the pose the first visit set: nothing is evaluated then, and reachedTwice() tells the caller to take the sequential walk.  A point that was no
// landmark moves with its reference keyframe if that keyframe is tagged (a vertex, or reached by the walk as none); a vertex the walk did not reach has a stale
// mTcwBefGBA in the reference: such points are counted (staleReferences()) and left untouched.  SetPose, SetWorldPos, the tags and mbLoopCorrected stay the
// caller's.  ctx == nullptr asks for the host evaluator by name (csrc/gba_apply_math.h compiled by g++); with a context, a device error throws — there is no
// fall-back.
class GbaMapUpdate {
 public:
  struct Graph {                                       // keyframes by id 0 .. n - 1
    std::vector<int32_t> origins;                      // mvpKeyFrameOrigins, in order
    std::vector<int32_t> child_off, child_kf;          // GetChilds() in the order the caller's set iterates, CSR over n + 1
    std::vector<int32_t> kf_cam;                       // camera in the BA problem, -1: no vertex
    std::vector<float> Tcw, Twc;                       // GetPose() / GetPoseInverse(), 12 floats each
  };
  struct Points {                                      // the non-bad points
    std::vector<float> pos;                            // GetWorldPos, 3 n
    std::vector<int32_t> vert, ref_kf;                 // BA landmark or -1; reference keyframe id or -1
  };
  GbaMapUpdate(HipContext* ctx, Graph g, Points p, const std::vector<double>& cam_qt, const std::vector<double>& pt_xyz);
  int reachedTwice() const { return n_twice_; }        // > 0: nothing was evaluated
  int staleReferences() const { return n_stale_; }
  const std::vector<int32_t>& order() const { return order_; }      // keyframe id per walk position
  const std::vector<int32_t>& parents() const { return parent_; }   // walk position of the parent, -1 for an origin
  const std::vector<float>& poses() const { return T_new_; }        // 12 per walk position
  const std::vector<float>& inverses() const { return Twc_new_; }   // 12 per walk position
  const std::vector<float>& positions() const { return pts_.pos; }  // after the update
  const std::vector<uint8_t>& status() const { return status_; }    // per point: 0 untouched, 1 optimised value, 2 moved
 private:
  Points pts_;
  std::vector<int32_t> order_, parent_;
  std::vector<float> T_new_, Twc_new_;
  std::vector<uint8_t> status_;
  int n_twice_ = 0, n_stale_ = 0;
};
// ccm_gba_apply_map's host form after the context through csrc/gba_apply_math.h on the calling thread; -1 where the device entry returns CCM_E_ARG
int gba_apply_map_host(int n_kf, const int32_t* kf_parent, const int32_t* kf_cam, const float* Tcw_old, const float* Twc_old, int n_pt, const float* pos,
                       const int32_t* pt_vert, const int32_t* pt_ref, int n_cam, const double* cam_qt, int n_lm, const double* pt_xyz, float* T_new, float* Twc_new,
                       float* pos_out, uint8_t* pt_status);

// KeyFrame::UpdateConnections (KeyFrame.cpp:629-711) for every keyframe of a corrected set (LoopFinder.cpp:612 / :655, MapMerger.cpp:392 / :487, Map.cpp:614) as ONE
// ccm_covis_update call, with the AddConnection / UpdateBestCovisibles calls (:392-426) the set's keyframes make on each other: per keyframe the final
// mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames and mvOrderedWeights, identical to the sequential walk.  Keyframes 0 .. n_kf - 1 are the
// set in walk order, the others observers outside it; order_key (distinct, one per keyframe) stands for the pointer order of the reference's std::map and sort.
// The lists are those of Sim3MapCorrection: keyframe i lists list_pt[list_off[i] .. list_off[i + 1]) (< 0: null), list_skip[e] != 0: a bad point; point p is
// observed by obs_kf[obs_off[p] .. obs_off[p + 1]).  Keyframes outside the set keep state only the caller knows: outsideCalls() are the AddConnection calls they
// receive, in the reference's order (walk order, then order_key).  A keyframe flagged EMPTY returns early in the reference and keeps its previous state: its rows
// hold what the set's calls build on an empty state, i.e. the AddConnection calls to apply to the state the caller has.  The spanning tree stays the caller's.
// ctx == nullptr asks for the host evaluator by name (csrc/covis_math.h compiled by g++); with a context, a device error throws — there is no fall-back.
class CovisibilityBatch {
 public:
  struct AddCall { int32_t target, source, weight; };
  CovisibilityBatch(HipContext* ctx, int n_kf, std::vector<int32_t> order_key, const std::vector<int32_t>& list_off, const std::vector<int32_t>& list_pt,
                    const std::vector<uint8_t>& list_skip, const std::vector<int32_t>& obs_off, const std::vector<int32_t>& obs_kf, int th = 15);
  int size() const { return n_kf_; }
  int flags(int i) const { return flags_[i]; }                                   // COVIS_EMPTY 1, COVIS_FALLBACK 2, COVIS_CHANGED 4
  std::map<int32_t, int> GetConnectedKeyFrameWeights(int i) const;               // mConnectedKeyFrameWeights, keyed by keyframe index
  std::vector<int32_t> GetVectorCovisibleKeyFrames(int i) const { return std::vector<int32_t>(ord_kf_.begin() + ord_off_[i], ord_kf_.begin() + ord_off_[i + 1]); }
  std::vector<int32_t> GetOrderedWeights(int i) const { return std::vector<int32_t>(ord_w_.begin() + ord_off_[i], ord_w_.begin() + ord_off_[i + 1]); }
  std::vector<int32_t> GetBestCovisibilityKeyFrames(int i, int N) const;         // KeyFrame.cpp:443-451
  std::vector<int32_t> GetCovisiblesByWeight(int i, int w) const;                // KeyFrame.cpp:453-468 (empty when every weight is >= w, as there)
  const std::vector<AddCall>& outsideCalls() const { return outside_; }
  // the flat tables: own counts, final weights (both by ascending keyframe index), ordered lists
  const std::vector<int32_t>& rowOff() const { return row_off_; }
  const std::vector<int32_t>& rowKf() const { return col_; }
  const std::vector<int32_t>& rowCount() const { return count_; }
  const std::vector<int32_t>& weightOff() const { return fw_off_; }
  const std::vector<int32_t>& weightKf() const { return fw_col_; }
  const std::vector<int32_t>& weight() const { return fw_w_; }
  const std::vector<int32_t>& orderedOff() const { return ord_off_; }
  const std::vector<int32_t>& orderedKf() const { return ord_kf_; }
  const std::vector<int32_t>& orderedWeight() const { return ord_w_; }
  const std::vector<int32_t>& allFlags() const { return flags_; }
 private:
  int n_kf_;
  std::vector<int32_t> key_, flags_, row_off_, col_, count_, fw_off_, fw_col_, fw_w_, ord_off_, ord_kf_, ord_w_;
  std::vector<AddCall> outside_;
};
// ccm_covis_update's arguments after the context through csrc/covis_math.h on the calling thread; -1 where the device entry returns CCM_E_ARG
int covis_update_host(int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt,
                      const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col,
                      int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags, int32_t* needed);

// LocalMapping::KeyFrameCullingV3's walk over the covisible keyframes of the picked keyframe (Mapping.cpp:804-862) as ONE ccm_kfcull_walk call: the verdict of every
// candidate, identical to the sequential walk in which culling a keyframe erases its observations, lowers Observations() of its points and turns points with <= 2
// observations bad before the next candidate is looked at.  The candidates are cand_flags.size() keyframes 0 .. in walk order (flag 1 SKIP: mId.first
// 0 or 1 or in mlpRecentAddedKFs; 2 NOT_ERASE: mbNotErase), n_all - n_cand other observers follow.  Candidate k lists list_pt[list_off[k] .. list_off[k + 1]) (< 0:
// null) with list_level = mvKeysUn[slot].octave; ONE record per distinct point: pt_nobs = Observations(), pt_bad = isBad(), its observers obs_kf[obs_off[p] ..
// obs_off[p + 1]) with the octave of the point's feature there and the observer's isBad().  thres = params::mapping::mfRedundancyThres.  The pick (GetRandKfPtr,
// mspKFsCheckedForCulling) and the calls `pKF->SetBadFlag(); ++mCulledKfs;` stay the caller's: for every keyframe of culled(), in that order.
// ctx == nullptr asks for the host evaluator by name (csrc/kfcull_math.h compiled by g++); with a context, a device error throws — there is no fall-back.
class KeyFrameCullingBatch {
 public:
  KeyFrameCullingBatch(HipContext* ctx, int n_all, const std::vector<uint8_t>& cand_flags, const std::vector<int32_t>& list_off, const std::vector<int32_t>& list_pt,
                       const std::vector<uint8_t>& list_level, const std::vector<int32_t>& pt_nobs, const std::vector<uint8_t>& pt_bad, const std::vector<int32_t>& obs_off,
                       const std::vector<int32_t>& obs_kf, const std::vector<uint8_t>& obs_level, const std::vector<uint8_t>& obs_bad, double thres, int n_levels,
                       int th_obs = 3);
  int size() const { return (int)verdict_.size(); }
  int verdict(int k) const { return verdict_[k]; }          // 0 kept, 1 culled, 2 skipped, 3 redundant but mbNotErase
  std::vector<int32_t> culled() const;                      // the candidates SetBadFlag is called on (verdicts 1 and 3), in walk order
  std::vector<int32_t> pointsGone() const;                  // the points the walk turned bad (not those that were bad before), ascending
  int reevaluated() const { return n_reeval_; }             // candidates counted again because an earlier erasure could reach one of their points
  const std::vector<int32_t>& nMPs() const { return n_mps_; }              // as counted at the candidate's own turn
  const std::vector<int32_t>& nRedundant() const { return n_red_; }
  const std::vector<uint8_t>& gone() const { return gone_; }               // isBad() of every point after the walk
  const std::vector<int32_t>& observations() const { return n_obs_; }      // Observations() of every point after the walk
 private:
  std::vector<uint8_t> verdict_, gone_, bad_before_;
  std::vector<int32_t> n_mps_, n_red_, n_obs_;
  int32_t n_reeval_ = 0;
};
// ccm_kfcull_walk's arguments after the context through csrc/kfcull_math.h on the calling thread; -1 where the device entry returns CCM_E_ARG
int kfcull_walk_host(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                     const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad,
                     int th_obs, double thres, int n_levels, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone, int32_t* pt_nobs_out, int32_t* n_reeval);
// the same walk on std::map observations copied per checked slot, as the reference's containers make it: a cost model for scripts/kfcull_profile.py; verdicts only
int kfcull_walk_mapcopy_model(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                              const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level,
                              const uint8_t* obs_bad, int th_obs, double thres, int n_levels, uint8_t* verdict);

// ---------------------------------------------------------------------------------------------------
// ORBVocabulary::transform (DBoW2 TemplatedVocabulary<FORB>, thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1260) as
// KeyFrame::ComputeBoW / Frame::ComputeBoW call it (levelsup = 4), and MapPoint::ComputeDistinctiveDescriptors
// (MapPoint.cpp:929-994) batched over many map points — SURVEY §8f rows 1 and 3.  The vocabulary keeps a host copy of its flat tree: KeyFrameStore::ingest
//  transforms the keyframes of a whole message on the device, and on that copy for the host-only store.
// ---------------------------------------------------------------------------------------------------
struct BowVector { std::vector<int32_t> word; std::vector<double> value; };                       // ascending word ids, L1-normalised
struct FeatureVector { std::vector<int32_t> node, off, idx; };                                     // ascending nodes, CSR, features in index order
class ORBVocabulary {
 public:
  // flat tree, see ccm_vocab_create (include/ccm_hip.h)
  ORBVocabulary(HipContext& ctx, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc,
                const int32_t* word_id, const double* weight);
  // ctx == nullptr: the host copy alone, for KeyFrameStore::ingest on the host-only store (transform then throws)
  ORBVocabulary(HipContext* ctx, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id,
                const double* weight);
  ~ORBVocabulary();
  ORBVocabulary(const ORBVocabulary&) = delete;
  ORBVocabulary& operator=(const ORBVocabulary&) = delete;
  void transform(const uint8_t* descriptors, int N, BowVector& v, FeatureVector& fv, int levelsup = 4) const;
  const ccm_vocab* handle() const { return voc_; }
  // the host copy of the flat tree, in the arguments' form
  int n_nodes() const { return n_nodes_; }
  int L() const { return L_; }
  const std::vector<int32_t>& child_off() const { return child_off_; }
  const std::vector<int32_t>& child_id() const { return child_id_; }
  const std::vector<uint8_t>& node_desc() const { return node_desc_; }
  const std::vector<int32_t>& word_id() const { return word_id_; }
  const std::vector<double>& weight() const { return weight_; }
 private:
  void keep(int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id, const double* weight);
  ccm_vocab* voc_ = nullptr;
  int n_nodes_ = 0, L_ = 0;
  std::vector<int32_t> child_off_, child_id_, word_id_;
  std::vector<uint8_t> node_desc_;
  std::vector<double> weight_;
};
// best descriptor per map point: desc rows off[p]..off[p+1] are the observations of point p; returns local indices
std::vector<int32_t> ComputeDistinctiveDescriptors(HipContext& ctx, const uint8_t* desc, const std::vector<int32_t>& off);

// ---------------------------------------------------------------------------------------------------
// KeyFrameDatabase — cslam/include/cslam/Database.h, cslam/src/Database.cpp.  Keyframes are keys (int64) with a client id; the
// map objects' accessors become arguments: map_keys = GetMapptr()->GetMmpKeyFrames() (nullptr: every keyframe), connected =
// GetConnectedKeyFrames(), ass_clients = bit c for every c in pMap->msuAssClients, neighbours(key, out) = GetBestCovisibilityKeyFrames(10).
// Phase 1 on the device (ccm_kfdb_query), phase 2 in kfdb_resolve.h.  One database may be shared by threads, each with its own context.
// ---------------------------------------------------------------------------------------------------
class KeyFrameDatabase {
 public:
  using Neighbours = std::function<void(int64_t, std::vector<int64_t>&)>;
  KeyFrameDatabase(HipContext& ctx, int n_words, int log_capacity = 0);
  explicit KeyFrameDatabase(ccm_kfdb* borrowed);   // a handle owned elsewhere (not destroyed here)
  ~KeyFrameDatabase();
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
  void add(HipContext& ctx, int64_t key, int32_t client, const BowVector& v);
  void erase(HipContext& ctx, int64_t key);
  void clear(HipContext& ctx);
  std::vector<int64_t> DetectLoopCandidates(HipContext& ctx, int64_t key, const BowVector& v, float minScore, const std::vector<int64_t>* map_keys,
                                            const std::vector<int64_t>& connected, const Neighbours& neighbours);
  std::vector<int64_t> DetectMapMatchCandidates(HipContext& ctx, const BowVector& v, float minScore, uint64_t ass_clients, const Neighbours& neighbours);
  std::vector<int64_t> DetectRelocalizationCandidates(HipContext& ctx, const BowVector& v, const Neighbours& neighbours);
  ccm_kfdb* handle() const { return db_; }
 private:
  std::vector<int64_t> detect(HipContext& ctx, const BowVector& v, float minScore, const ccm_kfdb_filter* f, const Neighbours& neighbours);
  ccm_kfdb* db_ = nullptr;
  bool owned_ = true;
};

// ---------------------------------------------------------------------------------------------------
// What the evaluators of the two RANSAC batches below share: the CSR over the candidates a pass can evaluate (N >= the sample size S; the others are never
// evaluated, which the schedules check) and the map from a pass's candidates to its rows.
// ---------------------------------------------------------------------------------------------------
struct RansacCsr {
  std::vector<int32_t> pt_off{0}, remap;   // remap: candidate -> CSR row, -1 without one
  std::vector<int32_t> cand_buf;           // the rows of the last pass's hypotheses
  bool append(int N, int S);               // the next candidate; true: it has a row, and the caller appends its per-point arrays
  int K() const { return (int)pt_off.size() - 1; }
  size_t rows(const std::vector<int32_t>& hyp_cand);   // fills cand_buf; returns the pass's mask words
};

// ---------------------------------------------------------------------------------------------------
// Sim3RansacBatch — the vpSim3Solvers loop of LoopFinder::ComputeSim3 (cslam/src/LoopFinder.cpp:288-346) and MapMatcher::ComputeSim3: one
// Sim3Solver per candidate (the correspondences its constructor gathers, Sim3Solver.cpp:5-92), iterate(mSolverIterations) round-robin until a
// call returns a Sim3.  next() returns that event (candidate, R, t, s = GetEstimated*, vbInliers in the candidate's mN1 numbering) and the
// caller runs SearchBySim3 + OptimizeSim3; on rejection it calls next() again, which goes on where the reference's loop goes on.  false: every
// candidate is discarded.  Hypotheses are evaluated in passes on the device (ccm_sim3_ransac_eval, schedule in sim3_schedule.h); the draws come
// from ::rand() through the calling thread's FIFO (or a supplied source), so the events are the sequential reference's.
// ---------------------------------------------------------------------------------------------------
struct Sim3Candidate {
  int n1 = 0;                       // mN1 = vpMatched12.size()
  std::vector<int32_t> indices1;    // mvnIndices1 (size N)
  std::vector<float> X3Dc1, X3Dc2;  // mvX3Dc1 / mvX3Dc2, 3 per correspondence
  std::vector<uint32_t> max_err1, max_err2;   // mvnMaxError1 / mvnMaxError2
  float K1[4] = {0, 0, 0, 0}, K2[4] = {0, 0, 0, 0};   // fx fy cx cy of pKF1->mK / pKF2->mK
};

class Sim3RansacBatch {
 public:
  struct Eval : RansacCsr {   // the device CSR over the candidates with N >= 3
    HipContext* ctx = nullptr;
    int fix_scale = 0;
    std::vector<float> X1, X2, K1, K2;
    std::vector<uint32_t> t1, t2;
    void add(int N, const float* x1, const float* x2, const float* k1, const float* k2, const uint32_t* thr1, const uint32_t* thr2);
    void operator()(const std::vector<int32_t>& hyp_cand, const std::vector<int32_t>& hyp_idx, std::vector<int32_t>& n_inl, std::vector<float>& rts,
                    std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask);
  };
  Sim3RansacBatch(HipContext& ctx, std::vector<Sim3Candidate> cands, const ccm_sim3::Params& p = ccm_sim3::Params(), bool fix_scale = false,
                  ccm_sim3::DrawSource src = ccm_sim3::rand_source());
  bool next(int& cand, float R[9], float t[3], float& s, std::vector<bool>& vbInliers, int& nInliers);
  const ccm_sim3::Schedule<Eval>& schedule() const { return sched_; }
 private:
  std::vector<Sim3Candidate> cands_;
  Eval eval_;
  ccm_sim3::Schedule<Eval> sched_;
};

// ---------------------------------------------------------------------------------------------------
// PnPRansacBatch — one cslam::PnPsolver per relocalisation candidate (the correspondences its constructor gathers, PnPSolver.cpp:57-100) and the round-robin
// `for each candidate not discarded: iterate(solver_iterations)` of a Relocalization().  next() returns the next call that returns a pose: the candidate, Tcw
// (4x4 f32, row-major: mRefinedTcw after a successful Refine, else mBestTcw of a call that ran out of iterations), vbInliers in the frame's keypoint numbering and
// nInliers; the caller runs PoseOptimizationClient and, on rejection, calls next() again, which goes on where the reference's loop goes on.  false: every candidate
// is discarded.  Hypotheses are evaluated in passes (ccm_pnp_ransac_eval, schedule in pnp_schedule.h; ctx == nullptr: pnp_math.h on the calling thread); the draws
// come from ::rand() through the calling thread's FIFO (the one Sim3RansacBatch uses) or a supplied source, so the events are the sequential reference's.
// ---------------------------------------------------------------------------------------------------
struct PnPCandidate : ccm_pnp::Candidate {
  int n_matches = 0;                        // vpMapPointMatches.size(): the length of vbInliers
  std::vector<int32_t> keypoint_indices;    // mvKeyPointIndices (size N)
};

class PnPRansacBatch {
 public:
  struct Eval : RansacCsr {   // the CSR over the candidates with N >= 4
    HipContext* ctx = nullptr;            // nullptr: the host evaluator
    std::vector<float> P3Dw, P2D, max_err;
    std::vector<double> cam;
    void operator()(const std::vector<int32_t>& hyp_cand, const std::vector<int32_t>& hyp_idx, std::vector<int32_t>& n_inl, std::vector<double>& Rt,
                    std::vector<int32_t>& mask_off, std::vector<uint32_t>& mask);
  };
  struct Pose {
    int cand = -1, nInliers = 0;
    bool refined = false, bNoMore = false;
    float Tcw[16];
    std::vector<bool> vbInliers;
  };
  PnPRansacBatch(HipContext* ctx, std::vector<PnPCandidate> cands, const ccm_pnp::Params& p = ccm_pnp::Params(), ccm_pnp::DrawSource src = ccm_pnp::rand_source());
  bool next(Pose& out);
  // one iterate(nIterations) of candidate c (the drop-in's call): true when it returns a pose; bNoMore as the reference sets it
  bool iterate(int c, int nIterations, bool& bNoMore, Pose& out);
  const ccm_pnp::Schedule<Eval>& schedule() const { return sched_; }
 private:
  void fill(const ccm_pnp::Event& ev, Pose& out) const;
  std::vector<int> n_matches_;
  std::vector<std::vector<int32_t>> kp_idx_;
  Eval eval_;
  ccm_pnp::Schedule<Eval> sched_;
};

// ---------------------------------------------------------------------------------------------------
// Initializer — cslam/include/cslam/Initializer.h: the arithmetic of Initialize() between the set drawing and ReconstructF / ReconstructH
// (FindHomography / FindFundamental, Initializer.cpp:120-219) and CheckRT (:794-903) for all motion hypotheses of an attempt at once.
// DecomposeE, the Faugeras decomposition and the accept / reject logic stay with the caller.
// ---------------------------------------------------------------------------------------------------
class TwoViewInitializer {
 public:
  typedef std::vector<int32_t> Sets;   // mvSets, 8 match indices per iteration
  struct Models {                      // what FindHomography / FindFundamental return; a model without a winner is all zeros
    float SH = 0, SF = 0, RH = 0;      // RH = SH / (SH + SF)
    float H21[9] = {0}, F21[9] = {0};
    int bestH = -1, bestF = -1;        // the winning iteration, -1: no score above 0
    std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;
  };
  struct Motion { float R[9]; float t[3]; };
  struct Reconstruction {              // what one CheckRT returns
    int nGood = 0; float parallax = 0;
    std::vector<float> vP3D;           // 3 per keypoint of frame 1 (zeros where the reference leaves Point3f())
    std::vector<bool> vbGood;          // per keypoint of frame 1
    std::vector<uint8_t> status;       // per match: the first gate (include/ccm_hip.h, ccm_twoview_check_rt)
  };
  // ctx == nullptr: every evaluation runs twoview_math.h on the calling thread.  K: 3x3 row-major; keys1: mvKeysUn of the reference frame, x y pairs.
  TwoViewInitializer(HipContext* ctx, const float K[9], std::vector<float> keys1, float sigma);
  // the set-drawing loop of Initializer.cpp:73-93 on the caller's rand (DUtils::Random::RandomInt on each value)
  static Sets DrawSets(int N, int iterations, const std::function<int()>& rand);
  // keys2: mvKeysUn of the current frame; vMatches12: per keypoint of frame 1 the index in frame 2 or -1.  Throws infrastructure_ex on fewer than 8 matches,
  // an index out of range or a bad set, and on a device error.
  Models FindModels(std::vector<float> keys2, const std::vector<int>& vMatches12, const Sets& sets);
  // CheckRT of every hypothesis (1..8) with the matches of the last FindModels
  std::vector<Reconstruction> CheckRTBatch(const std::vector<Motion>& hyp, const std::vector<bool>& vbMatchesInliers, float th2);
  int matches() const { return (int)first_.size(); }
  int keys1() const { return (int)(keys1_.size() / 2); }
 private:
  HipContext* ctx_;
  float K_[9], sigma_;
  std::vector<float> keys1_, keys2_, xy1_, xy2_;   // xy: in match order
  std::vector<int32_t> first_;                     // mvMatches12[i].first
};

// ---------------------------------------------------------------------------------------------------
// KeyFrameStore — the keyframes' static data of the two Fuse stages, resident on the device (include/ccm_hip.h ccm_kfstore_*), and a host shadow
// per live key: the record, mvKeysUn, the octaves, the descriptors and the grid.  The shadow's grid is the caller's when one is supplied, otherwise it is built
// here by KeyFrame::AssignFeaturesToGrid / PosInGrid (csrc/kfstore_math.h, the lines the device's grid kernel runs): the host evaluator of that kernel.
// A server adds a keyframe after the message constructor's AssignFeaturesToGrid with NO grid (mGrid is protected and need not be read: the rule reads what the
// keyframe keeps); a client's Frame-born keyframe needs the Frame's grid supplied.  erase where the map erases the keyframe.
// ctx == nullptr at construction asks for the host-only store by name.  One store is shared by all threads: add / erase / clear are serialised, shadows are
// handed out as shared_ptr, so a batch that holds them outlives an erase.
// ---------------------------------------------------------------------------------------------------
struct KfShadow {
  float rec[10];
  int n = 0, n_in = 0;
  std::vector<float> xy;
  std::vector<uint8_t> oct, desc;
  std::vector<int32_t> cell_off;    // 3601
  std::vector<uint16_t> cell_idx;   // n_in
  // set_featvec: mFeatVec as the device slot holds it, and mvKeysUn[i].angle (the shadow's alone: the rotation histogram is evaluated on the host)
  bool has_fv = false;
  std::vector<int32_t> fv_node, fv_off;
  std::vector<uint16_t> fv_idx;
  std::vector<float> angle;         // n
};

class KeyFrameStore {
 public:
  KeyFrameStore(HipContext* ctx, int max_kf, int max_feat);
  ~KeyFrameStore();
  KeyFrameStore(const KeyFrameStore&) = delete;
  KeyFrameStore& operator=(const KeyFrameStore&) = delete;
  // ccm_kfstore_add's arguments and refusals: 0, CCM_E_ARG or CCM_E_STATE, the store untouched by a refusal; a device error throws.  ctx: the calling thread's
  // (ignored by the host-only store).
  int add(HipContext* ctx, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
          const uint8_t* feat_desc, const int32_t* cell_off = nullptr, const int32_t* cell_idx = nullptr);
  // ccm_kfstore_set_featvec's arguments and refusals (0 or CCM_E_ARG, the store untouched by a refusal; a device error throws) and angle[n] = mvKeysUn[i].angle
  // (nullable: zeros).  A second call for the key replaces the first.  Right after add in the message constructor: ComputeBoW() has run by then.
  int set_featvec(HipContext* ctx, int64_t key, const FeatureVectorView& fv, const float* angle);
  // The keyframes of a message in ONE call (ccm_kfstore_ingest): add without a grid, ComputeBoW and set_featvec for all of them.
  // angle: mvKeysUn[i].angle of all features (nullable: zeros), the shadows' alone.  bow[m] / fv[m] are the keyframe's mBowVec / mFeatVec.  A shadow after ingest
  // equals the shadow after add + set_featvec.  The host-only store evaluates csrc/kfingest_math.h on the vocabulary's host copy.  ccm_kfstore_ingest's refusals.
  int ingest(HipContext* ctx, const ORBVocabulary& voc, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
             const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, std::vector<BowVector>& bow, std::vector<FeatureVector>& fv, int levelsup = 4);
  // the same on flat arrays (ccm_kfstore_ingest's outputs); dvoc: the device vocabulary (device store), tree: the flat tree on the host (host-only store)
  int ingest_flat(HipContext* ctx, const ccm_vocab* dvoc, const ::kfi_tree* tree, int levelsup, int M, const int64_t* keys, const float* kf_rec,
                  const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, int32_t* bow_n,
                  int32_t* bow_word, double* bow_value, int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node);
  void erase(HipContext* ctx, int64_t key);
  void clear(HipContext* ctx);
  int live() const;
  int free_slots() const;
  bool host_only() const { return h_ == nullptr; }
  ccm_kfstore* handle() const { return h_; }
  std::shared_ptr<const KfShadow> shadow(int64_t key) const;   // null: not live
  // the grid of one key: the device's (ccm_kfstore_get) with a context, the shadow's without; false: the key is not live
  bool get(HipContext* ctx, int64_t key, int* n, int* n_in, int32_t* cell_off, int32_t* cell_idx) const;
 private:
  bool keys_ok(int M, const int64_t* keys) const;
  ccm_kfstore* h_ = nullptr;
  int max_kf_ = 0, max_feat_ = 0;
  mutable std::shared_mutex mu_;
  std::unordered_map<int64_t, std::shared_ptr<const KfShadow>> live_;
};

// ---------------------------------------------------------------------------------------------------
// What a Fuse batch (SearchAndFuseBatch, SearchInNeighborsBatch below) keeps for its resolves: a copy of the keyframes (poses as Rcw, tcw, Ow; cell_idx in 16 bits)
// and points it was evaluated on, the call's scalars and level tables, and the pair evaluator on them (csrc/fuse_math.h).  Not part of the API.
// ---------------------------------------------------------------------------------------------------
struct FuseScene {
  int nlevels = 0; float logsf = 0, th = 0;
  std::vector<float> rec, pose, kxy, sf, isig, pos, normal, dmin, dmax;   // isig empty: the Sim3 form, which has no chi-square gate
  std::vector<int32_t> feat_off, cell_off;
  std::vector<uint16_t> cell_idx;
  std::vector<uint8_t> koct, kdesc, pdesc;
  std::vector<std::shared_ptr<const KfShadow>> shadow;   // a batch built on a KeyFrameStore: the keyframes' arrays are the store's shadows, shared, not copied
  // kfs, pts: a batch's KeyFrames and Points, already validated; pose15: 15 floats per keyframe; inv_level_sigma2 == nullptr: the Sim3 form
  template <class KFs, class Pts>
  void copy(const KFs& kfs, const float* pose15, const Pts& pts, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th);
  // the packed answer of keyframe k and a point given by its data and descriptor
  uint32_t eval(int k, const float* P3, const float* Pn, float dmin, float dmax, const uint8_t* desc) const;
  // the same for keyframes of a store: shared ownership of their shadows, the points and the call's values copied
  template <class Pts>
  void hold(std::vector<std::shared_ptr<const KfShadow>> kfs, const float* pose15, const Pts& pts, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
            float logScaleFactor, float th);
};

// ---------------------------------------------------------------------------------------------------
// SearchAndFuse — LoopFinder.cpp:709-734, MapMerger.cpp:574-598: matcher.Fuse(pKF, Scw, vpLoopMapPoints, 4, vpReplacePoints) for every keyframe of CorrectedSim3,
// each followed by the Replace loop.  The constructor evaluates every (keyframe, point) pair in ONE ccm_fuse_sim3_eval call (arguments as there) and
// copies what resolve needs; resolve(k, ...) then returns what the k-th Fuse call returns, whatever the calls before it did to the map: a table entry depends on the
// keyframe's static data, Scw_k and the point's position, normal, distance bounds and descriptor, and of these Replace / AddObservation change the descriptor
// alone, so a point whose current descriptor differs from the snapshot is evaluated again on the calling thread (fuse_math.h) and every other answer is read.
// ctx == nullptr asks for the host evaluator by name (csrc/fuse_math.h compiled by g++); with a context, a device error throws — there is no fall-back.
// GetMapPoint(bestIdx), vpReplacePoint, AddObservation / AddMapPoint and the Replace loop stay the caller's.
// ---------------------------------------------------------------------------------------------------
class SearchAndFuseBatch {
 public:
  struct KeyFrames {   // K keyframes, flat (include/ccm_hip.h, ccm_fuse_sim3_eval)
    int K = 0; const float* rec = nullptr; const int32_t* feat_off = nullptr; const float* feat_xy = nullptr; const uint8_t* feat_octave = nullptr;
    const uint8_t* feat_desc = nullptr; const int32_t* cell_off = nullptr; const int32_t* cell_idx = nullptr; const float* Scw = nullptr;
  };
  struct Points { int P = 0; const float* pos = nullptr; const float* normal = nullptr; const float* min_dist = nullptr; const float* max_dist = nullptr;
                  const uint8_t* desc = nullptr; };
  SearchAndFuseBatch(HipContext* ctx, const KeyFrames& kfs, const Points& pts, int nlevels, const float* scale_factors, float logScaleFactor, float th);
  // The same on keyframes of a store: keyframe k of the batch is the live key keys[k] (a key may repeat), Scw + 12 k its Sim3.  ONE ccm_fuse_sim3_eval_resident
  // call with ctx, or the host evaluation when the store is host-only.  The batch shares the shadows of its keyframes: an erase during its life leaves it valid.
  SearchAndFuseBatch(KeyFrameStore& store, HipContext* ctx, int K, const int64_t* keys, const float* Scw, const Points& pts, int nlevels, const float* scale_factors,
                     float logScaleFactor, float th);
  // The k-th Fuse call.  skip_now[i] != 0: the reference would `continue` now (pMP->isBad() || spAlreadyFound.count(pMP)); desc_now (nullable): the points' CURRENT
  // descriptors.  bestIdx[i] = the feature point i is fused with (-1: none), bestDist[i] its distance; returns nFused.
  int resolve(int k, const uint8_t* skip_now, const uint8_t* desc_now, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist);
  int keyframes() const { return K_; }
  int points() const { return P_; }
  const std::vector<uint32_t>& table() const { return table_; }   // k-major, as evaluated at construction
  const std::vector<int32_t>& nValid() const { return n_valid_; }
  const std::vector<int32_t>& nHit() const { return n_hit_; }
  long long n_reeval() const { return n_reeval_; }                 // pairs evaluated again by resolve because the descriptor had changed
 private:
  // both constructors: the keyframes are *flat, or keys of *store (the other is null)
  void init(const KeyFrames* flat, KeyFrameStore* store, const int64_t* keys, const float* Scw, HipContext* ctx, const Points& pts, int nlevels,
            const float* scale_factors, float logScaleFactor, float th);
  int K_ = 0, P_ = 0;
  FuseScene scene_;
  std::vector<int32_t> n_valid_, n_hit_;
  std::vector<uint32_t> table_;
  long long n_reeval_ = 0;
};
// ccm_fuse_sim3_eval's arguments after the context through csrc/fuse_math.h on the calling thread; -1 where the device entry returns CCM_E_ARG.
// n_cand (nullable, K P): the size of vIndices of every pair that reached the window (0 otherwise), for scripts/fuse_sim3_profile.py.
int fuse_sim3_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                        const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P,
                        const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid,
                        int32_t* n_hit, float* uv, int32_t* n_cand);

// ---------------------------------------------------------------------------------------------------
// SearchInNeighbors — Mapping.cpp:471-547: matcher.Fuse(pKFi, vpMapPointMatches) for every fuse target (:495-503), then matcher.Fuse(mpCurrentKeyFrame,
// vpFuseCandidates) with the targets' points (:510-529).  The constructor evaluates BOTH directions in ONE ccm_fuse_pose_eval call: call c < n_calls
// is the job (keyframe target[c], the current keyframe's points = the first n_current of pts), the last job is (keyframe `current`, the PREDICTED fuse candidates =
// the rest of pts: the union of the targets' points at build time in the reference's order).  Everything a resolve may need later is copied.
// resolve(c, ...) returns what the c-th Fuse call of the first loop returns, resolve_current(...) what the Fuse on the current keyframe returns, whatever the
// calls before did to the map: a pair that reached the window and whose current descriptor differs from the snapshot is evaluated again on the calling thread
// (fuse_math.h); a candidate the prediction missed (slot -1) is evaluated from what the caller passes for it.  ctx == nullptr asks for the host evaluator by
// name; with a context, a device error throws — there is no fall-back.  The map mutations stay the caller's.
// ---------------------------------------------------------------------------------------------------
class SearchInNeighborsBatch {
 public:
  struct KeyFrames {   // K keyframes, flat (include/ccm_hip.h, ccm_fuse_pose_eval); pose: Rcw (9), tcw (3), Ow (3) per keyframe
    int K = 0; const float* rec = nullptr; const int32_t* feat_off = nullptr; const float* feat_xy = nullptr; const uint8_t* feat_octave = nullptr;
    const uint8_t* feat_desc = nullptr; const int32_t* cell_off = nullptr; const int32_t* cell_idx = nullptr; const float* pose = nullptr;
  };
  struct Points { int P = 0; const float* pos = nullptr; const float* normal = nullptr; const float* min_dist = nullptr; const float* max_dist = nullptr;
                  const uint8_t* desc = nullptr; };
  // current < 0: no second direction (pts holds the current keyframe's points alone)
  SearchInNeighborsBatch(HipContext* ctx, const KeyFrames& kfs, int n_calls, const int32_t* target, int current, const Points& pts, int n_current, int nlevels,
                         const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th);
  // The same on keyframes of a store: keyframe k is the live key keys[k], pose + 15 k its pose; target and current index keys.  ONE ccm_fuse_pose_eval_resident
  // call with ctx, or the host evaluation when the store is host-only.  The batch shares the shadows of its keyframes.
  SearchInNeighborsBatch(KeyFrameStore& store, HipContext* ctx, int K, const int64_t* keys, const float* pose, int n_calls, const int32_t* target, int current,
                         const Points& pts, int n_current, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th);
  // The c-th Fuse call of the first loop.  skip_now[i] != 0: the reference would `continue` now (!pMP || isBad() || IsInKeyFrame(pKF) || mbDoNotReplace);
  // desc_now (nullable): the current keyframe's points' CURRENT descriptors.  bestIdx[i] = the feature point i is fused with (-1: none), bestDist[i] as the
  // reference leaves it (256: no candidate); returns nFused.
  int resolve(int c, const uint8_t* skip_now, const uint8_t* desc_now, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist);
  // Fuse(mpCurrentKeyFrame, vpFuseCandidates) for the n candidates the caller has NOW: slot[i] = candidate i's index among the predicted ones, or -1; skip_now and
  // desc_now (nullable) per candidate; fresh (n entries, read where slot[i] == -1 and the candidate is not skipped): position, normal, bounds, descriptor.
  int resolve_current(int n, const int32_t* slot, const uint8_t* skip_now, const uint8_t* desc_now, const Points& fresh, std::vector<int32_t>& bestIdx,
                      std::vector<int32_t>& bestDist);
  int calls() const { return C_; }
  int currentPoints() const { return P1_; }
  int predicted() const { return P2_; }
  const std::vector<uint32_t>& table() const { return table_; }   // call-major, then the predicted candidates; as evaluated at construction
  const std::vector<int32_t>& nValid() const { return n_valid_; } // per job
  const std::vector<int32_t>& nHit() const { return n_hit_; }
  long long n_reeval() const { return n_reeval_; }                 // pairs evaluated again because the descriptor had changed
  long long n_unpredicted() const { return n_unpredicted_; }       // candidates evaluated from fresh data
 private:
  // both constructors: the keyframes are *flat, or keys of *store (the other is null)
  void init(const KeyFrames* flat, KeyFrameStore* store, const int64_t* keys, const float* pose, HipContext* ctx, const int32_t* target, const Points& pts, int nlevels,
            const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th);
  int K_ = 0, C_ = 0, cur_ = -1, P1_ = 0, P2_ = 0;
  FuseScene scene_;
  std::vector<int32_t> target_, n_valid_, n_hit_;
  std::vector<uint32_t> table_;
  long long n_reeval_ = 0, n_unpredicted_ = 0;
};
// ccm_fuse_pose_eval's arguments after the context through csrc/fuse_math.h on the calling thread; -1 where the device entry returns CCM_E_ARG.
// n_cand (nullable, sum(job_n)): the size of vIndices of every pair that reached the window (0 otherwise), for scripts/fuse_pose_profile.py.
int fuse_pose_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                        const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2,
                        float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc,
                        int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv,
                        int32_t* n_cand);

// ccm_fuse_sim3_eval_resident's / ccm_fuse_pose_eval_resident's arguments after the context on the store's shadows through csrc/fuse_math.h on the calling thread;
// -1 where the device entry returns CCM_E_ARG (a key that is not live among it).
int fuse_sim3_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor,
                                 float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc,
                                 uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int fuse_pose_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors,
                                 const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                 const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n,
                                 uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);

// ---------------------------------------------------------------------------------------------------
// ComputeSim3's two projected searches on keyframes of a store (LoopFinder.cpp:326, :380; MapMatcher.cpp:330, :382).
// ---------------------------------------------------------------------------------------------------
// ccm_sim3_project_eval_resident's / ccm_sim3_pair_eval_resident's pairs through csrc/fuse_math.h on the calling thread, on plain keyframe arrays laid out as
// fuse_sim3_eval_host's (a mask is held to feat_off's feature counts) and on the shadows of a store; -1 where the device entry returns CCM_E_ARG.
int sim3_project_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                           const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels,
                           const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                           const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int sim3_pair_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc,
                        const int32_t* cell_off, const int32_t* cell_idx, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos,
                        const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4, const float* job_src_pose,
                        const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int sim3_project_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels,
                                    const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                    const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int sim3_pair_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P,
                                 const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4,
                                 const float* job_src_pose, const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid,
                                 int32_t* n_hit, float* uv);

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:308-446) on one key of a store.  The constructor evaluates every point against
// the INITIAL vpMatched (matched0[f] != 0: vpMatched[f] is set) in ONE ccm_sim3_project_eval_resident call, or on the calling thread when the store is host-only or
// ctx == nullptr; with a context a device error throws.  resolve replays the reference's loop in point order.  While that loop runs the mask only grows (a point
// that is accepted claims its feature, :439), and a growing mask changes the answer of a point in one case alone: its best candidate has been claimed.  (A best
// above TH_LOW stays above it when candidates leave; every other status finds nothing either way.)  So the table word is the answer except for a status-7 word
// whose feature an earlier point of THIS call has claimed; such a point is evaluated again on the calling thread with the current mask.
class Sim3ProjectionSearch {
 public:
  typedef SearchAndFuseBatch::Points Points;
  Sim3ProjectionSearch(KeyFrameStore& store, HipContext* ctx, int64_t key, const float* Scw12, const Points& pts, const uint8_t* matched0, int nlevels,
                       const float* scale_factors, float logScaleFactor, float th);
  // skip_now[i] != 0 (nullable): the reference would `continue` now (pMP->isBad() || spAlreadyFound.count(pMP)).  existing_idx[i] >= 0 (nullable): the keyframe
  // observes point i already (GetIndexInKeyFrame, :415); such a point claims nothing and is not counted, its best feature comes back in remap[i] and GetMapPoint /
  // RemapMapPointMatch (:420-434) stay the caller's.  matched (features() entries, in / out): >= 0 where vpMatched is set, on entry as matched0 said; point i's
  // claim writes i.  bestIdx[i]: the feature point i claimed, or -1.  Returns nmatches.
  int resolve(const uint8_t* skip_now, const int32_t* existing_idx, int32_t* matched, std::vector<int32_t>& bestIdx, std::vector<int32_t>& remap);
  int points() const { return P_; }
  int features() const { return N_; }
  const std::vector<uint32_t>& table() const { return table_; }   // as evaluated at construction
  int nValid() const { return n_valid_; }
  int nHit() const { return n_hit_; }
  long long n_reeval() const { return n_reeval_; }                 // points evaluated again by resolve because their feature had been claimed
 private:
  int P_ = 0, N_ = 0, n_valid_ = 0, n_hit_ = 0;
  FuseScene scene_;
  std::vector<uint32_t> table_;
  long long n_reeval_ = 0;
};

// ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cpp:1124-1348) on two keys of a store.  A side holds, per feature slot of its
// keyframe, live (pMP && !pMP->isBad()), the point's position, distance bounds and descriptor (read where live), and the keyframe's pose R (9, row-major), t (3).
// matches12_in[i] (N1 entries): -1 where vpMatches12[i] is null, otherwise the index of that point in keyframe 2 (GetIndexInKeyFrame(pKF2); any value outside
// 0 .. N2 - 1 where it has none).  The constructor computes vbAlreadyMatched1 / 2 (:1154-1164), packs the live unmatched points of both sides into two jobs, makes
// ONE ccm_sim3_pair_eval_resident call (the host evaluation when the store is host-only or ctx == nullptr; with a context a device error throws), unpacks
// vnMatch1 / 2 and runs ORBmatcher::MutualAgreement.  Both directions project with keyframe 1's intrinsics, as the reference does (:1127-1130).
class SearchBySim3Batch {
 public:
  struct Side { int N = 0; const uint8_t* live = nullptr; const float* pos = nullptr; const float* min_dist = nullptr; const float* max_dist = nullptr;
                const uint8_t* desc = nullptr; const float* pose = nullptr; };
  SearchBySim3Batch(KeyFrameStore& store, HipContext* ctx, int64_t key1, int64_t key2, const Side& kf1, const Side& kf2, float s12, const float* R12, const float* t12,
                    const int32_t* matches12_in, int nlevels, const float* scale_factors, float logScaleFactor, float th);
  int nFound() const { return n_found_; }
  const std::vector<int32_t>& matches12() const { return matches12_; }   // N1: the entry state, and the KF2 feature of every new match
  const std::vector<int32_t>& vnMatch1() const { return vn1_; }
  const std::vector<int32_t>& vnMatch2() const { return vn2_; }
  const std::vector<int32_t>& nValid() const { return n_valid_; }        // per direction
  const std::vector<int32_t>& nHit() const { return n_hit_; }
 private:
  int n_found_ = 0;
  std::vector<int32_t> matches12_, vn1_, vn2_, n_valid_, n_hit_;
};

// ccm_bow_pair_eval_resident's arguments after the context through csrc/bow_search_math.h on the calling thread, on the shadows of a store; -1 where the device
// entry returns CCM_E_ARG.
int bow_pair_eval_resident_host(const KeyFrameStore& store, int J, const int64_t* key1, const int64_t* key2, const int32_t* live1_off, const uint8_t* live1,
                                const int32_t* live2_off, const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist);

// ORBmatcher::SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) (ORBmatcher.cpp:565-698) for ALL candidates of a ComputeSim3 (LoopFinder.cpp:251-282,
// MapMatcher.cpp:271) on keys of a store that have their feature vector.  live1 (one byte per feature of key1) / live2[j] (per
// feature of keys2[j]): pMP && !pMP->isBad() of the slot.  The constructor evaluates every query of every candidate against the INITIAL vbMatched2 in ONE
// ccm_bow_pair_eval_resident call, or on the calling thread when the store is host-only or ctx == nullptr; with a context a device error throws.  It then replays
// the reference's loop per candidate: the common nodes ascending, the queries in list order, TH_LOW, the strict ratio test, the claims and the rotation histogram.
// A feature of keyframe 2 lies in exactly one node, so claims reach a query only from earlier queries of ITS node: the device word stands unless a feature claimed
// so far in the node is at a distance <= the word's bestDist2 from the query (one popcount on the shadows' descriptors each), and a word with
// bestDist1 >= TH_LOW stands whatever was claimed (fewer candidates never lower it).  A query that fails these tests is evaluated again on the calling thread over
// its node's segment minus the claimed features.
class SearchByBoWBatch {
 public:
  SearchByBoWBatch(KeyFrameStore& store, HipContext* ctx, int64_t key1, int C, const int64_t* keys2, const uint8_t* live1, const uint8_t* const* live2, float nnratio,
                   bool checkOrientation);
  int candidates() const { return (int)nmatches_.size(); }
  int nmatches(int j) const { return nmatches_.at((size_t)j); }
  const std::vector<int32_t>& matches12(int j) const { return matches12_.at((size_t)j); }   // per feature of key1: the feature of keys2[j] or -1
  const std::vector<uint64_t>& table() const { return table_; }                              // as evaluated at construction, candidate after candidate
  const std::vector<int32_t>& nQuery() const { return n_query_; }
  const std::vector<int32_t>& nDist() const { return n_dist_; }
  long long reevaluated() const { return n_reeval_; }
 private:
  std::vector<int> nmatches_;
  std::vector<std::vector<int32_t>> matches12_;
  std::vector<uint64_t> table_;
  std::vector<int32_t> n_query_, n_dist_;
  long long n_reeval_ = 0;
};

// ccm_tri_search_eval_resident's arguments after the context through csrc/tri_search_math.h on the calling thread, on the shadows of a store; -1 where the device
// entry returns CCM_E_ARG.
int tri_search_eval_resident_host(const KeyFrameStore& store, int J, const int64_t* key1, const int64_t* key2, const int32_t* has1_off, const uint8_t* has1,
                                  const int32_t* has2_off, const uint8_t* has2, const float* job_epi, int nlevels, const float* scale_factors, const float* level_sigma2,
                                  uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist);

// ORBmatcher::SearchForTriangulation(mpCurrentKeyFrame, pKF2_j, F12_j, ...) (ORBmatcher.cpp:700-852) for ALL neighbours of a CreateNewMapPoints (Mapping.cpp:277-470)
// on keys of a store that have their feature vector.  has1 (one byte per feature of key1) / has2[j] (per feature of keys2[j]):
// GetMapPoint(idx) != nullptr.  ep[j]: F12 and the epipole of neighbour j; sigma2_2 / sf2: mvLevelSigma2 / mvScaleFactors, nlevels entries.  The constructor
// evaluates every query of every neighbour in ONE ccm_tri_search_eval_resident call, or on the calling thread when the store is host-only or ctx == nullptr; with a
// context a device error throws.  The reference never sets vbMatched2, so a word is the whole answer of its query under the flags of the build.
// resolve(j, has1_now, has2_now, matches12) returns nmatches of the call against neighbour j under the flags of ITS moment (nullptr: the build's):
//   a query with has1_now set is dropped (:745-747: what the loop creates between calls);
//   a feature that had a map point at the build and has none now has no word and is evaluated on the calling thread;
//   a word stands unless its bestIdx2 has gained a map point or some feature of its node's segment of keyframe 2 has lost one; the query is then evaluated again
//   under has2_now by the same lines (a candidate that leaves without being the winner cannot change the winner).  reevaluated() counts these;
//   then :787-839 on the surviving matches in node order, then list order: the rotation histogram on the shadows' angles.
// F12 and the epipole are the build's: a caller whose poses changed builds a new batch.  predicted(j): resolve with the build's flags as (idx1, idx2) pairs in
// ascending idx1 (:844-849), which is what NewMapPointBatch's Neighbour::predicted takes.
class SearchForTriangulationBatch {
 public:
  using Epipolar = NewMapPointBatch::Epipolar;
  SearchForTriangulationBatch(KeyFrameStore& store, HipContext* ctx, int64_t key1, int C, const int64_t* keys2, const uint8_t* has1, const uint8_t* const* has2,
                              const Epipolar* ep, const float* sigma2_2, const float* sf2, int nlevels, bool checkOrientation);
  int neighbours() const { return (int)kfs2_.size(); }
  int features1() const { return kf1_->n; }
  int resolve(int j, const uint8_t* has1_now, const uint8_t* has2_now, std::vector<int32_t>& matches12);
  NewMapPointBatch::Pairs predicted(int j);
  const std::vector<uint32_t>& table() const { return table_; }   // as evaluated at construction, neighbour after neighbour
  const std::vector<int32_t>& nQuery() const { return n_query_; }
  const std::vector<int32_t>& nMatch() const { return n_match_; }
  const std::vector<int32_t>& nDist() const { return n_dist_; }
  long long reevaluated() const { return n_reeval_; }
 private:
  std::shared_ptr<const KfShadow> kf1_;
  std::vector<std::shared_ptr<const KfShadow>> kfs2_;
  std::vector<uint8_t> has1_, has2_;
  std::vector<int32_t> off1_, off2_;
  std::vector<float> epi_, sigma2_, sf_;
  std::vector<uint32_t> table_;
  std::vector<int32_t> n_query_, n_match_, n_dist_;
  int nlevels_; bool check_ori_;
  long long n_reeval_ = 0;
};

// ccm_mappoint_refresh_resident's arguments after the context through csrc/mappoint_math.h on the calling thread, on the shadows of a store; -1 where the device entry
// returns CCM_E_ARG, the outputs untouched.
int mappoint_refresh_eval_resident_host(const KeyFrameStore& store, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf,
                                        const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels, const float* scale_factors,
                                        int32_t* best_obs, uint8_t* best_desc, float* normal, float* min_dist, float* max_dist, uint8_t* status);

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) for the map points a map stage touched, on keys of a
// store: the refresh that follows ProcessNewKeyFrame, CreateNewMapPoints, SearchInNeighbors and every Replace.  Lists: point p
// owns the observations obs_off[p] .. obs_off[p + 1], each (obs_kf: index into keys, obs_feat: the feature index), non-bad observers in the order of mObservations.
// Refs: ref_kf[p] indexes keys (-1: the descriptor alone, as after Replace) and ref_feat[p] is observations[pRefKF]; normal / min_dist / max_dist are the points'
// current values, which a point keeps when it has no observation, no reference or a reference octave beyond the tables.  The constructor makes ONE
// ccm_mappoint_refresh_resident call, or evaluates on the calling thread when the store is host-only or ctx == nullptr; with a context a device error throws.
class MapPointRefresh {
 public:
  struct Lists { int P; const int32_t *obs_off, *obs_kf, *obs_feat; };
  struct Refs { const float* pos; const int32_t *ref_kf, *ref_feat; const float *normal, *min_dist, *max_dist; };
  MapPointRefresh(KeyFrameStore& store, HipContext* ctx, int K, const int64_t* keys, const float* kf_center, const Lists& lists, const Refs& refs, int nlevels,
                  const float* scale_factors);
  int points() const { return (int)best_.size(); }
  const std::vector<int32_t>& best() const { return best_; }        // the winning observation of every point's list, -1 for an empty list
  const uint8_t* descriptor(int p) const { return best_[(size_t)p] < 0 ? nullptr : desc_.data() + 32 * (size_t)p; }   // mDescriptor; nullptr: unchanged
  const std::vector<float>& normal() const { return normal_; }      // 3 per point
  const std::vector<float>& min_dist() const { return dmin_; }
  const std::vector<float>& max_dist() const { return dmax_; }
  const std::vector<uint8_t>& status() const { return status_; }    // MPM_DESC | MPM_NORMAL_DEPTH | MPM_OCTAVE_BEYOND of csrc/mappoint_math.h
 private:
  std::vector<int32_t> best_;
  std::vector<uint8_t> desc_, status_;
  std::vector<float> normal_, dmin_, dmax_;
};

// ---------------------------------------------------------------------------------------------------
// Optimizer — cslam/include/cslam/Optimizer.h:84-112 (numerics; graph walking is the integrator's glue)
// ---------------------------------------------------------------------------------------------------
struct BAProblem {   // owning, f64 like g2o; filled from KeyFrames / MapPoints via Converter (Converter.cc:40-119)
  std::vector<double> cam_qt;   // n_cam*7
  std::vector<uint8_t> cam_fixed;
  std::vector<double> cam_K;    // n_cam*4
  std::vector<double> pt_xyz;   // n_pt*3
  std::vector<int32_t> e_cam, e_pt;
  std::vector<double> e_obs, e_info;
  int n_cam() const { return (int)cam_fixed.size(); }
  int n_pt() const { return (int)pt_xyz.size() / 3; }
  int n_edge() const { return (int)e_cam.size(); }
};

class Optimizer {
 public:
  // PoseOptimizationClient (Optimizer.cpp:215-347): returns nInitialCorrespondences - nBad; outlier[] = mvbOutlier
  static int PoseOptimizationClient(HipContext& ctx, double cam_qt[7], int n, const double* Xw, const double* obs,
                                    const double* invSigma2, const double K[4], std::vector<uint8_t>& outlier);
  // LocalBundleAdjustmentClient numerics (Optimizer.cpp:532-602): optimize(5) Huber sqrt(5.991) -> outliers to level 1,
  // kernel off -> optimize(10).  pbStopFlag as in the reference.  to_erase[e] = 1 for observations the reference erases.
  static void LocalBundleAdjustmentClient(HipContext& ctx, BAProblem& p, bool* pbStopFlag, std::vector<uint8_t>& to_erase);
  // BundleAdjustmentClient / MapFusionGBA numerics (Optimizer.cpp:163-167, 786-797): optimize(nIterations), Huber sqrt(5.99)
  static void GlobalBundleAdjustment(HipContext& ctx, BAProblem& p, int nIterations, bool* pbStopFlag, bool bRobust,
                                     ccm_ba_stats* stats = nullptr);
  // OptimizeSim3 (Optimizer.cpp:861-1056).  Pair i of the valid correspondences (:911-947): P1c / P2c = the points in
  // their own keyframe's camera frame, obs = undistorted keypoints, invSigma2 per octave.  g2oS12 = [qx qy qz qw tx ty tz s]
  // in/out; keep[i] = 0 where the reference nulls vpMatches1[idx]; returns nIn (0 => g2oS12 untouched).
  static int OptimizeSim3(HipContext& ctx, double g2oS12[8], int n, const double* P1c, const double* P2c, const double* obs1,
                          const double* obs2, const double* invSigma2_1, const double* invSigma2_2, const double K1[4],
                          const double K2[4], float th2, bool bFixScale, std::vector<uint8_t>& keep);
  // OptimizeEssentialGraphLoopClosure / MapFusion numerics (Optimizer.cpp:1058-1331, 1333-1566): the caller builds the vertex
  // list (Siw per keyframe as [qx qy qz qw tx ty tz s], fixed = pLoopKF) and the edge list (i, j, Sji) exactly as the two
  // functions do (:1122-1260: loop connections, spanning tree, loop edges, covisibility >= minFeat) and applies the write-back
  // (:1268-1330) from the optimised vertices.  optimize(20) with setUserLambdaInit(1e-16).
  static void OptimizeEssentialGraph(HipContext& ctx, std::vector<double>& vScw, const std::vector<uint8_t>& fixed, bool bFixScale,
                                     const std::vector<int32_t>& e_i, const std::vector<int32_t>& e_j, const std::vector<double>& Sji,
                                     ccm_pg_stats* stats = nullptr);
};

// What relocalisation does with ONE pose PnPRansacBatch::next() returned (the body ORB-SLAM2's Tracking::Relocalization runs on it): the inliers of
// matchesF (SearchByBoW(KF, F): F.N entries, each a slot of the candidate keyframe or -1) seed F.mvpMapPoints, PoseOptimizationClient, and with 10 .. 49 inliers the
// two guided searches (th 10 / ORBdist 100, then th 3 / ORBdist 64) with an optimisation after each.  The matcher is ORBmatcher(0.9, true).  frame.Tcw is the PnP
// pose (rows 0..2); frame's pyramid members are the Frame's.  F.mvpMapPoints is overwritten.
struct RelocRefineResult {
  bool matched = false;
  int nGood = 0;
  float Tcw[16];                           // the frame's pose at the end
  int trace[5] = {-1, -1, -1, -1, -1};     // nGood of optimisation 1, nadd of search 1, nGood 2, nadd 2, nGood 3; -1: the step did not run
};
RelocRefineResult RelocalizationRefine(HipContext& ctx, FrameGridDev& grid, FrameView& F, const float K[4], const float* mvInvLevelSigma2,
                                       const ccm_guided_pose& frame, const KeyFramePoints& kf, const int32_t* matchesF, const uint8_t* vbInliers);

}  // namespace cslam
