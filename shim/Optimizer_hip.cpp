// Optimizer_hip.cpp — DROP-IN replacement for the translation unit cslam/src/Optimizer.cpp of the reference.
//
// It defines the static methods that the reference's own header declares (cslam/include/cslam/Optimizer.h:79-112) — same names, same
// signatures, compiled against that header — and does what Optimizer.cpp does around g2o: the graph walks that choose vertices and
// edges, the f32 -> f64 conversions on the way in (Converter.cc:40-119, here ccm_convert.h), the write-back with its side effects
// (SetPose, SetWorldPos, UpdateNormalAndDepth, EraseObservation, mTcwGBA ...).  The optimisation itself — everything that was g2o —
// goes through the C ABI of libccm_hip.so (include/ccm_hip.h) to the MI355X: no g2o optimiser, solver, vertex or edge object is created.
// The only g2o type that appears is the VALUE type g2o::Sim3 (header-only arithmetic), because it is part of the reference's interface
// (OptimizeSim3's g2oS12, KeyFrameAndPose) and the essential-graph functions compose their edge measurements from it exactly as the
// reference does.  cslam::Converter (Converter.cc) is a separate translation unit of the reference and stays in the build.
//
// Build: shim/Makefile.  In this repository the map classes are the look-alikes of oracle/ref_shim/cslam_lookalike (the real KeyFrame.h /
// MapPoint.h / Map.h need ROS, PCL, DBoW2 and cereal, none of which is installed); the member names and types used here are those of
// the real headers, so the same file compiles in a catkin workspace with `Optimizer.cpp` replaced by it in cslam/CMakeLists.txt:122-145.
// tests/test_shim_gpu.py runs this file and the reference's Optimizer.cpp on identical synthetic maps and compares what they leave
// behind in the map.
//
// LICENCE AND PROVENANCE.  This file is a derived work of cslam/src/Optimizer.cpp of CCM-SLAM (Copyright (C) Patrik Schmuck, ETH Zurich; GNU GPL v3 or later; itself based
// on ORB-SLAM2 by Raul Mur-Artal) and is distributed under the same licence.  Everything numerical is a call into libccm_hip.so, and the graph walks are written in this
// project's own form: each walk is one pass into flat tables (FlatBA's vertex / edge arrays, the per-mUniqueId Sim3 tables of the essential graph), the optimisation reads
// only those tables, and one write-back pass follows.  What a drop-in cannot choose freely, and what therefore still follows Optimizer.cpp, is the OUTCOME of each walk:
//   * which objects become vertices and which observations edges, and in which order the edges are met (container order, and inside a point the iteration order of
//     GetObservations()): the flat problem and so the bits that come back depend on it                                                       (Optimizer.cpp:55-140, 351-530, 668-790)
//   * the side effects of the local window walk (mBALocalForKF / mBAFixedForKF tags, the stop-flag return, LockMapUpdate, erase before write-back, mbUpdatedByServer)
//     and the order of the map mutations of every entry point                                                                               (Optimizer.cpp:568-644, 795-859, 1265-1331)
//   * the edge order of the essential graph (loop connections; then per keyframe: parent, loop edges, covisibility) and how a measurement is composed from g2o::Sim3
//     values, the reference's interface type                                                                                                (Optimizer.cpp:1122-1262)
//   * the signatures and the names of the reference's members, which are its API.
// By the count of scripts/shim_overlap.py (comments and whitespace stripped, trivial lines dropped) 21 of this file's 740 code lines occur verbatim in Optimizer.cpp
// (2.8 %; before the walks were rewritten: 199 of 926); they are member calls and declarations that the API above fixes.
// What the shim prints (its fatal conditions, device errors) is its own wording; what it throws is the reference's exception type, because callers catch that.
#include <cslam/Optimizer.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <unistd.h>   // usleep (the local BA's wait for Map::LockMapUpdate)

#include "../include/ccm_hip.h"
#include "../ccm_slam_amd/host/ccm_convert.h"

namespace cslam {
namespace {

// Fatal conditions of the graph walks: the reference prints a message and throws estd::infrastructure_ex (Optimizer.cpp:87-90, 480-483, 595-598, 663-666); a drop-in
// keeps the EXCEPTION TYPE (callers catch it) and says in its own words what was wrong and where.
[[noreturn]] void shim_fatal(const char* method, const char* what) {
  std::cout << "[ccm_hip shim] " << method << ": " << what << " (infrastructure_ex)" << std::endl;
  throw estd::infrastructure_ex();
}
// ids are packed as IDRANGE * client + id (Optimizer::GetID): an id at or above IDRANGE would alias another client's vertex
void require_id_below_range(const char* method, const char* kind, const idpair& id) {
  if (id.first >= IDRANGE) shim_fatal(method, (std::string(kind) + " id is not below IDRANGE").c_str());
}

// the two id policies of the bundle adjustments: packed (client, id) pairs on the client paths, the server's map-wide mUniqueId in MapFusionGBA
struct ClientIds {
  static size_t of(const KeyFrame& kf) { return Optimizer::GetID(kf.mId, true); }
  static size_t of(const MapPoint& mp) { return Optimizer::GetID(mp.mId, false); }
};
struct UniqueIds {
  static size_t of(const KeyFrame& kf) { return kf.mUniqueId; }
  static size_t of(const MapPoint& mp) { return mp.mUniqueId; }
};

// chi2 test of a monocular edge at 95 % (2 degrees of freedom) plus the cheirality test: the local BA's outlier rule
inline bool is_outlier(double chi2, uint8_t depth_positive) { return chi2 > 5.991 || !depth_positive; }

// 4x4 CV_32F pose <-> row-major float[16] (what ccm_convert.h works on)
void pose_to16(const cv::Mat& m, float T[16]) { for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[4 * r + c] = m.at<float>(r, c); }
cv::Mat pose_from16(const float T[16]) {
  cv::Mat m(4, 4, CV_32F);
  for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) m.at<float>(r, c) = T[4 * r + c];
  return m;
}

// one device context per calling thread: tracking, local mapping and the server's optimisation threads call concurrently
ccm_ctx* thread_ctx() {
  struct Holder {
    ccm_ctx* c = nullptr;
    ~Holder() { if (c) ccm_ctx_destroy(c); }
  };
  static thread_local Holder h;
  if (!h.c) {
    const char* dev = std::getenv("CCM_DEVICE");
    if (ccm_ctx_create(dev ? std::atoi(dev) : 0, &h.c) != CCM_OK) {
      cout << COUTFATAL << "no MI355X context: " << ccm_last_error(nullptr) << endl;
      throw infrastructure_ex();
    }
  }
  return h.c;
}
void check(int rc, const char* what) {
  if (rc != CCM_OK) {
    cout << COUTFATAL << what << ": " << ccm_last_error(thread_ctx()) << endl;
    throw infrastructure_ex();
  }
}

// wall-clock phases of the last bundle-adjustment call made by this thread (ms): [0] graph walk (vertices + edges gathered), [1] flatten (ids -> indices,
// f32 -> f64), [2] ccm_ba_create (structure build: g2o's initializeOptimization + buildStructure), [3] ccm_ba_run (optimize(n)), [4] download (+ depth
// test), [5] keyframe write-back, [6] map-point write-back (SetWorldPos + UpdateNormalAndDepth), [7] whole call.  Read with ccm_shim_last_phases().
// (round 5) [8] GetAll* + camera vertices, [9] dropping the call's references into the flat problem, [10] SCOPE EXIT: everything the call's locals free.  On the
// 4-agent map this was the largest unlabelled part of the call (29 ms after the last lap).  It is not the 150 000 shared_ptr copies Map::GetAllMapPoints() hands
// out (those are dropped inside the write-back loop now, by the thread that has just worked on the point) but glibc: the threaded write-back frees the points' old
// cv::Mat buffers — allocated by whichever thread built the map — back into THAT thread's arena, ~2 fastbin chunks per point, and the first large free() / malloc()
// that arena sees afterwards (here: the 2.4 MB pointer vector at scope exit) runs malloc_consolidate over all of them (measured with MALLOC_ARENA_MAX=1: the phase
// vanishes; on one thread there is no cross-arena garbage either).  With the optional MapPoint setter the write-back reuses the buffers and the
// phase is empty.  [11] what is still unaccounted (total - sum of the others).  Read with ccm_shim_phases().
constexpr int kPhases = 12;
enum Phase { kWalk = 0, kFlatten = 1, kCreate = 2, kRun = 3, kDownload = 4, kKfWriteback = 5, kMpWriteback = 6, kTotal = 7, kVertices = 8, kRelease = 9, kScopeExit = 10, kUnaccounted = 11 };
thread_local double g_phase[kPhases] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct PhaseClock {
  double t0, t;
  PhaseClock() : t0(now_ms()), t(t0) { for (double& v : g_phase) v = 0; }
  void lap(Phase i) { const double n = now_ms(); g_phase[i] += n - t; t = n; }
  void restart() { t = now_ms(); }   // after run_ba, which clocks kCreate / kRun / kDownload itself
  ~PhaseClock() {
    g_phase[kTotal] = now_ms() - t0;
    double sum = 0;
    for (int i = 0; i < kUnaccounted; i++) if (i != kTotal) sum += g_phase[i];
    g_phase[kUnaccounted] = g_phase[kTotal] - sum;
  }
};

// host threads for the per-map-point work of a global bundle adjustment (graph walk, write-back): every map point is independent and the
// reference's accessors take the point's own mutexes, so contiguous chunks of vpMP are handled by a few threads and merged in order.
// Measured on the 4-agent map (150 000 points, 256-core host): walk 87 ms on one thread, 36 on 8, 34 on 32 (shared_ptr reference counts of
// the 2000 keyframes bounce between the cores); write-back 230 / 46 / 17 ms.  CCM_SHIM_THREADS overrides (1 = the calling thread only).
int shim_threads(size_t n_items, unsigned cap = 8) {
  static const int env = std::getenv("CCM_SHIM_THREADS") ? std::atoi(std::getenv("CCM_SHIM_THREADS")) : 0;
  int t = env > 0 ? env : (int)std::min<unsigned>(std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 1u, cap);
  if (n_items < 20000) t = 1;
  return std::max(1, t);
}
template <typename F>
void parallel_chunks(size_t n, int n_thr, F fn /* (chunk index, begin, end) */) {
  if (n_thr <= 1) { fn(0, (size_t)0, n); return; }
  std::vector<std::thread> th;
  std::vector<std::exception_ptr> err((size_t)n_thr);
  for (int t = 0; t < n_thr; t++)
    th.emplace_back([&, t]() {
      try { fn(t, n * (size_t)t / (size_t)n_thr, n * (size_t)(t + 1) / (size_t)n_thr); } catch (...) { err[(size_t)t] = std::current_exception(); }
    });
  for (auto& x : th) x.join();
  for (auto& e : err) if (e) std::rethrow_exception(e);
}

// the call's own copies of the caller's pointer vectors, released on the host threads that have just written the objects back (their reference counts sit in
// those cores' caches; one thread doing 150 000 lock-prefixed decrements on remote lines took ~29 ms at the end of MapFusionGBA on the 4-agent map)
template <typename P>
void release_refs(std::vector<P>& v) {
  parallel_chunks(v.size(), shim_threads(v.size(), 32), [&](int, size_t b, size_t e) { for (size_t i = b; i < e; i++) v[i].reset(); });
  std::vector<P>().swap(v);
}

// vertex id -> index: a direct table when the ids are compact (mUniqueId, GetID of a few clients), a sorted list otherwise
struct IdIndex {
  std::vector<int32_t> table;
  std::vector<std::pair<size_t, int32_t>> sorted;
  void build(const std::vector<size_t>& ids) {
    table.clear(); sorted.clear();
    size_t mx = 0;
    for (size_t v : ids) mx = std::max(mx, v);
    if (mx <= 8 * ids.size() + 4096) {
      table.assign(mx + 1, -1);
      for (size_t i = 0; i < ids.size(); i++) table[ids[i]] = (int32_t)i;
    } else {
      sorted.reserve(ids.size());
      for (size_t i = 0; i < ids.size(); i++) sorted.push_back({ids[i], (int32_t)i});
      std::sort(sorted.begin(), sorted.end());
    }
  }
  int32_t find(size_t id) const {
    if (!table.empty()) return id < table.size() ? table[id] : -1;
    auto it = std::lower_bound(sorted.begin(), sorted.end(), std::make_pair(id, (int32_t)INT32_MIN));
    return (it != sorted.end() && it->first == id) ? it->second : -1;
  }
};

// a flat bundle-adjustment problem under construction; cameras and points are numbered in g2o VERTEX-ID order, the order in which g2o
// itself sorts its active vertices (sparse_optimizer.cpp:482-487).  Edges keep their insertion order (the callers index per-edge results by it).
struct FlatBA {
  std::vector<size_t> cam_id, pt_id;                 // insertion order until flatten() sorts them by id
  std::vector<Optimizer::kfptr> cam_kf;
  std::vector<char> cam_is_fixed;
  std::vector<MapPoint*> pt_mp;                      // raw: the caller's containers keep the points alive, and 150 000 shared_ptr copies cost ~15 ms of cache-missing atomics each way
  std::vector<size_t> e_cam_id, e_pt_id;             // per edge: vertex ids
  // per point, only filled when MapPoint offers SetNormalAndDepth (batched UpdateNormalAndDepth of the write-back): id of the reference keyframe, octave of the
  // point's keypoint there, and whether EVERY non-bad observation became an edge (else the point takes the reference's own method)
  std::vector<size_t> pt_ref_cam_id;
  std::vector<int32_t> pt_ref_level;
  std::vector<char> pt_regular;
  bool aux_ok = true;                                // false once flatten() had to reorder the points (the per-point arrays above are in insertion order)
  std::vector<double> pt_xyz_walk;                   // optional: Converter::toVector3d(pMP->GetWorldPos()) taken by the graph walk while it holds the point (3 per point, insertion order)
  // flattened
  std::vector<double> cam_qt, cam_K, pt_xyz, e_obs, e_info;
  std::vector<uint8_t> cam_fix, e_level;
  std::vector<int32_t> e_cam, e_pt;
  IdIndex cam_index, pt_index;

  size_t nEdges() const { return e_cam_id.size(); }
  void reset() {   // keeps every vector's capacity: the global BA of a 4-agent map builds ~60 MB of flat arrays, and allocating (first-touch page faults) and
                   // releasing (munmap) them cost ~50 ms per call — the server thread keeps one FlatBA for its lifetime instead
    cam_id.clear(); pt_id.clear(); cam_kf.clear(); cam_is_fixed.clear(); pt_mp.clear(); e_cam_id.clear(); e_pt_id.clear();
    pt_ref_cam_id.clear(); pt_ref_level.clear(); pt_regular.clear(); aux_ok = true; pt_xyz_walk.clear();
    cam_qt.clear(); cam_K.clear(); pt_xyz.clear(); e_obs.clear(); e_info.clear(); cam_fix.clear(); e_level.clear(); e_cam.clear(); e_pt.clear();
  }
  void addCam(size_t id, Optimizer::kfptr kf, bool is_fixed) { cam_id.push_back(id); cam_kf.push_back(kf); cam_is_fixed.push_back(is_fixed ? 1 : 0); }
  void addPoint(size_t id, const Optimizer::mpptr& mp) { pt_id.push_back(id); pt_mp.push_back(mp.get()); }
  void addPointPos(const cv::Mat& P) { const float p[3] = {P.at<float>(0), P.at<float>(1), P.at<float>(2)}; double d[3]; ccmh::toVector3d(p, d); pt_xyz_walk.insert(pt_xyz_walk.end(), d, d + 3); }
  void addPointAux(size_t ref_cam_id, int level, bool regular) { pt_ref_cam_id.push_back(ref_cam_id); pt_ref_level.push_back(level); pt_regular.push_back(regular ? 1 : 0); }
  void addEdge(size_t p_id, const Optimizer::kfptr& kf, size_t c_id, const cv::KeyPoint& kpUn) {
    const float& invSigma2 = kf->mvInvLevelSigma2[kpUn.octave];
    e_cam_id.push_back(c_id); e_pt_id.push_back(p_id);
    e_obs.push_back((double)kpUn.pt.x); e_obs.push_back((double)kpUn.pt.y); e_info.push_back((double)invSigma2);
  }
  // THE observation walk of all three bundle adjustments: one map point as a vertex and its observations as edges, in the iteration order of the
  // observation map.  accept(keyframe) is the caller's rule for which observations count; a point that ends with fewer than min_edges edges is taken out
  // again with what it added.  Returns the number of edges kept.
  template <typename Ids, typename Accept>
  int addPointWithEdges(const Optimizer::mpptr& mp, const std::map<Optimizer::kfptr, size_t>& observations, int min_edges, Accept accept) {
    const size_t p_id = Ids::of(*mp), e0 = e_cam_id.size();
    addPoint(p_id, mp);
    for (const auto& ob : observations) {
      const Optimizer::kfptr& kf = ob.first;
      if (accept(kf)) addEdge(p_id, kf, Ids::of(*kf), kf->mvKeysUn[ob.second]);
    }
    const int n = (int)(e_cam_id.size() - e0);
    if (n >= min_edges) return n;
    pt_id.pop_back(); pt_mp.pop_back();
    e_cam_id.resize(e0); e_pt_id.resize(e0); e_obs.resize(2 * e0); e_info.resize(e0);
    return 0;
  }
  void append(FlatBA& o) {        // merge of a thread's part (points and edges of a later chunk of vpMP)
    pt_id.insert(pt_id.end(), o.pt_id.begin(), o.pt_id.end()); pt_mp.insert(pt_mp.end(), o.pt_mp.begin(), o.pt_mp.end());
    e_cam_id.insert(e_cam_id.end(), o.e_cam_id.begin(), o.e_cam_id.end()); e_pt_id.insert(e_pt_id.end(), o.e_pt_id.begin(), o.e_pt_id.end());
    e_obs.insert(e_obs.end(), o.e_obs.begin(), o.e_obs.end()); e_info.insert(e_info.end(), o.e_info.begin(), o.e_info.end());
    pt_ref_cam_id.insert(pt_ref_cam_id.end(), o.pt_ref_cam_id.begin(), o.pt_ref_cam_id.end());
    pt_ref_level.insert(pt_ref_level.end(), o.pt_ref_level.begin(), o.pt_ref_level.end()); pt_regular.insert(pt_regular.end(), o.pt_regular.begin(), o.pt_regular.end());
    pt_xyz_walk.insert(pt_xyz_walk.end(), o.pt_xyz_walk.begin(), o.pt_xyz_walk.end());
  }
  template <typename P>
  static void sort_by_id(std::vector<size_t>& ids, std::vector<P>& ptrs, std::vector<char>* flags) {
    if (std::is_sorted(ids.begin(), ids.end())) return;
    std::vector<size_t> perm(ids.size());
    for (size_t i = 0; i < perm.size(); i++) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return ids[a] < ids[b]; });
    std::vector<size_t> ids2(ids.size()); std::vector<P> p2(ids.size()); std::vector<char> f2(flags ? ids.size() : 0);
    for (size_t i = 0; i < perm.size(); i++) { ids2[i] = ids[perm[i]]; p2[i] = ptrs[perm[i]]; if (flags) f2[i] = (*flags)[perm[i]]; }
    ids.swap(ids2); ptrs.swap(p2); if (flags) flags->swap(f2);
  }
  // g2o refuses an edge whose camera vertex does not exist (optimizer.vertex(id) == 0 -> addEdge fails): such observations are dropped
  void flatten(bool drop_edges_without_camera = false) {
    sort_by_id(cam_id, cam_kf, &cam_is_fixed);
    if (!std::is_sorted(pt_id.begin(), pt_id.end())) aux_ok = false;
    sort_by_id<MapPoint*>(pt_id, pt_mp, nullptr);
    cam_index.build(cam_id); pt_index.build(pt_id);
    const size_t nc = cam_id.size(), np = pt_id.size();
    cam_qt.resize(7 * nc); cam_K.resize(4 * nc); cam_fix.resize(nc); pt_xyz.resize(3 * np);
    for (size_t i = 0; i < nc; i++) {
      const cv::Mat Tcw = cam_kf[i]->GetPose();                                      // Converter::toSE3Quat(pKF->GetPose())
      float T[16];
      pose_to16(Tcw, T);
      ccmh::toSE3Quat(T, &cam_qt[7 * i]);
      cam_K[4 * i] = cam_kf[i]->fx; cam_K[4 * i + 1] = cam_kf[i]->fy; cam_K[4 * i + 2] = cam_kf[i]->cx; cam_K[4 * i + 3] = cam_kf[i]->cy;
      cam_fix[i] = cam_is_fixed[i] ? 1 : 0;
    }
    if (aux_ok && pt_xyz_walk.size() == 3 * np) pt_xyz.swap(pt_xyz_walk);             // the walk already read every position (same order: no point was moved)
    else
    parallel_chunks(np, shim_threads(np), [&](int, size_t b, size_t e) {
      for (size_t i = b; i < e; i++) {
        const cv::Mat P = pt_mp[i]->GetWorldPos();                                   // Converter::toVector3d(pMP->GetWorldPos())
        const float p[3] = {P.at<float>(0), P.at<float>(1), P.at<float>(2)};
        ccmh::toVector3d(p, &pt_xyz[3 * i]);
      }
    });
    const size_t ne = e_cam_id.size();
    e_cam.resize(ne); e_pt.resize(ne);
    // ids -> indices: two table look-ups per observation (955 000 on the 4-agent map: ~7 ms on one thread), independent from edge to edge
    std::vector<char> missing((size_t)shim_threads(ne) + 1, 0);
    parallel_chunks(ne, shim_threads(ne), [&](int t, size_t b, size_t e) {
      char miss = 0;
      for (size_t k = b; k < e; k++) { const int32_t ci = cam_index.find(e_cam_id[k]); e_cam[k] = ci; e_pt[k] = pt_index.find(e_pt_id[k]); miss |= ci < 0; }
      missing[(size_t)t] = miss;
    });
    bool any_missing = false;
    for (char m : missing) any_missing |= m != 0;
    size_t w = ne;
    if (any_missing && drop_edges_without_camera) {   // (rare: an observation of a keyframe that is not a vertex) ordered compaction
      w = 0;
      for (size_t k = 0; k < ne; k++) {
        if (e_cam[k] < 0) continue;
        if (w != k) { e_cam[w] = e_cam[k]; e_pt[w] = e_pt[k]; e_cam_id[w] = e_cam_id[k]; e_pt_id[w] = e_pt_id[k]; e_obs[2 * w] = e_obs[2 * k]; e_obs[2 * w + 1] = e_obs[2 * k + 1]; e_info[w] = e_info[k]; }
        w++;
      }
    }
    e_cam.resize(w); e_pt.resize(w); e_cam_id.resize(w); e_pt_id.resize(w); e_obs.resize(2 * w); e_info.resize(w);
    e_level.assign(w, 0);
  }
  ccm_ba_problem problem(double huber) {
    ccm_ba_problem P;
    P.n_cam = (int32_t)cam_id.size(); P.n_pt = (int32_t)pt_id.size(); P.n_edge = (int32_t)e_cam.size();
    P.cam_qt = cam_qt.data(); P.cam_fixed = cam_fix.data(); P.cam_K = cam_K.data(); P.pt_xyz = pt_xyz.data();
    P.e_cam = e_cam.data(); P.e_pt = e_pt.data(); P.e_obs = e_obs.data(); P.e_info = e_info.data(); P.e_level = e_level.data();
    P.huber_delta = huber;
    return P;
  }
  cv::Mat camPose(size_t id) {                                                       // Converter::toCvMat(vSE3->estimate())
    float T[16];
    ccmh::toCvMat(&cam_qt[7 * (size_t)cam_index.find(id)], T);
    return pose_from16(T);
  }
  cv::Mat pointPos(size_t id) {                                                      // Converter::toCvMat(vPoint->estimate())
    cv::Mat m(3, 1, CV_32F);
    const size_t i = (size_t)pt_index.find(id);
    for (int c = 0; c < 3; c++) m.at<float>(c) = (float)pt_xyz[3 * i + c];
    return m;
  }
};

// optimizer.initializeOptimization(0); optimizer.optimize(n) on the device.  keep != nullptr: the handle outlives the call (*keep == nullptr: it is
// created here; otherwise the problem of the earlier call is reused: the edges whose e_level became non-zero leave, the estimate stays — the second
// stage of the local BA, Optimizer.cpp:545-566); the caller releases it with ccm_ba_destroy.
void run_ba(FlatBA& f, double huber, int iterations, bool* pbStopFlag, std::vector<double>* chi2, std::vector<uint8_t>* depth_pos, ccm_ba** keep = nullptr) {
  ccm_ba_problem P = f.problem(huber);
  ccm_ba_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.max_iters = iterations;
  if (chi2) chi2->resize(f.nEdges(), 0.0);
  if (depth_pos) depth_pos->resize(f.nEdges(), 1);
  // = ccm_ba_optimize (one rank: a one-shot call never turns into a collective), split so that the phases can be read
  ccm_ctx* ctx = thread_ctx();
  ccm_ba* ba = keep ? *keep : nullptr;
  double t = now_ms();
  if (!ba) check(ccm_ba_create(ctx, &P, 0, 1, &ba), "ccm_ba_create");
  else check(ccm_ba_set_edge_levels(ba, f.e_level.data(), huber), "ccm_ba_set_edge_levels");
  double n = now_ms(); g_phase[kCreate] += n - t; t = n;
  int rc = ccm_ba_run(ba, &opt, reinterpret_cast<const volatile unsigned char*>(pbStopFlag), nullptr);
  n = now_ms(); g_phase[kRun] += n - t; t = n;
  if (rc == CCM_OK) rc = ccm_ba_download(ba, P.cam_qt, P.pt_xyz, chi2 ? chi2->data() : nullptr);
  if (rc == CCM_OK && depth_pos) rc = ccm_ba_depth_positive(&P, P.cam_qt, P.pt_xyz, depth_pos->data());
  if (keep) *keep = ba; else ccm_ba_destroy(ba);
  g_phase[kDownload] += now_ms() - t;
  check(rc, "ccm_ba_run");
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// batched MapPoint::UpdateNormalAndDepth for the write-back of a global BA — only when MapPoint offers SetNormalAndDepth (the optional patch of
// INTEGRATION.md; the reference keeps mNormalVector / mfMinDistance / mfMaxDistance protected without a setter, MapPoint.h:286-305).  Detected at compile
// time, so this translation unit builds against the unpatched header too and then calls the reference's method per point.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, typename = void> struct has_normal_depth_setter : std::false_type {};
template <typename T>
struct has_normal_depth_setter<T, decltype(std::declval<T&>().SetNormalAndDepth(std::declval<const cv::Mat&>(), 0.0f, 0.0f), void())> : std::true_type {};
constexpr bool kBatchedNormals = has_normal_depth_setter<MapPoint>::value;

template <typename MP> void store_normal_depth(MP* p, const float* n3, float mn, float mx, std::true_type) {
  cv::Mat n(3, 1, CV_32F);
  n.at<float>(0) = n3[0]; n.at<float>(1) = n3[1]; n.at<float>(2) = n3[2];
  p->SetNormalAndDepth(n, mn, mx);
}
template <typename MP> void store_normal_depth(MP*, const float*, float, float, std::false_type) {}

// SetWorldPos + UpdateNormalAndDepth (Optimizer.cpp:843-845) of every point of the flattened problem: positions by SetWorldPos as before; normal / depth
// range of the REGULAR points (every non-bad observation is an edge of the problem, reference keyframe among its cameras) by ONE call of
// ccm_update_normal_and_depth (MapPoint.cpp:779-823 on the device, bit-exact: tests/test_frame_gpu.py) over the problem's own edge lists — a point's edges
// are in the order the walk iterated its mObservations, which is the order the reference sums in; the other points take the reference's method.
// edge_skip (local BA): observations erased after the optimisation (they are no longer in mObservations); ref_from_walk: the reference keyframe and octave
// were recorded by the graph walk (global BA: no second GetObservations()), else they are asked of the point now (local BA: EraseObservation may have moved
// mpRefKF, MapPoint.cpp:474-476); pos_lock: SetWorldPos's bLock as the reference call site passes it.
template <typename Ids>
void batched_point_writeback(FlatBA& f, const std::vector<char>* edge_skip, bool ref_from_walk, bool pos_lock) {
  const size_t np = f.pt_id.size(), nc = f.cam_id.size(), ne = f.e_pt.size();
  std::vector<float> pos(3 * np), center(3 * nc), normal(3 * np, 0.0f), dmin(np, 0.0f), dmax(np, 0.0f);
  std::vector<int32_t> off(np + 1, 0), kf(ne), ref(np, 0), lvl(np, 0);
  for (size_t i = 0; i < np; i++) for (int c = 0; c < 3; c++) pos[3 * i + c] = (float)f.pt_xyz[3 * i + c];   // what pointPos() hands to SetWorldPos
  for (size_t i = 0; i < nc; i++) {
    const cv::Mat Ow = f.cam_kf[i]->GetCameraCenter();                                                      // after the keyframe write-back
    for (int c = 0; c < 3; c++) center[3 * i + c] = Ow.at<float>(c);
  }
  for (size_t k = 0; k < ne; k++) if (!edge_skip || !(*edge_skip)[k]) off[(size_t)f.e_pt[k] + 1]++;
  for (size_t i = 0; i < np; i++) off[i + 1] += off[i];
  {
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (size_t k = 0; k < ne; k++) if (!edge_skip || !(*edge_skip)[k]) kf[(size_t)fill[(size_t)f.e_pt[k]]++] = f.e_cam[k];   // stable: the walk's order inside a point
  }
  std::vector<char> regular(np, 0);
  for (size_t i = 0; i < np; i++) {
    int32_t r = -1;
    if (ref_from_walk) { r = f.pt_regular[i] ? f.cam_index.find(f.pt_ref_cam_id[i]) : -1; lvl[i] = f.pt_ref_level[i]; }
    else if (!f.pt_mp[i]->isBad()) {
      const Optimizer::kfptr pRef = f.pt_mp[i]->GetReferenceKeyFrame();
      const int idx = pRef ? f.pt_mp[i]->GetIndexInKeyFrame(pRef) : -1;
      if (pRef && idx >= 0) { r = f.cam_index.find(Ids::of(*pRef)); lvl[i] = pRef->mvKeysUn[idx].octave; }
    }
    regular[i] = r >= 0 && off[i + 1] > off[i];
    ref[i] = r >= 0 ? r : 0;
  }
  const std::vector<float>& sf = f.cam_kf[0]->mvScaleFactors;                                                // one table per map (ORBextractor parameters)
  check(ccm_update_normal_and_depth(thread_ctx(), (int)np, pos.data(), off.data(), kf.data(), (int)nc, center.data(), ref.data(), lvl.data(), sf.data(),
                                    (int)f.cam_kf[0]->mnScaleLevels, normal.data(), dmin.data(), dmax.data()), "ccm_update_normal_and_depth");
  parallel_chunks(np, shim_threads(np, 32), [&](int, size_t b, size_t e) {
    for (size_t i = b; i < e; i++) {
      MapPoint* pMP = f.pt_mp[i];
      if (pMP->isBad()) continue;
      cv::Mat p(3, 1, CV_32F);
      for (int c = 0; c < 3; c++) p.at<float>(c) = pos[3 * i + c];
      // A point whose position is locked may ignore the write (MapPoint::SetWorldPos returns early on a CLIENT, MapPoint.cpp:340-341): the batch values were
      // computed from the NEW position, so such a point takes the reference's own per-point method, which reads whatever position the point really has.
      const bool locked = pMP->IsPosLocked();
      pMP->SetWorldPos(p, pos_lock);
      if (regular[i] && !locked) store_normal_depth(pMP, &normal[3 * i], dmin[i], dmax[i], has_normal_depth_setter<MapPoint>());
      else pMP->UpdateNormalAndDepth();
    }
  });
}


// ---------------------------------------------------------------------------------------------------------------------------------
// write-back of a global bundle adjustment (BundleAdjustmentClient, MapFusionGBA)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
// Where the result goes.  direct: into the map itself (SetPose / SetWorldPos + UpdateNormalAndDepth, with the call site's bLock); otherwise a loop closure
// is waiting for it: poses and positions are parked in mTcwGBA / mPosGBA under the tag of that loop's keyframe and the map stays as it is.
struct GbaSink {
  bool direct, lock;
  idpair tag;
};

template <typename Ids>
void gba_write_keyframes(FlatBA& f, const std::vector<Optimizer::kfptr>& kfs, const GbaSink& to) {
  for (const Optimizer::kfptr& kf : kfs) {
    if (kf->isBad()) continue;
    const cv::Mat pose = f.camPose(Ids::of(*kf));
    if (to.direct) kf->SetPose(pose, to.lock);
    else {
      kf->mTcwGBA.create(4, 4, CV_32F);
      pose.copyTo(kf->mTcwGBA);
      kf->mBAGlobalForKF = to.tag;
    }
  }
}

// included[i]: point i became a vertex.  done(i) runs on the thread that has just worked on point i, whether or not it was written.
template <typename Ids, typename Done>
void gba_write_points(FlatBA& f, const std::vector<Optimizer::mpptr>& pts, const std::vector<char>& included, const GbaSink& to, int n_threads, Done done) {
  parallel_chunks(pts.size(), n_threads, [&](int, size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; i++) {
      MapPoint* mp = pts[i].get();
      if (included[i] && !mp->isBad()) {
        const cv::Mat pos = f.pointPos(Ids::of(*mp));
        if (to.direct) {
          mp->SetWorldPos(pos, to.lock);
          mp->UpdateNormalAndDepth();
        } else {
          mp->mPosGBA.create(3, 1, CV_32F);
          pos.copyTo(mp->mPosGBA);
          mp->mBAGlobalForKF = to.tag;
        }
      }
      done(i);
    }
  });
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// client side
// ---------------------------------------------------------------------------------------------------------------------------------
void Optimizer::GlobalBundleAdjustemntClient(mapptr pMap, size_t ClientId, int nIterations, bool* pbStopFlag, const idpair nLoopKF, const bool bRobust) {
  BundleAdjustmentClient(pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), ClientId, nIterations, pbStopFlag, nLoopKF, bRobust);
}

void Optimizer::BundleAdjustmentClient(const vector<kfptr>& vpKFs, const vector<mpptr>& vpMP, size_t ClientId, int nIterations, bool* pbStopFlag,
                                       const idpair nLoopKF, const bool bRobust) {
  const char* me = "Optimizer::BundleAdjustmentClient";
  const idpair origin(0, ClientId);                       // the client's first keyframe: the fixed camera, and as nLoopKF the sign for "no loop is waiting"
  FlatBA f;
  for (const kfptr& kf : vpKFs) {
    if (kf->isBad()) continue;
    require_id_below_range(me, "keyframe", kf->mId);
    f.addCam(ClientIds::of(*kf), kf, kf->mId == origin);
  }
  std::vector<char> included(vpMP.size(), 0);
  for (size_t i = 0; i < vpMP.size(); i++) {
    const mpptr& mp = vpMP[i];
    if (mp->isBad()) continue;
    require_id_below_range(me, "map point", mp->mId);
    included[i] = 0 < f.addPointWithEdges<ClientIds>(mp, mp->GetObservations(), 1, [&](const kfptr& kf) {
      if (kf->isBad()) return false;
      require_id_below_range(me, "keyframe", kf->mId);
      return true;
    });
  }
  f.flatten(true);
  const float thHuber2D = sqrt(5.99);
  run_ba(f, bRobust ? (double)thHuber2D : 0.0, nIterations, pbStopFlag, nullptr, nullptr);
  const GbaSink to{nLoopKF == origin, false, nLoopKF};
  gba_write_keyframes<ClientIds>(f, vpKFs, to);
  gba_write_points<ClientIds>(f, vpMP, included, to, 1, [](size_t) {});
}

int Optimizer::PoseOptimizationClient(Frame& Frame) {
  float T[16];
  pose_to16(Frame.mTcw, T);
  double cam_qt[7];
  ccmh::toSE3Quat(T, cam_qt);                                                         // Converter::toSE3Quat(Frame.mTcw)
  std::vector<double> Xw, obs, info;
  std::vector<int> slot;                                                              // per edge: index into the frame's keypoints
  {
    unique_lock<mutex> lock(MapPoint::mGlobalMutex);
    for (int i = 0; i < Frame.N; i++) {
      const mpptr& mp = Frame.mvpMapPoints[i];
      if (!mp) continue;
      Frame.mvbOutlier[i] = false;
      const cv::KeyPoint& kp = Frame.mvKeysUn[i];
      const cv::Mat P = mp->GetWorldPos();
      obs.insert(obs.end(), {kp.pt.x, kp.pt.y});
      info.push_back(Frame.mvInvLevelSigma2[kp.octave]);
      Xw.insert(Xw.end(), {P.at<float>(0), P.at<float>(1), P.at<float>(2)});
      slot.push_back(i);
    }
  }
  if (slot.size() < 3) return 0;
  const double K[4] = {Frame.fx, Frame.fy, Frame.cx, Frame.cy};
  std::vector<uint8_t> outlier(slot.size(), 0);
  int nInliers = 0;
  // the reference's four rounds of 10 iterations with their inlier / outlier reclassification run inside one kernel launch
  check(ccm_pose_optimize(thread_ctx(), cam_qt, (int)slot.size(), Xw.data(), obs.data(), info.data(), K, outlier.data(), &nInliers), "ccm_pose_optimize");
  for (size_t e = 0; e < slot.size(); e++) Frame.mvbOutlier[slot[e]] = outlier[e] != 0;
  ccmh::toCvMat(cam_qt, T);                                                           // Converter::toCvMat(SE3quat_recov)
  Frame.SetPose(pose_from16(T));
  return nInliers;
}

void Optimizer::LocalBundleAdjustmentClient(kfptr pKF, bool* pbStopFlag, mapptr pMap, size_t ClientId, eSystemState SysState) {
  const char* me = "Optimizer::LocalBundleAdjustmentClient";
  PhaseClock pc;
  // The window, as three vectors plus the tags the walk leaves on the objects (other code reads them, and they are how an object is met only once):
  // local keyframes = the current one and its covisible neighbours; local points = what they see; fixed cameras = whoever else sees a local point.
  // A bad neighbour is tagged but stays out.
  const idpair tag = pKF->mId;
  std::vector<kfptr> local_kfs(1, pKF), fixed_kfs;
  std::vector<mpptr> local_mps;
  pKF->mBALocalForKF = tag;
  for (const kfptr& kf : pKF->GetVectorCovisibleKeyFrames()) {
    kf->mBALocalForKF = tag;
    if (!kf->isBad()) local_kfs.push_back(kf);
  }
  for (const kfptr& kf : local_kfs)
    for (const mpptr& mp : kf->GetMapPointMatches())
      if (mp && !mp->isBad() && mp->mBALocalForKF != tag) {
        mp->mBALocalForKF = tag;
        local_mps.push_back(mp);
      }
  for (const mpptr& mp : local_mps)
    for (const auto& ob : mp->GetObservations()) {
      const kfptr& kf = ob.first;
      if (kf->mBALocalForKF == tag || kf->mBAFixedForKF == tag) continue;
      kf->mBAFixedForKF = tag;
      if (!kf->isBad()) fixed_kfs.push_back(kf);
    }
  FlatBA f;
  for (const kfptr& kf : local_kfs) {
    require_id_below_range(me, "keyframe", kf->mId);
    f.addCam(ClientIds::of(*kf), kf, kf->mId == idpair(0, ClientId));
  }
  for (const kfptr& kf : fixed_kfs) {
    require_id_below_range(me, "keyframe", kf->mId);
    f.addCam(ClientIds::of(*kf), kf, true);
  }
  for (const mpptr& mp : local_mps) {
    require_id_below_range(me, "map point", mp->mId);
    f.addPointWithEdges<ClientIds>(mp, mp->GetObservations(), 0, [&](const kfptr& kf) {
      require_id_below_range(me, "keyframe", kf->mId);
      return !kf->isBad();
    });
  }
  if (pbStopFlag && *pbStopFlag) return;                 // nothing has been flattened or written
  pc.lap(kWalk);
  f.flatten();
  pc.lap(kFlatten);
  // From here on an edge is an index: f.cam_kf[f.e_cam[i]] is its keyframe, f.pt_mp[f.e_pt[i]] its point (every index is valid: ccm_ba_create refuses a
  // problem with an edge whose camera or point is not a vertex).
  const size_t n_edges = f.nEdges();
  std::vector<double> chi2;
  std::vector<uint8_t> dpos;
  auto point_of = [&](size_t i) { return f.pt_mp[(size_t)f.e_pt[i]]; };
  auto outlier_of_live_point = [&](size_t i) { return !point_of(i)->isBad() && is_outlier(chi2[i], dpos[i]); };
  // 5 robust iterations; then, unless asked to stop, the outliers leave the problem (level 1; their chi2 keeps the value of the first pass) and 10
  // iterations without the robust kernel follow — both on one device-side problem
  struct Handle { ccm_ba* h = nullptr; ~Handle() { if (h) ccm_ba_destroy(h); } } session;
  const float thHuberMono = sqrt(5.991);
  run_ba(f, (double)thHuberMono, 5, pbStopFlag, &chi2, &dpos, &session.h);
  if (!(pbStopFlag && *pbStopFlag)) {
    for (size_t i = 0; i < n_edges; i++) if (outlier_of_live_point(i)) f.e_level[i] = 1;
    run_ba(f, 0.0, 10, pbStopFlag, &chi2, &dpos, &session.h);
  }
  pc.restart();
  std::vector<size_t> erase;                              // edge indices, in edge order; chosen before the wait for the map
  for (size_t i = 0; i < n_edges; i++) if (outlier_of_live_point(i)) erase.push_back(i);
  if (SysState != eSystemState::SERVER)
    while (!pMap->LockMapUpdate()) { usleep(params::timings::miLockSleep); }
  for (size_t i : erase) {
    const kfptr& kf = f.cam_kf[(size_t)f.e_cam[i]];
    const mpptr mp = point_of(i)->shared_from_this();
    kf->EraseMapPointMatch(mp);
    mp->EraseObservation(kf);
  }
  for (const kfptr& kf : local_kfs) {
    kf->SetPose(f.camPose(ClientIds::of(*kf)), false);
    kf->mbUpdatedByServer = false;
  }
  pc.lap(kKfWriteback);
  // A local point that is bad by now was erased from the map by its last EraseObservation; one that the map still holds is an inconsistency.
  auto alive = [&](const mpptr& mp) {
    if (mp->isBad() && pMap->GetMpPtr(mp->mId)) shim_fatal(me, "a local map point is flagged bad but the map still holds it");
    return !mp->isBad();
  };
  if (kBatchedNormals && !f.cam_kf.empty() && !f.pt_id.empty()) {
    // (with the optional MapPoint::SetNormalAndDepth) positions as below, normals and distance ranges of all local points by one device call over the
    // problem's edges minus the erased observations (an observation whose point turned bad belongs to a point the helper skips)
    for (const mpptr& mp : local_mps) alive(mp);
    std::vector<char> erased(n_edges, 0);
    for (size_t i = 0; i < n_edges; i++) erased[i] = point_of(i)->isBad() || is_outlier(chi2[i], dpos[i]);
    batched_point_writeback<ClientIds>(f, &erased, false, false);
  } else
    for (const mpptr& mp : local_mps)
      if (alive(mp)) {
        mp->SetWorldPos(f.pointPos(ClientIds::of(*mp)), false);
        mp->UpdateNormalAndDepth();
      }
  pc.lap(kMpWriteback);
  if (SysState != eSystemState::SERVER) pMap->UnLockMapUpdate();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// server side
// ---------------------------------------------------------------------------------------------------------------------------------
void Optimizer::MapFusionGBA(mapptr pMap, size_t ClientId, int nIterations, bool* pbStopFlag, idpair nLoopKF, const bool bRobust) {
  (void)ClientId;
  PhaseClock pc;
  {   // (everything the call owns lives in this scope, so that what its destructors cost is inside the last phase, not after it)
  vector<kfptr> vpKFs = pMap->GetAllKeyFrames();
  vector<mpptr> vpMP = pMap->GetAllMapPoints();
  if (pMap->mvpKeyFrameOrigins.empty()) shim_fatal("Optimizer::MapFusionGBA", "the map has no origin keyframe (mvpKeyFrameOrigins is empty)");
  const idpair FixedId = pMap->mvpKeyFrameOrigins.front()->mId;
  std::vector<char> included(vpMP.size(), 0);   // one byte per point: chunks of vpMP are walked by different threads
  static thread_local FlatBA f_keep;
  static thread_local std::vector<FlatBA> part_keep;
  FlatBA& f = f_keep;
  f.reset();
  // the flat arrays keep their capacity from call to call (per thread); the references into the caller's object graph do not outlive the call: a keyframe
  // erased from the map afterwards is destroyed when the reference would destroy it
  struct DropRefs {
    FlatBA& a; std::vector<FlatBA>& parts;
    ~DropRefs() { a.cam_kf.clear(); a.pt_mp.clear(); for (auto& g : parts) { g.cam_kf.clear(); g.pt_mp.clear(); } }
  } drop_refs{f_keep, part_keep};
  size_t maxKFid = 0;
  for (const kfptr& kf : vpKFs) {
    if (kf->isBad()) continue;
    f.addCam(kf->mUniqueId, kf, kf->mId == FixedId);
    maxKFid = std::max(maxKFid, (size_t)kf->mUniqueId);
  }
  pc.lap(kVertices);
  {
    // the map points in contiguous chunks of vpMP, one chunk per host thread (every point is independent; GetObservations() copies under the point's
    // own mutex exactly as in the reference); the chunks are appended in order, so vertices and edges keep the order of the sequential walk
    const int n_thr = shim_threads(vpMP.size());
    std::vector<FlatBA>& part = part_keep;
    if (part.size() < (size_t)n_thr) part.resize((size_t)n_thr);
    for (auto& g : part) g.reset();
    // an observation counts when its keyframe is a vertex: alive, and not newer than the newest keyframe this call has seen
    auto is_vertex = [&](const kfptr& kf) { return kf && !kf->isBad() && kf->mUniqueId <= maxKFid; };
    parallel_chunks(vpMP.size(), n_thr, [&](int t, size_t i0, size_t i1) {
      FlatBA& g = t == 0 ? f : part[(size_t)t];
      for (size_t i = i0; i < i1; i++) {
        const mpptr& mp = vpMP[i];
        if (mp->isBad()) continue;
        const map<kfptr, size_t> observations = mp->GetObservations();
        if (observations.size() < 2) continue;
        const int nEdges = g.addPointWithEdges<UniqueIds>(mp, observations, 2, is_vertex);   // a point needs two views to be constrained
        if (nEdges == 0) continue;
        included[i] = 1;
        g.addPointPos(mp->GetWorldPos());   // (the vertex estimate: read here, while this thread has the point's lines, instead of in a second pass over all points)
        if (kBatchedNormals) {   // what the batched UpdateNormalAndDepth of the write-back needs beside the edges
          int nLive = 0;         // observations the reference's method would use (non-bad keyframes): all of them must be edges
          for (const auto& ob : observations) if (ob.first && !ob.first->isBad()) nLive++;
          const kfptr pRef = mp->GetReferenceKeyFrame();
          const auto rit = pRef ? observations.find(pRef) : observations.end();
          const bool regular = nLive == nEdges && is_vertex(pRef) && rit != observations.end();
          g.addPointAux(regular ? pRef->mUniqueId : 0, regular ? pRef->mvKeysUn[rit->second].octave : 0, regular);
        }
      }
    });
    for (int t = 1; t < n_thr; t++) f.append(part[(size_t)t]);
  }
  pc.lap(kWalk);
  f.flatten(true);
  pc.lap(kFlatten);
  const float thHuber2D = sqrt(5.99);
  run_ba(f, bRobust ? (double)thHuber2D : 0.0, nIterations, pbStopFlag, nullptr, nullptr);
  pc.restart();
  const GbaSink to{nLoopKF == idpair(0, pMap->mMapId), true, nLoopKF};
  gba_write_keyframes<UniqueIds>(f, vpKFs, to);
  pc.lap(kKfWriteback);
  // every keyframe has its new pose: the per-point write-back (SetWorldPos + UpdateNormalAndDepth, 150 000 mutex-taking calls after a merge of four
  // agents) is independent from point to point
  const bool batched = kBatchedNormals && to.direct && f.aux_ok && f.pt_regular.size() == f.pt_id.size() && !f.cam_kf.empty();
  if (batched) batched_point_writeback<UniqueIds>(f, nullptr, true, true);
  else
    // (measured on the reference's REAL classes, 150 000 points: 63 - 78 ms for this loop on 32 threads against 18 on the look-alike — the real SetWorldPos takes the
    // process-wide MapPoint::mGlobalMutex (MapPoint.cpp:343) and the real UpdateNormalAndDepth two mutexes of every observing keyframe (isBad, GetCameraCenter).  Tried
    // and dropped: all positions on one thread with the normals following behind it (67 ms: the call itself is ~450 ns), positions on four threads then normals on all (66 - 82 ms).)
    // This call's copy of each pointer (Map::GetAllMapPoints() hands out 150 000 of them by value) is dropped by the thread that has just worked on the point:
    // releasing them in one go afterwards cost 13 - 30 ms on the 4-agent map (one lock-prefixed decrement per point on a line some other core holds)
    gba_write_points<UniqueIds>(f, vpMP, included, to, shim_threads(vpMP.size(), 32), [&](size_t i) { vpMP[i].reset(); });
  pc.lap(kMpWriteback);
  f.cam_kf.clear(); f.pt_mp.clear();   // no keyframe / map point is kept alive between calls; the flat arrays stay allocated
  pc.lap(kRelease);
  // the copies Map::GetAllMapPoints() / GetAllKeyFrames() handed out by value: released on several threads and INSIDE the phase clock (round 5: their
  // destructors used to run after the last lap, 29 ms that no phase showed)
  if (batched) release_refs(vpMP);
  release_refs(vpKFs);
  }
  pc.lap(kScopeExit);
}

int Optimizer::OptimizeSim3(kfptr pKF1, kfptr pKF2, std::vector<mpptr>& vpMatches1, g2o::Sim3& g2oS12, const float th2, bool bFixScale) {
  // one side of the two-view problem: its pose and intrinsics, and per correspondence the point in its camera frame, the keypoint and its information
  struct View {
    const kfptr& kf;
    const cv::Mat R, t;
    std::vector<double> Pc, obs, info;
    explicit View(const kfptr& k) : kf(k), R(k->GetRotation()), t(k->GetTranslation()) {}
    void add(const mpptr& mp, size_t kp) {
      const cv::Mat P = R * mp->GetWorldPos() + t;        // the cv::Mat arithmetic stays with the caller's data types (f32)
      Pc.insert(Pc.end(), {P.at<float>(0), P.at<float>(1), P.at<float>(2)});
      const cv::KeyPoint& k = kf->mvKeysUn[kp];
      obs.insert(obs.end(), {k.pt.x, k.pt.y});
      info.push_back(kf->mvInvLevelSigma2[k.octave]);
    }
    void intrinsics(double k4[4]) const { const cv::Mat& K = kf->mK; k4[0] = K.at<float>(0, 0); k4[1] = K.at<float>(1, 1); k4[2] = K.at<float>(0, 2); k4[3] = K.at<float>(1, 2); }
  } v1(pKF1), v2(pKF2);
  const vector<mpptr> vpMapPoints1 = pKF1->GetMapPointMatches();
  std::vector<size_t> slot;                               // per correspondence: index into vpMatches1
  for (size_t i = 0; i < vpMatches1.size(); i++) {
    const mpptr& mp2 = vpMatches1[i];
    if (!mp2) continue;
    const mpptr& mp1 = vpMapPoints1[i];
    const int i2 = mp2->GetIndexInKeyFrame(pKF2);
    if (!mp1 || mp1->isBad() || mp2->isBad() || i2 < 0) continue;
    v1.add(mp1, i);
    v2.add(mp2, (size_t)i2);
    slot.push_back(i);
  }
  double k1[4], k2[4], s8[8] = {g2oS12.rotation().x(), g2oS12.rotation().y(), g2oS12.rotation().z(), g2oS12.rotation().w(),
                                g2oS12.translation()[0], g2oS12.translation()[1], g2oS12.translation()[2], g2oS12.scale()};
  v1.intrinsics(k1); v2.intrinsics(k2);
  std::vector<uint8_t> keep(slot.size(), 1);
  int nIn = 0;
  check(ccm_sim3_optimize(thread_ctx(), s8, (int)slot.size(), v1.Pc.data(), v2.Pc.data(), v1.obs.data(), v2.obs.data(), v1.info.data(), v2.info.data(), k1, k2,
                          (double)th2, bFixScale ? 1 : 0, keep.data(), &nIn),
        "ccm_sim3_optimize");
  for (size_t e = 0; e < slot.size(); e++) if (!keep[e]) vpMatches1[slot[e]] = static_cast<mpptr>(NULL);
  if (nIn == 0) return 0;   // fewer than 10 survivors after the first pass: g2oS12 stays as it was
  g2oS12 = g2o::Sim3(Eigen::Quaterniond(s8[3], s8[0], s8[1], s8[2]), Eigen::Vector3d(s8[4], s8[5], s8[6]), s8[7]);
  return nIn;
}

namespace {
typedef std::vector<g2o::Sim3, Eigen::aligned_allocator<g2o::Sim3> > Sim3Vec;
void sim3_to8(const g2o::Sim3& S, double* p) {
  p[0] = S.rotation().x(); p[1] = S.rotation().y(); p[2] = S.rotation().z(); p[3] = S.rotation().w();
  p[4] = S.translation()[0]; p[5] = S.translation()[1]; p[6] = S.translation()[2]; p[7] = S.scale();
}
// edge list of an essential graph + the device call; vertices are indexed by mUniqueId
struct PoseGraph {
  std::vector<int32_t> e_i, e_j;
  std::vector<double> meas;
  void addEdge(size_t i, size_t j, const g2o::Sim3& Sji) { e_i.push_back((int32_t)i); e_j.push_back((int32_t)j); meas.resize(meas.size() + 8); sim3_to8(Sji, &meas[meas.size() - 8]); }
  // optimizer.initializeOptimization(); optimizer.optimize(20) with setUserLambdaInit(1e-16): vertices = the keyframes that were added (`present`)
  void optimize(const Sim3Vec& vScw, const std::vector<char>& present, size_t fixed_uid, bool bFixScale, Sim3Vec& out) {
    const size_t n = vScw.size();
    std::vector<int32_t> slot(n, -1);
    std::vector<double> sim3;
    std::vector<uint8_t> fixed;
    int nv = 0;
    for (size_t u = 0; u < n; u++) if (present[u]) { slot[u] = nv++; sim3.resize(sim3.size() + 8); sim3_to8(vScw[u], &sim3[sim3.size() - 8]); fixed.push_back(u == fixed_uid ? 1 : 0); }
    std::vector<int32_t> ei(e_i.size()), ej(e_j.size());
    for (size_t k = 0; k < e_i.size(); k++) { ei[k] = slot[e_i[k]]; ej[k] = slot[e_j[k]]; }
    check(ccm_pose_graph_optimize(thread_ctx(), nv, sim3.data(), fixed.data(), bFixScale ? 1 : 0, (int)ei.size(), ei.data(), ej.data(), meas.data(), 20, 1e-16, nullptr,
                                  nullptr),
          "ccm_pose_graph_optimize");
    out = vScw;
    for (size_t u = 0; u < n; u++) if (present[u]) { const double* p = &sim3[8 * (size_t)slot[u]]; out[u] = g2o::Sim3(Eigen::Quaterniond(p[3], p[0], p[1], p[2]), Eigen::Vector3d(p[4], p[5], p[6]), p[7]); }
  }
};
cv::Mat sim3_pose(const g2o::Sim3& Siw) {   // [R t/s; 0 1]
  double s8[8];
  sim3_to8(Siw, s8);
  float T[16];
  ccmh::sim3ToCvSE3(s8, T);
  return pose_from16(T);
}

// THE essential-graph optimisation, for a closed loop and for a map fusion.  `corrected` holds the Sim3 a loop closure has already given some keyframes (the
// initial estimate of those vertices), `uncorrected` the poses the same keyframes had before it (what the relative measurements of their edges are taken
// from); a map fusion has neither.  tagged_by / tagged_ref: the MapPoint members in which the correction step that ran before recorded, per point, for which
// current keyframe and relative to which keyframe it moved the point (the _LC pair or the _MM pair).
void optimize_essential_graph(Optimizer::mapptr pMap, Optimizer::kfptr pLoopKF, Optimizer::kfptr pCurKF, const Optimizer::KeyFrameAndPose* uncorrected,
                              const Optimizer::KeyFrameAndPose* corrected, const map<Optimizer::kfptr, set<Optimizer::kfptr> >& LoopConnections, bool bFixScale,
                              idpair MapPoint::*tagged_by, size_t MapPoint::*tagged_ref) {
  typedef Optimizer::kfptr kfptr;
  const vector<kfptr> kfs = pMap->GetAllKeyFrames();
  const vector<Optimizer::mpptr> mps = pMap->GetAllMapPoints();
  const int minFeat = params::opt::miEssGraphMinFeats;
  // 1. tables per mUniqueId: present (a vertex: the keyframe is alive), Scw (initial estimate: the corrected Sim3 where there is one, else the pose at scale 1)
  //    and Smw (the pose that measurements are composed from: the uncorrected Sim3 where there is one, else Scw).  A slot nobody fills is the identity.
  const size_t n = (size_t)pMap->GetMaxKFidUnique() + 1;
  Sim3Vec Scw(n), Smw;
  std::vector<char> present(n, 0);
  for (const kfptr& kf : kfs) {
    if (kf->isBad()) continue;
    const auto it = corrected->find(kf);
    Scw[kf->mUniqueId] = it != corrected->end() ? it->second : g2o::Sim3(Converter::toMatrix3d(kf->GetRotation()), Converter::toVector3d(kf->GetTranslation()), 1.0);
    present[kf->mUniqueId] = 1;
  }
  Smw = Scw;
  for (const auto& e : *uncorrected) if (e.first->mUniqueId < n) Smw[e.first->mUniqueId] = e.second;
  // 2. edges i -> j with the measurement Sji = Sjw * Swi.  The loop's own connections first, between the CORRECTED poses; then per keyframe, between the
  //    measurement poses: its parent in the spanning tree, its older loop edges, its older strong covisibility neighbours that are not yet connected.
  PoseGraph pg;
  set<pair<size_t, size_t> > connected;
  for (const auto& lc : LoopConnections) {
    const kfptr& kf = lc.first;
    if (kf->isBad()) continue;
    const size_t i = kf->mUniqueId;
    const g2o::Sim3 Swi = Scw[i].inverse();
    for (const kfptr& other : lc.second) {
      if (other->isBad()) continue;
      const size_t j = other->mUniqueId;
      const bool the_loop_itself = i == pCurKF->mUniqueId && j == pLoopKF->mUniqueId;
      if (!the_loop_itself && kf->GetWeight(other) < minFeat) continue;
      pg.addEdge(i, j, Scw[j] * Swi);
      connected.insert(std::minmax(i, j));
    }
  }
  for (const kfptr& kf : kfs) {
    const size_t i = kf->mUniqueId;
    const g2o::Sim3 Swi = Smw[i].inverse();
    const kfptr parent = kf->GetParent();
    if (parent) pg.addEdge(i, parent->mUniqueId, Smw[parent->mUniqueId] * Swi);
    const set<kfptr> loop_edges = kf->GetLoopEdges();
    for (const kfptr& other : loop_edges) {
      const size_t j = other->mUniqueId;
      if (j < i) pg.addEdge(i, j, Smw[j] * Swi);
    }
    for (const kfptr& other : kf->GetCovisiblesByWeight(minFeat)) {
      if (other->isBad() || other == parent || kf->hasChild(other) || loop_edges.count(other)) continue;
      const size_t j = other->mUniqueId;
      if (j < i && !connected.count(std::minmax(i, j))) pg.addEdge(i, j, Smw[j] * Swi);
    }
  }
  Sim3Vec Siw;                                             // optimised; what was no vertex keeps its Scw
  pg.optimize(Scw, present, pLoopKF->mUniqueId, bFixScale, Siw);
  // 3. write-back: every keyframe gets [R t/s]; every point moves with its reference keyframe: out of the old frame (Scw) and back through the new one
  Sim3Vec Swi(n);
  for (const kfptr& kf : kfs) {
    Swi[kf->mUniqueId] = Siw[kf->mUniqueId].inverse();
    kf->SetPose(sim3_pose(Siw[kf->mUniqueId]), true);
  }
  for (const Optimizer::mpptr& mp : mps) {
    if (mp->isBad()) continue;
    const MapPoint& p = *mp;
    const size_t r = p.*tagged_by == pCurKF->mId ? (size_t)(p.*tagged_ref) : (size_t)mp->GetReferenceKeyFrame()->mUniqueId;
    const Eigen::Matrix<double, 3, 1> Pw = Converter::toVector3d(mp->GetWorldPos());
    mp->SetWorldPos(Converter::toCvMat(Swi[r].map(Scw[r].map(Pw))), true);
    mp->UpdateNormalAndDepth();
  }
}
}  // namespace

void Optimizer::OptimizeEssentialGraphLoopClosure(mapptr pMap, kfptr pLoopKF, kfptr pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
                                                  const KeyFrameAndPose& CorrectedSim3, const map<kfptr, set<kfptr> >& LoopConnections, const bool& bFixScale) {
  optimize_essential_graph(pMap, pLoopKF, pCurKF, &NonCorrectedSim3, &CorrectedSim3, LoopConnections, bFixScale, &MapPoint::mCorrectedByKF_LC, &MapPoint::mCorrectedReference_LC);
}

void Optimizer::OptimizeEssentialGraphMapFusion(mapptr pMap, kfptr pLoopKF, kfptr pCurKF, const map<kfptr, set<kfptr> >& LoopConnections, const bool& bFixScale) {
  const KeyFrameAndPose none;
  optimize_essential_graph(pMap, pLoopKF, pCurKF, &none, &none, LoopConnections, bFixScale, &MapPoint::mCorrectedByKF_MM, &MapPoint::mCorrectedReference_MM);
}

}  // namespace cslam

// phases (ms) of the last LocalBundleAdjustmentClient / MapFusionGBA call of the calling thread, see g_phase above
extern "C" void ccm_shim_last_phases(double* out10) { for (int i = 0; i < 10; i++) out10[i] = cslam::g_phase[i]; }
// all phases: fills min(cap, 12) entries, returns 12
extern "C" int ccm_shim_phases(double* out, int cap) { for (int i = 0; i < cap && i < cslam::kPhases; i++) out[i] = cslam::g_phase[i]; return cslam::kPhases; }
