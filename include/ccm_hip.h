/*
 * ccm_hip.h — C ABI of libccm_hip.so, the MI355X (gfx950) back end for CCM-SLAM's
 * ORB-extract / Hamming-match / bundle-adjustment hot path.
 *
 * The reference has no FFI for this path: cslam::ORBextractor, cslam::ORBmatcher and
 * cslam::Optimizer are concrete C++ classes (cslam/include/cslam/ORBextractor.h:103-138,
 * ORBmatcher.h:100-139, Optimizer.h:84-112).  The drop-in replaces their three translation
 * units with the drop-in translation units under shim/ ({Optimizer,ORBextractor,ORBmatcher}_hip.cpp,
 * compiled against the reference's own headers), which flatten the shared_ptr graph into the POD
 * buffers below and call this ABI (matchers: through the host mirror ccm_slam_amd/host/).  Every
 * entry point cites the reference code it stands for.
 *
 * Conventions
 *   - plain C, POD only, caller-owned memory, no exceptions across the boundary;
 *   - return value: 0 = ok, <0 = error (CCM_E_*); ccm_last_error() gives a message;
 *   - handle based and re-entrant: one ccm_ctx per calling thread (own HIP stream);
 *     a ctx must not be used from two threads at once (reference threading: SURVEY §8b).
 *     Any number of contexts of ONE process may work on one device at the same time — the
 *     reference runs Tracking, LocalMapping and one global-BA thread per Map concurrently
 *     (ClientHandler.cpp:184, Map.cpp:1401-1402, LoopFinder.cpp:686-688): launches that need the
 *     whole device to themselves (the persistent reduced solve of ccm_ba_run) are put in order on
 *     the GPU by a per-device lease, see ccm_coresidency_stats;
 *   - "host" entry points take host pointers and do their own H2D/D2H; "_dev" entry points
 *     take device pointers obtained from ccm_dev_alloc (used by bench.py so that inputs are
 *     resident in HBM when the timed region starts).
 */
#ifndef CCM_HIP_H
#define CCM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCM_OK            0
#define CCM_E_ARG        -1   /* bad argument                                   */
#define CCM_E_HIP        -2   /* HIP runtime error (message in ccm_last_error)   */
#define CCM_E_NOGPU      -3   /* no gfx950 device visible: the product never falls back to CPU */
#define CCM_E_NUMERIC    -4   /* reduced system not positive definite / NaN      */
#define CCM_E_COMM       -5   /* RCCL error                                      */
#define CCM_E_STATE      -6   /* call sequence error                             */

typedef struct ccm_ctx ccm_ctx;

/* ---- context ------------------------------------------------------------------------- */
int         ccm_ctx_create(int device_id, ccm_ctx** out);
void        ccm_ctx_destroy(ccm_ctx* ctx);
const char* ccm_last_error(const ccm_ctx* ctx);   /* ctx may be NULL: last global error */
int         ccm_ctx_sync(ccm_ctx* ctx);           /* hipStreamSynchronize on the ctx stream */
int         ccm_device_count(void);
/* library/build identification, e.g. "ccm_hip 0.1 gfx950" */
const char* ccm_version(void);
/* The per-device lease of this process (all pointers nullable): launches = kernels launched under it (each needs all its workgroups
 * co-resident: the persistent PCG of a 33 .. 2048-camera bundle adjustment), chained = those that were ordered behind another
 * context's launch by an event wait on their own stream (no host thread blocks), aborted = those that still gave up waiting for their
 * peers — the trial is then repeated on the multi-kernel solver and the handle returns to the persistent one a few trials later —,
 * contexts = live contexts on the device.  Two PROCESSES sharing one device are not covered: give each its own GPU (north_star: one
 * agent per GPU) or run one of them with CCM_BA_NO_PERSIST=1. */
int         ccm_coresidency_stats(int device_id, int64_t* launches, int64_t* chained, int64_t* aborted, int* contexts);

/* device memory owned by the ctx' device (thin wrappers so callers need no HIP headers) */
int ccm_dev_alloc(ccm_ctx* ctx, size_t bytes, void** dptr);
int ccm_dev_free(ccm_ctx* ctx, void* dptr);
int ccm_memcpy_h2d(ccm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int ccm_memcpy_d2h(ccm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- per-kernel timing with HIP events on the ctx stream ------------------------------
 * bench.py's roofline leg: when enabled, every launch of the selected kernel class is
 * bracketed by hipEventRecord on the launching stream; ccm_prof_read drains the events and
 * returns launches and summed milliseconds since the last ccm_prof_reset.               */
/* Classes, not kernels.  ORB: CCM_K_PYR_RESIZE = orb_pyramid_kernel (all levels of a frame in one launch), CCM_K_FAST_NMS = orb_cells_kernel (per 30-px cell:
 * FAST-9/16 score, 3x3 NMS, the minThFAST retry) AND orb_octree_kernel (DistributeOctTree on the device; in the single-frame call the 7x7 blur tiles ride in
 * its launch), CCM_K_BLUR = orb_blur_frames_kernel of the grouped batch path and orb_blur_kernel of the host-octree path, CCM_K_BRIEF = orientation + steered descriptors (one kernel; CCM_K_ORIENT is unused), CCM_K_FAST_SCORE =
 * the score map of the test hook only. */
enum {
  CCM_K_HAMMING_DENSE = 0, CCM_K_HAMMING_CSR, CCM_K_PYR_RESIZE, CCM_K_FAST_SCORE, CCM_K_FAST_NMS,
  CCM_K_ORIENT, CCM_K_BLUR, CCM_K_BRIEF, CCM_K_BA_LINEARIZE, CCM_K_BA_CAM, CCM_K_BA_DINV,
  CCM_K_BA_SCHUR_DIAG, CCM_K_BA_SCHUR_OFF, CCM_K_BA_PCG_SPMV, CCM_K_BA_PCG_UPDATE,
  CCM_K_BA_BACKSUB, CCM_K_BA_UPDATE, CCM_K_BA_CHI2, CCM_K_POSEOPT, CCM_K_SIM3OPT, CCM_K_BA_PCG_PERSIST,
  CCM_K_BA_COARSE /* coarse operator + dense inverse of the two-level preconditioner */, CCM_K_BA_REDUCE /* trial scalars */,
  CCM_K_BA_ALLREDUCE /* the collectives of a sharded handle (RCCL all-reduce of [S | b_schur], of the trial scalars, of lambda_0's max): queue wait + wire time on the stream */, CCM_K_COUNT
};
int ccm_prof_enable(ccm_ctx* ctx, int kernel_class /* -1: all, -2: none */);
int ccm_prof_reset(ccm_ctx* ctx);
int ccm_prof_read(ccm_ctx* ctx, int kernel_class, int64_t* launches, double* total_ms);

/* ---- 256-bit Hamming ------------------------------------------------------------------
 * Replaces ORBmatcher::DescriptorDistance (cslam/src/ORBmatcher.cpp:1653-1669) and the
 * best / second-best scans inside the Search* methods (ORBmatcher.cpp:102-134, 220-245,
 * 1408-1433 ...).  Descriptors are rows of 32 bytes (cv::Mat N x 32 CV_8U, Frame.h:138).
 * Tie rule everywhere: strict '<' in candidate order, i.e. the FIRST minimum wins
 * (ORBmatcher.cpp:121,129).                                                              */

/* dense brute force: for every query row the best and second-best target over ALL T rows,
 * scanned in ascending target index.  best_idx = -1 / dists = 256 when T == 0.           */
int ccm_hamming_dense_best2(ccm_ctx* ctx, const uint8_t* q, int Q, const uint8_t* t, int T,
                            int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
int ccm_hamming_dense_best2_dev(ccm_ctx* ctx, const uint8_t* d_q, int Q, const uint8_t* d_t, int T,
                                int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist);

/* windowed / bucketed search (reference semantics): query i is compared with the ordered
 * candidate list cand_idx[cand_off[i] .. cand_off[i+1]) (the order GetFeaturesInArea
 * produced, Frame.cpp:228-250).  cand_dist receives one distance per candidate slot — the
 * host-side ordered resolution pass (claimed-feature skipping, ORBmatcher.cpp:113-115)
 * consumes it.  best2 outputs are computed ignoring claims and may be NULL.             */
int ccm_hamming_csr(ccm_ctx* ctx, const uint8_t* q, int Q, const uint8_t* t, int T,
                    const int32_t* cand_off, const int32_t* cand_idx,
                    uint16_t* cand_dist,
                    int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
int ccm_hamming_csr_dev(ccm_ctx* ctx, const uint8_t* d_q, int Q, const uint8_t* d_t, int T,
                        const int32_t* d_cand_off, const int32_t* d_cand_idx, int64_t n_cand,
                        uint16_t* d_cand_dist,
                        int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist);

/* S windowed searches in ONE launch and one read-back (round 5) — the per-keyframe fan-out of LocalMapping: up to 20 SearchForTriangulation calls
 * (cslam/src/Mapping.cpp:335) and as many Fuse calls (:503, :528) per new keyframe, each against ANOTHER keyframe's descriptors.  Search s owns the query
 * rows q_off[s] .. q_off[s+1] of q and the target rows t_off[s] .. t_off[s+1] of t (q_off[0] = t_off[0] = 0); cand_off / cand_idx / cand_dist run over ALL
 * queries back to back, and the candidate indices of a query are LOCAL to its search's target set.  Outputs as ccm_hamming_csr (best_idx local as well).
 * The _dev form takes, instead of the offsets, q_tbase[q] = first target row of the set query q searches in (nullable: one shared set). */
int ccm_hamming_csr_multi(ccm_ctx* ctx, int S, const uint8_t* q, const int32_t* q_off /* S+1 */, const uint8_t* t, const int32_t* t_off /* S+1 */,
                          const int32_t* cand_off, const int32_t* cand_idx, uint16_t* cand_dist,
                          int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
int ccm_hamming_csr_multi_dev(ccm_ctx* ctx, const uint8_t* d_q, int Q, const uint8_t* d_t, const int32_t* d_q_tbase,
                              const int32_t* d_cand_off, const int32_t* d_cand_idx, int64_t n_cand,
                              uint16_t* d_cand_dist, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist);

/* MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994), batched over P map points:
 * point p owns the descriptor rows off[p] .. off[p+1] (one per non-bad observing keyframe, in observation-map order);
 * best_local_idx[p] = index (within its own list) of the descriptor with the least median Hamming distance to the
 * others — median = element (int)(0.5*(N-1)) of the sorted row including the zero self distance, first minimum wins;
 * -1 for an empty list.  At most 256 observations per point.                                                        */
int ccm_distinctive_descriptors(ccm_ctx* ctx, const uint8_t* desc, const int32_t* off, int P, int32_t* best_local_idx);

/* DBoW2 vocabulary transform: TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
 * (cslam/thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1260) for a batch of descriptors.  The tree is passed flat:
 * node 0 is the root, children of node i are child_id[child_off[i] .. child_off[i+1]) in the vocabulary's child order
 * (a leaf has none), node_desc is n_nodes x 32 bytes, word_id / weight are per node (meaningful on leaves), L = depth.
 * Outputs per feature: word id, its weight (idf), and the node at level L - levelsup (0 when that level is <= 0).
 * BowVector accumulation / L1 normalisation and the FeatureVector map are host work on these arrays
 * (ccm_slam_amd/host: cslam::ORBVocabulary::transform; TemplatedVocabulary.h:1127-1190, BowVector.cpp:34-84); ccm_kfstore_ingest
 * below builds both vectors on the device for the keyframes of a message.                                                        */
typedef struct ccm_vocab ccm_vocab;
int  ccm_vocab_create(ccm_ctx* ctx, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc,
                      const int32_t* word_id, const double* weight, ccm_vocab** out);
void ccm_vocab_destroy(ccm_vocab* v);
int  ccm_bow_transform(ccm_vocab* v, const uint8_t* desc, int N, int levelsup, int32_t* word_out, double* weight_out, int32_t* node_out);

/* ---- ORB extraction -------------------------------------------------------------------
 * Replaces ORBextractor::ORBextractor / operator() (cslam/src/ORBextractor.cpp:579-639,
 * 1216-1278).  ccm_keypoint == cv::KeyPoint without class_id.                            */
typedef struct { float x, y, size, angle, response; int32_t octave; } ccm_keypoint;
typedef struct ccm_orb ccm_orb;

int  ccm_orb_create(ccm_ctx* ctx, int nfeatures, float scale_factor, int nlevels,
                    int ini_th_fast, int min_th_fast, ccm_orb** out);
void ccm_orb_destroy(ccm_orb* orb);
/* accessor mirrors of ORBextractor::GetScaleFactors() etc. (ORBextractor.h:114-136): fills
 * up to nlevels floats; which: 0 scale, 1 inv scale, 2 sigma2, 3 inv sigma2.             */
int  ccm_orb_get_table(const ccm_orb* orb, int which, float* out, int cap);
int  ccm_orb_features_per_level(const ccm_orb* orb, int32_t* out, int cap);
/* one frame, host buffers in and out.  kps/desc capacity (cap rows) should be >= ccm_orb_max_keypoints().
 * pyramid_out (nullable): nlevels caller buffers receiving the un-bordered level images
 * (mvImagePyramid, ORBextractor.h:138), each at least level_w*level_h bytes, row stride = level_w. */
int  ccm_orb_extract(ccm_orb* orb, const uint8_t* img, int w, int h, int stride,
                     ccm_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                     uint8_t* const* pyramid_out);
int  ccm_orb_level_size(const ccm_orb* orb, int w, int h, int level, int* lw, int* lh);
/* upper bound of keypoints one frame can return: nfeatures + 67 per level.  DistributeOctTree stops at >= N nodes per level and may overshoot by up to 3
 * (ORBextractor.cpp:837,898), but its FIRST pass splits every root before any count is checked (:759-843): a level returns up to 4 nIni nodes whatever N is
 * (7 features on a 752 x 480 frame: 64 keypoints); nIni = round(W / H) <= 16 is assumed, wider levels are truncated at this capacity.
 * A pyramid level smaller than one 30-px cell contributes no keypoint (its image is still produced); an image whose level is more than twice as high as wide,
 * or empty, is rejected with CCM_E_ARG (the reference divides by zero / throws there). */
int  ccm_orb_max_keypoints(const ccm_orb* orb);
/* host-only (no GPU): DistributeOctTree (ORBextractor.cpp:707-931) on candidates given relative to
 * (minX,minY); sel_out receives the indices of the kept candidates in the reference's output order. */
int  ccm_orb_distribute_octree(const float* x, const float* y, const float* response, int n, int minX, int maxX,
                               int minY, int maxY, int N, int32_t* sel_out, int cap, int* n_out);
/* batch of frames already resident in HBM (d_imgs: n_frames images, tightly packed w*h each);
 * outputs stay on the device: d_kps [n_frames][cap], d_desc [n_frames][cap][32],
 * d_counts [n_frames].  Every stage runs on the device (DistributeOctTree included, as in
 * ccm_orb_extract); frames go out in groups of four per launch, two groups in flight; only a frame
 * whose candidates overflow the octree kernel's LDS plan is redone through the host octree.  */
int  ccm_orb_extract_batch_dev(ccm_orb* orb, const uint8_t* d_imgs, int n_frames, int w, int h,
                               ccm_keypoint* d_kps, uint8_t* d_desc, int cap, int32_t* d_counts);

/* Per-frame glue between extraction and matching.  A ccm_frame holds, on the device, what the
 * window searches read from a Frame / KeyFrame: undistorted keypoints (Frame::UndistortKeyPoints, Frame.cpp:284-312 —
 * cv::undistortPoints with P = K, five fixed-point iterations), the image bounds (ComputeImageBounds, :314-347), the
 * 75x48 grid (AssignFeaturesToGrid / PosInGrid, :103-118, :254-265) and the descriptors.
 * K = fx fy cx cy (mK, f32); dist = mDistCoef k1 k2 p1 p2 [k3] (n_dist 0, 4 or 5; dist[0] == 0 means "no distortion",
 * :286).  ccm_frame_window_search evaluates a batch of Frame::GetFeaturesInArea(u, v, r, minLevel, maxLevel) calls
 * (:200-253; pass -1, -1 for KeyFrame::GetFeaturesInArea, KeyFrame.cpp:1162-1201) and the Hamming distance of every
 * candidate to the query's descriptor: cand_off[Q+1], cand_idx / cand_dist in the reference's enumeration order
 * (ix-major, iy, insertion order), ready for the host's ordered resolution pass.  Call it with cap = 0 to size.
 * u, v and r are not validated on the host; the window rule is total instead (csrc/frame_math.h frame_cell_range, the
 * same lines on host and device): a query whose r is NaN or negative, whose u or v is NaN, or whose window edge is
 * inf - inf has an empty list; otherwise the four cell products are clamped to [-1, 76] before the conversion to int,
 * so a window beyond the grid (an infinite u, v or r included) ends at the grid's rim and every window an int holds is
 * the reference's.  min_level > max_level >= 0 is an empty list by the reference's own level rule. */
typedef struct ccm_frame ccm_frame;
int  ccm_frame_create(ccm_ctx* ctx, const float K[4], const float* dist, int n_dist, int img_w, int img_h, ccm_frame** out);
void ccm_frame_destroy(ccm_frame* f);
int  ccm_frame_bounds(const ccm_frame* f, float bounds[4] /* mnMinX mnMinY mnMaxX mnMaxY */);
int  ccm_frame_set_keypoints(ccm_frame* f, const ccm_keypoint* kps /* mvKeys */, const uint8_t* desc /* n x 32 */, int n);
int  ccm_frame_get(ccm_frame* f, float* xy_un /* n x 2, nullable */, int32_t* cell_off /* 75*48+1, nullable */,
                   int32_t* cell_idx /* <= n, nullable */);
int  ccm_frame_window_search(ccm_frame* f, int Q, const float* u, const float* v, const float* r,
                             const int32_t* min_level, const int32_t* max_level, const uint8_t* qdesc /* Q x 32 */,
                             int32_t* cand_off /* Q+1 */, int32_t* cand_idx, uint16_t* cand_dist, int64_t cap,
                             int64_t* n_cand);

/* ORBmatcher::SearchByProjection(Frame&, kfptr, const set<mpptr>&, th, ORBdist) (ORBmatcher.cpp:1478-1604), the guided search of
 * relocalisation, up to its sequential pass: for all P map points of the keyframe at once the projection with the frame's pose and
 * its gates (:1482-1532, csrc/guided_search_math.h), the window of Frame::GetFeaturesInArea(u, v, th * mvScaleFactors[level],
 * level - 1, level + 1) on the resident grid, and the Hamming distance of every candidate.  The intrinsics and the image bounds are
 * the ccm_frame's own.  Tcw = rows 0..2 of mTcw, row-major; the camera centre is derived from it.  skip[i] != 0 (no live map point
 * in the slot, or the point is in sAlreadyFound; nullable: none) and every point a gate rejects have an empty list.
 * status: 0 skipped, 1 outside the image, 2 outside the distance range, 3 searched; u, v are written from status 1 on, level for 3.
 * cand_off / cand_idx / cand_dist, cap, n_cand and the sizing call (cap = 0) are ccm_frame_window_search's.
 * CCM_E_ARG: a null argument with P > 0, P < 0, nScaleLevels outside 1..16, th negative or not finite, cap too small (n_cand is set). */
typedef struct {
  float Tcw[12];
  float logScaleFactor;
  int32_t nScaleLevels;
  float scaleFactors[16];
} ccm_guided_pose;
int  ccm_frame_guided_search(ccm_frame* f, const ccm_guided_pose* pose, int P, const float* pos /* P x 3 */, const float* min_dist,
                             const float* max_dist, const uint8_t* desc /* P x 32 */, const uint8_t* skip /* P, nullable */, float th,
                             uint8_t* status, float* u, float* v, int32_t* level, int32_t* cand_off /* P+1 */, int32_t* cand_idx,
                             uint16_t* cand_dist, int64_t cap, int64_t* n_cand);

/* Frame::isInFrustum (Frame.cpp:139-198) for a batch of map points — Tracking::SearchLocalPoints' visibility loop.
 * The struct carries what the frame contributes (mRcw row-major, mtcw, mOw, intrinsics, image bounds, mfLogScaleFactor,
 * mnScaleLevels); per point: world position, mean viewing direction (GetNormal), mfMinDistance / mfMaxDistance.
 * Outputs = mbTrackInView, mTrackProjX/Y, mnTrackScaleLevel (PredictScale, MapPoint.cpp:854-869), mTrackViewCos. */
typedef struct {
  float Rcw[9], tcw[3], Ow[3];
  float fx, fy, cx, cy;
  float minX, maxX, minY, maxY;
  float logScaleFactor;
  int32_t nScaleLevels;
} ccm_frustum_frame;
int  ccm_frame_frustum(ccm_ctx* ctx, const ccm_frustum_frame* fr, int n, const float* P /* n x 3 */,
                       const float* normal /* n x 3 */, const float* min_dist, const float* max_dist,
                       float viewing_cos_limit, uint8_t* in_view, float* proj_x, float* proj_y, int32_t* level,
                       float* view_cos);

/* MapPoint::UpdateNormalAndDepth (MapPoint.cpp:779-823) for a batch of map points — called after every BA write-back
 * (Optimizer.cpp:636, 845) and for every new / fused point.  Per point i: world position pos[i] (mWorldPos), the list
 * obs_kf[obs_off[i] .. obs_off[i+1]) of its NON-BAD observing keyframes in the order the shim iterates mObservations (the
 * reference's std::map<kfptr, size_t> is ordered by heap address, so any order is a valid reference order; the f32 sum follows the
 * list), the reference keyframe ref_kf[i] (mpRefKF) and the octave ref_level[i] of its keypoint there; kf_center = GetCameraCenter()
 * of every keyframe, scale_factors = mvScaleFactors (shared by all keyframes of a map).  Outputs mNormalVector, mfMinDistance,
 * mfMaxDistance; a point whose list is empty keeps the values passed in (the reference returns early, :796-797). */
int  ccm_update_normal_and_depth(ccm_ctx* ctx, int n_pt, const float* pos /* n_pt x 3 */, const int32_t* obs_off /* n_pt+1 */,
                                 const int32_t* obs_kf, int n_kf, const float* kf_center /* n_kf x 3 */, const int32_t* ref_kf,
                                 const int32_t* ref_level, const float* scale_factors, int n_levels,
                                 float* normal /* n_pt x 3, in/out */, float* min_dist /* in/out */, float* max_dist /* in/out */);

/* ---- bundle adjustment ----------------------------------------------------------------
 * Replaces the g2o machinery driven by Optimizer::BundleAdjustmentClient /
 * LocalBundleAdjustmentClient / MapFusionGBA (cslam/src/Optimizer.cpp:40-212, 349-644,
 * 646-859): BlockSolver_6_3 + OptimizationAlgorithmLevenberg + EdgeSE3ProjectXYZ + Huber
 * (thirdparty/g2o/g2o/core/block_solver.hpp, optimization_algorithm_levenberg.cpp,
 * types/types_six_dof_expmap.{h,cpp}, core/robust_kernel_impl.cpp).
 * All state is f64.  cam_qt rows: qx qy qz qw tx ty tz (world -> camera, as g2o::SE3Quat).
 * ccm_ba_create / ccm_ba_reset_state only COPY these arrays to their device-side staging buffers (the structure is built on the device), so every
 * pointer may address host memory (pageable or pinned) or memory of the context's device; the one-shot ccm_ba_optimize, ccm_ba_download and
 * ccm_ba_depth_positive write / read host memory. */
typedef struct {
  int32_t n_cam, n_pt, n_edge;
  double*        cam_qt;     /* [n_cam*7]  in/out                                        */
  const uint8_t* cam_fixed;  /* [n_cam]    1 = vertex->setFixed(true)                    */
  const double*  cam_K;      /* [n_cam*4]  fx fy cx cy (e->fx.. come from the KF)        */
  double*        pt_xyz;     /* [n_pt*3]   in/out                                        */
  const int32_t* e_cam;      /* [n_edge]                                                 */
  const int32_t* e_pt;       /* [n_edge]                                                 */
  const double*  e_obs;      /* [n_edge*2] keypoint (undistorted) pixel                  */
  const double*  e_info;     /* [n_edge]   invSigma2 (information = I2 * invSigma2)      */
  const uint8_t* e_level;    /* [n_edge]   nullable; g2o edge level, only level 0 is optimised */
  double         huber_delta;/* <= 0: no robust kernel                                   */
} ccm_ba_problem;

typedef struct {
  int32_t max_iters;         /* optimizer.optimize(n)                                    */
  int32_t pcg_max_iters;     /* <=0: default 1000                                        */
  double  pcg_rel_tol;       /* <=0: default 1e-8 on sqrt(r.z / r0.z0); see DESIGN.md 4.1  */
  double  lambda_init;       /* <=0: tau * max diag(H), tau = 1e-5 (levenberg.cpp:166-180) */
  int32_t verbose;
} ccm_ba_options;

typedef struct {
  int32_t iters_done;        /* value optimize() would return                            */
  int32_t lm_trials;         /* total inner trials                                       */
  int32_t pcg_iters;         /* total PCG iterations                                     */
  int32_t stop_reason;       /* 0 iters exhausted, 1 stop flag, 2 trials exhausted/rho==0, 3 chi2 stagnation, 4 solver failure */
  double  chi2_initial, chi2_final, lambda_final;
  double  ms_setup, ms_total, ms_iters;   /* host wall clock */
  int32_t n_schur_blocks;    /* upper-triangular blocks incl. diagonal                   */
  int64_t n_pair_instances;
} ccm_ba_stats;

typedef struct ccm_ba ccm_ba;
typedef void (*ccm_ba_trial_cb)(void* user, int iteration, int trial_in_iteration, double chi2_trial, int accepted);

/* one-shot: build structure, upload, optimise, write cam_qt/pt_xyz back.  Always a single-rank solve, also on a context
 * that carries a multi-rank communicator (sharding is opt-in through the staged API below, called by all ranks).
 * stop_flag (nullable) is the reference's bool* pbStopFlag, polled between LM trials.
 * chi2_per_edge (nullable, in/out [n_edge]) = e->chi2() as the caller of optimize() sees it: for
 * active (level-0) edges the value of the last evaluated LM trial, inactive edges are left
 * untouched; depth_pos (nullable, [n_edge]) = e->isDepthPositive() at the final estimate.    */
int ccm_ba_optimize(ccm_ctx* ctx, ccm_ba_problem* prob, const ccm_ba_options* opt,
                    const volatile unsigned char* stop_flag,
                    double* chi2_per_edge, uint8_t* depth_pos, ccm_ba_stats* stats);

/* staged API (bench / multi-GPU): create uploads the problem and builds the Schur structure;
 * rank/nranks shard the landmarks (each rank owns a contiguous landmark range balanced by
 * pair count; camera state is replicated).  With nranks > 1 a communicator must be attached
 * before ccm_ba_run, and ccm_ba_run / ccm_ba_download are COLLECTIVE calls: every rank makes them with
 * the same options, and either every rank passes a stop flag or none does (the flag is reduced over
 * the ranks with each trial's scalars, so a flag raised on one rank stops all of them at the same trial). */
int  ccm_ba_create(ccm_ctx* ctx, const ccm_ba_problem* prob, int rank, int nranks, ccm_ba** out);
void ccm_ba_destroy(ccm_ba* ba);
int  ccm_ba_reset_state(ccm_ba* ba, const double* cam_qt, const double* pt_xyz); /* re-upload initial state */
/* SparseOptimizer::push() / pop() for all vertices (sparse_optimizer.cpp:600-613): save the current estimate on the device /
 * make the saved estimate current again (stream-ordered device copies; one level, a second push overwrites the first) */
int  ccm_ba_push_state(ccm_ba* ba);
int  ccm_ba_pop_state(ccm_ba* ba);
int  ccm_ba_run(ccm_ba* ba, const ccm_ba_options* opt, const volatile unsigned char* stop_flag,
                ccm_ba_stats* stats);
int  ccm_ba_download(ccm_ba* ba, double* cam_qt, double* pt_xyz, double* chi2_per_edge);
/* Second stage of Optimizer::LocalBundleAdjustmentClient on the SAME handle (Optimizer.cpp:545-566: outlier edges -> setLevel(1), robust kernel off,
 * optimize(10)): edges with e_level[e] != 0 ([n_edge], the caller's numbering) leave the optimisation, the Huber delta is replaced (<= 0: none), the
 * estimate stays; the next ccm_ba_run is the reference's initializeOptimization(0) + optimize(n) on the reduced edge set.  The call is a pure function of
 * (e_level, huber_delta) and of the informations given to ccm_ba_create: an edge whose level goes back to 0 takes part again with its original information
 * (a handle re-run after ccm_ba_pop_state passes its first-stage levels and delta again).  Only edges inactive at ccm_ba_create are not part of the handle
 * and cannot come back.  A deactivated edge contributes exact zeros whatever its residual is and keeps reporting the chi2 of the last pass it took part in. */
int  ccm_ba_set_edge_levels(ccm_ba* ba, const uint8_t* e_level, double huber_delta);
/* per-iteration record of the last ccm_ba_run: robust chi2 after the iteration, lambda after it, LM trials it took
 * (what g2o prints with setVerbose(true), sparse_optimizer.cpp:400-410); fills min(*n_iters, cap) entries */
int  ccm_ba_history(const ccm_ba* ba, int cap, double* chi2_per_iter, double* lambda_per_iter, int32_t* trials_per_iter,
                    int* n_iters);
/* called on the optimising thread after every LM trial, before the stop flag is polled (the place where
 * OptimizationAlgorithmLevenberg::solve tests terminate(), optimization_algorithm_levenberg.cpp:150); a caller can use it
 * to watch progress or to decide when to raise its stop flag.  cb == NULL removes it. */
int  ccm_ba_set_trial_callback(ccm_ba* ba, ccm_ba_trial_cb cb, void* user);
/* e->isDepthPositive() for every edge of the problem at the given state (host arithmetic, O(n_edge)) */
int  ccm_ba_depth_positive(const ccm_ba_problem* prob, const double* cam_qt, const double* pt_xyz, uint8_t* depth_pos);
/* host-only: split n landmark weights into nranks contiguous ranges (begin_out has nranks+1 entries) */
int  ccm_ba_partition(const int64_t* weight, int n, int nranks, int32_t* begin_out);
/* algorithmic byte count of one LM trial for the roofline */
int  ccm_ba_counts(const ccm_ba* ba, int64_t* n_active_edges, int64_t* n_active_pts,
                   int64_t* n_free_cams, int64_t* n_blocks, int64_t* n_pairs);


/* RCCL communicator for the sharded GBA.  id_bytes is an ncclUniqueId (128 bytes) produced by
 * ccm_comm_unique_id on rank 0 and broadcast by the launcher (bench.py uses torch.distributed). */
int ccm_comm_unique_id(uint8_t id_bytes[128]);
int ccm_comm_init(ccm_ctx* ctx, int nranks, int rank, const uint8_t id_bytes[128]);
int ccm_comm_destroy(ccm_ctx* ctx);

/* motion-only pose optimisation: Optimizer::PoseOptimizationClient (Optimizer.cpp:215-347):
 * 4 rounds x 10 LM iterations on one SE3 vertex with unary EdgeSE3ProjectXYZOnlyPose edges,
 * Huber sqrt(5.991) (dropped for the last round), chi2 threshold 5.991, dense 6x6 solve.
 * cam_qt in: Frame.mTcw as SE3Quat, out: optimised pose.  outlier[n] = Frame.mvbOutlier.
 * Returns via n_inlier the reference's return value (nInitialCorrespondences - nBad).     */
int ccm_pose_optimize(ccm_ctx* ctx, double cam_qt[7], int n, const double* Xw /*n*3*/,
                      const double* obs /*n*2*/, const double* info /*n*/, const double K[4],
                      uint8_t* outlier, int* n_inlier);

/* Sim3 between two keyframes from matched map points: Optimizer::OptimizeSim3 (Optimizer.cpp:861-1056).
 * sim3 = g2oS12 as [qx qy qz qw tx ty tz s] (in: Sim3Solver estimate, out: optimised; untouched when the call
 * returns *n_inlier = 0 because fewer than 10 pairs survive the first pass, :1015-1016).  Per valid pair i
 * (the shim filters null / bad map points and i2 < 0, :911-947): P1c = R1w*X1+t1w and P2c = R2w*X2+t2w (the fixed
 * VertexSBAPointXYZ estimates), obs1/obs2 = undistorted keypoints in KF1/KF2, info = mvInvLevelSigma2[octave].
 * Edges EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (types_seven_dof_expmap.h:133-172) with g2o's numeric
 * Jacobians (base_binary_edge.hpp:129-196), Huber (float)sqrt(th2), optimize(5) + optimize(10|5).
 * inlier[i] = 0 where the reference nulls vpMatches1[idx]. */
int  ccm_sim3_optimize(ccm_ctx* ctx, double sim3[8], int n, const double* P1c, const double* P2c,
                       const double* obs1, const double* obs2, const double* info1, const double* info2,
                       const double K1[4], const double K2[4], double th2, int fix_scale,
                       uint8_t* inlier, int* n_inlier);

/* Pose-graph numerics of Optimizer::OptimizeEssentialGraphLoopClosure / MapFusion (Optimizer.cpp:1058-1331, 1333-1566):
 * vertices = keyframes with estimate Siw as [qx qy qz qw tx ty tz s] (fixed[v] = the loop keyframe, fix_scale =
 * bFixScale), edges = EdgeSim3 with vertex(0) = e_i, vertex(1) = e_j, measurement Sji (same 8-double layout) and
 * information I7 (types_seven_dof_expmap.h:98-121); g2o's numeric Jacobians (base_binary_edge.hpp:129-196),
 * BlockSolver_7_3 + Levenberg with setUserLambdaInit(lambda_init = 1e-16 in the reference; <= 0 selects g2o's
 * tau * max-diagonal rule), optimize(max_iters = 20).  The caller keeps the graph walk that chooses the edges
 * (spanning tree, loop edges, covisibility >= minFeat, :1122-1260) and the SE3 / map-point write-back (:1268-1330).
 * The linear solve is a dense f64 Cholesky on the device (exact, like Eigen's sparse LDLT in the reference); the environment
 * variable CCM_PG_SOLVER=pcg selects a tree-preconditioned PCG instead (faster on large graphs, inexact-Newton path). */
typedef struct {
  int32_t iters_done, lm_trials, pcg_iters, reserved;
  double chi2_initial, chi2_final, lambda_final;
} ccm_pg_stats;
int  ccm_pose_graph_optimize(ccm_ctx* ctx, int n_vert, double* sim3 /* n_vert x 8, in/out */, const uint8_t* fixed,
                             int fix_scale, int n_edge, const int32_t* e_i, const int32_t* e_j,
                             const double* meas /* n_edge x 8 */, int max_iters, double lambda_init,
                             const volatile unsigned char* stop_flag /* nullable */, ccm_pg_stats* stats /* nullable */);

/* ---- keyframe database (place recognition) ---------------------------------------------
 * Replaces the inverted file of cslam::KeyFrameDatabase (cslam/src/Database.cpp:29-70) and phase 1 of DetectLoopCandidates /
 * DetectMapMatchCandidates / DetectRelocalizationCandidates (:74-146, :206-271, :331-385): which keyframes share words with the query,
 * how many, and the L1 score (thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-66, bit-identical in f64) of those with count > minCommonWords.
 * Phase 2 (covisibility accumulation, :148-201) is host work on the returned table: ccm_slam_amd/host/kfdb_resolve.h.
 * A keyframe is a key (the shim packs mId as id << 8 | client) with a client id `group` and its BowVector (word ids ascending, unique,
 * < n_words; at most 4096 words in a query).  Threading: one handle is shared by all threads, each call uses the caller's context and stream
 * (same device as the handle, else CCM_E_ARG); add / erase / clear are serialised and finished when they return, queries run concurrently
 * under a reader lock.  Contract: every query is computed on fresh state — equal to the reference when a keyframe is queried at most once per
 * query kind, which is how LoopFinder.cpp:142 and MapMatcher.cpp:150 call it (the reference's per-KeyFrame scratch fields mLoopQuery /
 * mnLoopWords / mLoopScore are not reproduced). */
typedef struct ccm_kfdb ccm_kfdb;
/* log_capacity: keyframes added after the last rebuild of the device inverted file that are scanned directly (0: 64) */
int  ccm_kfdb_create(ccm_ctx* ctx, int n_words, int log_capacity, ccm_kfdb** out);
void ccm_kfdb_destroy(ccm_kfdb* db);
/* KeyFrameDatabase::add (:37-43); a live key added twice: CCM_E_STATE (the reference never does it) */
int  ccm_kfdb_add(ccm_kfdb* db, ccm_ctx* ctx, int64_t key, int32_t group, int n, const int32_t* word, const double* value);
/* KeyFrameDatabase::erase (:45-64); an unknown key is a no-op, as there */
int  ccm_kfdb_erase(ccm_kfdb* db, ccm_ctx* ctx, int64_t key);
/* KeyFrameDatabase::clear (:66-70) */
int  ccm_kfdb_clear(ccm_kfdb* db, ccm_ctx* ctx);
/* Exclusions of phase 1.  DetectLoopCandidates: self_key = the query (pKFi->mId == pKF->mId), allow = GetMmpKeyFrames() of its map, exclude =
 * GetConnectedKeyFrames().  DetectMapMatchCandidates: exclude_groups = bit c set for every client id c in pMap->msuAssClients (ids >= 64 are
 * never excluded).  DetectRelocalizationCandidates: none (f = NULL). */
typedef struct {
  int64_t self_key;                          /* -1: none */
  const int64_t* allow; int n_allow;         /* NULL: every keyframe */
  const int64_t* exclude; int n_exclude;
  uint64_t exclude_groups;
} ccm_kfdb_filter;
/* Phase 1 of one query: the keyframes of lKFsSharingWords with count > minCommonWords, in that list's order, with their shared-word count and
 * score (f32 as the reference's `float si`, and the f64 it was rounded from).  Writes min(*n_out, cap) rows; *n_out = rows of the full table
 * (call again with cap >= *n_out if it was larger); n_sharing = size of lKFsSharingWords, max_common = maxCommonWords, generation = number of
 * mutations the query saw.  Empty database or no shared word: *n_out = 0.  Output pointers after n_out are nullable. */
int  ccm_kfdb_query(ccm_kfdb* db, ccm_ctx* ctx, int n, const int32_t* word, const double* value, const ccm_kfdb_filter* f,
                    int cap, int64_t* key_out, int32_t* count_out, float* score_out, double* score64_out,
                    int* n_out, int* n_sharing_out, int* max_common_out, uint64_t* generation_out);
/* mpVoc->score(q, kf) in f64 for m listed keys (LoopFinder.cpp:124-137); a key that is not in the database: CCM_E_ARG */
int  ccm_kfdb_score(ccm_kfdb* db, ccm_ctx* ctx, int n, const int32_t* word, const double* value,
                    const int64_t* keys, int m, double* out);

/* ---- Sim3 RANSAC (loop / map-match verification) ------------------------------------------
 * The hypotheses of cslam::Sim3Solver::iterate (cslam/src/Sim3Solver.cpp:120-197): per hypothesis ComputeSim3 on three correspondences
 * (:199-321) and CheckInliers (:324-348) over all of its candidate's points, bit-identical to the reference's f32 / f64 arithmetic under
 * OpenCV 4.2 baseline-build semantics.  Stateless: the RANSAC state, the round-robin of LoopFinder / MapMatcher::ComputeSim3
 * and the random draws stay on the host (ccm_slam_amd/host/sim3_schedule.h).
 * K candidates in CSR over pt_off[K + 1] (pt_off[0] = 0, every candidate >= 3 points): X3Dc1 / X3Dc2 = mvX3Dc1 / mvX3Dc2 (f32 x 3 per point),
 * K1 / K2 = fx fy cx cy per candidate, max_err1 / max_err2 = mvnMaxError1 / mvnMaxError2 (the reference's size_t thresholds).
 * H hypotheses: hyp_cand[h] and three distinct candidate-local point indices hyp_idx[3h .. 3h+2] (the sample order of the reference).
 * fix_scale = mbFixScale.  Out: n_inl[h] = mnInliersi, rts[13h ..] = mR12i (9, row-major), mt12i (3), ms12i; mask_off[H + 1] (written by the
 * call) = word offsets of the inlier masks, mask[mask_off[h] ..] = mvbInliersi, one bit per point (bit i % 32 of word i / 32), mask must hold
 * sum over h of ceil(N / 32) words.  CCM_E_ARG: null pointers, K < 1, H < 0, a candidate with N < 3, an index outside [0, N) or repeated in a
 * hypothesis.  One H2D copy, one launch and one D2H copy on the context's stream, scratch of the context; threads calling with their own
 * contexts run concurrently.
 * Contract of the host schedule built on it (cslam::Sim3RansacBatch): its events equal those of the sequential reference on the same sequence
 * of rand() values; values drawn for hypotheses after an event are kept in a per-thread FIFO and used first by the next draw, so the equality
 * holds across calls — only WHEN glibc's global stream advances differs. */
int  ccm_sim3_ransac_eval(ccm_ctx* ctx, int K, const int32_t* pt_off, const float* X3Dc1, const float* X3Dc2, const float* K1, const float* K2,
                          const uint32_t* max_err1, const uint32_t* max_err2, int H, const int32_t* hyp_cand, const int32_t* hyp_idx,
                          int fix_scale, int32_t* n_inl, float* rts, int32_t* mask_off, uint32_t* mask);

/* ---- PnP RANSAC (relocalisation) ---------------------------------------------------------------
 * The hypotheses of cslam::PnPsolver::iterate (cslam/src/PnPSolver.cpp:155-249): per hypothesis EPnP's compute_pose on four correspondences
 * (:468-516) and CheckInliers (:299-330) over all of its candidate's points, in the reference's own f64 / f32 arithmetic with the legacy
 * OpenCV calls restated for f64 (the lines are ccm_slam_amd/csrc/pnp_math.h, which also compiles for the host).  Stateless.
 * K candidates in CSR over pt_off[K + 1] (pt_off[0] = 0, every candidate >= 4 points): P3Dw = mvP3Dw (f32 x 3 per point), P2D = mvP2D (f32 x 2),
 * max_err = mvMaxError (f32), cam = fu fv uc vc per candidate (f64, as the reference's members).
 * H hypotheses: hyp_cand[h] and four distinct candidate-local point indices hyp_idx[4h .. 4h+3] in sample order.
 * Out: n_inl[h] = mnInliersi, Rt[12h ..] = mRi (9, row-major), mti (3); mask_off[H + 1] (written by the call) = word offsets of the inlier
 * masks, mask[mask_off[h] ..] = mvbInliersi, one bit per point (bit i % 32 of word i / 32, tail bits zero), mask must hold the sum over h of
 * ceil(N / 32) words.  Non-finite values are not trapped: a NaN pose compares false against every threshold.  CCM_E_ARG: null pointers, K < 1, H < 0, a candidate with N < 4,
 * an index outside [0, N) or repeated in a hypothesis.  H = 0 succeeds and does nothing.  One H2D copy, one launch and one D2H copy on the
 * context's stream, scratch of the context. */
int  ccm_pnp_ransac_eval(ccm_ctx* ctx, int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* max_err, const double* cam,
                         int H, const int32_t* hyp_cand, const int32_t* hyp_idx, int32_t* n_inl, double* Rt, int32_t* mask_off, uint32_t* mask);

/* ---- triangulation of new map points ---------------------------------------------------------
 * The per-match arithmetic of LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:353-448) for every match of up to 20 neighbours in ONE
 * launch: ray-parallax gate, linear triangulation (cv::SVD::compute on a 4x4 f32 matrix), the two depth tests, the two chi2 reprojection gates
 * and the scale-consistency gate, bit-identical to the reference's f32 / f64 arithmetic under OpenCV 4.2 baseline-build semantics
 * (the lines are ccm_slam_amd/csrc/triangulate_math.h, which also compiles for the host).  Stateless.
 * A camera record is 21 floats: Rcw (9, row-major), tcw (3), Ow (3), fx fy cx cy invfx invfy.  cam1 = the new keyframe, cam2 = one record per
 * neighbour group.  S groups in CSR over pair_off[S + 1] (pair_off[0] = 0, groups may be empty), P = pair_off[S] matches: xy = x1 y1 x2 y2 of
 * mvKeysUn per match, oct = octave1 octave2 per match.  sigma2_* / sf_* = mvLevelSigma2 / mvScaleFactors of the new keyframe (1) and of the
 * neighbours (2), nlevels entries each.  ratioFactor = 1.5f * mfScaleFactor.
 * Out: status[P] = the first gate at which the reference's loop `continue`s — 0 accepted, 1 parallax, 2 x3D(3) == 0, 3 z1 <= 0, 4 z2 <= 0,
 * 5 / 6 reprojection in keyframe 1 / 2, 7 a zero distance, 8 scale ratio; x3d[3P] = the point reached so far (NaN for status 1);
 * n_accepted[S] = matches with status 0 per group.
 * CCM_E_ARG: null pointers, S < 1, a decreasing pair_off, an octave outside [0, nlevels).  P == 0 succeeds with no launch.  One H2D copy, one
 * launch and one D2H copy on the context's stream, scratch of the context; threads calling with their own contexts run concurrently. */
int  ccm_triangulate_pairs(ccm_ctx* ctx, const float* cam1 /* 21 */, int S, const float* cam2 /* 21 S */, const int32_t* pair_off /* S+1 */,
                           const float* xy /* 4 P */, const int32_t* oct /* 2 P */, int nlevels, const float* sigma2_1, const float* sf_1,
                           const float* sigma2_2, const float* sf_2, float ratioFactor, uint8_t* status, float* x3d, int32_t* n_accepted);

/* ---- Sim3 correction of a closed loop's or merged map's keyframes and points ---------------------
 * The arithmetic of the correction loops of LoopFinder::CorrectLoop (cslam/src/LoopFinder.cpp:543-613) and MapMerger::MergeMaps
 * (cslam/src/MapMerger.cpp:289-395), and of the tail of both essential-graph optimisers (cslam/src/Optimizer.cpp:1279-1330), in TWO launches:
 * per keyframe the two Sim3s, the new pose [R | t / s] and its camera centre (KeyFrame::SetPose), per map point
 * CorrectedSwi.map(Siw.map(P)) and MapPoint::UpdateNormalAndDepth on the new position, bit-identical to the reference's f32 / f64 arithmetic
 * under OpenCV 4.2 baseline-build semantics (the lines are ccm_slam_amd/csrc/sim3_correct_math.h, which also compiles for the
 * host).  Stateless; no graph is touched: SetWorldPos, the tags, SetPose and UpdateConnections stay the caller's.
 * Keyframes: the set of n_kf >= 1 corrected keyframes IN THE ORDER THE REFERENCE'S LOOP WALKS THEM, followed by the observers outside the set,
 * n_obs_kf >= n_kf in all.  kf_center[3 n_obs_kf] = GetCameraCenter() before the call, kf_rank[n_obs_kf] = position in the walk (INT32_MAX
 * outside the set).  A pose is 12 floats: rows 0..2 of the 4x4, row-major; a Sim3 is 8 doubles: qx qy qz qw tx ty tz s.
 *   loop / merge form (Tiw != NULL): Tiw[12 n_kf] = GetPose(), cur = index of the current keyframe in the set, Twc = its GetPoseInverse(),
 *     Scw = the accepted mg2oScw.  S_non / S_cor [8 n_kf] are OUTPUTS: NonCorrectedSim3 and CorrectedSim3 (keyframe cur takes Scw itself).
 *   epilogue form (Tiw == NULL): S_non / S_cor are INPUTS (vScw and the optimised CorrectedSiw per keyframe); cur, Twc and Scw are not read.
 * Points (n_pt >= 0; 0 corrects the keyframes only and the per-point pointers may be NULL): pos[3 n_pt] = GetWorldPos(); owner = index in the
 * set of the keyframe whose two Sim3s move the point (loop form: the FIRST keyframe of the walk that lists it; epilogue form: its reference
 * keyframe, or mCorrectedReference_LC); owner_rank = kf_rank[owner] in the loop form, INT32_MAX in the epilogue form; observers in CSR over
 * obs_off[n_pt + 1] (obs_off[0] = 0; the non-bad keyframes of mObservations, summed in list order), ref_kf / ref_level = the reference
 * keyframe and the octave of the point's feature in it; scale_factors[n_levels] = mvScaleFactors.
 * Rule for the centres: the reference updates a point's normal and depth immediately, inside the walk, so observer k (and the reference
 * keyframe) shows its NEW centre iff k < n_kf and kf_rank[k] < owner_rank, its old centre otherwise.
 * Out: pos_out[3 n_pt] (may be pos), normal[3 n_pt] / min_dist / max_dist (in / out: a point with an empty observation list keeps what was
 * passed in; the bounds are mfMinDistance / mfMaxDistance), Tiw_new[12 n_kf], center_new[3 n_kf], and the two Sim3 tables in the loop form.
 * CCM_E_ARG: null pointers, n_kf < 1, n_obs_kf < n_kf, a decreasing obs_off, an owner outside [0, n_kf), an observer or reference keyframe
 * outside [0, n_obs_kf), a level outside [0, n_levels), cur outside [0, n_kf) in the loop form.  NaN / Inf positions propagate.  One H2D copy,
 * two launches and one D2H copy on the context's stream, scratch of the context; threads calling with their own contexts run concurrently. */
int  ccm_sim3_correct_map(ccm_ctx* ctx, int n_kf, const float* Tiw /* 12 n_kf or NULL */, int cur, const float* Twc /* 12 */, const double* Scw /* 8 */,
                          double* S_non /* 8 n_kf */, double* S_cor /* 8 n_kf */, int n_obs_kf, const float* kf_center /* 3 n_obs_kf */,
                          const int32_t* kf_rank /* n_obs_kf */, int n_pt, const float* pos /* 3 n_pt */, const int32_t* owner, const int32_t* owner_rank,
                          const int32_t* obs_off /* n_pt + 1 */, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level,
                          const float* scale_factors, int n_levels, float* pos_out, float* normal, float* min_dist, float* max_dist,
                          float* Tiw_new /* 12 n_kf */, float* center_new /* 3 n_kf */);

/* ---- covisibility graph of a corrected map ------------------------------------------------------------
 * KeyFrame::UpdateConnections (cslam/src/KeyFrame.cpp:629-711) run over a set of keyframes in a given walk order, with the AddConnection /
 * UpdateBestCovisibles calls (:392-426) the set's keyframes make on each other: what LoopFinder.cpp:612 / :655, MapMerger.cpp:392 / :487 and
 * Map.cpp:614 leave in mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames and mvOrderedWeights, identical to the sequential walk (DESIGN.md
 * §14; the rules are ccm_slam_amd/csrc/covis_math.h, which also compiles for the host).  Integers only, stateless; the spanning tree (:713-833)
 * stays the caller's and reads the ordered list returned here.
 * Keyframes 0 .. n_kf - 1: the set IN WALK ORDER, n_kf .. n_all - 1: observers outside it.  order_key[n_all]: distinct values standing for the
 * pointer order of std::map<kfptr, ...> and of sort on pair<int, kfptr>.  Keyframe i lists list_pt[list_off[i] .. list_off[i + 1]) (< 0: a null
 * entry; an entry listed twice counts twice), list_skip[e] != 0: the point is bad.  Point p is observed by obs_kf[obs_off[p] .. obs_off[p + 1]).
 * th: the weight from which a connection is made (the reference's 15), >= 1.
 * Out, all CSR over the set: (row_off, col, count) = the own counts C_i by ascending keyframe index; (fw_off, fw_col, fw_w) = the final
 * mConnectedKeyFrameWeights by ascending keyframe index; (ord_off, ord_kf, ord_w) = mvpOrderedConnectedKeyFrames / mvOrderedWeights;
 * flags[n_kf]: 1 EMPTY (no counted observer: the keyframe's own step returns early, and its rows hold what the set's AddConnection calls
 * build on an EMPTY state — the state it had before stays with the caller), 2 FALLBACK (no count reached th: the one maximal neighbour),
 * 4 CHANGED (a later keyframe's AddConnection rebuilt the ordered list from the whole map).
 * cap = entries each of the six variable-size arrays can hold; needed[3] = entries of the count rows, the final rows and the ordered lists
 * (-1: not reached).  When a needed value exceeds cap the call returns CCM_OK with only `needed` defined: call again with a larger cap.
 * CCM_E_ARG: null pointers, n_kf < 1, n_all < n_kf, th < 1, cap < 0, offsets that do not start at 0 or decrease, a point index >= n_pt, an
 * observer outside [0, n_all), a repeated order_key; nothing is launched.  One H2D copy, seven launches and one D2H copy (sized by cap) on the
 * context's stream, scratch of the context; threads calling with their own contexts run concurrently. */
int  ccm_covis_update(ccm_ctx* ctx, int n_kf, int n_all, const int32_t* order_key /* n_all */, const int32_t* list_off /* n_kf + 1 */,
                      const int32_t* list_pt, const uint8_t* list_skip, int n_pt, const int32_t* obs_off /* n_pt + 1 */, const int32_t* obs_kf,
                      int th, int cap, int32_t* row_off /* n_kf + 1 */, int32_t* col, int32_t* count, int32_t* fw_off /* n_kf + 1 */,
                      int32_t* fw_col, int32_t* fw_w, int32_t* ord_off /* n_kf + 1 */, int32_t* ord_kf, int32_t* ord_w, int32_t* flags /* n_kf */,
                      int32_t* needed /* 3 */);

/* ---- the server's keyframe culling walk -----------------------------------------------------------------
 * LocalMapping::KeyFrameCullingV3 (cslam/src/Mapping.cpp:804-862) over the covisible keyframes of the picked keyframe in walk order, with what
 * culling one of them does to the points it sees (KeyFrame::SetBadFlag, KeyFrame.cpp:990-997; MapPoint::EraseObservation, MapPoint.cpp:442-509;
 * MapPoint::SetBadFlag, :545-558): later candidates see fewer points, fewer observers and smaller counts, and the verdicts equal the reference's
 * sequential walk (the rules are ccm_slam_amd/csrc/kfcull_math.h, which also compiles for the host).  Integers and one f64
 * comparison, stateless; the graph side of SetBadFlag (connections, spanning tree, map erase sets) stays the caller's.
 * Keyframes 0 .. n_cand - 1: the candidates IN WALK ORDER, n_cand .. n_all - 1: the other observers.  cand_flags[n_cand]: 1 SKIP (mId.first 0 or
 * 1, or in mlpRecentAddedKFs: not evaluated, stays a valid observer), 2 NOT_ERASE (mbNotErase: evaluated, a redundant verdict erases nothing).
 * Candidate k lists list_pt[list_off[k] .. list_off[k + 1]) (< 0: a null slot; a point listed twice counts twice and is erased once),
 * list_level[e] = mvKeysUn[slot].octave.  ONE record per distinct point p: pt_nobs[p] = Observations() (it may differ from the length of the
 * list), pt_bad[p] = isBad(), observers obs_kf[obs_off[p] .. obs_off[p + 1]) with obs_level = the octave of the point's feature in that keyframe
 * and obs_bad = that keyframe's isBad().  A live point needs a non-bad listed observer (its reference keyframe), and a candidate that can be
 * erased a slot for every point that lists it: kfcull_math.h says why.  th_obs: the reference's 3; thres: Mapping.RedThres; levels < n_levels.
 * Out: verdict[n_cand]: 0 kept, 1 culled, 2 skipped, 3 redundant but not erasable (the caller calls SetBadFlag for 1 and 3, in walk order);
 * n_mps / n_red[n_cand]: nMPs and nRedundantObservations as counted at the candidate's own turn (0 when skipped); pt_gone / pt_nobs_out[n_pt]:
 * isBad() and Observations() of every point after the walk; n_reeval[1]: candidates counted again because an earlier erasure could reach one
 * of their points.
 * CCM_E_ARG: null pointers, n_cand < 1, n_all < n_cand, th_obs < 1, thres NaN, offsets that do not start at 0 or decrease, a point index
 * >= n_pt, an observer outside [0, n_all), a keyframe twice in one point's observers, a level outside [0, n_levels), a negative pt_nobs;
 * nothing is launched.  One H2D copy, two launches (every slot on the initial state; one workgroup that takes the candidates in order) and one
 * D2H copy on the context's stream, scratch of the context; threads calling with their own contexts run concurrently. */
int  ccm_kfcull_walk(ccm_ctx* ctx, int n_cand, int n_all, const uint8_t* cand_flags /* n_cand */, const int32_t* list_off /* n_cand + 1 */,
                     const int32_t* list_pt, const uint8_t* list_level, int n_pt, const int32_t* pt_nobs /* n_pt */, const uint8_t* pt_bad /* n_pt */,
                     const int32_t* obs_off /* n_pt + 1 */, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad, int th_obs,
                     double thres, int n_levels, uint8_t* verdict /* n_cand */, int32_t* n_mps /* n_cand */, int32_t* n_red /* n_cand */,
                     uint8_t* pt_gone /* n_pt */, int32_t* pt_nobs_out /* n_pt */, int32_t* n_reeval /* 1 */);

/* ---- a finished global BA applied to the map ---------------------------------------------------------------
 * What follows optimize() in MapFusionGBA and RunGBA: the recovery of the f64 estimates into f32 (cslam/src/Optimizer.cpp:803-857, Converter.cc:52-74)
 * and the map walk the reference carries three times (Map.cpp:1441-1568, LoopFinder.cpp ~895-1010, MapMerger.cpp ~640-755), bit-identical to the
 * reference's f32 / f64 arithmetic under OpenCV 4.2 baseline-build semantics (the lines are ccm_slam_amd/csrc/gba_apply_math.h, which
 * also compiles for the host).  Stateless except for the optional handle; no graph is touched: SetPose, SetWorldPos, the tags and mbLoopCorrected
 * stay the caller's.  A pose is 12 floats: rows 0..2 of the 4x4, row-major.
 * Keyframes: n_kf >= 1 IN THE ORDER THE REFERENCE'S LIST WALK VISITS THEM (breadth first from mvpKeyFrameOrigins, each child behind its parent).
 * kf_parent[k] = index in that order of the keyframe from whose child set k was reached, -1 for an origin; kf_cam[k] = its camera in the BA problem,
 * -1 if it was no vertex (mBAGlobalForKF != nLoopKF); Tcw_old / Twc_old = GetPose() / GetPoseInverse() before the walk.  A vertex takes
 * toCvMat(estimate); any other keyframe takes (Tcw_old[k] * Twc_old[parent]) * T_new[parent], the two 4x4 f32 products in that order.  A vertex under
 * a parent that was none keeps its own estimate.  An origin that was no vertex has no mTcwGBA and is refused.
 * Points (n_pt >= 0 non-bad points; 0 is legal with the per-point pointers NULL): pos = GetWorldPos(); pt_vert = the BA landmark, or -1;
 * pt_ref = the reference keyframe's index in the walk, or -1 when there is none, it was never tagged, or the walk did not reach it.  A landmark is
 * cast; any other point with pt_ref >= 0 moves as Xc = Rcw_old X + tcw_old, X' = Rwc_new Xc + Ow_new (one gemm each); the others are copied.
 * The optimised state comes in ONE of two forms that give the same bits:
 *   host form: cam_qt[7 n_cam] (qx qy qz qw tx ty tz) and pt_xyz[3 n_lm] as ccm_ba_download returns them, ba = NULL;
 *   handle form: ba = a ccm_ba of THIS context with one rank, cam_qt = pt_xyz = NULL (n_cam / n_lm are the handle's; the arguments are not read).  The
 *     state is read where it lies on the device; the handle is left as ccm_ba_download leaves it.
 * Out: T_new[12 n_kf], Twc_new[12 n_kf] = rows 0..2 of [Rwc | Ow] as KeyFrame::SetPose leaves them, pos_out[3 n_pt] (may be pos), pt_status[n_pt]:
 * 0 untouched, 1 took the optimised value, 2 moved with its reference keyframe.
 * CCM_E_ARG, with nothing launched: null pointers, n_kf < 1, n_pt < 0, kf_parent[k] >= k or < -1, a camera, landmark or reference index out of range,
 * an origin that was no vertex, both or neither state form, a handle of another context or with nranks > 1.  NaN / Inf propagate.  One H2D copy, at most
 * three launches (the keyframes that were no vertices get ONE workgroup, not launched when there is none; the handle form adds the handle's own
 * landmark reorder, as its download does) and one D2H copy on the context's stream, scratch of the context; threads calling with their own contexts run concurrently. */
int  ccm_gba_apply_map(ccm_ctx* ctx, int n_kf, const int32_t* kf_parent /* n_kf */, const int32_t* kf_cam /* n_kf */, const float* Tcw_old /* 12 n_kf */,
                       const float* Twc_old /* 12 n_kf */, int n_pt, const float* pos /* 3 n_pt */, const int32_t* pt_vert /* n_pt */,
                       const int32_t* pt_ref /* n_pt */, int n_cam, const double* cam_qt /* 7 n_cam or NULL */, int n_lm,
                       const double* pt_xyz /* 3 n_lm or NULL */, ccm_ba* ba /* or NULL */, float* T_new /* 12 n_kf */, float* Twc_new /* 12 n_kf */,
                       float* pos_out /* 3 n_pt */, uint8_t* pt_status /* n_pt */);

/* ---- two-view initialisation: H / F RANSAC and CheckRT ------------------------------------------
 * The arithmetic of cslam::Initializer (cslam/src/Initializer.cpp) between the set drawing and ReconstructF / ReconstructH, bit-identical to the reference's
 * f32 / f64 arithmetic under OpenCV 4.2 baseline-build semantics (the lines are ccm_slam_amd/csrc/twoview_math.h, which also compiles for the
 * host).  Both calls are stateless: one H2D copy, the launches and one D2H copy on the context's stream, scratch of the context; threads calling with their own
 * contexts run concurrently.
 *
 * ccm_twoview_ransac_eval: FindHomography / FindFundamental (:120-219) for H hypotheses.  N >= 8 matches: xy1 / xy2 = mvKeysUn of both sides in match order
 * (x y pairs), pn1 / pn2 = the same points as Normalize (:745-791) gives them — Normalize runs over ALL keypoints of a frame, on the host (tv_normalize) —,
 * T1, T2inv = T2.inv(), T2t = T2.t() (9 floats each, row-major), sigma = mSigma, sets = mvSets: 8 distinct match indices per hypothesis, reference order.
 * Out: scoreH[H] / scoreF[H] = currentScore of every iteration, H21[9 H] / F21[9 H] = H21i / F21i, maskH / maskF = vbCurrentInliers, one bit per match
 * (bit i % 32 of word i / 32), ceil(N / 32) words per hypothesis.  The winner is the caller's: the first hypothesis, in order, whose score is strictly greater
 * than the best so far, starting from 0 (a NaN or zero score never wins).  CCM_E_ARG, with nothing launched: null pointers, N < 8, H < 1, an index outside
 * [0, N) or repeated within a set. */
int  ccm_twoview_ransac_eval(ccm_ctx* ctx, int N, const float* xy1 /* 2 N */, const float* xy2, const float* pn1, const float* pn2, const float* T1 /* 9 */,
                             const float* T2inv, const float* T2t, float sigma, int H, const int32_t* sets /* 8 H */, float* scoreH, float* scoreF,
                             float* H21, float* F21, uint32_t* maskH, uint32_t* maskF);
/* ccm_twoview_check_rt: the loop of CheckRT (:826-890) under 1 <= n_hyp <= 8 motion hypotheses at once.  rec = one record of 27 floats per hypothesis:
 * P2 = K * [R | t] (12, row-major), O2 = -R.t() * t (3), R (9), t (3), as tv_prepare_rt of twoview_math.h computes them on the host.  K = mK (9, row-major),
 * N >= 1 matches as above, inlier_mask = vbMatchesInliers in the mask layout above, th2 = 4.0 * mSigma2 as a float.
 * Out, per (hypothesis, match) at [hyp * N + match]: status = 0 not an inlier, 1 a non-finite point, 2 / 3 depth in camera 1 / 2, 4 / 5 reprojection in
 * image 1 / 2, 6 counted with low parallax (nGood++, vbGood stays false), 7 counted and good; x3d[3] = p3dC1 (NaN for status 0); cos_parallax (NaN for
 * status 0 and 1).  nGood, the sort of the counted cosines and acos(...) * 180 / CV_PI are the caller's (cslam::TwoViewInitializer::CheckRTBatch).
 * CCM_E_ARG: null pointers, n_hyp outside [1, 8], N < 1. */
int  ccm_twoview_check_rt(ccm_ctx* ctx, int n_hyp, const float* rec /* 27 n_hyp */, const float* K /* 9 */, int N, const float* xy1, const float* xy2,
                          const uint32_t* inlier_mask, float th2, uint8_t* status, float* x3d, float* cos_parallax);

/* ---- SearchAndFuse: every Fuse(pKF, Scw, vpLoopMapPoints, th, vpReplacePoints) of a loop closure or a map merge -------------------
 * LoopFinder::SearchAndFuse (cslam/src/LoopFinder.cpp:709-734) and MapMerger::SearchAndFuse (MapMerger.cpp:574-598) call ORBmatcher::Fuse (ORBmatcher.cpp:995-1122)
 * once per keyframe of CorrectedSim3 with the same points.  This call evaluates the loop body of every (keyframe, point) pair up to its decision, bit-identical to the
 * reference's f32 / f64 arithmetic under OpenCV 4.2 baseline-build semantics (the lines are ccm_slam_amd/csrc/fuse_math.h, which also compiles
 * for the host).  Stateless; the skips (isBad(), spAlreadyFound) and the map mutations stay the caller's (cslam::SearchAndFuseBatch replays them).
 * Per keyframe k < K: kf_rec = fx fy cx cy, mnMinX mnMinY mnMaxX mnMaxY (the keyframe's int-truncated bounds as floats), mfGridElementWidthInv, mfGridElementHeightInv;
 * its features feat_off[k] .. feat_off[k + 1] (at most 65 535): feat_xy = mvKeysUn[i].pt, feat_octave, feat_desc (32 bytes each); its mGrid as a CSR of 75 x 48 cells
 * in x-major order (cell ix * 48 + iy): cell_off + k * 3601 holds 3601 offsets from 0 to the feature count, cell_idx + feat_off[k] the keyframe's feature indices
 * (0-based in the keyframe) in the order the cells' vectors hold them; Scw + 12 k = rows 0 .. 2 of the cv::Mat passed to Fuse.
 * Per call: nlevels in 1 .. 16, scale_factors[nlevels] = mvScaleFactors, logScaleFactor = mfLogScaleFactor, th (finite, > 0).
 * Per point i < P: pos, normal, mfMinDistance, mfMaxDistance and the 32 descriptor bytes.
 * Out: table[k * P + i] = feature index (bits 0-15, 0xFFFF none) | bestDist << 16 (9 bits, 511 none) | nPredictedLevel << 25 (4 bits, from status 4 on) | status << 29:
 * 0 behind the camera, 1 outside the image, 2 distance range, 3 viewing angle, 4 window empty, 5 no candidate at the level, 6 bestDist > TH_LOW = 50 (index and distance
 * reported), 7 a hit.  n_valid[k] / n_hit[k]: pairs with status >= 4 / == 7.  uv (nullable, 2 K P): u, v of the pair (0 for status 0).
 * K == 0 or P == 0 is legal and launches nothing.  CCM_E_ARG, with nothing launched: null pointers, more than 65 535 features in a keyframe, K * P > INT32_MAX, offsets
 * that do not start at 0 or decrease, a cell_off that does not end at the keyframe's feature count, a cell_idx outside the keyframe, nlevels outside 1 .. 16, th not
 * finite and positive.  NaN / Inf in the floats are no errors.  One H2D copy, one launch and one D2H copy on the context's stream, scratch of the context; threads
 * calling with their own contexts run concurrently. */
int  ccm_fuse_sim3_eval(ccm_ctx* ctx, int K, const float* kf_rec /* 10 K */, const int32_t* feat_off /* K + 1 */, const float* feat_xy, const uint8_t* feat_octave,
                        const uint8_t* feat_desc, const int32_t* cell_off /* 3601 K */, const int32_t* cell_idx, const float* Scw /* 12 K */, int nlevels,
                        const float* scale_factors, float logScaleFactor, float th, int P, const float* pos /* 3 P */, const float* normal /* 3 P */,
                        const float* min_dist, const float* max_dist, const uint8_t* pt_desc /* 32 P */, uint32_t* table /* K P */, int32_t* n_valid /* K */,
                        int32_t* n_hit /* K */, float* uv /* 2 K P or NULL */);

/* ---- SearchInNeighbors: every Fuse(pKF, vpMapPoints, th) of one LocalMapping::SearchInNeighbors, both directions -----------------------
 * LocalMapping::SearchInNeighbors (cslam/src/Mapping.cpp:471-547) calls ORBmatcher::Fuse(pKF, vpMapPoints, 3) (ORBmatcher.cpp:854-993) once per fuse target with the
 * current keyframe's points and once on the current keyframe with the targets' points.  This call evaluates the loop body of every pair of a JOB LIST up to its
 * decision, bit-identical to the reference (the lines are csrc/fuse_math.h, which also compiles for the host).
 * Stateless; the skips (isBad(), IsInKeyFrame, mbDoNotReplace) and the map mutations stay the caller's (cslam::SearchInNeighborsBatch replays them).
 * Keyframes, per-call values and points: as for ccm_fuse_sim3_eval, with two differences.  pose + 15 k = GetRotation() (9, row-major), GetTranslation() (3),
 * GetCameraCenter() (3) of keyframe k, in place of Scw; inv_level_sigma2[nlevels] = mvInvLevelSigma2.
 * Jobs: job j < J is keyframe job_kf[j] against the points job_pt0[j] .. job_pt0[j] + job_n[j] - 1.  Jobs may share keyframes and points; ranges may overlap.
 * Out: table has sum(job_n) words, job j's at the prefix sum of job_n, in point order; a word is ccm_fuse_sim3_eval's with status 5 = no candidate passed the level
 * filter and the gate e2 * inv_level_sigma2[octave] > 5.99.  n_valid[j] / n_hit[j]: the job's pairs with status >= 4 / == 7.  uv (nullable, 2 sum(job_n)).
 * J == 0, K == 0, P == 0 and job_n[j] == 0 are legal.  CCM_E_ARG, with nothing launched: whatever ccm_fuse_sim3_eval refuses (K * P > INT32_MAX among it), a null
 * inv_level_sigma2, null job arrays with J > 0, job_kf outside [0, K), a negative job_n or job_pt0, a job that ends beyond P, sum(job_n) > INT32_MAX.  NaN / Inf in
 * the floats are no errors.  One H2D copy, one launch and one D2H copy on the context's stream. */
int  ccm_fuse_pose_eval(ccm_ctx* ctx, int K, const float* kf_rec /* 10 K */, const int32_t* feat_off /* K + 1 */, const float* feat_xy, const uint8_t* feat_octave,
                        const uint8_t* feat_desc, const int32_t* cell_off /* 3601 K */, const int32_t* cell_idx, const float* pose /* 15 K */, int nlevels,
                        const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos /* 3 P */,
                        const float* normal /* 3 P */, const float* min_dist, const float* max_dist, const uint8_t* pt_desc /* 32 P */, int J,
                        const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table /* sum(job_n) */, int32_t* n_valid /* J */,
                        int32_t* n_hit /* J */, float* uv /* 2 sum(job_n) or NULL */);

/* ---- Keyframe feature store: the keyframes' static data of the two Fuse stages, resident on the device ------------------------------------
 * What ccm_fuse_sim3_eval / ccm_fuse_pose_eval read of a keyframe never changes after the keyframe is built (Replace / AddObservation touch point descriptors
 * alone), so it is uploaded once: kf_rec, feat_xy, feat_octave, feat_desc and the 75 x 48 grid as a CSR.  Fixed capacity: max_kf slots of max_feat
 * features (1 .. 65 535, rounded up to a multiple of 16), max_kf * max_feat <= INT32_MAX; nothing grows.
 * One handle is shared by all threads; every call uses the CALLER's context (same device as the handle, else CCM_E_ARG); add / erase / clear are serialised and
 * finished on the device when they return; the resident evaluators and get run concurrently and hold a reader lock from their key lookup to the end of their
 * download, so an erase waits for them. */
typedef struct ccm_kfstore ccm_kfstore;
int  ccm_kfstore_create(ccm_ctx* ctx, int max_kf, int max_feat, ccm_kfstore** out);
void ccm_kfstore_destroy(ccm_kfstore* store);
/* M >= 0 keyframes in one upload and one launch; arrays as for ccm_fuse_sim3_eval.  cell_off == cell_idx == NULL: the grid is built on the device by the keyframe's
 * own rule, KeyFrame::AssignFeaturesToGrid with KeyFrame::PosInGrid (KeyFrame.cpp:206-225, :265-275: the int bounds kf_rec[4], [5] and the inverses kf_rec[8], [9];
 * a keypoint outside the grid is in no cell; ascending feature index inside a cell) — the grid of every keyframe born from a message.  Both given: the caller's grid
 * (a Frame-born keyframe's, built from the Frame's float bounds), held to ccm_fuse_sim3_eval's rules except that it may end below the feature count.
 * Refusals leave the store untouched: CCM_E_STATE for a live key, a key repeated within the call, fewer than M free slots; CCM_E_ARG for a keyframe with more
 * than max_feat features, null pointers, one grid pointer without the other, and the offset / index rules. */
int  ccm_kfstore_add(ccm_kfstore* store, ccm_ctx* ctx, int M, const int64_t* keys /* M */, const float* kf_rec /* 10 M */, const int32_t* feat_off /* M + 1 */,
                     const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off /* 3601 M or NULL */,
                     const int32_t* cell_idx /* or NULL */);
/* frees the key's slot for reuse; an unknown key is a no-op */
int  ccm_kfstore_erase(ccm_kfstore* store, ccm_ctx* ctx, int64_t key);
int  ccm_kfstore_clear(ccm_kfstore* store, ccm_ctx* ctx);
int  ccm_kfstore_count(ccm_kfstore* store, int* live, int* free_slots);
/* one slot's grid as the device holds it: n features, n_in of them in the grid, cell_off[3601] (nullable), cell_idx[n_in] (nullable; room for n).  An unknown
 * key: CCM_E_ARG */
int  ccm_kfstore_get(ccm_kfstore* store, ccm_ctx* ctx, int64_t key, int* n, int* n_in, int32_t* cell_off, int32_t* cell_idx);
/* gives the live key its DBoW2::FeatureVector (mFeatVec) in the flat form of cslam::FeatureVectorView: nn node ids ascending, off[nn + 1] and the features of each
 * node in ascending index (the order addFeature pushes them).  Validated and uploaded as they are (the indices in 16 bits); nothing is sorted or built.  A second
 * call for the key replaces the first; erase, clear and the reuse of the slot drop the vector.  nn == 0 and off[nn] < n (features whose word is stopped are in no
 * node) are legal.  CCM_E_ARG, with the store untouched: a key that is not live, nn < 0, null pointers with nn > 0, node ids negative or not strictly ascending,
 * off[0] != 0, an empty node, an index outside [0, n) of the key, indices that do not ascend inside a node, a feature listed twice.  Locking is add's. */
int  ccm_kfstore_set_featvec(ccm_kfstore* store, ccm_ctx* ctx, int64_t key, int nn, const int32_t* node /* nn */, const int32_t* off /* nn + 1 */,
                             const int32_t* idx /* off[nn] */);
/* The M >= 0 keyframes of a message or a loaded map in ONE call: what KeyFrame::KeyFrame(ccmslam_msgs::KF*) and ProcessAfterLoad do per
 * keyframe through ComputeBoW and AssignFeaturesToGrid.  The keyframes go into free slots with their grid built on the device (ccm_kfstore_add with cell_off ==
 * cell_idx == NULL), every feature descends the vocabulary (ccm_bow_transform's rule, node at level L - levelsup), each keyframe's mBowVec and mFeatVec are built
 * on the device, bit-identical to TemplatedVocabulary::transform with BowVector::addWeight / normalize (a feature whose weight is not > 0 is in neither vector;
 * a word's value is its weights added in feature order; the norm is added in ascending word id and divided by), the feature vector is written into the slot as
 * ccm_kfstore_set_featvec would have, and both vectors come back.  One upload (the descriptors travel once), at most three launches, one download.
 * F = feat_off[M].  Keyframe m: bow_n[m] words and values from feat_off[m]; fv_nn[m] nodes from feat_off[m]; fv_nn[m] + 1 node offsets from feat_off[m] + m, the
 * first 0; the nodes' features from feat_off[m].  What lies behind a keyframe's counts is written as zeros.  feat_word / feat_node (both NULL or both given): the
 * descent's result per feature, ccm_bow_transform's word_out / node_out.
 * Refusals leave the store and the outputs untouched: every refusal of ccm_kfstore_add without a grid; CCM_E_ARG also for a NULL vocabulary, a vocabulary on another
 * device than the store, null output pointers, and a keyframe with more than KFI_MAX_FEAT = 4096 features (such a keyframe keeps the route ccm_bow_transform,
 * ccm_kfstore_add, ccm_kfstore_set_featvec).  The vocabulary's device arrays are read in place; the caller's context and stream; locking is add's. */
int  ccm_kfstore_ingest(ccm_kfstore* store, ccm_ctx* ctx, const ccm_vocab* voc, int levelsup, int M, const int64_t* keys /* M */, const float* kf_rec /* 10 M */,
                        const int32_t* feat_off /* M + 1 */, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, int32_t* bow_n /* M */,
                        int32_t* bow_word /* F */, double* bow_value /* F */, int32_t* fv_nn /* M */, int32_t* fv_node /* F */, int32_t* fv_off /* F + M */,
                        int32_t* fv_idx /* F */, int32_t* feat_word /* F or NULL */, int32_t* feat_node /* F or NULL */);

/* ccm_fuse_sim3_eval / ccm_fuse_pose_eval on keyframes of the store: keyframe k of the call is the live key keys[k] (a key may appear more than once), Scw / pose
 * per k as there.  Outputs, packing, statuses, counters and refusals are those of the two calls above; additionally CCM_E_ARG, with nothing launched, for a NULL
 * store, a store on another device and a key that is not live.  The upload carries the slot list, Scw / pose, the per-call tables and the points. */
int  ccm_fuse_sim3_eval_resident(ccm_ctx* ctx, ccm_kfstore* store, int K, const int64_t* keys /* K */, const float* Scw /* 12 K */, int nlevels,
                                 const float* scale_factors, float logScaleFactor, float th, int P, const float* pos /* 3 P */, const float* normal /* 3 P */,
                                 const float* min_dist, const float* max_dist, const uint8_t* pt_desc /* 32 P */, uint32_t* table /* K P */,
                                 int32_t* n_valid /* K */, int32_t* n_hit /* K */, float* uv /* 2 K P or NULL */);
int  ccm_fuse_pose_eval_resident(ccm_ctx* ctx, ccm_kfstore* store, int K, const int64_t* keys /* K */, const float* pose /* 15 K */, int nlevels,
                                 const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos /* 3 P */,
                                 const float* normal /* 3 P */, const float* min_dist, const float* max_dist, const uint8_t* pt_desc /* 32 P */, int J,
                                 const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table /* sum(job_n) */,
                                 int32_t* n_valid /* J */, int32_t* n_hit /* J */, float* uv /* 2 sum(job_n) or NULL */);

/* ---- ComputeSim3's two projected searches on keyframes of the store (the lines are csrc/fuse_math.h) -----------------------------------------
 * ccm_sim3_project_eval_resident: ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (cslam/src/ORBmatcher.cpp:308-446) for every (keyframe, point)
 * pair on the INITIAL vpMatched.  The pair is ccm_fuse_sim3_eval's (Sim3 decomposition, the four gates, PredictScale, the window, levels level - 1 .. level, TH_LOW)
 * with one rule more: feature f of keyframe k with feat_skip[skip_off[k] + f] != 0 (vpMatched[f] set) is skipped in the arg-min (:393).  A skipped feature in the
 * window still makes the window non-empty; when every candidate is skipped or off-level the status is 5.  What the reference's loop changes while it runs (the
 * claims of the points before) is the caller's to replay (cslam::Sim3ProjectionSearch, host/ccm_host.h).  Arguments, outputs, packing and refusals as
 * ccm_fuse_sim3_eval_resident; additionally CCM_E_ARG, with nothing launched, for a skip_off that does not start at 0 or decreases, a mask whose length
 * skip_off[k + 1] - skip_off[k] is not the feature count of key k in the store, and a null feat_skip with skip_off[K] > 0. */
int  ccm_sim3_project_eval_resident(ccm_ctx* ctx, ccm_kfstore* store, int K, const int64_t* keys /* K */, const float* Scw /* 12 K */,
                                    const int32_t* skip_off /* K + 1 */, const uint8_t* feat_skip, int nlevels, const float* scale_factors, float logScaleFactor,
                                    float th, int P, const float* pos /* 3 P */, const float* normal /* 3 P */, const float* min_dist, const float* max_dist,
                                    const uint8_t* pt_desc /* 32 P */, uint32_t* table /* K P */, int32_t* n_valid /* K */, int32_t* n_hit /* K */,
                                    float* uv /* 2 K P or NULL */);
/* ccm_sim3_pair_eval_resident: the two directional searches of ORBmatcher::SearchBySim3 (ORBmatcher.cpp:1124-1348) as a job list in ccm_fuse_pose_eval's layout;
 * one SearchBySim3 call is two jobs.  Job j projects the points job_pt0[j] .. + job_n[j] into the TARGET keyframe keys[job_kf[j]]:
 * p3Dc_b = sR_ba * (R_aw * X + t_aw) + t_ba with job_src_pose + 12 j = R_aw (9, row-major), t_aw (3) of the SOURCE keyframe and job_T + 12 j = sR_ba (9), t_ba (3)
 * (sR21, t21 for the direction 1 -> 2; sR12, t12 for 2 -> 1; ssm_derive of csrc/fuse_math.h makes them of s12, R12, t12).  job_K4 + 4 j = fx fy cx cy of the
 * projection: the reference reads them from pKF1 for BOTH directions (:1127-1130), so both jobs of a call carry pKF1's; the image bounds, the grid and the window are
 * the target's.  Depth, IsInImage, the range 0.8 min .. 1.2 max on the norm of the camera point, PredictScale, the window, levels level - 1 .. level, threshold
 * TH_HIGH = 100 (status 6: best above it); no viewing-angle gate (status 3 does not occur), no skip mask, no normals.  Outputs and refusals as
 * ccm_fuse_pose_eval_resident; additionally CCM_E_ARG for null job_K4 / job_src_pose / job_T with J > 0. */
int  ccm_sim3_pair_eval_resident(ccm_ctx* ctx, ccm_kfstore* store, int K, const int64_t* keys /* K */, int nlevels, const float* scale_factors, float logScaleFactor,
                                 float th, int P, const float* pos /* 3 P */, const float* min_dist, const float* max_dist, const uint8_t* pt_desc /* 32 P */, int J,
                                 const int32_t* job_kf, const float* job_K4 /* 4 J */, const float* job_src_pose /* 12 J */, const float* job_T /* 12 J */,
                                 const int32_t* job_pt0, const int32_t* job_n, uint32_t* table /* sum(job_n) */, int32_t* n_valid /* J */, int32_t* n_hit /* J */,
                                 float* uv /* 2 sum(job_n) or NULL */);

/* ---- ComputeSim3's SearchByBoW for all candidates on keyframes of the store (the lines are csrc/bow_search_math.h) ----------------------------------
 * Job j is one ORBmatcher::SearchByBoW(pKF1, pKF2, ...) (cslam/src/ORBmatcher.cpp:565-698) of the live keys key1[j], key2[j], both with a feature vector, evaluated
 * on the INITIAL vbMatched2 (all false).  live1 + live1_off[j] / live2 + live2_off[j]: one byte per feature of the keyframe, != 0 where the slot's map point is set
 * and not bad.  table + live1_off[j] holds one word per feature idx1 of keyframe 1 (bsm_pack / bsm_status / bsm_best / bsm_node2): status 0 when idx1 is not live,
 * in no node, or its node does not occur in keyframe 2; otherwise the reduction (:609-639) over the live features of the same node of keyframe 2 in list order,
 * status 1 when none is live, 2 when evaluated.  n_query[j]: words with status >= 1; n_dist[j]: Hamming distances evaluated.  What the reference's loop changes while
 * it runs (vbMatched2 claims) is the caller's to replay (cslam::SearchByBoWBatch, host/ccm_host.h).  One upload (slot pairs, offsets, mask bytes; no descriptors, no
 * feature vectors), ONE launch, one download, under the store's reader lock.  J == 0, nn == 0, key1[j] == key2[j] and one key in several jobs are legal.
 * CCM_E_ARG, with nothing launched: a NULL store, a store on another device, a key that is not live, a key without a feature vector, an offset array that does not
 * start at 0 or decreases, a mask whose length is not the key's feature count in the store, null masks with a positive length, null outputs. */
int  ccm_bow_pair_eval_resident(ccm_ctx* ctx, ccm_kfstore* store, int J, const int64_t* key1 /* J */, const int64_t* key2 /* J */, const int32_t* live1_off /* J + 1 */,
                                const uint8_t* live1, const int32_t* live2_off /* J + 1 */, const uint8_t* live2, uint64_t* table /* live1_off[J] */,
                                int32_t* n_query /* J */, int32_t* n_dist /* J */);

/* ---- CreateNewMapPoints' SearchForTriangulation for all neighbours on keyframes of the store (the lines are csrc/tri_search_math.h) -----------------
 * Job j is one ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, ...) (cslam/src/ORBmatcher.cpp:700-852) of the live keys key1[j], key2[j], both with a feature
 * vector.  has1 + has1_off[j] / has2 + has2_off[j]: one byte per feature of the keyframe, != 0 where GetMapPoint(idx) is non-null (bad or not, :743-747, :760-764).
 * job_epi + 11 j: F12 (9 floats, row-major), then the epipole ex, ey of keyframe 1's centre in keyframe 2 (:708-714); NaN and Inf are no error (every comparison is
 * then false, on host and device alike).  scale_factors / level_sigma2: mvScaleFactors / mvLevelSigma2 of keyframe 2, nlevels entries, the same for every job.
 * table + has1_off[j] holds one word per feature idx1 of keyframe 1 (tsm_pack / tsm_status / tsm_idx / tsm_dist): 0 when idx1 has a map point, is in no node, or
 * its node does not occur in keyframe 2; otherwise status 1 (no candidate accepted; bestDist 50) or 2 with bestIdx2 and bestDist as the loop :756-785 leaves them:
 * the smallest distance <= 50 among the candidates without a map point that pass the epipole gate and CheckDistEpipolarLine, at its LAST position in list order.
 * The reference never sets vbMatched2, so the words are the call's whole result before the rotation histogram (cslam::SearchForTriangulationBatch, host/ccm_host.h).
 * n_query[j]: words with status >= 1; n_match[j]: words with status 2; n_dist[j]: the sum over the queries of their node's candidates without a map point.
 * A store feature of keyframe 2 whose octave is >= nlevels is no candidate and neither table is read for it (as in ccm_fuse_pose_eval_resident); it still counts in
 * n_dist.  One upload, ONE launch, one download of 4 bytes per feature, under the store's reader lock.  J == 0, nn == 0, key1[j] == key2[j] and one key in several
 * jobs are legal.  CCM_E_ARG, with nothing launched and the outputs untouched: the refusals of ccm_bow_pair_eval_resident; nlevels outside 1 .. 256; with J > 0 a
 * null job_epi, null level tables or null outputs. */
int  ccm_tri_search_eval_resident(ccm_ctx* ctx, ccm_kfstore* store, int J, const int64_t* key1 /* J */, const int64_t* key2 /* J */, const int32_t* has1_off /* J + 1 */,
                                  const uint8_t* has1, const int32_t* has2_off /* J + 1 */, const uint8_t* has2, const float* job_epi /* 11 J */, int nlevels,
                                  const float* scale_factors, const float* level_sigma2, uint32_t* table /* has1_off[J] */, int32_t* n_query /* J */,
                                  int32_t* n_match /* J */, int32_t* n_dist /* J */);

/* ---- The refresh of map points after a map stage, on keyframes of the store (the lines are csrc/mappoint_math.h) -----------------------------------
 * MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) for P map points whose observers are live
 * keys.  Point p owns the observations obs_off[p] .. obs_off[p + 1]: the caller's non-bad observers in the order it iterates mObservations, each as (obs_kf: index
 * into keys, obs_feat: feature index in that keyframe).  kf_center + 3 k: GetCameraCenter() of keys[k].
 * Descriptor part: best_obs[p] is what ccm_distinctive_descriptors returns for the same rows (exact Hamming distances with a zero diagonal, the median element
 * (int)(0.5 * (N - 1)) of the sorted row, the FIRST index with the least median), -1 for an empty list.  best_desc + 32 p (nullable) receives the winner's 32 bytes;
 * an empty list leaves that row untouched.
 * Normal / depth part: the arithmetic of ccm_update_normal_and_depth (f32 in the reference's operand order, the norm in double, the sum in LIST order) on pos + 3 p,
 * with the level read from the store: the octave of feature ref_feat[p] of keys[ref_kf[p]] (what observations[pRefKF] yields; 0 when the reference keyframe is no
 * observer, which is the caller's to pass).  ref_kf[p] == -1 skips the part (MapPoint::Replace needs the descriptor alone); an empty list keeps the three values; a
 * store octave >= nlevels means neither table entry is read, the point keeps its three values and status says so.  normal / min_dist / max_dist are in/out.
 * status[p]: MPM_DESC (1) the descriptor part ran, MPM_NORMAL_DEPTH (2) the three values were written, MPM_OCTAVE_BEYOND (4).
 * One upload (8 bytes per observation, no descriptors), ONE launch, one download, under the store's reader lock.  P == 0, K == 0 with no observation, one key listed
 * twice and one keyframe observing a point twice are legal.  CCM_E_ARG, with nothing launched and every output untouched: a NULL store, a store on another device, a
 * key that is not live, an obs_off that does not start at 0 or decreases, more than 256 observations of one point, obs_kf outside [0, K), obs_feat or ref_feat
 * outside the key's feature count, ref_kf outside [-1, K), nlevels outside 1 .. 256, null arrays with a positive length, null pos / kf_center while some
 * ref_kf >= 0. */
int  ccm_mappoint_refresh_resident(ccm_ctx* ctx, ccm_kfstore* store, int K, const int64_t* keys /* K */, const float* kf_center /* 3 K */, int P,
                                   const int32_t* obs_off /* P + 1 */, const int32_t* obs_kf /* obs_off[P] */, const int32_t* obs_feat /* obs_off[P] */,
                                   const float* pos /* 3 P */, const int32_t* ref_kf /* P */, const int32_t* ref_feat /* P */, int nlevels, const float* scale_factors,
                                   int32_t* best_obs /* P */, uint8_t* best_desc /* 32 P or NULL */, float* normal /* 3 P */, float* min_dist /* P */,
                                   float* max_dist /* P */, uint8_t* status /* P */);

#ifdef __cplusplus
}
#endif
#endif /* CCM_HIP_H */
