// ccm_host_c.h — the C entry points of libccm_host.so (the host mirror of the reference's class API, ccm_host.h; defined in host/c_*.cpp): flat arrays in, flat arrays out.
// Used by the drop-in translation units under shim/ (which include the REFERENCE's class headers and therefore cannot include ccm_host.h, whose classes carry
// the same names) and by the Python harness.  Every entry returns -1000 when the device path throws (missing library, HIP error): there is no CPU fallback.
// `device` selects the GPU; each calling thread keeps one context per device for its lifetime (SURVEY 8b threading).
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int ccmh_search_by_projection_mp(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* fdesc, int N, float minX, float minY, float maxX, float maxY, const float* scale_factors, int n_mp, const uint8_t* in_view, const float* px, const float* py, const int32_t* lvl, const float* vcos, const uint8_t* mp_desc, float th, float nnratio, int32_t* frame_mp);
int ccmh_search_by_projection_last(int device, const float* kx, const float* ky, const int32_t* oct, const float* kangle, const uint8_t* fdesc, int N, float minX, float minY, float maxX, float maxY, const float* scale_factors, int n_last, const uint8_t* valid, const float* u, const float* v, const int32_t* l_oct, const float* l_angle, const uint8_t* l_desc, float th, int check_ori, int32_t* cur_mp);
int ccmh_local_ba(int device, int n_cam, int n_pt, int n_edge, double* cam_qt, const uint8_t* cam_fixed, const double* cam_K, double* pt_xyz, const int32_t* e_cam, const int32_t* e_pt, const double* e_obs, const double* e_info, uint8_t* to_erase);
int ccmh_search_by_projection_mp_dev(int device, const float* K, const float* dist, int n_dist, int w, int h, const void* kps_raw, const uint8_t* fdesc, int N, const float* scale_factors, int n_mp, const uint8_t* in_view, const float* px, const float* py, const int32_t* lvl, const float* vcos, const uint8_t* mp_desc, float th, float nnratio, int32_t* frame_mp, float* xy_un_out);
int ccmh_search_by_projection_last_dev(int device, const void* kps_un, const uint8_t* cdesc, int N, int w, int h, const float* scale_factors, int n_last, const uint8_t* valid, const float* u, const float* v, const int32_t* oct, const float* angle, const uint8_t* mp_desc, float th, int check_ori, int32_t* frame_mp);
int ccmh_optimize_sim3(int device, double* sim3, int n, const double* P1c, const double* P2c, const double* obs1, const double* obs2, const double* info1, const double* info2, const double* K1, const double* K2, float th2, int fix_scale, uint8_t* keep);
int ccmh_orb_extract(int device, int nfeatures, const uint8_t* img, int w, int h, void* kps_out, uint8_t* desc_out, int cap);
int ccmh_search_bow(int device, int mode, const int32_t* n1, const int32_t* o1, const int32_t* i1, int nn1, const int32_t* n2, const int32_t* o2, const int32_t* i2, int nn2, const uint8_t* has1, const uint8_t* has2, const uint8_t* d1, const float* x1, const float* y1, const float* a1, int N1, const uint8_t* d2, const float* x2, const float* y2, const int32_t* oct2, const float* a2, int N2, const float* F12, float ex, float ey, const float* sigma2_2, const float* sf2, float nnratio, int check_ori, int32_t* out);
/* the SearchForTriangulation fan-out of a new keyframe (Mapping.cpp:335) as ONE device launch: create computes the Hamming tables of all neighbours, resolve replays the
 * reference's sequential rules of the call against neighbour j with the map-point flags as they are at that call (NULL: as at create) */
void* ccmh_tri_batch_create(int device, float nnratio, int check_ori, const int32_t* n1, const int32_t* o1, const int32_t* i1, int nn1, const uint8_t* has1, const uint8_t* d1, const float* x1, const float* y1, const float* a1, int N1, int n_nb, const int32_t* const* n2, const int32_t* const* o2, const int32_t* const* i2, const int32_t* nn2, const uint8_t* const* has2, const uint8_t* const* d2, const float* const* x2, const float* const* y2, const int32_t* const* oct2, const float* const* a2, const int32_t* N2);
int ccmh_tri_batch_resolve(void* h, int j, const uint8_t* has1_now, const uint8_t* has2_now, const float* F12, float ex, float ey, const float* sigma2_2, const float* sf2, int32_t* matches12);
long long ccmh_tri_batch_candidates(void* h);
void ccmh_tri_batch_destroy(void* h);
/* the arithmetic between SearchForTriangulation and `new MapPoint` (Mapping.cpp:353-448) for every neighbour of a new keyframe (cslam::NewMapPointBatch): create sends the
 * predicted matches (idx12 = idx1 idx2 per match, CSR over pair_off[n_nb + 1]) out as ONE ccm_triangulate_pairs launch; points answers the matches neighbour j has NOW from
 * that table, the others through the same arithmetic on the host, and returns the number accepted (status / x3d as ccm_triangulate_pairs).  cam records: 21 floats each.
 * device < 0 asks for the host evaluator by name (no device is touched); with a device, a device error makes create return NULL.  create_tri takes the prediction from a
 * ccmh_tri_batch handle resolved with the flags of its build (F12 9 floats and exy = epipole x y per neighbour; oct1 = octaves of keyframe 1's features).
 * stats: out3 = predicted, hit, missed matches. */
void* ccmh_newpts_create(int device, const float* cam1, int N1, const float* x1, const float* y1, const int32_t* oct1, int n_nb, const float* cam2, const int32_t* N2, const float* const* x2, const float* const* y2, const int32_t* const* oct2, const int32_t* pair_off, const int32_t* idx12, int nlevels, const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2, float ratio_factor);
void* ccmh_newpts_create_tri(int device, void* tri_batch, const int32_t* oct1, const float* cam1, const float* cam2, const float* F12, const float* exy, int nlevels, const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2, float ratio_factor);
int ccmh_newpts_points(void* h, int j, int n, const int32_t* idx12, uint8_t* status, float* x3d);
int ccmh_newpts_stats(void* h, int64_t* out3);
void ccmh_newpts_destroy(void* h);
int ccmh_triangulate_pairs_host(const float* cam1, int S, const float* cam2, const int32_t* pair_off, const float* xy, const int32_t* oct, int nlevels, const float* sigma2_1, const float* sf_1, const float* sigma2_2, const float* sf_2, float ratio_factor, uint8_t* status, float* x3d, int32_t* n_accepted);
/* the Sim3 correction of a loop's / merged map's keyframes and points (cslam::Sim3MapCorrection, ONE ccm_sim3_correct_map call).  Keyframes 0 .. n_kf - 1: the set in walk
 * order, center[3 n_obs_kf]: theirs, then the outside observers'.  loop form: keyframe i lists list_pt[list_off[i] .. list_off[i + 1]) (< 0: null), list_skip[e] != 0: bad or
 * tagged already.  epilogue form: pt_kf[p] = keyframe whose Sim3 pair moves point p (< 0: skip).  Points 0 .. n_pt - 1 as ccm_sim3_correct_map.  device < 0 asks for the host
 * evaluator by name (no device is touched); with a device, a device error makes create return NULL.  results: any pointer may be NULL; tag[p] = keyframe that corrected p, -1 none.
 * ccmh_sim3_correct_map_host: the arguments of ccm_sim3_correct_map after the context through the same header on the calling thread (0, or -1 for its CCM_E_ARG cases). */
void* ccmh_sim3corr_create_loop(int device, int n_kf, int n_obs_kf, const float* Tiw, const float* center, int cur, const float* Twc, const double* Scw, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels);
void* ccmh_sim3corr_create_epilogue(int device, int n_kf, int n_obs_kf, const float* center, const double* S_non, const double* S_cor, const int32_t* pt_kf, int n_pt, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels);
int ccmh_sim3corr_results(void* h, float* pos, float* normal, float* min_dist, float* max_dist, int32_t* tag, float* Tiw_new, float* center_new, double* S_non, double* S_cor);
void ccmh_sim3corr_destroy(void* h);
int ccmh_sim3_correct_map_host(int n_kf, const float* Tiw, int cur, const float* Twc, const double* Scw, double* S_non, double* S_cor, int n_obs_kf, const float* kf_center, const int32_t* kf_rank, int n_pt, const float* pos, const int32_t* owner, const int32_t* owner_rank, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, float* pos_out, float* normal, float* min_dist, float* max_dist, float* Tiw_new, float* center_new);
/* a finished global BA applied to the map (cslam::GbaMapUpdate, ONE ccm_gba_apply_map call).  Keyframes by id 0 .. n_kf - 1 with origins[n_origins], the child sets in CSR over
 * child_off[n_kf + 1], kf_cam (-1: no vertex), Tcw / Twc 12 floats each; points with pos, vert (landmark or -1) and ref_kf (keyframe id or -1); the optimised state as
 * ccm_ba_download returns it.  device < 0 asks for the host evaluator by name (no device is touched); with a device, a device error makes create return NULL.
 * sizes: out4 = keyframes the walk reached, keyframes reached twice (> 0: nothing evaluated, take the sequential walk), points whose reference keyframe is tagged but unreached
 * (left untouched), points.  results: any pointer may be NULL; order / parent / T_new / Twc_new per walk position.
 * ccmh_gba_apply_map_host: the host form of ccm_gba_apply_map after the context through the same header on the calling thread (0, or -1 for its CCM_E_ARG cases). */
void* ccmh_gbaupd_create(int device, int n_kf, int n_origins, const int32_t* origins, const int32_t* child_off, const int32_t* child_kf, const int32_t* kf_cam, const float* Tcw, const float* Twc, int n_pt, const float* pos, const int32_t* vert, const int32_t* ref_kf, int n_cam, const double* cam_qt, int n_lm, const double* pt_xyz);
int ccmh_gbaupd_sizes(void* h, int64_t* out4);
int ccmh_gbaupd_results(void* h, int32_t* order, int32_t* parent, float* T_new, float* Twc_new, float* pos, uint8_t* status);
void ccmh_gbaupd_destroy(void* h);
int ccmh_gba_apply_map_host(int n_kf, const int32_t* kf_parent, const int32_t* kf_cam, const float* Tcw_old, const float* Twc_old, int n_pt, const float* pos, const int32_t* pt_vert, const int32_t* pt_ref, int n_cam, const double* cam_qt, int n_lm, const double* pt_xyz, float* T_new, float* Twc_new, float* pos_out, uint8_t* pt_status);
/* KeyFrame::UpdateConnections over a corrected set (cslam::CovisibilityBatch, ONE ccm_covis_update call; arguments as there).  device < 0 asks for the host evaluator by
 * name (no device is touched); with a device, a device error makes create return NULL.  sizes: out5 = n_kf, entries of the count rows, of the final rows, of the ordered
 * lists, outside AddConnection calls.  results: any pointer may be NULL; outside = target source weight per call, in the reference's order.  best / by_weight:
 * GetBestCovisibilityKeyFrames(N) / GetCovisiblesByWeight(w) of keyframe i, returns the length (min(length, cap) written).
 * ccmh_covis_update_host: the arguments of ccm_covis_update after the context through the same header on the calling thread (0, or -1 for its CCM_E_ARG cases). */
void* ccmh_covis_create(int device, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th);
int ccmh_covis_sizes(void* h, int64_t* out5);
int ccmh_covis_results(void* h, int32_t* flags, int32_t* row_off, int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* outside);
int ccmh_covis_best(void* h, int i, int N, int32_t* out, int cap);
int ccmh_covis_by_weight(void* h, int i, int w, int32_t* out, int cap);
void ccmh_covis_destroy(void* h);
int ccmh_covis_update_host(int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip, int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags, int32_t* needed);
/* LocalMapping::KeyFrameCullingV3's walk (cslam::KeyFrameCullingBatch, ONE ccm_kfcull_walk call; arguments as there).  device < 0 asks for the host evaluator by name (no
 * device is touched); with a device, a device error makes create return NULL.  results: any pointer may be NULL.  culled / points_gone: the candidates SetBadFlag is
 * called on in walk order / the points the walk turned bad; returns the length (min(length, cap) written).
 * ccmh_kfcull_walk_host: the arguments of ccm_kfcull_walk after the context through the same header on the calling thread (0, or -1 for its CCM_E_ARG cases).
 * ccmh_kfcull_walk_mapcopy_model: the walk on std::map observations copied per checked slot, a cost model of the reference's containers; verdicts only. */
void* ccmh_kfcull_create(int device, int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt, const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad, int th_obs, double thres, int n_levels);
int ccmh_kfcull_results(void* h, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone, int32_t* pt_nobs, int32_t* n_reeval);
int ccmh_kfcull_culled(void* h, int32_t* out, int cap);
int ccmh_kfcull_points_gone(void* h, int32_t* out, int cap);
void ccmh_kfcull_destroy(void* h);
int ccmh_kfcull_walk_host(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt, const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad, int th_obs, double thres, int n_levels, uint8_t* verdict, int32_t* n_mps, int32_t* n_red, uint8_t* pt_gone, int32_t* pt_nobs_out, int32_t* n_reeval);
int ccmh_kfcull_walk_mapcopy_model(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt, const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad, int th_obs, double thres, int n_levels, uint8_t* verdict);
int ccmh_search_for_initialization(int device, const float* x1, const float* y1, const int32_t* oct1, const float* a1, const uint8_t* d1, int N1, const float* x2, const float* y2, const int32_t* oct2, const float* a2, const uint8_t* d2, int N2, float minX, float minY, float maxX, float maxY, float* prev_xy, int window, float nnratio, int check_ori, int32_t* matches12);
int ccmh_projected_window_search(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, int N, float minX, float minY, float maxX, float maxY, const float* scale_factors, const float* inv_sigma2, int n_pts, const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, float th, int chi2_gate, int dist_threshold, int32_t* matched, int claim, const uint8_t* no_claim, int32_t* best_idx, int32_t* best_dist);
void* ccmh_fuse_batch_create(int device, int S, const int32_t* kf_off, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, const float* bounds4, const float* scale_factors, const float* inv_sigma2, const int32_t* pt_off, const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, float th);
void* ccmh_fuse_batch_create_cand(int device, int S, const int32_t* kf_off, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, const float* const* inv_sigma2, const int32_t* pt_off, const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, const int32_t* cand_off, const int32_t* cand_base, const int32_t* cand_idx, int chi2_gate, int dist_threshold);
long long ccmh_fuse_batch_candidates(void* h);
int ccmh_fuse_batch_resolve(void* h, int s, const uint8_t* skip_now, int n_pts, int32_t* best_idx, int32_t* best_dist);
void ccmh_fuse_batch_destroy(void* h);
int ccmh_projected_window_search_cand(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, int N, const float* inv_sigma2, int n_pts, const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, const int32_t* cand_off, const int32_t* cand_idx, int chi2_gate, int dist_threshold, int32_t* matched, int claim, const uint8_t* no_claim, int32_t* best_idx, int32_t* best_dist);
int ccmh_projected_window_search_dev(int device, const float* kx, const float* ky, const int32_t* oct, const uint8_t* kdesc, int N, float maxX, float maxY, const float* scale_factors, const float* inv_sigma2, int n_pts, const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* pdesc, float th, int chi2_gate, int dist_threshold, int32_t* matched, int claim, const uint8_t* no_claim, int32_t* best_idx, int32_t* best_dist);
int ccmh_bow_transform(int device, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id, const double* weight, const uint8_t* desc, int N, int levelsup, int32_t* bow_ids, double* bow_vals, int32_t* fv_nodes, int32_t* fv_off, int32_t* fv_idx, int32_t* sizes );
/* KeyFrameDatabase::DetectLoopCandidates / DetectMapMatchCandidates / DetectRelocalizationCandidates (Database.cpp:72-439) through the host mirror, on a
 * ccm_kfdb handle: kind 0 loop, 1 map match, 2 relocalisation; n_allow < 0 = every keyframe; neighbours = GetBestCovisibilityKeyFrames(10) as a table over
 * nb_key.  Returns the number of candidates (min(that, cap) written to out), -1000 on a device error. */
int ccmh_kfdb_detect(void* db, int device, int kind, int n, const int32_t* word, const double* value, float min_score, int64_t self_key, const int64_t* allow, int n_allow, const int64_t* exclude, int n_exclude, uint64_t exclude_groups, int n_nb_keys, const int64_t* nb_key, const int32_t* nb_off, const int64_t* nb_list, int64_t* out, int cap);
/* Sim3 RANSAC of LoopFinder / MapMatcher::ComputeSim3 (cslam::Sim3RansacBatch): candidate c = correspondences pt_off[c] .. pt_off[c+1] (mvX3Dc1 / mvX3Dc2 3 floats each,
 * mvnMaxError1 / 2, idx1 = mvnIndices1), n1[c] = mN1, K1 / K2 = fx fy cx cy per candidate.  draws: raw rand() values to use instead of ::rand() (NULL: ::rand()), after
 * the calling thread's FIFO.  next: 1 = a Sim3 (inliers[0 .. min(cap, mN1)) = vbInliers), 0 = every candidate discarded, -1 = the supplied draws ran out, -1000 = device
 * error.  draws_pending: the calling thread's FIFO of drawn but unused values (length returned, min(length, cap) copied front first). */
void* ccmh_sim3_ransac_create(int device, int K, const int32_t* pt_off, const float* X3Dc1, const float* X3Dc2, const float* K1, const float* K2, const uint32_t* max_err1, const uint32_t* max_err2, const int32_t* n1, const int32_t* idx1, double probability, int min_inliers, int max_iterations, int solver_iterations, int fix_scale, const int32_t* draws, int64_t n_draws);
int ccmh_sim3_ransac_next(void* h, int32_t* cand, float* R9, float* t3, float* s, uint8_t* inliers, int cap, int32_t* n_inliers);
int ccmh_sim3_ransac_stats(void* h, int64_t* out3);
void ccmh_sim3_ransac_destroy(void* h);
/* one Sim3Solver::iterate(n_iterations) of a single solver (shim/Sim3Solver_hip.cpp): state = [mnIterations, mnBestInliers] in / out, draws from ::rand()
 * through the thread's FIFO; flags = [success, bNoMore, best moved, its inliers], best_rts / best_mask written when the best moved.  0, or -1000 on a device error. */
int ccmh_sim3_solver_iterate(int device, int N, const float* X3Dc1, const float* X3Dc2, const float* K1, const float* K2, const uint32_t* max_err1, const uint32_t* max_err2, int fix_scale, int min_inliers, int max_iterations, int n_iterations, int32_t* state, float* best_rts, uint32_t* best_mask, int32_t* flags);
int ccmh_sim3_draws_pending(int32_t* out, int cap);
void ccmh_sim3_draws_clear(void);
/* cslam::TwoViewInitializer (the H / F RANSAC and CheckRT of cslam::Initializer).  device < 0: the host evaluator.  keys: x y pairs of mvKeysUn; sets: 8 match
 * indices per iteration.  find: scores3 = SH SF RH, best2 = the winning iterations (-1: none), inl_h / inl_f one byte per match; returns the number of matches,
 * -1 bad arguments, -1000 a device error.  check_rt: n_hyp motions of 12 floats (R row-major, t), inliers one byte per match; per hypothesis n_good, parallax,
 * p3d (3 N1), good (N1), status (matches).  draw_sets: Initializer.cpp:73-93 on raw rand() values (8 * iterations of them). */
void* ccmh_twoview_create(int device, const float* K9, int N1, const float* keys1, float sigma);
int ccmh_twoview_find(void* h, int N2, const float* keys2, const int32_t* matches12, int n_sets, const int32_t* sets, float* scores3, int32_t* best2, float* H21, float* F21, uint8_t* inl_h, uint8_t* inl_f);
int ccmh_twoview_check_rt(void* h, int n_hyp, const float* Rt, const uint8_t* inliers, float th2, int32_t* n_good, float* parallax, float* p3d, uint8_t* good, uint8_t* status);
void ccmh_twoview_destroy(void* h);
int ccmh_twoview_draw_sets(int N, int iterations, const int32_t* raw, int32_t* sets);
/* twoview_math.h compiled for the host: the arguments of ccm_twoview_ransac_eval / ccm_twoview_check_rt without the context (model: 0 both, 1 H only, 2 F only, for
 * the two-thread baseline of scripts/twoview_profile.py), Normalize, Mat::inv() of a 3x3, the CheckRT record, the three SVD shapes (shape 0: 16x9 -> vt.row(8) in
 * out[0..9); 1: 8x9 -> vt in out[0..81); 2: 3x3 -> w, u, vt in out[0..21)) and the score of given models (model 0 H with its inverse computed here, 1 F). */
int ccmh_twoview_ransac_eval_host(int N, const float* xy1, const float* xy2, const float* pn1, const float* pn2, const float* T1, const float* T2inv, const float* T2t, float sigma, int H, const int32_t* sets, int model, float* scoreH, float* scoreF, float* H21, float* F21, uint32_t* maskH, uint32_t* maskF);
int ccmh_twoview_check_rt_host(int n_hyp, const float* rec, const float* K9, int N, const float* xy1, const float* xy2, const uint32_t* inlier_mask, float th2, uint8_t* status, float* x3d, float* cos_parallax);
void ccmh_twoview_normalize(const float* xy, int n, float* pn, float* T9);
void ccmh_twoview_inv33(const float* S9, float* D9);
void ccmh_twoview_prepare_rt(const float* K9, const float* R9, const float* t3, float* rec27);
int ccmh_twoview_svd(int shape, const float* A, float* out);
int ccmh_twoview_score_host(int model, int n_models, const float* M, int N, const float* xy1, const float* xy2, float sigma, float* score, uint32_t* mask);
/* pnp_math.h (cslam::PnPsolver's EPnP and CheckInliers) compiled for the host.  compute_pose: n >= 4 correspondences (pws 3 n, us 2 n, cam = fu fv uc vc) -> R (row-major), t,
 * rep_errors[0..4) (entry 0 unused) and the chosen solution 1..3.  ransac_eval_host: the arguments of ccm_pnp_ransac_eval without the context (0, or -1 for its CCM_E_ARG
 * cases).  check_inliers: CheckInliers of one pose (Rt12 = R, t) over N points; returns mnInliersi, error2 (nullable) per point.  refine: Refine's compute_pose on the
 * points of best_inliers and its CheckInliers; returns mnRefinedInliers.  matrices: M' M, PW0' PW0 and CC of a compute_pose call, before their decompositions.
 * primitive: the restated C-API calls — which 0 / 1: cvSVD(MODIFY_A | U_T) of a 3x3 / 12x12 (out = w, then Ut); 2: cvSVD(MODIFY_A) with U and V of a 3x3 (out = w, U, V);
 * 3: cvInvert(CV_SVD) of a 3x3; 4 / 5 / 6: cvSolve(CV_SVD) of a 6x3 / 6x4 / 6x5 system; 7 / 8: cvMulTransposed(., ., 1) of rows x 3 / rows x 12; 9: qr_solve of a 6x4
 * system, out = X in and out, returns 1, or 0 at the singular exit. */
int ccmh_pnp_compute_pose(int n, const double* pws, const double* us, const double* cam4, double* R9, double* t3, double* rep_errors4, int32_t* chosen);
int ccmh_pnp_ransac_eval_host(int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* max_err, const double* cam, int H, const int32_t* hyp_cand, const int32_t* hyp_idx, int32_t* n_inl, double* Rt, int32_t* mask_off, uint32_t* mask);
int ccmh_pnp_check_inliers(int N, const float* P3Dw, const float* P2D, const float* max_err, const double* cam4, const double* Rt12, uint8_t* inliers, float* error2);
int ccmh_pnp_refine(int N, const float* P3Dw, const float* P2D, const float* max_err, const double* cam4, const uint8_t* best_inliers, double* Rt12, uint8_t* inliers);
int ccmh_pnp_matrices(int n, const double* pws, const double* us, const double* cam4, double* mtm144, double* pca9, double* cc9);
int ccmh_pnp_primitive(int which, int rows, const double* A, const double* b, double* out);
/* cslam::PnPRansacBatch (the PnPsolver of every relocalisation candidate and the round-robin of iterate()).  device < 0: the host evaluator.  candidate c = correspondences
 * pt_off[c] .. pt_off[c+1] (mvP3Dw 3 floats, mvP2D 2, mvSigma2, kp_idx = mvKeyPointIndices), n_matches[c] = vpMapPointMatches.size(), cam = fu fv uc vc (f64) per candidate;
 * the other arguments are SetRansacParameters' (min_set must be 4) and the nIterations of the round-robin's calls.  draws: raw rand() values to use instead of ::rand()
 * (NULL: ::rand()), after the calling thread's FIFO (ccmh_sim3_draws_pending: Sim3 and PnP share it).  next / iterate: 1 = a pose (Tcw 4x4 f32 row-major, inliers[0 ..
 * min(cap, n_matches)) = vbInliers, flags2 = [refined, bNoMore]), 0 = every candidate discarded / the call returned no pose (flags2[1] = bNoMore), -1 = the supplied
 * draws ran out, -1000 = an error.  stats: draws taken from the source, hypotheses, evaluator calls, Refine computations.  info: mnIterations, mRansacMaxIts,
 * mRansacMinInliers, discarded. */
void* ccmh_pnp_ransac_create(int device, int K, const int32_t* pt_off, const float* P3Dw, const float* P2D, const float* sigma2, const double* cam, const int32_t* n_matches, const int32_t* kp_idx, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2, int solver_iterations, const int32_t* draws, int64_t n_draws);
int ccmh_pnp_ransac_next(void* h, int32_t* cand, float* Tcw16, uint8_t* inliers, int cap, int32_t* n_inliers, int32_t* flags2);
int ccmh_pnp_ransac_iterate(void* h, int c, int n_iterations, float* Tcw16, uint8_t* inliers, int cap, int32_t* n_inliers, int32_t* flags2);
int ccmh_pnp_ransac_stats(void* h, int64_t* out4);
int ccmh_pnp_ransac_info(void* h, int c, int32_t* out4);
void ccmh_pnp_ransac_destroy(void* h);
/* cslam::SearchAndFuseBatch (every Fuse call of a SearchAndFuse from ONE ccm_fuse_sim3_eval call; arguments as there).  device < 0 asks for the host evaluator by name;
 * create returns NULL on bad arguments or a device error.  table: any pointer may be NULL.  resolve: the k-th Fuse call with the caller's current skips and descriptors
 * (both nullable); returns nFused, -1000 on an error, -1001 when n_pts is not the batch's.  eval_host: the arguments of ccm_fuse_sim3_eval after the context through
 * csrc/fuse_math.h on the calling thread (0, or -1 for its CCM_E_ARG cases); n_cand (nullable, K P): the size of vIndices per pair.  decompose: ORBmatcher.cpp:1004-1008. */
void* ccmh_fuse_sim3_create(int device, int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc);
int ccmh_fuse_sim3_table(void* h, uint32_t* table, int32_t* n_valid, int32_t* n_hit);
int ccmh_fuse_sim3_resolve(void* h, int k, const uint8_t* skip_now, const uint8_t* desc_now, int n_pts, int32_t* best_idx, int32_t* best_dist);
long long ccmh_fuse_sim3_n_reeval(void* h);
void ccmh_fuse_sim3_destroy(void* h);
int ccmh_fuse_sim3_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv, int32_t* n_cand);
void ccmh_fuse_sim3_decompose(const float* Scw12, float* pose15);
/* cslam::SearchInNeighborsBatch (both directions of a SearchInNeighbors from ONE ccm_fuse_pose_eval call; the keyframe, per-call and point arguments as there).  The
 * first n_current points are the current keyframe's, the rest the predicted fuse candidates; target[n_calls] = the keyframe of each call, current = the current
 * keyframe's index (-1: none).  device < 0 asks for the host evaluator by name; create returns NULL on bad arguments or a device error.  resolve / resolve_current
 * return nFused, -1000 on an error, -1001 when n_pts is not the batch's.  eval_host: ccm_fuse_pose_eval's arguments after the context on the calling thread. */
void* ccmh_fuse_pose_create(int device, int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int n_calls, const int32_t* target, int current, int n_current);
int ccmh_fuse_pose_table(void* h, uint32_t* table, int32_t* n_valid, int32_t* n_hit);
int ccmh_fuse_pose_resolve(void* h, int c, const uint8_t* skip_now, const uint8_t* desc_now, int n_pts, int32_t* best_idx, int32_t* best_dist);
int ccmh_fuse_pose_resolve_current(void* h, int n, const int32_t* slot, const uint8_t* skip_now, const uint8_t* desc_now, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* desc, int32_t* best_idx, int32_t* best_dist);
long long ccmh_fuse_pose_n_reeval(void* h);
long long ccmh_fuse_pose_n_unpredicted(void* h);
void ccmh_fuse_pose_destroy(void* h);
int ccmh_fuse_pose_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv, int32_t* n_cand);
void ccmh_to_se3quat(const float* Tcw16, double* qt7);
void ccmh_se3quat_to_cvmat(const double* qt7, float* Tcw16);
void ccmh_sim3_to_cvse3(const double* s8, float* Tcw16);
/* cslam::KeyFrameStore.  device < 0 at create asks for the host-only store by name; create returns NULL on bad arguments or a device error.  The
 * `device` of the other calls names the calling thread's context (ignored by a host-only store).  add returns 0, CCM_E_ARG (-1) or CCM_E_STATE (-6) as
 * ccm_kfstore_add does, -1000 on a device error; get returns -1 for a key that is not live.  eval_resident_host: the resident calls' arguments after the context on the
 * store's shadows through csrc/fuse_math.h (0, or -1 for their CCM_E_ARG cases).  create_resident: the batches' constructors on keys of a store; the handles are
 * used and destroyed through ccmh_fuse_sim3_* / ccmh_fuse_pose_* above. */
void* ccmh_kfstore_create(int device, int max_kf, int max_feat);
void ccmh_kfstore_destroy(void* h);
int ccmh_kfstore_add(void* h, int device, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx);
int ccmh_kfstore_erase(void* h, int device, int64_t key);
int ccmh_kfstore_clear(void* h, int device);
int ccmh_kfstore_count(void* h, int* live, int* free_slots);
void* ccmh_kfstore_handle(void* h);   /* the ccm_kfstore* of include/ccm_hip.h, NULL for a host-only store */
int ccmh_kfstore_get(void* h, int device, int64_t key, int* n, int* n_in, int32_t* cell_off, int32_t* cell_idx);
int ccmh_fuse_sim3_eval_resident_host(void* store, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int ccmh_fuse_pose_eval_resident_host(void* store, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
void* ccmh_fuse_sim3_create_resident(void* store, int device, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc);
void* ccmh_fuse_pose_create_resident(void* store, int device, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int n_calls, const int32_t* target, int current, int n_current);
/* ComputeSim3's two projected searches.  eval_host / eval_resident_host: the arguments of ccm_sim3_project_eval_resident /
 * ccm_sim3_pair_eval_resident after the context through csrc/fuse_math.h on the calling thread, on flat keyframe arrays (as ccmh_fuse_sim3_eval_host) or on a store's
 * shadows; 0, or -1 for the CCM_E_ARG cases.  ccmh_ssm_derive: ORBmatcher.cpp:1141-1143.  ccmh_sim3_project_*: cslam::Sim3ProjectionSearch (device < 0: the host
 * evaluation; create returns NULL on bad arguments, a key that is not live or a device error; resolve returns nmatches, -1000 on an error, -1001 when n_pts / n_feat are
 * not the search's).  ccmh_search_by_sim3_resident: cslam::SearchBySim3Batch in one call; returns nFound, -1000 on bad arguments or a device error; matches12 (N1),
 * vn1 (N1), vn2 (N2), n_valid2 / n_hit2 (2) are nullable. */
int ccmh_sim3_project_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int ccmh_sim3_pair_eval_host(int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4, const float* job_src_pose, const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int ccmh_sim3_project_eval_resident_host(void* store, int K, const int64_t* keys, const float* Scw, const int32_t* skip_off, const uint8_t* feat_skip, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
int ccmh_sim3_pair_eval_resident_host(void* store, int K, const int64_t* keys, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const float* job_K4, const float* job_src_pose, const float* job_T, const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv);
void ccmh_ssm_derive(float s12, const float* R12, const float* t12, float* sR12, float* sR21, float* t21);
void* ccmh_sim3_project_create(void* store, int device, int64_t key, const float* Scw12, const uint8_t* matched0, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc);
int ccmh_sim3_project_table(void* h, uint32_t* table, int32_t* n_valid, int32_t* n_hit);
int ccmh_sim3_project_resolve(void* h, const uint8_t* skip_now, const int32_t* existing_idx, int n_feat, int32_t* matched, int n_pts, int32_t* best_idx, int32_t* remap);
long long ccmh_sim3_project_n_reeval(void* h);
void ccmh_sim3_project_destroy(void* h);
int ccmh_search_by_sim3_resident(void* store, int device, int64_t key1, int64_t key2, int N1, const uint8_t* live1, const float* pos1, const float* min1, const float* max1, const uint8_t* desc1, const float* pose1, int N2, const uint8_t* live2, const float* pos2, const float* min2, const float* max2, const uint8_t* desc2, const float* pose2, float s12, const float* R12, const float* t12, const int32_t* matches12_in, int nlevels, const float* scale_factors, float logScaleFactor, float th, int32_t* matches12, int32_t* vn1, int32_t* vn2, int32_t* n_valid2, int32_t* n_hit2);
/* The store's feature vectors and ComputeSim3's SearchByBoW for all candidates.  ccmh_kfstore_set_featvec: cslam::KeyFrameStore::set_featvec
 * (0, CCM_E_ARG (-1), -1000 on a device error; angle nullable).  ccmh_bow_pair_eval_resident_host: ccm_bow_pair_eval_resident's arguments after the context on the
 * store's shadows through csrc/bow_search_math.h (0, or -1 for the CCM_E_ARG cases).  ccmh_bow_batch_*: cslam::SearchByBoWBatch (device < 0: the host evaluation;
 * create returns NULL on bad arguments, a key that is not live or has no feature vector, or a device error).  live2 + live2_off[j]: candidate j's mask.  result
 * returns nmatches of candidate j and copies matches12 (n_feat entries, nullable); -1000 for j out of range, -1001 when n_feat is not key1's feature count. */
int ccmh_kfstore_set_featvec(void* h, int device, int64_t key, int nn, const int32_t* node, const int32_t* off, const int32_t* idx, const float* angle);
/* cslam::KeyFrameStore::ingest on flat arrays: ccm_kfstore_ingest's arguments, outputs and refusals, and angle (nullable) for the shadows.
 * ccmh_kfstore_ingest: a device store, voc = the ccm_vocab* of include/ccm_hip.h.  ccmh_kfstore_ingest_host: the host-only store, the flat tree of ccm_vocab_create
 * evaluated by csrc/kfingest_math.h on the calling thread (-1000 for a device store). */
int ccmh_kfstore_ingest(void* h, int device, void* voc, int levelsup, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
                        const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, int32_t* bow_n, int32_t* bow_word, double* bow_value, int32_t* fv_nn,
                        int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node);
/* A test aid (the shadows are the mirror's own and no C entry returns them): 1: the shadows of `key` in the two stores are equal in every field (floats by their
 * bits), 0: they differ, -1: the key is not live in both.  Bound in ccm_slam_amd/kfstore.py; the tests of ingest compare a store after ingest with one after
 * add + set_featvec, and the device mirror with the host-only one. */
int ccmh_kfstore_shadow_equal(void* a, void* b, int64_t key);
int ccmh_kfstore_ingest_host(void* h, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id,
                             const double* weight, int levelsup, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
                             const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, int32_t* bow_n, int32_t* bow_word, double* bow_value,
                             int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node);
int ccmh_bow_pair_eval_resident_host(void* store, int J, const int64_t* key1, const int64_t* key2, const int32_t* live1_off, const uint8_t* live1, const int32_t* live2_off, const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist);
void* ccmh_bow_batch_create(void* store, int device, int64_t key1, int C, const int64_t* keys2, const uint8_t* live1, const int32_t* live2_off, const uint8_t* live2, float nnratio, int check_orientation);
int ccmh_bow_batch_result(void* h, int j, int n_feat, int32_t* matches12);
int ccmh_bow_batch_table(void* h, uint64_t* table, int32_t* n_query, int32_t* n_dist);
long long ccmh_bow_batch_n_reeval(void* h);
void ccmh_bow_batch_destroy(void* h);
/* CreateNewMapPoints' SearchForTriangulation for all neighbours.  ccmh_tri_search_eval_resident_host: ccm_tri_search_eval_resident's arguments
 * after the context on the store's shadows through csrc/tri_search_math.h (0, or -1 for the CCM_E_ARG cases).  ccmh_tri_search_*: cslam::SearchForTriangulationBatch
 * (device < 0: the host evaluation; create returns NULL on bad arguments, a key that is not live or has no feature vector, or a device error).  has2 + has2_off[j]:
 * neighbour j's map-point bytes; epi + 11 j: its F12 (row-major), ex, ey.  resolve returns nmatches of neighbour j under has1_now / has2_now (nullable: the flags of
 * the build) and copies matches12 (n_feat entries, nullable); -1000 for j out of range, -1001 when n_feat is not key1's feature count. */
int ccmh_tri_search_eval_resident_host(void* store, int J, const int64_t* key1, const int64_t* key2, const int32_t* has1_off, const uint8_t* has1, const int32_t* has2_off, const uint8_t* has2, const float* job_epi, int nlevels, const float* scale_factors, const float* level_sigma2, uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist);
void* ccmh_tri_search_create(void* store, int device, int64_t key1, int C, const int64_t* keys2, const uint8_t* has1, const int32_t* has2_off, const uint8_t* has2, const float* epi, const float* sigma2_2, const float* sf2, int nlevels, int check_orientation);
int ccmh_tri_search_resolve(void* h, int j, const uint8_t* has1_now, const uint8_t* has2_now, int n_feat, int32_t* matches12);
int ccmh_tri_search_table(void* h, uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist);
long long ccmh_tri_search_n_reeval(void* h);
void ccmh_tri_search_destroy(void* h);
/* The refresh of map points after a map stage.  ccmh_mappoint_refresh_eval_resident_host: ccm_mappoint_refresh_resident's arguments after the
 * context on the store's shadows through csrc/mappoint_math.h (0, or -1 for the CCM_E_ARG cases, the outputs untouched).  ccmh_mappoint_refresh_*:
 * cslam::MapPointRefresh (device < 0: the host evaluation; create returns NULL on bad arguments, a key that is not live or a device error); result copies the
 * accessors for P points, has_desc[p] = descriptor(p) != nullptr, and returns -1 when P is not the mirror's. */
int ccmh_mappoint_refresh_eval_resident_host(void* store, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels, const float* scale_factors, int32_t* best_obs, uint8_t* best_desc, float* normal, float* min_dist, float* max_dist, uint8_t* status);
void* ccmh_mappoint_refresh_create(void* store, int device, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, const float* normal, const float* min_dist, const float* max_dist, int nlevels, const float* scale_factors);
int ccmh_mappoint_refresh_result(void* h, int P, int32_t* best_obs, uint8_t* desc, uint8_t* has_desc, float* normal, float* min_dist, float* max_dist, uint8_t* status);
void ccmh_mappoint_refresh_destroy(void* h);
/* The guided search of relocalisation, ORBmatcher::SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist), and the refine chain behind a PnP pose (DESIGN.md
 * section 28).  pose / frame: a ccm_guided_pose (include/ccm_hip.h: Tcw 12 floats, logScaleFactor, nScaleLevels as int32, scaleFactors 16 floats).  The frame is given as
 * undistorted keypoints (the ccm_keypoint layout) and descriptors; bounds = mnMinX mnMinY mnMaxX mnMaxY; the forms with a device build a FrameGridDev of a w x h image
 * without distortion.  ccmh_guided_search_host: ccm_frame_guided_search's arguments after the frame through csrc/guided_search_math.h and a host grid, no device (0, or
 * -1 for its CCM_E_ARG cases).  ccmh_search_by_projection_kf_*: nmatches, frame_mp = F.mvpMapPoints in/out (a keyframe slot or -1); -1 for a bad argument (orb_dist
 * outside 0 .. 255 among them), -1000 when the device path throws; _cand is the drop-in's form: the lists are the caller's own Frame::GetFeaturesInArea results (CSR over
 * the P slots), ONE ccm_hamming_csr launch and the sequential pass.  ccmh_reloc_refine: cslam::RelocalizationRefine; 1 matched, 0 not; frame_mp, Tcw16, trace5 (nGood of
 * optimisation 1, nadd of search 1, nGood 2, nadd 2, nGood 3; -1: the step did not run) and n_good are outputs. */
int ccmh_guided_search_host(const void* kps_un, const uint8_t* fdesc, int N, const float* bounds, const float* K, const void* pose, int P, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const uint8_t* skip, float th, uint8_t* status, float* u, float* v, int32_t* level, int32_t* cand_off, int32_t* cand_idx, uint16_t* cand_dist, int64_t cap, int64_t* n_cand);
int ccmh_search_by_projection_kf_host(const void* kps_un, const uint8_t* fdesc, int N, const float* bounds, const float* K, const void* pose, int P, const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const float* angle, const uint8_t* already_found, float th, int orb_dist, int check_ori, int32_t* frame_mp);
int ccmh_search_by_projection_kf_dev(int device, const float* K, int w, int h, const void* kps_un, const uint8_t* fdesc, int N, const void* pose, int P, const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const float* angle, const uint8_t* already_found, float th, int orb_dist, int check_ori, int32_t* frame_mp);
int ccmh_search_by_projection_kf_cand(int device, const uint8_t* fdesc, const float* f_angle, int N, int P, const uint8_t* desc, const float* kf_angle, const int32_t* cand_off, const int32_t* cand_idx, int orb_dist, int check_ori, int32_t* frame_mp);
int ccmh_reloc_refine(int device, const float* K, int w, int h, const void* kps_un, const uint8_t* fdesc, int N, const float* inv_level_sigma2, const void* frame, int P, const uint8_t* live, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* desc, const float* angle, const int32_t* matches_f, const uint8_t* inliers, int32_t* frame_mp, float* Tcw16, int32_t* trace5, int32_t* n_good);

#ifdef __cplusplus
}
#endif
