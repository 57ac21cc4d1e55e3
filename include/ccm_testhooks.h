/* ccm_testhooks.h — TEST-ONLY entry points of libccm_testhooks.so (ccm_slam_amd/csrc/test_hooks.hip).  Not part of the product's C ABI:
 * libccm_hip.so exports none of these names and include/ccm_hip.h declares none; the library links against the product and reaches the
 * file-local kernels through the C++-linkage functions of ccm_slam_amd/csrc/test_internal.h.  Used by tests/ and scripts/ only. */
#ifndef CCM_TESTHOOKS_H
#define CCM_TESTHOOKS_H
#include "ccm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* one of the structure arrays that ccm_ba_create built on the device (ba_build.hip), by name; out == NULL only queries *bytes */
int  ccm_ba_debug_array(ccm_ba* ba, const char* name, void* out, size_t cap_bytes, size_t* bytes);

/* test hook: DistributeOctTree as the DEVICE runs it (orb_octree_kernel, one workgroup) on one level's candidates: integer positions inside the
 * level's W x H border box, responses 1..255, positions unique; sel_out: indices of the kept candidates in output order.  *overflow = 1 when
 * the set does not fit the kernel's LDS plan (the extractor then selects on the host). */
int  ccm_orb_debug_octree_dev(ccm_ctx* ctx, const int32_t* x, const int32_t* y, const int32_t* response, int n, int W, int H, int N,
                              int32_t* sel_out, int cap, int* n_out, int* overflow);

/* intermediate products for parity tests (host copies; any pointer may be NULL):
 * FAST score map and blurred image of one level of the LAST extracted frame.              */
int  ccm_orb_debug_level(ccm_orb* orb, int level, uint8_t* score_out, uint8_t* blur_out);
/* host wall-clock phases of the last ccm_orb_extract call, ms: [queue phase 1, wait for candidates, octree, queue phase 2,
 * wait + D2H, total] */
int  ccm_orb_debug_timing(const ccm_orb* orb, double out_ms[6]);
/* pre-octree FAST candidates of the last frame: returns count for the level, fills up to cap */
int  ccm_orb_debug_candidates(ccm_orb* orb, int level, ccm_keypoint* out, int cap, int* n_out);

/* test hook: this rank's partial reduced camera system [36*(n_free_cams+n_blocks) S | 6*n_free_cams b]
 * at the current state, i.e. the buffer the per-trial RCCL all-reduce sums; out == NULL only queries *count. */
int  ccm_ba_debug_partial_reduced(ccm_ba* ba, double lambda, double* out, size_t cap, size_t* count);

/* test hook: coarse level of the two-level PCG preconditioner at the current state: *na aggregates (0 = not in use), Ac and
 * its inverse [6 na x 6 na], prolongation blocks P_k = Ad(T_cw,k) [n_free_cams x 36]; cap = doubles available in Ac / Ainv. */
int  ccm_ba_debug_coarse(ccm_ba* ba, double lambda, int* na, double* Ac, double* Ainv, double* Pm, size_t cap);

/* test hook: ONE solve of the persistent PCG (ba_pcg_persist) of (S + lambda I) x = b at the current state, the coarse level on (coarse != 0, built at
 * this lambda) or off; x_out: [6 n_free_cams]; flags: [0] done, [1] CG iterations, [2] numeric failure, [3] the launch gave up waiting for its peers.
 * CCM_E_STATE when the handle has no persistent solver (or no coarse level although one is asked for). */
int  ccm_ba_debug_pcg_solve(ccm_ba* ba, double lambda, int coarse, double rel_tol, int max_it, double* x_out, size_t cap, int* flags);

/* TEST-ONLY in-process communicator: the ranks are threads of one process sharing one GPU, each with its own ccm_ctx; an all-reduce is
 * a rendezvous plus one reduction kernel that leaves the same bits in every rank's buffer (RCCL's contract).  Lets a single-GPU box
 * execute the complete multi-rank control flow of the sharded global BA (tests/test_sharded_loopback_gpu.py). */
int  ccm_comm_loopback_create(int nranks, void** group);
void ccm_comm_loopback_destroy(void* group);
int  ccm_comm_init_loopback(ccm_ctx* ctx, void* group, int rank);

/* test hook for the dense f64 Cholesky (MFMA tiles) behind ccm_pose_graph_optimize: solves A x = b for a host matrix
 * (n x n row-major, symmetric positive definite); *info = 0 or (the smallest column whose pivot is not positive and finite) + 1, in
 * every hook of this family. */
int  ccm_debug_dense_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info);
/* the same solve with a tile plan (what CCM_PG_SOLVER=dense runs): the panel, the trailing update and the substitutions visit only the
 * 64 x 64 tiles that a symbolic elimination of A's non-zero tiles marks. */
int  ccm_debug_planned_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info);
/* test hook for the tile-sparse, level-scheduled form of the same factorisation (what ccm_pose_graph_optimize uses by default): only the
 * non-zero 64 x 64 tiles of the factor are stored, tile columns of one elimination level run in one launch; the tile pattern is taken from
 * the non-zeros of A.  levels / tiles (nullable) receive the plan's level and tile counts. */
int  ccm_debug_tile_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info, int* levels, int* tiles);
/* same machinery, explicit inverse (used for the coarse level of the BA preconditioner) */
int  ccm_debug_dense_inverse(ccm_ctx* ctx, const double* A, int n, double* Ainv, int* info);

/* test hook for ccm_pose_graph_optimize: ONE linearisation of the graph at its given state and ONE solve of (H + lambda I) x = b, by the kernels and
 * launch shapes of the product path.  solver: 0 tile-sparse Cholesky, 1 dense Cholesky, 2 PCG with the spanning-forest preconditioner (at most
 * 2600 free vertices, else CCM_E_ARG), 3 block-Jacobi PCG; each is forced at any size.  rel_tol / max_it: the PCG stop rule and iteration limit.
 * r_in (nullable, 7F, solvers 2 and 3 only): z_out receives M^-1 r_in from one application of the solver's preconditioner.
 * The caller sets the three capacities and the pointers (any pointer may be null); F, nBlk, E_active and flags are written back.
 * F free vertices in vertex order; E_active edges with a free end, active[e] = their index in the edge list; blocks (blk_a, blk_b), blk_a <= blk_b, the F
 * diagonal ones first, H[49 nBlk] row-major with rows of blk_a; J[e][side][49] with J[k * 7 + d] = d err_k / d update_d; flags = done, iterations,
 * numeric failure, ended by the stall rule.  Forest (solver 2), per free vertex: t_parent (free slot or -1: a fixed vertex or none), t_code
 * (active edge * 2 + the side of this vertex, -1: root of a component without a fixed vertex), t_pos / t_out (DFS interval), t_order[pos]. */
typedef struct ccm_pg_debug_out {
  int32_t F, nBlk, E_active, reserved;
  int32_t flags[4];
  size_t  cap_free, cap_edge, cap_blk;
  int32_t *blk_a, *blk_b, *active;
  double  *H, *b, *J, *err, *x, *z_out;
  int32_t *t_parent, *t_code, *t_order, *t_pos, *t_out;
} ccm_pg_debug_out;
int  ccm_debug_pg_solve(ccm_ctx* ctx, int n_vert, const double* sim3, const uint8_t* fixed, int fix_scale, int n_edge, const int32_t* e_i, const int32_t* e_j,
                        const double* meas, double lambda, int solver, double rel_tol, int max_it, const double* r_in, ccm_pg_debug_out* out);

/* test hook for ccm_slam_amd/csrc/lane_xor.h (round 6: the cross-lane moves of every xor butterfly — DPP, v_permlane16_swap / v_permlane32_swap): for MASK = 1, 2, 4, 8, 16, 32
 * the 64 lanes' from_partner<MASK>(v), add_partner<MASK>(v) and __shfl_xor(v, MASK) of in64, then [3][64]: lanex::wave_sum, the __shfl_xor butterfly of the same values, and
 * lanex::wave_incl_scan_i32 of the integer pattern (37 lane mod 101) - 20. */
int  ccm_debug_lane_xor(ccm_ctx* ctx, const double* in64, double* out_6x3x64, double* sums_3x64);

/* test hook for ccm_slam_amd/csrc/block_red.h: one workgroup of 256 threads with ONE BlockRedT<4> object, LDS laid out as in the pose optimiser's kernel, runs in a
 * single launch  sum1, sum28_lds, sum28_lds, sum1, sum27, sum27, sum64<35>, sum64<35>, sum1.  The calls' inputs follow each other in `in`, slot s of thread t of a call
 * at s * 256 + t (1, 32, 32, 1, 32, 32, 64, 64, 1 slots: n_in = 259 * 256); `out` receives EVERY thread's results the same way (1, 28, 28, 1, 28, 28, 35, 35, 1
 * results: n_out = 185 * 256).  Other sizes: CCM_E_ARG. */
int  ccm_debug_block_red(ccm_ctx* ctx, const double* in, size_t n_in, double* out, size_t n_out);
/* test hook for lane_xor.h: lanex::from_partner_c(v, off) for off = 1, 2, 4, 8, 16, 32 as an unrolled loop constant ([6][64]) and lanex::wave_min_u32 of key64, all 64 lanes */
int  ccm_debug_lane_ops(ccm_ctx* ctx, const double* in64, const uint32_t* key64, double* partner_6x64, uint32_t* min64);

/* test hook for ccm_pose_optimize: the kernel's own staging and ONE linearisation at the given pose with GIVEN level / robust bytes per edge, in the launch shape the
 * product call takes at this n (n >= 1).  acc_out[28][256]: every thread's reduced sums, [k * 256 + thread] — k = 0..20 the upper triangle of H row by row, 21..26 b,
 * 27 the robust chi2; err_out[2n]: the residuals of the active edges, 0 elsewhere; shape: transpose reduction (1) or cross-lane (0), staged in LDS, dynamic LDS bytes. */
int  ccm_debug_poseopt_linearise(ccm_ctx* ctx, const double cam_qt[7], int n, const double* Xw, const double* obs, const double* info, const double K[4],
                                 const uint8_t* level, const uint8_t* robust, double* acc_out, double* err_out, int shape[3]);

/* test hook for ccm_sim3_optimize: the kernel's own staging, the chi2 of the pairs with alive != 0 at sim3, the 14 perturbed estimates of the numeric differentiation
 * and ONE accumulation of H and b, in the launch shape the product call takes at this n (n >= 1).  acc_out[35][256]: every thread's reduced sums, [k * 256 + thread] —
 * k = 0..27 the upper triangle of H row by row, 28..34 b; chi2_out[256]: every thread's robust chi2; err_out[4n]: the residuals of both edges of the alive pairs, 0
 * elsewhere; pert_out[14][16]: for d = 0..6 S(+delta e_d) (8) | its inverse (8), then the same for -delta; J_out[n][2][14]: per pair and side (0: x1 = S X2, 1:
 * x2 = S^-1 X1) the numeric Jacobian, row 0 (7) | row 1 (7), 0 for the other pairs; shape: staged in LDS, dynamic LDS bytes. */
int  ccm_debug_sim3opt_linearise(ccm_ctx* ctx, const double sim3[8], int n, const double* P1c, const double* P2c, const double* obs1, const double* obs2,
                                 const double* info1, const double* info2, const double K1[4], const double K2[4], double th2, int fix_scale,
                                 const uint8_t* alive, double* acc_out, double* chi2_out, double* err_out, double* pert_out, double* J_out, int shape[2]);

/* test hook for ccm_covis_update: the same call with a histogram window of 64 keyframe indices, so that a small n_all spans several windows */
int  ccm_debug_covis_update_small(ccm_ctx* ctx, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt,
                                  const uint8_t* list_skip, int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off,
                                  int32_t* col, int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf,
                                  int32_t* ord_w, int32_t* flags, int32_t* needed);

/* test hook for ccm_twoview_ransac_eval: the score walk of twoview_math.h (CheckHomography for model 0, the inverse computed on the device; CheckFundamental for
 * model 1) for n_models GIVEN 3x3 models over N matches; score[n_models], mask[n_models * ceil(N / 32)] */
int  ccm_debug_twoview_score(ccm_ctx* ctx, int model, int n_models, const float* M, int N, const float* xy1, const float* xy2, float sigma, float* score,
                             uint32_t* mask);

/* test hook for ccm_kfstore_ingest / ccm_kfstore_set_featvec: a live key's feature vector as its slot holds it.  *nn = the node count (-1: the key has no
 * vector); node / off / idx (nullable; room for n + 1, n + 1 and n entries, n the key's feature count) receive node[nn], off[nn + 1], idx[off[nn]]. */
int  ccm_kfstore_debug_get_featvec(ccm_kfstore* store, ccm_ctx* ctx, int64_t key, int* nn, int32_t* node, int32_t* off, int32_t* idx);

/* test hook for ccm_slam_amd/csrc/ba_math.h and sim3_math.h: lie_eval(op, in + 48 i, out + 40 i) of csrc/test_lie_ops.h for the items i < n (1 <= n <= 2^20), one
 * lane per item in workgroups of 256.  op: the LieOp number (tests/lie_reference.py lists every op's layout).  `out` is an in-out array: the device starts from the
 * caller's values (ba_spd6_inv leaves its output untouched on a false return); out[40 i + 39] receives the flag word. */
int  ccm_debug_lie_eval(ccm_ctx* ctx, int op, int n, const double* in, double* out);

#ifdef __cplusplus
}
#endif
#endif /* CCM_TESTHOOKS_H */
