// stage_blocks.h — the staged blocks (staged_block.h) of the map stages, one declaration per segment, in device order.  Plain C++:
// tests/host/staged_block_check.cpp rebuilds them on the CPU.  The members are initialised in the order they are written, the counts first.
#pragma once
#include "staged_block.h"
#include "triangulate_math.h"
#include "fuse_math.h"
#include "kfstore_math.h"
#include "bow_search_math.h"
#include "tri_search_math.h"
#include "mappoint_math.h"

// ccm_sim3_ransac_eval: the inputs, then the outputs.
struct Sim3RansacBlock : StagedBlock {
  const size_t K, Nt, H, words;
  Sim3RansacBlock(size_t K, size_t Nt, size_t H, size_t words) : K(K), Nt(Nt), H(H), words(words) {}
  StagedSeg<int32_t> pt_off = add<int32_t>(K + 1, SB_COPY);
  StagedSeg<float> X1 = add<float>(3 * Nt, SB_COPY), X2 = add<float>(3 * Nt, SB_COPY), K1 = add<float>(4 * K, SB_COPY), K2 = add<float>(4 * K, SB_COPY);
  StagedSeg<uint32_t> thr1 = add<uint32_t>(Nt, SB_COPY), thr2 = add<uint32_t>(Nt, SB_COPY);
  StagedSeg<int32_t> hyp_cand = add<int32_t>(H, SB_COPY), hyp_idx = add<int32_t>(3 * H, SB_COPY), mask_off = add<int32_t>(H + 1, SB_COPY);
  StagedSeg<int32_t> n_inl = add<int32_t>(H, SB_OUT);
  StagedSeg<float> rts = add<float>(13 * H, SB_OUT);
  StagedSeg<uint32_t> mask = add<uint32_t>(words, SB_OUT);
};

// ccm_pnp_ransac_eval: the intrinsics (f64) lead the inputs and the poses (f64) the outputs; four sample indices per hypothesis.
struct PnpRansacBlock : StagedBlock {
  const size_t K, Nt, H, words;
  PnpRansacBlock(size_t K, size_t Nt, size_t H, size_t words) : K(K), Nt(Nt), H(H), words(words) {}
  StagedSeg<double> cam = add<double>(4 * K, SB_COPY);
  StagedSeg<int32_t> pt_off = add<int32_t>(K + 1, SB_COPY);
  StagedSeg<float> P3Dw = add<float>(3 * Nt, SB_COPY), P2D = add<float>(2 * Nt, SB_COPY), max_err = add<float>(Nt, SB_COPY);
  StagedSeg<int32_t> hyp_cand = add<int32_t>(H, SB_COPY), hyp_idx = add<int32_t>(4 * H, SB_COPY), mask_off = add<int32_t>(H + 1, SB_COPY);
  StagedSeg<double> Rt = add<double>(12 * H, SB_OUT);
  StagedSeg<int32_t> n_inl = add<int32_t>(H, SB_OUT);
  StagedSeg<uint32_t> mask = add<uint32_t>(words, SB_OUT);
};

// ccm_triangulate_pairs: the inputs, then the outputs.  xy comes first and on 16 bytes for the kernel's float4 reads; the outputs start on 16 bytes as well.
struct TriBlock : StagedBlock {
  const size_t P, S, L;
  TriBlock(size_t P, size_t S, size_t L) : P(P), S(S), L(L) {}
  StagedSeg<float> xy = add<float>(4 * P, SB_COPY, 16);
  StagedSeg<float> cam1 = add<float>(TRI_CAM_FLOATS, SB_COPY), cam2 = add<float>(TRI_CAM_FLOATS * S, SB_COPY);
  StagedSeg<float> sigma2_1 = add<float>(L, SB_COPY), sf_1 = add<float>(L, SB_COPY), sigma2_2 = add<float>(L, SB_COPY), sf_2 = add<float>(L, SB_COPY);
  StagedSeg<uint32_t> oct = add<uint32_t>(P, SB_GEN);   // oct1 | oct2 << 16
  StagedSeg<int32_t> grp = add<int32_t>(P, SB_GEN);
  StagedSeg<float> x3d = add<float>(3 * P, SB_OUT, 16);
  StagedSeg<uint8_t> status = add<uint8_t>(P, SB_OUT);
};

// ccm_sim3_correct_map: the doubles lead the inputs and the outputs.  The loop form uploads Scw, Twc and Tiw and downloads the two Sim3 tables it computes; the
// epilogue form uploads the caller's tables instead, and the tables' place among the outputs stays on the device, so the download starts behind it.  S_swi is
// read by the point kernel only.
struct S3cBlock : StagedBlock {
  const size_t K, KO, P, L, NO; const bool loop;
  S3cBlock(size_t K, size_t KO, size_t P, size_t L, size_t NO, bool loop) : K(K), KO(KO), P(P), L(L), NO(NO), loop(loop) {}
  StagedSeg<double> Scw = add<double>(8, loop ? SB_COPY : SB_ZERO), S_non_in = add<double>(loop ? 0 : 8 * K, SB_COPY), S_cor_in = add<double>(loop ? 0 : 8 * K, SB_COPY);
  StagedSeg<float> Twc = add<float>(12, loop ? SB_COPY : SB_ZERO), Tiw = add<float>(loop ? 12 * K : 0, SB_COPY);
  StagedSeg<float> c_old = add<float>(3 * KO, SB_COPY), scale_factors = add<float>(L, SB_COPY);
  StagedSeg<float> pos = add<float>(3 * P, SB_COPY), normal_in = add<float>(3 * P, SB_COPY), dmin_in = add<float>(P, SB_COPY), dmax_in = add<float>(P, SB_COPY);
  StagedSeg<int32_t> kf_rank = add<int32_t>(KO, SB_COPY), owner = add<int32_t>(P, SB_COPY), owner_rank = add<int32_t>(P, SB_COPY);
  StagedSeg<int32_t> obs_off = add<int32_t>(P ? P + 1 : 0, SB_COPY), obs_kf = add<int32_t>(NO, SB_COPY), ref_kf = add<int32_t>(P, SB_COPY), ref_level = add<int32_t>(P, SB_COPY);
  StagedSeg<double> S_non = add<double>(8 * K, loop ? SB_OUT : SB_WORK), S_cor = add<double>(8 * K, loop ? SB_OUT : SB_WORK);
  StagedSeg<float> T_new = add<float>(12 * K, SB_OUT), c_new = add<float>(3 * K, SB_OUT);
  StagedSeg<float> pos_out = add<float>(3 * P, SB_OUT), normal_out = add<float>(3 * P, SB_OUT), dmin_out = add<float>(P, SB_OUT), dmax_out = add<float>(P, SB_OUT);
  StagedSeg<double> S_swi = add<double>(8 * K, SB_WORK);
};

// ccm_covis_update: the inputs, the work arrays, the outputs.  An empty map still has obs_off[0] = 0.
struct CovisBlock : StagedBlock {
  const size_t K, A, P, NL, NO, C;
  CovisBlock(size_t K, size_t A, size_t P, size_t NL, size_t NO, size_t C) : K(K), A(A), P(P), NL(NL), NO(NO), C(C) {}
  typedef StagedSeg<int32_t> Seg;
  Seg order_key = add<int32_t>(A, SB_COPY), list_off = add<int32_t>(K + 1, SB_COPY);
  Seg list_pt = add<int32_t>(NL, SB_GEN);   // null and skipped entries: -1
  Seg obs_off = add<int32_t>(P + 1, P ? SB_COPY : SB_ZERO), obs_kf = add<int32_t>(NO, SB_COPY);
  Seg row_size = add<int32_t>(K, SB_WORK), n_ge = add<int32_t>(K, SB_WORK), fb_col = add<int32_t>(K, SB_WORK), extra_cnt = add<int32_t>(K, SB_WORK);
  Seg cursor = add<int32_t>(K, SB_WORK), chg = add<int32_t>(K, SB_WORK), extra_off = add<int32_t>(K + 1, SB_WORK);
  Seg extra_src = add<int32_t>(C, SB_WORK), extra_w = add<int32_t>(C, SB_WORK);
  Seg hdr = add<int32_t>(4, SB_OUT), flags = add<int32_t>(K, SB_OUT);
  Seg row_off = add<int32_t>(K + 1, SB_OUT), fw_off = add<int32_t>(K + 1, SB_OUT), ord_off = add<int32_t>(K + 1, SB_OUT);
  Seg col = add<int32_t>(C, SB_OUT), count = add<int32_t>(C, SB_OUT), fw_col = add<int32_t>(C, SB_OUT), fw_w = add<int32_t>(C, SB_OUT);
  Seg ord_kf = add<int32_t>(C, SB_OUT), ord_w = add<int32_t>(C, SB_OUT);
};

// ccm_kfcull_walk: the outputs lead, so that the download is the head of the block; gone / nobs go up as the caller's pt_bad / pt_nobs and the work arrays as
// zeros, so one upload carries everything up to the slot bytes, which the eval kernel writes.
struct KfcullBlock : StagedBlock {
  const size_t K, P, NL, NO;
  KfcullBlock(size_t K, size_t P, size_t NL, size_t NO) : K(K), P(P), NL(NL), NO(NO) {}
  typedef StagedSeg<int32_t> Seg;
  Seg hdr = add<int32_t>(4, SB_OUT | SB_ZERO), verdict = add<int32_t>(K, SB_OUT | SB_ZERO), n_mps = add<int32_t>(K, SB_OUT | SB_ZERO), n_red = add<int32_t>(K, SB_OUT | SB_ZERO);
  Seg gone = add<int32_t>(P, SB_OUT | SB_GEN), nobs = add<int32_t>(P, SB_OUT | SB_COPY);
  Seg sums = add<int32_t>(4 * K, SB_ZERO);
  StagedSeg<uint32_t> erased = add<uint32_t>((K + 31) / 32, SB_ZERO);   // one bit per candidate
  Seg stamp = add<int32_t>(P, SB_ZERO);
  Seg cand_flags = add<int32_t>(K, SB_GEN), list_off = add<int32_t>(K + 1, SB_COPY), list_pt = add<int32_t>(NL, SB_COPY);
  Seg obs_off = add<int32_t>(P + 1, P ? SB_COPY : SB_ZERO), obs_kf = add<int32_t>(NO, SB_COPY);
  StagedSeg<uint8_t> list_level = add<uint8_t>(NL, SB_COPY), obs_level = add<uint8_t>(NO, SB_COPY), obs_bad = add<uint8_t>(NO, SB_COPY);
  StagedSeg<uint8_t> slot = add<uint8_t>(NL, SB_WORK);
};

// ccm_gba_apply_map: the doubles lead the inputs.  The host form uploads the optimised state (C cameras, L landmarks); the handle form declares both with zero
// length and reads the handle's own buffers.  NT keyframes that were no vertices in NL levels: tree_kf / lvl_off are written by the stage while it validates.
struct GbaApplyBlock : StagedBlock {
  const size_t K, P, C, L, NT, NL;
  GbaApplyBlock(size_t K, size_t P, size_t C, size_t L, size_t NT, size_t NL) : K(K), P(P), C(C), L(L), NT(NT), NL(NL) {}
  StagedSeg<double> cam_qt = add<double>(7 * C, SB_COPY), pt_xyz = add<double>(3 * L, SB_COPY);
  StagedSeg<float> Tcw_old = add<float>(12 * K, SB_COPY), Twc_old = add<float>(12 * K, SB_COPY), pos = add<float>(3 * P, SB_COPY);
  StagedSeg<int32_t> kf_parent = add<int32_t>(K, SB_COPY), kf_cam = add<int32_t>(K, SB_COPY), pt_vert = add<int32_t>(P, SB_COPY), pt_ref = add<int32_t>(P, SB_COPY);
  StagedSeg<int32_t> tree_kf = add<int32_t>(NT, SB_GEN), lvl_off = add<int32_t>(NT ? NL + 1 : 0, SB_GEN);
  StagedSeg<float> T_new = add<float>(12 * K, SB_OUT), Twc_new = add<float>(12 * K, SB_OUT), pos_out = add<float>(3 * P, SB_OUT);
  StagedSeg<uint8_t> status = add<uint8_t>(P, SB_OUT);
};

// ccm_twoview_ransac_eval: the inputs, the models the solve kernel leaves for the score kernel, the outputs.  words = ceil(N / 32) per hypothesis and model.
struct TwoViewRansacBlock : StagedBlock {
  const size_t N, H, words;
  TwoViewRansacBlock(size_t N, size_t H) : N(N), H(H), words((N + 31) / 32) {}
  StagedSeg<float> xy1 = add<float>(2 * N, SB_COPY), xy2 = add<float>(2 * N, SB_COPY), pn1 = add<float>(2 * N, SB_COPY), pn2 = add<float>(2 * N, SB_COPY);
  StagedSeg<float> T = add<float>(27, SB_GEN);   // T1, T2inv, T2t
  StagedSeg<int32_t> sets = add<int32_t>(8 * H, SB_COPY);
  StagedSeg<float> H12 = add<float>(9 * H, SB_WORK);
  StagedSeg<float> scoreH = add<float>(H, SB_OUT), scoreF = add<float>(H, SB_OUT), H21 = add<float>(9 * H, SB_OUT), F21 = add<float>(9 * H, SB_OUT);
  StagedSeg<uint32_t> maskH = add<uint32_t>(words * H, SB_OUT), maskF = add<uint32_t>(words * H, SB_OUT);
};

// ccm_twoview_check_rt: the inputs, then the outputs.  Q motion hypotheses of 27 floats each; one inlier mask of ceil(N / 32) words.
struct TwoViewCheckRtBlock : StagedBlock {
  const size_t N, Q;
  TwoViewCheckRtBlock(size_t N, size_t Q) : N(N), Q(Q) {}
  StagedSeg<float> xy1 = add<float>(2 * N, SB_COPY), xy2 = add<float>(2 * N, SB_COPY), rec = add<float>(27 * Q, SB_COPY), K = add<float>(9, SB_COPY);
  StagedSeg<uint32_t> inl = add<uint32_t>((N + 31) / 32, SB_COPY);
  StagedSeg<float> x3d = add<float>(3 * N * Q, SB_OUT), cosp = add<float>(N * Q, SB_OUT);
  StagedSeg<uint8_t> status = add<uint8_t>(N * Q, SB_OUT);
};

// ccm_kfstore_add: M keyframes with F features in all, on their way into the slots slot[m] of the store.  The descriptors lead, on 16 bytes, for the kernel's 16-byte
// copies.  A caller-supplied grid travels as cell_off and a 16-bit cell_idx the stage writes while it validates; without one both are declared with no elements and
// the kernel builds the grid.  n_in (the features in the grid, per keyframe) comes back.
struct KfstoreAddBlock : StagedBlock {
  const size_t M, F; const bool grid;
  KfstoreAddBlock(size_t M, size_t F, bool grid) : M(M), F(F), grid(grid) {}
  StagedSeg<uint8_t> desc = add<uint8_t>(32 * F, SB_COPY, 16);
  StagedSeg<int32_t> slot = add<int32_t>(M, SB_GEN), feat_off = add<int32_t>(M + 1, SB_COPY);
  StagedSeg<float> rec = add<float>(FSM_REC_FLOATS * M, SB_COPY), xy = add<float>(2 * F, SB_COPY);
  StagedSeg<int32_t> cell_off = add<int32_t>(grid ? M * (FSM_CELLS + 1) : 0, SB_COPY);
  StagedSeg<uint16_t> cell_idx = add<uint16_t>(grid ? F : 0, SB_GEN);
  StagedSeg<uint8_t> oct = add<uint8_t>(F, SB_COPY);
  StagedSeg<int32_t> n_in = add<int32_t>(M, SB_OUT);
};

// ccm_kfstore_ingest: what KfstoreAddBlock carries without a grid goes up; the features' weights (and their words and nodes, when the caller does
// not ask for them) stay on the device between the descent and the keyframes' workgroups; the values lead the download, on 8 bytes, then n_in, the two counts per
// keyframe, the two vectors (fv_off has one entry more per keyframe) and, when asked for, the per-feature words and nodes.
struct KfIngestBlock : StagedBlock {
  const size_t M, F; const bool want_feat;
  KfIngestBlock(size_t M, size_t F, bool want_feat) : M(M), F(F), want_feat(want_feat) {}
  StagedSeg<uint8_t> desc = add<uint8_t>(32 * F, SB_COPY, 16);
  StagedSeg<int32_t> slot = add<int32_t>(M, SB_GEN), feat_off = add<int32_t>(M + 1, SB_COPY);
  StagedSeg<float> rec = add<float>(FSM_REC_FLOATS * M, SB_COPY), xy = add<float>(2 * F, SB_COPY);
  StagedSeg<uint8_t> oct = add<uint8_t>(F, SB_COPY);
  StagedSeg<double> weight = add<double>(F, SB_WORK);
  StagedSeg<int32_t> work_word = add<int32_t>(want_feat ? 0 : F, SB_WORK), work_node = add<int32_t>(want_feat ? 0 : F, SB_WORK);
  StagedSeg<double> bow_value = add<double>(F, SB_OUT);
  StagedSeg<int32_t> n_in = add<int32_t>(M, SB_OUT), bow_n = add<int32_t>(M, SB_OUT), fv_nn = add<int32_t>(M, SB_OUT);
  StagedSeg<int32_t> bow_word = add<int32_t>(F, SB_OUT), fv_node = add<int32_t>(F, SB_OUT), fv_off = add<int32_t>(F + M, SB_OUT), fv_idx = add<int32_t>(F, SB_OUT);
  StagedSeg<int32_t> feat_word = add<int32_t>(want_feat ? F : 0, SB_OUT), feat_node = add<int32_t>(want_feat ? F : 0, SB_OUT);
};

// ccm_bow_pair_eval_resident: J jobs of BSM_JOB_INTS ints each (the two slots, their node counts, the jobs' first mask bytes and first work item,
// written by the stage while it validates) and the two sides' mask bytes, M1 and M2 in all.  The table has one 64-bit word per mask byte of side 1 and leads the
// outputs, on 8 bytes; it goes up as zeros (a feature no wave meets is no query) and so do the counters, which the kernel adds to.
struct BowPairResidentBlock : StagedBlock {
  const size_t J, M1, M2;
  BowPairResidentBlock(size_t J, size_t M1, size_t M2) : J(J), M1(M1), M2(M2) {}
  StagedSeg<int32_t> job = add<int32_t>(BSM_JOB_INTS * J, SB_GEN, 16);
  StagedSeg<uint8_t> live1 = add<uint8_t>(M1, SB_COPY), live2 = add<uint8_t>(M2, SB_COPY);
  StagedSeg<uint64_t> table = add<uint64_t>(M1, SB_OUT | SB_ZERO);
  StagedSeg<int32_t> n_query = add<int32_t>(J, SB_OUT | SB_ZERO), n_dist = add<int32_t>(J, SB_OUT | SB_ZERO);
};

// ccm_tri_search_eval_resident: J jobs of TSM_JOB_INTS ints each (BowPairResidentBlock's job record, its last int the job's first float), the
// doubles 3.84 * (double)level_sigma2[l] the stage writes (they lead the rest, on 8 bytes), TSM_EPI_FLOATS floats per job (F12, ex, ey), the scale factors of the L
// levels, and the two sides' map-point bytes, M1 and M2 in all.  The table has one 32-bit word per byte of side 1; it and the three counters go up as zeros.
struct TriSearchResidentBlock : StagedBlock {
  const size_t J, M1, M2, L;
  TriSearchResidentBlock(size_t J, size_t M1, size_t M2, size_t L) : J(J), M1(M1), M2(M2), L(L) {}
  StagedSeg<int32_t> job = add<int32_t>(TSM_JOB_INTS * J, SB_GEN, 16);
  StagedSeg<double> line_thr = add<double>(L, SB_GEN);
  StagedSeg<float> job_epi = add<float>(TSM_EPI_FLOATS * J, SB_COPY), scale_factors = add<float>(L, SB_COPY);
  StagedSeg<uint8_t> has1 = add<uint8_t>(M1, SB_COPY), has2 = add<uint8_t>(M2, SB_COPY);
  StagedSeg<uint32_t> table = add<uint32_t>(M1, SB_OUT | SB_ZERO);
  StagedSeg<int32_t> n_query = add<int32_t>(J, SB_OUT | SB_ZERO), n_match = add<int32_t>(J, SB_OUT | SB_ZERO), n_dist = add<int32_t>(J, SB_OUT | SB_ZERO);
};

// The six projected searches of fuse.hip are ONE layout: K keyframes, P points, L levels, and what the form's flags add.  A segment a form does
// not have is declared with no elements, so it takes no room, moves nothing, and the offsets of each form are what they would be alone.
//   FB_FLAT  the keyframes' own arrays travel, F features in all: kdesc, rec, feat_off, cell_off, kxy, cell_idx (16-bit, written by the stage while it validates), koct.
//            Without it the kernel reads them from the keyframe store's slots, and slot[K] (written while the keys are looked up) takes their place.
//   FB_JOBS  the work is J jobs in T tiles of FPM_TILE pairs, N = the sum of the jobs' points: job (keyframe, first point, points, first table word) and tile (job,
//            first pair of the job per workgroup), written by the stage while it validates the job arrays; the counters are per job and the table has N words.
//            Without it every keyframe meets every point: K counters, K * P words.
//   FB_CHI2  Fuse's pose form: inv_sigma2, and pose is the caller's (Rcw, tcw, Ow); the Sim3 forms' pose is the decomposed Scw, written by the stage.
//   FB_MASK  SearchByProjection: skip_off (K + 1) and M = skip_off[K] mask bytes, one per feature of every keyframe of the call.
//   FB_PAIR  SearchBySim3: no normals, and pose holds SSM_JOB_FLOATS per JOB (K4, the source pose, the transform), packed by the stage.
//   FuseSim3Block FB_FLAT | FusePoseBlock FB_FLAT JOBS CHI2 | FuseSim3ResidentBlock - | FusePoseResidentBlock JOBS CHI2 | Sim3ProjectResidentBlock MASK | Sim3PairResidentBlock JOBS PAIR
// The descriptors lead, on 16 bytes, for the kernel's 16-byte loads; the inputs follow, then the outputs: the two counters go up as zeros (the kernel adds to them) and
// lead the download, the table follows, uv is declared with no elements when the caller does not ask for it.
enum : unsigned { FB_FLAT = 1, FB_JOBS = 2, FB_CHI2 = 4, FB_MASK = 8, FB_PAIR = 16 };
struct FuseShape { unsigned form; size_t K, F, P, L, J, T, N, M; bool want_uv; };
struct FuseBlock : StagedBlock {
  const FuseShape s;
  const bool flat, jobs;
  const size_t C, W;   // counters, table words
  explicit FuseBlock(const FuseShape& s) : s(s), flat(s.form & FB_FLAT), jobs(s.form & FB_JOBS), C(jobs ? s.J : s.K), W(jobs ? s.N : s.K * s.P) {}
  StagedSeg<uint8_t> kdesc = add<uint8_t>(flat ? 32 * s.F : 0, SB_COPY, 16), pdesc = add<uint8_t>(32 * s.P, SB_COPY, 16);
  StagedSeg<int32_t> job = add<int32_t>(jobs ? FPM_JOB_INTS * s.J : 0, SB_GEN, 16), tile = add<int32_t>(jobs ? 2 * s.T : 0, SB_GEN);
  StagedSeg<int32_t> slot = add<int32_t>(flat ? 0 : s.K, SB_GEN), skip_off = add<int32_t>(s.form & FB_MASK ? s.K + 1 : 0, SB_COPY);
  StagedSeg<float> rec = add<float>(flat ? FSM_REC_FLOATS * s.K : 0, SB_COPY);
  StagedSeg<float> pose = add<float>(s.form & FB_PAIR ? SSM_JOB_FLOATS * s.J : FSM_POSE_FLOATS * s.K, jobs && !(s.form & FB_PAIR) ? SB_COPY : SB_GEN);
  StagedSeg<int32_t> feat_off = add<int32_t>(flat ? s.K + 1 : 0, SB_COPY), cell_off = add<int32_t>(flat ? s.K * (FSM_CELLS + 1) : 0, SB_COPY);
  StagedSeg<float> kxy = add<float>(flat ? 2 * s.F : 0, SB_COPY);
  StagedSeg<uint16_t> cell_idx = add<uint16_t>(flat ? s.F : 0, SB_GEN);
  StagedSeg<uint8_t> koct = add<uint8_t>(flat ? s.F : 0, SB_COPY);
  StagedSeg<float> scale_factors = add<float>(s.L, SB_COPY), inv_sigma2 = add<float>(s.form & FB_CHI2 ? s.L : 0, SB_COPY);
  StagedSeg<float> pos = add<float>(3 * s.P, SB_COPY), normal = add<float>(s.form & FB_PAIR ? 0 : 3 * s.P, SB_COPY), dmin = add<float>(s.P, SB_COPY), dmax = add<float>(s.P, SB_COPY);
  StagedSeg<uint8_t> skip = add<uint8_t>(s.form & FB_MASK ? s.M : 0, SB_COPY);
  StagedSeg<int32_t> n_valid = add<int32_t>(C, SB_OUT | SB_ZERO), n_hit = add<int32_t>(C, SB_OUT | SB_ZERO);
  StagedSeg<uint32_t> table = add<uint32_t>(W, SB_OUT);
  StagedSeg<float> uv = add<float>(s.want_uv ? 2 * W : 0, SB_OUT);
};
// the six entry points' names for it
struct FuseSim3Block : FuseBlock {
  FuseSim3Block(size_t K, size_t F, size_t P, size_t L, bool want_uv) : FuseBlock({FB_FLAT, K, F, P, L, 0, 0, 0, 0, want_uv}) {}
};
struct FusePoseBlock : FuseBlock {
  FusePoseBlock(size_t K, size_t F, size_t P, size_t L, size_t J, size_t T, size_t N, bool want_uv) : FuseBlock({FB_FLAT | FB_JOBS | FB_CHI2, K, F, P, L, J, T, N, 0, want_uv}) {}
};
struct FuseSim3ResidentBlock : FuseBlock {
  FuseSim3ResidentBlock(size_t K, size_t P, size_t L, bool want_uv) : FuseBlock({0, K, 0, P, L, 0, 0, 0, 0, want_uv}) {}
};
struct FusePoseResidentBlock : FuseBlock {
  FusePoseResidentBlock(size_t K, size_t P, size_t L, size_t J, size_t T, size_t N, bool want_uv) : FuseBlock({FB_JOBS | FB_CHI2, K, 0, P, L, J, T, N, 0, want_uv}) {}
};
struct Sim3ProjectResidentBlock : FuseBlock {
  Sim3ProjectResidentBlock(size_t K, size_t P, size_t L, size_t M, bool want_uv) : FuseBlock({FB_MASK, K, 0, P, L, 0, 0, 0, M, want_uv}) {}
};
struct Sim3PairResidentBlock : FuseBlock {
  Sim3PairResidentBlock(size_t K, size_t P, size_t L, size_t J, size_t T, size_t N, bool want_uv) : FuseBlock({FB_JOBS | FB_PAIR, K, 0, P, L, J, T, N, 0, want_uv}) {}
};

// The tracked frame's and LocalMapping's own entry points (hamming.hip, frame.hip).  Every descriptor segment stands on 16 bytes: the kernels read descriptors as uint4.
// ccm_frame_window_search and ccm_distinctive_descriptors are not here: measured on a block they were slower than their hand-packed forms.

// ccm_hamming_dense_best2: the two descriptor sets lead, the per-split partial results (3 n_split Q ints) stay on the device, the three outputs follow.
struct HammingDenseBlock : StagedBlock {
  const size_t Q, T, n_split;
  HammingDenseBlock(size_t Q, size_t T, size_t n_split) : Q(Q), T(T), n_split(n_split) {}
  StagedSeg<uint8_t> q = add<uint8_t>(32 * Q, SB_COPY, 16), t = add<uint8_t>(32 * T, SB_COPY, 16);
  StagedSeg<int32_t> part = add<int32_t>(3 * n_split * Q, SB_WORK);
  StagedSeg<int32_t> best_idx = add<int32_t>(Q, SB_OUT), best_dist = add<int32_t>(Q, SB_OUT), second_dist = add<int32_t>(Q, SB_OUT);
};

// ccm_hamming_csr and ccm_hamming_csr_multi: the descriptors lead, the lists follow; q_tbase (the first target row of each query's search, written by the stage) has
// no elements in the single-search call.  The 16-bit distances lead the outputs, so an odd n_cand leaves half a word of pad in front of the best / second triple.
// An output the caller does not ask for is declared with no elements, and the kernel then receives nullptr for it.
struct HammingCsrBlock : StagedBlock {
  const size_t Q, T, n_cand; const bool multi, want_dist, want_best;
  HammingCsrBlock(size_t Q, size_t T, size_t n_cand, bool multi, bool want_dist, bool want_best) : Q(Q), T(T), n_cand(n_cand), multi(multi), want_dist(want_dist), want_best(want_best) {}
  StagedSeg<uint8_t> q = add<uint8_t>(32 * Q, SB_COPY, 16), t = add<uint8_t>(32 * T, SB_COPY, 16);
  StagedSeg<int32_t> cand_off = add<int32_t>(Q + 1, SB_COPY), q_tbase = add<int32_t>(multi ? Q : 0, SB_GEN), cand_idx = add<int32_t>(n_cand, SB_COPY);
  StagedSeg<uint16_t> cand_dist = add<uint16_t>(want_dist ? n_cand : 0, SB_OUT);
  StagedSeg<int32_t> best_idx = add<int32_t>(want_best ? Q : 0, SB_OUT), best_dist = add<int32_t>(want_best ? Q : 0, SB_OUT), second_dist = add<int32_t>(want_best ? Q : 0, SB_OUT);
};

// ccm_bow_transform: N descriptors up; the leaf and the node at the asked level come back.  The tree is the vocabulary handle's own.
struct BowTransformBlock : StagedBlock {
  const size_t N;
  explicit BowTransformBlock(size_t N) : N(N) {}
  StagedSeg<uint8_t> desc = add<uint8_t>(32 * N, SB_COPY, 16);
  StagedSeg<int32_t> leaf = add<int32_t>(N, SB_OUT), nid = add<int32_t>(N, SB_OUT);
};

// ccm_frame_frustum: n map points; the byte flags come last, so that every float segment stays on a word.
struct FrustumBlock : StagedBlock {
  const size_t n;
  explicit FrustumBlock(size_t n) : n(n) {}
  StagedSeg<float> P = add<float>(3 * n, SB_COPY), normal = add<float>(3 * n, SB_COPY), dmin = add<float>(n, SB_COPY), dmax = add<float>(n, SB_COPY);
  StagedSeg<float> u = add<float>(n, SB_OUT), v = add<float>(n, SB_OUT), cos = add<float>(n, SB_OUT);
  StagedSeg<int32_t> level = add<int32_t>(n, SB_OUT);
  StagedSeg<uint8_t> in_view = add<uint8_t>(n, SB_OUT);
};

// ccm_frame_guided_search: P map points against the resident grid of one frame.  The descriptors lead, on 16 bytes, for the window kernel's uint4
// reads; skip is the caller's or, without one, zeros, written by the stage.  The gate kernel leaves each point's window (radius, level range) on the device for the
// window kernels, which read u and v from the outputs; cnt is the count pass's.  The candidate arrays have the caller's capacity and come last, the 16-bit one at the end.
struct GuidedSearchBlock : StagedBlock {
  const size_t P, cap;
  GuidedSearchBlock(size_t P, size_t cap) : P(P), cap(cap) {}
  StagedSeg<uint8_t> desc = add<uint8_t>(32 * P, SB_COPY, 16);
  StagedSeg<float> pos = add<float>(3 * P, SB_COPY), dmin = add<float>(P, SB_COPY), dmax = add<float>(P, SB_COPY);
  StagedSeg<uint8_t> skip = add<uint8_t>(P, SB_GEN);
  StagedSeg<float> radius = add<float>(P, SB_WORK);
  StagedSeg<int32_t> minl = add<int32_t>(P, SB_WORK), maxl = add<int32_t>(P, SB_WORK), cnt = add<int32_t>(P, SB_WORK);
  StagedSeg<float> u = add<float>(P, SB_OUT), v = add<float>(P, SB_OUT);
  StagedSeg<int32_t> level = add<int32_t>(P, SB_OUT), cand_off = add<int32_t>(P + 1, SB_OUT);
  StagedSeg<uint8_t> status = add<uint8_t>(P, SB_OUT);
  StagedSeg<int32_t> cand_idx = add<int32_t>(cap, SB_OUT);
  StagedSeg<uint16_t> cand_dist = add<uint16_t>(cap, SB_OUT);
};

// ccm_update_normal_and_depth: the inputs, then the outputs, which go up seeded with the caller's values: a point without observers keeps them.
struct NormalDepthBlock : StagedBlock {
  const size_t P, K, L, NO;
  NormalDepthBlock(size_t P, size_t K, size_t L, size_t NO) : P(P), K(K), L(L), NO(NO) {}
  StagedSeg<float> pos = add<float>(3 * P, SB_COPY), kf_center = add<float>(3 * K, SB_COPY), scale_factors = add<float>(L, SB_COPY);
  StagedSeg<int32_t> obs_off = add<int32_t>(P + 1, SB_COPY), obs_kf = add<int32_t>(NO, SB_COPY), ref_kf = add<int32_t>(P, SB_COPY), ref_level = add<int32_t>(P, SB_COPY);
  StagedSeg<float> normal = add<float>(3 * P, SB_OUT | SB_COPY), dmin = add<float>(P, SB_OUT | SB_COPY), dmax = add<float>(P, SB_OUT | SB_COPY);
};

// ccm_mappoint_refresh_resident: P points with M observations in all on K keys.  The stage writes, while it validates, the absolute feature row in the
// store of every observation (slot * stride + feat) and of every point's reference feature (-1: no normal / depth part), so the kernel does no slot arithmetic and the
// slots themselves do not travel, and the points sorted into the kernel's size classes (order).  obs_kf / ref_kf index the centres.  Without a point that asks for the
// normal / depth part (nd false) the centres, positions and the three seeded outputs are declared with no elements.  The seeded outputs lead the download (they are
// uploaded too); best_desc stands on 16 bytes from the download's start and has no elements when the caller does not ask for it.
struct MapPointRefreshBlock : StagedBlock {
  const size_t K, P, M, L; const bool nd, want_desc;
  MapPointRefreshBlock(size_t K, size_t P, size_t M, size_t L, bool nd, bool want_desc) : K(K), P(P), M(M), L(L), nd(nd), want_desc(want_desc) {}
  StagedSeg<float> kf_center = add<float>(nd ? 3 * K : 0, SB_COPY);
  StagedSeg<int32_t> obs_off = add<int32_t>(P + 1, SB_COPY), obs_row = add<int32_t>(M, SB_GEN), obs_kf = add<int32_t>(nd ? M : 0, SB_COPY);
  StagedSeg<float> pos = add<float>(nd ? 3 * P : 0, SB_COPY);
  StagedSeg<int32_t> ref_row = add<int32_t>(P, SB_GEN), ref_kf = add<int32_t>(nd ? P : 0, SB_COPY);
  StagedSeg<float> scale_factors = add<float>(L, SB_COPY);
  StagedSeg<int32_t> order = add<int32_t>(P, SB_GEN);
  StagedSeg<float> normal = add<float>(nd ? 3 * P : 0, SB_OUT | SB_COPY, 16), dmin = add<float>(nd ? P : 0, SB_OUT | SB_COPY), dmax = add<float>(nd ? P : 0, SB_OUT | SB_COPY);
  StagedSeg<int32_t> best_obs = add<int32_t>(P, SB_OUT);
  StagedSeg<uint8_t> status = add<uint8_t>(P, SB_OUT);
  StagedSeg<uint8_t> best_desc = add<uint8_t>(want_desc ? 32 * P : 0, SB_OUT, 16);
};
