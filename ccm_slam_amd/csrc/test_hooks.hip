// test_hooks.hip — TEST-ONLY entry points, built into libccm_testhooks.so (NOT into the product library libccm_hip.so, which it links against).
// They reach into handles through the internal headers; nothing in the product's timed paths knows about them.
#include "common.h"
#include "ba_types.h"
#include "test_internal.h"
#include "lane_xor.h"
#include "kfstore.h"
#include "../../include/ccm_testhooks.h"
#include <cstring>
#include <string>

// Copies one of the structure arrays that ccm_ba_create built on the device (ba_build.hip) to the host.  *bytes receives the size of the array;
// with out == nullptr only the size is returned.  tests/test_ba_structure_gpu.py recomputes every array with numpy and compares.
extern "C" int ccm_ba_debug_array(ccm_ba* ba, const char* name, void* out, size_t cap_bytes, size_t* bytes) {
  if (!ba || !name || !bytes) return CCM_E_ARG;
  ccm_ctx* ctx = ba->ctx;
  const BaDev& d = ba->d;
  const std::string n(name);
  const void* src = nullptr;
  size_t sz = 0;
  const size_t Cp = (size_t)d.Cp, L = (size_t)d.Lloc, E = (size_t)d.Eloc, nOff = (size_t)d.nOff, ent = (size_t)ba->n_row_entries, I = (size_t)ba->n_inst;
  const size_t n_cl = (Cp + kClu - 1) / kClu;
  auto host_int = [&](const int* p, size_t idx, int* v) -> int {
    CCM_HIP_CHECK(ctx, hipMemcpy(v, p + idx, sizeof(int), hipMemcpyDeviceToHost));
    return CCM_OK;
  };
  int tail = 0;
#define ARR(nm, ptr, count, T) if (n == nm) { src = (ptr); sz = (size_t)(count) * sizeof(T); }
  ARR("slot_cam", d.slot_cam, Cp, int) ARR("slot_pt", ba->d_slot_pt, ba->Lp, int) ARR("loc_edge_orig", ba->d_loc_edge_orig, E, int)
  ARR("pt_off", d.pt_off, L + 1, int) ARR("ed_cam", d.ed_cam, E, int) ARR("ed_cslot", d.ed_cslot, E, int) ARR("ed_pt", d.ed_pt, E, int)
  ARR("obs", d.obs, 2 * E, double) ARR("info", d.info, E, double)
  ARR("cam_off", d.cam_off, Cp + 1, int) ARR("rowblk_off", d.rowblk_off, Cp + 1, int) ARR("row_off", d.row_off, Cp + 1, int)
  ARR("row_col", d.row_col, ent, int) ARR("row_blk", d.row_blk, ent, uint32_t)
  ARR("inst_off", d.inst_off, nOff + 1, int) ARR("inst_a", d.inst_a, I, int) ARR("inst_c", d.inst_c, I, int) ARR("inst_al", d.inst_al, I, int)
  ARR("blk_i", ba->d_blk_i, Cp + nOff, int) ARR("blk_j", ba->d_blk_j, Cp + nOff, int)
  ARR("chunk_off", d.chunk_off, d.chunk_off ? d.n_chunk + 1 : 0, int)
  ARR("pers_uoff", ba->d_pers_uoff, ba->d_pers_uoff ? 2 * n_cl + 1 : 0, int) ARR("pers_loc", ba->d_pers_loc, ba->d_pers_loc ? ent : 0, int)
  ARR("pers_coff", ba->d_pers_coff, ba->d_pers_coff ? n_cl + 1 : 0, int)
  // the last trial's PCG flags ([1] iterations, [2] numeric failure, [3] the persistent launch gave up) and the persistent kernel's four abort words (clear between trials)
  ARR("pcg_flag", d.pcg_flag, 4, int) ARR("pers_flags", ba->d_pers_bar, ba->d_pers_bar ? 4 : 0, unsigned)
  ARR("row_unit_off", d.row_unit_off, d.row_unit_off ? Cp + 1 : 0, int) ARR("blk_unit0", d.blk_unit0, d.blk_unit0 ? nOff + 1 : 0, int)
#undef ARR
  if (n == "cam_edge" || n == "cam_pt") {
    if (int rc = host_int(d.cam_off, Cp, &tail)) return rc;
    src = n == "cam_edge" ? d.cam_edge : d.cam_pt; sz = (size_t)tail * sizeof(int);
  } else if (n == "cam_oi") {
    if (int rc = host_int(d.cam_off, Cp, &tail)) return rc;
    src = d.cam_oi; sz = 4 * (size_t)tail * sizeof(double);
  } else if (n == "pers_ucol") {
    if (ba->d_pers_uoff) { if (int rc = host_int(ba->d_pers_uoff, 2 * n_cl, &tail)) return rc; }
    src = ba->d_pers_ucol; sz = (size_t)tail * sizeof(int);
  } else if (n == "pers_cij" || n == "pers_cblk") {
    if (ba->d_pers_coff) { if (int rc = host_int(ba->d_pers_coff, n_cl, &tail)) return rc; }
    src = n == "pers_cij" ? (const void*)ba->d_pers_cij : (const void*)ba->d_pers_cblk; sz = (size_t)tail * sizeof(int);
  } else if (n == "unit_tab") {
    if (d.row_unit_off) { if (int rc = host_int(d.row_unit_off, Cp, &tail)) return rc; }
    src = d.unit_tab; sz = (size_t)tail * sizeof(int4);
  } else if (n == "cb_off" || n == "cb_ab") {
    src = n == "cb_off" ? ba->d_cb_off : ba->d_cb_ab;
    sz = ba->coarse_na ? (n == "cb_off" ? (size_t)ba->coarse_ncb + 1 : 2 * (size_t)ba->coarse_ncb) * sizeof(int) : 0;
  } else if (n == "cb_ent") {
    src = ba->d_cb_ent; sz = ba->coarse_na ? (Cp + nOff) * sizeof(int) : 0;
  } else if (n == "sizes") {   // Cp, Lp, Lloc, Eloc, nOff, max_cam_edges, row_units_max, pers_grid, coarse_na, coarse_ncb, n_chunk, lp_begin
    const int v[12] = {d.Cp, ba->Lp, d.Lloc, d.Eloc, d.nOff, d.max_cam_edges, d.row_units_max, ba->pers_grid, ba->coarse_na, ba->coarse_ncb, d.n_chunk, ba->lp_begin};
    *bytes = sizeof(v);
    if (out) { if (cap_bytes < sizeof(v)) return CCM_E_ARG; std::memcpy(out, v, sizeof(v)); }
    return CCM_OK;
  } else if (!src && sz == 0 && n != "chunk_off" && n != "cam_oi" && n.rfind("pers_", 0) != 0 && n != "row_unit_off" && n != "blk_unit0") {
    bool known = false;
    for (const char* k : {"slot_cam", "slot_pt", "loc_edge_orig", "pt_off", "ed_cam", "ed_cslot", "ed_pt", "obs", "info", "cam_off", "rowblk_off", "row_off", "row_col", "row_blk",
                          "inst_off", "inst_a", "inst_c", "inst_al", "blk_i", "blk_j"}) known = known || n == k;
    if (!known) return ccm_set_error(ctx, CCM_E_ARG, "ccm_ba_debug_array: unknown array " + n);
  }
  *bytes = sz;
  if (!out || !sz) return CCM_OK;
  if (cap_bytes < sz || !src) return CCM_E_ARG;
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(out, src, sz, hipMemcpyDeviceToHost));
  return CCM_OK;
}

// ---- C wrappers of the C++-linkage test entry points that live next to the file-local kernels they exercise (test_internal.h) ----
extern "C" int ccm_ba_debug_partial_reduced(ccm_ba* ba, double lambda, double* out, size_t cap, size_t* count) { return ccm_internal::ba_debug_partial_reduced(ba, lambda, out, cap, count); }
extern "C" int ccm_ba_debug_coarse(ccm_ba* ba, double lambda, int* na, double* Ac, double* Ainv, double* Pm, size_t cap) { return ccm_internal::ba_debug_coarse(ba, lambda, na, Ac, Ainv, Pm, cap); }
extern "C" int ccm_ba_debug_pcg_solve(ccm_ba* ba, double lambda, int coarse, double rel_tol, int max_it, double* x_out, size_t cap, int* flags) {
  return ccm_internal::ba_debug_pcg_solve(ba, lambda, coarse, rel_tol, max_it, x_out, cap, flags);
}
extern "C" int ccm_comm_loopback_create(int nranks, void** group) { return ccm_internal::comm_loopback_create(nranks, group); }
extern "C" void ccm_comm_loopback_destroy(void* group) { ccm_internal::comm_loopback_destroy(group); }
extern "C" int ccm_comm_init_loopback(ccm_ctx* ctx, void* group, int rank) { return ccm_internal::comm_init_loopback(ctx, group, rank); }
extern "C" int ccm_debug_dense_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info) { return ccm_internal::debug_dense_solve(ctx, A, b, n, x, info); }
extern "C" int ccm_debug_planned_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info) { return ccm_internal::debug_planned_solve(ctx, A, b, n, x, info); }
extern "C" int ccm_debug_tile_solve(ccm_ctx* ctx, const double* A, const double* b, int n, double* x, int* info, int* levels, int* tiles) { return ccm_internal::debug_tile_solve(ctx, A, b, n, x, info, levels, tiles); }
extern "C" int ccm_debug_dense_inverse(ccm_ctx* ctx, const double* A, int n, double* Ainv, int* info) { return ccm_internal::debug_dense_inverse(ctx, A, n, Ainv, info); }
extern "C" int ccm_debug_pg_solve(ccm_ctx* ctx, int n_vert, const double* sim3, const uint8_t* fixed, int fix_scale, int n_edge, const int32_t* e_i, const int32_t* e_j,
                                  const double* meas, double lambda, int solver, double rel_tol, int max_it, const double* r_in, ccm_pg_debug_out* out) {
  return ccm_internal::pg_debug_solve(ctx, n_vert, sim3, fixed, fix_scale, n_edge, e_i, e_j, meas, lambda, solver, rel_tol, max_it, r_in, out);
}
extern "C" int ccm_debug_poseopt_linearise(ccm_ctx* ctx, const double cam_qt[7], int n, const double* Xw, const double* obs, const double* info, const double K[4],
                                           const uint8_t* level, const uint8_t* robust, double* acc_out, double* err_out, int shape[3]) {
  return ccm_internal::poseopt_debug_linearise(ctx, cam_qt, n, Xw, obs, info, K, level, robust, acc_out, err_out, shape);
}
extern "C" int ccm_debug_sim3opt_linearise(ccm_ctx* ctx, const double sim3[8], int n, const double* P1c, const double* P2c, const double* obs1, const double* obs2,
                                           const double* info1, const double* info2, const double K1[4], const double K2[4], double th2, int fix_scale,
                                           const uint8_t* alive, double* acc_out, double* chi2_out, double* err_out, double* pert_out, double* J_out, int shape[2]) {
  return ccm_internal::sim3opt_debug_linearise(ctx, sim3, n, P1c, P2c, obs1, obs2, info1, info2, K1, K2, th2, fix_scale, alive, acc_out, chi2_out, err_out, pert_out, J_out, shape);
}
extern "C" int ccm_orb_debug_timing(const ccm_orb* o, double out_ms[6]) { return ccm_internal::orb_debug_timing(o, out_ms); }
extern "C" int ccm_orb_debug_level(ccm_orb* o, int level, uint8_t* score_out, uint8_t* blur_out) { return ccm_internal::orb_debug_level(o, level, score_out, blur_out); }
extern "C" int ccm_orb_debug_candidates(ccm_orb* o, int level, ccm_keypoint* out, int cap, int* n_out) { return ccm_internal::orb_debug_candidates(o, level, out, cap, n_out); }
extern "C" int ccm_orb_debug_octree_dev(ccm_ctx* ctx, const int32_t* x, const int32_t* y, const int32_t* response, int n, int W, int H, int N, int32_t* sel_out, int cap, int* n_out, int* overflow) {
  return ccm_internal::orb_debug_octree_dev(ctx, x, y, response, n, W, H, N, sel_out, cap, n_out, overflow);
}
// ccm_covis_update with a histogram window of 64 keyframe indices instead of the product's: the multi-window path at a small n_all (tests/test_covis_gpu.py)
extern "C" int ccm_debug_covis_update_small(ccm_ctx* ctx, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_skip,
                                            int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col, int32_t* count,
                                            int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags, int32_t* needed) {
  return ccm_internal::covis_update_window(ctx, 1, n_kf, n_all, order_key, list_off, list_pt, list_skip, n_pt, obs_off, obs_kf, th, cap, row_off, col, count, fw_off, fw_col,
                                           fw_w, ord_off, ord_kf, ord_w, flags, needed);
}

// lane_xor.h against __shfl_xor: out[6][3][64] doubles — for MASK = 1, 2, 4, 8, 16, 32: from_partner<MASK>(v), add_partner<MASK>(v) and __shfl_xor(v, MASK) of the 64 lanes'
// values in[64]; sum_out[0] = lanex::wave_sum, sum_out[1] = the __shfl_xor butterfly 32 ... 1, sum_out[2] = lanex::wave_incl_scan_i32 of the pattern (37 lane mod 101) - 20.  tests/test_lane_xor_gpu.py.
namespace {
template <int MASK>
__device__ void lane_xor_case(const double v, double* out, int slot) {
  const int lane = threadIdx.x;
  out[(3 * slot + 0) * 64 + lane] = lanex::from_partner<MASK>(v);
  out[(3 * slot + 1) * 64 + lane] = lanex::add_partner<MASK>(v);
  out[(3 * slot + 2) * 64 + lane] = __shfl_xor(v, MASK, 64);
}
__global__ __launch_bounds__(64) void lane_xor_probe(const double* in, double* out, double* sum_out) {
  const double v = in[threadIdx.x];
  lane_xor_case<1>(v, out, 0); lane_xor_case<2>(v, out, 1); lane_xor_case<4>(v, out, 2);
  lane_xor_case<8>(v, out, 3); lane_xor_case<16>(v, out, 4); lane_xor_case<32>(v, out, 5);
  double a = lanex::wave_sum(v), b = v;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) b += __shfl_xor(b, off, 64);
  sum_out[threadIdx.x] = a; sum_out[64 + threadIdx.x] = b;
  sum_out[128 + threadIdx.x] = (double)lanex::wave_incl_scan_i32((int)(threadIdx.x * 37 % 101) - 20);   // (integer scan of a fixed pattern)
}
}  // namespace
extern "C" int ccm_debug_lane_xor(ccm_ctx* ctx, const double* in64, double* out_6x3x64, double* sums_2x64 /* [3][64]: wave sums by lane_xor.h, by __shfl_xor, inclusive integer scan */) {
  if (!ctx || !in64 || !out_6x3x64 || !sums_2x64) return CCM_E_ARG;
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double* d = nullptr;
  CCM_HIP_CHECK(ctx, hipMalloc(&d, (64 + 6 * 3 * 64 + 192) * sizeof(double)));
  CCM_HIP_CHECK(ctx, hipMemcpy(d, in64, 64 * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lane_xor_probe, dim3(1), dim3(64), 0, ctx->stream, d, d + 64, d + 64 + 6 * 3 * 64);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(out_6x3x64, d + 64, 6 * 3 * 64 * sizeof(double), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipMemcpy(sums_2x64, d + 64 + 6 * 3 * 64, 192 * sizeof(double), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipFree(d));
  return CCM_OK;
}

// block_red.h as the LM kernels use it: ONE BlockRedT<4> object in one workgroup of 256 threads, its LDS laid out as in poseopt_kernel<true> ([2 * 4 * 64 | kTrDoubles]
// doubles), and in a single launch the sequence  sum1, sum28_lds, sum28_lds, sum1, sum27, sum27, sum64<35>, sum64<35>, sum1  — the ping-pong phase and the transpose block
// are reused back to back as in a kernel.  Call c reads slot s of thread t from in[in_off(c) + s * 256 + t] (1 / 32 / 64 slots) and writes EVERY thread's result k to
// out[out_off(c) + k * 256 + t] (1 / 28 / 28 / 35 results).  tests/test_block_red_gpu.py.
#include "block_red.h"
namespace {
constexpr int kProbeT = blockred::kThreads;
__global__ __launch_bounds__(kProbeT) void block_red_probe(const double* in, double* out) {
  using Red = blockred::BlockRedT<4>;
  __shared__ __attribute__((aligned(16))) double sm[2 * 4 * 64 + Red::kTrDoubles];
  double* const tr = sm + 2 * 4 * 64;
  const int t = threadIdx.x;
  Red red{sm, 0, t & 63, t >> 6};
  auto one = [&]() { const double s = red.sum1(in[t]); in += kProbeT; out[t] = s; out += kProbeT; };
  auto wide = [&](int which) {   // 0: sum28_lds, 1: sum27
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; k++) acc[k] = in[k * kProbeT + t];
    in += 32 * kProbeT;
    if (which == 0) red.sum28_lds(acc, tr); else red.sum27(acc);
#pragma unroll
    for (int k = 0; k < 28; k++) out[k * kProbeT + t] = acc[k];
    out += 28 * kProbeT;
  };
  auto wide64 = [&]() {
    double acc[64];
#pragma unroll
    for (int k = 0; k < 64; k++) acc[k] = in[k * kProbeT + t];
    in += 64 * kProbeT;
    red.sum64<35>(acc);
#pragma unroll
    for (int k = 0; k < 35; k++) out[k * kProbeT + t] = acc[k];
    out += 35 * kProbeT;
  };
  one(); wide(0); wide(0); one(); wide(1); wide(1); wide64(); wide64(); one();
}
constexpr int kProbeIn = (3 * 1 + 4 * 32 + 2 * 64) * kProbeT, kProbeOut = (3 * 1 + 4 * 28 + 2 * 35) * kProbeT;

// lanex::from_partner_c with `off` an unrolled loop constant (as sum27 / sum64 call it) and lanex::wave_min_u32, all 64 lanes
__global__ __launch_bounds__(64) void lane_ops_probe(const double* in, const uint32_t* key, double* partner, uint32_t* kmin) {
  const double v = in[threadIdx.x];
  int slot = 0;
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) partner[64 * slot++ + threadIdx.x] = lanex::from_partner_c(v, off);
  kmin[threadIdx.x] = lanex::wave_min_u32(key[threadIdx.x]);
}
}  // namespace
extern "C" int ccm_debug_block_red(ccm_ctx* ctx, const double* in, size_t n_in, double* out, size_t n_out) {
  if (!ctx || !in || !out || n_in != (size_t)kProbeIn || n_out != (size_t)kProbeOut) return CCM_E_ARG;
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double* d = nullptr;
  CCM_HIP_CHECK(ctx, hipMalloc(&d, (size_t)(kProbeIn + kProbeOut) * sizeof(double)));
  CCM_HIP_CHECK(ctx, hipMemcpy(d, in, (size_t)kProbeIn * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(block_red_probe, dim3(1), dim3(kProbeT), 0, ctx->stream, d, d + kProbeIn);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(out, d + kProbeIn, (size_t)kProbeOut * sizeof(double), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipFree(d));
  return CCM_OK;
}
extern "C" int ccm_debug_lane_ops(ccm_ctx* ctx, const double* in64, const uint32_t* key64, double* partner_6x64, uint32_t* min64) {
  if (!ctx || !in64 || !key64 || !partner_6x64 || !min64) return CCM_E_ARG;
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double* d = nullptr;   // in 64 | partner 6 * 64 | key 64 (u32) | min 64 (u32)
  CCM_HIP_CHECK(ctx, hipMalloc(&d, (64 + 6 * 64 + 64) * sizeof(double)));
  uint32_t* dk = reinterpret_cast<uint32_t*>(d + 64 + 6 * 64);
  CCM_HIP_CHECK(ctx, hipMemcpy(d, in64, 64 * sizeof(double), hipMemcpyHostToDevice));
  CCM_HIP_CHECK(ctx, hipMemcpy(dk, key64, 64 * sizeof(uint32_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lane_ops_probe, dim3(1), dim3(64), 0, ctx->stream, d, dk, d + 64, dk + 64);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(partner_6x64, d + 64, 6 * 64 * sizeof(double), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipMemcpy(min64, dk + 64, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipFree(d));
  return CCM_OK;
}

// tv_score of twoview_math.h on the device for GIVEN models (one lane per model; model 0: homographies, their inverses by tv_inv33 on the device; 1: fundamental
// matrices): plants a match whose chi2 sits on a threshold float.  tests/test_twoview_gpu.py compares with ccmh_twoview_score_host.
#include "twoview_math.h"
namespace {
__global__ __launch_bounds__(64) void twoview_score_probe(int model, int n_models, const float* M, int N, const float* xy1, const float* xy2, float sigma, float* score,
                                                          uint32_t* mask) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= n_models) return;
  float m[9], inv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 9; k++) m[k] = M[9 * (size_t)h + k];
  if (model == 0) tv_inv33(m, inv);
  score[h] = tv_score(model == 0, m, inv, N, xy1, xy2, sigma, mask + (size_t)h * ((N + 31) / 32));
}
}  // namespace
extern "C" int ccm_debug_twoview_score(ccm_ctx* ctx, int model, int n_models, const float* M, int N, const float* xy1, const float* xy2, float sigma, float* score,
                                       uint32_t* mask) {
  if (!ctx || model < 0 || model > 1 || n_models < 1 || N < 1 || !M || !xy1 || !xy2 || !score || !mask) return CCM_E_ARG;
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t words = ((size_t)N + 31) / 32, nM = 9 * (size_t)n_models, nxy = 2 * (size_t)N;
  float* d = nullptr;   // M, xy1, xy2, score, mask
  CCM_HIP_CHECK(ctx, hipMalloc(&d, (nM + 2 * nxy + n_models + words * n_models) * sizeof(float)));
  float *d_xy1 = d + nM, *d_xy2 = d_xy1 + nxy, *d_score = d_xy2 + nxy;
  uint32_t* d_mask = reinterpret_cast<uint32_t*>(d_score + n_models);
  CCM_HIP_CHECK(ctx, hipMemcpy(d, M, nM * sizeof(float), hipMemcpyHostToDevice));
  CCM_HIP_CHECK(ctx, hipMemcpy(d_xy1, xy1, nxy * sizeof(float), hipMemcpyHostToDevice));
  CCM_HIP_CHECK(ctx, hipMemcpy(d_xy2, xy2, nxy * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(twoview_score_probe, dim3((unsigned)((n_models + 63) / 64)), dim3(64), 0, ctx->stream, model, n_models, d, N, d_xy1, d_xy2, sigma, d_score, d_mask);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(score, d_score, n_models * sizeof(float), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipMemcpy(mask, d_mask, words * n_models * sizeof(uint32_t), hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipFree(d));
  return CCM_OK;
}

// A live key's feature vector as its slot of the keyframe store holds it (ccm_kfstore_set_featvec, ccm_kfstore_ingest): nn, node[nn], off[nn + 1], idx[off[nn]]
// (room for n + 1, n + 1 and n entries, n the key's feature count).  nn = -1: the key has no vector.  tests/test_kfingest_gpu.py.
extern "C" int ccm_kfstore_debug_get_featvec(ccm_kfstore* st, ccm_ctx* ctx, int64_t key, int* nn, int32_t* node, int32_t* off, int32_t* idx) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_debug_get_featvec")) return rc;
  if (!nn) return CCM_E_ARG;
  std::shared_lock<std::shared_mutex> lk(st->mu);
  auto it = st->live.find(key);
  if (it == st->live.end()) return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfstore_debug_get_featvec: key not in the store");
  const size_t s = (size_t)it->second, g0 = s * (size_t)st->stride;
  const int n = st->h_n[s], c = st->h_fv_nn[s];
  *nn = c;
  if (c <= 0 || !node || !off || !idx) return CCM_OK;
  if (c > n) return ccm_set_error(ctx, CCM_E_STATE, "ccm_kfstore_debug_get_featvec: more nodes than features");
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(node, st->d_fv_node + g0, (size_t)c * 4, hipMemcpyDeviceToHost));
  CCM_HIP_CHECK(ctx, hipMemcpy(off, st->d_fv_off + g0 + s, ((size_t)c + 1) * 4, hipMemcpyDeviceToHost));
  const int L = off[c];
  if (L < 0 || L > n) return ccm_set_error(ctx, CCM_E_STATE, "ccm_kfstore_debug_get_featvec: the slot's offsets are not a feature vector's");
  std::vector<uint16_t> h((size_t)L);
  if (L) CCM_HIP_CHECK(ctx, hipMemcpy(h.data(), st->d_fv_idx + g0, (size_t)L * 2, hipMemcpyDeviceToHost));
  for (int i = 0; i < L; i++) idx[i] = h[i];
  return CCM_OK;
}

// test_lie_ops.h on the device: one lane per item in workgroups of 256, item i reads in[48 i ...] and writes out[40 i ...]; `out` is copied to the device first (ba_spd6_inv
// must leave its output untouched on a false return).  tests/test_lie_math_gpu.py compares with tests/lie_reference.py.
#include "test_lie_ops.h"
namespace {
__global__ __launch_bounds__(256) void lie_eval_probe(int op, int n, const double* in, double* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  lie_eval(op, in + (size_t)kLieIn * i, out + (size_t)kLieOut * i);
}
}  // namespace
extern "C" int ccm_debug_lie_eval(ccm_ctx* ctx, int op, int n, const double* in, double* out) {
  if (!ctx || op < 0 || op >= LIE_N_OPS || n < 1 || n > (1 << 20) || !in || !out) return CCM_E_ARG;
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t n_in = (size_t)kLieIn * n, n_out = (size_t)kLieOut * n;
  struct Buf { double* p = nullptr; ~Buf() { if (p) (void)hipFree(p); } } buf;   // freed on every return, the early ones of CCM_HIP_CHECK included
  CCM_HIP_CHECK(ctx, hipMalloc(&buf.p, (n_in + n_out) * sizeof(double)));
  double* const d = buf.p;
  CCM_HIP_CHECK(ctx, hipMemcpy(d, in, n_in * sizeof(double), hipMemcpyHostToDevice));
  CCM_HIP_CHECK(ctx, hipMemcpy(d + n_in, out, n_out * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lie_eval_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, n, d, d + n_in);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpy(out, d + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost));
  return CCM_OK;
}
