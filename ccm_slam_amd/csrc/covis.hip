// covis.hip — the covisibility graph of a corrected map on the device: ccm_covis_update, KeyFrame::UpdateConnections (KeyFrame.cpp:629-711) over a set of
// keyframes in walk order with the AddConnection / UpdateBestCovisibles calls (:392-426) they make on each other.  The rules are covis_math.h.
//
// Layout: one workgroup of 256 lanes per keyframe of the set in every per-keyframe kernel.
//   count   lanes stride over the keyframe's list entries and walk each point's observers; a dense uint32 histogram over a window of kCvWindow keyframe
//           indices lives in LDS (atomicAdd on LDS; integer sums do not depend on arrival order), windows follow one another until n_all is covered.  Non-zero
//           counters are compacted 256 columns at a time in ascending column order: ballot + popcount inside a wave, four wave totals through LDS.  The kernel
//           runs twice: the first pass leaves the row sizes, a one-workgroup scan turns them into offsets, the second pass writes (column, count) and the
//           row's event facts (entries >= th, the fallback column).
//   pair    per entry (i, t) with t in the set, binary search of i in row t: an event of i that reaches t and that C_t lacks is an extra entry of t (counted,
//           then placed through a cursor: the order of arrival is sorted away below); an event of t that reaches i with another weight marks i CHANGED.
//   final   the final weight row = the count row with the weights that reached it, merged with the extras by rank (ascending column); the ordered list = a rank
//           sort of (weight, order_key) keys through LDS tiles of kCvTile keys: rank = number of larger keys, keys are distinct, rows of any length.
// Everything the call writes is bounded by the caller's capacity `cap` (entries per variable-size array): the scans leave the sizes needed in the header, and a
// stage whose size exceeds cap is skipped together with what follows it.
#include "common.h"
#include "covis_math.h"
#include "stage_blocks.h"
#include "test_internal.h"
#include <limits.h>

namespace {

constexpr int kCvBlock = 256;
constexpr int kCvWaves = kCvBlock / 64;
constexpr int kCvWindow = 16384;      // 64 KB of LDS: two workgroups per CU
constexpr int kCvWindowSmall = 64;    // test hook: several windows at a small n_all
constexpr int kCvTile = 1024;

struct CovisArgs {
  int n_kf, n_all, cap;
  uint32_t th;
  const int32_t *order_key, *list_off, *list_pt, *obs_off, *obs_kf;
  // work arrays [n_kf] (extra_off: n_kf + 1; extra_src / extra_w: cap)
  int32_t *row_size, *n_ge, *fb_col, *extra_cnt, *cursor, *chg, *extra_off, *extra_src, *extra_w;
  // output block
  int32_t *hdr, *flags, *row_off, *fw_off, *ord_off, *col, *count, *fw_col, *fw_w, *ord_kf, *ord_w;
};

__device__ inline int32_t cv_clamp(int64_t v) { return v > INT_MAX ? INT_MAX : (int32_t)v; }

template <int W, bool WRITE>
__global__ __launch_bounds__(kCvBlock) void covis_count_kernel(CovisArgs a) {
  __shared__ uint32_t hist[W];
  __shared__ uint32_t wave_tot[kCvWaves];
  __shared__ uint32_t red_c[kCvWaves];
  __shared__ int32_t red_key[kCvWaves], red_col[kCvWaves], red_nge[kCvWaves];
  if (WRITE && a.hdr[0] > a.cap) return;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t e0 = a.list_off[i], e1 = a.list_off[i + 1];
  const int32_t out0 = WRITE ? a.row_off[i] : 0;
  int32_t running = 0, nge = 0, best_col = -1, best_key = 0;
  uint32_t best_c = 0;
  for (int w0 = 0; w0 < a.n_all; w0 += W) {
    const int wn = a.n_all - w0 < W ? a.n_all - w0 : W;
    for (int k = tid; k < wn; k += kCvBlock) hist[k] = 0;
    __syncthreads();
    for (int32_t e = e0 + tid; e < e1; e += kCvBlock) {
      const int32_t p = a.list_pt[e];          // packed: null and skipped entries are both < 0
      if (!covis_entry_counts(p, 0)) continue;
      const int32_t o1 = a.obs_off[p + 1];
      for (int32_t o = a.obs_off[p]; o < o1; o++) {
        const int32_t j = a.obs_kf[o];
        if (covis_observer_counts(j, i) && (uint32_t)(j - w0) < (uint32_t)wn) atomicAdd(&hist[j - w0], 1u);
      }
    }
    __syncthreads();
    for (int c0 = 0; c0 < wn; c0 += kCvBlock) {
      const int k = c0 + tid;
      const uint32_t v = k < wn ? hist[k] : 0;
      const unsigned long long m = __ballot(v != 0);
      if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int q = 0; q < kCvWaves; q++) { const uint32_t t = wave_tot[q]; total += t; if (q < wave) before += t; }
      if (v != 0) {
        const int32_t c = w0 + k;
        if (WRITE) {
          const int32_t at = out0 + running + (int32_t)before + (int32_t)__popcll(m & ((1ull << lane) - 1));
          a.col[at] = c; a.count[at] = (int32_t)v;
          if (v >= a.th) nge++;
          const int32_t key = a.order_key[c];
          if (best_col < 0 || covis_fallback_better(v, key, best_c, best_key)) { best_c = v; best_key = key; best_col = c; }
        }
      }
      running += (int32_t)total;
      __syncthreads();
    }
  }
  if (!WRITE) {
    if (tid == 0) { a.row_size[i] = running; a.extra_cnt[i] = 0; a.cursor[i] = 0; a.chg[i] = 0; }
    return;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t oc = __shfl_xor(best_c, off, 64);
    const int32_t ok = __shfl_xor(best_key, off, 64), ocol = __shfl_xor(best_col, off, 64);
    nge += __shfl_xor(nge, off, 64);
    if (ocol >= 0 && (best_col < 0 || covis_fallback_better(oc, ok, best_c, best_key))) { best_c = oc; best_key = ok; best_col = ocol; }
  }
  if (lane == 0) { red_c[wave] = best_c; red_key[wave] = best_key; red_col[wave] = best_col; red_nge[wave] = nge; }
  __syncthreads();
  if (tid == 0) {
    nge = 0; best_col = -1; best_c = 0; best_key = 0;
    for (int q = 0; q < kCvWaves; q++) {
      nge += red_nge[q];
      if (red_col[q] >= 0 && (best_col < 0 || covis_fallback_better(red_c[q], red_key[q], best_c, best_key))) { best_c = red_c[q]; best_key = red_key[q]; best_col = red_col[q]; }
    }
    a.n_ge[i] = nge;
    a.fb_col[i] = nge > 0 ? -1 : best_col;
    a.flags[i] = running == 0 ? COVIS_EMPTY : nge == 0 ? COVIS_FALLBACK : 0;
  }
}

// exclusive scan of n sizes by one workgroup: off[0 .. n] (clamped to INT_MAX), returns the total; part: kCvBlock + 1 words of LDS
template <class F>
__device__ int64_t covis_scan(int n, F size_of, int32_t* off, int64_t* part) {
  const int tid = threadIdx.x;
  const int chunk = (n + kCvBlock - 1) / kCvBlock;
  const int b = tid * chunk < n ? tid * chunk : n, e = b + chunk < n ? b + chunk : n;
  int64_t s = 0;
  for (int k = b; k < e; k++) s += size_of(k);
  __syncthreads();
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < kCvBlock; t++) { const int64_t v = part[t]; part[t] = run; run += v; }
    part[kCvBlock] = run;
  }
  __syncthreads();
  int64_t run = part[tid];
  for (int k = b; k < e; k++) { off[k] = cv_clamp(run); run += size_of(k); }
  const int64_t total = part[kCvBlock];
  if (tid == 0) off[n] = cv_clamp(total);
  return total;
}

__global__ __launch_bounds__(kCvBlock) void covis_scan_rows_kernel(CovisArgs a) {
  __shared__ int64_t part[kCvBlock + 1];
  const int64_t total = covis_scan(a.n_kf, [&](int k) { return (int64_t)a.row_size[k]; }, a.row_off, part);
  if (threadIdx.x == 0) { a.hdr[0] = cv_clamp(total); a.hdr[1] = -1; a.hdr[2] = -1; a.hdr[3] = 0; }
}

__global__ __launch_bounds__(kCvBlock) void covis_scan_final_kernel(CovisArgs a) {
  __shared__ int64_t part[kCvBlock + 1];
  if (a.hdr[0] > a.cap) return;
  for (int k = threadIdx.x; k < a.n_kf; k += kCvBlock)
    if (a.chg[k] || a.extra_cnt[k] > 0) a.flags[k] |= COVIS_CHANGED;
  __syncthreads();
  covis_scan(a.n_kf, [&](int k) { return (int64_t)a.extra_cnt[k]; }, a.extra_off, part);
  const int64_t n_fw = covis_scan(a.n_kf, [&](int k) { return (int64_t)a.row_size[k] + a.extra_cnt[k]; }, a.fw_off, part);
  const int64_t n_ord = covis_scan(a.n_kf, [&](int k) {
    return (int64_t)covis_ord_size((a.flags[k] & COVIS_CHANGED) != 0, a.row_size[k] + a.extra_cnt[k], a.row_size[k], a.n_ge[k]); }, a.ord_off, part);
  if (threadIdx.x == 0) { a.hdr[1] = cv_clamp(n_fw); a.hdr[2] = cv_clamp(n_ord); }
}

// FILL = false: count the extras of every target and mark the rows whose ordered list is rebuilt; FILL = true: place the extras
template <bool FILL>
__global__ __launch_bounds__(kCvBlock) void covis_pair_kernel(CovisArgs a) {
  if (a.hdr[0] > a.cap) return;
  if (FILL && (a.hdr[1] > a.cap || a.hdr[2] > a.cap)) return;
  const int i = blockIdx.x;
  const int32_t r0 = a.row_off[i], L0 = a.row_size[i], nge = a.n_ge[i], fb = a.fb_col[i];
  for (int32_t e = threadIdx.x; e < L0; e += kCvBlock) {
    const int32_t t = a.col[r0 + e];
    if (t >= a.n_kf) continue;
    const uint32_t c = (uint32_t)a.count[r0 + e];
    const int32_t rt = a.row_off[t], Lt = a.row_size[t];
    const int32_t pos = covis_find(a.col, rt, rt + Lt, i);
    if (pos < 0 && covis_is_event(c, t, a.th, nge, fb) && covis_reaches(i, t, Lt == 0)) {
      if (FILL) {
        const int32_t slot = a.extra_off[t] + atomicAdd(&a.cursor[t], 1);
        a.extra_src[slot] = i; a.extra_w[slot] = (int32_t)c;
      } else {
        atomicAdd(&a.extra_cnt[t], 1);
      }
    }
    if (!FILL && pos >= 0 && covis_reaches(t, i, false)) {
      const uint32_t ct = (uint32_t)a.count[pos];
      if (ct != c && covis_is_event(ct, i, a.th, a.n_ge[t], a.fb_col[t])) atomicOr(&a.chg[i], 1);
    }
  }
}

__global__ __launch_bounds__(kCvBlock) void covis_final_kernel(CovisArgs a) {
  __shared__ uint64_t tile[kCvTile];
  if (a.hdr[0] > a.cap || a.hdr[1] > a.cap || a.hdr[2] > a.cap) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int32_t r0 = a.row_off[i], L0 = a.row_size[i], x0 = a.extra_off[i], X = a.extra_cnt[i], L = L0 + X, f0 = a.fw_off[i], o0 = a.ord_off[i];
  const bool changed = (a.flags[i] & COVIS_CHANGED) != 0;
  const int32_t nge = a.n_ge[i], fb = a.fb_col[i];
  // the final weights, ascending column: a row entry keeps its place plus the extras below it, an extra goes behind the row entries and extras below it
  for (int32_t e = tid; e < L; e += kCvBlock) {
    int32_t c, w, rank;
    if (e < L0) {
      c = a.col[r0 + e]; w = a.count[r0 + e]; rank = e;
      if (c < a.n_kf && covis_reaches(c, i, false)) {
        const int32_t rt = a.row_off[c];
        const int32_t pos = covis_find(a.col, rt, rt + a.row_size[c], i);
        if (pos >= 0 && covis_is_event((uint32_t)a.count[pos], i, a.th, a.n_ge[c], a.fb_col[c])) w = a.count[pos];
      }
    } else {
      c = a.extra_src[x0 + e - L0]; w = a.extra_w[x0 + e - L0];
      rank = covis_lower(a.col, r0, r0 + L0, c);
    }
    for (int32_t x = 0; x < X; x++) rank += a.extra_src[x0 + x] < c;
    a.fw_col[f0 + rank] = c; a.fw_w[f0 + rank] = w;
  }
  __syncthreads();
  // the ordered list: every final entry when the list was rebuilt by UpdateBestCovisibles, the row's own events otherwise
  for (int32_t c0 = 0; c0 < L; c0 += kCvBlock) {
    const int32_t e = c0 + tid;
    uint64_t mine = 0;
    int32_t c = 0, w = 0;
    if (e < L) {
      c = a.fw_col[f0 + e]; w = a.fw_w[f0 + e];
      if (changed || covis_is_event((uint32_t)w, c, a.th, nge, fb)) mine = covis_sort_key((uint32_t)w, a.order_key[c]);
    }
    int32_t rank = 0;
    for (int32_t t0 = 0; t0 < L; t0 += kCvTile) {
      const int32_t tn = L - t0 < kCvTile ? L - t0 : kCvTile;
      __syncthreads();
      for (int32_t k = tid; k < tn; k += kCvBlock) {
        const int32_t kc = a.fw_col[f0 + t0 + k], kw = a.fw_w[f0 + t0 + k];
        tile[k] = changed || covis_is_event((uint32_t)kw, kc, a.th, nge, fb) ? covis_sort_key((uint32_t)kw, a.order_key[kc]) : 0;
      }
      __syncthreads();
      if (mine)
        for (int32_t k = 0; k < tn; k++) rank += tile[k] > mine;
    }
    if (mine) { a.ord_kf[o0 + rank] = c; a.ord_w[o0 + rank] = w; }
  }
}

template <int W>
void covis_launch(ccm_ctx* ctx, const CovisArgs& a) {
  const dim3 grid((unsigned)a.n_kf), block(kCvBlock), one(1);
  hipLaunchKernelGGL((covis_count_kernel<W, false>), grid, block, 0, ctx->stream, a);
  hipLaunchKernelGGL(covis_scan_rows_kernel, one, block, 0, ctx->stream, a);
  hipLaunchKernelGGL((covis_count_kernel<W, true>), grid, block, 0, ctx->stream, a);
  hipLaunchKernelGGL(covis_pair_kernel<false>, grid, block, 0, ctx->stream, a);
  hipLaunchKernelGGL(covis_scan_final_kernel, one, block, 0, ctx->stream, a);
  hipLaunchKernelGGL(covis_pair_kernel<true>, grid, block, 0, ctx->stream, a);
  hipLaunchKernelGGL(covis_final_kernel, grid, block, 0, ctx->stream, a);
}

}  // namespace

namespace ccm_internal {
int covis_update_window(ccm_ctx* ctx, int small_window, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt,
                        const uint8_t* list_skip, int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col,
                        int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags,
                        int32_t* needed) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_covis_update: ";
  if (!row_off || !fw_off || !ord_off || !flags || !needed || (cap > 0 && (!col || !count || !fw_col || !fw_w || !ord_kf || !ord_w)))
    return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "bad args");
  if (const char* why = covis_check_args(n_kf, n_all, order_key, list_off, list_pt, list_skip, n_pt, obs_off, obs_kf, th, cap))
    return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  const size_t NL = (size_t)list_off[n_kf];
  CovisBlock b((size_t)n_kf, (size_t)n_all, (size_t)n_pt, NL, n_pt ? (size_t)obs_off[n_pt] : 0, (size_t)cap);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  b.put(b.order_key, order_key); b.put(b.list_off, list_off);
  int32_t* h_lpt = b.up(b.list_pt);
  for (size_t e = 0; e < NL; e++) h_lpt[e] = covis_entry_counts(list_pt[e], list_skip[e]) ? list_pt[e] : -1;
  if (n_pt) b.put(b.obs_off, obs_off);
  b.put(b.obs_kf, obs_kf);
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  CovisArgs a;
  a.n_kf = n_kf; a.n_all = n_all; a.cap = cap; a.th = (uint32_t)th;
  a.order_key = b.dev(b.order_key); a.list_off = b.dev(b.list_off); a.list_pt = b.dev(b.list_pt); a.obs_off = b.dev(b.obs_off); a.obs_kf = b.dev(b.obs_kf);
  a.row_size = b.dev(b.row_size); a.n_ge = b.dev(b.n_ge); a.fb_col = b.dev(b.fb_col); a.extra_cnt = b.dev(b.extra_cnt); a.cursor = b.dev(b.cursor);
  a.chg = b.dev(b.chg); a.extra_off = b.dev(b.extra_off); a.extra_src = b.dev(b.extra_src); a.extra_w = b.dev(b.extra_w);
  a.hdr = b.dev(b.hdr); a.flags = b.dev(b.flags); a.row_off = b.dev(b.row_off); a.fw_off = b.dev(b.fw_off); a.ord_off = b.dev(b.ord_off);
  a.col = b.dev(b.col); a.count = b.dev(b.count); a.fw_col = b.dev(b.fw_col); a.fw_w = b.dev(b.fw_w); a.ord_kf = b.dev(b.ord_kf); a.ord_w = b.dev(b.ord_w);
  if (small_window) covis_launch<kCvWindowSmall>(ctx, a); else covis_launch<kCvWindow>(ctx, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  b.get(b.hdr, needed, 3);
  if (needed[0] > cap || needed[1] > cap || needed[2] > cap) return CCM_OK;   // nothing else is defined: the caller comes back with a larger cap
  b.get(b.flags, flags); b.get(b.row_off, row_off); b.get(b.fw_off, fw_off); b.get(b.ord_off, ord_off);
  const size_t n0 = (size_t)needed[0], n1 = (size_t)needed[1], n2 = (size_t)needed[2];
  b.get(b.col, col, n0); b.get(b.count, count, n0);
  b.get(b.fw_col, fw_col, n1); b.get(b.fw_w, fw_w, n1);
  b.get(b.ord_kf, ord_kf, n2); b.get(b.ord_w, ord_w, n2);
  return CCM_OK;
}
}  // namespace ccm_internal

extern "C" int ccm_covis_update(ccm_ctx* ctx, int n_kf, int n_all, const int32_t* order_key, const int32_t* list_off, const int32_t* list_pt,
                                const uint8_t* list_skip, int n_pt, const int32_t* obs_off, const int32_t* obs_kf, int th, int cap, int32_t* row_off, int32_t* col,
                                int32_t* count, int32_t* fw_off, int32_t* fw_col, int32_t* fw_w, int32_t* ord_off, int32_t* ord_kf, int32_t* ord_w, int32_t* flags,
                                int32_t* needed) {
  return ccm_internal::covis_update_window(ctx, 0, n_kf, n_all, order_key, list_off, list_pt, list_skip, n_pt, obs_off, obs_kf, th, cap, row_off, col, count, fw_off,
                                           fw_col, fw_w, ord_off, ord_kf, ord_w, flags, needed);
}
