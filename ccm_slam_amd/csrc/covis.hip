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
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // device block in 4-byte words.  inputs: [order_key n_all | list_off n_kf + 1 | list_pt NL (null and skipped entries: -1) | obs_off n_pt + 1 | obs_kf NO];
  // work: 6 arrays of n_kf, extra_off n_kf + 1, extra_src / extra_w cap; outputs: [hdr 4 | flags n_kf | row_off, fw_off, ord_off n_kf + 1 each | six arrays of
  // cap].  One H2D of the inputs, one D2H of the outputs, both through the pinned staging buffer.
  const size_t K = (size_t)n_kf, A = (size_t)n_all, P = (size_t)n_pt, NL = (size_t)list_off[n_kf], NO = n_pt ? (size_t)obs_off[n_pt] : 0, C = (size_t)cap;
  const size_t n_in = A + (K + 1) + NL + (P + 1) + NO;
  const size_t n_work = 6 * K + (K + 1) + 2 * C;
  const size_t n_out = 4 + K + 3 * (K + 1) + 6 * C;
  void* scratch = nullptr;
  int rc = ccm_scratch(ctx, (n_in + n_work + n_out) * 4 + 64, &scratch);
  if (rc) return rc;
  void* pin = nullptr;
  rc = ccm_pin_scratch(ctx, (n_in > n_out ? n_in : n_out) * 4 + 64, &pin);
  if (rc) return rc;
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // the block may still feed an earlier copy
  int32_t* hp = (int32_t*)pin;
  size_t o = 0;
  auto put = [&](const void* src, size_t n) { const size_t at = o; if (n) memcpy(hp + o, src, n * 4); o += n; return at; };
  const size_t o_key = put(order_key, A);
  const size_t o_loff = put(list_off, K + 1);
  const size_t o_lpt = o;
  for (size_t e = 0; e < NL; e++) hp[o++] = covis_entry_counts(list_pt[e], list_skip[e]) ? list_pt[e] : -1;
  const size_t o_ooff = o;
  if (n_pt) put(obs_off, P + 1); else hp[o++] = 0;
  const size_t o_okf = put(obs_kf, NO);
  int32_t* d = (int32_t*)scratch;
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(d, hp, n_in * 4, hipMemcpyHostToDevice, ctx->stream));
  CovisArgs a;
  a.n_kf = n_kf; a.n_all = n_all; a.cap = cap; a.th = (uint32_t)th;
  a.order_key = d + o_key; a.list_off = d + o_loff; a.list_pt = d + o_lpt; a.obs_off = d + o_ooff; a.obs_kf = d + o_okf;
  int32_t* w = d + n_in;
  a.row_size = w; a.n_ge = w + K; a.fb_col = w + 2 * K; a.extra_cnt = w + 3 * K; a.cursor = w + 4 * K; a.chg = w + 5 * K; a.extra_off = w + 6 * K;
  a.extra_src = a.extra_off + K + 1; a.extra_w = a.extra_src + C;
  int32_t* dout = w + n_work;
  a.hdr = dout; a.flags = dout + 4; a.row_off = a.flags + K; a.fw_off = a.row_off + K + 1; a.ord_off = a.fw_off + K + 1;
  a.col = a.ord_off + K + 1; a.count = a.col + C; a.fw_col = a.count + C; a.fw_w = a.fw_col + C; a.ord_kf = a.fw_w + C; a.ord_w = a.ord_kf + C;
  if (small_window) covis_launch<kCvWindowSmall>(ctx, a); else covis_launch<kCvWindow>(ctx, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(hp, dout, n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t* h = hp;
  needed[0] = h[0]; needed[1] = h[1]; needed[2] = h[2];
  if (needed[0] > cap || needed[1] > cap || needed[2] > cap) return CCM_OK;   // nothing else is defined: the caller comes back with a larger cap
  h += 4;
  memcpy(flags, h, K * 4); h += K;
  memcpy(row_off, h, (K + 1) * 4); h += K + 1;
  memcpy(fw_off, h, (K + 1) * 4); h += K + 1;
  memcpy(ord_off, h, (K + 1) * 4); h += K + 1;
  const size_t n0 = (size_t)needed[0], n1 = (size_t)needed[1], n2 = (size_t)needed[2];
  if (n0) { memcpy(col, h, n0 * 4); memcpy(count, h + C, n0 * 4); }
  if (n1) { memcpy(fw_col, h + 2 * C, n1 * 4); memcpy(fw_w, h + 3 * C, n1 * 4); }
  if (n2) { memcpy(ord_kf, h + 4 * C, n2 * 4); memcpy(ord_w, h + 5 * C, n2 * 4); }
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
