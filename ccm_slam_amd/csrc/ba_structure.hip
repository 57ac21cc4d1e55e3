// ba_structure.hip — the pair structure of the Schur complement, built on the device.
// buildStructure (block_solver.hpp:143-295) needs, for every pair of free cameras that share a landmark, one Hschur block
// and the list of (edge_a, edge_c) observation pairs that contribute to it.  On the 4-agent merged map that is 3.1 M
// pairs in 64 k blocks; building it on the host (generate, two counting-sort passes, run-length split) was 55 % of
// ccm_ba_create.  Here: one thread per landmark counts its pairs, a workgroup per 32 landmarks emits them (key = ia*Cp + ic, value = both
// edge positions), a stable LSD radix sort groups them by block while keeping the landmark order inside a block (the summation order
// of the gather kernel, hence bit-identical results), run-length encoding yields the block list.  A sharded rank sorts
// the keys of ALL landmarks for the (global, rank-independent) block list and the pairs of its OWN landmarks for the
// instance lists, and finds its per-block ranges by binary search.  rocPRIM supplies scan and run-length encode, and the sort:
// one workgroup up to 1024 items, block sort + merge passes up to 2^18, onesweep above (ba_sort.h; rocPRIM itself would merge up to 2^20).
#include "common.h"
#include "ba_sort.h"
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <vector>

namespace {

constexpr int kTPB = 256;

// edges of a landmark are sorted by pose slot, fixed cameras (slot -1) first; a pair needs two different free cameras.  The pairs of a landmark are enumerated
// row after row: row a (an observation of a free camera) pairs with every later observation c of another camera, c ascending.  The order is sorted, so the
// later observations of the SAME camera follow a directly: row a holds positions a + 1 + d .. k1 - 1, d = row_same(...) of them skipped.
__device__ __forceinline__ int row_same(const int* __restrict__ cslot, int a, int k1, int ia) {
  int d = 0;
  while (a + 1 + d < k1 && cslot[a + 1 + d] == ia) d++;
  return d;
}

// one thread per landmark: the number of its pairs
__global__ void pairs_count_kernel(const int* __restrict__ pt_off, const int* __restrict__ cslot, int l0, int n_l, int* __restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_l) return;
  const int k1 = pt_off[l0 + i + 1];
  int n = 0;
  for (int a = pt_off[l0 + i]; a < k1; a++) {
    const int ia = cslot[a];
    if (ia >= 0) n += k1 - 1 - a - row_same(cslot, a, k1, ia);
  }
  cnt[i] = n;
}

// the emit: a workgroup takes kEmitLm consecutive landmarks and writes their pairs with thread t on pair t, t + 256, ... of the workgroup's range, so that every
// store of a wave is contiguous (one thread per landmark wrote its ~21 pairs to consecutive positions: neighbouring lanes 250 bytes apart, 0.46 TB/s).  The rows
// of the landmarks (their observations, in order) go through LDS in tiles of one row per thread: pose slots staged, each row's length and same-camera skip
// computed by its thread, lengths prefix-summed over the workgroup; a pair index then finds its row by binary search in that prefix (empty rows, those of fixed
// cameras and every landmark's last, share their successor's offset and are never found).  A landmark may span tiles: a row needs only its landmark's end
// (binary search in the workgroup's kEmitLm + 1 offsets) and the pose slots behind it, which are read from memory where they lie outside the tile.
// 32 landmarks (~200 rows, ~700 pairs on the 4-agent map) measured best of 16 ... 128 with one to four rows per thread.
constexpr int kEmitLm = 32;
__global__ __launch_bounds__(kTPB) void pairs_emit_kernel(const int* __restrict__ pt_off, const int* __restrict__ cslot, int l0, int n_l, int Cp,
                                                          const int* __restrict__ poff, uint32_t* __restrict__ keys, unsigned long long* __restrict__ vals) {
  __shared__ int s_off[kEmitLm + 1];  // first observation of each landmark of the workgroup, and the end
  __shared__ int s_cs[kTPB];          // pose slots of the tile's rows
  __shared__ int s_skip[kTPB];        // observations of the same camera behind each row
  __shared__ int s_row[kTPB + 1];     // index (inside the tile) of each row's first pair: exclusive scan of the lengths
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * kEmitLm, nl = min(kEmitLm, n_l - i0);
  for (int j = t; j <= nl; j += kTPB) s_off[j] = pt_off[l0 + i0 + j];
  __syncthreads();
  const int e0 = s_off[0], e1 = s_off[nl];
  int w = poff[i0];                   // where the tile's first pair goes
  for (int r0 = e0; r0 < e1; r0 += kTPB) {
    const int nr = min(kTPB, e1 - r0);
    if (t < nr) s_cs[t] = cslot[r0 + t];
    __syncthreads();
    auto cs = [&](int x) { return x - r0 < nr ? s_cs[x - r0] : cslot[x]; };
    int len = 0, d = 0;               // row t of the tile
    if (t < nr) {
      const int a = r0 + t, ia = s_cs[t];
      if (ia >= 0) {
        int lo = 0, hi = nl;          // its landmark: the last one that begins at or before a
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= a) lo = mid; else hi = mid; }
        const int k1 = s_off[lo + 1];
        while (a + 1 + d < k1 && cs(a + 1 + d) == ia) d++;
        len = k1 - 1 - a - d;
      }
      s_skip[t] = d;
    }
    s_row[t + 1] = len;
    if (t == 0) s_row[0] = 0;
    __syncthreads();
    for (int off = 1; off < kTPB; off <<= 1) {   // inclusive Hillis-Steele scan of s_row[1 ..]
      const int v = (t >= off) ? s_row[t + 1 - off] : 0;
      __syncthreads();
      s_row[t + 1] += v;
      __syncthreads();
    }
    const int n_tile = s_row[kTPB];   // (rows at and behind nr have length 0)
    for (int p = t; p < n_tile; p += kTPB) {
      int lo = 0, hi = nr;            // the row of pair p: the last one whose first pair is at or before p
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_row[mid] <= p) lo = mid; else hi = mid; }
      const int a = r0 + lo, c = a + 1 + s_skip[lo] + (p - s_row[lo]);
      keys[w + p] = (uint32_t)s_cs[lo] * (uint32_t)Cp + (uint32_t)cs(c);
      if (vals) vals[w + p] = ((unsigned long long)(uint32_t)a << 32) | (uint32_t)c;
    }
    w += n_tile;
    __syncthreads();                  // (the next tile overwrites what the pair loop reads)
  }
}

__global__ void split_kernel(const unsigned long long* vals, int n, int eb, int* inst_a, int* inst_c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  inst_a[i] = (int)(vals[i] >> 32) - eb;
  inst_c[i] = (int)(uint32_t)vals[i] - eb;
}

// inst_off[b] = first own pair with key >= U[b]; inst_off[nOff] = n_own
__global__ void ranges_kernel(const uint32_t* U, int nOff, const uint32_t* own_keys, int n_own, int* inst_off) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nOff) return;
  if (b == nOff) { inst_off[b] = n_own; return; }
  const uint32_t key = U[b];
  int lo = 0, hi = n_own;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (own_keys[mid] < key) lo = mid + 1; else hi = mid; }
  inst_off[b] = lo;
}

struct Tmp {
  ccm_ctx* ctx;
  std::vector<std::pair<void*, size_t>> blocks;
  template <typename T> int get(size_t n, T** out) {
    void* p = nullptr; size_t actual = 0;
    if (int rc = ccm_pool_get(ctx, std::max<size_t>(n, 1) * sizeof(T), &p, &actual)) return rc;
    blocks.push_back({p, actual});
    *out = (T*)p;
    return CCM_OK;
  }
  ~Tmp() { hipStreamSynchronize(ctx->stream); for (auto& b : blocks) ccm_pool_put(ctx, b.first, b.second); }
};

#define ST_RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
#define ST_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return ccm_set_error(ctx, CCM_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// counts + emits the pairs of landmarks [l0, l1) ; returns device keys (and values) plus the number of pairs
int emit_pairs(ccm_ctx* ctx, Tmp& tmp, const int* d_pt_off, const int* d_cslot, int l0, int l1, int Cp, bool with_vals, uint32_t** keys,
               unsigned long long** vals, int* n_out) {
  const int n_l = l1 - l0;
  *keys = nullptr; if (vals) *vals = nullptr; *n_out = 0;
  if (n_l <= 0) return CCM_OK;
  int *cnt = nullptr, *poff = nullptr;
  ST_RC(tmp.get((size_t)n_l + 1, &cnt)); ST_RC(tmp.get((size_t)n_l + 1, &poff));
  ST_HIP(hipMemsetAsync(cnt + n_l, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(pairs_count_kernel, dim3(ccm_div_up(n_l, kTPB)), dim3(kTPB), 0, ctx->stream, d_pt_off, d_cslot, l0, n_l, cnt);
  size_t bytes = 0;
  ST_HIP(rocprim::exclusive_scan(nullptr, bytes, cnt, poff, 0, (size_t)n_l + 1, rocprim::plus<int>(), ctx->stream));
  char* scratch = nullptr;
  ST_RC(tmp.get(bytes, &scratch));
  ST_HIP(rocprim::exclusive_scan(scratch, bytes, cnt, poff, 0, (size_t)n_l + 1, rocprim::plus<int>(), ctx->stream));
  int total = 0;
  ST_HIP(hipMemcpyAsync(&total, poff + n_l, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ST_HIP(hipStreamSynchronize(ctx->stream));
  *n_out = total;
  if (total == 0) return CCM_OK;
  ST_RC(tmp.get((size_t)total, keys));
  if (with_vals) ST_RC(tmp.get((size_t)total, vals));
  hipLaunchKernelGGL(pairs_emit_kernel, dim3((unsigned)ccm_div_up(n_l, kEmitLm)), dim3(kTPB), 0, ctx->stream, d_pt_off, d_cslot, l0, n_l, Cp,
                     (const int*)poff, *keys, with_vals ? *vals : (unsigned long long*)nullptr);
  ST_HIP(hipGetLastError());
  return CCM_OK;
}

}  // namespace

// d_pt_off [Lp+1] / d_cslot [E] (device): landmark-sorted edge ranges and the pose slot (-1 = fixed) of every edge position.
// Own landmarks [lb, le), eb = first own edge position.  Outputs (device, blocks appended to `keep`, owned by the caller): the global block
// list d_U [nOff] (key = ia * Cp + ic, ascending), inst_off [nOff+1] / inst_a / inst_c [n_inst].  Two host syncs (pair count, block count).
int ccm_ba_build_pairs(ccm_ctx* ctx, const int* d_pt_off, const int* d_cslot, int Lp, int Cp, int lb, int le, int eb,
                       uint32_t** d_U_out, int* nOff_out, int** d_inst_off, int** d_inst_a, int** d_inst_c, int64_t* n_inst,
                       std::vector<std::pair<void*, size_t>>& keep) {
  if (Cp > 65535) return ccm_set_error(ctx, CCM_E_ARG, "bundle adjustment: more than 65535 free cameras (32-bit block keys)");
  *n_inst = 0; *nOff_out = 0; *d_U_out = nullptr;
  auto keep_get = [&](size_t n, int** out) -> int {
    void* p = nullptr; size_t actual = 0;
    if (int rc = ccm_pool_get(ctx, std::max<size_t>(n, 1) * sizeof(int), &p, &actual)) return rc;
    keep.push_back({p, actual}); *out = (int*)p; return CCM_OK;
  };
  Tmp tmp{ctx, {}};
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)Cp * (uint64_t)Cp) bits++;
  const bool whole = (lb == 0 && le == Lp);
  // ---- own pairs, sorted by block (stable: landmark order inside a block) ----
  uint32_t* ok = nullptr; unsigned long long* ov = nullptr; int n_own = 0;
  ST_RC(emit_pairs(ctx, tmp, d_pt_off, d_cslot, lb, le, Cp, true, &ok, &ov, &n_own));
  uint32_t* ok_sorted = ok; unsigned long long* ov_sorted = ov;
  if (n_own) {
    uint32_t* ok2 = nullptr; unsigned long long* ov2 = nullptr;
    ST_RC(tmp.get((size_t)n_own, &ok2)); ST_RC(tmp.get((size_t)n_own, &ov2));
    rocprim::double_buffer<uint32_t> kb(ok, ok2);
    rocprim::double_buffer<unsigned long long> vb(ov, ov2);
    const bool onesweep = ba_sort_onesweep((size_t)n_own);
    size_t bytes = 0;
    ST_HIP(ba_radix_sort_pairs(onesweep, nullptr, bytes, kb, vb, (unsigned)n_own, bits, ctx->stream));
    char* scratch = nullptr;
    ST_RC(tmp.get(bytes, &scratch));
    ST_HIP(ba_radix_sort_pairs(onesweep, scratch, bytes, kb, vb, (unsigned)n_own, bits, ctx->stream));
    ok_sorted = kb.current(); ov_sorted = vb.current();
  }
  // ---- global block list: keys of all landmarks (the own ones when this rank owns everything) ----
  uint32_t* gk_sorted = ok_sorted; int n_all = n_own;
  if (!whole) {
    uint32_t* gk = nullptr;
    ST_RC(emit_pairs(ctx, tmp, d_pt_off, d_cslot, 0, Lp, Cp, false, &gk, nullptr, &n_all));
    gk_sorted = gk;
    if (n_all) {
      uint32_t* gk2 = nullptr;
      ST_RC(tmp.get((size_t)n_all, &gk2));
      rocprim::double_buffer<uint32_t> kb(gk, gk2);
      const bool onesweep = ba_sort_onesweep((size_t)n_all);
      size_t bytes = 0;
      ST_HIP(ba_radix_sort_keys(onesweep, nullptr, bytes, kb, (unsigned)n_all, bits, ctx->stream));
      char* scratch = nullptr;
      ST_RC(tmp.get(bytes, &scratch));
      ST_HIP(ba_radix_sort_keys(onesweep, scratch, bytes, kb, (unsigned)n_all, bits, ctx->stream));
      gk_sorted = kb.current();
    }
  }
  int nOff = 0;
  uint32_t* U = nullptr; unsigned* counts = nullptr; int* runs = nullptr;
  if (n_all) {
    ST_RC(tmp.get((size_t)n_all, &U)); ST_RC(tmp.get((size_t)n_all, &counts)); ST_RC(tmp.get(1, &runs));
    size_t bytes = 0;
    ST_HIP(rocprim::run_length_encode(nullptr, bytes, gk_sorted, (unsigned)n_all, U, counts, runs, ctx->stream));
    char* scratch = nullptr;
    ST_RC(tmp.get(bytes, &scratch));
    ST_HIP(rocprim::run_length_encode(scratch, bytes, gk_sorted, (unsigned)n_all, U, counts, runs, ctx->stream));
    ST_HIP(hipMemcpyAsync(&nOff, runs, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ST_HIP(hipStreamSynchronize(ctx->stream));
  }
  int* U_keep = nullptr;
  ST_RC(keep_get((size_t)nOff, &U_keep));
  if (nOff) ST_HIP(hipMemcpyAsync(U_keep, U, (size_t)nOff * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
  ST_RC(keep_get((size_t)nOff + 1, d_inst_off)); ST_RC(keep_get((size_t)n_own, d_inst_a)); ST_RC(keep_get((size_t)n_own, d_inst_c));
  hipLaunchKernelGGL(ranges_kernel, dim3(ccm_div_up(nOff + 1, kTPB)), dim3(kTPB), 0, ctx->stream, (const uint32_t*)U, nOff, (const uint32_t*)ok_sorted, n_own,
                     *d_inst_off);
  if (n_own) hipLaunchKernelGGL(split_kernel, dim3(ccm_div_up(n_own, kTPB)), dim3(kTPB), 0, ctx->stream, (const unsigned long long*)ov_sorted, n_own, eb, *d_inst_a, *d_inst_c);
  ST_HIP(hipGetLastError());
  *d_U_out = (uint32_t*)U_keep;
  *nOff_out = nOff;
  *n_inst = n_own;
  return CCM_OK;   // ~Tmp waits for the stream before the temporaries go back to the pool
}
