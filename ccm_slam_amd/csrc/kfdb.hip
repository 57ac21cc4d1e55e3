// kfdb.hip — the keyframe database of place recognition on the device: KeyFrameDatabase::add / erase / clear and phase 1 of
// DetectLoopCandidates / DetectMapMatchCandidates / DetectRelocalizationCandidates (cslam/src/Database.cpp:37-146, 206-271, 329-385).
//
// Layout (one ccm_kfdb handle):
//   slot arena   per added keyframe its BowVector (word ids int32 ascending, L1 values f64) contiguous in d_word / d_val, and a KfdbSlot
//                (offset, length, client id, alive).  Slots are numbered in add() order and a compaction keeps that order, so the slot
//                number orders keyframes exactly as the reference's insertion-ordered word lists do.
//   base file    a CSR over the vocabulary's words (n_words + 1 offsets) listing the slots < base_end that carry the word, rebuilt on the
//                device by a counting sort: word histogram over live slots, exclusive scan, atomic-cursor scatter.  The order of the
//                slots inside one word's list is whatever the atomics give: the query never needs it (see below).
//   append log   slots base_end .. n_slots, added since the last rebuild; the query scans them directly.  A rebuild follows when the log
//                passes log_capacity keyframes or dead (erased) slots pass a quarter of the arena (then the arena is compacted first).
//
// Why no list order is needed: the reference lists a keyframe in lKFsSharingWords when it first meets it, walking the query's words in
// ascending id and each word's list in insertion order.  So its position is fixed by (r*, add order), r* = rank in the query's BowVector of
// the first query word the keyframe shares.  The count kernel takes r* with an atomic minimum and the shared-word count with an atomic add
// (both order-independent, so results are deterministic); the host sorts the few selected slots by (r*, add order).
//
// Query chain (caller's stream, scratch of the caller's context): count -> select -> score, then one read-back.
//   count   load-balanced walk over the postings of the query's words (prefix over the list lengths, one lane per posting found by
//           binary search) + one block per log slot (each lane binary-searches its word in the query's word list in LDS); filters from a
//           per-query slot bitset (map membership, self, connected keyframes) and the client-id mask.
//   select  max_common, min_common = (int)(max_common * 0.8f), compaction of the slots with count > min_common.
//   score   one wave per selected slot: L1Scoring::score (thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-66) with the common words' terms
//           compacted in word order through a ballot prefix and added IN ORDER by one lane in f64 — bit-identical to the reference,
//           -0.0 for disjoint vectors included.
// No float atomics anywhere.
#include "common.h"

#include <algorithm>
#include <numeric>
#include <shared_mutex>
#include <unordered_map>

namespace {

constexpr int kMaxQueryWords = 4096;   // LDS plan of the count / score kernels (a BowVector has at most one word per ORB feature)
constexpr int kDefaultLogCap = 64;
constexpr int kCountBaseBlocks = 128;  // grid-stride walk over the postings of the base file
constexpr int kScoreBlocks = 256;      // one wave each, grid-stride over the selected slots
constexpr int kScanChunk = 1024;       // elements per block of the scan (256 threads x 4)
constexpr int kFirstReadBack = 512;    // selected rows read back with the header; more need a second copy

struct KfdbSlot { int32_t off, len, group, alive; };
struct KfdbSel { int32_t slot, first, count, pad; double score; };   // first = nq - r*

// ---- block-wide helpers -----------------------------------------------------------------------------------
// exclusive prefix of v over a block of NT threads (NT multiple of 64); *total = sum.  lds: NT / 64 ints.
template <int NT>
__device__ inline int block_excl_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) lds[wv] = x;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; w++) {
    const int s = lds[w];
    if (w < wv) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

// first index i with a[i] == w in the ascending list a[0..n), -1 if absent
__device__ inline int lds_find(const int32_t* a, int n, int32_t w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == w) ? lo : -1;
}

// ---- rebuild: counting sort of the live slots' words ------------------------------------------------------
__global__ __launch_bounds__(256) void kfdb_hist_kernel(const KfdbSlot* slot, const int32_t* word, int32_t* hist) {
  const KfdbSlot s = slot[blockIdx.x];
  if (!s.alive) return;
  for (int t = threadIdx.x; t < s.len; t += 256) atomicAdd(&hist[word[s.off + t]], 1);
}

__global__ __launch_bounds__(256) void kfdb_scan_reduce_kernel(const int32_t* a, int n, int32_t* bsum) {
  __shared__ int lds[4];
  const int base = blockIdx.x * kScanChunk + threadIdx.x * 4;
  int v = 0;
  for (int k = 0; k < 4; k++) if (base + k < n) v += a[base + k];
  int total;
  block_excl_scan<256>(v, lds, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// exclusive scan of nb block sums in place, one block
__global__ __launch_bounds__(1024) void kfdb_scan_bsum_kernel(int32_t* bsum, int nb) {
  __shared__ int lds[16];
  int carry = 0;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int total;
    const int ex = block_excl_scan<1024>(v, lds, &total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(256) void kfdb_scan_apply_kernel(int32_t* a, int n, const int32_t* bsum, int32_t* cursor) {
  __shared__ int lds[4];
  const int base = blockIdx.x * kScanChunk + threadIdx.x * 4;
  int v[4], s = 0;
  for (int k = 0; k < 4; k++) { v[k] = base + k < n ? a[base + k] : 0; s += v[k]; }
  int total;
  int run = bsum[blockIdx.x] + block_excl_scan<256>(s, lds, &total);
  for (int k = 0; k < 4; k++) {
    if (base + k < n) { a[base + k] = run; cursor[base + k] = run; }
    run += v[k];
  }
}

__global__ __launch_bounds__(256) void kfdb_scatter_kernel(const KfdbSlot* slot, const int32_t* word, int32_t* cursor, int32_t* csr_slot) {
  const KfdbSlot s = slot[blockIdx.x];
  if (!s.alive) return;
  for (int t = threadIdx.x; t < s.len; t += 256) csr_slot[atomicAdd(&cursor[word[s.off + t]], 1)] = (int32_t)blockIdx.x;
}

// compaction: new slot b takes the terms of an old slot (mv[b] = src offset, dst offset, length)
__global__ __launch_bounds__(256) void kfdb_compact_kernel(const int32_t* mv, const int32_t* w_in, const double* v_in, int32_t* w_out, double* v_out) {
  const int src = mv[3 * blockIdx.x], dst = mv[3 * blockIdx.x + 1], len = mv[3 * blockIdx.x + 2];
  for (int t = threadIdx.x; t < len; t += 256) { w_out[dst + t] = w_in[src + t]; v_out[dst + t] = v_in[src + t]; }
}

// ---- query ------------------------------------------------------------------------------------------------
__device__ inline bool kfdb_pass(const KfdbSlot& s, int slot, const uint32_t* allow_bits, uint64_t excl_groups) {
  if (!s.alive) return false;
  if (!((allow_bits[slot >> 5] >> (slot & 31)) & 1u)) return false;
  return !(s.group >= 0 && s.group < 64 && ((excl_groups >> s.group) & 1ull));
}

// blocks [0, n_base_blocks): postings of the base file; block n_base_blocks + j: log slot base_end + j.
// dynamic LDS: qw[nq], pref[nq + 1]
__global__ __launch_bounds__(256) void kfdb_count_kernel(const int32_t* qw, int nq, const int32_t* csr_off, const int32_t* csr_slot, const KfdbSlot* slot,
                                                         const int32_t* word, int base_end, int n_base_blocks, const uint32_t* allow_bits, uint64_t excl_groups,
                                                         int32_t* count, uint32_t* first) {
  extern __shared__ int32_t sm[];
  int32_t* s_qw = sm;
  int32_t* s_pref = sm + nq;
  __shared__ int lds[4];
  for (int i = threadIdx.x; i < nq; i += 256) s_qw[i] = qw[i];
  __syncthreads();
  if ((int)blockIdx.x < n_base_blocks) {
    int carry = 0;
    for (int base = 0; base < nq; base += 256) {
      const int i = base + threadIdx.x;
      const int len = i < nq ? csr_off[s_qw[i] + 1] - csr_off[s_qw[i]] : 0;
      int total;
      const int ex = block_excl_scan<256>(len, lds, &total);
      if (i < nq) s_pref[i] = carry + ex;
      carry += total;
    }
    if (threadIdx.x == 0) s_pref[nq] = carry;
    __syncthreads();
    const int total = s_pref[nq];
    for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += n_base_blocks * 256) {
      int lo = 0, hi = nq - 1;   // last i with pref[i] <= p
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_pref[mid] <= p) lo = mid; else hi = mid - 1;
      }
      const int sl = csr_slot[csr_off[s_qw[lo]] + (p - s_pref[lo])];
      const KfdbSlot s = slot[sl];
      if (kfdb_pass(s, sl, allow_bits, excl_groups)) {
        atomicAdd(&count[sl], 1);
        atomicMax(&first[sl], (uint32_t)(nq - lo));
      }
    }
  } else {
    const int sl = base_end + (int)blockIdx.x - n_base_blocks;
    const KfdbSlot s = slot[sl];
    if (!kfdb_pass(s, sl, allow_bits, excl_groups)) return;
    for (int t = threadIdx.x; t < s.len; t += 256) {
      const int i = lds_find(s_qw, nq, word[s.off + t]);
      if (i >= 0) {
        atomicAdd(&count[sl], 1);
        atomicMax(&first[sl], (uint32_t)(nq - i));
      }
    }
  }
}

// one block: hdr = {n_sel, max_common, n_sharing, min_common}; sel rows in slot order
__global__ __launch_bounds__(1024) void kfdb_select_kernel(const int32_t* count, const uint32_t* first, int n_slots, int32_t* hdr, KfdbSel* sel) {
  __shared__ int s_max[16], s_cnt[16], lds[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int mx = 0, listed = 0;
  for (int s = threadIdx.x; s < n_slots; s += 1024) {
    const int c = count[s];
    mx = max(mx, c);
    listed += c > 0;
  }
  for (int d = 32; d; d >>= 1) { mx = max(mx, __shfl_xor(mx, d, 64)); listed += __shfl_xor(listed, d, 64); }
  if (lane == 0) { s_max[wv] = mx; s_cnt[wv] = listed; }
  __syncthreads();
  int max_common = 0, n_sharing = 0;
  for (int w = 0; w < 16; w++) { max_common = max(max_common, s_max[w]); n_sharing += s_cnt[w]; }
  const int min_common = (int)((float)max_common * 0.8f);   // Database.cpp:118 (int minCommonWords = maxCommonWords*0.8f)
  int carry = 0;
  for (int base = 0; base < n_slots; base += 1024) {
    const int s = base + threadIdx.x;
    const int c = s < n_slots ? count[s] : 0;
    const int take = c > min_common;
    int total;
    const int pos = carry + block_excl_scan<1024>(take, lds, &total);
    if (take) { KfdbSel r; r.slot = s; r.first = (int32_t)first[s]; r.count = c; r.pad = 0; r.score = 0.0; sel[pos] = r; }
    carry += total;
  }
  if (threadIdx.x == 0) { hdr[0] = carry; hdr[1] = max_common; hdr[2] = n_sharing; hdr[3] = min_common; }
}

// one wave per row: score(q, slot) as L1Scoring::score.  Rows: sel[i].slot (sel != nullptr, n = *n_dev) or slots[i] (n = n_host).
// dynamic LDS: qv[nq] (f64), qw[nq]
__global__ __launch_bounds__(64) void kfdb_score_kernel(const int32_t* qw, const double* qv, int nq, const KfdbSlot* slot, const int32_t* word, const double* val,
                                                        KfdbSel* sel, const int32_t* n_dev, const int32_t* slots, int n_host, double* out) {
  extern __shared__ double smd[];
  double* s_qv = smd;
  int32_t* s_qw = (int32_t*)(smd + nq);
  __shared__ double s_term[64];
  const int lane = threadIdx.x;
  for (int i = lane; i < nq; i += 64) { s_qw[i] = qw[i]; s_qv[i] = qv[i]; }
  __syncthreads();
  const int n = sel ? *n_dev : n_host;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const KfdbSlot s = slot[sel ? sel[r].slot : slots[r]];
    double acc = 0.0;
    for (int base = 0; base < s.len; base += 64) {
      const int t = base + lane;
      bool hit = false;
      double term = 0.0;
      if (t < s.len) {
        const int i = lds_find(s_qw, nq, word[s.off + t]);
        if (i >= 0) {
          const double vi = s_qv[i], wi = val[s.off + t];
          term = fabs(vi - wi) - fabs(vi) - fabs(wi);   // ScoringObject.cpp:42
          hit = true;
        }
      }
      const unsigned long long m = __ballot(hit);
      if (hit) s_term[__popcll(m & ((1ull << lane) - 1ull))] = term;
      __syncthreads();
      if (lane == 0) {
        const int k = __popcll(m);
        for (int j = 0; j < k; j++) acc += s_term[j];   // in word order, one rounding per term as the reference's loop
      }
      __syncthreads();
    }
    if (lane == 0) {
      const double sc = -acc / 2.0;   // ScoringObject.cpp:63
      if (sel) sel[r].score = sc; else out[r] = sc;
    }
  }
}

int check_words(ccm_ctx* ctx, int n_words, int n, const int32_t* word, const double* value, const char* what) {
  if (n < 0 || (n && (!word || !value))) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": bad BowVector arguments");
  for (int i = 0; i < n; i++) {
    if (word[i] < 0 || word[i] >= n_words) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": word id out of range");
    if (i && word[i] <= word[i - 1]) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": word ids must be ascending and unique");
  }
  return CCM_OK;
}

}  // namespace

struct ccm_kfdb {
  int device = 0, n_words = 0, log_cap = kDefaultLogCap;
  std::shared_mutex mu;   // queries shared, mutations exclusive
  uint64_t generation = 0;
  // device
  int32_t* d_word = nullptr; double* d_val = nullptr; int64_t term_cap = 0;
  KfdbSlot* d_slot = nullptr; int slot_cap = 0;
  int32_t* d_csr_off = nullptr;    // [n_words + 1]
  int32_t* d_cursor = nullptr;     // [n_words + 1], rebuild only
  int32_t* d_bsum = nullptr;       // scan block sums
  int32_t* d_csr_slot = nullptr; int64_t csr_cap = 0;
  // host mirror of the slot table
  std::vector<KfdbSlot> slot;
  std::vector<int64_t> key, seq;
  std::unordered_map<int64_t, int> live;   // key -> slot
  int64_t n_terms = 0, next_seq = 0;
  int n_slots = 0, base_end = 0, n_dead = 0;
};

namespace {

int kfdb_ctx_ok(ccm_kfdb* db, ccm_ctx* ctx, const char* what) {
  if (!db || !ctx) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": NULL handle");
  if (ctx->device != db->device) return ccm_set_error(ctx, CCM_E_ARG, std::string(what) + ": the context is on another device than the database");
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  return CCM_OK;
}

template <class T>
int grow(ccm_ctx* ctx, T** p, int64_t* cap, int64_t need, int64_t keep) {
  if (need <= *cap) return CCM_OK;
  int64_t nc = std::max<int64_t>(*cap, 1024);
  while (nc < need) nc *= 2;
  T* q = nullptr;
  CCM_HIP_CHECK(ctx, hipMalloc(&q, (size_t)nc * sizeof(T)));
  if (keep) CCM_HIP_CHECK(ctx, hipMemcpyAsync(q, *p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (*p) CCM_HIP_CHECK(ctx, hipFree(*p));
  *p = q; *cap = nc;
  return CCM_OK;
}

// compaction of dead slots (if any) and counting-sort rebuild of the base file over every slot; caller holds the exclusive lock
int kfdb_rebuild(ccm_kfdb* db, ccm_ctx* ctx) {
  if (db->n_dead) {
    std::vector<int32_t> mv;
    std::vector<KfdbSlot> ns; std::vector<int64_t> nk, nq;
    int64_t off = 0;
    for (int s = 0; s < db->n_slots; s++) {
      if (!db->slot[s].alive) continue;
      KfdbSlot t = db->slot[s];
      mv.push_back(t.off); mv.push_back((int32_t)off); mv.push_back(t.len);
      t.off = (int32_t)off; off += t.len;
      ns.push_back(t); nk.push_back(db->key[s]); nq.push_back(db->seq[s]);
    }
    if (!ns.empty()) {
      int32_t* w2 = nullptr; double* v2 = nullptr; int32_t* d_mv = nullptr;
      CCM_HIP_CHECK(ctx, hipMalloc(&w2, (size_t)db->term_cap * 4));
      CCM_HIP_CHECK(ctx, hipMalloc(&v2, (size_t)db->term_cap * 8));
      CCM_HIP_CHECK(ctx, hipMalloc(&d_mv, mv.size() * 4));
      CCM_HIP_CHECK(ctx, hipMemcpyAsync(d_mv, mv.data(), mv.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(kfdb_compact_kernel, dim3((unsigned)ns.size()), dim3(256), 0, ctx->stream, d_mv, db->d_word, db->d_val, w2, v2);
      CCM_HIP_CHECK(ctx, hipGetLastError());
      CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
      hipFree(d_mv); hipFree(db->d_word); hipFree(db->d_val);
      db->d_word = w2; db->d_val = v2;
      CCM_HIP_CHECK(ctx, hipMemcpyAsync(db->d_slot, ns.data(), ns.size() * sizeof(KfdbSlot), hipMemcpyHostToDevice, ctx->stream));
    }
    db->slot.swap(ns); db->key.swap(nk); db->seq.swap(nq);
    db->n_slots = (int)db->slot.size(); db->n_terms = off; db->n_dead = 0;
    db->live.clear();
    for (int s = 0; s < db->n_slots; s++) db->live[db->key[s]] = s;
  }
  const int n = db->n_words + 1;
  CCM_HIP_CHECK(ctx, hipMemsetAsync(db->d_csr_off, 0, (size_t)n * 4, ctx->stream));
  { int rc = grow(ctx, &db->d_csr_slot, &db->csr_cap, std::max<int64_t>(db->n_terms, 1), 0); if (rc) return rc; }
  if (db->n_slots) {
    const int nb = ccm_div_up(n, kScanChunk);
    hipLaunchKernelGGL(kfdb_hist_kernel, dim3(db->n_slots), dim3(256), 0, ctx->stream, db->d_slot, db->d_word, db->d_csr_off);
    hipLaunchKernelGGL(kfdb_scan_reduce_kernel, dim3(nb), dim3(256), 0, ctx->stream, db->d_csr_off, n, db->d_bsum);
    hipLaunchKernelGGL(kfdb_scan_bsum_kernel, dim3(1), dim3(1024), 0, ctx->stream, db->d_bsum, nb);
    hipLaunchKernelGGL(kfdb_scan_apply_kernel, dim3(nb), dim3(256), 0, ctx->stream, db->d_csr_off, n, db->d_bsum, db->d_cursor);
    hipLaunchKernelGGL(kfdb_scatter_kernel, dim3(db->n_slots), dim3(256), 0, ctx->stream, db->d_slot, db->d_word, db->d_cursor, db->d_csr_slot);
    CCM_HIP_CHECK(ctx, hipGetLastError());
  }
  db->base_end = db->n_slots;
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return CCM_OK;
}

// H2D of n_bytes from host memory through the context's pinned staging block
int stage_h2d(ccm_ctx* ctx, void* dst, const void* src, size_t n_bytes) {
  if (!n_bytes) return CCM_OK;
  void* pin = nullptr;
  { int rc = ccm_pin_scratch(ctx, n_bytes, &pin); if (rc) return rc; }
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // the block may still feed an earlier copy
  std::memcpy(pin, src, n_bytes);
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(dst, pin, n_bytes, hipMemcpyHostToDevice, ctx->stream));
  return CCM_OK;
}

}  // namespace

extern "C" int ccm_kfdb_create(ccm_ctx* ctx, int n_words, int log_capacity, ccm_kfdb** out) {
  if (!ctx || !out || n_words <= 0 || n_words >= (1 << 30) || log_capacity < 0) return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfdb_create: bad args");
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ccm_kfdb* db = new ccm_kfdb();
  db->device = ctx->device; db->n_words = n_words; db->log_cap = log_capacity ? log_capacity : kDefaultLogCap;
  const int n = n_words + 1;
  const bool ok = hipMalloc(&db->d_csr_off, (size_t)n * 4) == hipSuccess && hipMalloc(&db->d_cursor, (size_t)n * 4) == hipSuccess &&
                  hipMalloc(&db->d_bsum, (size_t)ccm_div_up(n, kScanChunk) * 4) == hipSuccess &&
                  hipMemsetAsync(db->d_csr_off, 0, (size_t)n * 4, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    ccm_kfdb_destroy(db);
    return ccm_set_error(ctx, CCM_E_HIP, "ccm_kfdb_create: device allocation failed");
  }
  *out = db;
  return CCM_OK;
}

extern "C" void ccm_kfdb_destroy(ccm_kfdb* db) {
  if (!db) return;
  hipSetDevice(db->device);
  hipFree(db->d_word); hipFree(db->d_val); hipFree(db->d_slot); hipFree(db->d_csr_off); hipFree(db->d_cursor); hipFree(db->d_bsum); hipFree(db->d_csr_slot);
  delete db;
}

extern "C" int ccm_kfdb_add(ccm_kfdb* db, ccm_ctx* ctx, int64_t key, int32_t group, int n, const int32_t* word, const double* value) {
  { int rc = kfdb_ctx_ok(db, ctx, "ccm_kfdb_add"); if (rc) return rc; }
  { int rc = check_words(ctx, db->n_words, n, word, value, "ccm_kfdb_add"); if (rc) return rc; }
  std::unique_lock<std::shared_mutex> lk(db->mu);
  if (db->live.count(key)) return ccm_set_error(ctx, CCM_E_STATE, "ccm_kfdb_add: the key is already in the database");
  if (db->n_terms + n >= ((int64_t)1 << 31)) return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfdb_add: more than 2^31 words in the database");
  int64_t scap = db->slot_cap;
  { int rc = grow(ctx, &db->d_slot, &scap, db->n_slots + 1, db->n_slots); if (rc) return rc; }
  db->slot_cap = (int)scap;
  if (db->n_terms + n > db->term_cap) {
    int64_t c1 = db->term_cap, c2 = db->term_cap;
    { int rc = grow(ctx, &db->d_word, &c1, db->n_terms + n, db->n_terms); if (rc) return rc; }
    { int rc = grow(ctx, &db->d_val, &c2, db->n_terms + n, db->n_terms); if (rc) return rc; }
    db->term_cap = c1;
  }
  const KfdbSlot s{(int32_t)db->n_terms, n, group, 1};
  // one staged copy: terms then the slot record
  const size_t bw = (size_t)n * 4, bv = (size_t)n * 8;
  void* pin = nullptr;
  { int rc = ccm_pin_scratch(ctx, bw + bv + sizeof(KfdbSlot), &pin); if (rc) return rc; }
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (n) { std::memcpy(pin, value, bv); std::memcpy((char*)pin + bv, word, bw); }
  std::memcpy((char*)pin + bv + bw, &s, sizeof s);
  if (n) {
    CCM_HIP_CHECK(ctx, hipMemcpyAsync(db->d_val + db->n_terms, pin, bv, hipMemcpyHostToDevice, ctx->stream));
    CCM_HIP_CHECK(ctx, hipMemcpyAsync(db->d_word + db->n_terms, (char*)pin + bv, bw, hipMemcpyHostToDevice, ctx->stream));
  }
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(db->d_slot + db->n_slots, (char*)pin + bv + bw, sizeof s, hipMemcpyHostToDevice, ctx->stream));
  db->slot.push_back(s); db->key.push_back(key); db->seq.push_back(db->next_seq++);
  db->live[key] = db->n_slots;
  db->n_slots++; db->n_terms += n;
  if (db->n_slots - db->base_end > db->log_cap || db->n_dead * 4 > db->n_slots) {
    int rc = kfdb_rebuild(db, ctx);
    if (rc) return rc;
  }
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  db->generation++;
  return CCM_OK;
}

extern "C" int ccm_kfdb_erase(ccm_kfdb* db, ccm_ctx* ctx, int64_t key) {
  { int rc = kfdb_ctx_ok(db, ctx, "ccm_kfdb_erase"); if (rc) return rc; }
  std::unique_lock<std::shared_mutex> lk(db->mu);
  auto it = db->live.find(key);
  if (it == db->live.end()) return CCM_OK;   // Database.cpp:45-64: a keyframe that is not listed is not found
  const int s = it->second;
  db->live.erase(it);
  db->slot[s].alive = 0;
  db->n_dead++;
  { int rc = stage_h2d(ctx, &db->d_slot[s].alive, &db->slot[s].alive, sizeof(int32_t)); if (rc) return rc; }
  if (db->n_dead * 4 > db->n_slots) {
    int rc = kfdb_rebuild(db, ctx);
    if (rc) return rc;
  }
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  db->generation++;
  return CCM_OK;
}

extern "C" int ccm_kfdb_clear(ccm_kfdb* db, ccm_ctx* ctx) {
  { int rc = kfdb_ctx_ok(db, ctx, "ccm_kfdb_clear"); if (rc) return rc; }
  std::unique_lock<std::shared_mutex> lk(db->mu);
  db->slot.clear(); db->key.clear(); db->seq.clear(); db->live.clear();
  db->n_terms = 0; db->n_slots = db->base_end = db->n_dead = 0;
  CCM_HIP_CHECK(ctx, hipMemsetAsync(db->d_csr_off, 0, (size_t)(db->n_words + 1) * 4, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  db->generation++;
  return CCM_OK;
}

extern "C" int ccm_kfdb_query(ccm_kfdb* db, ccm_ctx* ctx, int n, const int32_t* word, const double* value, const ccm_kfdb_filter* f, int cap, int64_t* key_out,
                              int32_t* count_out, float* score_out, double* score64_out, int* n_out, int* n_sharing_out, int* max_common_out,
                              uint64_t* generation_out) {
  { int rc = kfdb_ctx_ok(db, ctx, "ccm_kfdb_query"); if (rc) return rc; }
  if (!n_out || cap < 0 || (cap && (!key_out || !count_out || !score_out || !score64_out)) || n > kMaxQueryWords ||
      (f && ((f->n_allow < 0 || (f->n_allow && !f->allow)) || (f->n_exclude < 0 || (f->n_exclude && !f->exclude)))))
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfdb_query: bad args (at most 4096 query words)");
  { int rc = check_words(ctx, db->n_words, n, word, value, "ccm_kfdb_query"); if (rc) return rc; }
  std::shared_lock<std::shared_mutex> lk(db->mu);
  *n_out = 0;
  if (n_sharing_out) *n_sharing_out = 0;
  if (max_common_out) *max_common_out = 0;
  if (generation_out) *generation_out = db->generation;
  const int ns = db->n_slots;
  if (n == 0 || db->live.empty()) return CCM_OK;
  // per-query slot bitset: map membership (allow), the query itself, its connected keyframes
  const int nbw = ccm_div_up(ns, 32);
  std::vector<uint32_t> bits(nbw, (f && f->allow) ? 0u : ~0u);
  if (f && f->allow)
    for (int i = 0; i < f->n_allow; i++) { auto it = db->live.find(f->allow[i]); if (it != db->live.end()) bits[it->second >> 5] |= 1u << (it->second & 31); }
  auto drop = [&](int64_t k) { auto it = db->live.find(k); if (it != db->live.end()) bits[it->second >> 5] &= ~(1u << (it->second & 31)); };
  if (f) {
    if (f->self_key != -1) drop(f->self_key);
    for (int i = 0; i < f->n_exclude; i++) drop(f->exclude[i]);
  }
  const uint64_t groups = f ? f->exclude_groups : 0;
  // scratch: qv | qw | bits | count | first | hdr | sel
  const size_t b_qv = ccm_align256((size_t)n * 8), b_qw = ccm_align256((size_t)n * 4), b_bits = ccm_align256((size_t)nbw * 4);
  const size_t b_cnt = ccm_align256((size_t)ns * 8), b_hdr = 32, b_sel = (size_t)ns * sizeof(KfdbSel);
  void* sc = nullptr;
  { int rc = ccm_scratch(ctx, b_qv + b_qw + b_bits + b_cnt + b_hdr + b_sel, &sc); if (rc) return rc; }
  char* p = (char*)sc;
  double* d_qv = (double*)p; int32_t* d_qw = (int32_t*)(p + b_qv); uint32_t* d_bits = (uint32_t*)(p + b_qv + b_qw);
  int32_t* d_count = (int32_t*)(p + b_qv + b_qw + b_bits); uint32_t* d_first = (uint32_t*)(d_count + ns);
  int32_t* d_hdr = (int32_t*)(p + b_qv + b_qw + b_bits + b_cnt); KfdbSel* d_sel = (KfdbSel*)((char*)d_hdr + b_hdr);
  const size_t b_in = b_qv + b_qw + (size_t)nbw * 4;
  const size_t b_rb = b_hdr + (size_t)std::min(ns, kFirstReadBack) * sizeof(KfdbSel);
  void* pin = nullptr;
  { int rc = ccm_pin_scratch(ctx, std::max(b_in, b_rb), &pin); if (rc) return rc; }
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(pin, value, (size_t)n * 8); std::memcpy((char*)pin + b_qv, word, (size_t)n * 4); std::memcpy((char*)pin + b_qv + b_qw, bits.data(), (size_t)nbw * 4);
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(d_qv, pin, b_in, hipMemcpyHostToDevice, ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, (size_t)ns * 8, ctx->stream));
  const int n_base_blocks = db->base_end ? kCountBaseBlocks : 0, n_log = ns - db->base_end;
  if (n_base_blocks + n_log)
    hipLaunchKernelGGL(kfdb_count_kernel, dim3(n_base_blocks + n_log), dim3(256), (size_t)(2 * n + 1) * 4, ctx->stream, d_qw, n, db->d_csr_off, db->d_csr_slot,
                       db->d_slot, db->d_word, db->base_end, n_base_blocks, d_bits, groups, d_count, d_first);
  hipLaunchKernelGGL(kfdb_select_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_count, d_first, ns, d_hdr, d_sel);
  hipLaunchKernelGGL(kfdb_score_kernel, dim3(std::min(ns, kScoreBlocks)), dim3(64), (size_t)n * 12, ctx->stream, d_qw, d_qv, n, db->d_slot, db->d_word, db->d_val,
                     d_sel, d_hdr, nullptr, 0, nullptr);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(pin, d_hdr, b_rb, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  int32_t hdr[4];
  std::memcpy(hdr, pin, sizeof hdr);
  const int n_sel = hdr[0];
  std::vector<KfdbSel> rows(n_sel);
  if (n_sel <= kFirstReadBack) {
    if (n_sel) std::memcpy(rows.data(), (char*)pin + b_hdr, (size_t)n_sel * sizeof(KfdbSel));
  } else {
    CCM_HIP_CHECK(ctx, hipMemcpyAsync(rows.data(), d_sel, (size_t)n_sel * sizeof(KfdbSel), hipMemcpyDeviceToHost, ctx->stream));
    CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  // lKFsSharingWords order: (r*, add order); first = nq - r*
  std::sort(rows.begin(), rows.end(), [&](const KfdbSel& a, const KfdbSel& b) {
    return a.first != b.first ? a.first > b.first : db->seq[a.slot] < db->seq[b.slot];
  });
  const int m = std::min(n_sel, cap);
  for (int i = 0; i < m; i++) {
    key_out[i] = db->key[rows[i].slot];
    count_out[i] = rows[i].count;
    score64_out[i] = rows[i].score;
    score_out[i] = (float)rows[i].score;   // float si = mpVoc->score(...) (Database.cpp:129)
  }
  *n_out = n_sel;
  if (n_sharing_out) *n_sharing_out = hdr[2];
  if (max_common_out) *max_common_out = hdr[1];
  return CCM_OK;
}

extern "C" int ccm_kfdb_score(ccm_kfdb* db, ccm_ctx* ctx, int n, const int32_t* word, const double* value, const int64_t* keys, int m, double* out) {
  { int rc = kfdb_ctx_ok(db, ctx, "ccm_kfdb_score"); if (rc) return rc; }
  if (m < 0 || (m && (!keys || !out)) || n > kMaxQueryWords) return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfdb_score: bad args (at most 4096 query words)");
  { int rc = check_words(ctx, db->n_words, n, word, value, "ccm_kfdb_score"); if (rc) return rc; }
  if (m == 0) return CCM_OK;
  std::shared_lock<std::shared_mutex> lk(db->mu);
  std::vector<int32_t> slots(m);
  for (int i = 0; i < m; i++) {
    auto it = db->live.find(keys[i]);
    if (it == db->live.end()) return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfdb_score: key not in the database");
    slots[i] = it->second;
  }
  const size_t b_qv = ccm_align256((size_t)n * 8), b_qw = ccm_align256((size_t)n * 4), b_sl = ccm_align256((size_t)m * 4);
  void* sc = nullptr;
  { int rc = ccm_scratch(ctx, b_qv + b_qw + b_sl + (size_t)m * 8, &sc); if (rc) return rc; }
  char* p = (char*)sc;
  double* d_qv = (double*)p; int32_t* d_qw = (int32_t*)(p + b_qv); int32_t* d_sl = (int32_t*)(p + b_qv + b_qw); double* d_out = (double*)(p + b_qv + b_qw + b_sl);
  void* pin = nullptr;
  { int rc = ccm_pin_scratch(ctx, std::max(b_qv + b_qw + (size_t)m * 4, (size_t)m * 8), &pin); if (rc) return rc; }
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (n) { std::memcpy(pin, value, (size_t)n * 8); std::memcpy((char*)pin + b_qv, word, (size_t)n * 4); }
  std::memcpy((char*)pin + b_qv + b_qw, slots.data(), (size_t)m * 4);
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(d_qv, pin, b_qv + b_qw + (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(kfdb_score_kernel, dim3(std::min(m, kScoreBlocks)), dim3(64), (size_t)n * 12, ctx->stream, d_qw, d_qv, n, db->d_slot, db->d_word, db->d_val,
                     nullptr, nullptr, d_sl, m, d_out);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(pin, d_out, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(out, pin, (size_t)m * 8);
  return CCM_OK;
}
