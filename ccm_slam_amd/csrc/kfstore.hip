// kfstore.hip — the keyframe feature store: what ORBmatcher::Fuse reads of a keyframe and no Fuse call changes (the 10-float record, mvKeysUn, the octaves, the
// descriptors and mGrid as a CSR), kept on the device for the map's life, so that the two batched Fuse stages (fuse.hip, ccm_fuse_*_eval_resident) upload the
// poses and the points alone.  The second piece of per-keyframe state on the device beside the BoW database (kfdb.hip), with the same handle idiom.
//
// Layout (one ccm_kfstore handle): a fixed number of slots, one per keyframe, each field an array indexed by slot with a stride of `stride`
// features (max_feat rounded up to 16, so that every slot's descriptors, xy, octaves and 16-bit cell_idx start on 16 bytes).  The host keeps key -> slot and a
// stack of free slots; nothing grows.
//
// ccm_kfstore_add is one staged upload (stage_blocks.h KfstoreAddBlock) and one launch of kfstore_add_kernel, one workgroup of four waves per keyframe: it copies
// the keyframe into its slot and either copies the caller's grid or builds it by KeyFrame::AssignFeaturesToGrid (kfstore_math.h kfg_cell_of):
//   count    each wave owns a contiguous quarter of the features and counts them into its own LDS histogram over the 3 600 cells (integer LDS atomics);
//   scan     a workgroup scan over the cells gives cell_off and, in place of the counts, each wave's cursor per cell: the waves' quarters ascend, so wave w's
//            features of a cell follow those of the waves below it;
//   scatter  each wave walks its quarter in chunks of 64, in order; inside a chunk the lanes of equal cell are ranked by lane index with a ballot loop over the
//            distinct cells present (at most 64 rounds), and the cell's first lane moves the cursor on.  The indices of a cell therefore ascend: the reference's
//            push_back order, on which fsm_window_best's tie-break rests.
// No comparison sort, no float atomics, nothing waits on another workgroup, every loop is bounded by a count validated on the host.
//
// ccm_kfstore_set_featvec gives a live key its DBoW2::FeatureVector: the flat arrays are validated (bow_search_math.h bsm_check_featvec) and copied
// into the slot as they are, the indices in 16 bits; nothing is sorted or built.  A slot's vector goes with its tenant: add, erase and clear mark it absent.
//
// ccm_kfstore_ingest (kfingest.hip) does add without a grid and set_featvec for the keyframes of a message in one call, the vector built on the
// device; it launches kfstore_add_kernel<true> through kfstore_launch_add_build (kfstore.h).
#include "kfstore.h"
#include "bow_search_math.h"
#include "stage_blocks.h"

#include <algorithm>

namespace {

constexpr int kAddThreads = 256, kAddWaves = kAddThreads / 64;
constexpr int kCellsPerThread = (FSM_CELLS + kAddThreads - 1) / kAddThreads;   // 15

// workgroup m: keyframe m of the call into slot[m].  kBuild: the grid is built here; otherwise it is the caller's, validated on the host.
template <bool kBuild>
__global__ __launch_bounds__(kAddThreads) void kfstore_add_kernel(KfAddArgs a) {
  const int m = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int s = a.slot[m];
  const int32_t f0 = a.feat_off[m], n = a.feat_off[m + 1] - f0;
  const size_t g0 = (size_t)s * (size_t)a.stride;
  const float* xy_in = a.xy_in + 2 * (size_t)f0;
  float* rec = a.rec + (size_t)s * FSM_REC_FLOATS;
  int32_t* cell_off = a.cell_off + (size_t)s * (FSM_CELLS + 1);
  uint16_t* cell_idx = a.cell_idx + g0;
  // the keyframe's own arrays into the slot; the descriptors 16 bytes at a time (both sides lie on 16 bytes)
  if (t < FSM_REC_FLOATS) rec[t] = a.rec_in[(size_t)m * FSM_REC_FLOATS + t];
  for (int i = t; i < 2 * n; i += kAddThreads) a.xy[2 * g0 + i] = xy_in[i];
  for (int i = t; i < n; i += kAddThreads) a.oct[g0 + i] = a.oct_in[f0 + i];
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.desc_in + 32 * (size_t)f0);
    uint4* dst = reinterpret_cast<uint4*>(a.desc + 32 * g0);
    for (int i = t; i < 2 * n; i += kAddThreads) dst[i] = src[i];
  }
  if (!kBuild) {
    const int32_t* co = a.cell_off_in + (size_t)m * (FSM_CELLS + 1);
    const int32_t n_in = co[FSM_CELLS];   // <= n
    for (int i = t; i <= FSM_CELLS; i += kAddThreads) cell_off[i] = co[i];
    for (int i = t; i < n_in; i += kAddThreads) cell_idx[i] = a.cell_idx_in[f0 + i];
    if (t == 0) { a.n[s] = n; a.n_in[s] = n_in; a.n_in_out[m] = n_in; }
    return;
  }
  __shared__ int32_t hist[kAddWaves][FSM_CELLS];   // counts, then cursors
  __shared__ int scan_lds[kAddWaves];
  const float* krec = a.rec_in + (size_t)m * FSM_REC_FLOATS;   // workgroup-uniform: the bounds and the inverses come through the scalar unit
  for (int i = t; i < kAddWaves * FSM_CELLS; i += kAddThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
  // the wave's quarter: [q0, q1), walked in `chunks` chunks of 64 (the same number for every wave, so that the barriers below are met by all)
  const int per = (n + kAddWaves - 1) / kAddWaves;
  const int q0 = min(w * per, n), q1 = min(q0 + per, n);
  const int chunks = (per + 63) / 64;
  for (int c = 0; c < chunks; c++) {
    const int f = q0 + c * 64 + lane;
    int cell;
    if (f < q1 && kfg_cell_of(krec, xy_in[2 * f], xy_in[2 * f + 1], &cell)) atomicAdd(&hist[w][cell], 1);
  }
  __syncthreads();
  // scan: thread t takes the cells [c0, c1)
  {
    const int c0 = min(t * kCellsPerThread, FSM_CELLS), c1 = min(c0 + kCellsPerThread, FSM_CELLS);
    int sum = 0;
    for (int c = c0; c < c1; c++)
      for (int v = 0; v < kAddWaves; v++) sum += hist[v][c];
    // exclusive prefix of sum over the workgroup
    int x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) scan_lds[w] = x;
    __syncthreads();
    int run = x - sum, total = 0;
    for (int v = 0; v < kAddWaves; v++) {
      if (v < w) run += scan_lds[v];
      total += scan_lds[v];
    }
    for (int c = c0; c < c1; c++) {
      cell_off[c] = run;
      for (int v = 0; v < kAddWaves; v++) { const int cnt = hist[v][c]; hist[v][c] = run; run += cnt; }
    }
    if (t == 0) { cell_off[FSM_CELLS] = total; a.n[s] = n; a.n_in[s] = total; a.n_in_out[m] = total; }
  }
  __syncthreads();
  // scatter
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c = 0; c < chunks; c++) {
    const int f = q0 + c * 64 + lane;
    int cell = -1;
    const bool in = f < q1 && kfg_cell_of(krec, xy_in[2 * f], xy_in[2 * f + 1], &cell);
    int rank = 0, cnt = 0;
    bool first = false;
    unsigned long long todo = __ballot(in);
    while (todo) {   // one round per distinct cell among the chunk's lanes
      const int lead = __ffsll((long long)todo) - 1;
      const int lc = __shfl(cell, lead, 64);
      const unsigned long long same = __ballot(in && cell == lc);
      if (in && cell == lc) { rank = (int)__popcll(same & below); cnt = (int)__popcll(same); first = lane == lead; }
      todo &= ~same;
    }
    const int cur = in ? hist[w][cell] : 0;
    __syncthreads();   // every lane has read its cursor before the cell's first lane moves it
    if (in) {
      cell_idx[cur + rank] = (uint16_t)f;
      if (first) hist[w][cell] = cur + cnt;
    }
    __syncthreads();
  }
}

}  // namespace

void kfstore_launch_add_build(ccm_ctx* ctx, const KfAddArgs& a, int M) {
  hipLaunchKernelGGL(kfstore_add_kernel<true>, dim3((unsigned)M), dim3(kAddThreads), 0, ctx->stream, a);
}

extern "C" int ccm_kfstore_create(ccm_ctx* ctx, int max_kf, int max_feat, ccm_kfstore** out) {
  if (!ctx) return CCM_E_ARG;
  const int stride = kfg_stride(max_feat);
  if (!out || max_kf < 1 || !stride || (int64_t)max_kf * (int64_t)stride > (int64_t)INT32_MAX)
    return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfstore_create: bad args (max_feat 1 .. 65535, max_kf * max_feat <= INT32_MAX)");
  CCM_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ccm_kfstore* st = new ccm_kfstore();
  st->device = ctx->device; st->max_kf = max_kf; st->max_feat = max_feat; st->stride = stride;
  const size_t K = (size_t)max_kf, G = K * (size_t)stride;
  const bool ok = hipMalloc(&st->d_rec, K * FSM_REC_FLOATS * 4) == hipSuccess && hipMalloc(&st->d_n, K * 4) == hipSuccess && hipMalloc(&st->d_n_in, K * 4) == hipSuccess &&
                  hipMalloc(&st->d_cell_off, K * (FSM_CELLS + 1) * 4) == hipSuccess && hipMalloc(&st->d_cell_idx, G * 2) == hipSuccess &&
                  hipMalloc(&st->d_xy, G * 8) == hipSuccess && hipMalloc(&st->d_oct, G) == hipSuccess && hipMalloc(&st->d_desc, G * 32) == hipSuccess &&
                  hipMalloc(&st->d_fv_node, G * 4) == hipSuccess && hipMalloc(&st->d_fv_off, (G + K) * 4) == hipSuccess && hipMalloc(&st->d_fv_idx, G * 2) == hipSuccess &&
                  hipMemsetAsync(st->d_n, 0, K * 4, ctx->stream) == hipSuccess && hipMemsetAsync(st->d_n_in, 0, K * 4, ctx->stream) == hipSuccess &&
                  hipMemsetAsync(st->d_cell_off, 0, K * (FSM_CELLS + 1) * 4, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    ccm_kfstore_destroy(st);
    return ccm_set_error(ctx, CCM_E_HIP, "ccm_kfstore_create: device allocation failed");
  }
  st->free_slots.resize(K);
  st->h_n.assign(K, 0);
  st->h_fv_nn.assign(K, -1);
  for (int s = 0; s < max_kf; s++) st->free_slots[s] = max_kf - 1 - s;   // slot 0 is taken first
  *out = st;
  return CCM_OK;
}

extern "C" void ccm_kfstore_destroy(ccm_kfstore* st) {
  if (!st) return;
  hipSetDevice(st->device);
  hipFree(st->d_rec); hipFree(st->d_n); hipFree(st->d_n_in); hipFree(st->d_cell_off); hipFree(st->d_cell_idx); hipFree(st->d_xy); hipFree(st->d_oct); hipFree(st->d_desc);
  hipFree(st->d_fv_node); hipFree(st->d_fv_off); hipFree(st->d_fv_idx);
  delete st;
}

extern "C" int ccm_kfstore_add(ccm_kfstore* st, ccm_ctx* ctx, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
                               const uint8_t* feat_octave, const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_add")) return rc;
  const char* const me = "ccm_kfstore_add: ";
  if (M > 0 && !keys) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "null pointers");
  if (const char* why = kfg_check_add(M, st->max_feat, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx))
    return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  if (M == 0) return CCM_OK;
  std::unique_lock<std::shared_mutex> lk(st->mu);
  if (int rc = kfstore_keys_ok(st, ctx, me, M, keys)) return rc;
  const size_t F = (size_t)feat_off[M];
  const bool grid = cell_off != nullptr;
  KfstoreAddBlock b((size_t)M, F, grid);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  b.put(b.desc, feat_desc); b.put(b.feat_off, feat_off); b.put(b.rec, kf_rec); b.put(b.xy, feat_xy); b.put(b.oct, feat_octave);
  int32_t* h_slot = b.up(b.slot);
  for (int m = 0; m < M; m++) h_slot[m] = st->free_slots[st->free_slots.size() - 1 - (size_t)m];
  if (grid) {
    b.put(b.cell_off, cell_off);
    uint16_t* h_idx = b.up(b.cell_idx);
    std::memset(h_idx, 0, F * sizeof(uint16_t));
    for (int m = 0; m < M; m++) {
      const int32_t n_in = cell_off[(size_t)m * (FSM_CELLS + 1) + FSM_CELLS];
      for (int32_t j = 0; j < n_in; j++) h_idx[feat_off[m] + j] = (uint16_t)cell_idx[feat_off[m] + j];
    }
  }
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  KfAddArgs a = {};
  a.stride = st->stride;
  a.slot = b.dev(b.slot); a.feat_off = b.dev(b.feat_off); a.cell_off_in = b.dev(b.cell_off); a.rec_in = b.dev(b.rec); a.xy_in = b.dev(b.xy);
  a.cell_idx_in = b.dev(b.cell_idx); a.oct_in = b.dev(b.oct); a.desc_in = b.dev(b.desc);
  a.rec = st->d_rec; a.xy = st->d_xy; a.n = st->d_n; a.n_in = st->d_n_in; a.cell_off = st->d_cell_off; a.n_in_out = b.dev(b.n_in);
  a.cell_idx = st->d_cell_idx; a.oct = st->d_oct; a.desc = st->d_desc;
  if (grid) hipLaunchKernelGGL(kfstore_add_kernel<false>, dim3((unsigned)M), dim3(kAddThreads), 0, ctx->stream, a);
  else kfstore_launch_add_build(ctx, a, M);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;   // synchronises: the slots are written when the keys become live
  for (int m = 0; m < M; m++) {
    st->h_n[(size_t)st->free_slots.back()] = feat_off[m + 1] - feat_off[m];
    st->h_fv_nn[(size_t)st->free_slots.back()] = -1;   // the previous tenant's vector is not the new one's
    st->live[keys[m]] = st->free_slots.back(); st->free_slots.pop_back();
  }
  return CCM_OK;
}

extern "C" int ccm_kfstore_set_featvec(ccm_kfstore* st, ccm_ctx* ctx, int64_t key, int nn, const int32_t* node, const int32_t* off, const int32_t* idx) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_set_featvec")) return rc;
  const char* const me = "ccm_kfstore_set_featvec: ";
  std::unique_lock<std::shared_mutex> lk(st->mu);   // add's lock: no resident evaluator reads the slot meanwhile
  auto it = st->live.find(key);
  if (it == st->live.end()) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "key not in the store");
  const size_t s = (size_t)it->second;
  const int n = st->h_n[s];
  std::vector<uint8_t> seen((size_t)n + 1);
  if (const char* why = bsm_check_featvec(n, nn, node, off, idx, seen.data())) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  if (nn > 0) {
    // pinned: node[nn] | off[nn + 1] | idx[off[nn]] (16-bit), then one copy per array into the slot
    const size_t L = (size_t)off[nn], b_off = (size_t)nn * 4, b_idx = b_off + ((size_t)nn + 1) * 4;
    void* pin = nullptr;
    if (int rc = ccm_pin_scratch(ctx, b_idx + L * 2, &pin)) return rc;
    CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // the block may still feed an earlier copy
    char* p = (char*)pin;
    std::memcpy(p, node, (size_t)nn * 4);
    std::memcpy(p + b_off, off, ((size_t)nn + 1) * 4);
    uint16_t* h_idx = (uint16_t*)(p + b_idx);
    for (size_t i = 0; i < L; i++) h_idx[i] = (uint16_t)idx[i];
    const size_t g0 = s * (size_t)st->stride;
    st->h_fv_nn[s] = -1;   // a copy that fails leaves the key without a vector, not with half of one
    CCM_HIP_CHECK(ctx, hipMemcpyAsync(st->d_fv_node + g0, p, (size_t)nn * 4, hipMemcpyHostToDevice, ctx->stream));
    CCM_HIP_CHECK(ctx, hipMemcpyAsync(st->d_fv_off + g0 + s, p + b_off, ((size_t)nn + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    CCM_HIP_CHECK(ctx, hipMemcpyAsync(st->d_fv_idx + g0, p + b_idx, L * 2, hipMemcpyHostToDevice, ctx->stream));
    CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  st->h_fv_nn[s] = nn;
  return CCM_OK;
}

extern "C" int ccm_kfstore_erase(ccm_kfstore* st, ccm_ctx* ctx, int64_t key) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_erase")) return rc;
  std::unique_lock<std::shared_mutex> lk(st->mu);   // waits for the resident evaluators that read the slot
  auto it = st->live.find(key);
  if (it == st->live.end()) return CCM_OK;
  st->free_slots.push_back(it->second);
  st->h_fv_nn[(size_t)it->second] = -1;
  st->live.erase(it);
  return CCM_OK;
}

extern "C" int ccm_kfstore_clear(ccm_kfstore* st, ccm_ctx* ctx) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_clear")) return rc;
  std::unique_lock<std::shared_mutex> lk(st->mu);
  st->live.clear();
  st->h_fv_nn.assign((size_t)st->max_kf, -1);
  st->free_slots.resize((size_t)st->max_kf);
  for (int s = 0; s < st->max_kf; s++) st->free_slots[s] = st->max_kf - 1 - s;
  return CCM_OK;
}

extern "C" int ccm_kfstore_count(ccm_kfstore* st, int* live, int* free_slots) {
  if (!st) return CCM_E_ARG;
  std::shared_lock<std::shared_mutex> lk(st->mu);
  if (live) *live = (int)st->live.size();
  if (free_slots) *free_slots = (int)st->free_slots.size();
  return CCM_OK;
}

extern "C" int ccm_kfstore_get(ccm_kfstore* st, ccm_ctx* ctx, int64_t key, int* n, int* n_in, int32_t* cell_off, int32_t* cell_idx) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_get")) return rc;
  std::shared_lock<std::shared_mutex> lk(st->mu);
  auto it = st->live.find(key);
  if (it == st->live.end()) return ccm_set_error(ctx, CCM_E_ARG, "ccm_kfstore_get: key not in the store");
  const size_t s = (size_t)it->second;
  // pinned: n | n_in | cell_off[FSM_CELLS + 1] | cell_idx[stride] (16-bit)
  const size_t b_off = 8, b_idx = b_off + (FSM_CELLS + 1) * 4;
  void* pin = nullptr;
  if (int rc = ccm_pin_scratch(ctx, b_idx + (size_t)st->stride * 2, &pin)) return rc;
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // the block may still feed an earlier copy
  char* p = (char*)pin;
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(p, st->d_n + s, 4, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(p + 4, st->d_n_in + s, 4, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(p + b_off, st->d_cell_off + s * (FSM_CELLS + 1), (FSM_CELLS + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipMemcpyAsync(p + b_idx, st->d_cell_idx + s * (size_t)st->stride, (size_t)st->stride * 2, hipMemcpyDeviceToHost, ctx->stream));
  CCM_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  int32_t nn[2];
  std::memcpy(nn, p, 8);
  if (nn[0] < 0 || nn[0] > st->max_feat || nn[1] < 0 || nn[1] > nn[0]) return ccm_set_error(ctx, CCM_E_STATE, "ccm_kfstore_get: the slot's counts are not a keyframe's");
  if (n) *n = nn[0];
  if (n_in) *n_in = nn[1];
  if (cell_off) std::memcpy(cell_off, p + b_off, (FSM_CELLS + 1) * 4);
  if (cell_idx) {
    const uint16_t* h = (const uint16_t*)(p + b_idx);
    for (int32_t j = 0; j < nn[1]; j++) cell_idx[j] = h[j];
  }
  return CCM_OK;
}
