// kfingest.hip — ccm_kfstore_ingest: the M keyframes of a message into free slots of the keyframe store with their grid, their DBoW2 BowVector and
// FeatureVector built on the device, in one staged upload (stage_blocks.h KfIngestBlock: what ccm_kfstore_add carries, the descriptors once), three launches on the
// caller's stream and one download.  What KeyFrame::KeyFrame(ccmslam_msgs::KF*) and ProcessAfterLoad do per keyframe through ComputeBoW and AssignFeaturesToGrid.
//   1  kfstore_add_kernel<true> (kfstore.hip) as it is: the slot copy and the grid.
//   2  kfi_descend_kernel: one wave per feature of the call descends the vocabulary tree (vocab.h, bow_descend_kernel's rule) on the staged descriptors and leaves
//      the feature's word, weight and node at level L - levelsup.
//   3  kfi_vectors_kernel: one workgroup per keyframe.  The kept features' (word, feature) and (node, feature) keys (kfingest_math.h kfi_key) go into LDS, a
//      dropped feature's place holds a key behind all others, and a bitonic network orders both arrays in the same passes; the keys are unique, so the order is
//      the one of the reference's maps.  A packed workgroup scan over the run heads numbers the distinct words and nodes.  The lane of a word's head adds the
//      word's run in feature order (addWeight), one lane adds the norm in word order (normalize), all lanes divide (an IEEE f64 division).  The node heads give
//      fv_node / fv_off, the sorted node keys fv_idx, written to the slot (layout of kfstore.h, as ccm_kfstore_set_featvec leaves it) and to the call's outputs.
// No float atomics, no comparison sort in global memory, nothing waits on another workgroup; every loop is bounded by a count validated on the host (a keyframe's
// features <= KFI_MAX_FEAT, the tree's nodes).
#include "kfstore.h"
#include "kfingest_math.h"
#include "stage_blocks.h"
#include "vocab.h"

#include <algorithm>

namespace {

constexpr int kWave = 64, kVecThreads = 256, kVecWaves = kVecThreads / kWave;

struct KfiArgs {
  int stride, n_nodes, nid_level, F;
  const int32_t *slot, *feat_off;
  const uint32_t* desc;
  // the vocabulary's
  const int32_t *child_off, *child_id, *word_id;
  const uint32_t* node_desc;
  const double* node_weight;
  // per feature of the call
  int32_t *feat_word, *feat_node;
  double* feat_weight;
  // outputs
  int32_t *bow_n, *bow_word, *fv_nn, *fv_node, *fv_off, *fv_idx;
  double* bow_value;
  // the store's
  int32_t *s_fv_node, *s_fv_off;
  uint16_t* s_fv_idx;
};

__global__ __launch_bounds__(256) void kfi_descend_kernel(KfiArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int f = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave);
  if (f >= a.F) return;
  uint32_t d[8];
  {
    const uint32_t* dp = a.desc + (size_t)f * 8;   // wave-uniform
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = dp[k];
  }
  int nid;
  const int leaf = vocab_descend_wave(d, lane, a.child_off, a.child_id, a.node_desc, a.n_nodes, a.nid_level, &nid);
  if (lane == 0) { a.feat_word[f] = a.word_id[leaf]; a.feat_weight[f] = a.node_weight[leaf]; a.feat_node[f] = nid; }
}

// workgroup m: keyframe m of the call, n <= P features.
template <int P>
__global__ __launch_bounds__(kVecThreads) void kfi_vectors_kernel(KfiArgs a) {
  __shared__ uint64_t wk[P], nk[P];   // (word, feature) and (node, feature), ascending after the sort, the kept ones first
  __shared__ double wl[P], val[P];    // the features' weights; the words' values
  __shared__ int scan_lds[kVecWaves], s_kept;
  __shared__ double s_norm;
  const int m = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const int s = a.slot[m];
  const int32_t f0 = a.feat_off[m], n = a.feat_off[m + 1] - f0;
  if (n > P) return;   // never: the host picks P by the call's largest keyframe (workgroup-uniform, ahead of every barrier)
  int Pn = 1;
  while (Pn < n) Pn <<= 1;
  for (int i = t; i < Pn; i += kVecThreads) {
    uint64_t kw = KFI_NO_KEY, kn = KFI_NO_KEY;
    if (i < n) {
      const double wt = a.feat_weight[f0 + i];
      wl[i] = wt;
      if (kfi_kept(wt)) { kw = kfi_key(a.feat_word[f0 + i], i); kn = kfi_key(a.feat_node[f0 + i], i); }
    }
    wk[i] = kw; nk[i] = kn;
  }
  if (t == 0) s_kept = 0;
  __syncthreads();
  // the bitonic network over Pn places, both arrays in the same passes
  for (int k = 2; k <= Pn; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (Pn >> 1); p += kVecThreads) {
        const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const uint64_t x = wk[lo], y = wk[hi];
        if ((x > y) == up) { wk[lo] = y; wk[hi] = x; }
        const uint64_t u = nk[lo], v = nk[hi];
        if ((u > v) == up) { nk[lo] = v; nk[hi] = u; }
      }
      __syncthreads();
    }
  for (int i = t; i < Pn; i += kVecThreads)
    if (wk[i] != KFI_NO_KEY && (i + 1 == Pn || wk[i + 1] == KFI_NO_KEY)) s_kept = i + 1;   // the last kept place: one lane at most
  __syncthreads();
  const int kept = s_kept;
  // run heads, the words' in the low half and the nodes' in the high half of one int (each at most 4096); thread t takes the places [c0, c1)
  const int per = max(1, Pn / kVecThreads);
  const int c0 = min(t * per, kept), c1 = min(c0 + per, kept);
  int sum = 0;
  for (int i = c0; i < c1; i++) {
    sum += (i == 0 || kfi_key_id(wk[i]) != kfi_key_id(wk[i - 1])) ? 1 : 0;
    sum += (i == 0 || kfi_key_id(nk[i]) != kfi_key_id(nk[i - 1])) ? 1 << 16 : 0;
  }
  int x = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) scan_lds[w] = x;
  __syncthreads();
  int run = x - sum, total = 0;
  for (int v = 0; v < kVecWaves; v++) {
    if (v < w) run += scan_lds[v];
    total += scan_lds[v];
  }
  const int nw = total & 0xFFFF, nn = total >> 16;
  int rw = run & 0xFFFF, rn = run >> 16;
  const size_t g0 = (size_t)s * (size_t)a.stride;
  int32_t *o_word = a.bow_word + f0, *o_node = a.fv_node + f0, *o_off = a.fv_off + f0 + m, *o_idx = a.fv_idx + f0;
  double* o_value = a.bow_value + f0;
  int32_t *s_node = a.s_fv_node + g0, *s_off = a.s_fv_off + g0 + (size_t)s;
  uint16_t* s_idx = a.s_fv_idx + g0;
  for (int i = c0; i < c1; i++) {
    const uint64_t kw = wk[i], kn = nk[i];
    if (i == 0 || kfi_key_id(kw) != kfi_key_id(wk[i - 1])) {
      // addWeight: the first occurrence's weight, then += w per further occurrence in feature order
      const int32_t id = kfi_key_id(kw);
      double acc = wl[kfi_key_feat(kw)];
      for (int j = i + 1; j < kept && kfi_key_id(wk[j]) == id; j++) acc += wl[kfi_key_feat(wk[j])];
      o_word[rw] = id; val[rw] = acc; rw++;
    }
    if (i == 0 || kfi_key_id(kn) != kfi_key_id(nk[i - 1])) {
      o_node[rn] = kfi_key_id(kn); o_off[rn] = i;
      s_node[rn] = kfi_key_id(kn); s_off[rn] = i;
      rn++;
    }
    o_idx[i] = kfi_key_feat(kn); s_idx[i] = (uint16_t)kfi_key_feat(kn);
  }
  if (t == 0) { a.bow_n[m] = nw; a.fv_nn[m] = nn; o_off[nn] = kept; s_off[nn] = kept; }
  __syncthreads();
  if (t == 0) {   // normalize: the sum of fabs in ascending word id, one after the other
    double norm = 0.0;
    for (int r = 0; r < nw; r++) norm += fabs(val[r]);
    s_norm = norm;
  }
  __syncthreads();
  const double norm = s_norm;
  // what lies behind the counts goes out as zeros, so that the outputs are a function of the inputs
  for (int r = t; r < n; r += kVecThreads) {
    if (r < nw) o_value[r] = norm > 0.0 ? val[r] / norm : val[r];
    else { o_value[r] = 0.0; o_word[r] = 0; }
    if (r >= nn) { o_node[r] = 0; o_off[r + 1] = 0; }
    if (r >= kept) o_idx[r] = 0;
  }
}

}  // namespace

extern "C" int ccm_kfstore_ingest(ccm_kfstore* st, ccm_ctx* ctx, const ccm_vocab* voc, int levelsup, int M, const int64_t* keys, const float* kf_rec,
                                  const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave, const uint8_t* feat_desc, int32_t* bow_n, int32_t* bow_word,
                                  double* bow_value, int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node) {
  if (int rc = kfstore_ctx_ok(st, ctx, "ccm_kfstore_ingest")) return rc;
  const char* const me = "ccm_kfstore_ingest: ";
  if (!voc) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "NULL vocabulary");
  if (voc->ctx->device != st->device) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "the vocabulary is on another device than the store");
  if (M > 0 && !keys) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "null pointers");
  if (const char* why = kfi_check_ingest(M, st->max_feat, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx))
    return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + why);
  if ((feat_word == nullptr) != (feat_node == nullptr)) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "feat_word and feat_node are both NULL or both given");
  if (M == 0) return CCM_OK;
  std::unique_lock<std::shared_mutex> lk(st->mu);
  if (int rc = kfstore_keys_ok(st, ctx, me, M, keys)) return rc;
  const size_t F = (size_t)feat_off[M];
  int max_n = 0;
  for (int m = 0; m < M; m++) max_n = std::max(max_n, feat_off[m + 1] - feat_off[m]);
  const bool want_feat = feat_word != nullptr;
  KfIngestBlock b((size_t)M, F, want_feat);
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  b.put(b.desc, feat_desc); b.put(b.feat_off, feat_off); b.put(b.rec, kf_rec); b.put(b.xy, feat_xy); b.put(b.oct, feat_octave);
  int32_t* h_slot = b.up(b.slot);
  for (int m = 0; m < M; m++) h_slot[m] = st->free_slots[st->free_slots.size() - 1 - (size_t)m];
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  KfAddArgs g = {};
  g.stride = st->stride;
  g.slot = b.dev(b.slot); g.feat_off = b.dev(b.feat_off); g.rec_in = b.dev(b.rec); g.xy_in = b.dev(b.xy); g.oct_in = b.dev(b.oct); g.desc_in = b.dev(b.desc);
  g.rec = st->d_rec; g.xy = st->d_xy; g.n = st->d_n; g.n_in = st->d_n_in; g.cell_off = st->d_cell_off; g.n_in_out = b.dev(b.n_in);
  g.cell_idx = st->d_cell_idx; g.oct = st->d_oct; g.desc = st->d_desc;
  kfstore_launch_add_build(ctx, g, M);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  KfiArgs a = {};
  a.stride = st->stride; a.n_nodes = voc->n_nodes; a.nid_level = voc->L - levelsup; a.F = (int)F;
  a.slot = b.dev(b.slot); a.feat_off = b.dev(b.feat_off); a.desc = (const uint32_t*)b.dev(b.desc);
  a.child_off = voc->d_child_off; a.child_id = voc->d_child_id; a.word_id = voc->d_word_id; a.node_desc = voc->d_node_desc; a.node_weight = voc->d_weight;
  a.feat_word = want_feat ? b.dev(b.feat_word) : b.dev(b.work_word); a.feat_node = want_feat ? b.dev(b.feat_node) : b.dev(b.work_node);
  a.feat_weight = b.dev(b.weight);
  a.bow_n = b.dev(b.bow_n); a.bow_word = b.dev(b.bow_word); a.fv_nn = b.dev(b.fv_nn); a.fv_node = b.dev(b.fv_node); a.fv_off = b.dev(b.fv_off); a.fv_idx = b.dev(b.fv_idx);
  a.bow_value = b.dev(b.bow_value);
  a.s_fv_node = st->d_fv_node; a.s_fv_off = st->d_fv_off; a.s_fv_idx = st->d_fv_idx;
  if (F) {
    hipLaunchKernelGGL(kfi_descend_kernel, dim3((unsigned)ccm_div_up((int64_t)F, 4)), dim3(256), 0, ctx->stream, a);
    CCM_HIP_CHECK(ctx, hipGetLastError());
  }
  if (max_n <= 1024) hipLaunchKernelGGL(kfi_vectors_kernel<1024>, dim3((unsigned)M), dim3(kVecThreads), 0, ctx->stream, a);
  else hipLaunchKernelGGL(kfi_vectors_kernel<KFI_MAX_FEAT>, dim3((unsigned)M), dim3(kVecThreads), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;   // synchronises: the slots are written when the keys become live
  b.get(b.bow_n, bow_n); b.get(b.bow_word, bow_word); b.get(b.bow_value, bow_value);
  b.get(b.fv_nn, fv_nn); b.get(b.fv_node, fv_node); b.get(b.fv_off, fv_off); b.get(b.fv_idx, fv_idx);
  if (want_feat) { b.get(b.feat_word, feat_word); b.get(b.feat_node, feat_node); }
  for (int m = 0; m < M; m++) {   // as add followed by set_featvec leave the slot
    const size_t s = (size_t)st->free_slots.back();
    st->h_n[s] = feat_off[m + 1] - feat_off[m];
    st->h_fv_nn[s] = fv_nn[m];
    st->live[keys[m]] = (int)s; st->free_slots.pop_back();
  }
  return CCM_OK;
}
