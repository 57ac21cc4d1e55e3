// bowsearch.hip — ORBmatcher::SearchByBoW(pKF1, pKF2, ...) (cslam/src/ORBmatcher.cpp:565-698) of ComputeSim3 for all candidates on keyframes of the keyframe store:
// ccm_bow_pair_eval_resident (include/ccm_hip.h).  The descriptors and the feature vectors are the store's (kfstore.hip, ccm_kfstore_set_featvec);
// the call uploads the slot pairs, the offsets and the mask bytes, launches ONE kernel and downloads the table and the counters (stage_blocks.h
// BowPairResidentBlock).  The lines are bow_search_math.h's; the wave's walk and the host stage are fv_pair.h's, and this file is the form they take here.
//
// A feature is a query, and a candidate counted and usable, when its live byte is set; a lane keeps nothing per query or candidate beyond the descriptor.  The key
// of a pair is (distance << 16 | list position).  The pass's best and second best are two butterfly minima, the second over the keys without the winner (keys are
// unique: the position bits); the holding lane merges them behind what the earlier passes left (bsm_merge: strict '<', so the first position keeps the index).
#include "fv_pair.h"

namespace {

using BowArgs = fvp::FvPairArgs<uint64_t>;

struct BowForm {
  using Args = BowArgs;
  using Best = BowBest;
  struct Query {};
  struct Cand {};
  __device__ BowForm(const Args&, const int32_t*, size_t, size_t) {}
  static __device__ bool is_query(uint8_t live) { return live != 0; }
  static __device__ bool is_counted(uint8_t live) { return live != 0; }
  __device__ Query query(bool, int) const { return {}; }
  static __device__ Query lane_read(Query, int) { return {}; }
  __device__ bool candidate(bool live, int, Cand&) const { return live; }
  static __device__ uint32_t key(int d, uint32_t pos, Query, Cand) { return (uint32_t)d << 16 | pos; }
  static __device__ void reduce(uint32_t key, int my_idx2, int pos0, bool holds, Best& part) {
    const uint32_t m1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lanex::wave_min_u32(key));   // below kNoKey: the pass has a live candidate
    const uint32_t m2 = lanex::wave_min_u32(key == m1 ? fvp::kNoKey : key);
    Best r;
    r.d1 = (int)(m1 >> 16);
    r.d2 = m2 == fvp::kNoKey ? BSM_NONE : (int)(m2 >> 16);
    // a candidate at distance 256 is no best candidate (:631 is a strict '<' against 256)
    r.idx = r.d1 < BSM_NONE ? __builtin_amdgcn_readlane(my_idx2, (int)(m1 & 0xFFFFu) - pos0) : -1;
    if (holds) part = bsm_merge(part, r);
  }
  static __device__ Best empty() { return bsm_empty(); }
  __device__ uint64_t word(bool, const Best& part, uint32_t cands, int nb) const { return bsm_pack(cands ? BSM_EVALUATED : BSM_NO_CANDIDATE, part, nb); }
  __device__ void add_counters(const Args&, int) const {}
};

__global__ __launch_bounds__(fvp::kThreads) void bow_pair_kernel(BowArgs a) { fvp::fv_pair_wave<BowForm>(a); }

}  // namespace

extern "C" int ccm_bow_pair_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int J, const int64_t* key1, const int64_t* key2, const int32_t* live1_off, const uint8_t* live1,
                                          const int32_t* live2_off, const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  if (!ctx) return CCM_E_ARG;
  using B = BowPairResidentBlock;
  const fvp::FvPairCall<B> c = {"ccm_bow_pair_eval_resident: ", "bow", "bow_pair", nullptr, nullptr, J, key1, key2, live1_off, live1, &B::live1, live2_off, live2, &B::live2,
                                table, n_query, n_dist, nullptr, nullptr};
  return fvp::fv_pair_stage(ctx, st, c, bow_pair_kernel, 0, [](const B&) {}, [](const B&, BowArgs&) {});
}
