// trisearch.hip — ORBmatcher::SearchForTriangulation (cslam/src/ORBmatcher.cpp:700-852) of LocalMapping::CreateNewMapPoints for all neighbours on keyframes of the
// keyframe store: ccm_tri_search_eval_resident (include/ccm_hip.h).  Descriptors, mvKeysUn, octaves and feature vectors are the store's; the call uploads
// the slot pairs, the offsets, 11 floats per job, the level tables and the map-point bytes, launches ONE kernel and downloads one 32-bit word per feature of every
// job's keyframe 1 and three counters per job (stage_blocks.h TriSearchResidentBlock).  The lines are tri_search_math.h's; the wave's walk and the host stage are
// fv_pair.h's, and this file is the form they take here.
//
// A feature is a query, and a candidate counted, when it has no map point.  The holding lane keeps its query's epipolar line (a, b, c, den of :162-168, computed
// once), which reaches the wave by four lane reads.  Per pass a lane keeps its candidate's keypoint and line threshold; the candidate is usable when its octave is one
// of the tables' and it lies outside the epipole's radius, a gate that does not depend on the query and runs once per pass.  The line gate (one correctly rounded
// f32 division, one comparison in double) runs only in lanes whose distance is at most TH_LOW.  The pass's winner is ONE butterfly minimum of the key
// (distance << 16 | 0xFFFF - list position): the smallest distance, and among equals the LARGEST position, as :770's `dist > bestDist` leaves it; a lane whose
// candidate fails any test holds the no-key value.  The holding lane merges with '<=' (tsm_merge), so a later pass wins ties.
#include "fv_pair.h"

namespace {

struct TriArgs : fvp::FvPairArgs<uint32_t> {
  int nlevels;              // the levels of the two tables
  const float *epi, *sf;    // TSM_EPI_FLOATS per job; scale_factors[nlevels]
  const double* thr;        // 3.84 * (double)level_sigma2[l]
  const uint8_t* oct;       // the store's
  const float* xy;
  uint32_t* n_match;
};

__device__ __forceinline__ float lane_read(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

struct TriForm {
  using Args = TriArgs;
  using Best = TriBest;
  using Query = TriLine;
  struct Cand { float x2, y2; double thr; };
  const Args& a;
  const float* epi;
  const float ex, ey;
  const float2 *xy1, *xy2;
  const uint8_t* oct2;
  uint32_t n_m = 0;
  __device__ TriForm(const Args& a, const int32_t* job, size_t g1, size_t g2)
      : a(a), epi(a.epi + job[7]), ex(epi[9]), ey(epi[10]), xy1(reinterpret_cast<const float2*>(a.xy + 2 * g1)), xy2(reinterpret_cast<const float2*>(a.xy + 2 * g2)), oct2(a.oct + g2) {}
  static __device__ bool is_query(uint8_t has) { return has == 0; }
  static __device__ bool is_counted(uint8_t has) { return has == 0; }
  __device__ Query query(bool my_query, int idx1) const {
    Query l = {0.0f, 0.0f, 0.0f, 0.0f};
    if (my_query) { const float2 p = xy1[idx1]; l = tsm_line(p.x, p.y, epi); }
    return l;
  }
  static __device__ Query lane_read(const Query& l, int q) { return {::lane_read(l.a, q), ::lane_read(l.b, q), ::lane_read(l.c, q), ::lane_read(l.den, q)}; }
  __device__ bool candidate(bool free2, int idx2, Cand& c) const {
    bool ok = false;
    c = {0.0f, 0.0f, 0.0};
    if (free2) {
      const int o = oct2[idx2];
      if (o < a.nlevels) {   // an octave the tables do not have: no candidate, and neither table is read
        const float2 p = xy2[idx2];
        c.x2 = p.x; c.y2 = p.y;
        ok = !tsm_epipole_gate(ex, ey, c.x2, c.y2, a.sf[o]);
        c.thr = a.thr[o];
      }
    }
    return ok;
  }
  static __device__ uint32_t key(int d, uint32_t pos, const Query& l, const Cand& c) {
    return d <= TSM_TH_LOW && tsm_line_gate_thr(l.a, l.b, l.c, l.den, c.x2, c.y2, c.thr) ? (uint32_t)d << 16 | (0xFFFFu - pos) : fvp::kNoKey;
  }
  static __device__ void reduce(uint32_t key, int my_idx2, int pos0, bool holds, Best& part) {
    const uint32_t m1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)lanex::wave_min_u32(key));
    if (m1 == fvp::kNoKey) return;   // wave-uniform
    const Best r = {(int)(m1 >> 16), __builtin_amdgcn_readlane(my_idx2, (int)(0xFFFFu - (m1 & 0xFFFFu)) - pos0)};
    if (holds) part = tsm_merge(part, r);
  }
  static __device__ Best empty() { return tsm_empty(); }
  __device__ uint32_t word(bool my_query, const Best& part, uint32_t, int) {
    const bool matched = my_query && part.idx >= 0;
    n_m += (uint32_t)__popcll(__ballot(matched));
    return tsm_pack(matched ? TSM_MATCHED : TSM_NO_MATCH, part);
  }
  __device__ void add_counters(const Args& a, int j) const { if (n_m) atomicAdd(a.n_match + j, n_m); }
};

__global__ __launch_bounds__(fvp::kThreads) void tri_search_kernel(TriArgs a) { fvp::fv_pair_wave<TriForm>(a); }

}  // namespace

extern "C" int ccm_tri_search_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int J, const int64_t* key1, const int64_t* key2, const int32_t* has1_off, const uint8_t* has1,
                                            const int32_t* has2_off, const uint8_t* has2, const float* job_epi, int nlevels, const float* scale_factors,
                                            const float* level_sigma2, uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  if (!ctx) return CCM_E_ARG;
  using B = TriSearchResidentBlock;
  const fvp::FvPairCall<B> c = {"ccm_tri_search_eval_resident: ", "tri", "tri_search", tsm_check_args(J, job_epi, nlevels, scale_factors, level_sigma2),
                                (int64_t)J * TSM_EPI_FLOATS > (int64_t)INT32_MAX ? "too many jobs" : nullptr, J, key1, key2, has1_off, has1, &B::has1, has2_off, has2, &B::has2,
                                table, n_query, n_dist, n_match, &B::n_match};
  return fvp::fv_pair_stage(
      ctx, st, c, tri_search_kernel, TSM_EPI_FLOATS,
      [&](const B& b) {
        double* h_thr = b.up(b.line_thr);
        for (int l = 0; l < nlevels; l++) h_thr[l] = tsm_line_thr(level_sigma2[l]);
        b.put(b.job_epi, job_epi); b.put(b.scale_factors, scale_factors);
      },
      [&](const B& b, TriArgs& a) {
        a.nlevels = nlevels; a.epi = b.dev(b.job_epi); a.sf = b.dev(b.scale_factors); a.thr = b.dev(b.line_thr);
        a.oct = st->d_oct; a.xy = st->d_xy; a.n_match = (uint32_t*)b.dev(b.n_match);
      },
      (size_t)nlevels);
}
