// tri_search_math.h — the inner lines of ORBmatcher::SearchForTriangulation (cslam/src/ORBmatcher.cpp:700-852) with CheckDistEpipolarLine (:159-176), once, for the
// form of trisearch.hip and for the host: the epipole gate, the epipolar line of a query and its gate, the update of (bestDist, bestIdx2) by one
// accepted candidate, the merge of a pass behind the running result, the packing of one result word, the argument rules and the host evaluator of a whole
// ccm_tri_search_eval_resident call (its walk over the common nodes is bow_search_math.h's fv_pair_walk_host).  The f32 expressions keep the reference's operand
// order; compile with -ffp-contract=off (a product and a sum are two roundings).  The reference never sets vbMatched2 (:721, :763), so a query's result depends on
// the query alone.
#pragma once
#include <math.h>
#include "bow_search_math.h"
#define TSM_HD BSM_HD

#define TSM_TH_LOW 50         // bestDist before any candidate (:753); a candidate at this distance is accepted (:770)
#define TSM_EPI_FLOATS 11     // a job's floats: F12 (9, row-major), ex, ey
#define TSM_JOB_INTS BSM_JOB_INTS   // a job on the device: BSM_JOB_INTS' layout, and its last int, unused there, is the job's first float (11 j)
#define TSM_MAX_LEVELS 256    // an octave is one byte
enum { TSM_NOT_A_QUERY = 0, TSM_NO_MATCH = 1, TSM_MATCHED = 2 };

struct TriBest { int d, idx; };   // bestDist, bestIdx2
struct TriLine { float a, b, c, den; };

TSM_HD TriBest tsm_empty() { return TriBest{TSM_TH_LOW, -1}; }

// :775-778.  true: the candidate is inside the epipole's radius and is skipped.  `100 * sf` is int * float: 100 converts to float, one f32 product.
TSM_HD bool tsm_epipole_gate(float ex, float ey, float x2, float y2, float sf2_oct) {
  const float distex = ex - x2, distey = ey - y2;
  const float dxx = distex * distex, dyy = distey * distey;
  return dxx + dyy < (float)100 * sf2_oct;
}

// :162-164 and :168 for the keypoint (x1, y1) of keyframe 1; F12 row-major, so F12.at(r, c) = F12[3 r + c]
TSM_HD TriLine tsm_line(float x1, float y1, const float F12[9]) {
  TriLine l;
  l.a = x1 * F12[0] + y1 * F12[3] + F12[6];
  l.b = x1 * F12[1] + y1 * F12[4] + F12[7];
  l.c = x1 * F12[2] + y1 * F12[5] + F12[8];
  l.den = l.a * l.a + l.b * l.b;
  return l;
}

// :166-175 against a threshold already widened: thr = 3.84 * (double)mvLevelSigma2[octave] (the literal is a double, so the reference compares in double)
TSM_HD bool tsm_line_gate_thr(float a, float b, float c, float den, float x2, float y2, double thr) {
  const float num = a * x2 + b * y2 + c;
  if (den == 0) return false;
  const float dsqr = num * num / den;
  return (double)dsqr < thr;
}
TSM_HD double tsm_line_thr(float sigma2_oct) { return 3.84 * (double)sigma2_oct; }
TSM_HD bool tsm_line_gate(float a, float b, float c, float x2, float y2, float sigma2_oct) {
  return tsm_line_gate_thr(a, b, c, a * a + b * b, x2, y2, tsm_line_thr(sigma2_oct));
}

// :770 and :782-783 for a candidate that passed every gate: `dist > TH_LOW || dist > bestDist` rejects, so an equal distance replaces the winner (the later position
// wins).  best.d starts at TH_LOW and only falls, so d <= best.d implies d <= TH_LOW.
TSM_HD void tsm_accept(TriBest& best, int d, int idx2) {
  if (d <= best.d) { best.d = d; best.idx = idx2; }
}

// What the loop leaves after the candidates of `a` followed by those of `b`: b's winner stands unless a's is strictly nearer.
TSM_HD TriBest tsm_merge(const TriBest& a, const TriBest& b) { return b.idx >= 0 && b.d <= a.d ? b : a; }

// One result word.  bits 0-15: bestIdx2 + 1 (0: none), 16-23: bestDist (0 .. 50; 50 without a match, as :753 leaves it), 30-31: the status.
TSM_HD uint32_t tsm_pack(int status, const TriBest& b) {
  if (status == TSM_NOT_A_QUERY) return 0;
  return (uint32_t)(b.idx + 1) | (uint32_t)b.d << 16 | (uint32_t)status << 30;
}
TSM_HD int tsm_status(uint32_t w) { return (int)(w >> 30); }
TSM_HD int tsm_idx(uint32_t w) { return (int)(w & 0xFFFFu) - 1; }
TSM_HD int tsm_dist(uint32_t w) { return (int)(w >> 16 & 0xFFu); }

// The scalar rules of ccm_tri_search_eval_resident behind ccm_bow_pair_eval_resident's; nullptr, or what is wrong.
static inline const char* tsm_check_args(int J, const float* job_epi, int nlevels, const float* scale_factors, const float* level_sigma2) {
  if (nlevels < 1 || nlevels > TSM_MAX_LEVELS) return "nlevels outside 1 .. 256";
  if (J > 0 && (!scale_factors || !level_sigma2)) return "null level tables";
  if (J > 0 && !job_epi) return "null job_epi";
  return nullptr;
}

// A keyframe as the evaluator reads it: the feature vector and descriptors (BowKf), mvKeysUn as xy pairs and the octaves.
struct TriKf { BowKf k; const float* xy; const uint8_t* oct; };
struct TriLevels { int nlevels; const float* sf; const float* sigma2; };

// One candidate for one query: its distance when it passes :763 (has2 == 0), :770 against TH_LOW, the epipole gate and the line gate; -1 otherwise.  A feature whose
// octave is at or above nlevels is no candidate and the tables are not read for it (fuse_math.h's fsm_candidate treats it the same way: `o > level`, level < nlevels).
static inline int tsm_candidate_host(const uint8_t* qdesc, const TriLine& l, const TriKf& k2, int idx2, const uint8_t* has2, const float* epi, const TriLevels& lv) {
  if (has2[idx2]) return -1;
  const int o = k2.oct[idx2];
  if (o >= lv.nlevels) return -1;
  const int d = bsm_hamming(qdesc, k2.k.desc + 32 * (size_t)idx2);
  if (d > TSM_TH_LOW) return -1;
  const float x2 = k2.xy[2 * (size_t)idx2], y2 = k2.xy[2 * (size_t)idx2 + 1];
  if (tsm_epipole_gate(epi[9], epi[10], x2, y2, lv.sf[o])) return -1;
  if (!tsm_line_gate_thr(l.a, l.b, l.c, l.den, x2, y2, tsm_line_thr(lv.sigma2[o]))) return -1;
  return d;
}

// :753-785 for the query idx1 over node2's segment of keyframe 2, in list order.  *n_free: the candidates without a map point.
static inline TriBest tsm_reduce_host(const TriKf& k1, int idx1, const TriKf& k2, int node2, const uint8_t* has2, const float* epi, const TriLevels& lv, int* n_free) {
  const TriLine l = tsm_line(k1.xy[2 * (size_t)idx1], k1.xy[2 * (size_t)idx1 + 1], epi);
  TriBest b = tsm_empty();
  int cnt = 0;
  for (int32_t s = k2.k.off[node2]; s < k2.k.off[node2 + 1]; s++) {
    const int idx2 = k2.k.idx[s];
    if (!has2[idx2]) cnt++;
    const int d = tsm_candidate_host(k1.k.desc + 32 * (size_t)idx1, l, k2, idx2, has2, epi, lv);
    if (d >= 0) tsm_accept(b, d, idx2);
  }
  *n_free = cnt;
  return b;
}

// One job of ccm_tri_search_eval_resident on the calling thread: table (k1.k.n words), *n_query, *n_match, *n_dist.
static inline void tri_job_eval_host(const TriKf& k1, const TriKf& k2, const uint8_t* has1, const uint8_t* has2, const float* epi, const TriLevels& lv, uint32_t* table,
                                     int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  *n_query = *n_match = *n_dist = 0;
  fv_pair_walk_host(k1.k, k2.k, has1, false, table, [&](int idx1, int b) {
    int n_free = 0;
    const TriBest r = tsm_reduce_host(k1, idx1, k2, b, has2, epi, lv, &n_free);
    ++*n_query;
    *n_match += r.idx >= 0;
    *n_dist = (int32_t)((uint32_t)*n_dist + (uint32_t)n_free);   // wraps as the kernel's unsigned add does
    return tsm_pack(r.idx >= 0 ? TSM_MATCHED : TSM_NO_MATCH, r);
  });
}

// A whole call: job j is (k1[j], k2[j]) under the masks has1 + has1_off[j], has2 + has2_off[j] and the floats job_epi + 11 j; its words start at table + has1_off[j].
static inline void tri_search_eval_host(int J, const TriKf* k1, const TriKf* k2, const int32_t* has1_off, const uint8_t* has1, const int32_t* has2_off, const uint8_t* has2,
                                        const float* job_epi, const TriLevels& lv, uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  for (int j = 0; j < J; j++)
    tri_job_eval_host(k1[j], k2[j], has1 + has1_off[j], has2 + has2_off[j], job_epi + TSM_EPI_FLOATS * (size_t)j, lv, table + has1_off[j], n_query + j, n_match + j,
                      n_dist + j);
}
