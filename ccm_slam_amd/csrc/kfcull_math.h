// kfcull_math.h — the rules of the server's keyframe culling walk, LocalMapping::KeyFrameCullingV3 (cslam/src/Mapping.cpp:804-862) with what culling a keyframe does
// to the points it sees (KeyFrame::SetBadFlag, KeyFrame.cpp:990-997; MapPoint::EraseObservation, MapPoint.cpp:442-509; MapPoint::SetBadFlag, :545-558), host + device.
// The kernels of kfcull.hip run these lines; the host evaluator of cslam::KeyFrameCullingBatch (host/ccm_host.cpp) compiles them with g++.  Integers only, plus
// the one f64 multiply and compare of the verdict.
//
// Keyframes 0 .. n_cand - 1 are the candidates in walk order, n_cand .. n_all - 1 the other observers.  State per point p: n(p) = Observations() (given by the
// caller, it may differ from the length of the list), the observer list (keyframe, octave of the point's feature there, bad flag), gone(p) (initially the caller's
// bad flag), and the set of erased candidates.
//   turn of k     every slot i of k's list with a point p that is not null and not gone: nMPs++; if n(p) > th_obs, count the observers of p that are not bad, not
//                 erased, not k and whose octave is <= level(k, i) + 1, stopping at th_obs; the slot is redundant iff the count reached th_obs (the early break
//                 makes this independent of the observers' order)
//   verdict       redundant iff (double)nRed > thres * (double)nMPs
//   erasing k     (a redundant candidate without NOT_ERASE) k joins the erased set; every DISTINCT point p of its list that is not gone and lists k as observer:
//                 n(p)--, and gone(p) = 1 if n(p) <= 2 or no observer of p is left that is neither bad nor erased.  A slot whose point does not list k erases nothing.
//   SKIP          the candidate is not evaluated and stays a valid observer; NOT_ERASE: evaluated, a redundant verdict is reported (3) and erases nothing
// An erased candidate is bad (KeyFrame::SetBadFlag sets mbBad) and has left the observations of the points it listed, so "not erased" covers both.
//
// Invariant the second `gone` case relies on, and which the reference maintains: a live point's reference keyframe mpRefKF is one of its listed, non-bad observers.
// EraseObservation re-selects mpRefKF among the non-bad observers only when the erased keyframe was the reference, and discards the point when none is left; under
// the invariant "no live observer left" happens exactly when that re-selection fails, whichever observer the reference was.  It holds across the walk as long as
// every candidate that can be erased has a slot for each point that lists it (the reference's AddObservation / AddMapPoint pairs), so that an erased keyframe never
// stays listed as a point's reference.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KFCULL_HD __host__ __device__ inline
#else
#define KFCULL_HD inline
#endif

enum { KFCULL_SKIP = 1, KFCULL_NOT_ERASE = 2 };                                         // cand_flags
enum { KFCULL_KEPT = 0, KFCULL_CULLED = 1, KFCULL_SKIPPED = 2, KFCULL_REDUNDANT_NOT_ERASED = 3 };   // verdict
enum { KFCULL_SLOT_COUNTED = 1, KFCULL_SLOT_REDUNDANT = 2, KFCULL_SLOT_VOLATILE = 4 };  // the per-slot byte of the first kernel

// pMP && !pMP->isBad()
KFCULL_HD bool kfcull_slot_counts(int32_t pt, int32_t gone) { return pt >= 0 && !gone; }
// pMP->Observations() > thObs
KFCULL_HD bool kfcull_point_is_checked(int32_t n_obs, int32_t th_obs) { return n_obs > th_obs; }
// one observer inside the loop of Mapping.cpp:831-847
KFCULL_HD bool kfcull_observer_counts(int32_t kf, bool bad, bool erased, int32_t k, int32_t level, int32_t slot_level) {
  return !bad && !erased && kf != k && level <= slot_level + 1;
}
// the erased set: one bit per candidate; observers outside the candidates are never in it
KFCULL_HD bool kfcull_erased(const uint32_t* mask, int32_t n_cand, int32_t kf) { return kf < n_cand && ((mask[kf >> 5] >> (kf & 31)) & 1u); }
// min(th_obs, counting observers) of one slot of candidate k
KFCULL_HD int32_t kfcull_count_observers(const int32_t* obs_kf, const uint8_t* obs_level, const uint8_t* obs_bad, int32_t o0, int32_t o1, const uint32_t* erased,
                                         int32_t n_cand, int32_t k, int32_t slot_level, int32_t th_obs) {
  int32_t n = 0;
  for (int32_t o = o0; o < o1; o++) {
    const int32_t kf = obs_kf[o];
    if (kfcull_observer_counts(kf, obs_bad[o] != 0, kfcull_erased(erased, n_cand, kf), k, obs_level[o], slot_level) && ++n >= th_obs) break;
  }
  return n;
}
// nRedundantObservations > params::mapping::mfRedundancyThres * nMPs: the int converts to double, one multiply, one compare
KFCULL_HD bool kfcull_redundant(int32_t n_red, int32_t n_mps, double thres) { return (double)n_red > thres * (double)n_mps; }
KFCULL_HD int32_t kfcull_verdict(bool redundant, int32_t flags) { return !redundant ? KFCULL_KEPT : (flags & KFCULL_NOT_ERASE) ? KFCULL_REDUNDANT_NOT_ERASED : KFCULL_CULLED; }
// can the erasure of this observer change a slot of candidate k: it is walked before k and can be erased at all
KFCULL_HD bool kfcull_observer_is_volatile(int32_t kf, int32_t k, const int32_t* cand_flags) { return kf < k && cand_flags[kf] == 0; }
// after nObs--: `if (nObs <= 2) bBad = true`, or the re-selection of mpRefKF found no keyframe
KFCULL_HD bool kfcull_point_goes(int32_t n_after, bool live_observer_left) { return n_after <= 2 || !live_observer_left; }
// candidate k's counts of the initial state stand unless an earlier candidate was erased and one of k's slots is volatile
KFCULL_HD bool kfcull_reevaluated(bool erased_before, int32_t n_volatile_slots) { return erased_before && n_volatile_slots > 0; }

#include <vector>
// the argument checks shared by ccm_kfcull_walk and the host evaluator: nullptr, or what is wrong
inline const char* kfcull_check_args(int n_cand, int n_all, const uint8_t* cand_flags, const int32_t* list_off, const int32_t* list_pt, const uint8_t* list_level, int n_pt,
                                     const int32_t* pt_nobs, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* obs_level,
                                     const uint8_t* obs_bad, int th_obs, double thres, int n_levels) {
  if (n_cand < 1 || n_all < n_cand || n_pt < 0 || th_obs < 1 || !cand_flags || !list_off) return "bad args";
  if (thres != thres) return "thres is NaN";
  if (list_off[0] != 0) return "list_off[0] != 0";
  for (int i = 0; i < n_cand; i++) if (list_off[i + 1] < list_off[i]) return "list_off decreases";
  const int32_t NL = list_off[n_cand];
  if (NL && (!list_pt || !list_level)) return "bad args";
  if (n_pt && (!obs_off || !pt_nobs || !pt_bad)) return "bad args";
  if (n_pt && obs_off[0] != 0) return "obs_off[0] != 0";
  for (int p = 0; p < n_pt; p++) if (obs_off[p + 1] < obs_off[p]) return "obs_off decreases";
  const int32_t NO = n_pt ? obs_off[n_pt] : 0;
  if (NO && (!obs_kf || !obs_level || !obs_bad)) return "bad args";
  for (int32_t e = 0; e < NL; e++) {
    if (list_pt[e] >= n_pt) return "point index out of range";
    if ((int)list_level[e] >= n_levels) return "level out of range";
  }
  for (int p = 0; p < n_pt; p++) if (pt_nobs[p] < 0) return "negative pt_nobs";
  std::vector<int32_t> seen_by((size_t)n_all, -1);
  for (int p = 0; p < n_pt; p++)
    for (int32_t o = obs_off[p]; o < obs_off[p + 1]; o++) {
      const int32_t kf = obs_kf[o];
      if (kf < 0 || kf >= n_all) return "observer out of range";
      if ((int)obs_level[o] >= n_levels) return "level out of range";
      if (seen_by[kf] == p) return "a keyframe twice in one point's observers";
      seen_by[kf] = p;
    }
  return nullptr;
}
