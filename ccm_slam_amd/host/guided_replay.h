// guided_replay.h — the sequential parts of the matcher's searches that need no device and none of the mirror's classes, so that a stand-alone program can run them
// (tests/host/guided_search_check.cpp): the rotation-consistency filter every search ends in (ORBmatcher.cpp:1607-1648 and the bin rule, e.g. :1568-1575) and the
// sequential pass of SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist) (:1494-1602) on the candidate lists ccm_frame_guided_search returns.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace ccm_guided {

constexpr int kHistoLength = 30;   // ORBmatcher::HISTO_LENGTH

inline void threeMaxima(const std::vector<int>* histo, int L, int& ind1, int& ind2, int& ind3) {   // ORBmatcher.cpp:1607-1648
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = (int)histo[i].size();
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) ind3 = -1;
}
inline int histBin(float rot) {
  if (rot < 0.0) rot += 360.0f;
  int bin = (int)std::round(rot * (1.0f / kHistoLength));   // upstream quirk: 30-degree bins (:1358)
  if (bin == kHistoLength) bin = 0;
  return bin;
}
// The rotation-consistency filter of every search: a match is added under the difference of its two keypoints' angles, and the matches of every bin but the three
// fullest are rejected, bins ascending, a bin's matches in the order they were added.  The source asserts 0 <= bin < HISTO_LENGTH; angles that leave the range
// (a difference of 915 degrees or more) are the caller's error here as there.
struct RotationFilter {
  std::vector<int> hist[kHistoLength];
  void add(float rot, int index) {
    const int bin = histBin(rot);
    if (bin < 0 || bin >= kHistoLength) throw std::invalid_argument("RotationFilter: an angle difference outside the histogram");
    hist[bin].push_back(index);
  }
  template <class Reject>
  void reject_outliers(Reject reject) const {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    threeMaxima(hist, kHistoLength, ind1, ind2, ind3);
    for (int i = 0; i < kHistoLength; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int k : hist[i]) reject(k);
    }
  }
};

// :1494-1602 on the lists: the slots in order; a feature that holds anything (mvpMapPoints[i2] >= 0) is skipped; dist < bestDist is strict, so the first of equal
// distances in GetFeaturesInArea's order wins; bestDist <= ORBdist is inclusive; a match claims its feature for the slots behind it; the histogram takes the
// keyframe slot's angle minus the frame feature's (frameAngle(i2)); matches outside the three fullest bins are taken back.  Returns nmatches.
template <class FrameAngle>
int replay(int n_slots, const int32_t* off, const int32_t* idx, const uint16_t* dist, const float* kf_angle, FrameAngle frameAngle, int n_features, int32_t* mvpMapPoints,
           int ORBdist, bool checkOrientation) {
  if (ORBdist < 0 || ORBdist > 255) throw std::invalid_argument("SearchByProjection: ORBdist must be 0 .. 255");   // at 256 the source would index with bestIdx2 = -1
  if (checkOrientation && n_slots && !kf_angle) throw std::invalid_argument("SearchByProjection: the rotation check needs the keyframe's angles");
  int nmatches = 0;
  RotationFilter rot;
  for (int i = 0; i < n_slots; i++) {
    int bestDist = 256, bestIdx2 = -1;
    for (int s = off[i]; s < off[i + 1]; s++) {
      const int i2 = idx[s];
      if (i2 < 0 || i2 >= n_features) throw std::invalid_argument("SearchByProjection: a candidate the frame does not have");
      if (mvpMapPoints[i2] >= 0) continue;
      if ((int)dist[s] < bestDist) { bestDist = dist[s]; bestIdx2 = i2; }
    }
    if (bestDist <= ORBdist) {
      mvpMapPoints[bestIdx2] = i;
      nmatches++;
      if (checkOrientation) rot.add(kf_angle[i] - frameAngle(bestIdx2), bestIdx2);
    }
  }
  if (checkOrientation) rot.reject_outliers([&](int k) { mvpMapPoints[k] = -1; nmatches--; });
  return nmatches;
}

}  // namespace ccm_guided
