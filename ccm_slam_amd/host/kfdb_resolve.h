// kfdb_resolve.h — phase 2 of KeyFrameDatabase::DetectLoopCandidates / DetectMapMatchCandidates / DetectRelocalizationCandidates
// (cslam/src/Database.cpp:148-201, 273-326, 387-438) on the phase-1 table that ccm_kfdb_query returns: the keyframes with
// count > minCommonWords in lKFsSharingWords order and their float score si.  Header-only, so that the host mirror (ccm_host.cpp, keys)
// and the drop-in translation unit (shim/Database_hip.cpp, kfptr) run the same lines.  Float arithmetic exactly as the reference's:
// accScore += si in neighbour order, pBestKF moves on a strictly larger score, bestAccScore starts at minScore, retain accScore >
// 0.75f * bestAccScore, first occurrence of a pBestKF wins.
//
// A neighbour contributes when it is in the table (listed in this query with count > minCommonWords), with its si even if si < minScore.
// Relocalisation calls this with minScore = 0: its phase 2 keeps every scored keyframe (si >= 0 always holds for a listed keyframe) and starts
// bestAccScore at 0; a neighbour that was listed but not scored contributes 0.0f there (the reference reads an uninitialised mRelocScore,
// KeyFrame.cpp:36-58), which changes neither accScore nor pBestKF, so the same lines serve.
#pragma once
#include <cstddef>
#include <map>
#include <set>
#include <vector>

namespace kfdb {

// keys / si: the table in list order (n rows).  neighbours(key, out) fills out with GetBestCovisibilityKeyFrames(10) of key.
template <class Key, class Neighbours>
std::vector<Key> resolve(const std::vector<Key>& keys, const std::vector<float>& si, float minScore, Neighbours neighbours) {
  std::map<Key, float> scored;
  for (size_t i = 0; i < keys.size(); i++) scored.emplace(keys[i], si[i]);
  std::vector<std::pair<float, Key>> acc_and_match;
  float bestAccScore = minScore;
  std::vector<Key> nb;
  for (size_t i = 0; i < keys.size(); i++) {
    if (!(si[i] >= minScore)) continue;
    nb.clear();
    neighbours(keys[i], nb);
    float bestScore = si[i];
    float accScore = si[i];
    Key pBestKF = keys[i];
    for (const Key& k2 : nb) {
      auto it = scored.find(k2);
      if (it == scored.end()) continue;
      accScore += it->second;
      if (it->second > bestScore) {
        pBestKF = k2;
        bestScore = it->second;
      }
    }
    acc_and_match.emplace_back(accScore, pBestKF);
    if (accScore > bestAccScore) bestAccScore = accScore;
  }
  const float minScoreToRetain = 0.75f * bestAccScore;
  std::set<Key> added;
  std::vector<Key> out;
  for (const auto& am : acc_and_match)
    if (am.first > minScoreToRetain && added.insert(am.second).second) out.push_back(am.second);
  return out;
}

}  // namespace kfdb
