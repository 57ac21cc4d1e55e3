// c_api_util.h — what the C entry points (c_*.cpp, declared in ccm_host_c.h) say alike, each written once: the calling thread's context, the guards that turn an
// exception into the function's error value, the handle cast, the copies into the caller's arrays and a Frame from flat arrays.  Not installed, not for shim/.
#pragma once
#include "ccm_host.h"
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

namespace ccmh_c __attribute__((visibility("hidden"))) {

// One context per (calling thread, device), created on first use and kept for the thread's lifetime: the reference's threads (tracking, mapping, loop finder ...)
// each call the matcher / optimizer from their own loop, so the per-call cost is a map lookup, not a stream + buffer set-up.  Defined once, in
// c_api_util.cpp: a copy per unit would give a thread one context per unit.
cslam::HipContext& thread_context(int device);
// device < 0 asks for the host evaluator
inline cslam::HipContext* ctx_or_null(int device) { return device < 0 ? nullptr : &thread_context(device); }

// f() with a std::exception mapped to the entry point's error value: nullptr from a create; -1000; -1 for a bad argument (std::invalid_argument) and -1000 else
template <class F>
void* guard_ptr(F&& f) {
  try { return f(); } catch (const std::exception&) { return nullptr; }
}
template <class F>
int guard_int(F&& f) {
  try { return f(); } catch (const std::exception&) { return -1000; }
}
template <class F>
int guard_arg(F&& f) {
  try { return f(); } catch (const std::invalid_argument&) { return -1; } catch (const std::exception&) { return -1000; }
}

// the object behind a handle
template <class T>
T* as(void* h) { return static_cast<T*>(h); }

// v into dst where the caller asked for it
template <class T>
void copy_out(T* dst, const std::vector<T>& v) {
  if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
}
// at most cap entries of v into out (nullable); the size of v
inline int view(const std::vector<int32_t>& v, int32_t* out, int cap) {
  if (out) for (int k = 0; k < (int)v.size() && k < cap; k++) out[k] = v[k];
  return (int)v.size();
}
// The tail of a resolve: n, or -1001 when the caller's n_pts is not the batch's.  (The three projected window searches end in it too: their vectors are
// assigned P.n = n_pts entries on every path, so -1001 cannot be returned there and they copy what they always copied.)
inline int copy_best(int n, int n_pts, const std::vector<int32_t>& bi, const std::vector<int32_t>& bd, int32_t* best_idx, int32_t* best_dist) {
  if ((int)bi.size() != n_pts) return -1001;
  if (n_pts) { std::memcpy(best_idx, bi.data(), bi.size() * 4); std::memcpy(best_dist, bd.data(), bd.size() * 4); }
  return n;
}

// keypoints from coordinate arrays (ang, oct: nullable) and from an array of cslam::KeyPoint behind a void pointer
inline std::vector<cslam::KeyPoint> mk_keys(const float* x, const float* y, const int32_t* oct, const float* ang, int N) {
  std::vector<cslam::KeyPoint> k(N);
  for (int i = 0; i < N; i++) k[i] = cslam::KeyPoint{x[i], y[i], 31.f, ang ? ang[i] : 0.f, 0.f, oct ? oct[i] : 0};
  return k;
}
inline std::vector<cslam::KeyPoint> raw_keys(const void* kps, int N) {
  return std::vector<cslam::KeyPoint>(static_cast<const cslam::KeyPoint*>(kps), static_cast<const cslam::KeyPoint*>(kps) + N);
}

// A Frame from flat arrays: the keypoints it owns and the view on them.  bounds (nullable): minX minY maxX maxY; frame_mp: the caller's mvpMapPoints, or nullptr.
struct FlatFrame {
  std::vector<cslam::KeyPoint> keys;
  std::vector<int32_t> free_mp;
  cslam::FrameView F;
  FlatFrame(std::vector<cslam::KeyPoint> k, const uint8_t* desc, const float* bounds, const float* scale_factors, int32_t* frame_mp) : keys(std::move(k)) {
    F.N = (int)keys.size(); F.mvKeysUn = keys.data(); F.mDescriptors = desc;
    if (bounds) { F.mnMinX = bounds[0]; F.mnMinY = bounds[1]; F.mnMaxX = bounds[2]; F.mnMaxY = bounds[3]; }
    F.mvScaleFactors = scale_factors; F.mvpMapPoints = frame_mp;
  }
  // the same with the bounds of a device grid
  FlatFrame(std::vector<cslam::KeyPoint> k, const uint8_t* desc, const cslam::FrameGridDev& g, const float* scale_factors, int32_t* frame_mp)
      : FlatFrame(std::move(k), desc, nullptr, scale_factors, frame_mp) {
    F.mnMinX = g.mnMinX; F.mnMinY = g.mnMinY; F.mnMaxX = g.mnMaxX; F.mnMaxY = g.mnMaxY;
  }
  FlatFrame(FlatFrame&&) = default;   // a moved vector keeps its array: F stays valid
  FlatFrame(const FlatFrame&) = delete;
  // mvpMapPoints of a caller that has none: every feature free (-1), kept here
  FlatFrame& all_free() { free_mp.assign(keys.size(), -1); F.mvpMapPoints = free_mp.data(); return *this; }
};

}  // namespace ccmh_c
