// c_api_util.cpp — the one definition behind c_api_util.h: the calling thread's contexts
#include "c_api_util.h"
#include <map>
#include <memory>

namespace ccmh_c {

cslam::HipContext& thread_context(int device) {
  thread_local std::map<int, std::unique_ptr<cslam::HipContext>> ctxs;
  auto& c = ctxs[device];
  if (!c) c.reset(new cslam::HipContext(device));
  return *c;
}

}  // namespace ccmh_c
