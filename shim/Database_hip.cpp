// Database_hip.cpp — DROP-IN replacement for the translation unit cslam/src/Database.cpp of the reference: the KeyFrameDatabase that
// LoopFinder (LoopFinder.cpp:142) and MapMatcher (MapMatcher.cpp:150) query for every new keyframe, compiled against the reference's own
// Database.h.  The inverted file lives on the MI355X (ccm_kfdb_*, include/ccm_hip.h); phase 1 of every Detect* call (which keyframes share
// enough words, their L1 scores) is one device query, phase 2 (covisibility accumulation) runs the shared lines of
// ccm_slam_amd/host/kfdb_resolve.h on the reference's own KeyFrame::GetBestCovisibilityKeyFrames(10).
//
// Contract (include/ccm_hip.h): each query is computed on fresh state, which equals the reference whenever a keyframe is queried at most
// once per query kind — how LoopFinder and MapMatcher call it.  The KeyFrame scratch fields mLoopQuery / mnLoopWords / mLoopScore /
// mMatchQuery / mRelocQuery / mnRelocWords / mRelocScore are not written: nothing outside Database.cpp reads them.
// Device state lives in a registry keyed by the database's address (Database.h declares no destructor, so it lives until the process exits;
// there is one database per process, ServerSystem.cpp:185, ClientSystem.cpp:56).  mvInvertedFile stays empty.
// Keys pack mId as (id << 8) | client.  The key -> kfptr table keeps a keyframe alive until it is erased, as the reference's lists do.
// With a vocabulary whose scoring type is not L1 the device still finds and counts the keyframes and the scores come from mpVoc->score.
// There is no CPU path: if the device call fails the method throws estd::infrastructure_ex.
#include <cslam/Database.h>

#include <cstdlib>
#include <memory>
#include <unordered_map>

#include "../include/ccm_hip.h"
#include "../ccm_slam_amd/host/kfdb_resolve.h"

namespace cslam {

namespace {
typedef boost::shared_ptr<KeyFrame> kfptr;

int device() { static const int d = std::getenv("CCM_DEVICE") ? std::atoi(std::getenv("CCM_DEVICE")) : 0; return d; }

void fail(const char* what, ccm_ctx* ctx) {
  cout << COUTFATAL << "KeyFrameDatabase::" << what << ": the MI355X path failed: " << ccm_last_error(ctx) << endl;
  throw estd::infrastructure_ex();
}

// one context per calling thread (LoopFinder, MapMatcher and the mapping threads each call from their own loop)
ccm_ctx* thread_ctx() {
  struct Owner { ccm_ctx* c = nullptr; ~Owner() { if (c) ccm_ctx_destroy(c); } };
  thread_local Owner o;
  if (!o.c && ccm_ctx_create(device(), &o.c) != CCM_OK) fail("context", nullptr);
  return o.c;
}

int64_t pack(const idpair& id) {
  if (id.second >= 256 || id.first >= ((size_t)1 << 55)) {
    cout << COUTFATAL << "KeyFrameDatabase: keyframe id " << id.first << " / client " << id.second << " out of the key range" << endl;
    throw estd::infrastructure_ex();
  }
  return (int64_t)((id.first << 8) | id.second);
}

struct State {
  ccm_kfdb* db = nullptr;
  std::mutex mu;                                 // the key -> keyframe table
  std::unordered_map<int64_t, kfptr> kf;
};

State& state(const KeyFrameDatabase* self, size_t n_words) {
  static std::mutex reg_mu;
  static std::map<const KeyFrameDatabase*, std::unique_ptr<State>> reg;
  std::lock_guard<std::mutex> lk(reg_mu);
  std::unique_ptr<State>& s = reg[self];
  if (!s) {
    s.reset(new State());
    ccm_ctx* ctx = thread_ctx();
    if (ccm_kfdb_create(ctx, (int)n_words, 0, &s->db) != CCM_OK) fail("KeyFrameDatabase", ctx);
  }
  return *s;
}

void flatten(const DBoW2::BowVector& v, std::vector<int32_t>& w, std::vector<double>& x) {
  w.clear(); x.clear();
  for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { w.push_back((int32_t)it->first); x.push_back(it->second); }
}

// phase 1 on the device, phase 2 in kfdb_resolve.h
vector<kfptr> detect(State& st, const vocptr& voc, const DBoW2::BowVector& q, float minScore, const ccm_kfdb_filter* f) {
  std::vector<int32_t> w; std::vector<double> x;
  flatten(q, w, x);
  ccm_ctx* ctx = thread_ctx();
  std::vector<int64_t> key(64); std::vector<int32_t> cnt(64); std::vector<float> si(64); std::vector<double> s64(64);
  int n = 0;
  for (;;) {
    if (ccm_kfdb_query(st.db, ctx, (int)w.size(), w.data(), x.data(), f, (int)key.size(), key.data(), cnt.data(), si.data(), s64.data(), &n, nullptr, nullptr,
                       nullptr) != CCM_OK)
      fail("Detect*Candidates", ctx);
    if (n <= (int)key.size()) break;
    key.resize(n); cnt.resize(n); si.resize(n); s64.resize(n);
  }
  std::vector<kfptr> kfs; std::vector<float> scores;
  {
    std::lock_guard<std::mutex> lk(st.mu);
    for (int i = 0; i < n; i++) {
      auto it = st.kf.find(key[i]);
      if (it == st.kf.end()) continue;   // erased since the query
      kfs.push_back(it->second); scores.push_back(si[i]);
    }
  }
  if (voc->getScoringType() != DBoW2::L1_NORM)
    for (size_t i = 0; i < kfs.size(); i++) scores[i] = (float)voc->score(q, kfs[i]->mBowVec);
  return kfdb::resolve(kfs, scores, minScore, [](const kfptr& k, std::vector<kfptr>& out) { out = k->GetBestCovisibilityKeyFrames(10); });
}
}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const vocptr pVoc) : mpVoc(pVoc) {
  state(this, pVoc->size());
  cout << "+++++ KeyFrame Database Initialized (MI355X) +++++" << endl;
}

void KeyFrameDatabase::add(kfptr pKF) {
  State& st = state(this, mpVoc->size());
  std::vector<int32_t> w; std::vector<double> x;
  flatten(pKF->mBowVec, w, x);
  const int64_t k = pack(pKF->mId);
  ccm_ctx* ctx = thread_ctx();
  std::lock_guard<std::mutex> lk(st.mu);
  const int rc = ccm_kfdb_add(st.db, ctx, k, (int32_t)pKF->mId.second, (int)w.size(), w.data(), x.data());
  if (rc == CCM_E_STATE) return;   // already listed: the reference never adds a keyframe twice
  if (rc != CCM_OK) fail("add", ctx);
  st.kf[k] = pKF;
}

void KeyFrameDatabase::erase(kfptr pKF) {
  State& st = state(this, mpVoc->size());
  const int64_t k = pack(pKF->mId);
  ccm_ctx* ctx = thread_ctx();
  std::lock_guard<std::mutex> lk(st.mu);
  if (ccm_kfdb_erase(st.db, ctx, k) != CCM_OK) fail("erase", ctx);
  st.kf.erase(k);
}

void KeyFrameDatabase::clear() {
  State& st = state(this, mpVoc->size());
  ccm_ctx* ctx = thread_ctx();
  std::lock_guard<std::mutex> lk(st.mu);
  if (ccm_kfdb_clear(st.db, ctx) != CCM_OK) fail("clear", ctx);
  st.kf.clear();
}

vector<KeyFrameDatabase::kfptr> KeyFrameDatabase::DetectLoopCandidates(kfptr pKF, float minScore) {
  State& st = state(this, mpVoc->size());
  set<kfptr> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
  std::map<idpair, kfptr> mpAllKfsInMap = pKF->GetMapptr()->GetMmpKeyFrames();
  std::vector<int64_t> allow, exclude;
  allow.reserve(mpAllKfsInMap.size() + 1);
  for (std::map<idpair, kfptr>::const_iterator it = mpAllKfsInMap.begin(); it != mpAllKfsInMap.end(); ++it) allow.push_back(pack(it->first));
  for (set<kfptr>::const_iterator it = spConnectedKeyFrames.begin(); it != spConnectedKeyFrames.end(); ++it) exclude.push_back(pack((*it)->mId));
  allow.push_back(-1);   // never a key: keeps the pointer non-NULL for an empty map (which admits nothing)
  ccm_kfdb_filter f{pack(pKF->mId), allow.data(), (int)allow.size() - 1, exclude.data(), (int)exclude.size(), 0};
  return detect(st, mpVoc, pKF->mBowVec, minScore, &f);
}

vector<KeyFrameDatabase::kfptr> KeyFrameDatabase::DetectMapMatchCandidates(kfptr pKF, float minScore, mapptr pMap) {
  State& st = state(this, mpVoc->size());
  ccm_kfdb_filter f{-1, nullptr, 0, nullptr, 0, 0};
  std::vector<int64_t> exclude;
  bool wide = false;
  for (set<size_t>::const_iterator it = pMap->msuAssClients.begin(); it != pMap->msuAssClients.end(); ++it) {
    if (*it < 64) f.exclude_groups |= 1ull << *it;
    else wide = true;
  }
  if (wide) {   // client ids beyond the mask: list their keyframes
    std::lock_guard<std::mutex> lk(st.mu);
    for (auto it = st.kf.begin(); it != st.kf.end(); ++it)
      if (pMap->msuAssClients.count((size_t)(it->first & 0xff))) exclude.push_back(it->first);
    f.exclude = exclude.data(); f.n_exclude = (int)exclude.size();
  }
  return detect(st, mpVoc, pKF->mBowVec, minScore, &f);
}

// Outside the parity contract (no caller in CCM-SLAM): a neighbour that shares words but was not scored contributes 0.0f, where the
// reference reads an uninitialised mRelocScore (KeyFrame.cpp:36-58); see kfdb_resolve.h.
std::vector<KeyFrameDatabase::kfptr> KeyFrameDatabase::DetectRelocalizationCandidates(Frame& F) {
  State& st = state(this, mpVoc->size());
  return detect(st, mpVoc, F.mBowVec, 0.0f, nullptr);
}

// ---- map-point bookkeeping of the database (plain host maps) --------------------------------------------------------
void KeyFrameDatabase::AddMP(mpptr pMP) {
  if (!pMP) return;
  unique_lock<mutex> lock(mMutexMPs);
  mmpMPs[pMP->mId] = pMP;
}

void KeyFrameDatabase::AddDirectBad(size_t id, size_t cid) {
  unique_lock<mutex> lock(mMutexMPs);
  mmbDirectBad[idpair(id, cid)] = true;
}

bool KeyFrameDatabase::FindMP(size_t id, size_t cid) {
  unique_lock<mutex> lock(mMutexMPs);
  return mmpMPs.count(idpair(id, cid)) > 0;
}

bool KeyFrameDatabase::FindDirectBad(size_t id, size_t cid) {
  unique_lock<mutex> lock(mMutexMPs);
  return mmbDirectBad.count(idpair(id, cid)) > 0;
}

void KeyFrameDatabase::ResetMPs() {
  unique_lock<mutex> lock(mMutexMPs);
  mmbDirectBad.clear();
  mmpMPs.clear();
}

}  // namespace cslam
