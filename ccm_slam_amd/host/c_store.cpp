// c_store.cpp — C entry points of KeyFrameStore and of what reads its shadows: SearchByBoWBatch, SearchForTriangulationBatch, MapPointRefresh
#include "ccm_host_c.h"
#include "ccm_host.h"
#include "c_api_util.h"
#include "../csrc/kfingest_math.h"
#include <cstring>

using namespace ccmh_c;

extern "C" {
// KeyFrameStore through C, and the batches built on it
void* ccmh_kfstore_create(int device, int max_kf, int max_feat) {
  return guard_ptr([&]() -> void* { return new cslam::KeyFrameStore(ctx_or_null(device), max_kf, max_feat); });
}
void ccmh_kfstore_destroy(void* h) { delete as<cslam::KeyFrameStore>(h); }
int ccmh_kfstore_add(void* h, int device, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
                     const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    return as<cslam::KeyFrameStore>(h)->add(ctx_or_null(device), M, keys, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off,
                                                      cell_idx);
  });
}
int ccmh_kfstore_erase(void* h, int device, int64_t key) {
  if (!h) return -1000;
  return guard_int([&]() -> int { as<cslam::KeyFrameStore>(h)->erase(ctx_or_null(device), key); return 0; });
}
int ccmh_kfstore_clear(void* h, int device) {
  if (!h) return -1000;
  return guard_int([&]() -> int { as<cslam::KeyFrameStore>(h)->clear(ctx_or_null(device)); return 0; });
}
int ccmh_kfstore_count(void* h, int* live, int* free_slots) {
  if (!h) return -1000;
  const cslam::KeyFrameStore& s = *as<cslam::KeyFrameStore>(h);
  if (live) *live = s.live();
  if (free_slots) *free_slots = s.free_slots();
  return 0;
}
void* ccmh_kfstore_handle(void* h) { return h ? as<cslam::KeyFrameStore>(h)->handle() : nullptr; }
int ccmh_kfstore_get(void* h, int device, int64_t key, int* n, int* n_in, int32_t* cell_off, int32_t* cell_idx) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    return as<cslam::KeyFrameStore>(h)->get(ctx_or_null(device), key, n, n_in, cell_off, cell_idx) ? 0 : -1;
  });
}

// the store's feature vectors and ComputeSim3's SearchByBoW for all candidates through C
int ccmh_kfstore_set_featvec(void* h, int device, int64_t key, int nn, const int32_t* node, const int32_t* off, const int32_t* idx, const float* angle) {
  if (!h) return -1000;
  return guard_int([&]() -> int {
    return as<cslam::KeyFrameStore>(h)->set_featvec(ctx_or_null(device), key, cslam::FeatureVectorView{nn, node, off, idx}, angle);
  });
}
int ccmh_kfstore_ingest(void* h, int device, void* voc, int levelsup, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
                        const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, int32_t* bow_n, int32_t* bow_word, double* bow_value, int32_t* fv_nn,
                        int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node) {
  if (!h || device < 0) return -1000;
  return guard_int([&]() -> int {
    return as<cslam::KeyFrameStore>(h)->ingest_flat(&thread_context(device), as<const ccm_vocab>(voc), nullptr, levelsup, M, keys, kf_rec, feat_off,
                                                              feat_xy, feat_octave, feat_desc, angle, bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx, feat_word,
                                                              feat_node);
  });
}
int ccmh_kfstore_shadow_equal(void* a, void* b, int64_t key) {
  if (!a || !b) return -1000;
  const std::shared_ptr<const cslam::KfShadow> x = as<cslam::KeyFrameStore>(a)->shadow(key), y = as<cslam::KeyFrameStore>(b)->shadow(key);
  if (!x || !y) return -1;
  auto bits = [](const std::vector<float>& u, const std::vector<float>& v) { return u.size() == v.size() && (u.empty() || !std::memcmp(u.data(), v.data(), u.size() * 4)); };
  return !std::memcmp(x->rec, y->rec, sizeof x->rec) && x->n == y->n && x->n_in == y->n_in && bits(x->xy, y->xy) && x->oct == y->oct && x->desc == y->desc &&
         x->cell_off == y->cell_off && x->cell_idx == y->cell_idx && x->has_fv == y->has_fv && x->fv_node == y->fv_node && x->fv_off == y->fv_off &&
         x->fv_idx == y->fv_idx && bits(x->angle, y->angle);
}
int ccmh_kfstore_ingest_host(void* h, int n_nodes, int L, const int32_t* child_off, const int32_t* child_id, const uint8_t* node_desc, const int32_t* word_id,
                             const double* weight, int levelsup, int M, const int64_t* keys, const float* kf_rec, const int32_t* feat_off, const float* feat_xy,
                             const uint8_t* feat_octave, const uint8_t* feat_desc, const float* angle, int32_t* bow_n, int32_t* bow_word, double* bow_value,
                             int32_t* fv_nn, int32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* feat_word, int32_t* feat_node) {
  if (!h) return -1000;
  cslam::KeyFrameStore& st = *as<cslam::KeyFrameStore>(h);
  if (!st.host_only()) return -1000;
  const bool no_tree = n_nodes <= 0 || !child_off || !node_desc || !word_id || !weight || (child_off[n_nodes] > 0 && !child_id);
  const ::kfi_tree tree = {n_nodes, L, child_off, child_id, node_desc, word_id, weight};
  return guard_int([&]() -> int {
    return st.ingest_flat(nullptr, nullptr, no_tree ? nullptr : &tree, levelsup, M, keys, kf_rec, feat_off, feat_xy, feat_octave, feat_desc, angle, bow_n, bow_word, bow_value,
                          fv_nn, fv_node, fv_off, fv_idx, feat_word, feat_node);
  });
}
int ccmh_bow_pair_eval_resident_host(void* store, int J, const int64_t* key1, const int64_t* key2, const int32_t* live1_off, const uint8_t* live1, const int32_t* live2_off,
                                     const uint8_t* live2, uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  if (!store) return -1;
  return cslam::bow_pair_eval_resident_host(*as<cslam::KeyFrameStore>(store), J, key1, key2, live1_off, live1, live2_off, live2, table, n_query, n_dist);
}
void* ccmh_bow_batch_create(void* store, int device, int64_t key1, int C, const int64_t* keys2, const uint8_t* live1, const int32_t* live2_off, const uint8_t* live2,
                            float nnratio, int check_orientation) {
  if (!store || C < 0 || (C > 0 && !live2_off)) return nullptr;
  return guard_ptr([&]() -> void* {
    std::vector<const uint8_t*> l2((size_t)C);
    for (int j = 0; j < C; j++) l2[j] = live2 ? live2 + live2_off[j] : nullptr;
    return new cslam::SearchByBoWBatch(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), key1, C, keys2, live1, l2.data(), nnratio,
                                       check_orientation != 0);
  });
}
int ccmh_bow_batch_result(void* h, int j, int n_feat, int32_t* matches12) {
  if (!h) return -1000;
  const cslam::SearchByBoWBatch& b = *as<cslam::SearchByBoWBatch>(h);
  if (j < 0 || j >= b.candidates()) return -1000;
  if (n_feat != (int)b.matches12(j).size()) return -1001;
  if (matches12 && n_feat) std::memcpy(matches12, b.matches12(j).data(), (size_t)n_feat * 4);
  return b.nmatches(j);
}
int ccmh_bow_batch_table(void* h, uint64_t* table, int32_t* n_query, int32_t* n_dist) {
  if (!h) return -1;
  const cslam::SearchByBoWBatch& b = *as<cslam::SearchByBoWBatch>(h);
  copy_out(table, b.table());
  if (n_query && b.candidates()) std::memcpy(n_query, b.nQuery().data(), (size_t)b.candidates() * 4);
  if (n_dist && b.candidates()) std::memcpy(n_dist, b.nDist().data(), (size_t)b.candidates() * 4);
  return 0;
}
long long ccmh_bow_batch_n_reeval(void* h) { return h ? as<cslam::SearchByBoWBatch>(h)->reevaluated() : -1; }
void ccmh_bow_batch_destroy(void* h) { delete as<cslam::SearchByBoWBatch>(h); }

// CreateNewMapPoints' SearchForTriangulation for all neighbours through C
int ccmh_tri_search_eval_resident_host(void* store, int J, const int64_t* key1, const int64_t* key2, const int32_t* has1_off, const uint8_t* has1, const int32_t* has2_off,
                                       const uint8_t* has2, const float* job_epi, int nlevels, const float* scale_factors, const float* level_sigma2, uint32_t* table,
                                       int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  if (!store) return -1;
  return cslam::tri_search_eval_resident_host(*as<cslam::KeyFrameStore>(store), J, key1, key2, has1_off, has1, has2_off, has2, job_epi, nlevels, scale_factors,
                                              level_sigma2, table, n_query, n_match, n_dist);
}
void* ccmh_tri_search_create(void* store, int device, int64_t key1, int C, const int64_t* keys2, const uint8_t* has1, const int32_t* has2_off, const uint8_t* has2,
                             const float* epi, const float* sigma2_2, const float* sf2, int nlevels, int check_orientation) {
  if (!store || C < 0 || (C > 0 && (!has2_off || !epi))) return nullptr;
  return guard_ptr([&]() -> void* {
    std::vector<const uint8_t*> h2((size_t)C);
    std::vector<cslam::SearchForTriangulationBatch::Epipolar> ep((size_t)C);
    for (int j = 0; j < C; j++) {
      h2[j] = has2 ? has2 + has2_off[j] : nullptr;
      std::memcpy(ep[j].F12, epi + 11 * (size_t)j, 9 * sizeof(float));
      ep[j].ex = epi[11 * (size_t)j + 9]; ep[j].ey = epi[11 * (size_t)j + 10];
    }
    return new cslam::SearchForTriangulationBatch(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), key1, C, keys2, has1,
                                                  h2.data(), ep.data(), sigma2_2, sf2, nlevels, check_orientation != 0);
  });
}
int ccmh_tri_search_resolve(void* h, int j, const uint8_t* has1_now, const uint8_t* has2_now, int n_feat, int32_t* matches12) {
  if (!h) return -1000;
  cslam::SearchForTriangulationBatch& b = *as<cslam::SearchForTriangulationBatch>(h);
  if (j < 0 || j >= b.neighbours()) return -1000;
  if (n_feat != b.features1()) return -1001;
  std::vector<int32_t> m;
  const int n = b.resolve(j, has1_now, has2_now, m);
  if (matches12 && n_feat) std::memcpy(matches12, m.data(), (size_t)n_feat * 4);
  return n;
}
int ccmh_tri_search_table(void* h, uint32_t* table, int32_t* n_query, int32_t* n_match, int32_t* n_dist) {
  if (!h) return -1;
  const cslam::SearchForTriangulationBatch& b = *as<cslam::SearchForTriangulationBatch>(h);
  copy_out(table, b.table());
  if (n_query && b.neighbours()) std::memcpy(n_query, b.nQuery().data(), (size_t)b.neighbours() * 4);
  if (n_match && b.neighbours()) std::memcpy(n_match, b.nMatch().data(), (size_t)b.neighbours() * 4);
  if (n_dist && b.neighbours()) std::memcpy(n_dist, b.nDist().data(), (size_t)b.neighbours() * 4);
  return 0;
}
long long ccmh_tri_search_n_reeval(void* h) { return h ? as<cslam::SearchForTriangulationBatch>(h)->reevaluated() : -1; }
void ccmh_tri_search_destroy(void* h) { delete as<cslam::SearchForTriangulationBatch>(h); }

// the refresh of map points through C
int ccmh_mappoint_refresh_eval_resident_host(void* store, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf,
                                             const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, int nlevels,
                                             const float* scale_factors, int32_t* best_obs, uint8_t* best_desc, float* normal, float* min_dist, float* max_dist,
                                             uint8_t* status) {
  if (!store) return -1;
  return cslam::mappoint_refresh_eval_resident_host(*as<cslam::KeyFrameStore>(store), K, keys, kf_center, P, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat,
                                                    nlevels, scale_factors, best_obs, best_desc, normal, min_dist, max_dist, status);
}
void* ccmh_mappoint_refresh_create(void* store, int device, int K, const int64_t* keys, const float* kf_center, int P, const int32_t* obs_off, const int32_t* obs_kf,
                                   const int32_t* obs_feat, const float* pos, const int32_t* ref_kf, const int32_t* ref_feat, const float* normal, const float* min_dist,
                                   const float* max_dist, int nlevels, const float* scale_factors) {
  if (!store) return nullptr;
  return guard_ptr([&]() -> void* {
    return new cslam::MapPointRefresh(*as<cslam::KeyFrameStore>(store), ctx_or_null(device), K, keys, kf_center,
                                      {P, obs_off, obs_kf, obs_feat}, {pos, ref_kf, ref_feat, normal, min_dist, max_dist}, nlevels, scale_factors);
  });
}
int ccmh_mappoint_refresh_result(void* h, int P, int32_t* best_obs, uint8_t* desc, uint8_t* has_desc, float* normal, float* min_dist, float* max_dist, uint8_t* status) {
  if (!h) return -1;
  const cslam::MapPointRefresh& m = *as<cslam::MapPointRefresh>(h);
  if (P != m.points()) return -1;
  for (int p = 0; p < P; p++) {
    best_obs[p] = m.best()[(size_t)p]; status[p] = m.status()[(size_t)p];
    const uint8_t* d = m.descriptor(p);
    has_desc[p] = d != nullptr;
    if (d) std::memcpy(desc + 32 * (size_t)p, d, 32);
    for (int c = 0; c < 3; c++) normal[3 * (size_t)p + c] = m.normal()[3 * (size_t)p + c];
    min_dist[p] = m.min_dist()[(size_t)p]; max_dist[p] = m.max_dist()[(size_t)p];
  }
  return 0;
}
void ccmh_mappoint_refresh_destroy(void* h) { delete as<cslam::MapPointRefresh>(h); }
}  // extern "C"
