// fuse.hip — the two batched Fuse stages, one launch each.
//   ccm_fuse_sim3_eval: every (keyframe, point) pair of a SearchAndFuse (cslam/src/LoopFinder.cpp:709-734, MapMerger.cpp:574-598).  A pair is one call of the loop
//     body of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cpp:1030-1118) up to the decision, without the map mutations.
//   ccm_fuse_pose_eval: every Fuse call of a LocalMapping::SearchInNeighbors (cslam/src/Mapping.cpp:471-547), both directions.  A pair is one pass of the loop body
//     of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cpp:883-965) up to the decision, without the skips and the map mutations.
//   ccm_fuse_sim3_eval_resident, ccm_fuse_pose_eval_resident: the same two calls on keyframes of a keyframe store (kfstore.hip), whose static
//     data is on the device already: the same pair body with kResident, which takes the keyframe's arrays from its slot of the store.
//   ccm_sim3_project_eval_resident: ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:308-446) on the INITIAL vpMatched: the Sim3
//     form's pair with a skip mask per feature of the keyframe (kMask).  ccm_sim3_pair_eval_resident: both directions of ORBmatcher::SearchBySim3 (:1124-1348) as
//     jobs of the pose form's layout: ssm_gate where Fuse has fsm_gate (kPair), no chi-square gate, TH_HIGH.  Both on keyframes of a store only.
// The lines of a pair are fuse_math.h; the two forms differ in the chi-square gate of the candidate (kChi2) and in how a workgroup finds its work.
//
// Layout.  fuse_sim3_kernel: the grid is (tiles of 256 points) x K keyframes, folded into one dimension.  fuse_pose_kernel: the work is a list
// of jobs, job j = keyframe job_kf[j] x points job_pt0[j] .. + job_n[j]; one workgroup takes a tile of 256 pairs of ONE job, and the stage writes (job, first pair)
// per workgroup while it validates the job arrays, so the kernel's first read is tile[blockIdx.x].  Either way a workgroup has one keyframe, so the keyframe's
// record, pose and offsets are addressed by workgroup-uniform values and loaded once per wave, and from there both kernels are fuse_pair: one lane per pair runs
// the gates.  A lane that passes them reads its cell range from the keyframe's CSR grid and walks its candidates alone: the query descriptor in 8 registers, a
// candidate two 16-byte loads, xor and popcount.  A window whose cells hold more than FSM_WIDE features is handed to the whole wave, one after the other (as
// kfcull_eval_kernel hands long observer lists over): the candidates of each grid column strided over the lanes, the minimum of dist << 16 | CSR position taken
// through lane_xor.h.  The switch is the feature count read from cell_off.  n_valid / n_hit: ballot popcounts per wave, one integer atomicAdd each.  No float
// atomics, no lane leaves early, nothing waits on another workgroup, every loop is bounded by a count read from the inputs (validated on the host before the launch).
#include "common.h"
#include "fuse_math.h"
#include "kfstore.h"
#include "lane_xor.h"
#include "stage_blocks.h"
#include <chrono>
#include <cstdio>

namespace {

static_assert(FPM_TILE == 256, "both kernels run 256 lanes, one per pair");

// everything either kernel reads.  P, tiles: the Sim3 form's grid; job, tile, inv_sigma2: the pose form's; slot, stride: the resident forms', whose rec, kxy, cell_off,
// cell_idx, koct and kdesc are the store's arrays; skip, skip_off: the masks of the projection search (keyframe k's bytes start at skip + skip_off[k])
struct FuseArgs {
  int P, tiles, nlevels;
  float th, logsf;
  const float *rec, *pose, *kxy, *scale_factors, *inv_sigma2, *pos, *normal, *dmin, *dmax;
  const int32_t *feat_off, *cell_off, *job, *tile;
  const uint16_t* cell_idx;
  const uint8_t *koct, *kdesc, *pdesc;
  uint32_t* table;
  int32_t *n_valid, *n_hit;
  float* uv;   // nullptr: not asked for
  const int32_t* slot;
  int stride;
  const uint8_t* skip;
  const int32_t* skip_off;
};

// the minimum of a 32-bit key over the wave; a u32 is exact in a double, so lane_xor.h's f64 exchange carries it
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t key) {
  double v = (double)key;
  v = fmin(v, lanex::from_partner<32>(v)); v = fmin(v, lanex::from_partner<16>(v)); v = fmin(v, lanex::from_partner<8>(v));
  v = fmin(v, lanex::from_partner<4>(v)); v = fmin(v, lanex::from_partner<2>(v)); v = fmin(v, lanex::from_partner<1>(v));
  return (uint32_t)v;
}

// One pair per lane: keyframe k (workgroup-uniform) x point i, answered into table[out] (and uv) and counted into n_valid / n_hit[counter] (workgroup-uniform).
// A dead lane (!live) reads nothing through i and writes nothing, but stays for the wave-wide part, which needs all 64.
// kResident: the keyframe's static arrays are a slot of the keyframe store (kfstore.hip): slot[k] and slot[k] * stride take the place of k and feat_off[k].  Both are
// workgroup-uniform like k, so the addresses still come from the scalar unit.
// pose (workgroup-uniform): the keyframe's 15 floats, or with kPair the job's SSM_JOB_FLOATS, which ssm_gate reads where the other forms run fsm_gate; the pair form
// reads no normals and accepts up to TH_HIGH.  kMask: feature f of the keyframe with skip[skip_off[k] + f] != 0 is no candidate, in either walk.
template <bool kChi2, bool kResident, bool kMask = false, bool kPair = false>
__device__ __forceinline__ void fuse_pair(const FuseArgs& a, int k, const float* pose, int i, bool live, uint32_t out, int counter) {
  const int lane = threadIdx.x & 63;
  const int s = kResident ? a.slot[k] : k;
  const float* rec = a.rec + (size_t)s * FSM_REC_FLOATS;
  const uint8_t* skip = kMask ? a.skip + a.skip_off[k] : nullptr;
  const uint32_t dist_th = kPair ? FSM_TH_HIGH : FSM_TH_LOW;
  const int32_t f0 = kResident ? s * a.stride : a.feat_off[k];   // slots * stride <= INT32_MAX
  const int32_t* cell_off = a.cell_off + (size_t)s * (FSM_CELLS + 1);
  const uint16_t* cell_idx = a.cell_idx + f0;
  const float* kxy = a.kxy + 2 * (size_t)f0;
  const uint8_t* koct = a.koct + f0;
  const uint8_t* kdesc = a.kdesc + 32 * (size_t)f0;

  int status = FSM_BEHIND, level = 0;
  float u = 0.0f, v = 0.0f, r = 0.0f;
  int x0 = 0, x1 = -1, y0 = 0, y1 = 0;
  uint32_t word = fsm_pack(FSM_BEHIND, 0, FSM_NO_DIST, FSM_NO_IDX);
  bool wide = false;
  if (live) {
    const float P3[3] = {a.pos[3 * (size_t)i], a.pos[3 * (size_t)i + 1], a.pos[3 * (size_t)i + 2]};
    if (kPair) {
      status = ssm_gate(rec, pose, P3, a.dmin[i], a.dmax[i], a.nlevels, a.logsf, u, v, level);
    } else {
      const float Pn[3] = {a.normal[3 * (size_t)i], a.normal[3 * (size_t)i + 1], a.normal[3 * (size_t)i + 2]};
      status = fsm_gate(rec, pose, P3, Pn, a.dmin[i], a.dmax[i], a.nlevels, a.logsf, u, v, level);
    }
    word = fsm_pack(status, 0, FSM_NO_DIST, FSM_NO_IDX);
    if (status == FSM_EMPTY) {
      r = a.th * a.scale_factors[level];
      bool any = false;
      uint32_t key = ~0u;
      if (fsm_cell_range(rec, u, v, r, x0, x1, y0, y1)) {
        if (fsm_window_count(cell_off, x0, x1, y0, y1) > FSM_WIDE) {
          wide = true;
        } else {
          uint32_t q[8];
          fsm_load_desc(a.pdesc + 32 * (size_t)i, q);
          for (int ix = x0; ix <= x1; ix++) {
            const int32_t c0 = cell_off[ix * FSM_GRID_ROWS + y0], c1 = cell_off[ix * FSM_GRID_ROWS + y1 + 1];
            for (int32_t p = c0; p < c1; p++) {
              bool in;
              const int d = fsm_candidate<kChi2, kMask>(kxy, koct, kdesc, cell_idx[p], u, v, r, level, a.inv_sigma2, q, in, skip);
              any |= in;
              if (d >= 0) key = min(key, ((uint32_t)d << 16) | (uint32_t)p);
            }
          }
        }
      }
      if (!wide) word = fsm_finish(level, any, key, cell_idx, dist_th);
    }
  }
  // the wide windows: the wave takes them one by one
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int si = __shfl(i, src, 64), sl = __shfl(level, src, 64);
    const float su = __shfl(u, src, 64), sv = __shfl(v, src, 64), sr = __shfl(r, src, 64);
    const int sx0 = __shfl(x0, src, 64), sx1 = __shfl(x1, src, 64), sy0 = __shfl(y0, src, 64), sy1 = __shfl(y1, src, 64);
    uint32_t q[8];
    fsm_load_desc(a.pdesc + 32 * (size_t)si, q);
    bool any = false;
    uint32_t key = ~0u;
    for (int ix = sx0; ix <= sx1; ix++) {
      const int32_t c0 = cell_off[ix * FSM_GRID_ROWS + sy0], c1 = cell_off[ix * FSM_GRID_ROWS + sy1 + 1];
      for (int32_t p = c0 + lane; p < c1; p += 64) {
        bool in;
        const int d = fsm_candidate<kChi2, kMask>(kxy, koct, kdesc, cell_idx[p], su, sv, sr, sl, a.inv_sigma2, q, in, skip);
        any |= in;
        if (d >= 0) key = min(key, ((uint32_t)d << 16) | (uint32_t)p);
      }
    }
    any = __ballot(any) != 0;
    key = wave_min_u32(key);
    if (lane == src) word = fsm_finish(level, any, key, cell_idx, dist_th);
  }
  if (live) {
    a.table[out] = word;
    if (a.uv) { a.uv[2 * (size_t)out] = u; a.uv[2 * (size_t)out + 1] = v; }
  }
  const int st = (int)(word >> 29);
  const int nv = (int)__popcll(__ballot(live && st >= FSM_EMPTY)), nh = (int)__popcll(__ballot(live && st == FSM_HIT));
  if (lane == 0) {
    if (nv) atomicAdd(&a.n_valid[counter], nv);
    if (nh) atomicAdd(&a.n_hit[counter], nh);
  }
}

// workgroup = (keyframe k, tile of 256 points): word k * P + i (K * P <= INT32_MAX), the counters are the keyframe's
template <bool kResident, bool kMask = false>
__device__ __forceinline__ void fuse_sim3_body(const FuseArgs& a) {
  const int k = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
  const int i = tile * FPM_TILE + (int)threadIdx.x;
  fuse_pair<false, kResident, kMask>(a, k, a.pose + (size_t)k * FSM_POSE_FLOATS, i, i < a.P, (uint32_t)k * (uint32_t)a.P + (uint32_t)i, k);
}
__global__ __launch_bounds__(FPM_TILE) void fuse_sim3_kernel(FuseArgs a) { fuse_sim3_body<false>(a); }
__global__ __launch_bounds__(FPM_TILE) void fuse_sim3_resident_kernel(FuseArgs a) { fuse_sim3_body<true>(a); }
__global__ __launch_bounds__(FPM_TILE) void proj_sim3_resident_kernel(FuseArgs a) { fuse_sim3_body<true, true>(a); }

// workgroup = tile[blockIdx.x] = (job j, first pair of the job): the job's words start at its out0, the counters are the job's
template <bool kResident, bool kPair = false>
__device__ __forceinline__ void fuse_pose_body(const FuseArgs& a) {
  const int j = a.tile[2 * (size_t)blockIdx.x], i0 = a.tile[2 * (size_t)blockIdx.x + 1];
  const int32_t* jr = a.job + FPM_JOB_INTS * (size_t)j;
  const int k = jr[0], pt0 = jr[1], n = jr[2], out0 = jr[3];
  const int e = i0 + (int)threadIdx.x;   // the pair's place in the job
  const bool live = e < n;
  const float* pose = kPair ? a.pose + (size_t)j * SSM_JOB_FLOATS : a.pose + (size_t)k * FSM_POSE_FLOATS;
  fuse_pair<!kPair, kResident, false, kPair>(a, k, pose, live ? pt0 + e : pt0, live, (uint32_t)out0 + (uint32_t)e, j);
}
__global__ __launch_bounds__(FPM_TILE) void fuse_pose_kernel(FuseArgs a) { fuse_pose_body<false>(a); }
__global__ __launch_bounds__(FPM_TILE) void fuse_pose_resident_kernel(FuseArgs a) { fuse_pose_body<true>(a); }
__global__ __launch_bounds__(FPM_TILE) void sim3_pair_resident_kernel(FuseArgs a) { fuse_pose_body<true, true>(a); }

typedef std::chrono::steady_clock Clock;
double us_between(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); }

// what a caller passes to every form: the level tables and scalars, the points, the outputs.  inv_sigma2 and normal: null where the form has no such segment.
struct FuseCall {
  int nlevels; const float *scale_factors, *inv_sigma2; float logsf, th;
  const float *pos, *normal, *dmin, *dmax; const uint8_t* pt_desc;
  uint32_t* table; int32_t *n_valid, *n_hit; float* uv;
};
// the keyframes: the caller's flat arrays (st == nullptr), or the slots of a store, which fuse_store_slots made of the keys under the reader lock the caller holds
struct FuseKfs {
  const float* rec; const int32_t* feat_off; const float* xy; const uint8_t *oct, *desc; const int32_t *cell_off, *cell_idx;
  const ccm_kfstore* st; const int32_t* slots;
};

// The host side of the upload for everything but the form's own segments (pose; job and tile; the masks), and the kernels' view of the block.  A segment the form does
// not have has no elements: put() copies nothing, and what the kernel's pointer to it holds does not matter.
FuseArgs fuse_stage_inputs(const FuseBlock& b, const FuseCall& c, const FuseKfs& kf) {
  FuseArgs a = {};
  if (kf.st) {
    b.put(b.slot, kf.slots);
    a.rec = kf.st->d_rec; a.kxy = kf.st->d_xy; a.cell_off = kf.st->d_cell_off; a.cell_idx = kf.st->d_cell_idx; a.koct = kf.st->d_oct; a.kdesc = kf.st->d_desc;
    a.slot = b.dev(b.slot); a.stride = kf.st->stride;
  } else {
    b.put(b.kdesc, kf.desc); b.put(b.rec, kf.rec); b.put(b.feat_off, kf.feat_off); b.put(b.cell_off, kf.cell_off); b.put(b.kxy, kf.xy); b.put(b.koct, kf.oct);
    uint16_t* h_idx = b.up(b.cell_idx);
    for (size_t f = 0; f < b.cell_idx.count; f++) h_idx[f] = (uint16_t)kf.cell_idx[f];
    a.rec = b.dev(b.rec); a.kxy = b.dev(b.kxy); a.feat_off = b.dev(b.feat_off); a.cell_off = b.dev(b.cell_off); a.cell_idx = b.dev(b.cell_idx);
    a.koct = b.dev(b.koct); a.kdesc = b.dev(b.kdesc);
  }
  b.put(b.pdesc, c.pt_desc); b.put(b.scale_factors, c.scale_factors); b.put(b.inv_sigma2, c.inv_sigma2);
  b.put(b.pos, c.pos); b.put(b.normal, c.normal); b.put(b.dmin, c.dmin); b.put(b.dmax, c.dmax);
  a.nlevels = c.nlevels; a.th = c.th; a.logsf = c.logsf;
  a.P = (int)b.s.P; a.tiles = (int)((b.s.P + FPM_TILE - 1) / FPM_TILE);
  a.pose = b.dev(b.pose); a.scale_factors = b.dev(b.scale_factors); a.inv_sigma2 = b.dev(b.inv_sigma2);
  a.pos = b.dev(b.pos); a.normal = b.dev(b.normal); a.dmin = b.dev(b.dmin); a.dmax = b.dev(b.dmax); a.pdesc = b.dev(b.pdesc);
  a.job = b.dev(b.job); a.tile = b.dev(b.tile); a.skip = b.dev(b.skip); a.skip_off = b.dev(b.skip_off);
  a.table = b.dev(b.table); a.n_valid = b.dev(b.n_valid); a.n_hit = b.dev(b.n_hit);
  a.uv = b.uv.count ? b.dev(b.uv) : nullptr;
  return a;
}

int fuse_store_ok(ccm_ctx* ctx, const ccm_kfstore* st, const char* me) {
  if (!st) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "NULL store");
  if (st->device != ctx->device) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "the context is on another device than the store");
  return CCM_OK;
}

// keys -> slots under the caller's reader lock; CCM_E_ARG for a key that is not live
int fuse_store_slots(ccm_ctx* ctx, const ccm_kfstore* st, int K, const int64_t* keys, const char* me, std::vector<int32_t>* slots) {
  slots->resize((size_t)K);
  for (int k = 0; k < K; k++) {
    auto it = st->live.find(keys[k]);
    if (it == st->live.end()) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "a key is not in the store");
    (*slots)[k] = it->second;
  }
  return CCM_OK;
}

// the form's own segments.  The Sim3 forms' pose: the decomposed Scw of every keyframe
void fuse_pack_scw(const FuseBlock& b, const float* Scw) {
  float* h_pose = b.up(b.pose);
  for (size_t k = 0; k < b.s.K; k++) fsm_decompose_scw(Scw + 12 * k, h_pose + FSM_POSE_FLOATS * k);
}
// the job forms' job and tile segments from the (validated) job arrays
void fuse_pack_jobs(const FuseBlock& b, const int32_t* job_kf, const int32_t* job_pt0, const int32_t* job_n) {
  int32_t* h_job = b.up(b.job);
  int32_t* h_tile = b.up(b.tile);
  int32_t out0 = 0;
  size_t t = 0;
  for (size_t j = 0; j < b.s.J; j++) {
    h_job[FPM_JOB_INTS * j] = job_kf[j]; h_job[FPM_JOB_INTS * j + 1] = job_pt0[j];
    h_job[FPM_JOB_INTS * j + 2] = job_n[j]; h_job[FPM_JOB_INTS * j + 3] = out0;
    for (int32_t e = 0; e < job_n[j]; e += FPM_TILE, t++) { h_tile[2 * t] = (int32_t)j; h_tile[2 * t + 1] = e; }
    out0 += job_n[j];
  }
}

// One call from the validated arguments on: the counters zeroed and nothing launched for empty work; otherwise the block, the upload (pack: the form's own segments),
// one workgroup per tile of a job or per (keyframe, tile of points), the download and the caller's outputs.  A resident form's caller holds the store's reader lock
// until this returns.  CCM_DBG=fuse: the call's three host phases on stderr as "[tag] ..." (scripts/fuse_sim3_profile.py, fuse_pose_profile.py and kfstore_profile.py
// read them); the clock is read whether or not they are printed.
template <class Pack>
int fuse_stage_run(ccm_ctx* ctx, const char* me, const char* tag, void (*kernel)(FuseArgs), const FuseShape& s, const FuseCall& c, const FuseKfs& kf, Pack pack) {
  FuseBlock b(s);
  for (size_t i = 0; i < b.C; i++) c.n_valid[i] = c.n_hit[i] = 0;
  if (b.W == 0) return CCM_OK;
  if (int rc = ccm_staged_begin(ctx, b, me)) return rc;
  const Clock::time_point t0 = Clock::now();
  FuseArgs a = fuse_stage_inputs(b, c, kf);
  pack(b);
  const Clock::time_point t1 = Clock::now();
  if (int rc = ccm_staged_upload(ctx, b)) return rc;
  // K * tiles <= K * P + K workgroups: K * P <= INT32_MAX holds, and so does the grid limit for every K and P a map has; the jobs' tiles fpm_check_jobs bounds
  const uint64_t groups = b.jobs ? (uint64_t)s.T : (uint64_t)s.K * (uint64_t)a.tiles;
  if (groups > (uint64_t)INT32_MAX) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + "too many workgroups");
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(FPM_TILE), 0, ctx->stream, a);
  CCM_HIP_CHECK(ctx, hipGetLastError());
  if (int rc = ccm_staged_download(ctx, b)) return rc;
  const Clock::time_point t2 = Clock::now();
  b.get(b.n_valid, c.n_valid); b.get(b.n_hit, c.n_hit); b.get(b.table, c.table);
  if (c.uv) b.get(b.uv, c.uv);
  if (ccm_dbg("fuse")) {
    const double unpack_us = us_between(t2, Clock::now());
    char jobs[48] = "";
    if (b.jobs) snprintf(jobs, sizeof jobs, " J=%zu pairs=%zu", s.J, s.N);
    fprintf(stderr, "[%s] K=%zu P=%zu%s pack_us=%.1f device_us=%.1f unpack_us=%.1f up_bytes=%zu down_bytes=%zu\n", tag, s.K, s.P, jobs, us_between(t0, t1),
            us_between(t1, t2), unpack_us, b.up_bytes(), b.down_bytes());
  }
  return CCM_OK;
}

#define FUSE_REFUSE(why) return ccm_set_error(ctx, CCM_E_ARG, std::string(me) + (why))

}  // namespace

extern "C" int ccm_fuse_sim3_eval(ccm_ctx* ctx, int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
                                  const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* Scw, int nlevels,
                                  const float* scale_factors, float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist,
                                  const float* max_dist, const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_fuse_sim3_eval: ";
  if (const char* why = fsm_check_args(K, P, feat_off, cell_off, cell_idx, nlevels, th)) FUSE_REFUSE(why);
  const size_t F = K ? (size_t)feat_off[K] : 0;
  if (const char* why = fsm_check_kf_pointers(K, P, kf_rec, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit,
                                              fsm_feats_ok(F, feat_xy, feat_octave, feat_desc)))
    FUSE_REFUSE(why);
  return fuse_stage_run(ctx, me, "fuse", fuse_sim3_kernel, {FB_FLAT, (size_t)K, F, (size_t)P, (size_t)nlevels, 0, 0, 0, 0, uv != nullptr},
                        {nlevels, scale_factors, nullptr, logScaleFactor, th, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv},
                        {kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, nullptr, nullptr}, [&](const FuseBlock& b) { fuse_pack_scw(b, Scw); });
}

extern "C" int ccm_fuse_pose_eval(ccm_ctx* ctx, int K, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
                                  const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx, const float* pose, int nlevels,
                                  const float* scale_factors, const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos,
                                  const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf,
                                  const int32_t* job_pt0, const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_fuse_pose_eval: ";
  if (const char* why = fsm_check_args(K, P, feat_off, cell_off, cell_idx, nlevels, th)) FUSE_REFUSE(why);
  int64_t total = 0, tiles = 0;
  if (const char* why = fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles)) FUSE_REFUSE(why);
  const size_t F = K ? (size_t)feat_off[K] : 0;
  if (const char* why = fsm_check_job_pointers(K, P, J, total, true, kf_rec, pose, scale_factors, inv_level_sigma2, pos, normal, min_dist, max_dist, pt_desc, table,
                                               n_valid, n_hit, fsm_feats_ok(F, feat_xy, feat_octave, feat_desc)))
    FUSE_REFUSE(why);
  return fuse_stage_run(ctx, me, "fuse_pose", fuse_pose_kernel,
                        {FB_FLAT | FB_JOBS | FB_CHI2, (size_t)K, F, (size_t)P, (size_t)nlevels, (size_t)J, (size_t)tiles, (size_t)total, 0, uv != nullptr},
                        {nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv},
                        {kf_rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, nullptr, nullptr},
                        [&](const FuseBlock& b) { b.put(b.pose, pose); fuse_pack_jobs(b, job_kf, job_pt0, job_n); });
}

extern "C" int ccm_fuse_sim3_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int K, const int64_t* keys, const float* Scw, int nlevels, const float* scale_factors,
                                           float logScaleFactor, float th, int P, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                                           const uint8_t* pt_desc, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_fuse_sim3_eval_resident: ";
  if (int rc = fuse_store_ok(ctx, st, me)) return rc;
  if (const char* why = fsm_check_scalars(K, P, nlevels, th)) FUSE_REFUSE(why);
  if (const char* why = fsm_check_kf_pointers(K, P, keys, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, true)) FUSE_REFUSE(why);
  std::shared_lock<std::shared_mutex> lk(st->mu);   // from the key lookup to the end of the download: no slot read here is reused meanwhile
  std::vector<int32_t> slots;
  if (int rc = fuse_store_slots(ctx, st, K, keys, me, &slots)) return rc;
  return fuse_stage_run(ctx, me, "fuse_resident", fuse_sim3_resident_kernel, {0, (size_t)K, 0, (size_t)P, (size_t)nlevels, 0, 0, 0, 0, uv != nullptr},
                        {nlevels, scale_factors, nullptr, logScaleFactor, th, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv},
                        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st, slots.data()}, [&](const FuseBlock& b) { fuse_pack_scw(b, Scw); });
}

extern "C" int ccm_fuse_pose_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int K, const int64_t* keys, const float* pose, int nlevels, const float* scale_factors,
                                           const float* inv_level_sigma2, float logScaleFactor, float th, int P, const float* pos, const float* normal,
                                           const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J, const int32_t* job_kf, const int32_t* job_pt0,
                                           const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_fuse_pose_eval_resident: ";
  if (int rc = fuse_store_ok(ctx, st, me)) return rc;
  if (const char* why = fsm_check_scalars(K, P, nlevels, th)) FUSE_REFUSE(why);
  int64_t total = 0, tiles = 0;
  if (const char* why = fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles)) FUSE_REFUSE(why);
  if (const char* why = fsm_check_job_pointers(K, P, J, total, true, keys, pose, scale_factors, inv_level_sigma2, pos, normal, min_dist, max_dist, pt_desc, table,
                                               n_valid, n_hit, true))
    FUSE_REFUSE(why);
  std::shared_lock<std::shared_mutex> lk(st->mu);
  std::vector<int32_t> slots;
  if (int rc = fuse_store_slots(ctx, st, K, keys, me, &slots)) return rc;
  return fuse_stage_run(ctx, me, "fuse_pose_resident", fuse_pose_resident_kernel,
                        {FB_JOBS | FB_CHI2, (size_t)K, 0, (size_t)P, (size_t)nlevels, (size_t)J, (size_t)tiles, (size_t)total, 0, uv != nullptr},
                        {nlevels, scale_factors, inv_level_sigma2, logScaleFactor, th, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv},
                        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st, slots.data()},
                        [&](const FuseBlock& b) { b.put(b.pose, pose); fuse_pack_jobs(b, job_kf, job_pt0, job_n); });
}

extern "C" int ccm_sim3_project_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int K, const int64_t* keys, const float* Scw, const int32_t* skip_off,
                                              const uint8_t* feat_skip, int nlevels, const float* scale_factors, float logScaleFactor, float th, int P, const float* pos,
                                              const float* normal, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, uint32_t* table,
                                              int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_sim3_project_eval_resident: ";
  if (int rc = fuse_store_ok(ctx, st, me)) return rc;
  if (const char* why = fsm_check_scalars(K, P, nlevels, th)) FUSE_REFUSE(why);
  if (const char* why = fsm_check_kf_pointers(K, P, keys, Scw, scale_factors, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, true)) FUSE_REFUSE(why);
  std::shared_lock<std::shared_mutex> lk(st->mu);
  std::vector<int32_t> slots;
  if (int rc = fuse_store_slots(ctx, st, K, keys, me, &slots)) return rc;
  std::vector<int32_t> kf_n((size_t)K);
  for (int k = 0; k < K; k++) kf_n[k] = st->h_n[(size_t)slots[k]];
  if (const char* why = fsm_check_skip(K, skip_off, feat_skip, kf_n.data())) FUSE_REFUSE(why);
  return fuse_stage_run(ctx, me, "sim3_project", proj_sim3_resident_kernel,
                        {FB_MASK, (size_t)K, 0, (size_t)P, (size_t)nlevels, 0, 0, 0, K > 0 ? (size_t)skip_off[K] : 0, uv != nullptr},
                        {nlevels, scale_factors, nullptr, logScaleFactor, th, pos, normal, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv},
                        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st, slots.data()},
                        [&](const FuseBlock& b) { b.put(b.skip_off, skip_off); b.put(b.skip, feat_skip); fuse_pack_scw(b, Scw); });
}

extern "C" int ccm_sim3_pair_eval_resident(ccm_ctx* ctx, ccm_kfstore* st, int K, const int64_t* keys, int nlevels, const float* scale_factors, float logScaleFactor,
                                           float th, int P, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* pt_desc, int J,
                                           const int32_t* job_kf, const float* job_K4, const float* job_src_pose, const float* job_T, const int32_t* job_pt0,
                                           const int32_t* job_n, uint32_t* table, int32_t* n_valid, int32_t* n_hit, float* uv) {
  if (!ctx) return CCM_E_ARG;
  const char* const me = "ccm_sim3_pair_eval_resident: ";
  if (int rc = fuse_store_ok(ctx, st, me)) return rc;
  if (const char* why = fsm_check_scalars(K, P, nlevels, th)) FUSE_REFUSE(why);
  int64_t total = 0, tiles = 0;
  if (const char* why = fpm_check_jobs(J, K, P, job_kf, job_pt0, job_n, &total, &tiles)) FUSE_REFUSE(why);
  if (const char* why = fsm_check_pair_jobs(J, job_K4, job_src_pose, job_T)) FUSE_REFUSE(why);
  if (const char* why = fsm_check_job_pointers(K, P, J, total, false, keys, nullptr, scale_factors, nullptr, pos, nullptr, min_dist, max_dist, pt_desc, table, n_valid,
                                               n_hit, true))
    FUSE_REFUSE(why);
  std::shared_lock<std::shared_mutex> lk(st->mu);
  std::vector<int32_t> slots;
  if (int rc = fuse_store_slots(ctx, st, K, keys, me, &slots)) return rc;
  return fuse_stage_run(ctx, me, "sim3_pair", sim3_pair_resident_kernel,
                        {FB_JOBS | FB_PAIR, (size_t)K, 0, (size_t)P, (size_t)nlevels, (size_t)J, (size_t)tiles, (size_t)total, 0, uv != nullptr},
                        {nlevels, scale_factors, nullptr, logScaleFactor, th, pos, nullptr, min_dist, max_dist, pt_desc, table, n_valid, n_hit, uv},
                        {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st, slots.data()}, [&](const FuseBlock& b) {
                          ssm_pack_jobs(J, job_K4, job_src_pose, job_T, b.up(b.pose));
                          fuse_pack_jobs(b, job_kf, job_pt0, job_n);
                        });
}
