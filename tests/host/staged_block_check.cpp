// staged_block_check.cpp — csrc/staged_block.h and ten declarations of csrc/stage_blocks.h on the CPU (tests/test_staged_block_cpu.py builds this with
// -fsanitize=address,undefined): the five map stages that were declared first, and the five blocks of six entry points of hamming.hip and frame.hip (the CSR
// block serves two of them).  Every offset and total is compared with the closed formulas and the put() sequences that the wrappers held before the blocks were declared (4-byte
// words; copied here as they stood, the five later ones by their element counts), every aligned segment is checked, the optional outputs are declared both
// ways, and the host side is filled to the declared lengths in a malloc'd block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "stage_blocks.h"

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)
#define EXPECT_EQ(a, b) do { const size_t _a = (a), _b = (b); if (_a != _b) { printf("FAIL line %d: %s = %zu, %s = %zu\n", __LINE__, #a, _a, #b, _b); g_fail++; } } while (0)

// A bound block on a host buffer of exactly pin_bytes().  seg() checks a segment's word offset against the walk `o` of the old wrapper and advances it; up()
// also fills the segment's host view to its declared length, down() reads it to its declared length.
struct Check {
  StagedBlock& b;
  unsigned char* h;
  std::vector<char> filled;
  size_t o = 0;
  explicit Check(StagedBlock& blk) : b(blk) {
    const char* why = b.finish();
    if (why) { printf("FAIL: %s\n", why); g_fail++; }
    h = (unsigned char*)malloc(b.pin_bytes() ? b.pin_bytes() : 1);
    memset(h, 0xa5, b.pin_bytes());
    b.bind(h, nullptr);
    filled.assign(b.up_bytes(), 0);
  }
  ~Check() { free(h); }
  template <class T> void seg(const StagedSeg<T>& s, size_t words, size_t align = 4) {
    EXPECT_EQ(s.off, 4 * o);
    EXPECT_EQ(s.off % align, 0);
    EXPECT_EQ(s.off % alignof(T), 0);
    o += words;
  }
  template <class T> void up(const StagedSeg<T>& s, size_t words, bool zero = false, size_t align = 4) {
    seg(s, words, align);
    EXPECT_EQ((size_t)((unsigned char*)b.up(s) - h) % align, 0);
    EXPECT(s.off >= b.up_begin() && s.off + s.count * sizeof(T) <= b.up_begin() + b.up_bytes());
    if (zero) return;
    memset(b.up(s), 0xff, s.count * sizeof(T));
    for (size_t i = 0; i < s.count * sizeof(T); i++) filled[s.off - b.up_begin() + i] = 1;
  }
  template <class T> void down(const StagedSeg<T>& s, size_t words, size_t align = 4) {
    seg(s, words, align);
    EXPECT_EQ((size_t)((const unsigned char*)b.down(s) - h) % align, 0);
    EXPECT(s.off >= b.down_begin() && s.off + s.count * sizeof(T) <= b.down_begin() + b.down_bytes());
    std::vector<T> dst(s.count + 1);
    b.get(s, dst.data());
  }
  // what the stage did not write is zero: SB_ZERO segments, the pad of byte segments, alignment pads
  void pads_are_zero() {
    for (size_t i = 0; i < filled.size(); i++)
      if (h[i] != (filled[i] ? 0xff : 0)) { printf("FAIL: host byte %zu of the upload is 0x%02x\n", i, h[i]); g_fail++; return; }
  }
  void ranges(size_t up0, size_t n_up, size_t down0, size_t n_down, size_t total) {
    EXPECT_EQ(b.up_begin(), 4 * up0); EXPECT_EQ(b.up_bytes(), 4 * n_up);
    EXPECT_EQ(b.down_begin(), 4 * down0); EXPECT_EQ(b.down_bytes(), 4 * n_down);
    EXPECT_EQ(b.bytes(), 4 * total);
    EXPECT_EQ(b.pin_bytes(), 4 * (n_up > n_down ? n_up : n_down));
    pads_are_zero();
  }
};

static void sim3_ransac(size_t K, size_t Nt, size_t H, size_t words) {
  const size_t n_in = (K + 1) + 6 * Nt + 8 * K + 2 * Nt + 4 * H + (H + 1);
  const size_t n_out = 14 * H + words;
  Sim3RansacBlock b(K, Nt, H, words);
  Check c(b);
  c.up(b.pt_off, K + 1); c.up(b.X1, 3 * Nt); c.up(b.X2, 3 * Nt); c.up(b.K1, 4 * K); c.up(b.K2, 4 * K); c.up(b.thr1, Nt); c.up(b.thr2, Nt);
  c.up(b.hyp_cand, H); c.up(b.hyp_idx, 3 * H); c.up(b.mask_off, H + 1);
  EXPECT_EQ(c.o, n_in);
  c.down(b.n_inl, H); c.down(b.rts, 13 * H); c.down(b.mask, words);
  EXPECT_EQ(c.o, n_in + n_out);
  c.ranges(0, n_in, n_in, n_out, n_in + n_out);
}

static void triangulate(size_t P, size_t S, size_t L) {
  const size_t n_in = (4 * P + TRI_CAM_FLOATS * (S + 1) + 4 * L + 2 * P + 3) & ~(size_t)3;
  const size_t n_out = 3 * P + (P + 3) / 4;
  TriBlock b(P, S, L);
  Check c(b);
  c.up(b.xy, 4 * P, false, 16); c.up(b.cam1, TRI_CAM_FLOATS); c.up(b.cam2, TRI_CAM_FLOATS * S);
  c.up(b.sigma2_1, L); c.up(b.sf_1, L); c.up(b.sigma2_2, L); c.up(b.sf_2, L); c.up(b.oct, P); c.up(b.grp, P);
  EXPECT_EQ(c.o, 4 * P + TRI_CAM_FLOATS * (S + 1) + 4 * L + 2 * P);
  c.o = n_in;
  c.down(b.x3d, 3 * P, 16); c.down(b.status, (P + 3) / 4);
  EXPECT_EQ(c.o, n_in + n_out);
  c.ranges(0, n_in, n_in, n_out, n_in + n_out);
}

static void sim3_correct(size_t K, size_t KO, size_t P, size_t L, size_t NO, bool loop) {
  const size_t n_in_d = 8 + (loop ? 0 : 16 * K);
  const size_t n_in = (2 * n_in_d + 12 + (loop ? 12 * K : 0) + 3 * KO + L + 8 * P + KO + 2 * P + (P ? P + 1 : 0) + NO + 2 * P + 1) & ~(size_t)1;
  const size_t n_out = (2 * 16 * K + 15 * K + 8 * P + 1) & ~(size_t)1;
  S3cBlock b(K, KO, P, L, NO, loop);
  Check c(b);
  c.up(b.Scw, 16, !loop, 8); c.up(b.S_non_in, loop ? 0 : 16 * K, false, 8); c.up(b.S_cor_in, loop ? 0 : 16 * K, false, 8);
  c.up(b.Twc, 12, !loop); c.up(b.Tiw, loop ? 12 * K : 0); c.up(b.c_old, 3 * KO); c.up(b.scale_factors, L);
  c.up(b.pos, 3 * P); c.up(b.normal_in, 3 * P); c.up(b.dmin_in, P); c.up(b.dmax_in, P);
  c.up(b.kf_rank, KO); c.up(b.owner, P); c.up(b.owner_rank, P); c.up(b.obs_off, P ? P + 1 : 0); c.up(b.obs_kf, NO); c.up(b.ref_kf, P); c.up(b.ref_level, P);
  EXPECT_EQ((c.o + 1) & ~(size_t)1, n_in);
  c.o = n_in;
  if (loop) { c.down(b.S_non, 16 * K, 8); c.down(b.S_cor, 16 * K, 8); } else { c.seg(b.S_non, 16 * K, 8); c.seg(b.S_cor, 16 * K, 8); }
  EXPECT_EQ(c.o, n_in + 32 * K);
  c.down(b.T_new, 12 * K); c.down(b.c_new, 3 * K); c.down(b.pos_out, 3 * P); c.down(b.normal_out, 3 * P); c.down(b.dmin_out, P); c.down(b.dmax_out, P);
  EXPECT_EQ((c.o + 1) & ~(size_t)1, n_in + n_out);
  c.o = n_in + n_out;
  c.seg(b.S_swi, 16 * K, 8);
  // the epilogue form skips the caller's own tables: its download starts 32 K words into the output block
  const size_t skip_out = loop ? 0 : 32 * K;
  c.ranges(0, n_in, n_in + skip_out, n_out - skip_out, n_in + n_out + 2 * 8 * K);
}

static void covis(size_t K, size_t A, size_t P, size_t NL, size_t NO, size_t C) {
  const size_t n_in = A + (K + 1) + NL + (P + 1) + NO;
  const size_t n_work = 6 * K + (K + 1) + 2 * C;
  const size_t n_out = 4 + K + 3 * (K + 1) + 6 * C;
  CovisBlock b(K, A, P, NL, NO, C);
  Check c(b);
  c.up(b.order_key, A); c.up(b.list_off, K + 1); c.up(b.list_pt, NL); c.up(b.obs_off, P + 1, P == 0); c.up(b.obs_kf, NO);
  EXPECT_EQ(c.o, n_in);
  c.seg(b.row_size, K); c.seg(b.n_ge, K); c.seg(b.fb_col, K); c.seg(b.extra_cnt, K); c.seg(b.cursor, K); c.seg(b.chg, K); c.seg(b.extra_off, K + 1);
  c.seg(b.extra_src, C); c.seg(b.extra_w, C);
  EXPECT_EQ(c.o, n_in + n_work);
  c.down(b.hdr, 4); c.down(b.flags, K); c.down(b.row_off, K + 1); c.down(b.fw_off, K + 1); c.down(b.ord_off, K + 1);
  c.down(b.col, C); c.down(b.count, C); c.down(b.fw_col, C); c.down(b.fw_w, C); c.down(b.ord_kf, C); c.down(b.ord_w, C);
  EXPECT_EQ(c.o, n_in + n_work + n_out);
  c.ranges(0, n_in, n_in + n_work, n_out, n_in + n_work + n_out);
}

static void kfcull(size_t K, size_t P, size_t NL, size_t NO) {
  const size_t EW = (K + 31) / 32, WL = (NL + 3) / 4, WO = (NO + 3) / 4;
  const size_t n_out = 4 + 3 * K + 2 * P;
  const size_t n_work = 4 * K + EW + P;
  const size_t n_in = K + (K + 1) + NL + (P + 1) + NO + WL + 2 * WO;
  const size_t n_up = n_out + n_work + n_in;
  KfcullBlock b(K, P, NL, NO);
  Check c(b);
  c.up(b.hdr, 4, true); c.up(b.verdict, K, true); c.up(b.n_mps, K, true); c.up(b.n_red, K, true); c.up(b.gone, P); c.up(b.nobs, P);
  EXPECT_EQ(c.o, n_out);
  c.up(b.sums, 4 * K, true); c.up(b.erased, EW, true); c.up(b.stamp, P, true);
  EXPECT_EQ(c.o, n_out + n_work);
  c.up(b.cand_flags, K); c.up(b.list_off, K + 1); c.up(b.list_pt, NL); c.up(b.obs_off, P + 1, P == 0); c.up(b.obs_kf, NO);
  c.up(b.list_level, WL); c.up(b.obs_level, WO); c.up(b.obs_bad, WO);
  EXPECT_EQ(c.o, n_up);
  c.seg(b.slot, WL);
  // the outputs are the head of the uploaded range: read them back from there
  c.o = 0;
  c.down(b.hdr, 4); c.down(b.verdict, K); c.down(b.n_mps, K); c.down(b.n_red, K); c.down(b.gone, P); c.down(b.nobs, P);
  c.ranges(0, n_up, 0, n_out, n_up + WL);
}

// ---- the tracked frame's and LocalMapping's entry points: the element counts of their former hand-packed layouts, without the 256-byte rounding those had ----

// ccm_hamming_dense_best2: q 32 Q bytes | t 32 T bytes; the partials of ccm_hamming_dense_best2_dev, 3 n_split Q ints; out 3 Q ints
static void hamming_dense(size_t Q, size_t T, size_t n_split) {
  const size_t n_in = 8 * Q + 8 * T, n_work = 3 * n_split * Q, n_out = 3 * Q;
  HammingDenseBlock b(Q, T, n_split);
  Check c(b);
  c.up(b.q, 8 * Q, false, 16); c.up(b.t, 8 * T, false, 16);
  EXPECT_EQ(c.o, n_in);
  c.seg(b.part, n_work);
  c.down(b.best_idx, Q); c.down(b.best_dist, Q); c.down(b.second_dist, Q);
  c.ranges(0, n_in, n_in + n_work, n_out, n_in + n_work + n_out);
}

// ccm_hamming_csr(_multi): q | t | cand_off (Q + 1) | q_tbase (Q, _multi only) | cand_idx (n_cand); out cand_dist (n_cand u16) | 3 Q ints.  An output that is
// not asked for takes no room and moves nothing.
static void hamming_csr(size_t Q, size_t T, size_t n_cand, bool multi, bool want_dist, bool want_best) {
  const size_t n_in = 8 * Q + 8 * T + (Q + 1) + (multi ? Q : 0) + n_cand;
  const size_t w_dist = want_dist ? (n_cand + 1) / 2 : 0, w_best = want_best ? Q : 0;
  HammingCsrBlock b(Q, T, n_cand, multi, want_dist, want_best);
  Check c(b);
  c.up(b.q, 8 * Q, false, 16); c.up(b.t, 8 * T, false, 16); c.up(b.cand_off, Q + 1); c.up(b.q_tbase, multi ? Q : 0); c.up(b.cand_idx, n_cand);
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.q_tbase.count, multi ? Q : 0); EXPECT_EQ(b.cand_dist.count, want_dist ? n_cand : 0); EXPECT_EQ(b.best_idx.count, w_best);
  c.down(b.cand_dist, w_dist); c.down(b.best_idx, w_best); c.down(b.best_dist, w_best); c.down(b.second_dist, w_best);
  c.ranges(0, n_in, n_in, w_dist + 3 * w_best, n_in + w_dist + 3 * w_best);
}

// ccm_bow_transform: desc 32 N bytes; out leaf (N) | nid (N)
static void bow_transform(size_t N) {
  BowTransformBlock b(N);
  Check c(b);
  c.up(b.desc, 8 * N, false, 16);
  c.down(b.leaf, N); c.down(b.nid, N);
  c.ranges(0, 8 * N, 8 * N, 2 * N, 10 * N);
}

// ccm_frame_frustum: P 3n | normal 3n | dmin n | dmax n (8n floats in);  u n | v n | cos n | level n | in_view n bytes (out)
static void frustum(size_t n) {
  FrustumBlock b(n);
  Check c(b);
  c.up(b.P, 3 * n); c.up(b.normal, 3 * n); c.up(b.dmin, n); c.up(b.dmax, n);
  EXPECT_EQ(c.o, 8 * n);
  c.down(b.u, n); c.down(b.v, n); c.down(b.cos, n); c.down(b.level, n); c.down(b.in_view, (n + 3) / 4);
  c.ranges(0, 8 * n, 8 * n, 4 * n + (n + 3) / 4, 12 * n + (n + 3) / 4);
}

// ccm_update_normal_and_depth: [pos 3np | kf_center 3nk | scale n_levels | obs_off np+1 | obs_kf no | ref_kf np | ref_level np] -> [normal 3np | dmin np | dmax np];
// the outputs travel both ways
static void normal_depth(size_t np, size_t nk, size_t n_levels, size_t no) {
  const size_t in_words = 3 * np + 3 * nk + n_levels + (np + 1) + no + 2 * np, out_words = 5 * np;
  NormalDepthBlock b(np, nk, n_levels, no);
  Check c(b);
  c.up(b.pos, 3 * np); c.up(b.kf_center, 3 * nk); c.up(b.scale_factors, n_levels); c.up(b.obs_off, np + 1); c.up(b.obs_kf, no); c.up(b.ref_kf, np); c.up(b.ref_level, np);
  EXPECT_EQ(c.o, in_words);
  c.up(b.normal, 3 * np); c.up(b.dmin, np); c.up(b.dmax, np);
  EXPECT_EQ(c.o, in_words + out_words);
  c.o = in_words;
  c.down(b.normal, 3 * np); c.down(b.dmin, np); c.down(b.dmax, np);
  c.ranges(0, in_words + out_words, in_words, out_words, in_words + out_words);
}

int main() {
  for (size_t Q : {1, 3, 65})
    for (size_t T : {0, 1, 130})
      for (size_t n_split : {1, 3}) hamming_dense(Q, T, n_split);
  for (size_t Q : {1, 2, 7})
    for (size_t T : {0, 1, 9})
      for (size_t n_cand : {0, 1, 2, 5})       // an odd n_cand: the 16-bit distances end on half a word in front of the int32 outputs
        for (int form = 0; form < 8; form++) hamming_csr(Q, T, T ? n_cand : 0, form & 1, form & 2, form & 4);
  for (size_t N : {1, 5}) bow_transform(N);
  for (size_t n : {1, 4, 7, 130}) frustum(n);
  for (size_t np : {1, 3})
    for (size_t nk : {0, 2})
      for (size_t no : {0, 1, 6}) normal_depth(np, nk, 8, nk ? no : 0);
  for (size_t H : {0, 1, 5})
    for (size_t K : {1, 3}) sim3_ransac(K, 3 * K + 14 * (K - 1), H, H * 2 + (H > 1));
  for (size_t P : {0, 1, 3, 4, 5, 130})
    for (size_t S : {1, 2, 3})                // 21 (S + 1) words of cameras: an odd count in front of the 16-byte-aligned outputs when S is even
      for (size_t L : {1, 8}) triangulate(P, S, L);
  for (int loop = 0; loop < 2; loop++)
    for (size_t K : {1, 2})
      for (size_t P : {0, 3})
        for (size_t L : {1, 8})               // L = 1 with KO = K leaves an odd word count in front of the 8-byte-aligned Sim3 tables
          for (size_t KO : {K, K + 2}) sim3_correct(K, KO, P, L, P ? 2 * P + 1 : 0, loop != 0);
  for (size_t K : {1, 2, 70})
    for (size_t P : {0, 9})
      for (size_t C : {0, 1, 64}) {
        covis(K, K + 3, P, 0, P ? 3 * P : 0, C);
        covis(K, K, P, 5 * K, P ? 3 * P : 0, C);
      }
  for (size_t K : {1, 33})
    for (size_t P : {0, 5})
      for (size_t NL : {0, 1, 3, 4, 5})
        for (size_t NO : {0, 1, 3, 4, 5}) kfcull(K, P, NL, P ? NO : 0);
  // a device-only segment between two uploaded ones: no single copy carries the upload
  {
    StagedBlock b;
    b.add<float>(3, SB_COPY); b.add<float>(2, SB_WORK); b.add<int32_t>(1, SB_GEN); b.add<float>(4, SB_OUT);
    EXPECT(b.finish() != nullptr);
  }
  // ... and the same for the download, an unknown role, a segment that is work and output at once
  {
    StagedBlock b;
    b.add<float>(3, SB_COPY); b.add<float>(4, SB_OUT); b.add<float>(2, SB_WORK); b.add<float>(4, SB_OUT);
    EXPECT(b.finish() != nullptr);
    StagedBlock r0, r1, r2;
    r0.add<float>(1, 0); EXPECT(r0.finish() != nullptr);
    r1.add<float>(1, SB_WORK | SB_OUT); EXPECT(r1.finish() != nullptr);
    r2.add<float>(1, SB_COPY | SB_ZERO); EXPECT(r2.finish() != nullptr);
  }
  // a download that starts on a word while one of its segments needs 8 bytes: the pinned side would misalign it
  {
    StagedBlock b;
    b.add<float>(1, SB_COPY); b.add<float>(1, SB_OUT); b.add<double>(1, SB_OUT);
    EXPECT(b.finish() != nullptr);
  }
  if (g_fail) { printf("staged block: %d failures\n", g_fail); return 1; }
  printf("staged block ok\n");
  return 0;
}
