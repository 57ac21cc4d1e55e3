// fuse_sim3_block_check.cpp — FuseSim3Block of csrc/stage_blocks.h on the CPU (tests/test_fuse_sim3_block_cpu.py builds this with -fsanitize=address,undefined).
// Every segment's offset against the segments in front of it, the two copied ranges, and every segment filled (or read) to its declared length in a malloc'd
// block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "stage_blocks.h"

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)
#define EXPECT_EQ(a, b) do { const size_t _a = (a), _b = (b); if (_a != _b) { printf("FAIL line %d: %s = %zu, %s = %zu\n", __LINE__, #a, _a, #b, _b); g_fail++; } } while (0)

struct Check {
  StagedBlock& b;
  unsigned char* h;
  std::vector<char> filled;   // 1: written by the stage, 2: declared as zeros
  size_t o = 0;               // bytes, rounded up to words behind every segment
  explicit Check(StagedBlock& blk) : b(blk) {
    const char* why = b.finish();
    if (why) { printf("FAIL: %s\n", why); g_fail++; }
    h = (unsigned char*)malloc(b.pin_bytes() ? b.pin_bytes() : 1);
    memset(h, 0xa5, b.pin_bytes());
    b.bind(h, nullptr);
    filled.assign(b.up_bytes(), 0);
  }
  ~Check() { free(h); }
  template <class T> void seg(const StagedSeg<T>& s, size_t count, size_t align) {
    size_t al = alignof(T) > 4 ? alignof(T) : 4;
    if (align > al) al = align;
    o = (o + al - 1) & ~(al - 1);
    EXPECT_EQ(s.off, o);
    EXPECT_EQ(s.count, count);
    o = (o + count * sizeof(T) + 3) & ~(size_t)3;
  }
  template <class T> void up(const StagedSeg<T>& s, size_t count, bool through_put, size_t align = 0) {
    seg(s, count, align);
    EXPECT(s.off >= b.up_begin() && s.off + s.count * sizeof(T) <= b.up_begin() + b.up_bytes());
    if (through_put) {
      std::vector<T> src(count + 1);
      memset(src.data(), 0xff, count * sizeof(T));
      b.put(s, src.data());
    } else {
      memset(b.up(s), 0xff, count * sizeof(T));     // a segment the stage writes in place
    }
    for (size_t i = 0; i < count * sizeof(T); i++) filled[s.off - b.up_begin() + i] = 1;
  }
  template <class T> void zero_and_down(const StagedSeg<T>& s, size_t count) {   // uploaded as zeros, downloaded
    seg(s, count, 0);
    EXPECT(s.off >= b.up_begin() && s.off + s.count * sizeof(T) <= b.up_begin() + b.up_bytes());
    EXPECT(s.off >= b.down_begin() && s.off + s.count * sizeof(T) <= b.down_begin() + b.down_bytes());
    std::vector<T> dst(count + 1);
    b.get(s, dst.data());
  }
  template <class T> void down(const StagedSeg<T>& s, size_t count) {
    seg(s, count, 0);
    EXPECT(s.off >= b.down_begin() && s.off + s.count * sizeof(T) <= b.down_begin() + b.down_bytes());
    std::vector<T> dst(count + 1);
    b.get(s, dst.data());
  }
  void uploaded_bytes() {   // what the stage did not write is zero
    for (size_t i = 0; i < filled.size(); i++)
      if (h[i] != (filled[i] ? 0xff : 0)) { printf("FAIL: host byte %zu of the upload is 0x%02x\n", i, h[i]); g_fail++; break; }
  }
};

static size_t words(size_t bytes) { return (bytes + 3) & ~(size_t)3; }

static void fuse(size_t K, size_t F, size_t P, size_t L, bool uv) {
  FuseSim3Block b(K, F, P, L, uv);
  Check c(b);
  c.up(b.kdesc, 32 * F, true, 16); c.up(b.pdesc, 32 * P, true, 16);
  c.up(b.rec, FSM_REC_FLOATS * K, true); c.up(b.pose, FSM_POSE_FLOATS * K, false);
  c.up(b.feat_off, K + 1, true); c.up(b.cell_off, K * (FSM_CELLS + 1), true);
  c.up(b.kxy, 2 * F, true); c.up(b.cell_idx, F, false); c.up(b.koct, F, true);
  c.up(b.scale_factors, L, true);
  c.up(b.pos, 3 * P, true); c.up(b.normal, 3 * P, true); c.up(b.dmin, P, true); c.up(b.dmax, P, true);
  const size_t n_in = 32 * F + 32 * P + 4 * (25 * K + K + 1 + K * (FSM_CELLS + 1) + 2 * F + L + 8 * P) + words(2 * F) + words(F);
  EXPECT_EQ(c.o, n_in);
  c.zero_and_down(b.n_valid, K); c.zero_and_down(b.n_hit, K);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in + 8 * K);
  c.uploaded_bytes();
  c.down(b.table, K * P); c.down(b.uv, uv ? 2 * K * P : 0);
  const size_t n_out = 8 * K + 4 * K * P + (uv ? 8 * K * P : 0);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in + 8 * K > n_out ? n_in + 8 * K : n_out);
}

int main() {
  for (int uv = 0; uv < 2; uv++) {
    fuse(0, 0, 0, 8, uv); fuse(0, 0, 5, 8, uv); fuse(3, 1001, 0, 8, uv);
    fuse(1, 0, 1, 1, uv);                                       // a keyframe without features
    for (size_t K : {1, 2, 3, 8})
      for (size_t F : {1, 2, 3, 5, 333, 1000})
        for (size_t P : {1, 63, 64, 65, 257, 2500}) fuse(K, K * F - (K > 1), P, K == 3 ? 16 : 8, uv);   // (one keyframe of several without features' worth less)
  }
  fuse(300, 300 * 957, 40, 8, true);
  if (g_fail) { printf("fuse_sim3 block: %d failures\n", g_fail); return 1; }
  printf("fuse_sim3 block ok\n");
  return 0;
}
