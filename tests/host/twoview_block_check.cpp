// twoview_block_check.cpp — TwoViewRansacBlock and TwoViewCheckRtBlock of csrc/stage_blocks.h on the CPU (tests/test_twoview_block_cpu.py builds this with
// -fsanitize=address,undefined).  Every segment's offset against the segments in front of it, the two copied ranges, and every segment filled (or read) to its
// declared length in a malloc'd block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
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
  std::vector<char> filled;
  size_t o = 0;   // bytes, rounded up to words behind every segment
  explicit Check(StagedBlock& blk) : b(blk) {
    const char* why = b.finish();
    if (why) { printf("FAIL: %s\n", why); g_fail++; }
    h = (unsigned char*)malloc(b.pin_bytes() ? b.pin_bytes() : 1);
    memset(h, 0xa5, b.pin_bytes());
    b.bind(h, nullptr);
    filled.assign(b.up_bytes(), 0);
  }
  ~Check() { free(h); }
  template <class T> void seg(const StagedSeg<T>& s, size_t count) {
    const size_t al = alignof(T) > 4 ? alignof(T) : 4;
    o = (o + al - 1) & ~(al - 1);
    EXPECT_EQ(s.off, o);
    EXPECT_EQ(s.count, count);
    o = (o + count * sizeof(T) + 3) & ~(size_t)3;
  }
  template <class T> void up(const StagedSeg<T>& s, size_t count, bool through_put) {
    seg(s, count);
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
  template <class T> void work(const StagedSeg<T>& s, size_t count) { seg(s, count); }
  template <class T> void down(const StagedSeg<T>& s, size_t count) {
    seg(s, count);
    EXPECT(s.off >= b.down_begin() && s.off + s.count * sizeof(T) <= b.down_begin() + b.down_bytes());
    std::vector<T> dst(count + 1);
    b.get(s, dst.data());
  }
  void uploaded_bytes() {   // what the stage did not write is zero
    for (size_t i = 0; i < filled.size(); i++)
      if (h[i] != (filled[i] ? 0xff : 0)) { printf("FAIL: host byte %zu of the upload is 0x%02x\n", i, h[i]); g_fail++; break; }
  }
};

static void ransac(size_t N, size_t H) {
  TwoViewRansacBlock b(N, H);
  Check c(b);
  const size_t words = (N + 31) / 32;
  EXPECT_EQ(b.words, words);
  c.up(b.xy1, 2 * N, true); c.up(b.xy2, 2 * N, true); c.up(b.pn1, 2 * N, true); c.up(b.pn2, 2 * N, true);
  c.up(b.T, 27, false); c.up(b.sets, 8 * H, true);
  const size_t n_in = 4 * (8 * N + 27 + 8 * H);
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in);
  c.uploaded_bytes();
  c.work(b.H12, 9 * H);
  c.down(b.scoreH, H); c.down(b.scoreF, H); c.down(b.H21, 9 * H); c.down(b.F21, 9 * H); c.down(b.maskH, words * H); c.down(b.maskF, words * H);
  const size_t n_out = 4 * (20 * H + 2 * words * H);
  EXPECT_EQ(b.down_begin(), n_in + 36 * H); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + 36 * H + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in > n_out ? n_in : n_out);
}

static void check_rt(size_t N, size_t Q) {
  TwoViewCheckRtBlock b(N, Q);
  Check c(b);
  c.up(b.xy1, 2 * N, true); c.up(b.xy2, 2 * N, true); c.up(b.rec, 27 * Q, true); c.up(b.K, 9, true); c.up(b.inl, (N + 31) / 32, true);
  const size_t n_in = 4 * (4 * N + 27 * Q + 9 + (N + 31) / 32);
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in);
  c.uploaded_bytes();
  c.down(b.x3d, 3 * N * Q); c.down(b.cosp, N * Q); c.down(b.status, N * Q);
  const size_t n_out = 16 * N * Q + ((N * Q + 3) & ~(size_t)3);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in > n_out ? n_in : n_out);
}

int main() {
  for (size_t N : {8, 9, 31, 32, 33, 64, 65, 1000})
    for (size_t H : {1, 2, 63, 64, 65, 200}) ransac(N, H);
  for (size_t N : {1, 2, 3, 5, 31, 32, 33, 1000})
    for (size_t Q : {1, 3, 4, 8}) check_rt(N, Q);
  if (g_fail) { printf("twoview blocks: %d failures\n", g_fail); return 1; }
  printf("twoview blocks ok\n");
  return 0;
}
