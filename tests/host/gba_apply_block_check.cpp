// gba_apply_block_check.cpp — GbaApplyBlock of csrc/stage_blocks.h on the CPU (tests/test_gba_apply_block_cpu.py builds this with -fsanitize=address,undefined).
// Both forms of ccm_gba_apply_map and n_pt == 0: every segment's offset against the segments in front of it, the alignment of the doubles, the two copied
// ranges, and every segment filled (or read) to its declared length in a malloc'd block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "stage_blocks.h"

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)
#define EXPECT_EQ(a, b) do { const size_t _a = (a), _b = (b); if (_a != _b) { printf("FAIL line %d: %s = %zu, %s = %zu\n", __LINE__, #a, _a, #b, _b); g_fail++; } } while (0)

struct Check {
  GbaApplyBlock& b;
  unsigned char* h;
  std::vector<char> filled;
  size_t o = 0;   // bytes, rounded up to words behind every segment
  explicit Check(GbaApplyBlock& blk) : b(blk) {
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
  template <class T> void up(const StagedSeg<T>& s, size_t count) {
    seg(s, count);
    EXPECT_EQ((size_t)((unsigned char*)b.up(s) - h) % alignof(T), 0);
    EXPECT(s.off >= b.up_begin() && s.off + s.count * sizeof(T) <= b.up_begin() + b.up_bytes());
    std::vector<T> src(count + 1);
    memset(src.data(), 0xff, count * sizeof(T));
    b.put(s, src.data());
    for (size_t i = 0; i < count * sizeof(T); i++) filled[s.off - b.up_begin() + i] = 1;
  }
  template <class T> void down(const StagedSeg<T>& s, size_t count) {
    seg(s, count);
    EXPECT_EQ((size_t)((const unsigned char*)b.down(s) - h) % alignof(T), 0);
    EXPECT(s.off >= b.down_begin() && s.off + s.count * sizeof(T) <= b.down_begin() + b.down_bytes());
    std::vector<T> dst(count + 1);
    b.get(s, dst.data());
  }
};

// C, L: cameras and landmarks of the host form, 0 0 in the handle form
static void gba_apply(size_t K, size_t P, size_t C, size_t L, size_t NT, size_t NL) {
  GbaApplyBlock b(K, P, C, L, NT, NL);
  Check c(b);
  c.up(b.cam_qt, 7 * C); c.up(b.pt_xyz, 3 * L);
  EXPECT_EQ(c.o, 8 * (7 * C + 3 * L));                                    // the doubles lead
  c.up(b.Tcw_old, 12 * K); c.up(b.Twc_old, 12 * K); c.up(b.pos, 3 * P);
  c.up(b.kf_parent, K); c.up(b.kf_cam, K); c.up(b.pt_vert, P); c.up(b.pt_ref, P);
  c.up(b.tree_kf, NT); c.up(b.lvl_off, NT ? NL + 1 : 0);
  const size_t n_in = 8 * (7 * C + 3 * L) + 4 * (24 * K + 3 * P + 2 * K + 2 * P + NT + (NT ? NL + 1 : 0));
  EXPECT_EQ(c.o, n_in);
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), n_in);
  for (size_t i = 0; i < c.filled.size(); i++)                             // what the stage did not write is zero: no pad in this block
    if (c.h[i] != (c.filled[i] ? 0xff : 0)) { printf("FAIL: host byte %zu of the upload is 0x%02x\n", i, c.h[i]); g_fail++; break; }
  c.down(b.T_new, 12 * K); c.down(b.Twc_new, 12 * K); c.down(b.pos_out, 3 * P); c.down(b.status, P);
  const size_t n_out = 4 * (24 * K + 3 * P) + ((P + 3) & ~(size_t)3);
  EXPECT_EQ(c.o, n_in + n_out);
  EXPECT_EQ(b.down_begin(), n_in); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), n_in + n_out);
  EXPECT_EQ(b.pin_bytes(), n_in > n_out ? n_in : n_out);
}

int main() {
  for (size_t K : {1, 2, 65})
    for (size_t P : {0, 1, 3, 4, 5, 197})
      for (size_t NT : {0, 1, 7}) {
        if (NT >= K) continue;
        const size_t NL = NT ? (NT > 3 ? 3 : 1) : 0;
        gba_apply(K, P, K + 1, P / 2, NT, NL);     // host form; P / 2 == 0: no landmarks
        gba_apply(K, P, 1, 0, NT, NL);
        gba_apply(K, P, 0, 0, NT, NL);             // handle form: the state segments have zero length
      }
  if (g_fail) { printf("gba apply block: %d failures\n", g_fail); return 1; }
  printf("gba apply block ok\n");
  return 0;
}
