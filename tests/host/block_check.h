// block_check.h — what fuse_sim3_block_check.cpp and fuse_pose_block_check.cpp share: the failure counter and Check, which walks a staged block's segments in
// their declared order, checks every offset against the segments in front of it, and fills (or reads) every segment to its declared length in a malloc'd block of
// exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#pragma once
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
