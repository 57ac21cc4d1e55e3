// staged_block.h — the layout of a stage's staged device block.  Plain C++: no HIP, so that tests/host/staged_block_check.cpp checks it on the CPU.
//
// A stage declares its segments once, in device order; offsets, the block size and the two copied ranges follow from the declarations alone.  The block lives in
// the context's device scratch.  Its uploaded range is packed into the context's pinned block and goes up in ONE copy, its downloaded range comes back into the
// pinned block in ONE copy (both land at the pinned block's start).  ccm_staged_begin / _upload / _download (common.h) do the device side.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// What a segment is.  A segment that the kernels both receive and return (kfcull's gone / nobs) is SB_OUT together with what fills it.
enum : unsigned {
  SB_COPY = 1,   // input, copied from the caller: put()
  SB_GEN = 2,    // input, written by the stage through up()
  SB_ZERO = 4,   // uploaded as zeros
  SB_WORK = 8,   // device only: neither copied up nor down
  SB_OUT = 16,   // downloaded
};

template <class T>
struct StagedSeg { size_t off, count; };   // byte offset in the device block, elements

class StagedBlock {
 public:
  // One declaration per segment.  Segments start on a 4-byte word, on alignof(T), and on `align` bytes where more is needed (16 for float4 reads); a segment of
  // one-byte elements is padded to whole words.  count == 0 is legal.
  template <class T>
  StagedSeg<T> add(size_t count, unsigned role, size_t align = 0) {
    size_t al = alignof(T) > 4 ? alignof(T) : 4;
    if (align > al) al = align;
    const unsigned fill = role & (SB_COPY | SB_GEN | SB_ZERO | SB_WORK);
    if ((al & (al - 1)) || al % alignof(T) || (fill & (fill - 1)) || (role & ~31u) || !role || ((role & SB_WORK) && (role & SB_OUT))) fail("a bad segment declaration");
    if (n_ == kMax) { fail("too many segments"); return {end_, 0}; }
    const size_t off = (end_ + al - 1) & ~(al - 1);
    seg_[n_++] = Seg{off, count * sizeof(T), al, role};
    end_ = (off + count * sizeof(T) + 3) & ~(size_t)3;
    return {off, count};
  }
  // Closes the declaration: the copied ranges.  Returns nullptr, or why the declaration is not a staged block.  A range runs from its first segment to the start
  // of the first segment behind its last one, so the alignment pad in front of that segment travels with it.
  const char* finish() {
    range(SB_COPY | SB_GEN | SB_ZERO, up0_, up1_, "the uploaded segments are not contiguous");
    range(SB_OUT, down0_, down1_, "the downloaded segments are not contiguous");
    return err_;
  }
  size_t bytes() const { return end_; }   // the device block
  size_t up_begin() const { return up0_; }
  size_t up_bytes() const { return up1_ - up0_; }
  size_t down_begin() const { return down0_; }
  size_t down_bytes() const { return down1_ - down0_; }
  size_t pin_bytes() const { return up_bytes() > down_bytes() ? up_bytes() : down_bytes(); }
  void* host() const { return h_; }
  void* device() const { return d_; }
  // Binds the block to its two bases and prepares the host side of the upload: SB_ZERO segments, the pad of byte segments and the alignment pads are zeroed.
  void bind(void* host, void* dev) {
    h_ = (char*)host; d_ = (char*)dev;
    size_t at = up0_;   // the end of what the stage writes so far: everything between two such segments is zeroed
    for (int i = 0; i < n_; i++) {
      const Seg& g = seg_[i];
      if (g.off < up0_ || g.off >= up1_ || (g.role & SB_ZERO) || !g.bytes) continue;
      memset(h_ + at - up0_, 0, g.off - at);
      at = g.off + g.bytes;
    }
    memset(h_ + at - up0_, 0, up1_ - at);
  }
  // Typed views of a segment: on the device, in the pinned block before the upload, in the pinned block after the download.
  template <class T> T* dev(const StagedSeg<T>& s) const { return (T*)(d_ + s.off); }
  template <class T> T* up(const StagedSeg<T>& s) const { return (T*)(h_ + s.off - up0_); }
  template <class T> const T* down(const StagedSeg<T>& s) const { return (const T*)(h_ + s.off - down0_); }
  template <class T> void put(const StagedSeg<T>& s, const void* src) const { if (s.count) memcpy(up(s), src, s.count * sizeof(T)); }
  template <class T> void get(const StagedSeg<T>& s, void* dst) const { get(s, dst, s.count); }
  template <class T> void get(const StagedSeg<T>& s, void* dst, size_t count) const { if (count) memcpy(dst, down(s), count * sizeof(T)); }
 private:
  static constexpr int kMax = 32;
  struct Seg { size_t off, bytes, align; unsigned role; };
  void fail(const char* why) { if (!err_) err_ = why; }
  void range(unsigned roles, size_t& r0, size_t& r1, const char* why) {
    int first = -1, last = -1;
    for (int i = 0; i < n_; i++)
      if (seg_[i].role & roles) { if (first < 0) first = i; last = i; }
    r0 = r1 = 0;
    if (first < 0) return;
    r0 = seg_[first].off;
    r1 = last + 1 < n_ ? seg_[last + 1].off : end_;
    for (int i = first; i <= last; i++) {
      if (!(seg_[i].role & roles)) fail(why);
      if ((seg_[i].off - r0) % seg_[i].align) fail("a copied range starts below the alignment of one of its segments");   // the pinned side starts at 0
    }
  }
  Seg seg_[kMax];
  int n_ = 0;
  size_t end_ = 0, up0_ = 0, up1_ = 0, down0_ = 0, down1_ = 0;
  const char* err_ = nullptr;
  char *h_ = nullptr, *d_ = nullptr;
};
