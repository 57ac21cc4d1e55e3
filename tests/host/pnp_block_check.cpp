// pnp_block_check.cpp — PnpRansacBlock of csrc/stage_blocks.h on the CPU (tests/test_pnp_block_cpu.py builds this with -fsanitize=address,undefined).  Every
// segment's offset against the segments in front of it (the f64 segments on 8 bytes), the two copied ranges, and every segment filled (or read) to its declared
// length in a malloc'd block of exactly pin_bytes(), so that an overrun is the sanitizer's to report.
#include "block_check.h"

static void ransac(size_t K, size_t Nt, size_t H, size_t nw) {
  PnpRansacBlock b(K, Nt, H, nw);
  Check c(b);
  c.up(b.cam, 4 * K, true); c.up(b.pt_off, K + 1, true); c.up(b.P3Dw, 3 * Nt, true); c.up(b.P2D, 2 * Nt, true); c.up(b.max_err, Nt, true);
  c.up(b.hyp_cand, H, true); c.up(b.hyp_idx, 4 * H, true); c.up(b.mask_off, H + 1, true);
  const size_t n_in = 32 * K + 4 * (K + 1 + 6 * Nt + 5 * H + H + 1);
  EXPECT_EQ(c.o, n_in);
  const size_t rt_at = (n_in + 7) & ~(size_t)7;   // the pad in front of the f64 poses travels with the upload, as zeros
  EXPECT_EQ(b.up_begin(), 0); EXPECT_EQ(b.up_bytes(), rt_at);
  c.uploaded_bytes();
  c.down(b.Rt, 12 * H); c.down(b.n_inl, H); c.down(b.mask, nw);
  const size_t n_out = 96 * H + words(4 * H + 4 * nw);
  EXPECT_EQ(b.Rt.off, rt_at); EXPECT_EQ(b.Rt.off % 8, 0); EXPECT_EQ(b.cam.off % 8, 0);
  EXPECT_EQ(b.down_begin(), rt_at); EXPECT_EQ(b.down_bytes(), n_out);
  EXPECT_EQ(b.bytes(), rt_at + n_out);
}

int main() {
  for (size_t K : {1, 2, 3, 10})
    for (size_t N : {4, 5, 31, 32, 33, 64, 65, 200})
      for (size_t H : {1, 2, 4, 5, 300}) ransac(K, K * N, H, H * ((N + 31) / 32));
  if (g_fail) { printf("pnp block: %d failures\n", g_fail); return 1; }
  printf("pnp block ok\n");
  return 0;
}
