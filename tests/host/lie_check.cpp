// lie_check.cpp — ccm_slam_amd/csrc/test_lie_ops.h (every function of ba_math.h / sim3_math.h behind one switch) on the CPU, as a stand-alone program that
// tests/test_lie_math_cpu.py builds with -fsanitize=address,undefined and runs over the case file it writes: the in-domain tables, the out-of-domain cases (zero
// quaternion, s <= 0, theta = pi, NaN entries, singular systems) and the raw libm arguments.  Every item is evaluated in heap blocks of exactly 48 and 40 doubles,
// so a read or write past an op's layout is an error here; the outputs beyond the op's own count must keep the value they started with, and the flag word is 0 or 1.
// File: int32 blocks; per block int32 op, int32 outputs, int32 n, then n * 48 doubles.
#include "test_lie_ops.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: lie_check <case file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t blocks = 0;
  if (!read_all(f, &blocks, 4) || blocks < 1) { fprintf(stderr, "bad header\n"); return 2; }
  const double kStart = -12345.678;
  long items = 0, nonfinite = 0;
  for (int b = 0; b < blocks; b++) {
    int32_t h[3];
    if (!read_all(f, h, sizeof(h)) || h[1] < 1 || h[1] > kLieFlag || h[2] < 1) { fprintf(stderr, "bad block %d\n", b); return 2; }
    const int op = h[0], n_out = h[1], n = h[2];
    for (int i = 0; i < n; i++) {
      std::unique_ptr<double[]> in(new double[kLieIn]), out(new double[kLieOut]);
      if (!read_all(f, in.get(), kLieIn * sizeof(double))) { fprintf(stderr, "short block %d\n", b); return 2; }
      for (int k = 0; k < kLieOut; k++) out[k] = kStart;
      if (!lie_eval(op, in.get(), out.get())) { fprintf(stderr, "block %d: unknown op %d\n", b, op); return 1; }
      for (int k = n_out; k < kLieFlag; k++)
        if (out[k] != kStart) { fprintf(stderr, "block %d op %d item %d: output %d written\n", b, op, i, k); return 1; }
      if (out[kLieFlag] != 0.0 && out[kLieFlag] != 1.0) { fprintf(stderr, "block %d op %d item %d: flag %g\n", b, op, i, out[kLieFlag]); return 1; }
      if (out[kLieFlag] == 0.0) {   // only ba_spd6_inv returns false, and then it leaves Inv as it was
        if (op != LIE_SPD6_INV) { fprintf(stderr, "block %d op %d item %d: flag 0\n", b, op, i); return 1; }
        for (int k = 0; k < n_out; k++)
          if (out[k] != kStart) { fprintf(stderr, "block %d item %d: Inv[%d] written on a false return\n", b, i, k); return 1; }
      }
      for (int k = 0; k < n_out; k++) nonfinite += !(out[k] - out[k] == 0.0);
      items++;
    }
  }
  char extra;
  if (fread(&extra, 1, 1, f) != 0) { fprintf(stderr, "trailing bytes\n"); return 2; }
  fclose(f);
  if (lie_eval(LIE_N_OPS, nullptr, nullptr) || lie_eval(-1, nullptr, nullptr)) { fprintf(stderr, "an unknown op was accepted\n"); return 1; }
  printf("lie ops ok: %d blocks, %ld items, %ld non-finite outputs\n", blocks, items, nonfinite);
  return 0;
}
