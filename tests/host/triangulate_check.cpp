// triangulate_check.cpp — csrc/triangulate_math.h (the kernel's arithmetic) compiled for the host and run on a file of matches, for
// tests/test_triangulate_cpu.py.  in: int32 S, P, nlevels; float ratioFactor; cam1 (21 f32); cam2 (21 S); pair_off (S + 1 i32); xy (4 P f32);
// oct (2 P i32); sigma2_1, sf_1, sigma2_2, sf_2 (nlevels f32 each).  out: status (P bytes), x3d (3 P f32).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "triangulate_math.h"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto hdr = rd<int32_t>(f, 3);
  const int S = hdr[0], P = hdr[1], L = hdr[2];
  const float ratio = rd<float>(f, 1)[0];
  const auto cam1 = rd<float>(f, TRI_CAM_FLOATS), cam2 = rd<float>(f, (size_t)TRI_CAM_FLOATS * S);
  const auto off = rd<int32_t>(f, S + 1);
  const auto xy = rd<float>(f, 4 * (size_t)P);
  const auto oct = rd<int32_t>(f, 2 * (size_t)P);
  const auto s1 = rd<float>(f, L), f1 = rd<float>(f, L), s2 = rd<float>(f, L), f2 = rd<float>(f, L);
  fclose(f);
  std::vector<uint8_t> status(P);
  std::vector<float> x3d(3 * (size_t)P);
  TriCam c1;
  memcpy(&c1, cam1.data(), sizeof c1);
  for (int s = 0; s < S; s++) {
    TriCam c2;
    memcpy(&c2, cam2.data() + (size_t)TRI_CAM_FLOATS * s, sizeof c2);
    for (int i = off[s]; i < off[s + 1]; i++)
      status[i] = (uint8_t)tri_pair(c1, c2, xy[4 * i], xy[4 * i + 1], oct[2 * i], xy[4 * i + 2], xy[4 * i + 3], oct[2 * i + 1], s1.data(), f1.data(), s2.data(), f2.data(),
                                    ratio, &x3d[3 * (size_t)i]);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(status.data(), 1, status.size(), o);
  fwrite(x3d.data(), sizeof(float), x3d.size(), o);
  fclose(o);
  return 0;
}
