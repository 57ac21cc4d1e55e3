// frame_math_check — csrc/frame_math.h compiled for the host, as host/ccm_host.cpp compiles it, behind a file interface: tests/test_frame_reference_cpu.py writes
// inputs, runs one mode and compares the output with tests/frame_reference.py and the oracle.  Built with the undefined-behaviour sanitizer and its
// float-cast-overflow check, so a float that no int holds reaching a conversion ends the program.
//   cell    in: FrameBounds (6 f32) | n x (x y)                                out: n i32 cells
//   range   in: FrameBounds (6 f32) | n x (u v r)                              out: n x (ok x0 x1 y0 y1) i32
//   frustum in: frame (24 f32) | nLevels, cosLimit (2 f32) | n x (P3 Pn3 dmin dmax)   out: n x (in_view u v level cos) as 32-bit words
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "frame_math.h"

static std::vector<float> read_all(const char* path) {
  std::vector<float> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  float buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(float), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  const std::vector<float> in = read_all(argv[2]);
  std::vector<int32_t> out;
  if (mode == "cell" || mode == "range") {
    if (in.size() < 6) return 3;
    const FrameBounds b{in[0], in[1], in[2], in[3], in[4], in[5]};
    const int w = mode == "cell" ? 2 : 3;
    const size_t n = (in.size() - 6) / w;
    for (size_t i = 0; i < n; i++) {
      const float* q = in.data() + 6 + w * i;
      if (w == 2) { out.push_back(frame_cell_of(b, q[0], q[1])); continue; }
      int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
      const bool ok = frame_cell_range(b, q[0], q[1], q[2], x0, x1, y0, y1);
      out.insert(out.end(), {ok ? 1 : 0, x0, x1, y0, y1});
    }
  } else if (mode == "frustum") {
    if (in.size() < 26) return 3;
    FrustumFrame f;
    memcpy(&f, in.data(), 24 * sizeof(float));
    f.nScaleLevels = (int)in[24];
    const float cosLimit = in[25];
    const size_t n = (in.size() - 26) / 8;
    for (size_t i = 0; i < n; i++) {
      const float* q = in.data() + 26 + 8 * i;
      float u = 0, v = 0, c = 0;
      int l = 0;
      const bool ok = frame_in_frustum(f, q, q + 3, q[6], q[7], cosLimit, u, v, l, c);
      if (!ok) { u = v = c = 0; l = 0; }
      int32_t w[5] = {ok ? 1 : 0, 0, 0, l, 0};
      memcpy(&w[1], &u, 4); memcpy(&w[2], &v, 4); memcpy(&w[4], &c, 4);
      out.insert(out.end(), w, w + 5);
    }
  } else {
    return 2;
  }
  FILE* f = fopen(argv[3], "wb");
  if (!f) return 4;
  if (!out.empty()) fwrite(out.data(), sizeof(int32_t), out.size(), f);
  fclose(f);
  return 0;
}
