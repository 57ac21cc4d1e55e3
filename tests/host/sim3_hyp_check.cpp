// sim3_hyp_check.cpp — the per-hypothesis lines of ccm_slam_amd/csrc/sim3_ransac_math.h (what the kernel of sim3ransac.hip runs) compiled for the
// host, on hypotheses written by tests/test_sim3_ransac_cpu.py: argv[1] = input file, argv[2] = output file.
// in  (little-endian int32 / float32): K, Ntot, H, fix_scale | pt_off[K+1] | X1[3 Ntot] | X2[3 Ntot] | K1[4K] | K2[4K] | thr1[Ntot] | thr2[Ntot] |
//     hyp_cand[H] | hyp_idx[3H]
// out: per hypothesis n_inl (int32), rts (13 float32), then the inlier flags of its candidate's points (one byte each)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sim3_ransac_math.h"

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  if (fread(hdr, 4, 4, f) != 4) return 2;
  const int K = hdr[0], Nt = hdr[1], H = hdr[2], fix = hdr[3];
  std::vector<int32_t> pt_off, hc, hi;
  std::vector<float> X1, X2, K1, K2;
  std::vector<uint32_t> t1, t2;
  if (!rd(f, pt_off, K + 1) || !rd(f, X1, 3 * (size_t)Nt) || !rd(f, X2, 3 * (size_t)Nt) || !rd(f, K1, 4 * (size_t)K) || !rd(f, K2, 4 * (size_t)K) ||
      !rd(f, t1, Nt) || !rd(f, t2, Nt) || !rd(f, hc, H) || !rd(f, hi, 3 * (size_t)H))
    return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (int h = 0; h < H; h++) {
    const int c = hc[h], p0 = pt_off[c], N = pt_off[c + 1] - p0;
    float x1[3][3], x2[3][3];
    for (int j = 0; j < 3; j++)
      for (int r = 0; r < 3; r++) { x1[j][r] = X1[3 * (p0 + hi[3 * h + j]) + r]; x2[j][r] = X2[3 * (p0 + hi[3 * h + j]) + r]; }
    S3Hyp hy;
    s3_compute_sim3(x1, x2, fix != 0, hy);
    std::vector<uint8_t> in(N);
    int32_t n = 0;
    for (int i = 0; i < N; i++) {
      in[i] = s3_inlier(hy, &X1[3 * (p0 + i)], &X2[3 * (p0 + i)], &K1[4 * c], &K2[4 * c], t1[p0 + i], t2[p0 + i]) ? 1 : 0;
      n += in[i];
    }
    float rts[13];
    for (int i = 0; i < 9; i++) rts[i] = hy.R[i];
    for (int i = 0; i < 3; i++) rts[9 + i] = hy.t[i];
    rts[12] = hy.s;
    fwrite(&n, 4, 1, o);
    fwrite(rts, 4, 13, o);
    fwrite(in.data(), 1, N, o);
  }
  fclose(o);
  return 0;
}
