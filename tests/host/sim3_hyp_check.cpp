// sim3_hyp_check.cpp — the per-hypothesis lines of ccm_slam_amd/csrc/sim3_ransac_math.h (what the kernel of sim3ransac.hip runs) compiled for the
// host and walked by ransac_wave.h's host walk, on hypotheses written by tests/test_sim3_ransac_cpu.py: argv[1] = input file, argv[2] = output file.
// in  (little-endian int32 / float32): K, Ntot, H, fix_scale | pt_off[K+1] | X1[3 Ntot] | X2[3 Ntot] | K1[4K] | K2[4K] | thr1[Ntot] | thr2[Ntot] |
//     hyp_cand[H] | hyp_idx[3H]
// out: per hypothesis n_inl (int32), rts (13 float32), then the inlier flags of its candidate's points (one byte each)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ransac_wave.h"
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
  std::vector<int32_t> n_inl(H), mask_off(H + 1);
  std::vector<float> rts(13 * (size_t)H);
  int64_t words = 0;
  if (ransac_check_hyps<3>(K, pt_off.data(), H, hc.data(), hi.data(), mask_off.data(), &words, true)) return 2;
  std::vector<uint32_t> mask((size_t)words);
  ransac_eval_host<Sim3HypForm>(Sim3RansacArgs{K, H, fix != 0, pt_off.data(), X1.data(), X2.data(), K1.data(), K2.data(), t1.data(), t2.data(), hc.data(), hi.data(),
                                           mask_off.data(), n_inl.data(), rts.data(), mask.data()});
  for (int h = 0; h < H; h++) {
    const int N = pt_off[hc[h] + 1] - pt_off[hc[h]];
    std::vector<uint8_t> in(N);
    for (int i = 0; i < N; i++) in[i] = mask[mask_off[h] + (i >> 5)] >> (i & 31) & 1u;
    fwrite(&n_inl[h], 4, 1, o);
    fwrite(&rts[13 * (size_t)h], 4, 13, o);
    fwrite(in.data(), 1, N, o);
  }
  fclose(o);
  return 0;
}
