// ba_sort.h — the stable LSD radix sorts of the BA structure build (ba_build.hip, ba_structure.hip), with the rocPRIM path chosen by measured size.
//
// rocprim::radix_sort_pairs / radix_sort_keys pick one of three algorithms by size alone (device_radix_sort.hpp, radix_sort_impl):
//   n <= 1024                      one workgroup sorts everything (radix_sort_block_sort)
//   n <= merge_sort_limit (2^20)   block sort of 1024-item tiles, then log2(n / 1024) merge passes over the whole array (each a partition and a merge launch)
//   above                          onesweep: one histogram launch, then one pass per 8 key bits
// The 4-agent map has 954 782 observations, 9 % under the limit: its two observation-sized sorts paid ten merge passes where an 11-bit key needs two onesweep
// passes and a 29-bit key four.  A radix_sort_config whose MergeSortLimit is 0 takes the merge path out: single block up to 1024 items, onesweep above.  All
// three are stable, so the sorted arrays are the same whichever runs.
//
// Measured on MI355X (random keys, sort alone, microseconds; 8 of them are the timing's own):
//     n          u64 key 29 bits, int     u32 key 11 bits, int     u32 key 22 bits, u64 value
//                default   no merge       default   no merge       default   no merge
//     23 000        46        109            41         69            43          72     (a local window)
//     66 000         -          -            55         71             -           -     (S blocks of the 4-agent map)
//    200 000        78        114            67         72            74          78
//    262 000       112        121            99         75           109          80
//    270 000       135        122           117         73           127          80
//    573 000       165        130           140         77           150          87     (observations of the 3-agent map)
//    954 782       200        136           162         81           192          97     (observations of the 4-agent map)
// Onesweep costs 60 - 110 us however small the input (histogram, look-back), the merge path grows by a pass (two launches over everything) at every doubling,
// with one such step at 2^18 items; above it onesweep wins for every key width the build uses, below it it loses or ties.  So every call site takes it from
// kBaOnesweepFrom items on: on the 4-agent map the two observation-sized sorts (954 782), on its 64 k - 66 k block sorts and in a local window nothing changes.
// CCM_BA_SORT, read at every sort of ccm_ba_create: "merge" keeps rocPRIM's own choice everywhere (A / B runs), "onesweep" takes the merge path out at every
// size (tests/test_ba_structure_sorts_gpu.py: the small problems of the suite through the same code as the large maps).
#pragma once
#include <cstdlib>
#include <cstring>
#include <rocprim/rocprim.hpp>

constexpr size_t kBaOnesweepFrom = ((size_t)1 << 18) + 1;

using BaSortNoMerge = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;

inline bool ba_sort_onesweep(size_t n) {
  const char* s = getenv("CCM_BA_SORT");
  if (s && !strcmp(s, "merge")) return false;
  if (s && !strcmp(s, "onesweep")) return true;
  return n >= kBaOnesweepFrom;
}

// the two calls rocPRIM's interface asks for (size query, sort) share one body: `scratch` == nullptr asks for the size
template <typename K, typename V>
inline hipError_t ba_radix_sort_pairs(bool onesweep, void* scratch, size_t& bytes, rocprim::double_buffer<K>& kb, rocprim::double_buffer<V>& vb, unsigned n, unsigned bits,
                                      hipStream_t st) {
  return onesweep ? rocprim::radix_sort_pairs<BaSortNoMerge>(scratch, bytes, kb, vb, n, 0u, bits, st)
                  : rocprim::radix_sort_pairs(scratch, bytes, kb, vb, n, 0u, bits, st);
}
template <typename K>
inline hipError_t ba_radix_sort_keys(bool onesweep, void* scratch, size_t& bytes, rocprim::double_buffer<K>& kb, unsigned n, unsigned bits, hipStream_t st) {
  return onesweep ? rocprim::radix_sort_keys<BaSortNoMerge>(scratch, bytes, kb, n, 0u, bits, st) : rocprim::radix_sort_keys(scratch, bytes, kb, n, 0u, bits, st);
}
