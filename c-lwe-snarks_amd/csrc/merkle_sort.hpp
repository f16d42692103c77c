// merkle_sort.hpp -- plain C++, compiled by hipcc for the kernels of merkle.hip AND by a host compiler (tests/merkle_sort_host_check.cpp): the device sort of
// multi-word keys (key_sort: k_sort_tiles, k_sort_merge), its merge-path partition, and the scratch of the two calls built on it, mfh_merkle_load_keys and
// mfh_merkle_check_table (include/mfhip.h has the data model, merkle_keys.hpp keys and their words).
//
// An ENTRY is KW key words and one uint32 tag, KW + 1 consecutive words (KW = key_words(key_bytes) = 1 .. 8).  The order is lexicographic over all KW + 1
// words: keys ascending, the tag ascending on equal keys.  Tags are distinct, so the entries are totally ordered and the sorted array is ONE fixed permutation
// of the input, whatever order threads or workgroups run in.
//
// The sort.  k_sort_tiles sorts every tile of kSortTile entries in LDS (one workgroup a tile, bitonic); then sort_passes(n) launches of k_sort_merge, pass p
// merging neighbouring runs of kSortTile << p entries from one buffer into the other.  A workgroup of a merge pass owns kSortTile consecutive OUTPUT entries;
// as runs are multiples of the tile these lie in one pair of runs (a, b), between the diagonals d0 and d1 of that pair's merge.  merge_path(a, na, b, nb, d) is
// how many of the first d outputs come from a: the workgroup merges a[merge_path(d0), merge_path(d1)) with b[d0 - merge_path(d0), d1 - merge_path(d1)).
//
// Scratch, byte offsets as functions of (depth, n, key_bytes) -- n the keys of a load, or the most live records of a check (2^depth):
//   load_scratch    ent0 | ent1   the two buffers of the sort, n entries each                   n (kw + 1) 4 bytes each
//                   status        sentinel | duplicate rank | where0 | where1                    16 bytes
//   check_scratch   mask | count | slots | dense | total   range_scratch's, with max_links = n    (merkle_range.hpp)
//                   ent0 | ent1   the two buffers of the sort                                     n (kw + 1) 4 bytes each
//                   result        total | leaf | chain (64 bits) | node (64 bits)                 32 bytes, 8-byte aligned
//                   digests       SHA-256 of every slot's record                                  2^depth 32 bytes, 16-byte aligned
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MF_SORT_HD __host__ __device__ __forceinline__
#else
#define MF_SORT_HD inline
#endif

namespace mf {

constexpr uint32_t kSortTile = 1024;  // entries a tile: (8 + 1) words x 1 024 = 36 KiB of LDS at KW = 8

inline uint32_t sort_key_words(uint32_t key_bytes) { return (key_bytes + 3) / 4; }  // (merkle_keys.hpp's key_words: this header stands alone)
inline uint32_t sort_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kSortTile - 1) / kSortTile); }
// merge passes behind the tile sort: ceil(log2(tiles)), 0 for one tile or none
inline uint32_t sort_passes(uint32_t n) {
  uint32_t p = 0;
  while (((uint64_t)1 << p) < sort_tiles(n)) p++;
  return p;
}
inline size_t sort_buffer_bytes(uint32_t n, uint32_t key_bytes) { return (size_t)n * (sort_key_words(key_bytes) + 1) * 4; }

// x < y over the KW + 1 words of two entries
template <int KW>
MF_SORT_HD bool sort_less(const uint32_t *x, const uint32_t *y) {
  for (int j = 0; j <= KW; j++)
    if (x[j] != y[j]) return x[j] < y[j];
  return false;
}

// How many of the first `diag` entries of the merge of the sorted runs a (na entries) and b (nb entries) come from a, an entry of a going first where it
// equals one of b; diag <= na + nb.  A binary search along the diagonal: reads only a[m] with m < na and b[diag - 1 - m] with diag - 1 - m < nb.
template <int KW>
MF_SORT_HD uint32_t merge_path(const uint32_t *a, uint32_t na, const uint32_t *b, uint32_t nb, uint32_t diag) {
  uint32_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (sort_less<KW>(b + (size_t)(diag - 1 - m) * (KW + 1), a + (size_t)m * (KW + 1))) hi = m; else lo = m + 1;
  }
  return lo;
}

// The slice of one workgroup of a merge pass over n entries in runs of `run` (a multiple of kSortTile): outputs [out0, out0 + count) of the pair of runs
// a = [a_at, a_at + na), b = [a_at + na, a_at + na + nb), between the diagonals d0 and d0 + count of that pair.  (A last run without a partner: nb = 0.)
struct MergeSlice {
  uint32_t out0, count, a_at, na, nb, d0;
};
MF_SORT_HD MergeSlice merge_slice(uint32_t n, uint32_t run, uint32_t group) {
  MergeSlice s;
  s.out0 = group * kSortTile;
  const uint64_t base = (uint64_t)(s.out0 / (2 * (uint64_t)run)) * 2 * run, mid = base + run < n ? base + run : n, end = base + 2 * (uint64_t)run < n ? base + 2 * (uint64_t)run : n;
  s.a_at = (uint32_t)base;
  s.na = (uint32_t)(mid - base);
  s.nb = (uint32_t)(end - mid);
  s.d0 = s.out0 - s.a_at;
  s.count = s.na + s.nb - s.d0 < kSortTile ? s.na + s.nb - s.d0 : kSortTile;
  return s;
}

struct LoadScratch {
  size_t ent0_at, ent1_at, status_at, bytes;
};
inline LoadScratch load_scratch(uint32_t depth, uint32_t n, uint32_t key_bytes) {
  (void)depth;
  LoadScratch s{};
  s.ent0_at = 0;
  s.ent1_at = s.ent0_at + sort_buffer_bytes(n, key_bytes);
  s.status_at = s.ent1_at + sort_buffer_bytes(n, key_bytes);
  s.bytes = s.status_at + 16;
  return s;
}

struct CheckScratch {
  uint32_t nb;  // workgroups of 256 records
  size_t mask_at, count_at, slots_at, dense_at, total_at, ent0_at, ent1_at, result_at, digests_at, bytes;
};
inline CheckScratch check_scratch(uint32_t depth, uint32_t n, uint32_t key_bytes) {
  CheckScratch s{};
  s.nb = (uint32_t)((((uint64_t)1 << depth) + 255) / 256);
  s.mask_at = 0;
  s.count_at = s.mask_at + (size_t)s.nb * 4 * 8;
  s.slots_at = s.count_at + (size_t)s.nb * 4;
  s.dense_at = s.slots_at + (size_t)n * 4;
  s.total_at = s.dense_at + (size_t)n * 2 * sort_key_words(key_bytes) * 4;
  s.ent0_at = s.total_at + 4;
  s.ent1_at = s.ent0_at + sort_buffer_bytes(n, key_bytes);
  s.result_at = (s.ent1_at + sort_buffer_bytes(n, key_bytes) + 7) & ~(size_t)7;
  s.digests_at = (s.result_at + 32 + 15) & ~(size_t)15;
  s.bytes = s.digests_at + ((size_t)32 << depth);
  return s;
}

}  // namespace mf
