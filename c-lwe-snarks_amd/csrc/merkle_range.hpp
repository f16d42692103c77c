// merkle_range.hpp -- host only, plain C++: the host side of mfh_merkle_range_rows and mfh_merkle_range_rows_cut (merkle.hip), the records of a key RANGE
// [a, b] of an indexed table (merkle_keys.hpp has keys and their words; include/mfhip.h the data model).
//
// The links of [a, b] are the live records with hi >= a and lo <= b: in a well-formed table the records (p, k_1), (k_1, k_2), .., (k_n, s) around and between
// the members k_1 < .. < k_n of the range, p < a and b < s.  The device selects them in table order (k_range_flags and the inert search's scan and select),
// makes a dense array of their keys (k_range_keys) and puts slots and keys into key order (k_range_order); the host checks that they chain (range_status).
//
// range_scratch: the device scratch of one call, byte offsets as functions of (depth, max_links, key_bytes):
//   mask    4 words of 64 flags a workgroup of 256 records (k_inert_flags' layout)          nb * 32 bytes, nb = ceil(2^depth / 256)
//   count   a word a workgroup, its exclusive prefix sums after the scan                    nb * 4
//   slots   the matching slots in table order                                               max_links * 4
//   dense   lo | hi of every selected slot as 2 kw words, in table order                    max_links * 2 kw * 4
//   total   the number of links of the whole table                                          4
//   order   the selected slots in key order                                                 max_links * 4
//   okeys   lo | hi of every selected slot as 2 kw words, in key order                      max_links * 2 kw * 4
// total | order | okeys lie together: they come back in ONE copy (result_bytes), as the inert search's total | slots do.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "merkle_keys.hpp"

namespace mf {

constexpr uint32_t kMaxRangeLinks = 1u << 16;  // k_range_order compares every pair of links: quadratic

struct RangeScratch {
  uint32_t nb;  // workgroups of 256 records
  size_t mask_at, count_at, slots_at, dense_at, total_at, order_at, okeys_at, bytes;
};

// the bytes of max_links slots' keys as words: lo | hi, kw words each
inline size_t range_keys_bytes(uint32_t max_links, uint32_t key_bytes) { return (size_t)max_links * 2 * key_words(key_bytes) * 4; }

inline RangeScratch range_scratch(uint32_t depth, uint32_t max_links, uint32_t key_bytes) {
  RangeScratch s{};
  s.nb = (uint32_t)((((uint64_t)1 << depth) + 255) / 256);
  s.mask_at = 0;
  s.count_at = s.mask_at + (size_t)s.nb * 4 * 8;
  s.slots_at = s.count_at + (size_t)s.nb * 4;
  s.dense_at = s.slots_at + (size_t)max_links * 4;
  s.total_at = s.dense_at + range_keys_bytes(max_links, key_bytes);
  s.order_at = s.total_at + 4;
  s.okeys_at = s.order_at + (size_t)max_links * 4;
  s.bytes = s.okeys_at + range_keys_bytes(max_links, key_bytes);
  return s;
}

// the bytes of total | order | okeys, what one copy brings back
inline size_t range_result_bytes(uint32_t max_links, uint32_t key_bytes) { return 4 + (size_t)max_links * 4 + range_keys_bytes(max_links, key_bytes); }

inline int words_compare(const uint32_t *x, const uint32_t *y, uint32_t kw) {
  for (uint32_t j = 0; j < kw; j++)
    if (x[j] != y[j]) return x[j] < y[j] ? -1 : 1;
  return 0;
}

// the key_bytes bytes of a key out of its words: the inverse of key_to_words
inline void words_to_key(const uint32_t *w, uint32_t key_bytes, uint8_t *key) {
  for (uint32_t b = 0; b < key_bytes; b++) key[b] = (uint8_t)(w[b / 4] >> (8 * (3 - b % 4)));
}

// Do the n ordered links okeys (n x 2 kw words, lo | hi a link) chain across [a, b] (kw words each)?  0: n >= 1, lo_0 < a, hi_i == lo_i+1 for every i and
// hi_n-1 > b -- the links tile an open range that covers [a, b].  2 otherwise, and *first <- the first link at which a check fails (0 for n = 0 and for
// lo_0 >= a; i + 1 where hi_i != lo_i+1; n - 1 for hi_n-1 <= b).  Reads n * 2 kw words of okeys and kw words of a and of b.
inline int range_status(const uint32_t *okeys, uint32_t n, uint32_t kw, const uint32_t *a, const uint32_t *b, uint32_t *first = nullptr) {
  uint32_t at = 0;
  bool good = n >= 1 && words_compare(okeys, a, kw) < 0;
  for (uint32_t i = 0; good && i + 1 < n; i++)
    if (words_compare(okeys + ((size_t)2 * i + 1) * kw, okeys + ((size_t)2 * i + 2) * kw, kw) != 0) {
      good = false;
      at = i + 1;
    }
  if (good && words_compare(okeys + ((size_t)2 * (n - 1) + 1) * kw, b, kw) <= 0) {
    good = false;
    at = n - 1;
  }
  if (first) *first = good ? 0 : at;
  return good ? 0 : 2;
}

}  // namespace mf
