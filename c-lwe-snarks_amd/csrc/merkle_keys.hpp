// merkle_keys.hpp -- host only, plain C++: the query side of mfh_merkle_absent_rows (merkle.hip).
//
// A key is key_bytes bytes, 1 <= key_bytes <= 32, compared as a big-endian unsigned integer: memcmp order.  The device compares WORDS: key_words(key_bytes)
// = ceil(key_bytes / 4) uint32, word j holding bytes 4 j .. 4 j + 3 with byte 4 j in its top 8 bits, a last partial word left-aligned and zero-padded.
// Keys of one key_bytes all carry the same padding, so the lexicographic order of their words is the memcmp order of their bytes.
//
// keys_prepare: the nq queries sorted (stable: equal keys keep their order), de-duplicated and converted to words -- what k_key_locate binary-searches.
// keys_scatter: the two result words per UNIQUE query that the kernel leaves (range record | present record, 0xFFFFFFFF = none) back to one index and one
// status per query, in the caller's order, through the permutation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace mf {

constexpr uint32_t kMaxKeyBytes = 32;
constexpr uint32_t kNoRecord = 0xFFFFFFFFu;

inline uint32_t key_words(uint32_t key_bytes) { return (key_bytes + 3) / 4; }

inline void key_to_words(const uint8_t *key, uint32_t key_bytes, uint32_t *w) {
  for (uint32_t j = 0; j < key_words(key_bytes); j++) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; b++) v = v << 8 | (4 * j + b < key_bytes ? key[4 * j + b] : 0u);
    w[j] = v;
  }
}

// the all-zero and the all-0xFF key: never members, never queries
inline bool key_is_sentinel(const uint8_t *key, uint32_t key_bytes) {
  bool zero = true, ones = true;
  for (uint32_t b = 0; b < key_bytes; b++) {
    zero = zero && key[b] == 0x00;
    ones = ones && key[b] == 0xFF;
  }
  return zero || ones;
}

struct KeyPlan {
  uint32_t nu = 0;              // unique queries
  std::vector<uint32_t> order;  // order[j] = the query at sorted position j (equal keys: ascending query number)
  std::vector<uint32_t> slot;   // slot[k] = the position of query k among the unique sorted queries
  std::vector<uint32_t> words;  // nu x key_words(key_bytes), ascending
};

// query k is the key_bytes bytes at keys + k * stride
inline void keys_prepare(const uint8_t *keys, size_t stride, uint32_t key_bytes, uint32_t nq, KeyPlan &p) {
  const uint32_t kw = key_words(key_bytes);
  p.order.resize(nq);
  p.slot.resize(nq);
  for (uint32_t k = 0; k < nq; k++) p.order[k] = k;
  std::stable_sort(p.order.begin(), p.order.end(), [&](uint32_t a, uint32_t b) { return memcmp(keys + a * stride, keys + b * stride, key_bytes) < 0; });
  p.words.clear();
  p.words.reserve((size_t)nq * kw);
  p.nu = 0;
  for (uint32_t j = 0; j < nq; j++) {
    const uint8_t *key = keys + p.order[j] * stride;
    if (!j || memcmp(keys + p.order[j - 1] * stride, key, key_bytes)) {
      p.words.resize((size_t)(p.nu + 1) * kw);
      key_to_words(key, key_bytes, p.words.data() + (size_t)p.nu * kw);
      p.nu++;
    }
    p.slot[p.order[j]] = p.nu - 1;
  }
}

// res: nu range records, then nu present records.  status 1 (present) with the present record where there is one, else 0 (absent) with the range record,
// else 2 with kNoRecord
inline void keys_scatter(const KeyPlan &p, uint32_t nq, const uint32_t *res, uint32_t *index, uint8_t *status) {
  for (uint32_t k = 0; k < nq; k++) {
    const uint32_t range = res[p.slot[k]], present = res[p.nu + p.slot[k]];
    index[k] = present != kNoRecord ? present : range;
    status[k] = present != kNoRecord ? 1 : range != kNoRecord ? 0 : 2;
  }
}

}  // namespace mf
