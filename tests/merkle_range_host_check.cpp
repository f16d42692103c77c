// The host half of the range reads (mfh_merkle_range_rows, mfh_merkle_range_rows_cut) in csrc/merkle_range.hpp -- the scratch layout and the chain check of
// the ordered links -- as a program of its own (tests/test_merkle_range_host_cpu.py builds it with the address and undefined-behaviour sanitizers, runs it
// and compares what it prints with values computed independently).  Every line of standard input is one of
//   scratch <depth> <max_links> <key_bytes>
//       prints  scratch <nb> <mask_at> <count_at> <slots_at> <dense_at> <total_at> <order_at> <okeys_at> <bytes> <result_bytes>
//   status <key_bytes> <a> <b> <n> [<lo> <hi>] x n            keys in hex, key_bytes bytes each
//       prints  status <0|2> <first>      mf::range_status over the links' words (mf::key_to_words)
//               keys <hex of lo | hi of every link>   the words turned back into bytes (mf::words_to_key)
// The links' words, the two bounds' words and the bytes written back live in heap allocations of exactly their sizes, so a read or write one word outside
// is a heap overflow the address sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "merkle_range.hpp"

template <class T> static T *exact(size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (!p) exit(3);
  return p;
}

static int refuse() {
  fprintf(stderr, "merkle_range_host_check: expected `scratch <depth in 1 .. 24> <max_links <= 65536> <key_bytes in 1 .. 32>` or `status <key_bytes> <a> <b> <n> "
                  "<lo> <hi> ..` with keys of key_bytes bytes in hex\n");
  return 2;
}

// key_bytes bytes out of 2 key_bytes hex digits; false when the token is anything else
static bool unhex(const char *tok, unsigned key_bytes, uint8_t *out) {
  if (!tok || strlen(tok) != 2 * (size_t)key_bytes) return false;
  for (unsigned b = 0; b < key_bytes; b++) {
    unsigned v = 0;
    if (sscanf(tok + 2 * b, "%2x", &v) != 1) return false;
    out[b] = (uint8_t)v;
  }
  return true;
}

int main() {
  char buf[1 << 16];
  while (fgets(buf, sizeof buf, stdin)) {
    std::vector<char *> tok;
    for (char *t = strtok(buf, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
    if (tok.empty()) return refuse();
    if (!strcmp(tok[0], "scratch")) {
      if (tok.size() != 4) return refuse();
      const unsigned depth = (unsigned)atoi(tok[1]), max_links = (unsigned)atoi(tok[2]), key_bytes = (unsigned)atoi(tok[3]);
      if (depth < 1 || depth > 24 || max_links > mf::kMaxRangeLinks || key_bytes < 1 || key_bytes > mf::kMaxKeyBytes) return refuse();
      const mf::RangeScratch s = mf::range_scratch(depth, max_links, key_bytes);
      printf("scratch %u %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s.nb, s.mask_at, s.count_at, s.slots_at, s.dense_at, s.total_at, s.order_at, s.okeys_at, s.bytes,
             mf::range_result_bytes(max_links, key_bytes));
    } else if (!strcmp(tok[0], "status")) {
      if (tok.size() < 5) return refuse();
      const unsigned key_bytes = (unsigned)atoi(tok[1]), n = (unsigned)atoi(tok[4]);
      if (key_bytes < 1 || key_bytes > mf::kMaxKeyBytes || tok.size() != 5 + 2 * (size_t)n) return refuse();
      const uint32_t kw = mf::key_words(key_bytes);
      std::vector<uint8_t> keys((size_t)(2 + 2 * n) * key_bytes);  // a | b | lo, hi of every link: parsed before anything is allocated
      for (unsigned i = 0; i < 2 + 2 * n; i++)
        if (!unhex(tok[i < 2 ? 2 + i : 3 + i], key_bytes, keys.data() + (size_t)i * key_bytes)) return refuse();
      uint32_t *a = exact<uint32_t>(kw), *b = exact<uint32_t>(kw), *okeys = exact<uint32_t>((size_t)n * 2 * kw);
      mf::key_to_words(keys.data(), key_bytes, a);
      mf::key_to_words(keys.data() + key_bytes, key_bytes, b);
      for (unsigned i = 0; i < 2 * n; i++) mf::key_to_words(keys.data() + (size_t)(2 + i) * key_bytes, key_bytes, okeys + (size_t)i * kw);
      uint32_t first = 0xFFFFFFFFu;
      const int st = mf::range_status(okeys, n, kw, a, b, &first);
      if (st != mf::range_status(okeys, n, kw, a, b)) return 4;  // (the same without `first`)
      printf("status %d %u\n", st, first);
      uint8_t *back = exact<uint8_t>((size_t)n * 2 * key_bytes);
      for (unsigned i = 0; i < 2 * n; i++) mf::words_to_key(okeys + (size_t)i * kw, key_bytes, back + (size_t)i * key_bytes);
      std::string hex;
      for (size_t j = 0; j < (size_t)n * 2 * key_bytes; j++) {
        char two[3];
        snprintf(two, sizeof two, "%02x", back[j]);
        hex += two;
      }
      printf("keys %s\n", hex.c_str());
      free(a);
      free(b);
      free(okeys);
      free(back);
    } else {
      return refuse();
    }
  }
  return 0;
}
