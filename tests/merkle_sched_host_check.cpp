// The update schedule of csrc/merkle_sched.hpp (mf::merkle_schedule) against a brute-force O(n^2 depth) search, as a program of its own
// (tests/test_merkle_sched_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <pattern> <depth> <n> <seed> [<spoil>]
// pattern "same" (every update at one leaf), "alt" (two sibling leaves strictly alternating) or "random" (draws from a small pool of leaves, half of them
// neighbours of the others at levels 0 .. 2: heavy repeats, siblings and cousins).  The indices and the three outputs live in heap allocations of exactly
// their sizes (one never-touched byte when a size is zero), so a write or read one entry outside them is a heap overflow the address sanitizer reports.
// With spoil = 1 the search is run on indices of which one was changed AFTER the schedule was made: the comparison must then fail (status 1).
// Prints "ok <pattern> <depth> <n>" per line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "merkle_sched.hpp"

static uint64_t rng_state;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

template <class T> static T *exact(size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (!p) exit(3);
  return p;
}

int main() {
  char buf[256], pattern[16];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned depth = 0, n = 0, spoil = 0;
    unsigned long long seed = 0;
    const int got = sscanf(buf, "%15s %u %u %llu %u", pattern, &depth, &n, &seed, &spoil);
    const int kind = !strcmp(pattern, "same") ? 0 : !strcmp(pattern, "alt") ? 1 : !strcmp(pattern, "random") ? 2 : -1;
    if (got < 4 || kind < 0 || depth < 1 || depth > 31 || spoil > 1) {
      fprintf(stderr, "merkle_sched_host_check: expected <same|alt|random> <depth in 1 .. 31> <n> <seed> [<spoil 0|1>]\n");
      return 2;
    }
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const uint32_t mask = (uint32_t)((1ull << depth) - 1);
    uint32_t *idx = exact<uint32_t>(n);
    if (kind == 0) {
      const uint32_t x = rnd() & mask;
      for (uint32_t k = 0; k < n; k++) idx[k] = x;
    } else if (kind == 1) {
      const uint32_t x = rnd() & mask;
      for (uint32_t k = 0; k < n; k++) idx[k] = x ^ (k & 1);
    } else {
      const uint32_t want = n / 16 > 2 ? n / 16 : 2;
      const uint32_t npool = (uint64_t)want > (uint64_t)mask + 1 ? mask + 1 : want;
      std::vector<uint32_t> pool(npool);
      for (uint32_t i = 0; i < npool; i++) pool[i] = (i & 1) ? (pool[i - 1] ^ (1u << (rnd() % (depth < 3 ? depth : 3)))) & mask : rnd() & mask;
      for (uint32_t k = 0; k < n; k++) idx[k] = pool[rnd() % npool];
    }
    int32_t *same0 = exact<int32_t>(n), *sib = exact<int32_t>((size_t)depth * n);
    uint32_t *last = exact<uint32_t>(n);
    mf::merkle_schedule(depth, n, idx, same0, sib, last);
    if (spoil && n) idx[rnd() % n] ^= 1;

    bool ok = true;
    for (uint32_t k = 0; k < n && ok; k++) {
      uint32_t want_last = 0;
      for (uint32_t l = 0; l <= depth; l++) {
        int32_t s = -1, o = -1;
        for (uint32_t j = 0; j < k; j++) {
          if (idx[j] >> l == idx[k] >> l) s = (int32_t)j;
          if (idx[j] >> l == ((idx[k] >> l) ^ 1)) o = (int32_t)j;
        }
        bool later = false;
        for (uint32_t j = k + 1; j < n; j++) later |= idx[j] >> l == idx[k] >> l;
        if (!later) want_last |= 1u << l;
        if (l == 0 && same0[k] != s) ok = false;
        if (l < depth && sib[(size_t)l * n + k] != o) ok = false;
      }
      if (last[k] != want_last) ok = false;
      if (!ok) fprintf(stderr, "merkle_sched_host_check: %s depth %u n %u: the schedule differs at update %u\n", pattern, depth, n, k);
    }
    free(idx);
    free(same0);
    free(sib);
    free(last);
    if (!ok) return 1;
    printf("ok %s %u %u\n", pattern, depth, n);
  }
  return 0;
}
