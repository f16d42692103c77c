// same_cut of csrc/merkle_sched.hpp (mf::merkle_schedule with cuts) against a brute-force O(n^2) search, as a program of its own
// (tests/test_merkle_cuts_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <pattern> <depth> <n> <seed> <spoil> <cut> [<cut> ..]
// pattern "same", "alt" or "random" as tests/merkle_sched_host_check.cpp draws them; the cuts ascending, 1 <= cut < depth.  Every array lives in a heap
// allocation of exactly its size (one never-touched byte when a size is zero), so a write or read one entry outside is a heap overflow the address
// sanitizer reports.  The three outputs without cuts are computed a second time by a call WITHOUT the trailing arguments and must be identical: the cuts
// change nothing else.  With spoil = 1 one index is changed AFTER the schedule was made: the comparison must then fail (status 1).
// Prints "ok <pattern> <depth> <n> <ncuts>" per line.
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
  char buf[512], pattern[16];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned depth = 0, n = 0, spoil = 0;
    unsigned long long seed = 0;
    int used = 0;
    const int got = sscanf(buf, "%15s %u %u %llu %u%n", pattern, &depth, &n, &seed, &spoil, &used);
    const int kind = !strcmp(pattern, "same") ? 0 : !strcmp(pattern, "alt") ? 1 : !strcmp(pattern, "random") ? 2 : -1;
    std::vector<uint32_t> cut_list;
    bool bad = got < 5 || kind < 0 || depth < 2 || depth > 31 || spoil > 1;
    if (!bad) {
      const char *at = buf + used;
      unsigned c = 0;
      int step = 0;
      while (sscanf(at, "%u%n", &c, &step) == 1) {
        bad = bad || c < 1 || c >= depth || (!cut_list.empty() && c <= cut_list.back());
        cut_list.push_back(c);
        at += step;
      }
      bad = bad || cut_list.empty();
    }
    if (bad) {
      fprintf(stderr, "merkle_cuts_host_check: expected <same|alt|random> <depth in 2 .. 31> <n> <seed> <spoil 0|1> <ascending cuts in [1, depth)>\n");
      return 2;
    }
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const uint32_t mask = (uint32_t)((1ull << depth) - 1), ncuts = (uint32_t)cut_list.size();
    uint32_t *idx = exact<uint32_t>(n), *cuts = exact<uint32_t>(ncuts);
    memcpy(cuts, cut_list.data(), ncuts * sizeof(uint32_t));
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
      for (uint32_t i = 0; i < npool; i++) pool[i] = (i & 1) ? (pool[i - 1] ^ (1u << (rnd() % depth))) & mask : rnd() & mask;  // neighbours at EVERY level
      for (uint32_t k = 0; k < n; k++) idx[k] = pool[rnd() % npool];
    }
    int32_t *same0 = exact<int32_t>(n), *sib = exact<int32_t>((size_t)depth * n), *same_cut = exact<int32_t>((size_t)ncuts * n);
    uint32_t *last = exact<uint32_t>(n);
    int32_t *same0_b = exact<int32_t>(n), *sib_b = exact<int32_t>((size_t)depth * n);
    uint32_t *last_b = exact<uint32_t>(n);
    mf::merkle_schedule(depth, n, idx, same0, sib, last, ncuts, cuts, same_cut);
    mf::merkle_schedule(depth, n, idx, same0_b, sib_b, last_b);
    bool ok = !n || (!memcmp(same0, same0_b, n * sizeof(int32_t)) && !memcmp(sib, sib_b, (size_t)depth * n * sizeof(int32_t)) && !memcmp(last, last_b, n * sizeof(uint32_t)));
    if (!ok) fprintf(stderr, "merkle_cuts_host_check: %s depth %u n %u: the cuts changed the schedule without cuts\n", pattern, depth, n);
    if (spoil && n) idx[rnd() % n] ^= 1u << cuts[0];

    for (uint32_t g = 0; g < ncuts && ok; g++)
      for (uint32_t k = 0; k < n && ok; k++) {
        int32_t s = -1;
        for (uint32_t j = 0; j < k; j++)
          if (idx[j] >> cuts[g] == idx[k] >> cuts[g]) s = (int32_t)j;
        if (same_cut[(size_t)g * n + k] != s) {
          ok = false;
          fprintf(stderr, "merkle_cuts_host_check: %s depth %u n %u: the schedule differs at cut %u, update %u\n", pattern, depth, n, cuts[g], k);
        }
      }
    free(idx); free(cuts); free(same0); free(sib); free(same_cut); free(last); free(same0_b); free(sib_b); free(last_b);
    if (!ok) return 1;
    printf("ok %s %u %u %u\n", pattern, depth, n, ncuts);
  }
  return 0;
}
