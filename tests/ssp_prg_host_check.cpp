// ssp_prg_host_check.cpp -- the generator of csrc/ssp_prg.hpp as a program: reads lines "seed slot k" (C integer syntax: decimal or 0x...), prints
// "rowkey raw coeff" (decimal) per line.  tests/test_witness_ref_cpu.py compiles it with g++ -fsanitize=address,undefined and compares its output with
// the numpy restatement (tests/witness_ref.py) and with the recorded numbers of tests/golden/ssp_prg.json.  Exit 2 on a malformed line.
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "ssp_prg.hpp"

static bool number(const char *&s, uint64_t max, uint64_t &out) {
  while (*s == ' ') s++;
  if (*s < '0' || *s > '9') return false;
  char *end = nullptr;
  errno = 0;
  const unsigned long long v = strtoull(s, &end, 0);
  if (errno || end == s || v > max) return false;
  s = end;
  out = v;
  return true;
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    const char *s = line;
    uint64_t seed, slot, k;
    if (!number(s, UINT64_MAX, seed) || !number(s, UINT32_MAX, slot) || !number(s, UINT32_MAX, k)) return 2;
    while (*s == ' ') s++;
    if (*s != '\n' && *s != '\0') return 2;
    const uint32_t rk = mf::ssp_prg_rowkey(seed, (uint32_t)slot);
    printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", rk, mf::ssp_prg_raw(rk, (uint32_t)k), mf::ssp_prg_coeff(rk, (uint32_t)k));
  }
  return 0;
}
