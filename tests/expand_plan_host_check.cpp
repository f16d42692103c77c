// The launch plan of k_expand_mm (csrc/expand_plan.hpp: expand_plan(n, logq, nrows[, periods]) -> {ppc, gx, gy}) as a program of its own
// (tests/test_expand_plan_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).  n = 1470, both logq.
// For EVERY nrows from 1 to 2^21 + 1 (that holds 1 .. 4096, every multiple of 64 and its neighbours, 16 384, 16 385, 32 768, 33 792, 33 793, 87 381, 131 072 and 2^20):
//   2 <= ppc <= 10;  23 ppc + 1 <= 256 (a chunk's blocks, one more for a row that starts mid-block, lie in two consecutive spans of 256 counters: what the kernel's
//   two sets of span constants rely on);  (gx - 1) ppc < nper <= gx ppc (the chunks cover the periods and the last one is not empty);  1024 (gy - 1) < nrows <= 1024 gy;
//   ppc does not decrease as nrows grows.
// Pinned values: ppc == 2 at 32 768 and at 87 381 - 65 536 rows at logq 736 (the default instance's regions; at logq 1472 regions of that size lie above the threshold
// below and take what the restated rule gives), ppc == 10 at 2^20 rows; the first nrows with ppc == 3 is 33 793 at logq
// 736 and 16 385 at 1472 -- both recomputed here from the rule "the most periods per chunk that still leave 4096 workgroups", written as nested loops that COUNT the
// workgroups.  A forced count (2 .. 10) is taken as it is, with the same covering condition.
// Argument "spoil": the restated rule asks for 8192 workgroups; the program must then fail (status 1).  Prints "ok <plans checked>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "expand_plan.hpp"

static const uint32_t N = 1470;

// workgroups of a launch whose chunks hold p periods, counted one by one: a block of 1024 rows x a chunk
static uint64_t count_workgroups(uint32_t nper, uint32_t nrows, uint32_t p) {
  uint64_t wgs = 0;
  for (uint32_t row0 = 0; row0 < nrows; row0 += 1024)
    for (uint32_t m0 = 0; m0 < nper; m0 += p) wgs++;
  return wgs;
}
// the rule: the most periods per chunk (at most 10) that still leave `want` workgroups, and never fewer than 2
static uint32_t restate(uint32_t nper, uint32_t nrows, uint64_t want) {
  for (uint32_t p = 10; p > 2; p--)
    if (count_workgroups(nper, nrows, p) >= want) return p;
  return 2;
}

int main(int argc, char **argv) {
  const bool spoil = argc > 1 && !strcmp(argv[1], "spoil");
  unsigned long plans = 0;
  for (int q = 0; q < 2; q++) {
    const uint32_t logq = q ? 1472 : 736;
    uint32_t nper = 0;  // periods of a row, counted: 4 coordinates (logq 736) or 2 (1472) each, the b coordinate included
    for (uint32_t c = 0; c < N + 1; c += q ? 2 : 4) nper++;
    uint32_t prev = 0, first3 = 0;
    for (uint32_t nrows = 1; nrows <= (1u << 21) + 1; nrows++) {
      const ExpandPlan pl = expand_plan(N, logq, nrows);
      plans++;
      if (pl.ppc < 2 || pl.ppc > 10 || 23 * pl.ppc + 1 > 256) { fprintf(stderr, "logq %u nrows %u: ppc %u\n", logq, nrows, pl.ppc); return 1; }
      if (!pl.gx || (uint64_t)(pl.gx - 1) * pl.ppc >= nper || (uint64_t)pl.gx * pl.ppc < nper) { fprintf(stderr, "logq %u nrows %u: gx %u ppc %u nper %u\n", logq, nrows, pl.gx, pl.ppc, nper); return 1; }
      if (!pl.gy || (uint64_t)1024 * pl.gy < nrows || (uint64_t)1024 * (pl.gy - 1) >= nrows) { fprintf(stderr, "logq %u nrows %u: gy %u\n", logq, nrows, pl.gy); return 1; }
      if (pl.ppc < prev) { fprintf(stderr, "logq %u nrows %u: ppc %u after %u\n", logq, nrows, pl.ppc, prev); return 1; }
      prev = pl.ppc;
      if (!first3 && pl.ppc >= 3) {
        if (pl.ppc != 3) { fprintf(stderr, "logq %u nrows %u: ppc jumps from 2 to %u\n", logq, nrows, pl.ppc); return 1; }
        first3 = nrows;
      }
      // the rule restated, where it is cheap to count: the small regions and the row counts named above
      const bool named = nrows <= 4096 || (nrows >= 16384 && nrows <= 16385) || nrows == 32768 || nrows == 33792 || nrows == 33793 ||
                         nrows == 87381 || nrows == 87381 - 65536 || nrows == 131072 || nrows == 1u << 20 || nrows == 1u << 21;
      if (named && pl.ppc != restate(nper, nrows, spoil ? 8192 : 4096)) {
        fprintf(stderr, "the plan differs from the rule: logq %u nrows %u: ppc %u, the loops give %u\n", logq, nrows, pl.ppc, restate(nper, nrows, spoil ? 8192 : 4096));
        return 1;
      }
    }
    // the first region that takes 3 periods per chunk, found by counting workgroups
    uint32_t want3 = 0;
    for (uint32_t nrows = 1; !want3; nrows += (nrows % 1024 == 0) ? 1 : 1024 - nrows % 1024)  // (the count changes only behind a multiple of 1024: visit 1, 1024, 1025, 2048, 2049, ...)
      if (restate(nper, nrows, 4096) >= 3) want3 = nrows;
    if (first3 != want3 || want3 != (q ? 16385u : 33793u)) { fprintf(stderr, "logq %u: first nrows with ppc 3 is %u, the loops give %u\n", logq, first3, want3); return 1; }
    if ((!q && (expand_plan(N, logq, 32768).ppc != 2 || expand_plan(N, logq, 87381 - 65536).ppc != 2)) || expand_plan(N, logq, 1u << 20).ppc != 10) {
      fprintf(stderr, "logq %u: pinned plans differ\n", logq);
      return 1;
    }
    // forced counts
    for (uint32_t periods = 2; periods <= 10; periods++)
      for (uint32_t nrows = 1; nrows <= 4096; nrows += 37) {
        const ExpandPlan pl = expand_plan(N, logq, nrows, periods), au = expand_plan(N, logq, nrows);
        plans++;
        if (pl.ppc != periods || pl.gy != au.gy || (uint64_t)(pl.gx - 1) * periods >= nper || (uint64_t)pl.gx * periods < nper) {
          fprintf(stderr, "forced: logq %u nrows %u periods %u: ppc %u gx %u gy %u\n", logq, nrows, periods, pl.ppc, pl.gx, pl.gy);
          return 1;
        }
      }
  }
  printf("ok %lu\n", plans);
  return 0;
}
