// expand_plan.hpp -- plain C++ shared by the host side of expandmm.hip and a host check (tests/expand_plan_host_check.cpp): the launch plan of k_expand_mm.
//
// A row of n + 1 coordinates is `nper` periods of 23 AES blocks (4 coordinates per period at logq 736, 2 at 1472).  A workgroup is 16 waves = 16 k-steps of 64 rows and
// walks a CHUNK of `ppc` consecutive periods of its rows: grid = (gx chunks, gy blocks of 1024 rows).  The kernel's counter-mode shortcut holds the span constants of two
// consecutive spans of 256 counter blocks, so a chunk's 23 ppc (+ 1, for a row that starts mid-block) consecutive blocks per lane must fit 256: ppc <= 10.  Within that,
// ppc is the largest value that still leaves 4096 workgroups (about eight rounds of the 512 workgroup slots), and never below 2.  `periods` (mfh_set_expand_periods: 2 .. 10)
// forces ppc; 0 = automatic.
#pragma once
#include <stdint.h>

constexpr uint32_t EXPAND_MAX_PERIODS = 10, EXPAND_MIN_PERIODS = 2;

struct ExpandPlan { uint32_t ppc, gx, gy; };

constexpr ExpandPlan expand_plan(uint32_t n, uint32_t logq, uint32_t nrows, uint32_t periods = 0) {
  const uint32_t cpm = logq == 736 ? 4 : 2;  // coordinates per period
  const uint32_t ksteps = (nrows + 63) / 64, nper = (n + 1 + cpm - 1) / cpm;
  const uint32_t gy = (ksteps + 15) / 16;
  uint32_t ppc = EXPAND_MAX_PERIODS;
  if (periods)
    ppc = periods;
  else
    while (ppc > EXPAND_MIN_PERIODS && (uint64_t)gy * ((nper + ppc - 1) / ppc) < 4096) ppc--;
  return ExpandPlan{ppc, (nper + ppc - 1) / ppc, gy};
}
