// The slot arithmetic of csrc/mms_slots.hpp -- what the host and the persistent streaming kernels share: mms_item, mms_slots / mms_nblk, mms_slot_valid, mms_flat -- against a
// restatement by plain nested loops, as a program of its own (tests/test_mms_queue_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).
// Sweep: 1 .. 130 tile groups, ngr in {2, 4, 8, 16} groups per region with one and two regions, map 0 and 1, 1 .. 3 row chunks.  Per case:
//   (a) the valid flat indices of the eight queues (mms_flat -> (chunk, slot), mms_slot_valid, mms_item with the QUEUE's XCD) enumerate every (group, tile group, chunk)
//       exactly once, and an invalid index names a tile group that does not exist;
//   (b) slot by slot, mms_item equals the static map written out as loops (map 0: tile groups outermost, all groups inside; map 1: blocks of 32 slots = 32 / ngr tile groups
//       x the ngr groups of ONE region, regions alternating per block), so the order inside a 32-slot block is the static walk's: workgroup cu of an XCD takes slot
//       32 r + cu in round r, and flat index chunk * 32 nblk + 32 r + cu is that item;
//   (c) the count tables live in heap allocations of exactly their sizes: an index outside them is a heap overflow the address sanitizer reports.
// Argument "spoil": the restatement of (b) is shifted by one tile group for one case; the program must then fail (status 1).  Prints "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mms_slots.hpp"

struct Item { uint32_t grp, tg; };

// the static map of XCD `xcd` as loops: slot -> item, padded to whole blocks of 32 with tile groups that may not exist
static uint32_t restate(uint32_t xcd, uint32_t tgs, uint32_t ngt, uint32_t ngr, uint32_t map, Item *out /* nblk * 32 */, uint32_t cap) {
  const uint32_t tgx = (tgs + 7) / 8;
  uint32_t slot = 0;
  if (map == 0) {
    for (uint32_t t = 0; slot < cap; t++)
      for (uint32_t g = 0; g < ngt && slot < cap; g++) out[slot++] = Item{g, t * 8 + xcd};
    return tgx * ngt;
  }
  const uint32_t nreg = ngt / ngr, tpb = 32 / ngr;
  uint32_t used = 0;
  for (uint32_t tb = 0; slot < cap; tb++)  // a block of tpb tile groups ...
    for (uint32_t reg = 0; reg < nreg && slot < cap; reg++) {  // ... for one region after the other: 32 slots each
      for (uint32_t t = 0; t < tpb; t++)
        for (uint32_t g = 0; g < ngr; g++) out[slot++] = Item{reg * ngr + g, (tb * tpb + t) * 8 + xcd};
      if (tb * tpb < tgx) used = slot;
    }
  return used;
}

int main(int argc, char **argv) {
  const bool spoil = argc > 1 && !strcmp(argv[1], "spoil");
  unsigned long cases = 0;
  for (uint32_t tgs = 1; tgs <= 130; tgs++)
    for (uint32_t ngr = 2; ngr <= 16; ngr *= 2)
      for (uint32_t nreg = 1; nreg <= 2; nreg++)
        for (uint32_t map = 0; map <= 1; map++)
          for (uint32_t nchunks = 1; nchunks <= 3; nchunks++) {
            const uint32_t ngt = ngr * nreg, nblk = mms_nblk(tgs, ngt, ngr, map), per_chunk = nblk * 32;
            if (mms_slots(tgs, ngt, ngr, map) > per_chunk || !nblk) { fprintf(stderr, "mms_nblk does not hold the slots\n"); return 1; }
            uint32_t *count = (uint32_t *)calloc((size_t)nchunks * ngt * tgs, sizeof(uint32_t));
            Item *want = (Item *)malloc((size_t)per_chunk * sizeof(Item));
            if (!count || !want) return 3;
            for (uint32_t xcd = 0; xcd < 8; xcd++) {
              const uint32_t used = restate(xcd, tgs, ngt, ngr, map, want, per_chunk);
              if (used != mms_slots(tgs, ngt, ngr, map)) { fprintf(stderr, "mms_slots differs from the loops: tgs %u ngt %u ngr %u map %u\n", tgs, ngt, ngr, map); return 1; }
              if (spoil && tgs == 77 && xcd == 3) want[per_chunk / 2].tg += 8;
              for (uint32_t flat = 0; flat < nchunks * per_chunk; flat++) {
                uint32_t chunk, slot, grp, tg;
                mms_flat(flat, nblk, chunk, slot);
                if (chunk >= nchunks || slot >= per_chunk || chunk * per_chunk + slot != flat) { fprintf(stderr, "mms_flat: flat %u -> (%u, %u)\n", flat, chunk, slot); return 1; }
                mms_item(xcd, slot, ngt, ngr, map, grp, tg);
                if (grp != want[slot].grp || tg != want[slot].tg) {
                  fprintf(stderr, "the map differs: tgs %u ngt %u ngr %u map %u xcd %u slot %u: (%u, %u), the loops give (%u, %u)\n", tgs, ngt, ngr, map, xcd, slot, grp, tg,
                          want[slot].grp, want[slot].tg);
                  return 1;
                }
                const bool valid = mms_slot_valid(xcd, slot, ngt, ngr, map, tgs);
                if (valid != (tg < tgs) || grp >= ngt || (tg & 7) != xcd) { fprintf(stderr, "validity: tgs %u xcd %u slot %u\n", tgs, xcd, slot); return 1; }
                if (valid) count[((size_t)chunk * ngt + grp) * tgs + tg]++;
              }
            }
            for (size_t i = 0; i < (size_t)nchunks * ngt * tgs; i++)
              if (count[i] != 1) {
                fprintf(stderr, "not exactly once: tgs %u ngt %u ngr %u map %u chunks %u: entry %zu taken %u times\n", tgs, ngt, ngr, map, nchunks, i, count[i]);
                return 1;
              }
            free(count);
            free(want);
            cases++;
          }
  printf("ok %lu\n", cases);
  return 0;
}
