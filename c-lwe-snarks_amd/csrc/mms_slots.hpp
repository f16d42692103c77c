// mms_slots.hpp -- plain C++ shared by host and kernels: the slot space of a streaming launch with several groups (evalmm.hip: k_mmstream, k_mmstream_p, k_mmstream_pb,
// k_mmstream_w) and the item queues of the persistent grid over it.
//
// A launch serves `ngt` groups of coefficient vectors, `ngr` of them per region (ngt / ngr regions), over `tgs` tile groups of 16 row tiles and `nchunks` row chunks.
// Tile group tg belongs to XCD tg & 7, and every XCD numbers its (group, tile group) pairs by a SLOT:
//   map 0: slot -> (slot % ngt, slot / ngt): the 32 workgroups an XCD runs at a time are 32 / ngt tile groups x all groups of BOTH regions -- an image's
//          fragments are shared by ngr workgroups, a group's digit fragments by 32 / ngt of them;
//   map 1: 32 consecutive slots are 32 / ngr tile groups x the ngr groups of ONE region (regions alternate per 32 slots): the fragments are shared by ngr
//          workgroups as before, a group's digit fragments by 32 / ngr -- the digit fragments are as many bytes per workgroup as the image's, so with two
//          regions this halves their share of the L2 misses.  Needs ngr | 32; the host picks map 0 otherwise.
// An XCD's slots are padded to whole blocks of 32 (`nblk` of them); a slot whose tile group does not exist (tg >= tgs) is empty.  The items of an XCD in the order the
// persistent grid takes them -- chunk outermost, then the slots -- have the FLAT index chunk * 32 nblk + slot: the queue of an XCD is one counter over that index.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MMS_HD __host__ __device__ __forceinline__
#else
#define MMS_HD inline
#endif

// Which (group, tile group) slot `slot` of XCD `xcd` is.
MMS_HD void mms_item(uint32_t xcd, uint32_t slot, uint32_t ngt, uint32_t ngr, uint32_t map, uint32_t &grp, uint32_t &tg) {
  if (map == 0) {
    grp = slot % ngt;
    tg = (slot / ngt) * 8 + xcd;
  } else {
    const uint32_t blk = slot >> 5, i = slot & 31, nreg = ngt / ngr, tpb = 32 / ngr;
    grp = (blk % nreg) * ngr + i % ngr;
    tg = ((blk / nreg) * tpb + i / ngr) * 8 + xcd;
  }
}
// slots per XCD (before the padding to blocks of 32) and the 32-slot blocks that hold them
MMS_HD uint32_t mms_slots(uint32_t tgs, uint32_t ngt, uint32_t ngr, uint32_t map) {
  const uint32_t tgx = (tgs + 7) / 8;  // tile groups per XCD
  return map ? (tgx + 32 / ngr - 1) / (32 / ngr) * (ngt / ngr) * 32 : tgx * ngt;
}
MMS_HD uint32_t mms_nblk(uint32_t tgs, uint32_t ngt, uint32_t ngr, uint32_t map) { return (mms_slots(tgs, ngt, ngr, map) + 31) / 32; }
// true when slot `slot` of XCD `xcd` is an item (its tile group exists)
MMS_HD bool mms_slot_valid(uint32_t xcd, uint32_t slot, uint32_t ngt, uint32_t ngr, uint32_t map, uint32_t tgs) {
  uint32_t grp, tg;
  mms_item(xcd, slot, ngt, ngr, map, grp, tg);
  return tg < tgs;
}
// flat index of an XCD's queue -> (chunk, slot)
MMS_HD void mms_flat(uint32_t flat, uint32_t nblk, uint32_t &chunk, uint32_t &slot) {
  chunk = flat / (nblk * 32);
  slot = flat % (nblk * 32);
}
