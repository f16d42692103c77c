// merkle_grow.hpp -- plain C++, compiled by hipcc for the kernels of merkle.hip AND by a host compiler (tests/merkle_grow_host_check.cpp): where every node of
// a GROWN tree comes from, and the roots of the all-inert subtrees it is filled with (mfh_merkle_grow, mfh_merkle_grow_leaves: include/mfhip.h has the calls).
//
// Growth.  A tree of depth d becomes the LEFTMOST subtree of a tree of depth D > d whose other leaves are all the inert leaf E_0 -- SHA-256 of an all-zero
// record of `length` bytes for a tree over records, 32 zero bytes for a tree of leaves (mfh_merkle_create's).  With E_l+1 = node(E_l, E_l) the root of every
// subtree of height l right of the old tree is the constant E_l, and the nodes above the old root R are the SPINE S_d = R, S_l+1 = node(S_l, E_l): D - d
// compressions, S_D the new root -- a public function of R (words.grown_root).
//
// Placement.  A tree's memory is 2^(depth + 1) nodes of 32 bytes in heap order (merkle.hip): level l (0 = the leaves) starts at byte 32 << (depth - l), node
// i of it is position p = 2^(depth - l) + i, position 0 is unused.  For a position p of the NEW tree grow_node says which of four things it is:
//   kGrowCopy    l <= d and i < 2^(d - l): the old tree's node of that level and index, old position `from` = 2^(d - l) + i (the old root among them: S_d)
//   kGrowInert   every other node off the spine: the constant E_l
//   kGrowSpine   l > d and i = 0: S_l, D - d positions
//   kGrowUnused  p = 0
// Every position has one kind, the copies are a bijection onto the old positions 1 .. 2^(d + 1) - 1, and nothing of the old tree outside them is named.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sha256_dev.hpp"

#if defined(__HIPCC__)
#define MF_GROW_HD __host__ __device__ __forceinline__
#else
#define MF_GROW_HD inline
#endif

namespace mf {

constexpr uint32_t kGrowMaxDepth = 24;  // (merkle.hip's kMaxDepth: this header stands alone)

enum GrowKind : uint32_t { kGrowUnused = 0, kGrowCopy = 1, kGrowInert = 2, kGrowSpine = 3 };

struct GrowNode {
  uint32_t kind, level, index, from;  // from: the old position of a copy, else 0
};

// the level of position p >= 1 of a tree of `depth`: depth - floor(log2 p)
MF_GROW_HD uint32_t grow_level(uint32_t depth, uint32_t p) { return depth - (31u - (uint32_t)__builtin_clz(p)); }

// what position p < 2^(new_depth + 1) of the tree grown from `depth` to `new_depth` is; 1 <= depth < new_depth <= kGrowMaxDepth
MF_GROW_HD GrowNode grow_node(uint32_t depth, uint32_t new_depth, uint32_t p) {
  GrowNode n{kGrowUnused, 0, 0, 0};
  if (!p) return n;
  n.level = grow_level(new_depth, p);
  n.index = p - (1u << (new_depth - n.level));
  if (n.level <= depth) {
    const uint32_t width = 1u << (depth - n.level);  // the old tree's nodes of this level
    n.kind = n.index < width ? kGrowCopy : kGrowInert;
    n.from = n.index < width ? width + n.index : 0;
  } else {
    n.kind = n.index ? kGrowInert : kGrowSpine;
  }
  return n;
}

// the 16-byte units of a tree's whole memory, the grid of k_grow_nodes: two a node
MF_GROW_HD uint32_t grow_units(uint32_t new_depth) { return 4u << new_depth; }

// E_0 .. E_kGrowMaxDepth as the tree stores them: node l = the 8 dwords at w + 8 l, each holding 4 digest BYTES in memory order (the big-endian word
// byte-swapped on a little-endian machine), so a kernel stores them as they are.  A kernel argument: 800 bytes.
struct alignas(16) GrowRoots {
  uint32_t w[(kGrowMaxDepth + 1) * 8];
};

MF_GROW_HD uint32_t grow_bswap(uint32_t v) { return v >> 24 | (v >> 8 & 0xFF00u) | (v << 8 & 0xFF0000u) | v << 24; }

// E_0 .. E_depth into r (the entries above stay zero).  records = true: E_0 = SHA-256 of `length` zero bytes; false: E_0 = 32 zero bytes, `length` unused.
// HOST work: depth + sha256_blocks(length) dependent compressions, microseconds at the lengths of records.
inline void grow_inert_roots(bool records, uint32_t length, uint32_t depth, GrowRoots &r) {
  for (uint32_t &x : r.w) x = 0;
  uint32_t cur[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (records) {
    const uint32_t iv[8] = MF_SHA256_IV;
    for (int j = 0; j < 8; j++) cur[j] = iv[j];
    for (uint32_t b = 0; b < sha256_blocks(length); b++) {
      uint32_t w[16];
      for (uint32_t t = 0; t < 16; t++) w[t] = sha256_pad_word(0, length, b, t);
      sha256_compress(cur, w);
    }
  }
  for (uint32_t l = 0;; l++) {
    for (int j = 0; j < 8; j++) r.w[8 * l + j] = grow_bswap(cur[j]);
    if (l == depth) break;
    uint32_t w[16], h[8] = MF_SHA256_IV;
    for (int j = 0; j < 8; j++) w[j] = w[8 + j] = cur[j];
    sha256_compress(h, w);
    for (int j = 0; j < 8; j++) cur[j] = h[j];
  }
}

}  // namespace mf
