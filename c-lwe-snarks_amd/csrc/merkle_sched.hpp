// merkle_sched.hpp -- host only, plain C++: the schedule of a batch of sequential one-leaf updates of a Merkle tree (mfh_merkle_update_rows, merkle.hip).
//
// Update k = 0 .. n - 1 sets leaf idx[k] and recomputes its ancestors; node idx[k] >> l of level l (0 = the leaves, depth = the root) is the node it
// touches there.  The level-synchronous kernel needs to know, per update and level, WHOSE value it reads and whether its own value is the node's last:
//   same0[k]        the last j < k with idx[j] == idx[k], or -1: the old leaf of update k is update j's new leaf, else the stored leaf
//   sib[l * n + k]  the last j < k with idx[j] >> l == (idx[k] >> l) ^ 1, or -1, for l < depth: the sibling of update k at level l is update j's value of
//                   that node, else the stored node
//   last[k]         bit l, l <= depth, set when no j > k has idx[j] >> l == idx[k] >> l: update k's value of the node is what the tree keeps
// and, for a path cut at levels cuts[0] < cuts[1] < .. (the rows of words.MerkleSegment, k_merkle_cut_rows):
//   same_cut[g * n + k]  the last j < k with idx[j] >> cuts[g] == idx[k] >> cuts[g], or -1: the old value of update k's node of level cuts[g] is update j's
//                        value of it, else the stored node -- what `seen` holds at that level before update k overwrites it
//
// How: the distinct nodes of a level, sorted, are the distinct nodes of the level below shifted by one and deduplicated, and a node's sibling, if the
// batch touches it, is its neighbour in that sorted list.  So one sort of the indices gives every level a dense numbering of its touched nodes, and one
// pass over the updates per level, with a table "last update at this node so far" over that numbering, gives the three answers:
// O(n log n + n depth) time, O(n) memory beside the outputs, no hashing.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mf {

// idx[k] < 2^depth, 1 <= depth <= 31; same0: n entries, sib: depth * n, last: n.  n = 0 writes nothing.
// ncuts > 0: cuts[0] < cuts[1] < .. < cuts[ncuts - 1] <= depth, same_cut: ncuts * n entries.
inline void merkle_schedule(uint32_t depth, uint32_t n, const uint32_t *idx, int32_t *same0, int32_t *sib, uint32_t *last, uint32_t ncuts = 0,
                            const uint32_t *cuts = nullptr, int32_t *same_cut = nullptr) {
  if (!n) return;
  uint32_t g = 0;  // the next cut at or above the current level
  std::vector<uint32_t> node(idx, idx + n);  // the distinct touched nodes of the current level, sorted
  std::sort(node.begin(), node.end());
  node.erase(std::unique(node.begin(), node.end()), node.end());
  std::vector<uint32_t> id(n);               // update k touches node[id[k]]
  for (uint32_t k = 0; k < n; k++) id[k] = (uint32_t)(std::lower_bound(node.begin(), node.end(), idx[k]) - node.begin());
  std::vector<int32_t> seen, other;          // per node: the last update at it so far; its sibling's number, or -1
  std::vector<uint32_t> up;                  // per node: its parent's number in the next level's list
  for (uint32_t k = 0; k < n; k++) last[k] = 0;
  for (uint32_t l = 0; l <= depth; l++) {
    const uint32_t m = (uint32_t)node.size();
    seen.assign(m, -1);
    other.assign(m, -1);
    for (uint32_t i = 0; i + 1 < m; i++)
      if (!(node[i] & 1) && node[i + 1] == node[i] + 1) { other[i] = (int32_t)(i + 1); other[i + 1] = (int32_t)i; }
    int32_t *cut = g < ncuts && cuts[g] == l ? same_cut + (size_t)g++ * n : nullptr;
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t i = id[k];
      if (l == 0) same0[k] = seen[i];
      if (l < depth) sib[(size_t)l * n + k] = other[i] >= 0 ? seen[other[i]] : -1;
      if (cut) cut[k] = seen[i];
      seen[i] = (int32_t)k;
    }
    for (uint32_t k = 0; k < n; k++)
      if (seen[id[k]] == (int32_t)k) last[k] |= 1u << l;
    if (l == depth) break;
    // the next level: parents of the sorted nodes are sorted too; equal neighbours collapse
    up.resize(m);
    uint32_t out = 0;
    for (uint32_t i = 0; i < m; i++) {
      const uint32_t p = node[i] >> 1;
      if (out && node[out - 1] == p) { up[i] = out - 1; continue; }
      node[out] = p;  // (out <= i: position i has been read)
      up[i] = out++;
    }
    node.resize(out);
    for (uint32_t k = 0; k < n; k++) id[k] = up[id[k]];
  }
}

}  // namespace mf
