// merkle_remove.hpp -- host only, plain C++: the plan of a batch of sequential key removes from an indexed table (mfh_merkle_remove_keys, merkle.hip).
//
// Remove j = 0 .. nk - 1 takes key_j out of the table: the live record whose own key (lo) is key_j, slot s_j, becomes the all-zero record, and the live record
// whose hi is key_j, slot P_j, gets hi <- the hi of record s_j.  The device located every key against the table BEFORE the batch -- own[j], the lowest live
// record with lo = key_j, and prev[j], the lowest live record with hi = key_j -- but adjacent members may both be in the batch, so the record to change and
// the hi it receives depend on what was removed earlier.  With the batch sorted by key, ranks r and r + 1 are LINKED when prev[order[r + 1]] == own[order[r]]:
// the two keys are neighbours in the set.  For remove j:
//   P_j      walk left from rank[j] over linked ranks whose remove index is below j (gone by then: each handed its range to its left neighbour).  Where the
//            walk stops at a linked rank that has not been removed yet, P_j is that key's own record, else prev of the leftmost rank reached -- one value:
//            a link says the two are the same record.
//   the hi   walk right the same way.  Where the walk stops at a linked, not-yet-removed rank the new hi is that KEY (hi_key[j] = its remove index);
//            else it is the before-batch hi of own of the rightmost rank reached (hi_key[j] = -1, hi_rec[j] = that record).
//   idx      the 2 nk record updates, in mfh_merkle_update_records' order: idx[2 j] = P_j, idx[2 j + 1] = own[j]
// Every new record's sources are the table as it stood before the batch and the batch's keys: a surviving record's lo and payload never change during the
// batch.  So one launch builds all the records, with no ordering among them (k_remove_records).
// How: one sort by key; a union-find over the ranks whose sets are the maximal runs of removed ranks joined by links, each with its leftmost and rightmost
// rank.  Walking the batch in order, both walks of remove j are one find on each neighbour; then rank[j] joins its removed neighbours.  O(nk log nk) for the
// sort, near-linear behind it.  The keys must be distinct (the caller refuses a key given twice) and every own and prev found.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace mf {

struct RemovePlan {
  std::vector<int32_t> hi_key;   // nk
  std::vector<uint32_t> hi_rec;  // nk
  std::vector<uint32_t> idx;     // 2 nk
};

// key j is the key_bytes bytes at keys + j * stride; own[j] and prev[j] its located records
inline void remove_plan(const uint8_t *keys, size_t stride, uint32_t key_bytes, uint32_t nk, const uint32_t *own, const uint32_t *prev, RemovePlan &out) {
  out.hi_key.assign(nk, -1);
  out.hi_rec.assign(nk, 0);
  out.idx.resize((size_t)2 * nk);
  std::vector<uint32_t> order(nk), rank(nk), parent(nk), left(nk), right(nk);
  std::vector<uint8_t> gone(nk, 0);
  for (uint32_t j = 0; j < nk; j++) order[j] = parent[j] = left[j] = right[j] = j;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return memcmp(keys + a * stride, keys + b * stride, key_bytes) < 0; });
  for (uint32_t r = 0; r < nk; r++) rank[order[r]] = r;
  auto linked = [&](uint32_t r) { return prev[order[r + 1]] == own[order[r]]; };  // ranks r and r + 1
  auto find = [&](uint32_t r) {
    uint32_t root = r;
    while (parent[root] != root) root = parent[root];
    while (parent[r] != root) {
      const uint32_t up = parent[r];
      parent[r] = root;
      r = up;
    }
    return root;
  };
  auto join = [&](uint32_t a, uint32_t b) {  // two runs that touch become one
    a = find(a), b = find(b);
    parent[b] = a;
    left[a] = std::min(left[a], left[b]);
    right[a] = std::max(right[a], right[b]);
  };
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t r = rank[j];
    const bool run_l = r > 0 && linked(r - 1) && gone[r - 1], run_r = r + 1 < nk && linked(r) && gone[r + 1];
    const uint32_t l = run_l ? left[find(r - 1)] : r, h = run_r ? right[find(r + 1)] : r;  // the leftmost and the rightmost rank reached
    out.idx[(size_t)2 * j] = prev[order[l]];  // (where rank l - 1 is linked and still there, this is its own record)
    out.idx[(size_t)2 * j + 1] = own[j];
    if (h + 1 < nk && linked(h)) {  // (not gone: the run would have reached it)
      out.hi_key[j] = (int32_t)order[h + 1];
    } else {
      out.hi_rec[j] = own[order[h]];
    }
    gone[r] = 1;
    if (run_l) join(r - 1, r);
    if (run_r) join(r, r + 1);
  }
}

}  // namespace mf
