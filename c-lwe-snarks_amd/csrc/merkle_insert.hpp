// merkle_insert.hpp -- host only, plain C++: the plan of a batch of sequential key inserts into an indexed table (mfh_merkle_insert_keys, merkle.hip).
//
// Insert j = 0 .. nk - 1 puts key_j into the table: the record whose range (lo, hi) holds key_j gets hi <- key_j, and the record (key_j, the old hi, payload_j)
// goes into the inert slot s_j.  The device located every key against the table BEFORE the batch (record p_j), but a later key may fall into a range that an
// earlier key of the batch has split: the inserts with one p_j form a group, and within a group the record to change is that of the nearest earlier key.
//   pred[j]  -1: the table's record p_j; else the insert i < j with p_i == p_j and the largest key below key_j -- its record, in slot s_i, holds key_j by then
//   succ[j]  -1: the new record's hi is the table's record p_j's hi; else the insert i < j with p_i == p_j and the smallest key above key_j: hi = key_i
//   idx      the 2 nk record updates, in mfh_merkle_update_records' order: idx[2 j] = pred[j] < 0 ? p_j : s_pred[j] (hi <- key_j), idx[2 j + 1] = s_j
// How: one sort of the inserts by (p, key) gives every insert a rank in which a group is a contiguous run in key order; walking the batch in order with an
// ordered set of the ranks seen so far, the neighbours of rank[j] in the set, where they belong to the same group, are pred and succ.  O(nk log nk).
// The keys must be distinct (the caller refuses a key given twice).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

namespace mf {

struct InsertPlan {
  std::vector<int32_t> pred, succ;  // nk each
  std::vector<uint32_t> idx;        // 2 nk
};

// key j is the key_bytes bytes at keys + j * stride; p[j] its located record, s[j] its slot
inline void insert_plan(const uint8_t *keys, size_t stride, uint32_t key_bytes, uint32_t nk, const uint32_t *p, const uint32_t *s, InsertPlan &out) {
  out.pred.assign(nk, -1);
  out.succ.assign(nk, -1);
  out.idx.resize((size_t)2 * nk);
  std::vector<uint32_t> order(nk), rank(nk);
  for (uint32_t j = 0; j < nk; j++) order[j] = j;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (p[a] != p[b]) return p[a] < p[b];
    return memcmp(keys + a * stride, keys + b * stride, key_bytes) < 0;
  });
  for (uint32_t r = 0; r < nk; r++) rank[order[r]] = r;
  std::set<uint32_t> seen;
  for (uint32_t j = 0; j < nk; j++) {
    const auto above = seen.lower_bound(rank[j]);
    if (above != seen.end() && p[order[*above]] == p[j]) out.succ[j] = (int32_t)order[*above];
    if (above != seen.begin()) {
      const uint32_t below = order[*std::prev(above)];
      if (p[below] == p[j]) out.pred[j] = (int32_t)below;
    }
    seen.insert(above, rank[j]);
    out.idx[(size_t)2 * j] = out.pred[j] < 0 ? p[j] : s[out.pred[j]];
    out.idx[(size_t)2 * j + 1] = s[j];
  }
}

}  // namespace mf
