// merkle_absent_row.hpp -- host only, plain C++: the sizes and the row splice of mfh_merkle_absent_rows (merkle.hip).
//
// The packed input row of words.MerkleAbsent(key_bytes, length, depth): 32 zero bytes where the root is computed | the query's key_bytes bytes | the
// located record's `length` bytes | depth siblings of 32 bytes as words | ceil(depth / 8) index bytes.  Its sibling offset, 32 + key_bytes + length, is in
// general no multiple of 4, and k_merkle_paths writes words.  So the device keeps two staged pieces per query and the host splices them with the query
// (which it has) while it copies out of the pinned buffer:
//   the path row   what k_merkle_paths writes for words.MerklePath: 32 zero bytes, the LEAF (not used here), the siblings at byte 64, the index behind
//                  them; stride = its 64 + 32 depth + ceil(depth / 8) bytes rounded up to 16
//   the head       what k_absent_gather writes: the record at byte 0 of a slot of record_head_pitch(length) bytes (merkle_record_row.hpp)
// A query for which no record was found (status 2) gets the zero bytes and the query alone: its staged pieces come from a stand-in index and are not read.
#pragma once
#include "merkle_record_row.hpp"

namespace mf {

inline size_t absent_path_row_bytes(uint32_t depth) { return 64 + (size_t)32 * depth + (depth + 7) / 8; }
inline size_t absent_row_bytes(uint32_t key_bytes, uint32_t length, uint32_t depth) {
  return 32 + (size_t)key_bytes + length + (size_t)32 * depth + (depth + 7) / 8;
}

// row <- the absent_row_bytes(key_bytes, length, depth) bytes of one query (found), or its first 32 + key_bytes (not found); reads `length` bytes at head
// and path_row[64, absent_path_row_bytes(depth)) when found; writes nothing behind those bytes
inline void absent_row(uint8_t *row, const uint8_t *key, const uint8_t *head, const uint8_t *path_row, uint32_t key_bytes, uint32_t length, uint32_t depth,
                       bool found) {
  memset(row, 0, 32);
  memcpy(row + 32, key, key_bytes);
  if (!found) return;
  memcpy(row + 32 + key_bytes, head, length);
  memcpy(row + 32 + key_bytes + (size_t)length, path_row + 64, absent_path_row_bytes(depth) - 64);
}

}  // namespace mf
