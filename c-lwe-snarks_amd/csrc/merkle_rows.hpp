// merkle_rows.hpp -- host only, plain C++: the one packed input row of the Merkle statements of words.py, its sizes, and the splice that puts a row
// together out of what the device staged (merkle.hip).
//
// The row:  Z zero bytes where the root(s) are computed | a head | depth siblings of 32 bytes as words | ceil(depth / 8) index bytes
//   words.MerklePath(depth)                       Z = 32, head = the leaf's 32 bytes                 row_bytes(32, 32, depth)
//   words.MerkleRecord(length, depth)             Z = 32, head = the record                          row_bytes(32, length, depth)
//   words.MerkleUpdate(depth)                     Z = 64, head = old leaf | new leaf                 row_bytes(64, 64, depth)
//   words.MerkleRecordUpdate(length, depth)       Z = 64, head = old record | new record             row_bytes(64, 2 length, depth)
//   words.MerkleAbsent(key_bytes, length, depth)  Z = 32, head = the query's key | the located record   row_bytes(32, key_bytes + length, depth)
// The kernels write whole rows where the tail lands on a 16-byte unit: k_merkle_paths the path row (tail at byte 64), k_merkle_update_level the level row
// (tail at byte 128), both staged at staged_stride of their bytes.  A head of records puts the tail anywhere, so for those statements the device stages two
// pieces per row and the host splices them while it copies out of the pinned buffer (splice_row):
//   the staged row  a path row or a level row; only its tail is read
//   the heads       what k_record_gather / k_absent_gather write: each record at the start of a slot of record_head_pitch(length) bytes (whole-unit stores)
// An absent query for which no record was found (status 2) gets the zero bytes and its key alone: its staged pieces come from a stand-in index and are not read.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <initializer_list>

namespace mf {

inline size_t row_tail_bytes(uint32_t depth) { return (size_t)32 * depth + (depth + 7) / 8; }
inline size_t row_bytes(size_t zeros, size_t head_bytes, uint32_t depth) { return zeros + head_bytes + row_tail_bytes(depth); }
inline size_t staged_stride(size_t row_bytes) { return (row_bytes + 15) & ~(size_t)15; }
inline size_t record_head_pitch(uint32_t length) { return ((size_t)length + 15) & ~(size_t)15; }

// the most updates whose rows of row_bytes fit a stage of stage_bytes, at least one and at most nupd (nupd > 0)
inline uint32_t update_chunk(uint32_t nupd, size_t row_bytes, size_t stage_bytes) {
  const size_t fit = stage_bytes / row_bytes;
  return (uint32_t)(fit < 1 ? 1 : fit < nupd ? fit : nupd);
}

struct RowPiece {
  const uint8_t *p;
  size_t bytes;
};

// row <- `zeros` zero bytes | the head's pieces, in order | the row_tail_bytes(depth) bytes at staged + tail_at (64 in a path row, 128 in a level row).
// staged = nullptr (not found) stops after the pieces.  Reads the pieces' bytes and that tail, and writes nothing behind the row's bytes.
inline void splice_row(uint8_t *row, size_t zeros, std::initializer_list<RowPiece> head, const uint8_t *staged, size_t tail_at, uint32_t depth) {
  memset(row, 0, zeros);
  row += zeros;
  for (const RowPiece &h : head) {
    if (h.bytes) memcpy(row, h.p, h.bytes);
    row += h.bytes;
  }
  if (staged) memcpy(row, staged + tail_at, row_tail_bytes(depth));
}

}  // namespace mf
