// merkle_record_row.hpp -- host only, plain C++: the sizes and the row splice of mfh_merkle_update_records (merkle.hip).
//
// The packed input row of words.MerkleRecordUpdate(length, depth): 64 zero bytes where the two roots are computed | the old record's `length` bytes |
// the new record's `length` bytes | depth siblings of 32 bytes as words | ceil(depth / 8) index bytes.  Its sibling offset, 64 + 2 length, is in general
// no multiple of 16, and k_merkle_update_level writes its siblings at 16-byte units of a row of its own.  So the device keeps two staged pieces per update
// and the host splices them while it copies out of the pinned buffer:
//   the level row  what k_merkle_update_level writes for words.MerkleUpdate: 128 bytes of head (zeros and the two LEAVES, not used here), the siblings at
//                  byte 128, the index behind them; stride = its 128 + 32 depth + ceil(depth / 8) bytes rounded up to 16
//   the heads      what k_record_gather writes: the old record at byte 0 and the new record at byte head_pitch(length) of a slot of 2 head_pitch bytes,
//                  head_pitch = length rounded up to 16 (both 16-byte aligned: whole-unit stores)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace mf {

inline size_t update_row_bytes(uint32_t depth) { return 128 + (size_t)32 * depth + (depth + 7) / 8; }
inline size_t record_update_row_bytes(uint32_t length, uint32_t depth) { return 64 + 2 * (size_t)length + (size_t)32 * depth + (depth + 7) / 8; }
inline size_t record_head_pitch(uint32_t length) { return ((size_t)length + 15) & ~(size_t)15; }

// the most updates whose rows of row_bytes fit a stage of stage_bytes, at least one and at most nupd (nupd > 0)
inline uint32_t update_chunk(uint32_t nupd, size_t row_bytes, size_t stage_bytes) {
  const size_t fit = stage_bytes / row_bytes;
  return (uint32_t)(fit < 1 ? 1 : fit < nupd ? fit : nupd);
}

// row <- the record_update_row_bytes(length, depth) bytes of one update; reads level_row[128, update_row_bytes(depth)) and the `length` bytes at head and at
// head + record_head_pitch(length); writes nothing behind the row's bytes
inline void record_update_row(uint8_t *row, const uint8_t *head, const uint8_t *level_row, uint32_t length, uint32_t depth) {
  memset(row, 0, 64);
  if (length) {
    memcpy(row + 64, head, length);
    memcpy(row + 64 + (size_t)length, head + record_head_pitch(length), length);
  }
  memcpy(row + 64 + 2 * (size_t)length, level_row + 128, update_row_bytes(depth) - 128);
}

}  // namespace mf
