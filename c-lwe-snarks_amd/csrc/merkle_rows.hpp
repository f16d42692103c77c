// merkle_rows.hpp -- host only, plain C++: the one packed input row of the Merkle statements of words.py, its sizes, and the splice that puts a row
// together out of what the device staged (merkle.hip).
//
// The row:  Z zero bytes where the root(s) are computed | a head | depth siblings of 32 bytes as words | ceil(depth / 8) index bytes
//   words.MerklePath(depth)                       Z = 32, head = the leaf's 32 bytes                 row_bytes(32, 32, depth)
//   words.MerkleRecord(length, depth)             Z = 32, head = the record                          row_bytes(32, length, depth)
//   words.MerkleUpdate(depth)                     Z = 64, head = old leaf | new leaf                 row_bytes(64, 64, depth)
//   words.MerkleRecordUpdate(length, depth)       Z = 64, head = old record | new record             row_bytes(64, 2 length, depth)
//   words.MerkleAbsent(key_bytes, length, depth)  Z = 32, head = the query's key | the located record   row_bytes(32, key_bytes + length, depth)
//   words.MerkleInsert(key_bytes, length, depth)  Z = 64, head = the key | old record of p | old record of s | new record of s, and TWO tails' siblings:
//                                                 depth siblings of p | depth siblings of s | ceil(2 depth / 8) index bytes, bit l < depth = bit l of p,
//                                                 bit depth + l = bit l of s                      pair_row_bytes(key_bytes, 3, length, depth)
//   words.MerkleInsert(.., joined=False)          the same behind Z = 128 (four tops)                pair_row_bytes(key_bytes, 3, length, depth, 128)
//   words.MerkleRemove(key_bytes, length, depth)  the insert's row without a new record of s: Z = 64 (128 with joined=False), head = the key | old record of
//                                                 p | old record of s, the two tails as the insert's  pair_row_bytes(key_bytes, 2, length, depth)
//   words.MerkleTransfer(key_bytes, length, depth, amount_bytes)   the remove's row with three public pieces where it has the key: Z = 64 (128 with joined=False),
//                                                 head = k_from | k_to | the amount as amount_bytes big-endian bytes | old record of p | old record of s, the two
//                                                 tails as the insert's                           pair_row_bytes(2 key_bytes + amount_bytes, 2, length, depth)
//   words.MerkleAdjust(key_bytes, length, depth, amount_bytes)   ONE record and one tail behind three public pieces: Z = 64, head = the key | the amount as
//                                                 amount_bytes big-endian bytes | the side byte | the old record    row_bytes(64, key_bytes + amount_bytes + 1 + length, depth)
//   words.MerkleWrite(key_bytes, length, depth, field, expect)   ONE record and one tail behind the key and the F = hi - lo bytes of the value, with expect=True the
//                                                 F expected bytes in front of it: Z = 64, head = the key | [e |] v | the old record
//                                                                                                 row_bytes(64, key_bytes + F [+ F] + length, depth)
//   words.MerkleSegment(levels)                   the GIVEN nodes stand in front of the computed tops: old node as words | new node as words | 64 zero
//                                                 bytes | levels siblings as words | ceil(levels / 8) index bytes      segment_row_bytes(levels)
//   words.MerkleClimb(levels)                     the GIVEN node stands in front of the computed top: the node as words | 32 zero bytes | levels siblings as
//                                                 words | ceil(levels / 8) index bytes            climb_row_bytes(levels) = row_bytes(32, 32, levels)
// A path cut at levels c_0 < .. < c_G-1 (the mfh_merkle_*_cut calls) gives G + 1 rows an update: segment 0 is the statement's own row over the subtree of
// height c_0 -- the head, the first c_0 siblings of the level row, the index masked to c_0 bits (splice_cut_tail) -- and segment g >= 1 a MerkleSegment row
// of c_g - c_g-1 levels (c_G = depth), which k_merkle_cut_rows writes whole: its tail too starts at byte 128.
// A cut READ (mfh_merkle_paths_cut, mfh_merkle_absent_rows_cut) gives G + 1 rows a statement, all staged by ONE launch of k_merkle_climb_rows in one layout
// of 5 + 2 levels units, the tail at byte 64 as in a path row: segment 0 is the statement's own row over the subtree of height c_0 (a path row whole; under a
// head of records its tail alone is read, splice_row with depth = c_0) and segment g >= 1 a MerkleClimb row whole (ClimbPlan, climb_plan, climb_chunk).
// The kernels write whole rows where the tail lands on a 16-byte unit: k_merkle_paths the path row (tail at byte 64), k_merkle_update_level the level row
// (tail at byte 128), both staged at staged_stride of their bytes.  A head of records puts the tail anywhere, so for those statements the device stages two
// pieces per row and the host splices them while it copies out of the pinned buffer (splice_row):
//   the staged row  a path row or a level row; only its tail is read
//   the heads       what k_record_gather / k_absent_gather write: each record at the start of a slot of record_head_pitch(length) bytes (whole-unit stores)
// A key step (insert, remove) is two record updates: its row is spliced out of the heads and the level rows of both (splice_pair_row), the index bits written
// by the host.
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

// the row of a key step, two record updates (p, s) under one pair of roots: the key and nrec records in its head, then TWO tails' siblings and both indices' bits
inline size_t pair_row_bytes(uint32_t key_bytes, uint32_t nrec, uint32_t length, uint32_t depth, size_t zeros = 64) {
  return zeros + key_bytes + (size_t)nrec * length + (size_t)64 * depth + (2 * depth + 7) / 8;
}

inline size_t segment_row_bytes(uint32_t levels) { return row_bytes(64, 64, levels); }
// the 16-byte units of a staged segment row: 8 of nodes and zeros, 2 a sibling, 1 for the index
inline uint32_t segment_row_units(uint32_t levels) { return 9 + 2 * levels; }
// the staged bytes of the upper segments of ONE update of a path of `depth` levels cut at cuts[0 .. ncuts)
inline size_t cut_staged_bytes(uint32_t depth, uint32_t ncuts, const uint32_t *cuts) {
  size_t units = 0;
  for (uint32_t g = 0; g < ncuts; g++) units += segment_row_units((g + 1 < ncuts ? cuts[g + 1] : depth) - cuts[g]);
  return units * 16;
}
// ... and the bytes of their rows as the caller gets them
inline size_t cut_rows_bytes(uint32_t depth, uint32_t ncuts, const uint32_t *cuts) {
  size_t bytes = 0;
  for (uint32_t g = 0; g < ncuts; g++) bytes += segment_row_bytes((g + 1 < ncuts ? cuts[g + 1] : depth) - cuts[g]);
  return bytes;
}

// ---- cut reads.  Every segment of a read path is staged as 5 + 2 levels units of 16 bytes: 4 of node and zeros (a path row: zeros and leaf), 2 a sibling,
// 1 for the index.  The staged row's first climb_row_bytes(levels) bytes ARE the caller's row (the index unit's low bytes are its last bytes).
inline size_t climb_row_bytes(uint32_t levels) { return row_bytes(32, 32, levels); }
inline uint32_t climb_row_units(uint32_t levels) { return 5 + 2 * levels; }
// the levels of segment g = 0 .. ncuts of a path of `depth` levels cut at cuts[0 .. ncuts), and the level at which it starts
inline uint32_t climb_lo(uint32_t g, const uint32_t *cuts) { return g ? cuts[g - 1] : 0; }
inline uint32_t climb_levels(uint32_t g, uint32_t depth, uint32_t ncuts, const uint32_t *cuts) { return (g < ncuts ? cuts[g] : depth) - climb_lo(g, cuts); }
// the staged units of ALL ncuts + 1 segments of ONE statement
inline size_t climb_staged_units(uint32_t depth, uint32_t ncuts, const uint32_t *cuts) {
  size_t units = 0;
  for (uint32_t g = 0; g <= ncuts; g++) units += climb_row_units(climb_levels(g, depth, ncuts, cuts));
  return units;
}
// ... and the bytes of its UPPER segments' rows as the caller gets them (segment 0's row is the call's own)
inline size_t climb_rows_bytes(uint32_t depth, uint32_t ncuts, const uint32_t *cuts) {
  size_t bytes = 0;
  for (uint32_t g = 1; g <= ncuts; g++) bytes += climb_row_bytes(climb_levels(g, depth, ncuts, cuts));
  return bytes;
}
// the statements of one chunk of a cut read of n statements (n > 0) whose segment 0 row is rowb0 bytes: the most whose rows of ALL segments fit the stage
inline uint32_t climb_chunk(uint32_t n, size_t rowb0, uint32_t depth, uint32_t ncuts, const uint32_t *cuts, size_t stage_bytes) {
  return update_chunk(n, rowb0 + climb_rows_bytes(depth, ncuts, cuts), stage_bytes);
}

// The plan of k_merkle_climb_rows, handed to it by value: segment g covers levels [lo, lo + levels) and its k staged rows start at unit `base` of the stage, one
// segment behind the other; `head` is the unit of a row at which the stored node idx >> lo of level lo goes -- 2 in segment 0 (the leaf of a path row), 0 above
// it (the given node of a MerkleClimb row) -- or kClimbNoHead, the first unit behind the head, where the host splices a head of records and the four head units
// stay zero.
constexpr uint32_t kClimbMaxSegments = 24;  // cuts lie below the depth, and that is at most 24
constexpr uint32_t kClimbNoHead = 4;
struct ClimbPlan {
  uint32_t nseg;
  uint32_t lo[kClimbMaxSegments], levels[kClimbMaxSegments], base[kClimbMaxSegments], head[kClimbMaxSegments];
};
// (1 <= cuts[0] < .. < cuts[ncuts - 1] < depth <= 24, k > 0.)  *widest <- the most units of a row of any segment: the launch's items a statement
inline ClimbPlan climb_plan(uint32_t depth, uint32_t ncuts, const uint32_t *cuts, uint32_t k, bool leaf_head, uint32_t *widest) {
  ClimbPlan plan{};
  uint32_t units = 0, wide = 0;
  for (uint32_t g = 0; g <= ncuts; g++) {
    plan.lo[g] = climb_lo(g, cuts);
    plan.levels[g] = climb_levels(g, depth, ncuts, cuts);
    plan.base[g] = units;
    plan.head[g] = g ? 0 : leaf_head ? 2 : kClimbNoHead;
    units += k * climb_row_units(plan.levels[g]);
    if (climb_row_units(plan.levels[g]) > wide) wide = climb_row_units(plan.levels[g]);
  }
  plan.nseg = ncuts + 1;
  if (widest) *widest = wide;
  return plan;
}

// the updates of one chunk of a batch of nk key steps (nk > 0): the most STEPS whose rows of row_bytes fit the stage, at least one, two updates each -- always
// even, so both updates of a step are in one chunk even when one row alone exceeds the stage
inline uint32_t pair_chunk(uint32_t nk, size_t row_bytes, size_t stage_bytes) { return 2 * update_chunk(nk, row_bytes, stage_bytes); }

// What a batch of nk steps of R record updates each (R = 2: insert, remove, transfer; R = 1: adjust, write) keeps at the front of the device scratch for the
// whole call: fresh = the R nk new records at a pitch of record_head_pitch(length) | the plan, `words` words a step (the step's build kernel says which) | the
// keys, key_bytes a step, packed (0: none go up) | the payloads, pay a step, packed (0: none).  skip = their bytes rounded up to 16: behind them, one after the
// other, the call's searches and per chunk the updates' scratch.  ch: the updates a chunk -- whole steps whose rows of rowb bytes and, of a path cut at
// cuts[0 .. ncuts) (ncuts = 0: uncut), R MerkleSegment rows an upper segment fit the stage together, at least one step
struct StepLayout {
  uint32_t R, ch;
  size_t fresh_bytes, plan_bytes, keys_bytes, pay_bytes, skip, rowb;
  size_t up_bytes() const { return plan_bytes + keys_bytes + pay_bytes; }  // what goes up: all but fresh, which the build kernel writes
};

inline StepLayout step_layout(uint32_t R, uint32_t words, uint32_t nk, uint32_t length, size_t key_bytes, size_t pay, size_t rowb, uint32_t depth, uint32_t ncuts,
                              const uint32_t *cuts, size_t stage_bytes) {
  StepLayout s{};
  s.R = R;
  s.fresh_bytes = (size_t)R * nk * record_head_pitch(length);
  s.plan_bytes = (size_t)nk * words * 4;
  s.keys_bytes = (size_t)nk * key_bytes;
  s.pay_bytes = (size_t)nk * pay;
  s.skip = (s.fresh_bytes + s.up_bytes() + 15) & ~(size_t)15;
  s.rowb = rowb;
  s.ch = R * update_chunk(nk, rowb + R * cut_rows_bytes(depth, ncuts, cuts), stage_bytes);
  return s;
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

// at <- the tail of a segment-0 row: the first c0 siblings of the level row `staged` (tail at byte 128), then the ceil(c0 / 8) bytes of index mod 2^c0
inline void splice_cut_tail(uint8_t *at, const uint8_t *staged, uint32_t c0, uint32_t index) {
  memcpy(at, staged + 128, (size_t)32 * c0);
  const uint32_t low = index & (uint32_t)(((uint64_t)1 << c0) - 1);
  for (uint32_t b = 0; b < (c0 + 7) / 8; b++) at[(size_t)32 * c0 + b] = (uint8_t)(low >> (8 * b));
}

// row <- the climb_row_bytes(levels) bytes of a segment's row of a cut read out of its staged row; staged = nullptr (an absent query with no record): all zero
inline void splice_climb_row(uint8_t *row, const uint8_t *staged, uint32_t levels) {
  if (staged) memcpy(row, staged, climb_row_bytes(levels));
  else memset(row, 0, climb_row_bytes(levels));
}

// row <- the input row of a key step whose two updates' level rows are staged_p and staged_s (tails at byte 128): `zeros` zero bytes | the head's pieces, in
// order (the key, then the step's records out of the two updates' heads) | p's siblings | s's siblings | the index bytes of (p, s).  Reads the pieces' bytes --
// key_bytes and `length` each -- and 32 depth bytes of each level row; writes pair_row_bytes(key_bytes, nrec, length, depth, zeros) bytes and nothing behind
// them.  Segment 0 of a cut step (joined=False): zeros = 128, depth = c_0 -- the first c_0 siblings of each level row -- and p, s already reduced mod 2^c_0.
inline void splice_pair_row(uint8_t *row, size_t zeros, std::initializer_list<RowPiece> head, const uint8_t *staged_p, const uint8_t *staged_s, uint32_t depth,
                            uint32_t p, uint32_t s) {
  splice_row(row, zeros, head, nullptr, 0, 0);
  row += zeros;
  for (const RowPiece &h : head) row += h.bytes;
  memcpy(row, staged_p + 128, (size_t)32 * depth);
  memcpy(row + (size_t)32 * depth, staged_s + 128, (size_t)32 * depth);
  row += (size_t)64 * depth;
  const uint64_t bits = (uint64_t)p | (uint64_t)s << depth;  // (depth <= 24: 48 bits)
  for (uint32_t b = 0; b < (2 * depth + 7) / 8; b++) row[b] = (uint8_t)(bits >> (8 * b));
}

}  // namespace mf
