// merkle_block.hpp -- host only, plain C++: the plan of a BLOCK, a sequence of steps of mixed kinds on the records of an indexed table whose records carry a
// balance (mfh_merkle_block_keys, merkle.hip), beside merkle_transfer.hpp, merkle_adjust.hpp and merkle_write.hpp.
//
// Step j = 0 .. nk - 1 is one of
//   kBlockTransfer  (a = the sender, b = the receiver, amount): transfer_plan's step, two record updates, the sender's first
//   kBlockAdjust    (a = the account, amount, side): adjust_plan's step, one record update
//   kBlockWrite     (a = the key, the field [lo, hi), value, expect or null): write_plan's step with a field of its OWN, one record update
// The balance is a record's bytes [2K, 2K + A), unsigned big-endian (merkle_transfer.hpp); a write may cover them, and a later transfer or adjust then reads
// the balance those bytes spell.  No step changes a key, so the record of a key is the one the device found against the table BEFORE the block.
//
// WINDOWS.  The keys are the nu UNIQUE keys of the block (keys_prepare's slots over the senders, receivers, accounts and written keys of all steps): a, b are
// positions among them.  Unique key u has ONE window [f0_u, f1_u) of its record: the hull of everything its steps touch -- the balance field for every
// transfer or adjust it occurs in, [lo, hi) for every write.  The device gathers the windows' bytes before the block into slots of whole 16-byte units,
// ceil((f1_u - f0_u) / 16) of them, key u's first unit at first[u], a prefix sum (block_windows; the total stays below 2^32 units): an account that only
// moves money costs one unit whatever another key's memo field is.
//
// block_plan walks the steps in order over the running window BYTES of every unique key, seeded from the gather:
//   status[j]   the first that applies, with the numbers the three calls use: 1 the key (a transfer's sender) is no member, 2 a transfer's receiver is no
//               member, 3 an overdraft against the RUNNING balance, 4 an overflow of the running balance, 5 the RUNNING field is not what the step expects
//   a step with a status is NOT applied: the steps behind it see the state without it
//   index[2 j], index[2 j + 1]   the step's records: (p, s) of a transfer, (the record, kNoRecord) of a one-record step; kNoRecord where there is none
//   first, failed                the first step with a status (nk: none), the steps with a status
// and, with skip = true or no failed step, the UPDATES of the applied steps in mfh_merkle_update_records' order:
//   first_update[nk + 1]   step j's updates are [first_update[j], first_update[j + 1]): 0 of a skipped step, 1 or 2
//   upd[r]                 update r's table record, its key's window (f0, f1) and `at`, where in `src` the window's f1 - f0 bytes RIGHT AFTER the step stand: a
//                          transfer's sender after the debit, then its receiver after the credit
// With skip = false and a failed step there is no update: first_update is all zero.  O(sum of the steps' window bytes) behind keys_prepare's sort.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "merkle_keys.hpp"
#include "merkle_rows.hpp"
#include "merkle_transfer.hpp"

namespace mf {

constexpr uint8_t kBlockTransfer = 0, kBlockAdjust = 1, kBlockWrite = 2;
inline uint32_t block_step_updates(uint8_t kind) { return kind == kBlockTransfer ? 2 : 1; }

struct BlockStep {
  uint8_t kind, side;
  uint32_t a, b;         // positions among the unique keys (b: a transfer's receiver)
  uint64_t amount;       // transfer, adjust
  uint32_t lo, hi;       // write
  const uint8_t *value;  // write: hi - lo bytes
  const uint8_t *expect; // write: hi - lo bytes, or null
};

// the windows of the nu unique keys and their gather slots: what k_window_gather reads per key is (f0, f1, first)
struct BlockWindows {
  std::vector<uint32_t> f0, f1, first;  // nu, nu, nu + 1: first[nu] = the units of all slots
  uint64_t units = 0;                   // (below 2^32 where the caller has bounded the new records' units: nu <= 2 nk keys, a window no longer than a record)
  uint64_t max_updates = 0, max_src = 0;  // the updates of all steps, and their windows' bytes: what the block's scratch is sized by; the caller refuses max_src >= 2^32
  uint32_t bytes(uint32_t u) const { return f1[u] > f0[u] ? f1[u] - f0[u] : 0; }  // (0: a key no step names; the driver has none)
};

inline void block_windows(uint32_t nk, const BlockStep *steps, uint32_t nu, uint32_t key_bytes, uint32_t amount_bytes, BlockWindows &w) {
  w.f0.assign(nu, 0xFFFFFFFFu);
  w.f1.assign(nu, 0);
  auto touch = [&](uint32_t u, uint32_t lo, uint32_t hi) {
    if (lo < w.f0[u]) w.f0[u] = lo;
    if (hi > w.f1[u]) w.f1[u] = hi;
  };
  for (uint32_t j = 0; j < nk; j++) {
    const BlockStep &s = steps[j];
    if (s.kind == kBlockWrite) touch(s.a, s.lo, s.hi);
    else touch(s.a, 2 * key_bytes, 2 * key_bytes + amount_bytes);
    if (s.kind == kBlockTransfer) touch(s.b, 2 * key_bytes, 2 * key_bytes + amount_bytes);
  }
  w.first.assign((size_t)nu + 1, 0);
  w.units = 0;
  for (uint32_t u = 0; u < nu; u++) {
    w.first[u] = (uint32_t)w.units;
    w.units += (w.bytes(u) + 15) / 16;
  }
  w.first[nu] = (uint32_t)w.units;
  w.max_updates = w.max_src = 0;
  for (uint32_t j = 0; j < nk; j++) {
    w.max_updates += block_step_updates(steps[j].kind);
    w.max_src += w.bytes(steps[j].a);
    if (steps[j].kind == kBlockTransfer) w.max_src += w.bytes(steps[j].b);
  }
}

struct BlockUpdate {
  uint32_t rec, f0, f1, at;  // (what k_window_records reads per update, in this order)
};

struct BlockPlan {
  std::vector<uint8_t> status;         // nk
  std::vector<uint32_t> index;         // 2 nk
  std::vector<uint32_t> first_update;  // nk + 1
  std::vector<BlockUpdate> upd;        // first_update[nk]
  std::vector<uint8_t> src;            // the updates' window bytes, one behind the other
  uint32_t first = 0, failed = 0;
};

// the A big-endian bytes at `at` as one integer
inline uint64_t balance_of(const uint8_t *at, uint32_t amount_bytes) {
  uint64_t v = 0;
  for (uint32_t b = 0; b < amount_bytes; b++) v = v << 8 | at[b];
  return v;
}

// win: the gathered slots, first[nu] units of 16 bytes, key u's window bytes from 16 first[u] on; afterwards what the applied steps left.  Only a slot's first
// f1 - f0 bytes are read or written.  rec[u]: the located record of unique key u, or kNoRecord
inline void block_plan(uint32_t nk, const BlockStep *steps, uint32_t key_bytes, uint32_t amount_bytes, const BlockWindows &w, const uint32_t *rec, uint8_t *win,
                       bool skip, BlockPlan &out) {
  const uint32_t K = key_bytes, A = amount_bytes;
  const uint64_t limit = balance_limit(A);
  out.status.assign(nk, 0);
  out.index.assign((size_t)2 * nk, kNoRecord);
  out.first_update.assign((size_t)nk + 1, 0);
  out.upd.clear();
  out.src.clear();
  out.first = nk;
  out.failed = 0;
  auto window = [&](uint32_t u) { return win + (size_t)16 * w.first[u]; };
  auto balance = [&](uint32_t u) { return window(u) + (2 * K - w.f0[u]); };  // (a key of a transfer or an adjust: its window holds the balance field)
  auto update = [&](uint32_t u) {
    out.upd.push_back({rec[u], w.f0[u], w.f1[u], (uint32_t)out.src.size()});
    out.src.insert(out.src.end(), window(u), window(u) + w.bytes(u));
  };
  for (uint32_t j = 0; j < nk; j++) {
    const BlockStep &s = steps[j];
    out.index[(size_t)2 * j] = rec[s.a];
    if (s.kind == kBlockTransfer) out.index[(size_t)2 * j + 1] = rec[s.b];
    uint8_t st = 0;
    if (rec[s.a] == kNoRecord) st = 1;
    else if (s.kind == kBlockTransfer) {
      if (rec[s.b] == kNoRecord) st = 2;
      else if (balance_of(balance(s.a), A) < s.amount) st = 3;
      else if (s.amount > limit - balance_of(balance(s.b), A)) st = 4;  // (a balance of A bytes <= limit: no wrap)
    } else if (s.kind == kBlockAdjust) {
      const uint64_t b = balance_of(balance(s.a), A);
      if (s.side && b < s.amount) st = 3;
      else if (!s.side && s.amount > limit - b) st = 4;
    } else if (s.expect && memcmp(window(s.a) + (s.lo - w.f0[s.a]), s.expect, s.hi - s.lo)) st = 5;
    out.status[j] = st;
    if (st) {
      out.failed++;
      if (out.first == nk) out.first = j;
    } else if (s.kind == kBlockTransfer) {
      balance_bytes(balance_of(balance(s.a), A) - s.amount, A, balance(s.a));
      update(s.a);
      balance_bytes(balance_of(balance(s.b), A) + s.amount, A, balance(s.b));
      update(s.b);
    } else if (s.kind == kBlockAdjust) {
      const uint64_t b = balance_of(balance(s.a), A);
      balance_bytes(s.side ? b - s.amount : b + s.amount, A, balance(s.a));
      update(s.a);
    } else {
      memcpy(window(s.a) + (s.lo - w.f0[s.a]), s.value, s.hi - s.lo);
      update(s.a);
    }
    out.first_update[(size_t)j + 1] = (uint32_t)out.upd.size();
  }
  if (out.failed && !skip) {  // fail-fast: nothing is applied
    out.first_update.assign((size_t)nk + 1, 0);
    out.upd.clear();
    out.src.clear();
  }
}

// a step's row bytes by kind, field, expectation and depth (merkle_rows.hpp): transfer_keys', adjust_keys' or write_keys' row.  cut: segment 0 of a cut call,
// `depth` = c_0 -- a transfer's row then has 128 zero bytes in front (joined=False)
inline size_t block_row_bytes(uint8_t kind, uint32_t key_bytes, uint32_t amount_bytes, uint32_t length, uint32_t depth, uint32_t lo, uint32_t hi, bool expect, bool cut) {
  if (kind == kBlockTransfer) return pair_row_bytes(2 * key_bytes + amount_bytes, 2, length, depth, cut ? 128 : 64);
  if (kind == kBlockAdjust) return row_bytes(64, (size_t)key_bytes + amount_bytes + 1 + length, depth);
  return row_bytes(64, (size_t)key_bytes + (expect ? 2 : 1) * (size_t)(hi - lo) + length, depth);
}

// What a block keeps at the front of the device scratch for the whole call: fresh = the new records of max_updates updates at a pitch of
// record_head_pitch(length) | the update descriptors, 16 bytes each | the source bytes, max_src of them.  skip = their bytes rounded up to 16: behind them, one
// after the other, the search with the windows' gather and per chunk the updates' scratch.  ch: the updates a chunk, UNIFORM as record_updates has them --
// the most whose rows fit the stage when every update is charged rowb bytes, the most row bytes an update of any step of the block stands for (a transfer's
// row is two updates'), and, of a path cut at cuts[0 .. ncuts), one MerkleSegment row an upper segment; at least one.  A transfer's two updates may fall into
// two chunks
struct BlockLayout {
  uint32_t ch;
  size_t fresh_bytes, desc_bytes, src_bytes, skip, rowb;
  size_t up_bytes() const { return desc_bytes + src_bytes; }  // what goes up: all but fresh, which k_window_records writes
};

inline BlockLayout block_layout(uint32_t max_updates, size_t max_src, uint32_t length, size_t rowb, uint32_t depth, uint32_t ncuts, const uint32_t *cuts,
                                size_t stage_bytes) {
  BlockLayout s{};
  s.fresh_bytes = (size_t)max_updates * record_head_pitch(length);
  s.desc_bytes = (size_t)max_updates * 16;
  s.src_bytes = max_src;
  s.skip = (s.fresh_bytes + s.up_bytes() + 15) & ~(size_t)15;
  s.rowb = rowb;
  s.ch = update_chunk(max_updates, rowb + cut_rows_bytes(depth, ncuts, cuts), stage_bytes);
  return s;
}

}  // namespace mf
