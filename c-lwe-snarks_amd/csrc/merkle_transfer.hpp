// merkle_transfer.hpp -- host only, plain C++: the plan of a batch of sequential transfers between the accounts of an indexed table (mfh_merkle_transfer_keys,
// merkle.hip), beside merkle_insert.hpp and merkle_remove.hpp.
//
// A record's balance is its bytes [2K, 2K + A), an unsigned big-endian integer, A = amount_bytes in [1, 8].  Transfer j = 0 .. nk - 1 moves amount[j] from the
// account `from[j]` to the account `to[j]`: record p_j, whose own key is the sender's, gets balance - amount, then record s_j, whose own key is the receiver's,
// gets balance + amount.  No key changes, so the records of the accounts are the ones the device found against the table BEFORE the batch -- but an account may
// occur in many steps, and a step sees the balances the earlier steps left: a later step may spend what an earlier step of the batch delivered.
// The accounts are the nu UNIQUE keys of the batch (keys_prepare's slots): from[j] and to[j] are positions among them, rec[u] the located record of unique key u
// (kNoRecord: not a member) and balance[u] its balance before the batch.  The plan walks the steps in order over a running balance per unique key:
//   status[j]   the first that applies: 1 the sender is no member, 2 the receiver is no member, 3 the sender's RUNNING balance is below the amount (an
//               overdraft), 4 the receiver's running balance plus the amount exceeds 2^(8A) - 1 (an overflow); else 0
//   a step with a status is NOT applied: the steps behind it see the balances without it
//   idx         the 2 nk record updates, in mfh_merkle_update_records' order: idx[2 j] = p_j, idx[2 j + 1] = s_j (kNoRecord where there is none)
//   fresh       the 2 nk new balances: fresh[2 j] the sender's right after step j, fresh[2 j + 1] the receiver's (of an applied step)
//   overdraft, overflow   the first step with status 3, with status 4; nk when there is none
// from[j] != to[j] (the caller refuses a transfer to oneself).  O(nk) behind keys_prepare's sort.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "merkle_keys.hpp"

namespace mf {

constexpr uint32_t kMaxAmountBytes = 8;

// the largest balance of amount_bytes bytes
inline uint64_t balance_limit(uint32_t amount_bytes) { return amount_bytes >= 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * amount_bytes)) - 1); }

struct TransferPlan {
  std::vector<uint32_t> idx;    // 2 nk
  std::vector<uint64_t> fresh;  // 2 nk
  std::vector<uint8_t> status;  // nk
  uint32_t overdraft = 0, overflow = 0, failed = 0;  // failed: the steps with a status
};

// balance: nu values, the accounts' balances before the batch; afterwards what the applied steps left
inline void transfer_plan(uint32_t nk, const uint32_t *from, const uint32_t *to, const uint64_t *amount, uint32_t amount_bytes, const uint32_t *rec,
                          uint64_t *balance, TransferPlan &out) {
  const uint64_t limit = balance_limit(amount_bytes);
  out.idx.resize((size_t)2 * nk);
  out.fresh.assign((size_t)2 * nk, 0);
  out.status.assign(nk, 0);
  out.overdraft = out.overflow = nk;
  out.failed = 0;
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t f = from[j], t = to[j];
    const uint64_t v = amount[j];
    out.idx[(size_t)2 * j] = rec[f];
    out.idx[(size_t)2 * j + 1] = rec[t];
    uint8_t st = 0;
    if (rec[f] == kNoRecord) st = 1;
    else if (rec[t] == kNoRecord) st = 2;
    else if (balance[f] < v) st = 3;
    else if (v > limit - balance[t]) st = 4;  // (balance[t] <= limit: no wrap)
    out.status[j] = st;
    if (st) {
      out.failed++;
      if (st == 3 && out.overdraft == nk) out.overdraft = j;
      if (st == 4 && out.overflow == nk) out.overflow = j;
      continue;
    }
    balance[f] -= v;
    balance[t] += v;
    out.fresh[(size_t)2 * j] = balance[f];
    out.fresh[(size_t)2 * j + 1] = balance[t];
  }
}

// at <- the amount_bytes big-endian bytes of a balance or an amount
inline void balance_bytes(uint64_t value, uint32_t amount_bytes, uint8_t *at) {
  for (uint32_t b = 0; b < amount_bytes; b++) at[b] = (uint8_t)(value >> (8 * (amount_bytes - 1 - b)));
}

}  // namespace mf
