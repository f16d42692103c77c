// merkle_adjust.hpp -- host only, plain C++: the plan of a batch of sequential deposits and withdrawals on the accounts of an indexed table
// (mfh_merkle_adjust_keys, merkle.hip), beside merkle_transfer.hpp.
//
// A record's balance is its bytes [2K, 2K + A), an unsigned big-endian integer, A = amount_bytes in [1, 8] (merkle_transfer.hpp).  Step j = 0 .. nk - 1 adds
// amount[j] to the balance of the account slot[j] (side[j] = 0, a deposit) or takes it off (side[j] = 1, a withdrawal).  No key changes, so the record of an
// account is the one the device found against the table BEFORE the batch -- but an account may occur in many steps, and a step sees the balance the earlier
// steps left: a withdrawal may spend what an earlier deposit of the batch delivered.
// The accounts are the nu UNIQUE keys of the batch (keys_prepare's slots): slot[j] is a position among them, rec[u] the located record of unique key u
// (kNoRecord: not a member) and balance[u] its balance before the batch.  The plan walks the steps in order over a running balance per unique key:
//   status[j]   the first that applies: 1 the key is no member, 3 a withdrawal above the RUNNING balance (an overdraft), 4 a deposit that takes the running
//               balance past 2^(8A) - 1 (an overflow); else 0.  2 stays unused: the numbers mean what transfer_plan's mean
//   a step with a status is NOT applied: the steps behind it see the balance without it
//   idx[j]      the record of step j (kNoRecord where there is none)
//   fresh[j]    the account's balance right after step j (of an applied step)
//   overdraft, overflow   the first step with status 3, with status 4; nk when there is none
//   failed      the steps with a status
// side = null: all deposits.  O(nk) behind keys_prepare's sort.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "merkle_keys.hpp"
#include "merkle_transfer.hpp"

namespace mf {

struct AdjustPlan {
  std::vector<uint32_t> idx;    // nk
  std::vector<uint64_t> fresh;  // nk
  std::vector<uint8_t> status;  // nk
  uint32_t overdraft = 0, overflow = 0, failed = 0;
};

// balance: nu values, the accounts' balances before the batch; afterwards what the applied steps left
inline void adjust_plan(uint32_t nk, const uint32_t *slot, const uint64_t *amount, const uint8_t *side, uint32_t amount_bytes, const uint32_t *rec, uint64_t *balance,
                        AdjustPlan &out) {
  const uint64_t limit = balance_limit(amount_bytes);
  out.idx.resize(nk);
  out.fresh.assign(nk, 0);
  out.status.assign(nk, 0);
  out.overdraft = out.overflow = nk;
  out.failed = 0;
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t u = slot[j];
    const uint64_t v = amount[j];
    const bool withdraw = side && side[j];
    out.idx[j] = rec[u];
    uint8_t st = 0;
    if (rec[u] == kNoRecord) st = 1;
    else if (withdraw && balance[u] < v) st = 3;
    else if (!withdraw && v > limit - balance[u]) st = 4;  // (balance[u] <= limit: no wrap)
    out.status[j] = st;
    if (st) {
      out.failed++;
      if (st == 3 && out.overdraft == nk) out.overdraft = j;
      if (st == 4 && out.overflow == nk) out.overflow = j;
      continue;
    }
    balance[u] = withdraw ? balance[u] - v : balance[u] + v;
    out.fresh[j] = balance[u];
  }
}

}  // namespace mf
