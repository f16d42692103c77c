// The host side of mfh_merkle_transfer_keys (csrc/merkle_transfer.hpp: the running balances, the 2 nk update indices, the new balances and the status of a batch
// of sequential transfers; csrc/merkle_rows.hpp: the transfer row's size and its splice) as a program of its own (tests/test_merkle_transfer_host_cpu.py builds
// it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <amount_bytes> <accounts> <nk> <mode> <seed>
// `accounts` random non-sentinel keys of 5 bytes stand in shuffled records of a table of 2 accounts + 3 slots, each with a balance of amount_bytes big-endian
// bytes behind its two keys; the other slots are inert.  The batches:
//   mode 0   ONE account sends nk times (nk = 3: three times) to the others in turn, within its balance; then once more than is left: an overdraft at the end
//   mode 1   a chain a -> b -> c ...: account i + 1 starts at 0 and sends on the amount it has just received, nk steps; then the same chain BACKWARDS in one
//            batch, in which every step but the last overdraws
//   mode 2   nk steps that are fine but for step pos, which overdraws by one -- for every pos in turn: the first overdraft is at pos, the steps behind it are
//            judged without it
//   mode 3   the receiver stands at the limit 2^(8 A) - 1 less nk - 1: nk transfers of one, the last of which is an overflow; then an amount of the whole
//            limit to an account at 0 (fine) and to an account at 1 (an overflow)
//   mode 4   nk random steps among the accounts and two keys that are no members, amounts around the balances: all four statuses occur
// Every batch goes through keys_prepare over all 2 nk keys (a key occurs many times), the located record and the balance of every UNIQUE key as the device
// reports them, and transfer_plan, and is checked against
//   the model    one step at a time on the table's BYTES: a linear scan for the live record whose lo is the key, the balances read and written as big-endian
//                bytes, sums in 128 bits -- idx, status and both new balances of every step, the first overdraft and the first overflow, the balances left
//   the splice   (length = 10 + amount_bytes + seed % 7) at depth 1 + seed % 24, 3 and 4 and zeros = 64 and 128: two rows at in_stride = row bytes + 3 out of
//                heap arrays of exactly the bytes the splice may read, the rest of the output untouched
// Prints "ok <amount_bytes> <accounts> <nk> <mode> <batches checked> <steps checked> <steps with a status> <row bytes>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "merkle_keys.hpp"
#include "merkle_rows.hpp"
#include "merkle_transfer.hpp"

static uint64_t rng_state;
static uint8_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint8_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 56);
}
static uint64_t rnd64() {
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v = v << 8 | rnd();
  return v;
}

static uint8_t *exact(size_t bytes) {
  uint8_t *p = (uint8_t *)malloc(bytes ? bytes : 1);
  if (!p) exit(3);
  return p;
}

constexpr uint32_t K = 5;
typedef std::vector<uint8_t> Key;
struct Step {
  Key from, to;
  uint64_t amount;
};

static unsigned g_a, g_acc, g_nk, g_mode;
#define CHECK(cond, what)                                                                                                  \
  do {                                                                                                                     \
    if (!(cond)) {                                                                                                         \
      fprintf(stderr, "merkle_transfer_host_check: amount_bytes %u accounts %u nk %u mode %u: %s\n", g_a, g_acc, g_nk, g_mode, what); \
      return 1;                                                                                                            \
    }                                                                                                                      \
  } while (0)

// the table: records of 2 K + A bytes, lo | hi | balance
struct Table {
  uint32_t A;
  std::vector<std::vector<uint8_t>> rec;
  bool live(size_t i) const { return memcmp(rec[i].data(), rec[i].data() + K, K) < 0; }
  uint32_t own(const Key &key) const {
    for (size_t i = 0; i < rec.size(); i++)
      if (live(i) && !memcmp(rec[i].data(), key.data(), K)) return (uint32_t)i;
    return mf::kNoRecord;
  }
  unsigned __int128 balance(uint32_t i) const {
    unsigned __int128 v = 0;
    for (uint32_t b = 0; b < A; b++) v = v << 8 | rec[i][2 * K + b];
    return v;
  }
  void set_balance(uint32_t i, unsigned __int128 v) {
    for (uint32_t b = 0; b < A; b++) rec[i][2 * K + b] = (uint8_t)(v >> (8 * (A - 1 - b)));
  }
};

static unsigned g_steps, g_failed;

// one batch against the model; *want_overdraft / *want_overflow: what the caller expects of the firsts, or -1
static int check_batch(const Table &start, const std::vector<Step> &batch, long want_overdraft, long want_overflow) {
  const uint32_t nk = (uint32_t)batch.size(), A = start.A, stride = K + 2;
  // the keys as the call lays them out: from, to, from, to .. packed; here with a stride, in an allocation of exactly its bytes
  uint8_t *keys = exact(nk ? (size_t)(2 * nk - 1) * stride + K : 0);
  for (uint32_t j = 0; j < nk; j++) {
    memcpy(keys + (size_t)2 * j * stride, batch[j].from.data(), K);
    memcpy(keys + ((size_t)2 * j + 1) * stride, batch[j].to.data(), K);
  }
  mf::KeyPlan plan_keys;
  mf::keys_prepare(keys, stride, K, 2 * nk, plan_keys);
  const uint32_t nu = plan_keys.nu;
  std::vector<uint32_t> rec(nu, mf::kNoRecord), from(nk), to(nk);
  std::vector<uint64_t> balance(nu, 0), amount(nk);
  for (uint32_t q = 0; q < 2 * nk; q++) {  // what the search and k_balance_gather report per unique key
    const Key &key = q & 1 ? batch[q / 2].to : batch[q / 2].from;
    const uint32_t u = plan_keys.slot[q];
    CHECK(u < nu, "a slot past the unique keys");
    rec[u] = start.own(key);
    balance[u] = rec[u] == mf::kNoRecord ? 0 : (uint64_t)start.balance(rec[u]);
  }
  free(keys);
  for (uint32_t j = 0; j < nk; j++) {
    from[j] = plan_keys.slot[2 * (size_t)j];
    to[j] = plan_keys.slot[2 * (size_t)j + 1];
    amount[j] = batch[j].amount;
  }
  mf::TransferPlan plan;
  mf::transfer_plan(nk, from.data(), to.data(), amount.data(), A, rec.data(), balance.data(), plan);
  CHECK(plan.idx.size() == (size_t)2 * nk && plan.fresh.size() == (size_t)2 * nk && plan.status.size() == nk, "the plan's sizes");
  // the model: one step at a time on the bytes
  Table t = start;
  const unsigned __int128 limit = ((unsigned __int128)1 << (8 * A)) - 1;
  CHECK((uint64_t)limit == mf::balance_limit(A), "balance_limit");
  uint32_t first_overdraft = nk, first_overflow = nk, failed = 0;
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t p = t.own(batch[j].from), s = t.own(batch[j].to);
    const unsigned __int128 v = batch[j].amount;
    uint8_t st = 0;
    if (p == mf::kNoRecord) st = 1;
    else if (s == mf::kNoRecord) st = 2;
    else if (t.balance(p) < v) st = 3;
    else if (t.balance(s) + v > limit) st = 4;
    CHECK(plan.idx[2 * (size_t)j] == p && plan.idx[2 * (size_t)j + 1] == s, "idx is not the model's (p, s)");
    CHECK(plan.status[j] == st, "the status is not the model's");
    g_steps++;
    if (st) {
      failed++, g_failed++;
      if (st == 3 && first_overdraft == nk) first_overdraft = j;
      if (st == 4 && first_overflow == nk) first_overflow = j;
      continue;
    }
    t.set_balance(p, t.balance(p) - v);
    t.set_balance(s, t.balance(s) + v);
    CHECK(plan.fresh[2 * (size_t)j] == (uint64_t)t.balance(p) && plan.fresh[2 * (size_t)j + 1] == (uint64_t)t.balance(s), "a new balance is not the model's");
    uint8_t be[8];
    mf::balance_bytes(plan.fresh[2 * (size_t)j], A, be);
    CHECK(!memcmp(be, t.rec[p].data() + 2 * K, A), "balance_bytes");
  }
  CHECK(plan.overdraft == first_overdraft && plan.overflow == first_overflow && plan.failed == failed, "the first overdraft, the first overflow or the count");
  CHECK(want_overdraft < 0 || first_overdraft == (uint32_t)want_overdraft, "the first overdraft is not where the batch put it");
  CHECK(want_overflow < 0 || first_overflow == (uint32_t)want_overflow, "the first overflow is not where the batch put it");
  for (uint32_t u = 0; u < nu; u++)
    if (rec[u] != mf::kNoRecord) CHECK(balance[u] == (uint64_t)t.balance(rec[u]), "a balance left is not the model's");
  // conservation: the applied steps move, they do not make
  unsigned __int128 before = 0, after = 0;
  for (size_t i = 0; i < start.rec.size(); i++)
    if (start.live(i)) before += start.balance((uint32_t)i), after += t.balance((uint32_t)i);
  CHECK(before == after, "the sum of the balances changed");
  return 0;
}

template <class T>
static void shuffle(std::vector<T> &v) {
  for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd64() % i]);
}

int main() {
  unsigned A, acc, nk, mode;
  unsigned long long seed;
  int got;
  while ((got = scanf("%u %u %u %u %llu", &A, &acc, &nk, &mode, &seed)) == 5) {
    if (A < 1 || A > 8 || acc < 3 || acc > 64 || nk < 1 || nk > 4096 || mode > 4 || (mode == 3 && nk > 200) || (mode == 0 && nk > 32)) return 2;
    g_a = A, g_acc = acc, g_nk = nk, g_mode = mode, g_steps = g_failed = 0;
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const uint64_t limit = mf::balance_limit(A);
    std::vector<Key> members;
    while (members.size() < acc + 2) {  // the last two are no members of the table
      Key k(K);
      for (auto &b : k) b = rnd();
      if (mf::key_is_sentinel(k.data(), K) || std::find(members.begin(), members.end(), k) != members.end()) continue;
      members.push_back(k);
    }
    const Key ghost_a = members[acc], ghost_b = members[acc + 1];
    members.resize(acc);
    std::sort(members.begin(), members.end());
    Table table{A, std::vector<std::vector<uint8_t>>(2 * acc + 3, std::vector<uint8_t>(2 * K + A, 0))};
    std::vector<uint32_t> pos(table.rec.size());
    for (size_t i = 0; i < pos.size(); i++) pos[i] = (uint32_t)i;
    shuffle(pos);
    for (size_t r = 0; r <= acc; r++) {  // record 0 the sentinel's; lo | hi
      std::vector<uint8_t> &rec = table.rec[pos[r]];
      if (r) memcpy(rec.data(), members[r - 1].data(), K);
      if (r < acc) memcpy(rec.data() + K, members[r].data(), K); else memset(rec.data() + K, 0xFF, K);
    }
    for (size_t r = acc + 1; r < pos.size(); r++)
      if (rnd() & 1) memset(table.rec[pos[r]].data(), 0xFF, r & 1 ? 2 * K : K);  // inert slots that are not all zero: lo == hi and lo > hi
    shuffle(members);  // account i, in no order
    auto slot = [&](unsigned i) { return table.own(members[i]); };
    unsigned batches = 0;
    if (mode == 0) {
      const uint64_t each = std::max<uint64_t>(1, limit / (4 * (uint64_t)nk));
      table.set_balance(slot(0), (unsigned __int128)each * nk + each / 2);
      std::vector<Step> batch;
      for (unsigned j = 0; j < nk; j++) batch.push_back({members[0], members[1 + j % (acc - 1)], each});
      if (int rc = check_batch(table, batch, nk, nk)) return rc;
      batch.push_back({members[0], members[1], each / 2 + 1});  // one more than is left
      if (int rc = check_batch(table, batch, nk, nk + 1)) return rc;
      batches = 2;
    } else if (mode == 1) {
      const uint64_t v = 1 + rnd64() % limit;
      table.set_balance(slot(0), v);
      std::vector<Step> batch;
      for (unsigned j = 0; j < nk; j++) batch.push_back({members[j % acc], members[(j + 1) % acc], v});
      if (int rc = check_batch(table, batch, nk, nk)) return rc;
      std::reverse(batch.begin(), batch.end());  // the last step first: nobody but account 0 has anything yet
      const long first = batch[0].from == members[0] ? (nk > 1 ? 1 : (long)nk) : 0;
      if (int rc = check_batch(table, batch, first, -1)) return rc;
      batches = 2;
    } else if (mode == 2) {
      for (unsigned i = 0; i < acc; i++) table.set_balance(slot(i), 10 + i);
      for (unsigned at = 0; at < nk; at++) {
        std::vector<Step> batch;
        std::vector<uint64_t> run(acc);
        for (unsigned i = 0; i < acc; i++) run[i] = 10 + i;
        for (unsigned j = 0; j < nk; j++) {
          const unsigned f = rnd() % acc, t = (f + 1 + rnd() % (acc - 1)) % acc;
          if (j == at) {
            batch.push_back({members[f], members[t], run[f] + 1});  // one more than the sender has at that step: not applied
            continue;
          }
          const uint64_t v = run[f] ? rnd64() % (run[f] + 1) : 0;
          if (run[t] + v > limit) {  // (A = 1: keep the receiver under the limit)
            batch.push_back({members[f], members[t], 0});
            continue;
          }
          run[f] -= v, run[t] += v;
          batch.push_back({members[f], members[t], v});
        }
        if (int rc = check_batch(table, batch, at, nk)) return rc;
        batches++;
      }
    } else if (mode == 3) {
      table.set_balance(slot(0), limit - (nk - 1));
      table.set_balance(slot(1), nk);
      std::vector<Step> batch(nk, Step{members[1], members[0], 1});
      if (int rc = check_batch(table, batch, nk, nk - 1)) return rc;
      table.set_balance(slot(0), limit);
      table.set_balance(slot(1), 0);
      table.set_balance(slot(2), 1);
      if (int rc = check_batch(table, {{members[0], members[1], limit}}, 1, 1)) return rc;
      if (int rc = check_batch(table, {{members[0], members[2], limit}}, 1, 0)) return rc;
      if (int rc = check_batch(table, {{members[0], members[2], limit - 1}, {members[1], members[2], 0}, {members[0], members[2], 1}}, 3, 2)) return rc;
      batches = 4;
    } else {
      for (unsigned i = 0; i < acc; i++) table.set_balance(slot(i), rnd() & 1 ? rnd64() % (limit / 2 + 1) : limit - rnd() % 3);
      std::vector<Step> batch;
      for (unsigned j = 0; j < nk; j++) {
        const unsigned f = rnd() % acc, t = (f + 1 + rnd() % (acc - 1)) % acc, odd = rnd() % 16;
        const uint64_t have = (uint64_t)table.balance(slot(f));
        const uint64_t v = rnd() & 1 ? rnd64() % (have / 4 + 2) : (rnd() & 1 ? have : rnd64() % (limit / 2 + 1));
        batch.push_back({odd == 0 ? ghost_a : members[f], odd == 1 ? ghost_b : members[t], v});
      }
      if (int rc = check_batch(table, batch, -1, -1)) return rc;
      batches = 1;
    }
    // the splice
    const uint32_t length = 2 * K + A + (uint32_t)(seed % 7);
    size_t rowb_seed = 0;
    for (uint32_t depth : {1 + (uint32_t)(seed % 24), 3u, 4u})
      for (size_t zeros : {(size_t)64, (size_t)128}) {
        const size_t idxb = (2 * depth + 7) / 8, rowb = mf::pair_row_bytes(2 * K + A, 2, length, depth, zeros), in_stride = rowb + 3;
        if (!rowb_seed) rowb_seed = rowb;
        CHECK(rowb == zeros + 2 * (size_t)K + A + 2 * (size_t)length + 64 * (size_t)depth + idxb, "the sizes differ");
        const unsigned nr = 2;
        const size_t out_bytes = (size_t)(nr - 1) * in_stride + rowb, staged_bytes = 128 + (size_t)32 * depth;
        uint8_t *head_p = exact(length), *head_s = exact(length), *staged_p = exact(staged_bytes), *staged_s = exact(staged_bytes), *out = exact(out_bytes), *want = exact(out_bytes);
        uint8_t *k_from = exact(K), *k_to = exact(K), *v = exact(A);
        for (size_t i = 0; i < K; i++) { k_from[i] = rnd(); k_to[i] = rnd(); }
        mf::balance_bytes(rnd64() & limit, A, v);
        for (size_t i = 0; i < length; i++) { head_p[i] = rnd(); head_s[i] = rnd(); }
        for (size_t i = 0; i < staged_bytes; i++) { staged_p[i] = rnd(); staged_s[i] = rnd(); }
        memset(out, 0xA5, out_bytes);
        memset(want, 0xA5, out_bytes);
        for (unsigned k = 0; k < nr; k++) {
          const uint32_t p = (uint32_t)rnd64() & ((1u << depth) - 1), s = k ? (1u << depth) - 1 : (uint32_t)rnd64() & ((1u << depth) - 1);
          uint8_t *w = want + k * in_stride;
          size_t at = 0;
          for (size_t i = 0; i < zeros; i++) w[at++] = 0;
          for (unsigned i = 0; i < K; i++) w[at++] = k_from[i];
          for (unsigned i = 0; i < K; i++) w[at++] = k_to[i];
          for (unsigned i = 0; i < A; i++) w[at++] = v[i];
          for (unsigned i = 0; i < length; i++) w[at++] = head_p[i];
          for (unsigned i = 0; i < length; i++) w[at++] = head_s[i];
          for (size_t i = 0; i < (size_t)32 * depth; i++) w[at++] = staged_p[128 + i];
          for (size_t i = 0; i < (size_t)32 * depth; i++) w[at++] = staged_s[128 + i];
          for (size_t i = 0; i < idxb; i++) w[at + i] = 0;
          for (uint32_t l = 0; l < depth; l++) {
            if ((p >> l) & 1) w[at + l / 8] |= (uint8_t)(1u << (l % 8));
            if ((s >> l) & 1) w[at + (depth + l) / 8] |= (uint8_t)(1u << ((depth + l) % 8));
          }
          CHECK(at + idxb == rowb, "the row's size");
          mf::splice_pair_row(out + k * in_stride, zeros, {{k_from, K}, {k_to, K}, {v, A}, {head_p, length}, {head_s, length}}, staged_p, staged_s, depth, p, s);
        }
        const bool same = !memcmp(out, want, out_bytes);
        free(head_p); free(head_s); free(staged_p); free(staged_s); free(out); free(want); free(k_from); free(k_to); free(v);
        CHECK(same, "the rows differ");
      }
    printf("ok %u %u %u %u %u %u %u %zu\n", A, acc, nk, mode, batches, g_steps, g_failed, rowb_seed);
  }
  return got == EOF ? 0 : 2;
}
