// The host side of mfh_merkle_adjust_keys (csrc/merkle_adjust.hpp: the running balances, the update index, the new balance and the status of every step of a
// batch of sequential deposits and withdrawals; csrc/merkle_rows.hpp: the adjust row's size and its splice) as a program of its own
// (tests/test_merkle_adjust_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <amount_bytes> <accounts> <nk> <mode> <seed>
// `accounts` random non-sentinel keys of 5 bytes stand in shuffled records of a table of 2 accounts + 3 slots, each with a balance of amount_bytes big-endian
// bytes behind its two keys; the other slots are inert.  The batches:
//   mode 0   nk random steps, both sides, among the accounts and two keys that are no members, amounts around the balances: keys repeat, a withdrawal may spend
//            what an earlier deposit delivered, and statuses 0, 1, 3 and 4 occur
//   mode 1   an account stands at the limit 2^(8 A) - 1 less nk - 1 (A = 8: next to 2^64 - 1, where balance + amount does not fit 64 bits): nk deposits of
//            one, the last of which is an overflow; then a deposit of the whole limit onto 0 (fine) and onto 1 (an overflow), a withdrawal of the whole limit
//            from the limit (fine), and the same deposits with side = null (all deposits)
//   mode 2   nk steps that are fine but for step pos, which overdraws by one (even pos) or overflows by one (odd pos) -- for every pos in turn: the first
//            failure is at pos, the steps behind it are judged without it, `failed` is 1
// Every batch goes through keys_prepare over the nk keys at a stride, the located record and the balance of every UNIQUE key as the device reports them, and
// adjust_plan -- every array a heap allocation of exactly its bytes -- and is checked against
//   the model    one step at a time on the table's BYTES: a linear scan for the live record whose lo is the key, the balance read and written as big-endian
//                bytes, sums in 128 bits -- idx, status and the new balance of every step, the first overdraft and the first overflow, the count of failed
//                steps, the balances left
//   the splice   (length = 10 + amount_bytes + seed % 7) at depth 1 + seed % 24: two rows at in_stride = row bytes + 3 out of heap arrays of exactly the bytes
//                the splice may read, uncut (splice_row with the staged tail) and cut at c_0 = 1 + seed % depth (splice_row, then splice_cut_tail), the rest of
//                the output untouched
// Prints "ok <amount_bytes> <accounts> <nk> <mode> <batches checked> <steps checked> <steps with a status> <row bytes>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "merkle_adjust.hpp"
#include "merkle_keys.hpp"
#include "merkle_rows.hpp"

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

template <class T>
static T *exact(size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (!p) exit(3);
  return p;
}

constexpr uint32_t K = 5;
typedef std::vector<uint8_t> Key;
struct Step {
  Key key;
  uint64_t amount;
  uint8_t side;
};

static unsigned g_a, g_acc, g_nk, g_mode;
#define CHECK(cond, what)                                                                                                  \
  do {                                                                                                                     \
    if (!(cond)) {                                                                                                         \
      fprintf(stderr, "merkle_adjust_host_check: amount_bytes %u accounts %u nk %u mode %u: %s\n", g_a, g_acc, g_nk, g_mode, what); \
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

// one batch against the model; want_overdraft / want_overflow: what the caller expects of the firsts, or -1.  no_sides: the batch is all deposits and goes to
// adjust_plan with side = null
static int check_batch(const Table &start, const std::vector<Step> &batch, long want_overdraft, long want_overflow, bool no_sides = false) {
  const uint32_t nk = (uint32_t)batch.size(), A = start.A, stride = K + 2;
  uint8_t *keys = exact<uint8_t>(nk ? (size_t)(nk - 1) * stride + K : 0);
  uint64_t *amount = exact<uint64_t>(nk);
  uint8_t *side = exact<uint8_t>(nk);
  for (uint32_t j = 0; j < nk; j++) {
    memcpy(keys + (size_t)j * stride, batch[j].key.data(), K);
    amount[j] = batch[j].amount;
    side[j] = batch[j].side;
    CHECK(!no_sides || !side[j], "a batch without sides is all deposits");
  }
  mf::KeyPlan plan_keys;
  mf::keys_prepare(keys, stride, K, nk, plan_keys);
  free(keys);
  const uint32_t nu = plan_keys.nu;
  uint32_t *rec = exact<uint32_t>(nu), *slot = exact<uint32_t>(nk);
  uint64_t *balance = exact<uint64_t>(nu);
  for (uint32_t j = 0; j < nk; j++) {  // what the search and k_balance_gather report per unique key
    const uint32_t u = plan_keys.slot[j];
    CHECK(u < nu, "a slot past the unique keys");
    slot[j] = u;
    rec[u] = start.own(batch[j].key);
    balance[u] = rec[u] == mf::kNoRecord ? 0 : (uint64_t)start.balance(rec[u]);
  }
  mf::AdjustPlan plan;
  mf::adjust_plan(nk, slot, amount, no_sides ? nullptr : side, A, rec, balance, plan);
  CHECK(plan.idx.size() == nk && plan.fresh.size() == nk && plan.status.size() == nk, "the plan's sizes");
  // the model: one step at a time on the bytes
  Table t = start;
  const unsigned __int128 limit = ((unsigned __int128)1 << (8 * A)) - 1;
  uint32_t overdraft = nk, overflow = nk, failed = 0;
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t i = t.own(batch[j].key);
    const unsigned __int128 v = batch[j].amount;
    uint8_t st = 0;
    if (i == mf::kNoRecord) st = 1;
    else if (batch[j].side && v > t.balance(i)) st = 3;
    else if (!batch[j].side && t.balance(i) + v > limit) st = 4;
    CHECK(plan.status[j] == st, "a step's status");
    CHECK(st != 2, "status 2 is unused");
    CHECK(plan.idx[j] == i, "a step's record");
    g_steps++;
    if (st) {
      g_failed++;
      failed++;
      if (st == 3 && overdraft == nk) overdraft = j;
      if (st == 4 && overflow == nk) overflow = j;
      continue;
    }
    t.set_balance(i, batch[j].side ? t.balance(i) - v : t.balance(i) + v);
    CHECK((unsigned __int128)plan.fresh[j] == t.balance(i), "a step's new balance");
    uint8_t be[8];
    mf::balance_bytes(plan.fresh[j], A, be);
    CHECK(!memcmp(be, t.rec[i].data() + 2 * K, A), "the new balance's big-endian bytes");
  }
  CHECK(plan.overdraft == overdraft && plan.overflow == overflow && plan.failed == failed, "the first overdraft, the first overflow, the failed steps");
  CHECK(want_overdraft < 0 || overdraft == (uint32_t)want_overdraft, "the batch's first overdraft is where it was put");
  CHECK(want_overflow < 0 || overflow == (uint32_t)want_overflow, "the batch's first overflow is where it was put");
  for (uint32_t j = 0; j < nk; j++)  // the balances left: what the applied steps made of them
    if (rec[slot[j]] != mf::kNoRecord) CHECK((unsigned __int128)balance[slot[j]] == t.balance(rec[slot[j]]), "a balance left behind the batch");
  free(rec);
  free(slot);
  free(balance);
  free(amount);
  free(side);
  return 0;
}

// two rows, uncut and cut, out of exact-size arrays
static int check_splice(uint32_t A, uint32_t length, uint32_t depth, uint32_t c0, size_t *rowb_out) {
  const size_t rowb = mf::row_bytes(64, (size_t)K + A + 1 + length, depth), stride = rowb + 3, tail = mf::row_tail_bytes(depth);
  *rowb_out = rowb;
  CHECK(rowb == 64 + K + A + 1 + length + (size_t)32 * depth + (depth + 7) / 8, "the row's bytes");
  uint8_t *out = exact<uint8_t>(2 * stride), *staged = exact<uint8_t>(128 + tail), *key = exact<uint8_t>(K), *amt = exact<uint8_t>(A), *head = exact<uint8_t>(length);
  for (size_t i = 0; i < 128 + tail; i++) staged[i] = rnd();
  for (uint32_t i = 0; i < K; i++) key[i] = rnd();
  for (uint32_t i = 0; i < A; i++) amt[i] = rnd();
  for (uint32_t i = 0; i < length; i++) head[i] = rnd();
  for (int cut = 0; cut < 2; cut++) {
    memset(out, 0xA5, 2 * stride);
    const uint32_t d0 = cut ? c0 : depth, index = (uint32_t)(rnd64() & ((1u << depth) - 1));
    const size_t rb = mf::row_bytes(64, (size_t)K + A + 1 + length, d0);
    for (int r = 0; r < 2; r++) {
      const uint8_t side = (uint8_t)r;
      uint8_t *row = out + r * stride;
      mf::splice_row(row, 64, {{key, K}, {amt, A}, {&side, 1}, {head, length}}, cut ? nullptr : staged, 128, depth);
      if (cut) mf::splice_cut_tail(row + 64 + K + A + 1 + length, staged, d0, index);
      for (size_t i = 0; i < 64; i++) CHECK(row[i] == 0, "the zero bytes");
      CHECK(!memcmp(row + 64, key, K) && !memcmp(row + 64 + K, amt, A) && row[64 + K + A] == side && !memcmp(row + 64 + K + A + 1, head, length), "the head's pieces");
      const uint8_t *t = row + 64 + K + A + 1 + length;
      CHECK(!memcmp(t, staged + 128, (size_t)32 * d0), "the siblings");
      if (!cut) CHECK(!memcmp(t, staged + 128, tail), "the staged tail");
      else
        for (uint32_t b = 0; b < (d0 + 7) / 8; b++) CHECK(t[(size_t)32 * d0 + b] == (uint8_t)((index & (uint32_t)(((uint64_t)1 << d0) - 1)) >> (8 * b)), "the index bytes mod 2^c_0");
      for (size_t i = rb; i < stride; i++) CHECK(row[i] == 0xA5, "a byte behind the row was written");
    }
  }
  free(out);
  free(staged);
  free(key);
  free(amt);
  free(head);
  return 0;
}

static int run(uint32_t A, uint32_t acc, uint32_t nk, uint32_t mode, uint64_t seed, unsigned *batches, size_t *rowb) {
  rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
  const uint64_t limit = mf::balance_limit(A);
  // a well-formed table: the accounts' keys sorted, record i = (k_i, k_i+1), the sentinel record and inert slots, shuffled
  std::vector<Key> keys;
  while (keys.size() < acc) {
    Key k(K);
    for (auto &b : k) b = rnd();
    if (mf::key_is_sentinel(k.data(), K) || std::find(keys.begin(), keys.end(), k) != keys.end()) continue;
    keys.push_back(k);
  }
  std::vector<Key> sorted = keys;
  std::sort(sorted.begin(), sorted.end());
  Table t{A, {}};
  const size_t slots = 2 * acc + 3;
  for (size_t i = 0; i <= acc; i++) {
    std::vector<uint8_t> r(2 * K + A, 0);
    if (i) memcpy(r.data(), sorted[i - 1].data(), K);
    if (i < acc) memcpy(r.data() + K, sorted[i].data(), K);
    else memset(r.data() + K, 0xFF, K);
    for (uint32_t b = 0; b < A; b++) r[2 * K + b] = rnd();
    t.rec.push_back(r);
  }
  while (t.rec.size() < slots) {  // inert: lo >= hi, any balance bytes
    std::vector<uint8_t> r(2 * K + A);
    for (auto &b : r) b = rnd();
    memcpy(r.data() + K, r.data(), K);
    if (rnd() & 1) r[K] = 0, r[0] |= 1;
    t.rec.push_back(r);
  }
  for (size_t i = t.rec.size() - 1; i > 0; i--) std::swap(t.rec[i], t.rec[rnd64() % (i + 1)]);
  *batches = 0;
  if (mode == 0) {
    Key stranger_a(K, 0x11), stranger_b(K, 0xEE);
    while (t.own(stranger_a) != mf::kNoRecord) stranger_a[0]++;
    while (t.own(stranger_b) != mf::kNoRecord) stranger_b[0]--;
    std::vector<Step> batch;
    for (uint32_t j = 0; j < nk; j++) {
      const unsigned pick = rnd();
      const Key &k = pick < 12 ? stranger_a : pick < 24 ? stranger_b : keys[rnd64() % acc];
      const uint32_t i = t.own(k);
      const uint64_t b = i == mf::kNoRecord ? 0 : (uint64_t)t.balance(i);
      const uint8_t side = rnd() & 1;
      uint64_t v;
      switch (rnd() & 3) {
        case 0: v = side ? b : limit - b; break;                  // exactly to the edge of the balance BEFORE the batch
        case 1: v = (side ? b : limit - b) / 2; break;
        case 2: v = rnd64() & limit; break;
        default: v = rnd() & 3; break;
      }
      batch.push_back({k, v, side});
    }
    if (check_batch(t, batch, -1, -1)) return 1;
    ++*batches;
  } else if (mode == 1) {
    const Key &a = keys[0], &zero = keys[1], &one = keys[2];
    t.set_balance(t.own(a), (unsigned __int128)limit - (nk - 1));
    t.set_balance(t.own(zero), 0);
    t.set_balance(t.own(one), 1);
    for (int no_sides = 0; no_sides < 2; no_sides++) {
      std::vector<Step> batch(nk, Step{a, 1, 0});
      if (check_batch(t, batch, -1, nk - 1, no_sides)) return 1;
      if (check_batch(t, {{zero, limit, 0}}, -1, 1, no_sides)) return 1;
      if (check_batch(t, {{one, limit, 0}}, -1, 0, no_sides)) return 1;
      if (check_batch(t, {{zero, limit, 0}, {one, limit - 1, 0}, {zero, 1, 0}, {one, 1, 0}}, -1, 2, no_sides)) return 1;
      *batches += 4;
    }
    if (check_batch(t, {{zero, limit, 0}, {zero, limit, 1}, {zero, 1, 1}}, 2, -1)) return 1;  // the whole limit in and out again, then one too many
    ++*batches;
  } else {
    for (uint32_t pos = 0; pos < nk; pos++) {
      const Key &a = keys[pos % acc];
      Table u = t;
      u.set_balance(u.own(a), pos & 1 ? (unsigned __int128)limit - nk : nk);  // every fine step moves one
      std::vector<Step> batch;
      const uint8_t side = pos & 1 ? 0 : 1;
      for (uint32_t j = 0; j < nk; j++) batch.push_back({a, 1, side});
      // before pos the steps moved pos units: what is left for step pos, plus one
      batch[pos].amount = (uint64_t)nk - pos + 1;
      if (check_batch(u, batch, side ? (long)pos : (long)nk, side ? (long)nk : (long)pos)) return 1;
      ++*batches;
    }
  }
  const uint32_t depth = 1 + (uint32_t)(seed % 24);
  return check_splice(A, 10 + A + (uint32_t)(seed % 7), depth, 1 + (uint32_t)(seed % depth), rowb);
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    unsigned A, acc, nk, mode;
    unsigned long long seed;
    if (sscanf(line, "%u %u %u %u %llu", &A, &acc, &nk, &mode, &seed) != 5) return 2;
    if (A < 1 || A > 8 || acc < 3 || acc > 64 || nk < 1 || nk > 4096 || mode > 2) return 2;
    if (mode != 0 && nk > 200) return 2;  // (modes 1 and 2 move nk units: they fit one byte of balance)
    g_a = A, g_acc = acc, g_nk = nk, g_mode = mode;
    g_steps = g_failed = 0;
    unsigned batches = 0;
    size_t rowb = 0;
    if (run(A, acc, nk, mode, seed, &batches, &rowb)) return 1;
    printf("ok %u %u %u %u %u %u %u %zu\n", A, acc, nk, mode, batches, g_steps, g_failed, rowb);
  }
  return 0;
}
