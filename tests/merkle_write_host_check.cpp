// The host side of mfh_merkle_write_keys (csrc/merkle_write.hpp: the running field value of every unique key, the update index and the status of every step of
// a batch of sequential writes, plain and compare-and-set; csrc/merkle_rows.hpp: the write row's size and its splice) as a program of its own
// (tests/test_merkle_write_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <field_bytes> <members> <nk> <mode> <seed>
// `members` random non-sentinel keys of 5 bytes stand in shuffled records of a table of 2 members + 3 slots; a record is lo | hi | 2 bytes | the field of
// field_bytes bytes | 1 byte; the other slots are inert.  The batches:
//   mode 0   nk random steps among the members and two keys that are no members; the expectation of a step is, by lot, the field as the steps before it left
//            it (so often a value that ONLY an earlier step of the batch wrote), the field as it stood before the batch (which an earlier step may have
//            overwritten: status 5), or random bytes.  Statuses 0, 1 and 5 occur.  The same steps then go through without expectations: 0 and 1 alone
//   mode 1   one key nk times with e_j = v_j-1, which only the batch satisfies; then the same with one more step that expects the value from BEFORE the batch,
//            which the table met then and the steps have since overwritten: status 5 at that step alone; then a no-op write v = e
//   mode 2   a chain as in mode 1 but for step pos, which expects a wrong value (even pos) or names a key that is no member (odd pos) -- for every pos in
//            turn: the first failure is at pos, `failed` is 1, and the step behind it is judged WITHOUT it, so it expects v_pos-1
// Every batch goes through keys_prepare over the nk keys at a stride, the located record and -- with expectations -- the field slot of every UNIQUE key as
// the device reports them (whole 16-byte units, zero behind the field, zero for a key that is no member), and write_plan; every array is a heap allocation of
// exactly its bytes (values and expectations at strides of F + 3 and F + 1, their last one F bytes), and without expectations the field array is null.  Checked
// against
//   the model    one step at a time on the table's BYTES: a linear scan for the live record whose lo is the key, the field compared and written byte by byte
//                -- idx and status of every step, the first failed step, the count of failed steps, the fields left
//   the splice   at depth 1 + seed % 24: two rows at in_stride = row bytes + 3 out of heap arrays of exactly the bytes the splice may read, with and without
//                the expected piece, uncut (splice_row with the staged tail) and cut at c_0 = 1 + seed % depth (splice_row, then splice_cut_tail), the rest
//                of the output untouched
// Prints "ok <field_bytes> <members> <nk> <mode> <batches checked> <steps checked> <steps with a status> <row bytes with expectations>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "merkle_keys.hpp"
#include "merkle_rows.hpp"
#include "merkle_write.hpp"

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

constexpr uint32_t K = 5, LO = 2 * K + 2;
typedef std::vector<uint8_t> Bytes;
struct Step {
  Bytes key, value, expect;
};

static unsigned g_f, g_mem, g_nk, g_mode;
#define CHECK(cond, what)                                                                                                \
  do {                                                                                                                   \
    if (!(cond)) {                                                                                                       \
      fprintf(stderr, "merkle_write_host_check: field_bytes %u members %u nk %u mode %u: %s\n", g_f, g_mem, g_nk, g_mode, what); \
      return 1;                                                                                                          \
    }                                                                                                                    \
  } while (0)

struct Table {
  uint32_t F;
  std::vector<Bytes> rec;
  bool live(size_t i) const { return memcmp(rec[i].data(), rec[i].data() + K, K) < 0; }
  uint32_t own(const Bytes &key) const {
    for (size_t i = 0; i < rec.size(); i++)
      if (live(i) && !memcmp(rec[i].data(), key.data(), K)) return (uint32_t)i;
    return mf::kNoRecord;
  }
  Bytes field(uint32_t i) const { return Bytes(rec[i].begin() + LO, rec[i].begin() + LO + F); }
};

static unsigned g_steps, g_failed;

static Bytes random_bytes(uint32_t n) {
  Bytes b(n);
  for (auto &x : b) x = rnd();
  return b;
}

// one batch against the model; conditional: the steps' expectations go to write_plan.  want_first: where the caller put the first failure, or -1
static int check_batch(const Table &start, const std::vector<Step> &batch, bool conditional, long want_first, long want_failed) {
  const uint32_t nk = (uint32_t)batch.size(), F = start.F, stride = K + 2;
  const size_t vstride = F + 3, estride = F + 1, pitch = mf::field_slot_bytes(F);
  CHECK(pitch >= F && pitch % 16 == 0 && pitch < F + 16, "the slot's bytes");
  uint8_t *keys = exact<uint8_t>(nk ? (size_t)(nk - 1) * stride + K : 0);
  uint8_t *value = exact<uint8_t>(nk ? (size_t)(nk - 1) * vstride + F : 0);
  uint8_t *expect = conditional ? exact<uint8_t>(nk ? (size_t)(nk - 1) * estride + F : 0) : nullptr;
  for (uint32_t j = 0; j < nk; j++) {
    memcpy(keys + (size_t)j * stride, batch[j].key.data(), K);
    memcpy(value + (size_t)j * vstride, batch[j].value.data(), F);
    if (conditional) memcpy(expect + (size_t)j * estride, batch[j].expect.data(), F);
  }
  mf::KeyPlan plan_keys;
  mf::keys_prepare(keys, stride, K, nk, plan_keys);
  free(keys);
  const uint32_t nu = plan_keys.nu;
  uint32_t *rec = exact<uint32_t>(nu), *slot = exact<uint32_t>(nk);
  uint8_t *field = conditional ? exact<uint8_t>((size_t)nu * pitch) : nullptr;
  for (uint32_t j = 0; j < nk; j++) {  // what the search and k_field_gather report per unique key
    const uint32_t u = plan_keys.slot[j];
    CHECK(u < nu, "a slot past the unique keys");
    slot[j] = u;
    rec[u] = start.own(batch[j].key);
    if (conditional) {
      memset(field + (size_t)u * pitch, 0, pitch);
      if (rec[u] != mf::kNoRecord) memcpy(field + (size_t)u * pitch, start.rec[rec[u]].data() + LO, F);
    }
  }
  mf::WritePlan plan;
  mf::write_plan(nk, slot, rec, F, value, vstride, expect, estride, field, pitch, plan);
  CHECK(plan.idx.size() == nk && plan.status.size() == nk, "the plan's sizes");
  // the model: one step at a time on the bytes
  Table t = start;
  uint32_t first = nk, failed = 0;
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t i = t.own(batch[j].key);
    uint8_t st = 0;
    if (i == mf::kNoRecord) st = 1;
    else if (conditional)
      for (uint32_t b = 0; b < F; b++)
        if (t.rec[i][LO + b] != batch[j].expect[b]) st = 5;
    CHECK(plan.status[j] == st, "a step's status");
    CHECK(plan.idx[j] == i, "a step's record");
    g_steps++;
    if (st) {
      g_failed++;
      failed++;
      if (first == nk) first = j;
      continue;
    }
    for (uint32_t b = 0; b < F; b++) t.rec[i][LO + b] = batch[j].value[b];
  }
  CHECK(plan.first == first && plan.failed == failed, "the first failed step, the failed steps");
  CHECK(want_first < 0 || first == (uint32_t)want_first, "the batch's first failure is where it was put");
  CHECK(want_failed < 0 || failed == (uint32_t)want_failed, "the batch's failed steps are as many as were put");
  if (conditional)
    for (uint32_t j = 0; j < nk; j++) {  // the fields left: what the applied steps made of them; behind F the slot is as it was
      const uint8_t *f = field + (size_t)slot[j] * pitch;
      if (rec[slot[j]] != mf::kNoRecord) CHECK(!memcmp(f, t.rec[rec[slot[j]]].data() + LO, F), "a field left behind the batch");
      for (size_t b = F; b < pitch; b++) CHECK(f[b] == 0, "a byte of a slot behind the field was written");
    }
  for (size_t i = 0; i < t.rec.size(); i++)
    CHECK(!memcmp(t.rec[i].data(), start.rec[i].data(), LO) && t.rec[i].back() == start.rec[i].back(), "the model wrote outside the field");
  free(rec);
  free(slot);
  free(field);
  free(value);
  free(expect);
  return 0;
}

// two rows, with and without the expected piece, uncut and cut, out of exact-size arrays
static int check_splice(uint32_t F, uint32_t length, uint32_t depth, uint32_t c0, size_t *rowb_out) {
  const size_t tail = mf::row_tail_bytes(depth);
  uint8_t *staged = exact<uint8_t>(128 + tail), *key = exact<uint8_t>(K), *val = exact<uint8_t>(F), *exp = exact<uint8_t>(F), *head = exact<uint8_t>(length);
  for (size_t i = 0; i < 128 + tail; i++) staged[i] = rnd();
  for (uint32_t i = 0; i < K; i++) key[i] = rnd();
  for (uint32_t i = 0; i < F; i++) val[i] = rnd(), exp[i] = rnd();
  for (uint32_t i = 0; i < length; i++) head[i] = rnd();
  for (int conditional = 0; conditional < 2; conditional++) {
    const size_t pub = (size_t)K + (conditional ? 2 : 1) * (size_t)F, rowb = mf::row_bytes(64, pub + length, depth), stride = rowb + 3;
    if (conditional) *rowb_out = rowb;
    CHECK(rowb == 64 + pub + length + (size_t)32 * depth + (depth + 7) / 8, "the row's bytes");
    uint8_t *out = exact<uint8_t>(2 * stride);
    for (int cut = 0; cut < 2; cut++) {
      memset(out, 0xA5, 2 * stride);
      const uint32_t d0 = cut ? c0 : depth, index = (uint32_t)(rnd64() & ((1u << depth) - 1));
      const size_t rb = mf::row_bytes(64, pub + length, d0);
      for (int r = 0; r < 2; r++) {
        uint8_t *row = out + r * stride;
        const mf::RowPiece e{conditional ? exp : nullptr, conditional ? (size_t)F : 0};
        mf::splice_row(row, 64, {{key, K}, e, {val, F}, {head, length}}, cut ? nullptr : staged, 128, depth);
        if (cut) mf::splice_cut_tail(row + 64 + pub + length, staged, d0, index);
        for (size_t i = 0; i < 64; i++) CHECK(row[i] == 0, "the zero bytes");
        CHECK(!memcmp(row + 64, key, K), "the key");
        if (conditional) CHECK(!memcmp(row + 64 + K, exp, F), "the expected bytes");
        CHECK(!memcmp(row + 64 + pub - F, val, F) && !memcmp(row + 64 + pub, head, length), "the value and the old record");
        const uint8_t *t = row + 64 + pub + length;
        CHECK(!memcmp(t, staged + 128, (size_t)32 * d0), "the siblings");
        if (!cut) CHECK(!memcmp(t, staged + 128, tail), "the staged tail");
        else
          for (uint32_t b = 0; b < (d0 + 7) / 8; b++) CHECK(t[(size_t)32 * d0 + b] == (uint8_t)((index & (uint32_t)(((uint64_t)1 << d0) - 1)) >> (8 * b)), "the index bytes mod 2^c_0");
        for (size_t i = rb; i < stride; i++) CHECK(row[i] == 0xA5, "a byte behind the row was written");
      }
    }
    free(out);
  }
  free(staged);
  free(key);
  free(val);
  free(exp);
  free(head);
  return 0;
}

static int run(uint32_t F, uint32_t mem, uint32_t nk, uint32_t mode, uint64_t seed, unsigned *batches, size_t *rowb) {
  rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
  const uint32_t length = LO + F + 1;
  // a well-formed table: the members' keys sorted, record i = (k_i, k_i+1), the sentinel record and inert slots, shuffled
  std::vector<Bytes> keys;
  while (keys.size() < mem) {
    Bytes k = random_bytes(K);
    if (mf::key_is_sentinel(k.data(), K) || std::find(keys.begin(), keys.end(), k) != keys.end()) continue;
    keys.push_back(k);
  }
  std::vector<Bytes> sorted = keys;
  std::sort(sorted.begin(), sorted.end());
  Table t{F, {}};
  const size_t slots = 2 * mem + 3;
  for (size_t i = 0; i <= mem; i++) {
    Bytes r = random_bytes(length);
    memset(r.data(), 0, 2 * K);
    if (i) memcpy(r.data(), sorted[i - 1].data(), K);
    if (i < mem) memcpy(r.data() + K, sorted[i].data(), K);
    else memset(r.data() + K, 0xFF, K);
    t.rec.push_back(r);
  }
  while (t.rec.size() < slots) {  // inert: lo >= hi, any payload.  Some carry a member's key as lo: the search must pass them by
    Bytes r = random_bytes(length);
    if (rnd() & 1) memcpy(r.data(), keys[rnd64() % mem].data(), K);
    memcpy(r.data() + K, r.data(), K);
    if (rnd() & 1) r[K] = 0, r[0] |= 1;
    t.rec.push_back(r);
  }
  for (size_t i = t.rec.size() - 1; i > 0; i--) std::swap(t.rec[i], t.rec[rnd64() % (i + 1)]);
  *batches = 0;
  if (mode == 0) {
    Bytes stranger_a(K, 0x11), stranger_b(K, 0xEE);
    while (t.own(stranger_a) != mf::kNoRecord) stranger_a[0]++;
    while (t.own(stranger_b) != mf::kNoRecord) stranger_b[0]--;
    std::vector<Step> batch;
    Table now = t;  // the table as the steps so far leave it, were all their expectations met
    for (uint32_t j = 0; j < nk; j++) {
      const unsigned pick = rnd();
      const Bytes &k = pick < 12 ? stranger_a : pick < 24 ? stranger_b : keys[rnd64() % mem];
      const uint32_t i = t.own(k);
      Bytes v = random_bytes(F), e;
      const unsigned lot = rnd() % 8;
      if (i == mf::kNoRecord || lot == 0) e = random_bytes(F);
      else if (lot == 1) e = t.field(i);  // as it stood before the batch
      else e = now.field(i);
      if (i != mf::kNoRecord && e == now.field(i)) memcpy(now.rec[i].data() + LO, v.data(), F);
      batch.push_back({k, v, e});
    }
    if (check_batch(t, batch, true, -1, -1)) return 1;
    if (check_batch(t, batch, false, -1, -1)) return 1;
    *batches += 2;
  } else if (mode == 1) {
    const Bytes &a = keys[0];
    std::vector<Step> chain;
    Bytes prev = t.field(t.own(a));
    for (uint32_t j = 0; j < nk; j++) {
      Bytes v = random_bytes(F);
      v[0] = (uint8_t)(prev[0] + 1);  // never the value it replaces
      chain.push_back({a, v, prev});
      prev = v;
    }
    if (check_batch(t, chain, true, nk, 0)) return 1;
    std::vector<Step> stale = chain;
    stale.push_back({a, random_bytes(F), t.field(t.own(a))});  // what the table held before the batch
    if (check_batch(t, stale, true, nk, 1)) return 1;
    if (check_batch(t, {{a, t.field(t.own(a)), t.field(t.own(a))}, {a, chain[0].value, t.field(t.own(a))}}, true, 2, 0)) return 1;  // a no-op, then a write
    *batches += 3;
  } else {
    Bytes stranger(K, 0x33);
    while (t.own(stranger) != mf::kNoRecord) stranger[0]++;
    for (uint32_t pos = 0; pos < nk; pos++) {
      const Bytes &a = keys[pos % mem];
      std::vector<Step> batch;
      Bytes prev = t.field(t.own(a));
      for (uint32_t j = 0; j < nk; j++) {
        Bytes v = random_bytes(F);
        v[0] = (uint8_t)(prev[0] + 1);
        if (j == pos) {
          Bytes wrong = prev;
          wrong[F - 1] ^= 0x80;
          batch.push_back(pos & 1 ? Step{stranger, v, prev} : Step{a, v, wrong});
          continue;  // not applied: the next step expects what this one found
        }
        batch.push_back({a, v, prev});
        prev = v;
      }
      if (check_batch(t, batch, true, pos, 1)) return 1;
      ++*batches;
    }
  }
  const uint32_t depth = 1 + (uint32_t)(seed % 24);
  return check_splice(F, length + (uint32_t)(seed % 7), depth, 1 + (uint32_t)(seed % depth), rowb);
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    unsigned F, mem, nk, mode;
    unsigned long long seed;
    if (sscanf(line, "%u %u %u %u %llu", &F, &mem, &nk, &mode, &seed) != 5) return 2;
    if (F < 1 || F > 256 || mem < 3 || mem > 64 || nk < 1 || nk > 4096 || mode > 2) return 2;
    if (mode != 0 && nk > 200) return 2;
    g_f = F, g_mem = mem, g_nk = nk, g_mode = mode;
    g_steps = g_failed = 0;
    unsigned batches = 0;
    size_t rowb = 0;
    if (run(F, mem, nk, mode, seed, &batches, &rowb)) return 1;
    printf("ok %u %u %u %u %u %u %u %zu\n", F, mem, nk, mode, batches, g_steps, g_failed, rowb);
  }
  return 0;
}
