// The host side of mfh_merkle_insert_keys (csrc/merkle_insert.hpp: predecessor, successor and the 2 nk update indices of a batch of sequential key inserts;
// csrc/merkle_rows.hpp: the key step's row size with three records, its splice and the chunk of whole steps) as a program of its own (tests/test_merkle_insert_host_cpu.py
// builds it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <key_bytes> <nk> <mode> <extra> <seed>
// A set of random non-sentinel keys is split into members and the batch -- mode 0, 1, 2: the batch is a run of neighbours in key order, so every key falls
// into ONE range, given in ascending, descending and shuffled order; 3: members and batch keys alternate in key order, one key per range, shuffled; 4: a
// random split, shuffled.  The members make a well-formed indexed table in shuffled positions with at least nk inert slots; the keys stand at a key_stride of
// key_bytes + extra in a heap allocation of exactly (nk - 1) * stride + key_bytes bytes.
// Checked against a brute-force sequential model that keeps the table as a list of (lo, hi) and inserts one key at a time -- the record whose range holds
// the key by a linear scan, the lowest inert slot of the list as it then stands:
//   the plan     idx[2 j] is the model's record, idx[2 j + 1] its slot; the records the plan describes (lo and hi by pred and succ, from the table BEFORE the
//                batch and the keys alone) are the model's two new records of insert j
//   the splice   (length = 2 key_bytes + extra) at depth 1 + seed % 24, 3 and 4 -- 2 depth is and is not a multiple of 8 -- two rows at in_stride = row bytes +
//                extra out of heap arrays of exactly the bytes the splice may read, the rest of the output untouched, the index bits set one by one
//   the chunk    pair_chunk is even, at least 2, at most 2 nk, and twice the inserts whose rows fit, whatever the stage
// Prints "ok <key_bytes> <nk> <mode> <distinct located records> <row bytes>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

#include "merkle_insert.hpp"
#include "merkle_keys.hpp"
#include "merkle_rows.hpp"

static uint64_t rng_state;
static uint8_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint8_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 56);
}
static uint32_t rnd32() { return (uint32_t)rnd() << 24 | (uint32_t)rnd() << 16 | (uint32_t)rnd() << 8 | rnd(); }

static uint8_t *exact(size_t bytes) {
  uint8_t *p = (uint8_t *)malloc(bytes ? bytes : 1);
  if (!p) exit(3);
  return p;
}

typedef std::vector<uint8_t> Key;
struct Rec {
  Key lo, hi;
  bool live() const { return lo < hi; }  // (vectors of one length compare as memcmp does)
};

#define CHECK(cond, what)                                                                              \
  do {                                                                                                 \
    if (!(cond)) {                                                                                     \
      fprintf(stderr, "merkle_insert_host_check: key_bytes %u nk %u mode %u: %s\n", kb, nk, mode, what); \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

template <class T>
static void shuffle(std::vector<T> &v) {
  for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd32() % i]);
}

int main() {
  char buf[256];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned kb = 0, nk = 0, mode = 0, extra = 0;
    unsigned long long seed = 0;
    if (sscanf(buf, "%u %u %u %u %llu", &kb, &nk, &mode, &extra, &seed) != 5 || kb < 1 || kb > 32 || nk > 4096 || mode > 4 || extra > 64 ||
        (kb == 1 && 2 * nk + 3 > 254)) {
      fprintf(stderr, "merkle_insert_host_check: expected <key_bytes in 1 .. 32> <nk <= 4096; 2 nk + 3 <= 254 at key_bytes 1> <mode <= 4> <extra <= 64> <seed>\n");
      return 2;
    }
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const size_t stride = kb + extra;
    // 2 nk + 3 distinct non-sentinel keys, sorted; the split into members and batch
    std::set<Key> drawn;
    while (drawn.size() < 2 * (size_t)nk + 3) {
      Key k(kb);
      for (unsigned b = 0; b < kb; b++) k[b] = rnd();
      if (!mf::key_is_sentinel(k.data(), kb)) drawn.insert(k);
    }
    std::vector<Key> all(drawn.begin(), drawn.end()), members, batch;
    if (mode <= 2) {
      const size_t at = rnd32() % (all.size() - nk + 1);
      for (size_t i = 0; i < all.size(); i++) (i >= at && i < at + nk ? batch : members).push_back(all[i]);
      if (mode == 1) std::reverse(batch.begin(), batch.end());
    } else if (mode == 3) {
      for (size_t i = 0; i < all.size(); i++) (i % 2 && batch.size() < nk ? batch : members).push_back(all[i]);
    } else {
      shuffle(all);
      batch.assign(all.begin(), all.begin() + nk);
      members.assign(all.begin() + nk, all.end());
      std::sort(members.begin(), members.end());
    }
    if (mode >= 2) shuffle(batch);
    CHECK(batch.size() == nk, "the batch's size");
    // the table: the sentinel record and one record per member, in shuffled positions of 2^depth slots with at least nk + 2 inert ones
    size_t slots_n = 2;
    while (slots_n < members.size() + 1 + nk + 2) slots_n *= 2;
    std::vector<uint32_t> pos(slots_n);
    for (size_t i = 0; i < slots_n; i++) pos[i] = (uint32_t)i;
    shuffle(pos);
    const Key zero(kb, 0x00), ones(kb, 0xFF);
    std::vector<Rec> table(slots_n, Rec{zero, zero});
    for (size_t r = 0; r <= members.size(); r++) table[pos[r]] = Rec{r ? members[r - 1] : zero, r < members.size() ? members[r] : ones};
    for (size_t r = members.size() + 1; r < slots_n; r++)
      if (rnd() & 1) table[pos[r]] = Rec{ones, r & 1 ? ones : zero};  // inert slots that are not all zero: lo == hi and lo > hi
    const std::vector<Rec> before = table;
    // what the device hands the plan: the located record of every key against the table BEFORE the batch, and the lowest nk inert slots, ascending
    const size_t keys_bytes = nk ? (size_t)(nk - 1) * stride + kb : 0;
    uint8_t *keys = exact(keys_bytes);
    memset(keys, 0xA5, keys_bytes);
    std::vector<uint32_t> located(nk), slot(nk);
    for (unsigned j = 0; j < nk; j++) {
      memcpy(keys + j * stride, batch[j].data(), kb);
      unsigned found = 0;
      for (size_t i = 0; i < slots_n; i++)
        if (before[i].lo < batch[j] && batch[j] < before[i].hi) { located[j] = (uint32_t)i; found++; }
      CHECK(found == 1, "the table is not well formed");
    }
    {
      unsigned j = 0;
      for (size_t i = 0; i < slots_n && j < nk; i++)
        if (!before[i].live()) slot[j++] = (uint32_t)i;
      CHECK(j == nk, "too few inert slots");
    }
    mf::InsertPlan plan;
    mf::insert_plan(keys, stride, kb, nk, located.data(), slot.data(), plan);
    CHECK(plan.pred.size() == nk && plan.succ.size() == nk && plan.idx.size() == 2 * (size_t)nk, "the plan's sizes");
    // the model, one key at a time
    for (unsigned j = 0; j < nk; j++) {
      size_t P = slots_n, S = slots_n;
      for (size_t i = 0; i < slots_n; i++)
        if (table[i].lo < batch[j] && batch[j] < table[i].hi) { CHECK(P == slots_n, "two ranges hold a key"); P = i; }
      for (size_t i = 0; i < slots_n && S == slots_n; i++)
        if (!table[i].live()) S = i;
      CHECK(P < slots_n && S < slots_n, "the model cannot insert");
      const Key old_hi = table[P].hi;
      table[P].hi = batch[j];
      table[S] = Rec{batch[j], old_hi};
      CHECK(plan.idx[2 * (size_t)j] == P && plan.idx[2 * (size_t)j + 1] == S && S == slot[j], "the update indices differ");
      const int32_t pred = plan.pred[j], succ = plan.succ[j];
      CHECK(pred < (int32_t)j && succ < (int32_t)j && pred >= -1 && succ >= -1, "pred or succ is no earlier insert");
      CHECK(pred < 0 || located[pred] == located[j], "pred is of another range");
      CHECK(succ < 0 || located[succ] == located[j], "succ is of another range");
      const Key &lo = pred < 0 ? before[located[j]].lo : batch[pred], &hi = succ < 0 ? before[located[j]].hi : batch[succ];
      CHECK(lo == table[P].lo && hi == old_hi, "the records the plan describes are not the model's");
      CHECK(pred < 0 ? P == located[j] : P == slot[pred], "the predecessor's slot");
    }
    const unsigned groups = (unsigned)std::set<uint32_t>(located.begin(), located.end()).size();
    if (mode <= 2) CHECK(groups == (nk ? 1u : 0u), "mode 0 .. 2 is one range");
    if (mode == 3) CHECK(groups == nk, "mode 3 is one key per range");
    // the splice
    const uint32_t length = 2 * kb + extra;
    const size_t hp = mf::record_head_pitch(length);
    size_t rowb_seed = 0;
    for (uint32_t depth : {1 + (uint32_t)(seed % 24), 3u, 4u}) {
      const size_t idxb = (2 * depth + 7) / 8, rowb = mf::pair_row_bytes(kb, 3, length, depth), in_stride = rowb + extra;
      if (!rowb_seed) rowb_seed = rowb;
      CHECK(rowb == 64 + (size_t)kb + 3 * (size_t)length + 64 * (size_t)depth + idxb && hp % 16 == 0 && hp >= length && hp < (size_t)length + 16, "the sizes differ");
      const unsigned nr = nk < 2 ? nk : 2;
      if (!nr) continue;
      const size_t out_bytes = (size_t)(nr - 1) * in_stride + rowb, staged_bytes = 128 + (size_t)32 * depth;
      uint8_t *head_p = exact(length), *head_s = exact(hp + length), *staged_p = exact(staged_bytes), *staged_s = exact(staged_bytes), *out = exact(out_bytes), *want = exact(out_bytes);
      for (size_t i = 0; i < length; i++) head_p[i] = rnd();
      for (size_t i = 0; i < hp + length; i++) head_s[i] = rnd();
      for (size_t i = 0; i < staged_bytes; i++) { staged_p[i] = rnd(); staged_s[i] = rnd(); }
      memset(out, 0xA5, out_bytes);
      memset(want, 0xA5, out_bytes);
      for (unsigned k = 0; k < nr; k++) {
        const uint32_t p = rnd32() & ((1u << depth) - 1), s = k ? (1u << depth) - 1 : rnd32() & ((1u << depth) - 1);
        uint8_t *w = want + k * in_stride;
        size_t at = 0;
        for (unsigned i = 0; i < 64; i++) w[at++] = 0;
        for (unsigned i = 0; i < kb; i++) w[at++] = keys[k * stride + i];
        for (unsigned i = 0; i < length; i++) w[at++] = head_p[i];
        for (unsigned i = 0; i < length; i++) w[at++] = head_s[i];
        for (unsigned i = 0; i < length; i++) w[at++] = head_s[hp + i];
        for (size_t i = 0; i < (size_t)32 * depth; i++) w[at++] = staged_p[128 + i];
        for (size_t i = 0; i < (size_t)32 * depth; i++) w[at++] = staged_s[128 + i];
        for (size_t i = 0; i < idxb; i++) w[at + i] = 0;
        for (uint32_t l = 0; l < depth; l++) {
          if ((p >> l) & 1) w[at + l / 8] |= (uint8_t)(1u << (l % 8));
          if ((s >> l) & 1) w[at + (depth + l) / 8] |= (uint8_t)(1u << ((depth + l) % 8));
        }
        CHECK(at + idxb == rowb, "the row's size");
        mf::splice_pair_row(out + k * in_stride, 64, {{keys + k * stride, kb}, {head_p, length}, {head_s, length}, {head_s + hp, length}}, staged_p, staged_s, depth, p, s);
      }
      const bool same = !memcmp(out, want, out_bytes);
      free(head_p); free(head_s); free(staged_p); free(staged_s); free(out); free(want);
      CHECK(same, "the rows differ");
    }
    // the chunk of whole inserts
    if (nk) {
      for (size_t stage : {(size_t)1, rowb_seed - 1, rowb_seed, 2 * rowb_seed + 1, (size_t)nk * rowb_seed - 1, (size_t)nk * rowb_seed, (size_t)64 << 20}) {
        const uint32_t ch = mf::pair_chunk(nk, rowb_seed, stage);
        const size_t fit = stage / rowb_seed, want = fit < 1 ? 1 : fit < nk ? fit : nk;
        CHECK(ch % 2 == 0 && ch >= 2 && ch <= 2 * nk && ch == 2 * want, "the chunk is not whole inserts");
      }
    }
    free(keys);
    printf("ok %u %u %u %u %zu\n", kb, nk, mode, groups, rowb_seed);
  }
  return 0;
}
