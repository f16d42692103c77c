// The host side of mfh_merkle_remove_keys (csrc/merkle_remove.hpp: the slot whose hi changes, the hi it receives and the 2 nk update indices of a batch of
// sequential key removes; csrc/merkle_rows.hpp: the key step's row size with two records and its splice) as a program of its own (tests/test_merkle_remove_host_cpu.py builds
// it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <key_bytes> <nk> <mode> <extra> <seed>
// A set of random non-sentinel keys makes a well-formed indexed table in shuffled positions, its inert slots all zero, lo == hi or lo > hi.  The batches:
//   mode 0   nk = 1 .. 6: a run of nk ADJACENT members, removed in EVERY one of its nk! orders, for the run at the smallest members (the first remove's P is the
//            sentinel record), at the largest (the inherited hi is FF..FF) and in between
//   mode 1   nk random members out of 2 nk + 3, shuffled
//   mode 2   every one of the nk members, shuffled: down to the empty set
//   mode 3   of 2 nk + 3 members each is in the batch with probability 3/4, shuffled: many runs of several lengths, removed interleaved
// The keys stand at a key_stride of key_bytes + extra in a heap allocation of exactly (n - 1) * stride + key_bytes bytes.  Every batch is checked against
//   the walk     the quadratic rule as merkle_remove.hpp states it, rank by rank: idx, hi_key and hi_rec are equal
//   the model    a sequential model that keeps the table as a list of (lo, hi) and removes one key at a time -- the lowest live record with lo = key, the
//                lowest live record with hi = key, by linear scans of the table as it then stands: idx[2 j] and idx[2 j + 1] are the model's records, and
//                the hi the plan describes (a key of the batch, or a hi of the table BEFORE the batch) is the one the model hands on; at the end the
//                model's table is the well-formed table of the members that are left
//   the splice   (length = 2 key_bytes + extra) at depth 1 + seed % 24, 3 and 4 -- 2 depth is and is not a multiple of 8 -- and zeros = 64 and 128: two rows at
//                in_stride = row bytes + extra out of heap arrays of exactly the bytes the splice may read, the rest of the output untouched
// Prints "ok <key_bytes> <nk> <mode> <batches checked> <removes checked> <row bytes>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

#include "merkle_keys.hpp"
#include "merkle_remove.hpp"
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

static unsigned g_kb, g_nk, g_mode;
#define CHECK(cond, what)                                                                                    \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      fprintf(stderr, "merkle_remove_host_check: key_bytes %u nk %u mode %u: %s\n", g_kb, g_nk, g_mode, what); \
      return 1;                                                                                              \
    }                                                                                                        \
  } while (0)

template <class T>
static void shuffle(std::vector<T> &v) {
  for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd32() % i]);
}

// one batch against the walk and the model; `members` sorted, `before` their table
static int check_batch(const std::vector<Key> &members, const std::vector<Rec> &before, const std::vector<Key> &batch, size_t stride) {
  const unsigned kb = g_kb;
  const uint32_t n = (uint32_t)batch.size();
  const size_t slots_n = before.size();
  const size_t keys_bytes = n ? (size_t)(n - 1) * stride + kb : 0;
  uint8_t *keys = exact(keys_bytes);
  memset(keys, 0xA5, keys_bytes);
  // what the device hands the plan: own and prev of every key against the table BEFORE the batch
  std::vector<uint32_t> own(n, mf::kNoRecord), prev(n, mf::kNoRecord);
  for (uint32_t j = 0; j < n; j++) {
    memcpy(keys + j * stride, batch[j].data(), kb);
    for (size_t i = slots_n; i-- > 0;) {
      if (before[i].live() && before[i].lo == batch[j]) own[j] = (uint32_t)i;
      if (before[i].live() && before[i].hi == batch[j]) prev[j] = (uint32_t)i;
    }
    CHECK(own[j] != mf::kNoRecord && prev[j] != mf::kNoRecord, "a key of the batch is no member");
  }
  mf::RemovePlan plan;
  mf::remove_plan(keys, stride, kb, n, own.data(), prev.data(), plan);
  free(keys);
  CHECK(plan.hi_key.size() == n && plan.hi_rec.size() == n && plan.idx.size() == 2 * (size_t)n, "the plan's sizes");
  // the quadratic walk
  std::vector<uint32_t> order(n), rank(n);
  for (uint32_t j = 0; j < n; j++) order[j] = j;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return batch[a] < batch[b]; });
  for (uint32_t r = 0; r < n; r++) rank[order[r]] = r;
  auto linked = [&](uint32_t r) { return prev[order[r + 1]] == own[order[r]]; };
  for (uint32_t j = 0; j < n; j++) {
    uint32_t l = rank[j], h = rank[j];
    while (l > 0 && linked(l - 1) && order[l - 1] < j) l--;
    while (h + 1 < n && linked(h) && order[h + 1] < j) h++;
    const uint32_t P = l > 0 && linked(l - 1) ? own[order[l - 1]] : prev[order[l]];
    CHECK(plan.idx[2 * (size_t)j] == P && plan.idx[2 * (size_t)j + 1] == own[j], "the update indices are not the walk's");
    if (h + 1 < n && linked(h)) {
      CHECK(plan.hi_key[j] == (int32_t)order[h + 1], "the inherited hi is not the walk's key");
    } else {
      CHECK(plan.hi_key[j] == -1 && plan.hi_rec[j] == own[order[h]], "the inherited hi is not the walk's record");
    }
  }
  // the model, one key at a time
  std::vector<Rec> table = before;
  const Key zero(kb, 0x00), ones(kb, 0xFF);
  for (uint32_t j = 0; j < n; j++) {
    size_t P = slots_n, S = slots_n;
    for (size_t i = slots_n; i-- > 0;) {
      if (table[i].live() && table[i].lo == batch[j]) S = i;
      if (table[i].live() && table[i].hi == batch[j]) P = i;
    }
    CHECK(P < slots_n && S < slots_n && P != S, "the model cannot remove");
    CHECK(plan.idx[2 * (size_t)j] == P && plan.idx[2 * (size_t)j + 1] == S, "the update indices are not the model's");
    CHECK(plan.hi_key[j] >= -1 && plan.hi_key[j] < (int32_t)n && (plan.hi_key[j] >= 0 || plan.hi_rec[j] < slots_n), "the plan's sources are out of range");
    const Key &hi = plan.hi_key[j] >= 0 ? batch[plan.hi_key[j]] : before[plan.hi_rec[j]].hi;
    CHECK(hi == table[S].hi, "the hi the plan describes is not the model's");
    CHECK(before[P].lo == table[P].lo && before[P].live(), "record P is not a record of the table before the batch");
    table[P].hi = table[S].hi;
    table[S] = Rec{zero, zero};
  }
  // what is left: the well-formed table of the remaining members, every other slot as it was or zero
  std::set<Key> gone(batch.begin(), batch.end());
  std::vector<Key> left;
  for (const Key &k : members)
    if (!gone.count(k)) left.push_back(k);
  std::vector<Rec> live;
  for (const Rec &r : table)
    if (r.live()) live.push_back(r);
  std::sort(live.begin(), live.end(), [](const Rec &a, const Rec &b) { return a.lo < b.lo; });
  CHECK(live.size() == left.size() + 1, "the number of live records");
  for (size_t r = 0; r < live.size(); r++)
    CHECK(live[r].lo == (r ? left[r - 1] : zero) && live[r].hi == (r < left.size() ? left[r] : ones), "the table left behind is not well formed");
  return 0;
}

int main() {
  char buf[256];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned kb = 0, nk = 0, mode = 0, extra = 0;
    unsigned long long seed = 0;
    if (sscanf(buf, "%u %u %u %u %llu", &kb, &nk, &mode, &extra, &seed) != 5 || kb < 1 || kb > 32 || nk > 4096 || mode > 3 || extra > 64 ||
        (kb == 1 && 2 * nk + 3 > 254) || (mode == 0 && (nk < 1 || nk > 6))) {
      fprintf(stderr, "merkle_remove_host_check: expected <key_bytes in 1 .. 32> <nk <= 4096; 2 nk + 3 <= 254 at key_bytes 1; 1 .. 6 in mode 0> <mode <= 3> <extra <= 64> <seed>\n");
      return 2;
    }
    g_kb = kb, g_nk = nk, g_mode = mode;
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const size_t stride = kb + extra;
    const size_t nmem = mode == 2 ? nk : 2 * (size_t)nk + 3;
    std::set<Key> drawn;
    while (drawn.size() < nmem) {
      Key k(kb);
      for (unsigned b = 0; b < kb; b++) k[b] = rnd();
      if (!mf::key_is_sentinel(k.data(), kb)) drawn.insert(k);
    }
    const std::vector<Key> members(drawn.begin(), drawn.end());
    // the table: the sentinel record and one record per member, in shuffled positions of 2^depth slots
    size_t slots_n = 2;
    while (slots_n < members.size() + 3) slots_n *= 2;
    std::vector<uint32_t> pos(slots_n);
    for (size_t i = 0; i < slots_n; i++) pos[i] = (uint32_t)i;
    shuffle(pos);
    const Key zero(kb, 0x00), ones(kb, 0xFF);
    std::vector<Rec> table(slots_n, Rec{zero, zero});
    for (size_t r = 0; r <= members.size(); r++) table[pos[r]] = Rec{r ? members[r - 1] : zero, r < members.size() ? members[r] : ones};
    for (size_t r = members.size() + 1; r < slots_n; r++)
      if (rnd() & 1) table[pos[r]] = Rec{ones, r & 1 ? ones : zero};  // inert slots that are not all zero: lo == hi and lo > hi
    unsigned batches = 0, removes = 0;
    if (mode == 0) {
      for (size_t at : {(size_t)0, members.size() - nk, (size_t)(1 + rnd32() % (members.size() - nk - 1))}) {
        std::vector<uint32_t> perm(nk);
        for (unsigned i = 0; i < nk; i++) perm[i] = i;
        do {
          std::vector<Key> batch;
          for (unsigned i = 0; i < nk; i++) batch.push_back(members[at + perm[i]]);
          if (int rc = check_batch(members, table, batch, stride)) return rc;
          batches++, removes += nk;
        } while (std::next_permutation(perm.begin(), perm.end()));
      }
    } else {
      std::vector<Key> batch;
      if (mode == 1) {
        batch = members;
        shuffle(batch);
        batch.resize(nk);
      } else if (mode == 2) {
        batch = members;
      } else {
        for (const Key &k : members)
          if (rnd() & 3) batch.push_back(k);
      }
      shuffle(batch);
      if (int rc = check_batch(members, table, batch, stride)) return rc;
      batches++, removes += (unsigned)batch.size();
    }
    // the splice
    const uint32_t length = 2 * kb + extra;
    size_t rowb_seed = 0;
    Key key(kb);
    for (unsigned b = 0; b < kb; b++) key[b] = rnd();
    for (uint32_t depth : {1 + (uint32_t)(seed % 24), 3u, 4u})
      for (size_t zeros : {(size_t)64, (size_t)128}) {
        const size_t idxb = (2 * depth + 7) / 8, rowb = mf::pair_row_bytes(kb, 2, length, depth, zeros), in_stride = rowb + extra;
        if (!rowb_seed) rowb_seed = rowb;
        CHECK(rowb == zeros + (size_t)kb + 2 * (size_t)length + 64 * (size_t)depth + idxb && mf::pair_row_bytes(kb, 2, length, depth) == rowb - zeros + 64, "the sizes differ");
        const unsigned nr = 2;
        const size_t out_bytes = (size_t)(nr - 1) * in_stride + rowb, staged_bytes = 128 + (size_t)32 * depth;
        uint8_t *head_p = exact(length), *head_s = exact(length), *staged_p = exact(staged_bytes), *staged_s = exact(staged_bytes), *out = exact(out_bytes), *want = exact(out_bytes);
        uint8_t *k_exact = exact(kb);
        memcpy(k_exact, key.data(), kb);
        for (size_t i = 0; i < length; i++) { head_p[i] = rnd(); head_s[i] = rnd(); }
        for (size_t i = 0; i < staged_bytes; i++) { staged_p[i] = rnd(); staged_s[i] = rnd(); }
        memset(out, 0xA5, out_bytes);
        memset(want, 0xA5, out_bytes);
        for (unsigned k = 0; k < nr; k++) {
          const uint32_t p = rnd32() & ((1u << depth) - 1), s = k ? (1u << depth) - 1 : rnd32() & ((1u << depth) - 1);
          uint8_t *w = want + k * in_stride;
          size_t at = 0;
          for (size_t i = 0; i < zeros; i++) w[at++] = 0;
          for (unsigned i = 0; i < kb; i++) w[at++] = key[i];
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
          mf::splice_pair_row(out + k * in_stride, zeros, {{k_exact, kb}, {head_p, length}, {head_s, length}}, staged_p, staged_s, depth, p, s);
        }
        const bool same = !memcmp(out, want, out_bytes);
        free(head_p); free(head_s); free(staged_p); free(staged_s); free(out); free(want); free(k_exact);
        CHECK(same, "the rows differ");
      }
    printf("ok %u %u %u %u %u %zu\n", kb, nk, mode, batches, removes, rowb_seed);
  }
  return 0;
}
