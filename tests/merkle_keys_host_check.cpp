// The host side of mfh_merkle_absent_rows (csrc/merkle_keys.hpp: the queries sorted, de-duplicated, turned into words, the results scattered back through
// the permutation; csrc/merkle_rows.hpp: the row's size and splice) as a program of its own (tests/test_merkle_keys_host_cpu.py builds it with the
// address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <key_bytes> <nq> <pool> <extra> <seed>
// nq queries are drawn from a pool of `pool` random non-sentinel keys (pool < nq forces duplicates; the pool's keys share their first key_bytes - 1 bytes in
// half of the cases, so the last byte decides), at a key_stride of key_bytes + extra, in a heap allocation of exactly (nq - 1) * stride + key_bytes bytes.
// Checked against a brute-force model that uses memcmp alone:
//   the plan     order is a permutation, sorted by memcmp, equal keys in ascending query number; the unique keys ascend strictly; slot[k] names query k's
//                key among them; the words are the big-endian words of the key, a last partial word left-aligned and zero-padded, and their
//                lexicographic order is the keys' memcmp order
//   the scatter  from made-up result words (range, present) per unique key: status 1 and the present record where there is one, else 0 and the range
//                record, else 2 and 0xFFFFFFFF -- for every query, duplicates alike
//   the splice   (length = 2 key_bytes + extra, depth = 1 + seed % 24) rows of in_stride = row bytes + extra out of staged pieces of exactly their sizes: a
//                found row in full, a not-found row's 32 + key_bytes bytes, the rest of the allocation untouched
// Prints "ok <key_bytes> <nq> <unique> <key words> <row bytes>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "merkle_keys.hpp"
#include "merkle_rows.hpp"

static uint64_t rng_state;
static uint8_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint8_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 56);
}

static uint8_t *exact(size_t bytes) {
  uint8_t *p = (uint8_t *)malloc(bytes ? bytes : 1);
  if (!p) exit(3);
  return p;
}

#define CHECK(cond, what)                                                                          \
  do {                                                                                             \
    if (!(cond)) {                                                                                 \
      fprintf(stderr, "merkle_keys_host_check: key_bytes %u nq %u: %s\n", kb, nq, what);           \
      return 1;                                                                                    \
    }                                                                                              \
  } while (0)

int main() {
  char buf[256];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned kb = 0, nq = 0, pool = 0, extra = 0;
    unsigned long long seed = 0;
    if (sscanf(buf, "%u %u %u %u %llu", &kb, &nq, &pool, &extra, &seed) != 5 || kb < 1 || kb > 32 || nq > 4096 || pool < 1 || pool > 4096 || extra > 64) {
      fprintf(stderr, "merkle_keys_host_check: expected <key_bytes in 1 .. 32> <nq <= 4096> <pool in 1 .. 4096> <extra <= 64> <seed>\n");
      return 2;
    }
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const size_t stride = kb + extra;
    const uint32_t kw = mf::key_words(kb);
    CHECK(kw == (kb + 3) / 4 && mf::kMaxKeyBytes == 32, "the word count differs");
    // the pool: non-sentinel keys, in half of the cases equal but for the last byte
    std::vector<uint8_t> pk((size_t)pool * kb);
    const bool last_only = seed & 1;
    for (unsigned i = 0; i < pool; i++) {
      uint8_t *key = pk.data() + (size_t)i * kb;
      do {
        for (unsigned b = 0; b < kb; b++) key[b] = last_only && b + 1 < kb ? (i ? pk[b] : rnd()) : rnd();
      } while (mf::key_is_sentinel(key, kb));
    }
    const size_t keys_bytes = nq ? (size_t)(nq - 1) * stride + kb : 0;
    uint8_t *keys = exact(keys_bytes);
    memset(keys, 0xA5, keys_bytes);
    for (unsigned k = 0; k < nq; k++) memcpy(keys + k * stride, pk.data() + (size_t)(((unsigned)rnd() << 8 | rnd()) % pool) * kb, kb);

    mf::KeyPlan plan;
    mf::keys_prepare(keys, stride, kb, nq, plan);
    // the plan against memcmp
    CHECK(plan.order.size() == nq && plan.slot.size() == nq && plan.words.size() == (size_t)plan.nu * kw && plan.nu <= nq && (plan.nu > 0) == (nq > 0), "the plan's sizes");
    std::vector<uint8_t> seen(nq, 0);
    for (unsigned j = 0; j < nq; j++) {
      CHECK(plan.order[j] < nq && !seen[plan.order[j]], "order is no permutation");
      seen[plan.order[j]] = 1;
      if (j) {
        const int cmp = memcmp(keys + plan.order[j - 1] * stride, keys + plan.order[j] * stride, kb);
        CHECK(cmp < 0 || (cmp == 0 && plan.order[j - 1] < plan.order[j]), "order is not sorted, or not stable");
      }
    }
    unsigned distinct = 0;
    for (unsigned j = 0; j < nq; j++)
      if (!j || memcmp(keys + plan.order[j - 1] * stride, keys + plan.order[j] * stride, kb)) distinct++;
    CHECK(distinct == plan.nu, "the number of unique keys");
    std::vector<const uint8_t *> ukey(plan.nu, nullptr);
    for (unsigned k = 0; k < nq; k++) {
      CHECK(plan.slot[k] < plan.nu, "a slot is out of range");
      const uint8_t *key = keys + k * stride;
      if (!ukey[plan.slot[k]]) ukey[plan.slot[k]] = key;
      CHECK(!memcmp(ukey[plan.slot[k]], key, kb), "two different keys share a slot");
    }
    for (unsigned u = 0; u < plan.nu; u++) {
      CHECK(ukey[u], "a slot without a query");
      const uint32_t *w = plan.words.data() + (size_t)u * kw;
      for (unsigned b = 0; b < 4 * kw; b++)  // byte b of the key stands in bits [24 - 8 (b % 4), 32 - 8 (b % 4)) of word b / 4; the padding is zero
        CHECK(((w[b / 4] >> (24 - 8 * (b % 4))) & 0xFF) == (b < kb ? ukey[u][b] : 0u), "the words differ");
      if (u) {
        CHECK(memcmp(ukey[u - 1], ukey[u], kb) < 0, "the unique keys do not ascend");
        const uint32_t *v = w - kw;
        unsigned j = 0;
        while (j < kw && v[j] == w[j]) j++;
        CHECK(j < kw && v[j] < w[j], "the words' order is not the keys'");
      }
    }
    // the scatter
    std::vector<uint32_t> res((size_t)2 * plan.nu), index(nq, 0x5A5A5A5A);
    std::vector<uint8_t> status(nq, 0x5A);
    for (unsigned u = 0; u < plan.nu; u++) {
      const unsigned kind = rnd() % 4;
      res[u] = kind & 1 ? 1000 + u : mf::kNoRecord;
      res[plan.nu + u] = kind & 2 ? 5000 + u : mf::kNoRecord;
    }
    mf::keys_scatter(plan, nq, res.data(), index.data(), status.data());
    for (unsigned k = 0; k < nq; k++) {
      const unsigned u = plan.slot[k];
      const uint32_t range = res[u], present = res[plan.nu + u];
      const uint32_t want_i = present != mf::kNoRecord ? present : range;
      const uint8_t want_s = present != mf::kNoRecord ? 1 : range != mf::kNoRecord ? 0 : 2;
      CHECK(index[k] == want_i && status[k] == want_s && (want_s != 2 || want_i == 0xFFFFFFFFu), "the scatter differs");
    }
    // the splice
    const uint32_t length = 2 * kb + extra, depth = 1 + (uint32_t)(seed % 24);
    const size_t idxb = (depth + 7) / 8, rowb = mf::row_bytes(32, (size_t)kb + length, depth), prb = mf::row_bytes(32, 32, depth), in_stride = rowb + extra;
    CHECK(rowb == 32 + (size_t)kb + length + 32 * (size_t)depth + idxb && prb == 64 + 32 * (size_t)depth + idxb, "the sizes differ");
    const unsigned nr = nq < 3 ? nq : 3;
    if (nr) {
      const size_t out_bytes = (size_t)(nr - 1) * in_stride + rowb;
      uint8_t *head = exact(length), *path = exact(prb), *out = exact(out_bytes), *want = exact(out_bytes);
      for (size_t i = 0; i < length; i++) head[i] = rnd();
      for (size_t i = 0; i < prb; i++) path[i] = rnd();
      memset(out, 0xA5, out_bytes);
      memset(want, 0xA5, out_bytes);
      for (unsigned k = 0; k < nr; k++) {
        const bool found = k != 1;
        uint8_t *w = want + k * in_stride;
        size_t at = 0;
        for (unsigned i = 0; i < 32; i++) w[at++] = 0;
        for (unsigned i = 0; i < kb; i++) w[at++] = keys[k * stride + i];
        if (found) {
          for (unsigned i = 0; i < length; i++) w[at++] = head[i];
          for (size_t i = 64; i < prb; i++) w[at++] = path[i];
          CHECK(at == rowb, "the row's size");
        }
        if (found) mf::splice_row(out + k * in_stride, 32, {{keys + k * stride, kb}, {head, length}}, path, 64, depth);
        else mf::splice_row(out + k * in_stride, 32, {{keys + k * stride, kb}}, nullptr, 64, depth);
      }
      const bool same = !memcmp(out, want, out_bytes);
      free(head);
      free(path);
      free(out);
      free(want);
      CHECK(same, "the rows differ");
    }
    free(keys);
    printf("ok %u %u %u %u %zu\n", kb, nq, plan.nu, kw, rowb);
  }
  return 0;
}
