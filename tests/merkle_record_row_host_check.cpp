// The host arithmetic of mfh_merkle_update_records (csrc/merkle_rows.hpp: the row's size, the chunk size, the splice of a staged head and a staged
// level row into the packed input row of words.MerkleRecordUpdate) as a program of its own (tests/test_merkle_record_row_host_cpu.py builds it with the
// address and undefined-behaviour sanitizers and runs it).  Every line of standard input is
//   <length> <depth> <extra> <n> <seed>
// n rows of row_bytes(64, 2 length, depth) + extra bytes (the in_stride) are spliced from n heads and n level rows.  The heads, the level rows and
// the output live in heap allocations of exactly their sizes: the heads n x 2 x head_pitch bytes less the last slot's unused tail (the splice reads
// `length` bytes of each half), the level rows n x row_bytes(64, 64, depth) at that exact stride, the output (n - 1) x in_stride + the row's bytes -- so a
// read or write one byte outside them is a heap overflow the address sanitizer reports.  The expected row is put together here byte by byte.
// Prints "ok <length> <depth> <extra> <n> <row bytes> <chunk of 1000000 updates at 64 MiB>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

int main() {
  char buf[256];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned length = 0, depth = 0, extra = 0, n = 0;
    unsigned long long seed = 0;
    if (sscanf(buf, "%u %u %u %u %llu", &length, &depth, &extra, &n, &seed) != 5 || depth < 1 || depth > 24 || length > (1u << 20) || n < 1 || n > 64) {
      fprintf(stderr, "merkle_record_row_host_check: expected <length <= 2^20> <depth in 1 .. 24> <extra> <n in 1 .. 64> <seed>\n");
      return 2;
    }
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    const size_t rowb = mf::row_bytes(64, 2 * (size_t)length, depth), lrb = mf::row_bytes(64, 64, depth), hp = mf::record_head_pitch(length), stride = rowb + extra;
    const size_t idxb = (depth + 7) / 8;
    if (rowb != 64 + 2 * (size_t)length + 32 * (size_t)depth + idxb || lrb != 128 + 32 * (size_t)depth + idxb || hp < length || hp % 16 || hp >= (size_t)length + 16) {
      fprintf(stderr, "merkle_record_row_host_check: the sizes differ\n");
      return 1;
    }
    const size_t heads_bytes = length ? (size_t)(n - 1) * 2 * hp + hp + length : 0, out_bytes = (size_t)(n - 1) * stride + rowb;
    uint8_t *heads = exact(heads_bytes), *levels = exact((size_t)n * lrb), *out = exact(out_bytes), *want = exact(out_bytes);
    for (size_t i = 0; i < heads_bytes; i++) heads[i] = rnd();
    for (size_t i = 0; i < (size_t)n * lrb; i++) levels[i] = rnd();
    for (size_t i = 0; i < out_bytes; i++) out[i] = want[i] = 0xA5;
    for (unsigned k = 0; k < n; k++) {
      uint8_t *w = want + (size_t)k * stride;
      size_t at = 0;
      for (unsigned i = 0; i < 64; i++) w[at++] = 0;
      for (unsigned i = 0; i < length; i++) w[at++] = heads[(size_t)k * 2 * hp + i];
      for (unsigned i = 0; i < length; i++) w[at++] = heads[(size_t)k * 2 * hp + hp + i];
      for (size_t i = 128; i < lrb; i++) w[at++] = levels[(size_t)k * lrb + i];
      if (at != rowb) return 1;
      const uint8_t *head = heads + (size_t)k * 2 * hp;
      mf::splice_row(out + (size_t)k * stride, 64, {{head, length}, {head + hp, length}}, levels + (size_t)k * lrb, 128, depth);
    }
    const bool ok = !memcmp(out, want, out_bytes);
    // the chunk: the most rows that fit, at least one, at most what there is
    const size_t stage = (size_t)64 << 20;
    const uint32_t ch = mf::update_chunk(1000000, rowb, stage);
    const bool chunk_ok = ch >= 1 && ch <= 1000000 && (ch == 1 || (size_t)ch * rowb <= stage) && (ch == 1000000 || ((size_t)ch + 1) * rowb > stage) &&
                          mf::update_chunk(1, rowb, stage) == 1 && mf::update_chunk(3, rowb, 1) == 1 && mf::update_chunk(7, 1, 5) == 5;
    free(heads);
    free(levels);
    free(out);
    free(want);
    if (!ok || !chunk_ok) {
      fprintf(stderr, "merkle_record_row_host_check: length %u depth %u extra %u: %s\n", length, depth, extra, ok ? "the chunk differs" : "the rows differ");
      return 1;
    }
    printf("ok %u %u %u %u %zu %u\n", length, depth, extra, n, rowb, ch);
  }
  return 0;
}
