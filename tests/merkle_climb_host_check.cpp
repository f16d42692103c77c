// The host half of the cut reads (mfh_merkle_paths_cut, mfh_merkle_absent_rows_cut) in csrc/merkle_rows.hpp -- the chunk arithmetic, the plan handed to
// k_merkle_climb_rows and the splice out of the staged rows -- as a program of its own (tests/test_merkle_climb_host_cpu.py builds it with the address and
// undefined-behaviour sanitizers, runs it and compares what it prints with sizes computed independently).  Every line of standard input is
//   <depth> <n> <key_bytes> <length> <stage_bytes> <dump> <cut> [<cut> ..]
// n > 0 statements; key_bytes = length = 0 is a call of paths (segment 0 a MerklePath row, the leaf in the staged row), else an absent call (segment 0 a
// MerkleAbsent row under a head of key and record); the cuts ascending, 1 <= cut < depth <= 24.  It prints
//   chunk <statements a chunk> <staged units a statement> <upper row bytes a statement> <widest row's units> <segments>
//   seg <lo> <levels> <base> <head>                      per segment of the FIRST chunk's plan
// and with dump = 1, for the first chunk, whose staged rows are filled with byte j of unit u of statement b of segment g = (131 g + 31 b + 7 u + j) mod 256,
// its key with 0xC0 + b and its record with 0x40 + byte mod 64:
//   row <g> <b> <hex>                                    every caller's row, spliced; statement b with b mod 3 = 2 has no record (status 2)
// The staged buffer and every caller's row live in heap allocations of exactly their sizes, so a read or write one byte outside is a heap overflow the
// address sanitizer reports.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "merkle_rows.hpp"

template <class T> static T *exact(size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (!p) exit(3);
  return p;
}

int main() {
  char buf[512];
  while (fgets(buf, sizeof buf, stdin)) {
    unsigned depth = 0, n = 0, key_bytes = 0, length = 0, dump = 0;
    unsigned long long stage = 0;
    int used = 0;
    const int got = sscanf(buf, "%u %u %u %u %llu %u%n", &depth, &n, &key_bytes, &length, &stage, &dump, &used);
    std::vector<uint32_t> cut_list;
    bool bad = got < 6 || depth < 2 || depth > 24 || !n || dump > 1 || !stage || (!key_bytes != !length);
    if (!bad) {
      const char *at = buf + used;
      unsigned c = 0;
      int step = 0;
      while (sscanf(at, "%u%n", &c, &step) == 1) {
        bad = bad || c < 1 || c >= depth || (!cut_list.empty() && c <= cut_list.back());
        cut_list.push_back(c);
        at += step;
      }
      bad = bad || cut_list.empty();
    }
    if (bad) {
      fprintf(stderr, "merkle_climb_host_check: expected <depth in 2 .. 24> <n > 0> <key_bytes> <length> <stage_bytes> <dump 0|1> <ascending cuts in [1, depth)>\n");
      return 2;
    }
    const uint32_t ncuts = (uint32_t)cut_list.size();
    uint32_t *cuts = exact<uint32_t>(ncuts);
    memcpy(cuts, cut_list.data(), ncuts * sizeof(uint32_t));
    const bool paths = !key_bytes;
    const size_t rowb0 = paths ? mf::climb_row_bytes(cuts[0]) : mf::row_bytes(32, (size_t)key_bytes + length, cuts[0]);
    const uint32_t ch = mf::climb_chunk(n, rowb0, depth, ncuts, cuts, (size_t)stage);
    const size_t su = mf::climb_staged_units(depth, ncuts, cuts);
    uint32_t widest = 0;
    const mf::ClimbPlan plan = mf::climb_plan(depth, ncuts, cuts, ch, paths, &widest);
    printf("chunk %u %zu %zu %u %u\n", ch, su, mf::climb_rows_bytes(depth, ncuts, cuts), widest, plan.nseg);
    for (uint32_t g = 0; g < plan.nseg; g++) printf("seg %u %u %u %u\n", plan.lo[g], plan.levels[g], plan.base[g], plan.head[g]);
    if (dump) {
      uint8_t *staged = exact<uint8_t>((size_t)ch * su * 16);
      for (uint32_t g = 0; g < plan.nseg; g++) {
        const uint32_t units = mf::climb_row_units(plan.levels[g]);
        for (uint32_t b = 0; b < ch; b++)
          for (uint32_t u = 0; u < units; u++)
            for (uint32_t j = 0; j < 16; j++) staged[((size_t)plan.base[g] + (size_t)b * units + u) * 16 + j] = (uint8_t)(131 * g + 31 * b + 7 * u + j);
      }
      uint8_t *key = exact<uint8_t>(key_bytes), *record = exact<uint8_t>(length);
      for (uint32_t g = 0; g < plan.nseg; g++) {
        const uint32_t units = mf::climb_row_units(plan.levels[g]);
        const size_t rowb = g ? mf::climb_row_bytes(plan.levels[g]) : rowb0;
        for (uint32_t b = 0; b < ch; b++) {
          const bool found = paths || b % 3 != 2;
          const uint8_t *st = staged + ((size_t)plan.base[g] + (size_t)b * units) * 16;
          uint8_t *row = exact<uint8_t>(rowb);
          memset(row, 0xAB, rowb);
          size_t wrote = rowb;
          if (g || paths) {
            mf::splice_climb_row(row, found ? st : nullptr, plan.levels[g]);
          } else {
            memset(key, 0xC0 + b, key_bytes);
            for (uint32_t j = 0; j < length; j++) record[j] = (uint8_t)(0x40 + j % 64);
            mf::splice_row(row, 32, {{key, key_bytes}, {record, found ? length : 0}}, found ? st : nullptr, 64, plan.levels[0]);
            if (!found) wrote = 32 + key_bytes;
          }
          printf("row %u %u ", g, b);
          for (size_t j = 0; j < wrote; j++) printf("%02x", row[j]);
          for (size_t j = wrote; j < rowb; j++)
            if (row[j] != 0xAB) {
              fprintf(stderr, "merkle_climb_host_check: segment %u statement %u: byte %zu behind the status 2 row's key was written\n", g, b, j);
              return 1;
            }
          printf("\n");
          free(row);
        }
      }
      free(staged); free(key); free(record);
    }
    free(cuts);
  }
  return 0;
}
