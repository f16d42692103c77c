// The host-compiled half of the device key sort in csrc/merkle_sort.hpp -- the tile size, the scratch layouts of mfh_merkle_load_keys and
// mfh_merkle_check_table, the slice of a merge pass' workgroup and the merge-path partition, the same text the kernels of merkle.hip compile -- as a program
// of its own (tests/test_merkle_sort_host_cpu.py builds it with the address and undefined-behaviour sanitizers, runs it and compares what it prints with
// values computed independently).  Every line of standard input is one of
//   tile
//       prints  tile <kSortTile>
//   scratch <depth> <n> <key_bytes>
//       prints  scratch <tiles> <passes> | <ent0_at> <ent1_at> <status_at> <bytes> | <nb> <mask_at> <count_at> <slots_at> <dense_at> <total_at> <ent0_at> <ent1_at>
//               <result_at> <digests_at> <bytes>                 (mf::load_scratch, then mf::check_scratch)
//   slice <n> <run> <group>
//       prints  slice <out0> <count> <a_at> <na> <nb> <d0>       (mf::merge_slice)
//   merge <kw> <na> <nb> <mode> <seed> <step>
//       two sorted runs of na and nb entries of kw key words and a tag, made here from the seed (mode 0: every word one of three values; 1: all keys equal, the
//       tag alone decides; 2: keys that differ in their last word alone).  mf::merge_path on EVERY diagonal 0 .. na + nb against a sequential merge; then the
//       slices between the diagonals 0, step, 2 step, .. each merged on its own into one output, which must be the whole merge.
//       prints  merge <na + nb> <slices> <FNV-1a over the merged tags>
// The runs, every slice's output and the whole merge live in heap allocations of exactly their sizes, so a read one word outside is a heap overflow the
// address sanitizer reports.  Exit 2: a malformed line; exit 4: the partition disagrees with the sequential merge.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "merkle_sort.hpp"

template <class T> static T *exact(size_t count) {
  T *p = (T *)malloc(count ? count * sizeof(T) : 1);
  if (!p) exit(3);
  return p;
}

static int refuse() {
  fprintf(stderr, "merkle_sort_host_check: expected `tile`, `scratch <depth in 1 .. 24> <n <= 2^depth> <key_bytes in 1 .. 32>`, `slice <n> <run> <group>` or "
                  "`merge <kw in 1 .. 8> <na> <nb> <mode in 0 .. 2> <seed> <step >= 1>`\n");
  return 2;
}

static bool number(const char *tok, uint64_t *v) {
  char *end = nullptr;
  if (!tok || !*tok || *tok == '-') return false;
  *v = strtoull(tok, &end, 10);
  return *end == 0;
}

static uint32_t lcg(uint32_t *state) {
  *state = (*state * 1103515245u + 12345u) & 0x7FFFFFFFu;
  return *state >> 16;
}

// a (p entries from a0) and b (q entries from b0) merged sequentially into out, an entry of a first where the two are equal
template <int KW>
static void merge_seq(const uint32_t *a, uint32_t p, const uint32_t *b, uint32_t q, uint32_t *out) {
  uint32_t i = 0, j = 0;
  while (i < p || j < q) {
    const bool take_a = j == q || (i < p && !mf::sort_less<KW>(b + (size_t)j * (KW + 1), a + (size_t)i * (KW + 1)));
    memcpy(out + (size_t)(i + j) * (KW + 1), take_a ? a + (size_t)i * (KW + 1) : b + (size_t)j * (KW + 1), (KW + 1) * 4);
    if (take_a) i++; else j++;
  }
}

template <int KW>
static int merge_case(uint32_t na, uint32_t nb, uint32_t mode, uint32_t seed, uint32_t step) {
  const uint32_t total = na + nb, W = KW + 1;
  uint32_t *a = exact<uint32_t>((size_t)na * W), *b = exact<uint32_t>((size_t)nb * W), *whole = exact<uint32_t>((size_t)total * W);
  uint32_t state = seed;
  for (uint32_t i = 0; i < total; i++) {
    uint32_t *e = i < na ? a + (size_t)i * W : b + (size_t)(i - na) * W;
    for (int j = 0; j < KW; j++) e[j] = mode == 0 ? lcg(&state) % 3 : mode == 1 ? 0x01020304u : j == KW - 1 ? lcg(&state) % 5 : 0xAAAAAAAAu;
    e[KW] = total - 1 - i;
  }
  auto sort_run = [&](uint32_t *run, uint32_t n) {
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return mf::sort_less<KW>(run + (size_t)x * W, run + (size_t)y * W); });
    std::vector<uint32_t> copy(run, run + (size_t)n * W);
    for (uint32_t i = 0; i < n; i++) memcpy(run + (size_t)i * W, copy.data() + (size_t)order[i] * W, W * 4);
  };
  sort_run(a, na);
  sort_run(b, nb);
  merge_seq<KW>(a, na, b, nb, whole);
  // every diagonal: the entries of a among the first d of the whole merge (tags below nb are b's: a's tags are total - 1 - i >= nb)
  uint32_t from_a = 0;
  for (uint32_t d = 0; d <= total; d++) {
    if (mf::merge_path<KW>(a, na, b, nb, d) != from_a) return 4;
    if (d < total && whole[(size_t)d * W + KW] >= nb) from_a++;
  }
  uint32_t *joined = exact<uint32_t>((size_t)total * W);
  uint32_t slices = 0, covered = 0;
  for (uint32_t d0 = 0; d0 < total || !slices; d0 += step) {
    const uint32_t d1 = std::min(d0 + step, total), a0 = mf::merge_path<KW>(a, na, b, nb, d0), a1 = mf::merge_path<KW>(a, na, b, nb, d1);
    const uint32_t b0 = d0 - a0, b1 = d1 - a1;
    if (a1 < a0 || b1 < b0) return 4;
    uint32_t *sa = exact<uint32_t>((size_t)(a1 - a0) * W), *sb = exact<uint32_t>((size_t)(b1 - b0) * W), *out = exact<uint32_t>((size_t)(d1 - d0) * W);
    memcpy(sa, a + (size_t)a0 * W, (size_t)(a1 - a0) * W * 4);  // (exact copies: merging the slice reads nothing outside it)
    memcpy(sb, b + (size_t)b0 * W, (size_t)(b1 - b0) * W * 4);
    merge_seq<KW>(sa, a1 - a0, sb, b1 - b0, out);
    memcpy(joined + (size_t)d0 * W, out, (size_t)(d1 - d0) * W * 4);
    covered += (a1 - a0) + (b1 - b0);
    slices++;
    free(sa);
    free(sb);
    free(out);
    if (!total) break;
  }
  if (covered != total || memcmp(joined, whole, (size_t)total * W * 4)) return 4;
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < total; i++) h = (h ^ joined[(size_t)i * W + KW]) * 16777619u;
  printf("merge %u %u %u\n", total, slices, h);
  free(a);
  free(b);
  free(whole);
  free(joined);
  return 0;
}

int main() {
  char buf[1 << 12];
  while (fgets(buf, sizeof buf, stdin)) {
    std::vector<char *> tok;
    for (char *t = strtok(buf, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
    if (tok.empty()) return refuse();
    uint64_t v[6] = {0, 0, 0, 0, 0, 0};
    for (size_t i = 1; i < tok.size(); i++)
      if (i > 6 || !number(tok[i], &v[i - 1])) return refuse();
    if (!strcmp(tok[0], "tile")) {
      if (tok.size() != 1) return refuse();
      printf("tile %u\n", mf::kSortTile);
    } else if (!strcmp(tok[0], "scratch")) {
      if (tok.size() != 4 || v[0] < 1 || v[0] > 24 || v[1] > ((uint64_t)1 << v[0]) || v[2] < 1 || v[2] > 32) return refuse();
      const uint32_t depth = (uint32_t)v[0], n = (uint32_t)v[1], key_bytes = (uint32_t)v[2];
      const mf::LoadScratch l = mf::load_scratch(depth, n, key_bytes);
      const mf::CheckScratch c = mf::check_scratch(depth, n, key_bytes);
      printf("scratch %u %u | %zu %zu %zu %zu | %u %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", mf::sort_tiles(n), mf::sort_passes(n), l.ent0_at, l.ent1_at, l.status_at,
             l.bytes, c.nb, c.mask_at, c.count_at, c.slots_at, c.dense_at, c.total_at, c.ent0_at, c.ent1_at, c.result_at, c.digests_at, c.bytes);
    } else if (!strcmp(tok[0], "slice")) {
      if (tok.size() != 4 || v[0] < 1 || v[0] > (1u << 24) || v[1] < mf::kSortTile || v[1] % mf::kSortTile || v[1] > (1u << 24) || v[2] >= mf::sort_tiles((uint32_t)v[0]))
        return refuse();
      const mf::MergeSlice s = mf::merge_slice((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
      printf("slice %u %u %u %u %u %u\n", s.out0, s.count, s.a_at, s.na, s.nb, s.d0);
    } else if (!strcmp(tok[0], "merge")) {
      if (tok.size() != 7 || v[0] < 1 || v[0] > 8 || v[1] > (1u << 16) || v[2] > (1u << 16) || v[3] > 2 || v[4] > 0x7FFFFFFFu || v[5] < 1 || v[5] > (1u << 16)) return refuse();
      const uint32_t na = (uint32_t)v[1], nb = (uint32_t)v[2], mode = (uint32_t)v[3], seed = (uint32_t)v[4], step = (uint32_t)v[5];
      int rc = 2;
      switch (v[0]) {
        case 1: rc = merge_case<1>(na, nb, mode, seed, step); break;
        case 2: rc = merge_case<2>(na, nb, mode, seed, step); break;
        case 3: rc = merge_case<3>(na, nb, mode, seed, step); break;
        case 4: rc = merge_case<4>(na, nb, mode, seed, step); break;
        case 5: rc = merge_case<5>(na, nb, mode, seed, step); break;
        case 6: rc = merge_case<6>(na, nb, mode, seed, step); break;
        case 7: rc = merge_case<7>(na, nb, mode, seed, step); break;
        case 8: rc = merge_case<8>(na, nb, mode, seed, step); break;
      }
      if (rc) return rc;
    } else {
      return refuse();
    }
  }
  return 0;
}
