// The host-compiled half of mfh_merkle_grow in csrc/merkle_grow.hpp -- where every node of a grown tree comes from (mf::grow_node) and the roots of the
// all-inert subtrees (mf::grow_inert_roots), the same text the kernels and the driver of merkle.hip compile -- as a program of its own
// (tests/test_merkle_grow_host_cpu.py builds it with the address and undefined-behaviour sanitizers, runs it and compares what it prints with values
// computed independently).  Every line of standard input is one of
//   place <depth> <new_depth>                       (new_depth <= 16: every position is visited)
//       walks the new tree level by level, index by index -- position 2^(new_depth - l) + i, the layout of merkle.hip -- and asks mf::grow_node about each:
//       the level and index it reports must be the walk's, the kind the one the level and index call for, a copy's `from` the old position of that level
//       and index.  Then every 16-byte unit of the new tree's memory is filled as k_grow_nodes and k_grow_spine fill it, from an old tree whose unit u
//       holds the value u and constants that hold their level: a copied unit must hold its old unit's number, a constant its level.
//       prints  place <copies> <inert> <spine> <unused> <old positions copied exactly once> <units written exactly once>
//   edge <depth> <new_depth>                        (any depths: arithmetic on the boundaries alone)
//       per level the positions at the edges of the three ranges -- the first and the last copy, the first and the last constant, the spine node -- and
//       positions 0 and 2^(new_depth + 1) - 1.
//       prints  edge <copies, summed from the boundaries> <inert> <spine> <positions asked>
//   roots <records: 0 | 1> <length> <depth>
//       prints  roots <E_0> .. <E_depth>            (mf::grow_inert_roots: 64 hex digits each, the bytes as the tree stores them)
// The two trees, the per-position counters and the constants live in heap allocations of exactly their sizes, so a read or a write one unit outside is a
// heap overflow the address sanitizer reports.  Exit 2: a malformed line; exit 4: the placement disagrees with the layout.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "merkle_grow.hpp"

template <class T> static T *exact(size_t count) {
  T *p = (T *)calloc(count ? count : 1, sizeof(T));
  if (!p) exit(3);
  return p;
}

static int refuse() {
  fprintf(stderr, "merkle_grow_host_check: expected `place <depth >= 1> <new_depth in depth + 1 .. 16>`, `edge <depth >= 1> <new_depth in depth + 1 .. 24>` or "
                  "`roots <0 | 1> <length <= 2^20> <depth <= 24>`\n");
  return 2;
}

static int wrong(const char *what, uint64_t at) {
  fprintf(stderr, "merkle_grow_host_check: %s at %llu\n", what, (unsigned long long)at);
  return 4;
}

static bool number(const char *tok, uint64_t *v) {
  char *end = nullptr;
  if (!tok || !*tok || *tok == '-') return false;
  *v = strtoull(tok, &end, 10);
  return *end == 0;
}

// what node i of level l of the grown tree is, from the statement of the growth alone
static uint32_t kind_of(uint32_t d, uint32_t l, uint64_t i) {
  if (l <= d) return i < ((uint64_t)1 << (d - l)) ? mf::kGrowCopy : mf::kGrowInert;
  return i ? mf::kGrowInert : mf::kGrowSpine;
}

static int ask(uint32_t d, uint32_t D, uint32_t l, uint64_t i, uint64_t count[4], uint64_t *from) {
  const uint64_t p = ((uint64_t)1 << (D - l)) + i;
  const mf::GrowNode n = mf::grow_node(d, D, (uint32_t)p);
  if (n.level != l || n.index != i) return wrong("level or index", p);
  if (n.kind != kind_of(d, l, i)) return wrong("kind", p);
  if (n.from != (n.kind == mf::kGrowCopy ? ((uint64_t)1 << (d - l)) + i : 0)) return wrong("from", p);
  count[n.kind]++;
  if (from) *from = n.from;
  return 0;
}

static int place(uint32_t d, uint32_t D) {
  const size_t old_nodes = (size_t)2 << d, new_nodes = (size_t)2 << D;
  uint8_t *asked = exact<uint8_t>(new_nodes), *copied = exact<uint8_t>(old_nodes), *written = exact<uint8_t>(2 * new_nodes);
  uint64_t count[4] = {0, 0, 0, 0};
  for (uint32_t l = 0; l <= D; l++)
    for (uint64_t i = 0; i < (uint64_t)1 << (D - l); i++) {
      uint64_t from = 0;
      if (int rc = ask(d, D, l, i, count, &from)) return rc;
      asked[((size_t)1 << (D - l)) + i]++;
      if (from) {
        if (from >= old_nodes) return wrong("a copy from outside the old tree", from);
        copied[from]++;
      }
    }
  if (mf::grow_node(d, D, 0).kind != mf::kGrowUnused) return wrong("position 0", 0);
  count[mf::kGrowUnused]++;
  for (size_t p = 1; p < new_nodes; p++)
    if (asked[p] != 1) return wrong("a position the walk did not reach once", p);
  uint64_t once = 0;
  for (size_t q = 1; q < old_nodes; q++) once += copied[q] == 1;
  if (copied[0]) return wrong("the old tree's unused position copied", 0);
  // the units, as the kernels move them: unit u of the old tree holds u, a constant of level l holds 0x80000000 | l, a spine node 0xC0000000 | its level
  uint32_t *from = exact<uint32_t>(2 * old_nodes), *nodes = exact<uint32_t>(2 * new_nodes);
  for (size_t u = 0; u < 2 * old_nodes; u++) from[u] = (uint32_t)u;
  if (mf::grow_units(D) != 2 * new_nodes) return wrong("grow_units", D);
  for (uint32_t g = 0; g < mf::grow_units(D); g++) {  // k_grow_nodes, a lane a unit
    const mf::GrowNode n = mf::grow_node(d, D, g >> 1);
    if (n.kind == mf::kGrowCopy) {
      nodes[g] = from[2 * (size_t)n.from + (g & 1)];
      written[g]++;
    } else if (n.kind == mf::kGrowInert) {
      nodes[g] = 0x80000000u | n.level;
      written[g]++;
    }
  }
  for (uint32_t l = d; l < D; l++) {  // k_grow_spine
    const size_t k = (size_t)1 << (D - l - 1);
    nodes[2 * k] = nodes[2 * k + 1] = 0xC0000000u | (l + 1);
    written[2 * k]++;
    written[2 * k + 1]++;
  }
  written[0]++;  // the memset of position 0
  written[1]++;
  uint64_t units_once = 0;
  for (size_t g = 0; g < 2 * new_nodes; g++) units_once += written[g] == 1;
  for (uint32_t l = 0; l <= D; l++)
    for (uint64_t i = 0; i < (uint64_t)1 << (D - l); i++)
      for (uint32_t half = 0; half < 2; half++) {
        const size_t g = 2 * (((size_t)1 << (D - l)) + i) + half;
        const uint32_t k = kind_of(d, l, i);
        const uint32_t want = k == mf::kGrowCopy ? (uint32_t)(2 * (((size_t)1 << (d - l)) + i) + half) : k == mf::kGrowInert ? 0x80000000u | l : 0xC0000000u | l;
        if (nodes[g] != want) return wrong("a unit's value", g);
      }
  printf("place %llu %llu %llu %llu %llu %llu\n", (unsigned long long)count[mf::kGrowCopy], (unsigned long long)count[mf::kGrowInert],
         (unsigned long long)count[mf::kGrowSpine], (unsigned long long)count[mf::kGrowUnused], (unsigned long long)once, (unsigned long long)units_once);
  free(asked);
  free(copied);
  free(written);
  free(from);
  free(nodes);
  return 0;
}

static int edge(uint32_t d, uint32_t D) {
  uint64_t count[4] = {0, 0, 0, 0}, copies = 0, inert = 0, spine = 0, asked = 0;
  for (uint32_t l = 0; l <= D; l++) {
    const uint64_t width = (uint64_t)1 << (D - l), old = l <= d ? (uint64_t)1 << (d - l) : 0;
    uint64_t first = 0, last = 0;
    if (old) {  // the copies [0, old): `from` runs over the old level, in order
      if (int rc = ask(d, D, l, 0, count, &first)) return rc;
      if (int rc = ask(d, D, l, old - 1, count, &last)) return rc;
      if (first != old || last != 2 * old - 1) return wrong("the old level's ends", l);
      copies += last - first + 1;
      asked += 2;
    } else {
      if (int rc = ask(d, D, l, 0, count, nullptr)) return rc;
      spine++;
      asked++;
    }
    const uint64_t c0 = old ? old : 1;  // the constants [c0, width)
    if (c0 < width) {
      if (int rc = ask(d, D, l, c0, count, nullptr)) return rc;
      if (int rc = ask(d, D, l, width - 1, count, nullptr)) return rc;
      inert += width - c0;
      asked += 2;
    }
  }
  if (mf::grow_node(d, D, 0).kind != mf::kGrowUnused) return wrong("position 0", 0);
  const mf::GrowNode top = mf::grow_node(d, D, (uint32_t)(((uint64_t)2 << D) - 1));  // the last leaf
  if (top.level != 0 || top.index != ((uint64_t)1 << D) - 1 || top.kind != mf::kGrowInert) return wrong("the last position", ((uint64_t)2 << D) - 1);
  printf("edge %llu %llu %llu %llu\n", (unsigned long long)copies, (unsigned long long)inert, (unsigned long long)spine, (unsigned long long)(asked + 2));
  return 0;
}

static int roots(bool records, uint32_t length, uint32_t depth) {
  mf::GrowRoots *r = (mf::GrowRoots *)aligned_alloc(alignof(mf::GrowRoots), sizeof(mf::GrowRoots));
  if (!r) exit(3);
  mf::grow_inert_roots(records, length, depth, *r);
  printf("roots");
  for (uint32_t l = 0; l <= depth; l++) {
    uint8_t b[32];
    memcpy(b, r->w + 8 * l, 32);
    printf(" ");
    for (int j = 0; j < 32; j++) printf("%02x", b[j]);
  }
  printf("\n");
  for (uint32_t j = 8 * (depth + 1); j < 8 * (mf::kGrowMaxDepth + 1); j++)
    if (r->w[j]) return wrong("a constant above the depth", j);
  free(r);
  return 0;
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    char *tok[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    for (char *t = strtok(line, " \n"); t && n < 5; t = strtok(nullptr, " \n")) tok[n++] = t;
    if (!n) continue;
    uint64_t a = 0, b = 0, c = 0;
    int rc = 2;
    if (!strcmp(tok[0], "place") && n == 3 && number(tok[1], &a) && number(tok[2], &b) && a >= 1 && a < b && b <= 16) rc = place((uint32_t)a, (uint32_t)b);
    else if (!strcmp(tok[0], "edge") && n == 3 && number(tok[1], &a) && number(tok[2], &b) && a >= 1 && a < b && b <= mf::kGrowMaxDepth) rc = edge((uint32_t)a, (uint32_t)b);
    else if (!strcmp(tok[0], "roots") && n == 4 && number(tok[1], &a) && number(tok[2], &b) && number(tok[3], &c) && a <= 1 && b <= (1u << 20) && c <= mf::kGrowMaxDepth)
      rc = roots(a == 1, (uint32_t)b, (uint32_t)c);
    if (rc == 2) return refuse();
    if (rc) return rc;
  }
  return 0;
}
