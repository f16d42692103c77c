// A stand-alone program (its own main; built with -fsanitize=address,undefined by tests/test_merkle_block_host_cpu.py) for csrc/merkle_block.hpp: block_windows,
// block_plan and block_layout against a sequential model that works on the TABLE'S BYTES, one step at a time, and against formulas written out literally.
// One case a line on stdin; one line of output a case; exit status 2 for a malformed line.
//   r <wb> <mem> <nk> <seed>   random blocks of nk steps of all three kinds among mem members and two keys that are no members; writes of wb bytes at several
//                              offsets (over the balance too), with expectations that hold, that only the block satisfies and that are stale; both policies
//   c <seed>                   the crafted blocks: every status alone and together, a write over the balance and a transfer that spends it, a compare-and-set
//                              that only an earlier adjust satisfies and one an earlier transfer has broken, windows of 1, 16, 17 and 39 bytes side by side
//   l <max_updates> <max_src> <length> <rowb> <depth> <ncuts> <stage>   block_layout against the literal formulas (cuts 1, 2, ..)
// Every array the plan reads is a heap allocation of exactly its bytes.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <string>

#include "merkle_block.hpp"

namespace {

using namespace mf;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

struct Step {  // a step as the caller states it, with bytes of its own
  uint8_t kind = 0, side = 0;
  uint32_t a = 0, b = 0, lo = 0, hi = 0;
  uint64_t amount = 0;
  std::vector<uint8_t> value, expect;
  bool has_expect = false;
};

struct Table {
  uint32_t K, A, length;
  std::vector<uint32_t> rec;                 // per unique key: its record, or kNoRecord
  std::vector<std::vector<uint8_t>> records;  // the table
};

uint64_t be(const uint8_t *p, uint32_t n) {
  uint64_t v = 0;
  for (uint32_t b = 0; b < n; b++) v = v << 8 | p[b];
  return v;
}
void put_be(uint8_t *p, uint32_t n, uint64_t v) {
  for (uint32_t b = 0; b < n; b++) p[b] = (uint8_t)(v >> (8 * (n - 1 - b)));
}

// the sequential model: one step on the table's bytes as they stand; returns the status and, for an applied step, appends the records it wrote
uint8_t model_step(Table &t, const Step &s, std::vector<std::pair<uint32_t, std::vector<uint8_t>>> &written) {
  const uint32_t K = t.K, A = t.A;
  const uint64_t limit = A >= 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * A)) - 1);
  if (t.rec[s.a] == kNoRecord) return 1;
  std::vector<uint8_t> &ra = t.records[t.rec[s.a]];
  if (s.kind == kBlockTransfer) {
    if (t.rec[s.b] == kNoRecord) return 2;
    std::vector<uint8_t> &rb = t.records[t.rec[s.b]];
    const uint64_t ba = be(ra.data() + 2 * K, A), bb = be(rb.data() + 2 * K, A);
    if (ba < s.amount) return 3;
    if (bb + s.amount < bb || bb + s.amount > limit) return 4;
    put_be(ra.data() + 2 * K, A, ba - s.amount);
    written.push_back({t.rec[s.a], ra});
    put_be(rb.data() + 2 * K, A, bb + s.amount);
    written.push_back({t.rec[s.b], rb});
    return 0;
  }
  if (s.kind == kBlockAdjust) {
    const uint64_t b = be(ra.data() + 2 * K, A);
    if (s.side && b < s.amount) return 3;
    if (!s.side && (b + s.amount < b || b + s.amount > limit)) return 4;
    put_be(ra.data() + 2 * K, A, s.side ? b - s.amount : b + s.amount);
    written.push_back({t.rec[s.a], ra});
    return 0;
  }
  if (s.has_expect && memcmp(ra.data() + s.lo, s.expect.data(), s.hi - s.lo)) return 5;
  memcpy(ra.data() + s.lo, s.value.data(), s.hi - s.lo);
  written.push_back({t.rec[s.a], ra});
  return 0;
}

struct Outcome {
  uint32_t failed, nupd;
};

// the plan of `steps` on `table` under both policies against the model
Outcome check_block(const Table &table, const std::vector<Step> &steps, const uint8_t *want_status = nullptr) {
  const uint32_t nk = (uint32_t)steps.size(), nu = (uint32_t)table.rec.size(), K = table.K, A = table.A;
  // exact-size heap arrays for everything the plan reads
  std::unique_ptr<BlockStep[]> bs(new BlockStep[nk]);
  std::vector<std::unique_ptr<uint8_t[]>> bytes;
  for (uint32_t j = 0; j < nk; j++) {
    const Step &s = steps[j];
    bs[j] = BlockStep{s.kind, s.side, s.a, s.b, s.amount, s.lo, s.hi, nullptr, nullptr};
    if (s.kind == kBlockWrite) {
      bytes.emplace_back(new uint8_t[s.hi - s.lo]);
      memcpy(bytes.back().get(), s.value.data(), s.hi - s.lo);
      bs[j].value = bytes.back().get();
      if (s.has_expect) {
        bytes.emplace_back(new uint8_t[s.hi - s.lo]);
        memcpy(bytes.back().get(), s.expect.data(), s.hi - s.lo);
        bs[j].expect = bytes.back().get();
      }
    }
  }
  BlockWindows w;
  block_windows(nk, bs.get(), nu, K, A, w);
  // the windows: the hull of what a key's steps touch, a prefix sum of whole units
  uint64_t units = 0, max_updates = 0, max_src = 0;
  for (uint32_t u = 0; u < nu; u++) {
    uint32_t f0 = 0xFFFFFFFFu, f1 = 0;
    for (const Step &s : steps) {
      const bool money_a = s.kind != kBlockWrite && s.a == u, money_b = s.kind == kBlockTransfer && s.b == u;
      if (money_a || money_b) f0 = std::min(f0, 2 * K), f1 = std::max(f1, 2 * K + A);
      if (s.kind == kBlockWrite && s.a == u) f0 = std::min(f0, s.lo), f1 = std::max(f1, s.hi);
    }
    CHECK(w.f0[u] == f0 && w.f1[u] == f1 && w.first[u] == units);
    if (f1 > f0) units += (f1 - f0 + 15) / 16;
  }
  for (const Step &s : steps) {
    max_updates += s.kind == kBlockTransfer ? 2 : 1;
    max_src += w.f1[s.a] - w.f0[s.a];
    if (s.kind == kBlockTransfer) max_src += w.f1[s.b] - w.f0[s.b];
  }
  CHECK(w.units == units && w.first[nu] == units && w.max_updates == max_updates && w.max_src == max_src);
  std::unique_ptr<uint32_t[]> rec(new uint32_t[nu]);
  for (uint32_t u = 0; u < nu; u++) rec[u] = table.rec[u];
  Outcome out{0, 0};
  for (int skip = 1; skip >= 0; skip--) {
    // what k_window_gather leaves: the window's bytes, zero behind them, all zero for a key that is no member
    std::unique_ptr<uint8_t[]> win(new uint8_t[(size_t)units * 16 + 1]);  // (+ 1: new[0] is legal but useless)
    memset(win.get(), 0, (size_t)units * 16);
    for (uint32_t u = 0; u < nu; u++)
      if (rec[u] != kNoRecord && w.f1[u] > w.f0[u]) memcpy(win.get() + (size_t)16 * w.first[u], table.records[rec[u]].data() + w.f0[u], w.f1[u] - w.f0[u]);
    BlockPlan plan;
    block_plan(nk, bs.get(), K, A, w, rec.get(), win.get(), skip != 0, plan);
    Table t = table;
    uint32_t failed = 0, first = nk, r = 0;
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> written;
    CHECK(plan.status.size() == nk && plan.index.size() == (size_t)2 * nk && plan.first_update.size() == (size_t)nk + 1);
    for (uint32_t j = 0; j < nk; j++) {
      const Step &s = steps[j];
      written.clear();
      const uint8_t st = model_step(t, s, written);
      CHECK(plan.status[j] == st);
      if (want_status) CHECK(st == want_status[j]);
      CHECK(plan.index[2 * (size_t)j] == table.rec[s.a]);
      CHECK(plan.index[2 * (size_t)j + 1] == (s.kind == kBlockTransfer ? table.rec[s.b] : kNoRecord));
      if (st) {
        failed++;
        if (first == nk) first = j;
      }
      if (!skip) continue;
      CHECK(plan.first_update[j] == r);
      CHECK(written.size() == (st ? 0u : s.kind == kBlockTransfer ? 2u : 1u));
      for (const auto &wr : written) {  // update r: the record BEFORE the block with the window taken from the source bytes is the model's record right after the step
        CHECK(r < plan.upd.size());
        const BlockUpdate &up = plan.upd[r];
        CHECK(up.rec == wr.first && up.f1 > up.f0 && up.f1 <= table.length && (size_t)up.at + (up.f1 - up.f0) <= plan.src.size());
        std::vector<uint8_t> fresh = table.records[up.rec];
        memcpy(fresh.data() + up.f0, plan.src.data() + up.at, up.f1 - up.f0);
        CHECK(fresh == wr.second);
        r++;
      }
      CHECK(plan.first_update[(size_t)j + 1] == r);
    }
    CHECK(plan.failed == failed && plan.first == first);
    if (skip) {
      CHECK(plan.upd.size() == r);
      out = {failed, r};
      size_t at = 0;  // the source bytes stand one behind the other in update order
      for (const BlockUpdate &up : plan.upd) {
        CHECK(up.at == at);
        at += up.f1 - up.f0;
      }
      CHECK(at == plan.src.size());
    } else if (failed) {  // fail-fast: no update
      CHECK(plan.upd.empty() && plan.src.empty());
      for (uint32_t x : plan.first_update) CHECK(x == 0);
    } else {
      CHECK(plan.upd.size() == out.nupd && plan.first_update[nk] == out.nupd);
    }
  }
  return out;
}

Table make_table(uint32_t K, uint32_t A, uint32_t length, uint32_t mem, uint32_t strangers, std::mt19937_64 &rng) {
  Table t{K, A, length, {}, {}};
  const uint32_t nrec = mem + 3;
  for (uint32_t i = 0; i < nrec; i++) {
    std::vector<uint8_t> r(length);
    for (uint8_t &x : r) x = (uint8_t)rng();
    t.records.push_back(r);
  }
  std::vector<uint32_t> slots(nrec);
  for (uint32_t i = 0; i < nrec; i++) slots[i] = i;
  std::shuffle(slots.begin(), slots.end(), rng);
  for (uint32_t u = 0; u < mem + strangers; u++) t.rec.push_back(kNoRecord);
  std::vector<uint32_t> who(mem + strangers);
  for (uint32_t u = 0; u < mem + strangers; u++) who[u] = u;
  std::shuffle(who.begin(), who.end(), rng);  // the strangers anywhere among the unique keys
  for (uint32_t m = 0; m < mem; m++) t.rec[who[m]] = slots[m];
  return t;
}

void random_case(uint32_t wb, uint32_t mem, uint32_t nk, uint64_t seed) {
  std::mt19937_64 rng(seed);
  const uint32_t K = 5, A = 1 + (uint32_t)(seed % 8), length = 2 * K + A + wb + 3 + (uint32_t)(seed % 7);
  Table table = make_table(K, A, length, mem, 2, rng);
  const uint32_t nu = mem + 2;
  const uint64_t limit = A >= 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * A)) - 1);
  uint32_t batches = 0, total = 0, failed = 0;
  for (int pass = 0; pass < 2; pass++) {
    // the model runs along while the block is drawn, so that an expectation can be made to hold at its step
    Table t = table;
    std::vector<Step> steps;
    std::vector<std::pair<uint32_t, std::vector<uint8_t>>> sink;
    for (uint32_t j = 0; j < nk; j++) {
      Step s;
      s.kind = (uint8_t)(rng() % 3);
      s.a = (uint32_t)(rng() % nu);
      if (s.kind == kBlockTransfer) do s.b = (uint32_t)(rng() % nu); while (s.b == s.a);
      if (s.kind != kBlockWrite) {
        const uint64_t pick = rng() % 8;
        s.amount = pick == 0 ? limit : pick == 1 ? 0 : pick < 5 ? rng() % 256 : rng() & limit;
        s.side = (uint8_t)(rng() % 2);
      } else {
        const uint32_t where = (uint32_t)(rng() % 3);  // over the balance, behind it, at the record's end
        s.lo = where == 0 ? 2 * K : where == 1 ? 2 * K + A + 1 : length - wb;
        s.hi = s.lo + wb;
        s.value.resize(wb);
        for (uint8_t &x : s.value) x = (uint8_t)rng();
        s.has_expect = pass == 0 && rng() % 2;
        if (s.has_expect) {
          s.expect.resize(wb);
          if (t.rec[s.a] != kNoRecord && rng() % 4) memcpy(s.expect.data(), t.records[t.rec[s.a]].data() + s.lo, wb);  // holds now -- often by the block alone
          else if (t.rec[s.a] != kNoRecord && rng() % 2) memcpy(s.expect.data(), table.records[t.rec[s.a]].data() + s.lo, wb);  // held before the block
          else for (uint8_t &x : s.expect) x = (uint8_t)rng();
        }
      }
      sink.clear();
      model_step(t, s, sink);
      steps.push_back(s);
    }
    const Outcome o = check_block(table, steps);
    batches++;
    total += nk;
    failed += o.failed;
  }
  printf("ok r %u %u %u %u %u %u\n", wb, mem, nk, batches, total, failed);
}

Step transfer(uint32_t a, uint32_t b, uint64_t v) {
  Step s;
  s.kind = kBlockTransfer, s.a = a, s.b = b, s.amount = v;
  return s;
}
Step adjust(uint32_t a, uint64_t v, uint8_t side) {
  Step s;
  s.kind = kBlockAdjust, s.a = a, s.amount = v, s.side = side;
  return s;
}
Step write(uint32_t a, uint32_t lo, std::vector<uint8_t> value, const std::vector<uint8_t> *expect = nullptr) {
  Step s;
  s.kind = kBlockWrite, s.a = a, s.lo = lo, s.hi = lo + (uint32_t)value.size(), s.value = value;
  if (expect) s.has_expect = true, s.expect = *expect;
  return s;
}

void crafted_case(uint64_t seed) {
  std::mt19937_64 rng(seed);
  const uint32_t K = 4, A = 2, length = 2 * K + A + 45;
  Table table = make_table(K, A, length, 4, 1, rng);
  // unique keys 0 .. 4; make key `gone` the stranger and m[0 .. 3] the members with balances 100, 50, 0, 0xFFFF
  uint32_t gone = 0, m[4], nm = 0;
  for (uint32_t u = 0; u < 5; u++)
    if (table.rec[u] == kNoRecord) gone = u;
    else m[nm++] = u;
  const uint64_t start[4] = {100, 50, 0, 0xFFFF};
  for (int i = 0; i < 4; i++) put_be(table.records[table.rec[m[i]]].data() + 2 * K, A, start[i]);
  auto balance_bytes_of = [&](uint64_t v) {
    std::vector<uint8_t> b(A);
    put_be(b.data(), A, v);
    return b;
  };
  uint32_t blocks = 0;
  auto run = [&](std::vector<Step> steps, std::vector<uint8_t> want, uint32_t want_upd) {
    CHECK(steps.size() == want.size());
    const Outcome o = check_block(table, steps, want.data());
    CHECK(o.nupd == want_upd);
    blocks++;
  };
  const std::vector<uint8_t> stale = {1, 2, 3}, one = {1};
  // every status alone
  run({transfer(gone, m[0], 1)}, {1}, 0);
  run({adjust(gone, 1, 0)}, {1}, 0);
  run({write(gone, 2 * K + A, {9})}, {1}, 0);
  run({transfer(m[0], gone, 1)}, {2}, 0);
  run({transfer(m[1], m[0], 51)}, {3}, 0);
  run({adjust(m[2], 1, 1)}, {3}, 0);
  run({transfer(m[0], m[3], 1)}, {4}, 0);
  run({adjust(m[3], 1, 0)}, {4}, 0);
  run({write(m[0], 2 * K + A + 3, {7, 7, 7}, &stale)}, {5}, 0);
  // ... and together, around steps that apply: 0-, 1- and 2-update steps side by side, and a step behind a skipped overdraft sees the balance without it
  run({adjust(m[2], 5, 0), transfer(gone, m[0], 1), transfer(m[2], m[0], 5), transfer(m[0], gone, 1), adjust(m[2], 1, 1), write(m[1], 2 * K + A, {4}),
       adjust(m[3], 1, 0), write(m[1], 2 * K + A, {5}, &one), transfer(m[0], m[1], 105), transfer(m[0], m[1], 106)},
      {0, 1, 0, 2, 3, 0, 4, 5, 0, 3}, 6);
  // a write over the balance, then a transfer that spends what those bytes spell (m[2] had 0)
  run({write(m[2], 2 * K, balance_bytes_of(300)), transfer(m[2], m[1], 300), transfer(m[2], m[1], 1)}, {0, 0, 3}, 3);
  // a compare-and-set on the balance bytes that only an earlier adjust of the block satisfies ...
  {
    const std::vector<uint8_t> after = balance_bytes_of(57);
    run({write(m[1], 2 * K, balance_bytes_of(0), &after), adjust(m[1], 7, 0), write(m[1], 2 * K, balance_bytes_of(1), &after)}, {5, 0, 0}, 2);
  }
  // ... and one that an earlier transfer has broken (m[0] has 100 before the block)
  {
    const std::vector<uint8_t> before = balance_bytes_of(100);
    run({write(m[0], 2 * K, balance_bytes_of(100), &before), transfer(m[0], m[1], 30), write(m[0], 2 * K, balance_bytes_of(5), &before)}, {0, 0, 5}, 3);
  }
  // a key in many steps across all kinds
  run({adjust(m[0], 10, 0), write(m[0], 2 * K + A + 1, {1, 2}), transfer(m[0], m[1], 110), write(m[0], 2 * K + 1, {9}), adjust(m[0], 9, 1), adjust(m[0], 1, 1)},
      {0, 0, 0, 0, 0, 3}, 6);
  // windows of 1, 16, 17 and 39 bytes, each beside a money-only key of one unit: the slots' first units are a prefix sum of different unit counts
  for (uint32_t wb : {1u, 16u, 17u, 39u}) {
    std::vector<uint8_t> v(wb, (uint8_t)wb);
    std::vector<Step> steps = {adjust(m[0], 1, 0), write(m[1], 2 * K + A + 2, v), adjust(m[2], 1, 0), write(m[3], length - wb, v)};
    run(steps, {0, 0, 0, 0}, 4);
  }
  printf("ok c %u\n", blocks);
}

void layout_case(uint32_t max_updates, size_t max_src, uint32_t length, size_t rowb, uint32_t depth, uint32_t ncuts, size_t stage) {
  std::unique_ptr<uint32_t[]> cuts(new uint32_t[ncuts + 1]);
  for (uint32_t g = 0; g < ncuts; g++) cuts[g] = g + 1;
  const BlockLayout s = block_layout(max_updates, max_src, length, rowb, depth, ncuts, ncuts ? cuts.get() : nullptr, stage);
  const size_t pitch = ((size_t)length + 15) / 16 * 16;
  CHECK(s.fresh_bytes == (size_t)max_updates * pitch);
  CHECK(s.desc_bytes == (size_t)max_updates * 16);
  CHECK(s.src_bytes == max_src);
  CHECK(s.up_bytes() == (size_t)max_updates * 16 + max_src);
  CHECK(s.skip == ((size_t)max_updates * pitch + (size_t)max_updates * 16 + max_src + 15) / 16 * 16);
  size_t upper = 0;  // one MerkleSegment row an upper segment: 128 bytes, 32 a level, the index bytes
  for (uint32_t g = 0; g < ncuts; g++) {
    const uint32_t levels = (g + 1 < ncuts ? g + 2 : depth) - (g + 1);
    upper += 128 + (size_t)32 * levels + (levels + 7) / 8;
  }
  size_t fit = stage / (rowb + upper);
  if (fit < 1) fit = 1;
  if (fit > max_updates) fit = max_updates;
  CHECK(s.ch == fit && s.rowb == rowb);
  printf("ok l %u %zu %zu\n", s.ch, s.skip, s.up_bytes());
}

}  // namespace

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    unsigned long long a[7];
    char kind = 0;
    const int got = sscanf(line, " %c %llu %llu %llu %llu %llu %llu %llu", &kind, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]);
    if (kind == 'r' && got == 5 && a[0] >= 1 && a[0] <= 256 && a[1] >= 2 && a[1] <= 64 && a[2] >= 1 && a[2] <= 4096) random_case((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], a[3]);
    else if (kind == 'c' && got == 2) crafted_case(a[0]);
    else if (kind == 'l' && got == 8 && a[0] >= 1 && a[2] >= 1 && a[2] <= (1u << 20) && a[3] >= 1 && a[4] >= 1 && a[4] <= 24 && a[5] < a[4] && a[6] >= 1)
      layout_case((uint32_t)a[0], (size_t)a[1], (uint32_t)a[2], (size_t)a[3], (uint32_t)a[4], (uint32_t)a[5], (size_t)a[6]);
    else return 2;
  }
  return 0;
}
