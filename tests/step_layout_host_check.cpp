// step_layout_host_check.cpp -- a program with its own main: mf::step_layout (csrc/merkle_rows.hpp), the front of the device scratch and the chunk of a batch
// of nk steps of R record updates each, against the formulas the key calls used before they shared it, written out here literally:
//   R = 2  the key steps (insert, remove, transfer): fresh = 2 nk pitch | plan = 12 nk | keys = nk K | payloads = nk P; the chunk is twice the steps whose
//          row and two MerkleSegment rows an upper segment fit the stage
//   R = 1  adjust and write: fresh = nk pitch | plan = 4 nk | payloads = nk P (the balances, the values), no keys; the chunk is the steps whose row and one
//          MerkleSegment row an upper segment fit the stage
// over nk in {1, 2, 1020, 4097}, length in {9, 16, 23, 55, 64}, K in {1, 4, 32} with 2 K <= length, payloads of 0, 1, 8 and 39 bytes, uncut and cut, at depths
// 1, 10 and 24, and a stage that holds many rows, a few, and less than one.  Prints "ok <cases>" and exits 0, or says what differs and exits 1.
#include <stdio.h>

#include <vector>

#include "merkle_rows.hpp"

namespace {

int failures = 0;

void differ(const char *what, uint32_t R, uint32_t nk, uint32_t length, uint32_t K, size_t P, uint32_t depth, uint32_t ncuts, size_t got, size_t want) {
  if (got == want) return;
  if (failures++ < 20) printf("R=%u nk=%u length=%u K=%u P=%zu depth=%u ncuts=%u: %s is %zu, the formula gives %zu\n", R, nk, length, K, P, depth, ncuts, what, got, want);
}

// the bytes of the upper segments' rows of one update as the caller gets them: a MerkleSegment row of v levels is 64 + 64 + 32 v + ceil(v / 8) bytes
size_t upper_rows(uint32_t depth, const std::vector<uint32_t> &cuts) {
  size_t bytes = 0;
  for (size_t g = 0; g < cuts.size(); g++) {
    const uint32_t levels = (g + 1 < cuts.size() ? cuts[g + 1] : depth) - cuts[g];
    bytes += 128 + (size_t)32 * levels + (levels + 7) / 8;
  }
  return bytes;
}

// the most rows of rowb bytes that fit the stage, at least one and at most n
uint32_t fit(uint32_t n, size_t rowb, size_t stage) {
  const size_t f = stage / rowb;
  return (uint32_t)(f < 1 ? 1 : f < n ? f : n);
}

}  // namespace

int main() {
  const uint32_t nks[] = {1, 2, 1020, 4097}, lengths[] = {9, 16, 23, 55, 64}, Ks[] = {1, 4, 32}, depths[] = {1, 10, 24};
  const size_t pays[] = {0, 1, 8, 39}, stages[] = {(size_t)64 << 20, (size_t)1 << 14, 100};
  size_t cases = 0;
  for (uint32_t depth : depths) {
    std::vector<std::vector<uint32_t>> cut_sets = {{}};  // uncut, then the cuts that depth has room for
    if (depth > 1) cut_sets.push_back({depth / 2});
    if (depth > 3) cut_sets.push_back({1, depth / 2, depth - 1});
    for (const auto &cuts : cut_sets)
      for (uint32_t nk : nks)
        for (uint32_t length : lengths)
          for (uint32_t K : Ks) {
            if (2 * K > length) continue;
            for (size_t P : pays)
              for (size_t stage : stages) {
                const uint32_t ncuts = (uint32_t)cuts.size(), d0 = ncuts ? cuts[0] : depth;
                const size_t pitch = ((size_t)length + 15) & ~(size_t)15, up = upper_rows(depth, cuts);
                {  // a key step: the remove's row, two records and two tails behind 64 (cut: 128) zero bytes and the key
                  const size_t rowb = (ncuts ? 128 : 64) + K + (size_t)2 * length + (size_t)64 * d0 + (2 * d0 + 7) / 8;
                  const mf::StepLayout s = mf::step_layout(2, 3, nk, length, K, P, rowb, depth, ncuts, cuts.data(), stage);
                  const size_t fresh = (size_t)2 * nk * pitch, plan = (size_t)nk * 3 * 4, keys = (size_t)nk * K, pay = (size_t)nk * P;
                  differ("fresh_bytes", 2, nk, length, K, P, depth, ncuts, s.fresh_bytes, fresh);
                  differ("plan_bytes", 2, nk, length, K, P, depth, ncuts, s.plan_bytes, plan);
                  differ("keys_bytes", 2, nk, length, K, P, depth, ncuts, s.keys_bytes, keys);
                  differ("pay_bytes", 2, nk, length, K, P, depth, ncuts, s.pay_bytes, pay);
                  differ("up_bytes", 2, nk, length, K, P, depth, ncuts, s.up_bytes(), plan + keys + pay);
                  differ("skip", 2, nk, length, K, P, depth, ncuts, s.skip, (fresh + plan + keys + pay + 15) & ~(size_t)15);
                  differ("ch", 2, nk, length, K, P, depth, ncuts, s.ch, 2 * fit(nk, rowb + (ncuts ? 2 * up : 0), stage));
                  differ("pair_chunk", 2, nk, length, K, P, depth, ncuts, s.ch, mf::pair_chunk(nk, rowb + 2 * up, stage));
                  differ("rowb", 2, nk, length, K, P, depth, ncuts, s.rowb, rowb);
                  differ("R", 2, nk, length, K, P, depth, ncuts, s.R, 2);
                }
                {  // a one-record step: the write's row, one record and one tail behind 64 zero bytes, the key and the P public bytes
                  const size_t rowb = 64 + K + P + length + (size_t)32 * d0 + (d0 + 7) / 8;
                  const mf::StepLayout s = mf::step_layout(1, 1, nk, length, 0, P, rowb, depth, ncuts, cuts.data(), stage);
                  const size_t fresh = (size_t)nk * pitch, plan = (size_t)nk * 4, pay = (size_t)nk * P;
                  differ("fresh_bytes", 1, nk, length, K, P, depth, ncuts, s.fresh_bytes, fresh);
                  differ("plan_bytes", 1, nk, length, K, P, depth, ncuts, s.plan_bytes, plan);
                  differ("keys_bytes", 1, nk, length, K, P, depth, ncuts, s.keys_bytes, 0);
                  differ("pay_bytes", 1, nk, length, K, P, depth, ncuts, s.pay_bytes, pay);
                  differ("up_bytes", 1, nk, length, K, P, depth, ncuts, s.up_bytes(), plan + pay);
                  differ("skip", 1, nk, length, K, P, depth, ncuts, s.skip, (fresh + plan + pay + 15) & ~(size_t)15);
                  differ("ch", 1, nk, length, K, P, depth, ncuts, s.ch, fit(nk, rowb + (ncuts ? up : 0), stage));
                  differ("rowb", 1, nk, length, K, P, depth, ncuts, s.rowb, rowb);
                  differ("R", 1, nk, length, K, P, depth, ncuts, s.R, 1);
                }
                cases++;
              }
          }
  }
  if (failures) {
    printf("%d differences\n", failures);
    return 1;
  }
  printf("ok %zu\n", cases);
  return 0;
}
