// The batch prover's plan header (csrc/batch_plan.hpp) as a program of its own (tests/test_batch_plan_host_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it).
//   row_chunks   every nrows in 1 .. 2^18 + 1 and 2 x 131 071, 2^20, 2^21 + 1; unit 128, 256; limit_rows 131 071, 256, 300, 1000, 4096 and what the GPU tests hand to
//                set_mm_chunk_rows (500, 512, 1024; 0 = 131 071); min_chunks 1, 2.  rpc is a multiple of the unit and at most the limit rounded down to whole units (at
//                least one unit), the chunks cover the rows, none is empty, and the result equals the rule written out step by step here.  Pinned at unit 256, limit
//                131 071 (by hand from the rule): 130 816 rows -> 1 chunk; 130 817 -> 2 x 65 536; 131 072 -> 2 x 65 536; 262 142 -> 3 x 87 552.
//   row_share    total 1, 7, 32 768, 129 536, 2^20, 2^32 - 1; world 1 .. 16: the shares tile [0, total) in order without a gap and differ by at most one.
//   CtGeom       (n, logq) = (1470, 736), (1470, 1472), m = 129 536 against the literal expressions.
//   smudge_term  against unsigned __int128 products: maglen 0, 1, 3, 4, 5, 8, 4 KW - 4; all-0xff and random magnitudes; both KW.
//   batch_route  the default instance (d 32 768, m 129 536, n 1470, logq 736) with room for the image: 31 statements regenerate (SG 248); 32 and 255 stream (SG 255, one
//                super-group, no streamed witness pass); 256 .. 2040 give 2 .. 8 super-groups and the streamed witness pass; 2041 gives 9 and none; public inputs, an SSP
//                that is not dense, batch_witness 0, batch_bw_merged 0 and !mms_ssp_ok each alone switch the pass off and nothing else; batch_slabs 3 gives 3 slabs, one
//                area per super-group, no pass; an image above 3/4 of the memory gives ceil(image / max(avail / 3, 1 GiB)) slabs, at most 256; so little memory that the
//                areas do not fit gives sub-calls of maxsg super-groups; a row length that is no multiple of 8 never streams.
// Argument "spoil": the restated chunk rule rounds the limit UP to whole units; the program must then fail (status 1).  Prints "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "batch_plan.hpp"

static unsigned long checks = 0;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

static int check_row_chunks(bool spoil) {
  const uint32_t units[] = {128, 256}, limits[] = {131071, 256, 300, 1000, 4096, 500, 512, 1024};
  std::vector<uint32_t> rows;
  for (uint32_t r = 1; r <= (1u << 18) + 1; r++) rows.push_back(r);
  rows.push_back(2 * 131071), rows.push_back(1u << 20), rows.push_back((1u << 21) + 1);
  for (uint32_t unit : units)
    for (uint32_t limit : limits)
      for (uint32_t mc = 1; mc <= 2; mc++)
        for (uint32_t nrows : rows) {
          const mf::RowChunks ch = mf::row_chunks(nrows, unit, limit, mc);
          checks++;
          uint32_t lim = limit / unit * unit;  // whole units, rounded down
          if (lim < unit) lim = unit;
          if (!ch.nchunks || !ch.rpc || ch.rpc % unit || ch.rpc > lim || (uint64_t)ch.nchunks * ch.rpc < nrows || (uint64_t)(ch.nchunks - 1) * ch.rpc >= nrows ||
              ch.rpad != (uint64_t)ch.nchunks * ch.rpc)
            FAIL("row_chunks(%u, %u, %u, %u) = {%u, %u, %u} breaks an invariant", nrows, unit, limit, mc, ch.nchunks, ch.rpc, ch.rpad);
          // the rule, step by step
          uint32_t rlim = spoil ? (limit + unit - 1) / unit * unit : lim;
          uint32_t k = nrows / rlim + (nrows % rlim ? 1 : 0);
          if (k < mc) k = mc;
          uint32_t per = nrows / k + (nrows % k ? 1 : 0);
          uint32_t rpc = (per / unit + (per % unit ? 1 : 0)) * unit;
          uint32_t nchunks = nrows / rpc + (nrows % rpc ? 1 : 0);
          if (ch.nchunks != nchunks || ch.rpc != rpc || ch.rpad != nchunks * rpc)
            FAIL("row_chunks differs from the rule: (%u, %u, %u, %u) = {%u, %u, %u}, the steps give {%u, %u, %u}", nrows, unit, limit, mc, ch.nchunks, ch.rpc, ch.rpad,
                 nchunks, rpc, nchunks * rpc);
        }
  const struct { uint32_t nrows, nchunks, rpc; } pins[] = {{130816, 1, 130816}, {130817, 2, 65536}, {131072, 2, 65536}, {262142, 3, 87552}};
  for (const auto &p : pins) {
    const mf::RowChunks ch = mf::row_chunks(p.nrows, 256, 131071);
    checks++;
    if (ch.nchunks != p.nchunks || ch.rpc != p.rpc) FAIL("row_chunks(%u, 256, 131071) = {%u, %u}, pinned {%u, %u}", p.nrows, ch.nchunks, ch.rpc, p.nchunks, p.rpc);
  }
  return 0;
}

static int check_row_share() {
  const uint64_t totals[] = {1, 7, 32768, 129536, 1u << 20, 0xffffffffull};
  for (uint64_t total : totals)
    for (uint32_t world = 1; world <= 16; world++) {
      uint64_t at = 0, lo_cnt = ~0ull, hi_cnt = 0;
      for (uint32_t rank = 0; rank < world; rank++) {
        const mf::Share s = mf::row_share(total, rank, world);
        checks++;
        if (s.lo != at) FAIL("row_share(%llu, %u, %u): starts at %llu, the previous share ends at %llu", (unsigned long long)total, rank, world, (unsigned long long)s.lo, (unsigned long long)at);
        at += s.cnt;
        if (s.cnt < lo_cnt) lo_cnt = s.cnt;
        if (s.cnt > hi_cnt) hi_cnt = s.cnt;
      }
      if (at != total || hi_cnt - lo_cnt > 1) FAIL("row_share(%llu, ., %u): covers %llu, sizes %llu .. %llu", (unsigned long long)total, world, (unsigned long long)at, (unsigned long long)lo_cnt, (unsigned long long)hi_cnt);
    }
  return 0;
}

static int check_geom() {
  const uint32_t n = 1470, m = 129536;
  for (uint32_t logq : {736u, 1472u}) {
    const mf::CtGeom g(n, logq, m);
    checks++;
    const bool q = logq == 736;
    if (g.ctb != (q ? 92u : 184u) || g.L != (q ? 12u : 23u) || g.KW != (q ? 22u : 46u) || g.ctl != (size_t)1471 * (q ? 12 : 23) || g.pstride != (uint64_t)5 * 1471 * (q ? 12 : 23) ||
        g.ctr_ct != (uint64_t)1470 * (q ? 92 : 184) || g.bstride != 16192)
      FAIL("CtGeom(%u, %u, %u) differs from the literal sizes", n, logq, m);
    if (g.ctb != logq / 8 || g.L != (logq + 63) / 64 || g.KW != 2 * (logq / 64) || g.ctl != (size_t)(n + 1) * ((logq + 63) / 64) || g.pstride != 5 * g.ctl ||
        g.ctr_ct != (uint64_t)(logq / 8) * n || g.bstride != (m + 6) / 8)
      FAIL("CtGeom(%u, %u, %u) differs from the expressions", n, logq, m);
  }
  return 0;
}

static int check_smudge() {
  uint64_t lcg = 0x9e3779b97f4a7c15ull;
  for (uint32_t KW : {22u, 46u}) {
    const size_t lens[] = {0, 1, 3, 4, 5, 8, (size_t)4 * KW - 4};
    for (size_t maglen : lens)
      for (int kind = 0; kind < 4; kind++) {  // all 0xff, then three random magnitudes
        std::vector<uint8_t> mag(maglen);  // (exactly maglen bytes: a read past them is the sanitizer's to report)
        for (auto &b : mag) {
          lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
          b = kind ? (uint8_t)(lcg >> 56) : 0xff;
        }
        std::vector<uint32_t> out(KW, 0xdeadbeefu);
        mf::smudge_term(mag.data(), maglen, KW, out.data());
        checks++;
        // u p by 128-bit steps over 64-bit limbs of u, compared word by word
        unsigned __int128 carry = 0;
        for (uint32_t l2 = 0; l2 < KW / 2; l2++) {
          uint64_t u = 0;
          for (size_t j = 0; j < 8; j++)
            if ((size_t)l2 * 8 + j < maglen) u |= (uint64_t)mag[(size_t)l2 * 8 + j] << (8 * j);
          const unsigned __int128 t = (unsigned __int128)u * 4294967291u + carry;
          if (out[2 * l2] != (uint32_t)t || out[2 * l2 + 1] != (uint32_t)(t >> 32)) FAIL("smudge_term(maglen %zu, KW %u, kind %d) differs at word %u", maglen, KW, kind, 2 * l2);
          carry = t >> 64;
        }
        if (carry) FAIL("smudge_term(maglen %zu, KW %u): the product leaves the KW words", maglen, KW);
      }
  }
  return 0;
}

static mf::BatchRouteIn default_in(uint32_t nproofs) {
  mf::BatchRouteIn in{};
  in.nproofs = nproofs, in.d = 32768, in.m = 129536, in.n = 1470, in.logq = 736;
  in.has_mm_image = false, in.batch_image = true, in.batch_slabs = 0;
  in.batch_witness = in.batch_bw_merged = in.ssp_dense = in.mms_ssp_ok = true, in.has_pub = false;
  in.image_bytes = (uint64_t)27 << 30, in.avail = (uint64_t)250 << 30, in.mem_ok = true;  // room for the image
  in.BG = 31, in.BSG = 255, in.BSG_REGEN = 248;
  return in;
}
static bool same_but_try_ws(const mf::BatchRoute &a, const mf::BatchRoute &b) {
  return a.will_stream == b.will_stream && a.SG == b.SG && a.nsg == b.nsg && a.slabs_ok == b.slabs_ok && a.nsl == b.nsl && a.sub_sg == b.sub_sg && a.nbuf == b.nbuf;
}

static int check_route() {
  {
    const mf::BatchRoute r = mf::batch_route(default_in(31));
    checks++;
    if (r.will_stream || r.slabs_ok || r.SG != 248 || r.nsg != 1 || r.nsl != 1 || r.sub_sg || r.nbuf != 2 || r.try_ws) FAIL("batch_route: 31 statements do not regenerate");
  }
  for (uint32_t np = 32; np <= 2041; np++) {
    const mf::BatchRoute r = mf::batch_route(default_in(np));
    checks++;
    const uint32_t nsg = (np + 254) / 255;
    if (!r.will_stream || !r.slabs_ok || r.SG != 255 || r.nsg != nsg || r.nsl != 1 || r.sub_sg || r.nbuf != 2) FAIL("batch_route: %u statements: SG %u nsg %u nsl %u", np, r.SG, r.nsg, r.nsl);
    if (r.try_ws != (nsg >= 2 && nsg <= 8)) FAIL("batch_route: %u statements (%u super-groups): try_ws %d", np, nsg, (int)r.try_ws);
    if ((np == 32 || np == 255) && (r.nsg != 1 || r.try_ws)) FAIL("batch_route: %u statements are one super-group without the streamed pass", np);
    if (np == 256 && (r.nsg != 2 || !r.try_ws)) FAIL("batch_route: 256 statements");
    if (np == 2040 && (r.nsg != 8 || !r.try_ws)) FAIL("batch_route: 2040 statements");
    if (np == 2041 && (r.nsg != 9 || r.try_ws)) FAIL("batch_route: 2041 statements");
  }
  {  // each switch alone turns the streamed pass off and nothing else
    const mf::BatchRoute base = mf::batch_route(default_in(765));
    if (!base.try_ws || base.nsg != 3) FAIL("batch_route: 765 statements take the streamed pass");
    for (int sw = 0; sw < 5; sw++) {
      mf::BatchRouteIn in = default_in(765);
      if (sw == 0) in.has_pub = true;
      if (sw == 1) in.ssp_dense = false;
      if (sw == 2) in.batch_witness = false;
      if (sw == 3) in.batch_bw_merged = false;
      if (sw == 4) in.mms_ssp_ok = false;
      const mf::BatchRoute r = mf::batch_route(in);
      checks++;
      if (r.try_ws || !same_but_try_ws(r, base)) FAIL("batch_route: switch %d does not turn off the streamed pass alone", sw);
    }
    // a registered image streams as well, with nothing to slab
    mf::BatchRouteIn in = default_in(765);
    in.has_mm_image = true;
    const mf::BatchRoute r = mf::batch_route(in);
    checks++;
    if (!r.will_stream || r.slabs_ok || r.SG != 255 || r.nsl != 1 || !r.try_ws) FAIL("batch_route: a registered image");
    in.nproofs = 20;  // ... whatever the statement count
    if (!mf::batch_route(in).will_stream || mf::batch_route(in).SG != 255) FAIL("batch_route: a registered image, 20 statements");
  }
  {
    mf::BatchRouteIn in = default_in(765);
    in.batch_slabs = 3;
    const mf::BatchRoute r = mf::batch_route(in);
    checks++;
    if (r.nsl != 3 || r.nbuf != r.nsg || r.nsg != 3 || r.try_ws || r.sub_sg) FAIL("batch_route: batch_slabs 3: nsl %u nbuf %u", r.nsl, r.nbuf);
    in.batch_slabs = 1000, in.d = 256, in.m = 10;  // capped at min(d, m)
    checks++;
    if (mf::batch_route(in).nsl != 10) FAIL("batch_route: forced slabs are capped at min(d, m)");
    in = default_in(20), in.batch_slabs = 3;  // one group: no image, no slabs
    checks++;
    if (mf::batch_route(in).nsl != 1 || mf::batch_route(in).nbuf != 2) FAIL("batch_route: forced slabs without an image to slab");
  }
  {  // the image does not fit
    const uint64_t GiB = (uint64_t)1 << 30;
    const struct { uint64_t image, avail; uint32_t nsl; } cases[] = {
        {363 * GiB, 250 * GiB, 5},      // ceil(363 / 83.33)
        {200 * GiB, 250 * GiB, 3},      // above 187.5 = 3/4 of 250
        {187 * GiB, 250 * GiB, 1},      // fits
        {8 * GiB, 2 * GiB, 8},          // budget = max(avail / 3, 1 GiB) = 1 GiB
        {1000 * GiB, 2 * GiB, 256}};    // capped
    for (const auto &k : cases) {
      mf::BatchRouteIn in = default_in(300);
      in.image_bytes = k.image, in.avail = k.avail;
      const mf::BatchRoute r = mf::batch_route(in);
      checks++;
      const uint64_t budget = k.avail / 3 > GiB ? k.avail / 3 : GiB;
      uint64_t want = k.image > k.avail / 4 * 3 ? (k.image + budget - 1) / budget : 1;
      if (want > 256) want = 256;
      if (r.nsl != k.nsl || r.nsl != want) FAIL("batch_route: image %llu GiB, avail %llu GiB: nsl %u, expected %u", (unsigned long long)(k.image / GiB), (unsigned long long)(k.avail / GiB), r.nsl, k.nsl);
      if (r.nbuf != (r.nsl > 1 ? r.nsg : 2u) || (r.nsl > 1 && r.try_ws)) FAIL("batch_route: slabs by memory: nbuf %u", r.nbuf);
    }
    mf::BatchRouteIn in = default_in(300);
    in.image_bytes = 363 * GiB, in.mem_ok = false;  // the memory could not be asked: no slabs
    checks++;
    if (mf::batch_route(in).nsl != 1) FAIL("batch_route: !mem_ok");
    // so little memory that the w | h | v areas of all super-groups do not fit in a quarter of it: area = 3 x 255 x d x 4 bytes
    in = default_in(255 * 40);
    in.image_bytes = 363 * GiB, in.avail = 4 * 10 * ((uint64_t)3 * 255 * 32768 * 4) + 12345;  // maxsg = 10 < nsg = 40
    const mf::BatchRoute r = mf::batch_route(in);
    checks++;
    if (r.nsg != 40 || r.sub_sg != 10) FAIL("batch_route: sub-calls: nsg %u sub_sg %u", r.nsg, r.sub_sg);
    in.nproofs = 255 * 10;  // the areas fit: none
    checks++;
    if (mf::batch_route(in).sub_sg != 0 || mf::batch_route(in).nsl < 2) FAIL("batch_route: no sub-calls when the areas fit");
    in.nproofs = 255 * 40, in.avail = 1000;  // maxsg is at least 1
    checks++;
    if (mf::batch_route(in).sub_sg != 1) FAIL("batch_route: sub-calls of at least one super-group");
  }
  for (uint32_t np : {32u, 300u, 2041u}) {  // n * logq / 8 is no multiple of 8: never a transient image
    mf::BatchRouteIn in = default_in(np);
    in.n = 1471;  // 1471 x 92
    const mf::BatchRoute r = mf::batch_route(in);
    checks++;
    if (r.will_stream || r.slabs_ok || r.SG != 248 || r.nsl != 1 || r.try_ws || mf::batch_transient(false, true, np, 31, 1471, 736)) FAIL("batch_route: an unaligned row length streams");
    in.batch_slabs = 3;
    if (mf::batch_route(in).nsl != 1) FAIL("batch_route: an unaligned row length takes slabs");
  }
  return 0;
}

int main(int argc, char **argv) {
  const bool spoil = argc > 1 && !strcmp(argv[1], "spoil");
  if (check_row_chunks(spoil) || check_row_share() || check_geom() || check_smudge() || check_route()) return 1;
  printf("ok %lu\n", checks);
  return 0;
}
