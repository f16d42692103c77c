// batch_plan.hpp -- plain C++ shared by the host side of snark.hip, evalmm.hip, mfhip.hip, witness.hip and a host check (tests/batch_plan_host_check.cpp): the arithmetic
// a batch call (mfh_prove_batch and the row-sharded sequence) and the row GEMM rest on, each rule written once.
//
//   row_chunks   how a launch cuts its rows into chunks that fit an int32 accumulator (mfh_set_mm_chunk_rows)
//   row_share    a rank's contiguous share of a region's rows: what the image writer, the image readers and the row slabs cut alike
//   CtGeom       the sizes of a ciphertext and of a proof struct, from (n, logq, m)
//   smudge_term  u p of one smudging draw (ct_smudge, src/lwe.c:65-76)
//   batch_route  everything mfh_prove_batch decides before it queues anything: image or keystream, super-groups, row slabs, sub-calls, the streamed witness pass
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace mf {

constexpr uint64_t plan_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
constexpr uint64_t plan_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
constexpr uint64_t plan_ceil(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// nrows > 0 rows in `nchunks` chunks of `rpc` rows, rpc a multiple of `unit` (the kernels' row stage) and at most limit_rows rounded DOWN to whole units (rounding a
// chunk of <= 131 071 rows up to a unit afterwards could reach 131 072: 2 x 131 071 rows are three chunks); never fewer than min_chunks chunks asked for, and no
// empty chunk.  rpad = nchunks * rpc: digit rows past nrows are zero.  Launches that share digit fragments (b_w and the streamed witness pass of a batch call) share
// (nrows, unit, limit_rows) and therefore the chunks.
struct RowChunks { uint32_t nchunks, rpc, rpad; };
constexpr RowChunks row_chunks(uint32_t nrows, uint32_t unit, uint32_t limit_rows, uint32_t min_chunks = 1) {
  if (!nrows) return RowChunks{0, 0, 0};
  const uint64_t lim = plan_max(unit, (uint64_t)limit_rows / unit * unit);
  const uint64_t k = plan_max(min_chunks, plan_ceil(nrows, lim));
  const uint64_t rpc = plan_ceil(plan_ceil(nrows, k), unit) * unit;  // <= lim
  const uint64_t nchunks = plan_ceil(nrows, rpc);
  return RowChunks{(uint32_t)nchunks, (uint32_t)rpc, (uint32_t)(nchunks * rpc)};
}

// rows [lo, lo + cnt) of `total`: rank's share of world (rank < world); the shares tile [0, total) in order and differ by at most one row
struct Share { uint64_t lo, cnt; };
constexpr Share row_share(uint64_t total, uint32_t rank, uint32_t world) {
  const uint64_t lo = total * rank / world;
  return Share{lo, total * ((uint64_t)rank + 1) / world - lo};
}

struct CtGeom {
  uint32_t ctb;      // bytes of a compressed coordinate
  uint32_t L;        // uint64 limbs of a value
  uint32_t KW;       // its 32-bit words below 2^(64 K), K = logq / 64: what the smudging terms and b_w's delta ct_t term span
  size_t ctl;        // limbs of a ciphertext: n + 1 values
  uint64_t pstride;  // limbs of a proof struct (h | hat_h | hat_v | v_w | b_w): component k of consecutive proofs
  uint64_t ctr_ct;   // stream bytes of a CRS row
  uint32_t bstride;  // bytes of a statement's m - 1 witness bits, packed densely
  constexpr CtGeom(uint32_t n, uint32_t logq, uint32_t m)
      : ctb(logq / 8), L((logq + 63) / 64), KW(2 * (logq / 64)), ctl((size_t)(n + 1) * ((logq + 63) / 64)), pstride(5 * ((uint64_t)(n + 1) * ((logq + 63) / 64))),
        ctr_ct((uint64_t)(logq / 8) * n), bstride((m + 6) / 8) {}
};

// out[0 .. KW) = u * p, u = the maglen little-endian bytes at mag, p = 2^32 - 5: schoolbook by 32-bit words (the caller has checked maglen + 4 <= 4 KW: no carry leaves)
constexpr uint32_t PLAN_P = 4294967291u;
inline void smudge_term(const uint8_t *mag, size_t maglen, uint32_t KW, uint32_t *out) {
  uint64_t carry = 0;
  for (uint32_t l = 0; l < KW; l++) {
    uint32_t w = 0;
    const size_t o = (size_t)l * 4;
    if (o < maglen) memcpy(&w, mag + o, maglen - o < 4 ? maglen - o : 4);
    const uint64_t t = (uint64_t)w * PLAN_P + carry;
    out[l] = (uint32_t)t;
    carry = t >> 32;
  }
}

// A call of nproofs statements streams a transient image of its own -- the CRS expanded once into MFMA A-fragment order -- when none is registered, the knob allows it
// (mfh_set_batch_image), more than one group of BG proofs would otherwise regenerate the keystream, and the row length suits the 256-column kernels.
constexpr bool batch_transient(bool has_mm_image, bool batch_image, uint32_t nproofs, uint32_t BG, uint32_t n, uint32_t logq) {
  return !has_mm_image && batch_image && nproofs > BG && (((uint64_t)n * (logq / 8)) & 7) == 0;
}

struct BatchRouteIn {
  uint32_t nproofs, d, m, n, logq;
  bool has_mm_image, batch_image;
  uint32_t batch_slabs;      // mfh_set_batch_slabs: 0 = by memory
  bool batch_witness, batch_bw_merged, has_pub, ssp_dense, mms_ssp_ok;
  uint64_t image_bytes;      // the whole CRS image
  uint64_t avail;            // free device memory + what the context holds and would re-use
  bool mem_ok;               // ... could be asked (looked at only when a transient image is wanted and no slab count is forced)
  uint32_t BG, BSG, BSG_REGEN;
};
struct BatchRoute {
  bool will_stream;  // the row work streams an image (the caller's, or the call's transient one)
  uint32_t SG, nsg;  // statements per super-group: BSG when it streams, BSG_REGEN when every group regenerates the keystream; super-groups of the call
  bool slabs_ok;     // the call would take a transient image: row slabs are possible
  uint32_t nsl;      // row slabs to start with (1: none; the caller may double them when a slab's image does not fit after all)
  uint32_t sub_sg;   // != 0: the w | h | v areas of the whole call would not fit -- sub-calls of sub_sg super-groups
  uint32_t nbuf;     // w | h | v areas: one per super-group with slabs (all chains run first), else two in turn
  bool try_ws;       // the streamed witness pass may be taken, as far as this can be told before the image question is settled (d_ssp != NULL and d % 64 == 0 are the caller's)
};
constexpr BatchRoute batch_route(const BatchRouteIn &in) {
  BatchRoute r{};
  r.slabs_ok = batch_transient(in.has_mm_image, in.batch_image, in.nproofs, in.BG, in.n, in.logq);
  r.will_stream = in.has_mm_image || r.slabs_ok;
  r.SG = r.will_stream ? in.BSG : in.BSG_REGEN;
  r.nsg = (uint32_t)plan_ceil(in.nproofs, r.SG);
  r.nsl = 1;
  if (r.slabs_ok && in.batch_slabs) {
    r.nsl = (uint32_t)plan_min(in.batch_slabs, plan_max(1, plan_min(in.d, in.m)));  // forced (tests, tuning)
  } else if (r.slabs_ok && in.mem_ok && in.image_bytes > in.avail / 4 * 3) {
    const uint64_t budget = plan_max(in.avail / 3, (uint64_t)1 << 30);
    r.nsl = (uint32_t)plan_min(256, plan_ceil(in.image_bytes, budget));
    const uint64_t area = (uint64_t)3 * in.BSG * in.d * 4, maxsg = plan_max(1, in.avail / 4 / area);
    if (r.nsg > maxsg) r.sub_sg = (uint32_t)maxsg;
  }
  r.nbuf = r.nsl > 1 ? r.nsg : 2;
  r.try_ws = in.batch_witness && r.nsl == 1 && r.will_stream && !in.has_pub && in.ssp_dense && in.m >= 2 && r.nsg >= 2 && r.nsg <= 8 && in.batch_bw_merged && in.mms_ssp_ok;
  return r;
}

}  // namespace mf
