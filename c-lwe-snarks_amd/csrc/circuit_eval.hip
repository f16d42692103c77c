// circuit_eval.hip -- mfh_circuit_create / mfh_circuit_assign: the witnesses of a Boolean circuit for a batch of statements, bitsliced on the device.
//
// One workgroup serves a block of 32 statements.  It keeps one uint32 word per wire in LDS, bit j = statement j of the block, so a gate is one word
// operation (^ & | ~) for all 32 statements.  The gates are sorted by level on the host (inputs level 0, a gate one more than its highest operand); the
// workgroup's threads evaluate one level at a time, with a barrier between levels, all levels in one launch (a ripple-carry chain has depth ~ ngates).
// Both transposes go through wave ballots:
//   in:  lanes 0..31 hold 32 input bits of statements 0..31, lanes 32..63 the next 32 bits: ballot t gives wire words of input bits t and t + 32;
//   out: lane l holds the word of wire 64 q + 1 + l: ballot((word >> j) & 1) is bits [64 q, 64 q + 64) of statement j's witness -- 8 output bytes.
// Assertions fold into one holds word per workgroup.
//
// mfh_circuit_create_global makes the second kind of program: k_circuit_eval_global is the same evaluation with the wire words in device memory
// (ctx->circ_state), one column of nw + 1 words per block of 32 statements, read and written by that block's workgroup alone -- so the workgroup barrier
// between levels orders everything, and the wire count is bounded by m - 1 instead of the LDS.  Gate records are 16 bytes {a, b, out, op}.
//
// mfh_circuit_create_ex makes extended programs of either kind (MAJ / SUM3 / CONST / LUT2 gates, equalities between wires): the EX = true instantiations
// of both kernels, with 16-byte records {a, b, c, out | op << 24}.  The EX = false instantiations are the kernels of the two other creates.
//
// mfh_circuit_create_out adds computed public outputs to an extended program: pairs (p, w) of an input wire p whose value is defined as that of wire w.
// The OUT = true instantiations (EX = true only) copy st[w] to st[p] for every pair after the last level, before the assertions and equalities are
// folded and the witness is written: bits [0, lu) of a witness row then carry the computed statement, whatever the caller put at p's input position.
//
// mfh_circuit_create_sum adds weighted-sum gates (MFH_GATE_WSUM): the SUM = true instantiations (EX = true only).  A head is served by one wave, the other
// way round from every other gate: lane j holds STATEMENT j's sum T_j = sum_e (bit j of term e's word) << shift_e as an ordinary integer (T < 2^24), and
// output wire i's word is the ballot of bit i of T over the lanes -- the transposes this file already does at both ends of a launch.  The wave first
// gathers up to 64 terms, one per lane (the term record and its wire word: one memory latency for 64 terms, in LDS or device memory alike), then walks them
// with v_readlane: four register instructions per term, no memory access in the loop, no counter array.  Within a level the heads come first in the gate
// order and go to the waves from the last one down, while the level's one-word gates fill the threads from the first wave up: a level of the SHA-256
// statement (2 - 4 heads, a few hundred cheap gates at most) then has no wave that does both.
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "ctx.hpp"

namespace {

constexpr uint32_t CWG = 512;        // threads per workgroup (8 waves)
constexpr uint32_t CSTMT = 32;       // statements per workgroup (bits of a wire word)
constexpr uint32_t CCHUNK = 8192;    // statements per launch (256 workgroups); longer calls run several chunks
constexpr uint32_t CWORDS = MFH_CIRCUIT_MAX_WIRES + 1;  // LDS wire words: wire 0 (unused) .. MFH_CIRCUIT_MAX_WIRES
// the device-memory kind: a chunk of statements is bounded by bytes (include/mfhip.h, mfh_circuit_assign)
constexpr size_t GPIN_BYTES = (size_t)64 << 20;     // pinned staging per chunk: statements x (in_stride + bits_stride + 1)
constexpr size_t GSTATE_BYTES = (size_t)256 << 20;  // wire state per chunk: blocks x column bytes (at least one column)
constexpr uint32_t GUNROLL = 4;                     // gates in flight per thread and level

// the word of an extended gate (mfh_circuit_create_ex) from its operands' words; op = MFH_GATE_* (LUT2: 16 + tt)
__device__ __forceinline__ uint32_t gate_ex(uint32_t op, uint32_t x, uint32_t y, uint32_t z) {
  if (op >= 16) {
    const uint32_t t0 = 0u - (op & 1), t1 = 0u - ((op >> 1) & 1), t2 = 0u - ((op >> 2) & 1), t3 = 0u - ((op >> 3) & 1);
    return (~x & ~y & t0) | (x & ~y & t1) | (~x & y & t2) | (x & y & t3);
  }
  switch (op) {
    case MFH_GATE_XOR: return x ^ y;
    case MFH_GATE_AND: return x & y;
    case MFH_GATE_OR: return x | y;
    case MFH_GATE_NOT: return ~x;
    case MFH_GATE_MAJ: return (x & y) | (z & (x | y));
    case MFH_GATE_SUM3: return x ^ y ^ z;
    case MFH_GATE_CONST0: return 0u;
    default: return ~0u;  // MFH_GATE_CONST1
  }
}

// One WSUM head, by one whole wave (every argument but lane is wave-uniform): terms[first .. first + nterms) = wire | shift << 24 in non-decreasing shift
// order, output wire i (i < nbits <= 24) = o + i.  Both halves of the wave compute the same 32 sums (j = lane & 31): the term walk is uniform.
__device__ __forceinline__ void wsum_head(uint32_t *st, const uint32_t *__restrict__ terms, uint32_t first, uint32_t nterms, uint32_t nbits, uint32_t o,
                                          uint32_t lane) {
  const uint32_t j = lane & 31;
  uint32_t T = 0;
  uint32_t next = lane < nterms ? terms[first + lane] : 0;  // the term records one gather ahead: their latency hides behind the walk
  for (uint32_t e0 = 0; e0 < nterms; e0 += 64) {
    const uint32_t n = min(64u, nterms - e0), t = next;
    next = e0 + 64 + lane < nterms ? terms[first + e0 + 64 + lane] : 0;
    const uint32_t word = lane < n ? st[t & 0xffffff] : 0, sh = t >> 24;
    for (uint32_t t = 0; t < n; t++) {
      const uint32_t w = __builtin_amdgcn_readlane(word, t), s = __builtin_amdgcn_readlane(sh, t);
      T += ((w >> j) & 1) << s;
    }
  }
  uint32_t mine = 0;
  for (uint32_t i = 0; i < nbits; i++) {
    const uint64_t bm = __ballot((T >> i) & 1);
    if (lane == i) mine = (uint32_t)bm;
  }
  if (lane < nbits) st[o + lane] = mine;
}

// Gate records sorted by level; level L is gates [lp[L], lp[L + 1]).  asserts[e] = {wire, value}.
//   EX = false (mfh_circuit_create):    gates[g] = uint2 {a | b << 16, out | op << 16}, ops XOR / AND / OR / NOT; equal / nequal unused
//   EX = true  (mfh_circuit_create_ex): gates[g] = uint4 {a, b, c, out | op << 24}, every op; equal[e] = {a, b} folds into holds with the assertions
// The extra arguments come last, so the EX = false instantiation is the kernel as it was before extended programs existed, instruction for instruction.
//   OUT = true (mfh_circuit_create_out, nout > 0): outputs[e] = {p, w}: st[p] = st[w] after the last level (no w is a p, every p once: no order among pairs).
// outputs / nout come last again, and the OUT = false instantiations never read them: their code is what it was before outputs existed.
//   SUM = true (mfh_circuit_create_sum with a WSUM gate): heads {first_term, nterms, nbits, out | MFH_GATE_WSUM << 24} are the first records of their
// level, [lp[L], hp[L]); WSUM_BIT records have no device record.  terms / hp come last, and the SUM = false instantiations never read them.
template <bool EX, bool OUT = false, bool SUM = false>
__global__ __launch_bounds__(CWG) void k_circuit_eval(const std::conditional_t<EX, uint4, uint2> *__restrict__ gates, const uint32_t *__restrict__ lp,
                                                      uint32_t nlev, const uint2 *__restrict__ asserts, uint32_t nasserts, uint32_t nin, uint32_t nw,
                                                      const uint8_t *__restrict__ in, size_t in_stride, uint32_t nstmt, uint8_t *__restrict__ out,
                                                      size_t bits_stride, uint8_t *__restrict__ holds, const uint2 *__restrict__ equal, uint32_t nequal,
                                                      const uint2 *__restrict__ outputs, uint32_t nout, const uint32_t *__restrict__ terms,
                                                      const uint32_t *__restrict__ hp) {
  static_assert(EX || !OUT, "outputs belong to extended programs");
  static_assert(EX || !SUM, "weighted sums belong to extended programs");
  __shared__ uint32_t st[CWORDS];
  __shared__ uint32_t hw;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = CWG / 64;
  const uint32_t s0 = blockIdx.x * CSTMT, j = lane & 31;
  const bool live = s0 + j < nstmt;  // the tail block: statements past nstmt read zeros and write nothing
  if (tid == 0) hw = ~0u;

  // ---- inputs: statement rows -> wire words (wire k + 1 = input bit k)
  const uint8_t *row = in + (size_t)(live ? s0 + j : 0) * in_stride;
  for (uint32_t it = wave; it * 64 < nin; it += nwaves) {  // (wave-uniform trip count: every lane takes part in the ballots)
    const uint32_t wd = 2 * it + (lane >> 5);
    uint32_t word = 0;
    if (live)
      for (uint32_t u = 0; u < 4; u++) {
        const size_t byte = (size_t)wd * 4 + u;
        if (byte < in_stride) word |= (uint32_t)row[byte] << (8 * u);
      }
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; t++) {
      const uint64_t bm = __ballot((word >> t) & 1);
      if (j == t) mine = lane < 32 ? (uint32_t)bm : (uint32_t)(bm >> 32);
    }
    const uint32_t k = wd * 32 + j;
    if (k < nin) st[k + 1] = mine;
  }
  __syncthreads();

  // ---- gates, level by level
  uint32_t g1 = nlev ? lp[0] : 0;
  for (uint32_t lv = 0; lv < nlev; lv++) {
    uint32_t g0 = g1;
    g1 = lp[lv + 1];
    if constexpr (SUM) {  // the level's heads, one wave each, from the last wave down
      const uint32_t h1 = hp[lv], uw = __builtin_amdgcn_readfirstlane(nwaves - 1 - wave);
      for (uint32_t h = g0 + uw; h < h1; h += nwaves) {
        const uint4 r = gates[h];
        wsum_head(st, terms, __builtin_amdgcn_readfirstlane(r.x), __builtin_amdgcn_readfirstlane(r.y), __builtin_amdgcn_readfirstlane(r.z),
                  __builtin_amdgcn_readfirstlane(r.w & 0xffffff), lane);
      }
      g0 = h1;
    }
    for (uint32_t g = g0 + tid; g < g1; g += CWG) {
      const auto r = gates[g];
      if constexpr (EX) {
        st[r.w & 0xffffff] = gate_ex(r.w >> 24, st[r.x], st[r.y], st[r.z]);
      } else {
        const uint32_t x = st[r.x & 0xffff], y = st[r.x >> 16], op = r.y >> 16;
        st[r.y & 0xffff] = op == MFH_GATE_XOR ? x ^ y : op == MFH_GATE_AND ? x & y : op == MFH_GATE_OR ? x | y : ~x;
      }
    }
    __syncthreads();
  }

  // ---- computed public outputs: the input wire p takes the value of wire w
  if constexpr (OUT) {
    for (uint32_t e = tid; e < nout; e += CWG) {
      const uint2 o = outputs[e];
      st[o.x] = st[o.y];
    }
    __syncthreads();
  }

  // ---- assertions
  uint32_t ok = ~0u;
  for (uint32_t e = tid; e < nasserts; e += CWG) {
    const uint2 a = asserts[e];
    ok &= a.y ? st[a.x] : ~st[a.x];
  }
  if constexpr (EX)
    for (uint32_t e = tid; e < nequal; e += CWG) {
      const uint2 q = equal[e];
      ok &= ~(st[q.x] ^ st[q.y]);
    }
  if (ok != ~0u) atomicAnd(&hw, ok);

  // ---- outputs: wire words -> statement rows, 8 bytes per statement and group of 64 wires; bytes [0, bits_stride) all written
  const uint32_t nq = (uint32_t)((bits_stride + 7) / 8);
  for (uint32_t q = wave; q < nq; q += nwaves) {
    const uint32_t i = q * 64 + 1 + lane;
    const uint32_t word = i <= nw ? st[i] : 0;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; t++) {
      const uint64_t bm = __ballot((word >> t) & 1);
      if (lane == t) mine = bm;
    }
    if (lane < 32 && live) {
      uint8_t *dst = out + (size_t)(s0 + lane) * bits_stride + (size_t)q * 8;
      const size_t left = bits_stride - (size_t)q * 8;
      if (left >= 8 && ((uintptr_t)dst & 7) == 0) {
        *reinterpret_cast<uint64_t *>(dst) = mine;
      } else {
        for (uint32_t u = 0; u < 8 && u < left; u++) dst[u] = (uint8_t)(mine >> (8 * u));
      }
    }
  }
  __syncthreads();
  if (tid < CSTMT && s0 + tid < nstmt && holds) holds[s0 + tid] = (hw >> tid) & 1;
}

// The kernel above with the wire words in device memory: st = this block's column of colw words (wire i at st[i]), gates[g] = {a, b, out, op}
// (EX: {a, b, c, out | op << 24}, and equal / nequal as above).  A column is read and written by its own workgroup only; __syncthreads() (workgroup-scope
// release / acquire) orders the levels, and the output pass after them.
template <bool EX, bool OUT = false, bool SUM = false>
__global__ __launch_bounds__(CWG) void k_circuit_eval_global(const uint4 *__restrict__ gates, const uint32_t *__restrict__ lp, uint32_t nlev,
                                                             const uint2 *__restrict__ asserts, uint32_t nasserts, uint32_t nin, uint32_t nw,
                                                             uint32_t *state, size_t colw, const uint8_t *__restrict__ in, size_t in_stride, uint32_t nstmt,
                                                             uint8_t *__restrict__ out, size_t bits_stride, uint8_t *__restrict__ holds,
                                                             const uint2 *__restrict__ equal, uint32_t nequal, const uint2 *__restrict__ outputs,
                                                             uint32_t nout, const uint32_t *__restrict__ terms, const uint32_t *__restrict__ hp) {
  static_assert(EX || !OUT, "outputs belong to extended programs");
  static_assert(EX || !SUM, "weighted sums belong to extended programs");
  __shared__ uint32_t hw;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = CWG / 64;
  const uint32_t s0 = blockIdx.x * CSTMT, j = lane & 31;
  const bool live = s0 + j < nstmt;  // the tail block: statements past nstmt read zeros and write nothing
  uint32_t *st = state + (size_t)blockIdx.x * colw;
  if (tid == 0) hw = ~0u;

  // ---- inputs: statement rows -> wire words (wire k + 1 = input bit k)
  const uint8_t *row = in + (size_t)(live ? s0 + j : 0) * in_stride;
  for (uint32_t it = wave; it * 64 < nin; it += nwaves) {  // (wave-uniform trip count: every lane takes part in the ballots)
    const uint32_t wd = 2 * it + (lane >> 5);
    uint32_t word = 0;
    if (live)
      for (uint32_t u = 0; u < 4; u++) {
        const size_t byte = (size_t)wd * 4 + u;
        if (byte < in_stride) word |= (uint32_t)row[byte] << (8 * u);
      }
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; t++) {
      const uint64_t bm = __ballot((word >> t) & 1);
      if (j == t) mine = lane < 32 ? (uint32_t)bm : (uint32_t)(bm >> 32);
    }
    const uint32_t k = wd * 32 + j;
    if (k < nin) st[k + 1] = mine;
  }
  __syncthreads();

  // ---- gates, level by level; GUNROLL gates per thread in flight (no gate of a level reads another's output)
  uint32_t g1 = nlev ? lp[0] : 0;
  for (uint32_t lv = 0; lv < nlev; lv++) {
    uint32_t g0 = g1;
    g1 = lp[lv + 1];
    if constexpr (SUM) {  // the level's heads, one wave each, from the last wave down
      const uint32_t h1 = hp[lv], uw = __builtin_amdgcn_readfirstlane(nwaves - 1 - wave);
      for (uint32_t h = g0 + uw; h < h1; h += nwaves) {
        const uint4 r = gates[h];
        wsum_head(st, terms, __builtin_amdgcn_readfirstlane(r.x), __builtin_amdgcn_readfirstlane(r.y), __builtin_amdgcn_readfirstlane(r.z),
                  __builtin_amdgcn_readfirstlane(r.w & 0xffffff), lane);
      }
      g0 = h1;
    }
    for (uint32_t g = g0 + tid; g < g1; g += GUNROLL * CWG) {
      uint4 r[GUNROLL];
      uint32_t x[GUNROLL], y[GUNROLL], z[GUNROLL];
#pragma unroll
      for (uint32_t u = 0; u < GUNROLL; u++)
        if (g + u * CWG < g1) r[u] = gates[g + u * CWG];
#pragma unroll
      for (uint32_t u = 0; u < GUNROLL; u++)
        if (g + u * CWG < g1) {
          x[u] = st[r[u].x];
          y[u] = st[r[u].y];
          if constexpr (EX) z[u] = st[r[u].z];
        }
#pragma unroll
      for (uint32_t u = 0; u < GUNROLL; u++)
        if (g + u * CWG < g1) {
          if constexpr (EX) {
            st[r[u].w & 0xffffff] = gate_ex(r[u].w >> 24, x[u], y[u], z[u]);
          } else {
            const uint32_t op = r[u].w;
            st[r[u].z] = op == MFH_GATE_XOR ? x[u] ^ y[u] : op == MFH_GATE_AND ? x[u] & y[u] : op == MFH_GATE_OR ? x[u] | y[u] : ~x[u];
          }
        }
    }
    __syncthreads();
  }

  // ---- computed public outputs: the input wire p takes the value of wire w
  if constexpr (OUT) {
    for (uint32_t e = tid; e < nout; e += CWG) {
      const uint2 o = outputs[e];
      st[o.x] = st[o.y];
    }
    __syncthreads();
  }

  // ---- assertions
  uint32_t ok = ~0u;
  for (uint32_t e = tid; e < nasserts; e += CWG) {
    const uint2 a = asserts[e];
    ok &= a.y ? st[a.x] : ~st[a.x];
  }
  if constexpr (EX)
    for (uint32_t e = tid; e < nequal; e += CWG) {
      const uint2 q = equal[e];
      ok &= ~(st[q.x] ^ st[q.y]);
    }
  if (ok != ~0u) atomicAnd(&hw, ok);

  // ---- outputs: wire words -> statement rows, 8 bytes per statement and group of 64 wires; bytes [0, bits_stride) all written
  const uint32_t nq = (uint32_t)((bits_stride + 7) / 8);
  for (uint32_t q = wave; q < nq; q += nwaves) {
    const uint32_t i = q * 64 + 1 + lane;
    const uint32_t word = i <= nw ? st[i] : 0;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; t++) {
      const uint64_t bm = __ballot((word >> t) & 1);
      if (lane == t) mine = bm;
    }
    if (lane < 32 && live) {
      uint8_t *dst = out + (size_t)(s0 + lane) * bits_stride + (size_t)q * 8;
      const size_t left = bits_stride - (size_t)q * 8;
      if (left >= 8 && ((uintptr_t)dst & 7) == 0) {
        *reinterpret_cast<uint64_t *>(dst) = mine;
      } else {
        for (uint32_t u = 0; u < 8 && u < left; u++) dst[u] = (uint8_t)(mine >> (8 * u));
      }
    }
  }
  __syncthreads();
  if (tid < CSTMT && s0 + tid < nstmt && holds) holds[s0 + tid] = (hw >> tid) & 1;
}

}  // namespace

struct mfh_circuit {
  int device = 0;
  bool global = false;  // false: wire state in LDS (k_circuit_eval); true: mfh_circuit_create_global / MFH_CIRCUIT_GLOBAL (k_circuit_eval_global, ctx->circ_state)
  bool ex = false;      // made by mfh_circuit_create_ex: 16-byte {a, b, c, out | op << 24} records and equalities, the EX = true kernels
  uint32_t nin = 0, ngates = 0, nasserts = 0, nequal = 0, nout = 0, nlev = 0;  // nout > 0: mfh_circuit_create_out with outputs, the OUT = true kernels
  bool sum = false;  // mfh_circuit_create_sum with a WSUM gate: the SUM = true kernels (ngates counts the WSUM_BIT records, which have no device record)
  // gates (uint2 or uint4 records, by level) | asserts (uint2) | equal (uint2) | outputs (uint2) | level_ptr (nlev + 1 words) | sum: head_end (nlev words) | terms
  void *mem = nullptr;
  const void *gates = nullptr;
  const uint2 *asserts = nullptr;
  const uint2 *equal = nullptr;
  const uint2 *outputs = nullptr;
  const uint32_t *lp = nullptr;
  const uint32_t *hp = nullptr;     // sum: hp[L] = the end of the heads of level L + 1, which are its first records
  const uint32_t *terms = nullptr;  // sum: wire | shift << 24
};

namespace {

// every kind: validate, level, sort by level, upload.  Records: mfh_circuit_create {a | b << 16, out | op << 16}; mfh_circuit_create_global {a, b, out, op};
// mfh_circuit_create_ex {a, b, c, out | op << 24} in both kinds.  ex programs take 4-word gates (op, a, b, c), the others 3-word (op, a, b).
// h_outputs: nout pairs (p, w) of mfh_circuit_create_out (ex programs only).  wsum: mfh_circuit_create_sum, which alone accepts WSUM / WSUM_BIT records
// and their nterms pairs (wire, shift) in h_terms; a program without a WSUM gate comes out as that of mfh_circuit_create_out.
int circuit_create(mfh_ctx *ctx, const char *name, bool global, bool ex, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts,
                   const uint32_t *h_asserts, uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, mfh_circuit **out,
                   bool wsum = false, uint32_t nterms = 0, const uint32_t *h_terms = nullptr) {
  if (!ctx || !out) return MFH_EINVAL;
  *out = nullptr;
  const std::string fn = std::string(name) + ": ";
  if ((ngates && !h_gates) || (nasserts && !h_asserts)) { ctx->err = fn + "gates / assertions without their array"; return MFH_EINVAL; }
  if (nequal && !h_equal) { ctx->err = fn + "equalities without their array"; return MFH_EINVAL; }
  if (nout && !h_outputs) { ctx->err = fn + "outputs without their array"; return MFH_EINVAL; }
  if (nterms && !h_terms) { ctx->err = fn + "terms without their array"; return MFH_EINVAL; }
  const uint64_t nw = (uint64_t)nin + ngates;
  if (nw > ctx->P.m - 1) { ctx->err = fn + "nin + ngates > m - 1"; return MFH_EINVAL; }
  if (!global && nw > MFH_CIRCUIT_MAX_WIRES) { ctx->err = fn + "nin + ngates > MFH_CIRCUIT_MAX_WIRES (the wire state must fit 128 KiB of LDS)"; return MFH_EINVAL; }
  if (ex && nw >= (1u << 24)) { ctx->err = fn + "nin + ngates >= 2^24 (the records' 24-bit wire field)"; return MFH_EINVAL; }
  const size_t gw = ex ? 4 : 3;  // words per input gate record
  // output pairs (p, w): source[p] = w for an output wire p, else 0.  An output wire has no value until the end of the evaluation, so nothing reads it
  // but its own pair's equality
  std::vector<uint32_t> source(nout ? (size_t)nin + 1 : 0, 0);
  for (uint32_t e = 0; e < nout; e++) {
    const uint32_t p = h_outputs[2 * e], w = h_outputs[2 * e + 1];
    if (p == 0 || p > nin) { ctx->err = fn + "an output wire p that is not an input wire (1 .. nin)"; return MFH_EINVAL; }
    if (w == 0 || w > nw) { ctx->err = fn + "an output's source wire w is 0 or above nin + ngates"; return MFH_EINVAL; }
    if (w == p) { ctx->err = fn + "an output wire defined as itself"; return MFH_EINVAL; }
    if (source[p]) { ctx->err = fn + "an output wire p given twice"; return MFH_EINVAL; }
    source[p] = w;
  }
  for (uint32_t e = 0; e < nout; e++) {
    const uint32_t w = h_outputs[2 * e + 1];
    if (w <= nin && source[w]) { ctx->err = fn + "an output's source wire w is itself an output wire"; return MFH_EINVAL; }
  }
  const auto is_out = [&](uint32_t w) { return nout && w <= nin && source[w] != 0; };
  std::vector<uint32_t> lvl(nw + 1, 0);
  uint32_t nlev = 0, nheads = 0, nbitrec = 0;
  uint32_t run_o = 0, run_n = 0, run_i = 0;  // inside a head's run of WSUM_BIT records: the head's output wire, its nbits, the next i
  for (uint32_t g = 0; g < ngates; g++) {
    const uint32_t *q = h_gates + gw * g;
    const uint32_t op = q[0], a = q[1], b = q[2], o = nin + 1 + g;
    if (!ex) {
      if (op > MFH_GATE_NOT) { ctx->err = fn + "unknown gate op"; return MFH_EINVAL; }
      if (a == 0 || a >= o || b == 0 || b >= o) { ctx->err = fn + "a gate operand is 0 or not below the gate's output wire"; return MFH_EINVAL; }
      lvl[o] = 1 + std::max(lvl[a], op == MFH_GATE_NOT ? lvl[a] : lvl[b]);
      nlev = std::max(nlev, lvl[o]);
      continue;
    }
    const uint32_t c = q[3];
    if (wsum && run_i < run_n) {  // the records after a head
      if (op != MFH_GATE_WSUM_BIT || a != run_i || b != 0 || c != 0) { ctx->err = fn + "a WSUM head not followed by its WSUM_BIT records in order"; return MFH_EINVAL; }
      lvl[o] = lvl[run_o];
      run_i++;
      nbitrec++;
      continue;
    }
    if (wsum && op == MFH_GATE_WSUM_BIT) { ctx->err = fn + "a WSUM_BIT record without a head"; return MFH_EINVAL; }
    if (wsum && op == MFH_GATE_WSUM) {  // (first_term, nterms, nbits) = (a, b, c)
      if (b == 0) { ctx->err = fn + "a WSUM gate with nterms = 0"; return MFH_EINVAL; }
      if ((uint64_t)a + b > nterms) { ctx->err = fn + "a WSUM gate's term range lies outside the term array"; return MFH_EINVAL; }
      if (c > 24) { ctx->err = fn + "a WSUM gate with nbits > 24"; return MFH_EINVAL; }
      uint64_t tmax = 0;
      uint32_t top = 0, prev = 0;
      for (uint32_t e = 0; e < b; e++) {
        const uint32_t w = h_terms[2 * ((size_t)a + e)], sh = h_terms[2 * ((size_t)a + e) + 1];
        if (w == 0 || w >= o) { ctx->err = fn + "a WSUM term wire is 0 or not below the head's output wire"; return MFH_EINVAL; }
        if (is_out(w)) { ctx->err = fn + "a WSUM term reads an output wire"; return MFH_EINVAL; }
        if (sh >= c) { ctx->err = fn + "a WSUM term with shift >= nbits"; return MFH_EINVAL; }
        if (sh < prev) { ctx->err = fn + "WSUM terms not in non-decreasing shift order"; return MFH_EINVAL; }
        prev = sh;
        tmax += (uint64_t)1 << sh;
        top = std::max(top, lvl[w]);
      }
      uint32_t len = 0;
      while (tmax >> len) len++;
      if (len != c) { ctx->err = fn + "a WSUM gate whose nbits is not the bit length of the sum of 2^shift"; return MFH_EINVAL; }
      if ((uint64_t)g + c > ngates) { ctx->err = fn + "a WSUM head not followed by its WSUM_BIT records in order"; return MFH_EINVAL; }
      lvl[o] = 1 + top;
      nlev = std::max(nlev, lvl[o]);
      run_o = o; run_n = c; run_i = 1;
      nheads++;
      continue;
    }
    if ((op > MFH_GATE_CONST1 && op < 16) || op >= 32) { ctx->err = fn + "unknown gate op"; return MFH_EINVAL; }
    if (op == MFH_GATE_CONST0 || op == MFH_GATE_CONST1) {
      if (a | b | c) { ctx->err = fn + "a CONST gate with an operand other than 0"; return MFH_EINVAL; }
      lvl[o] = 1;
    } else {
      const bool three = op == MFH_GATE_MAJ || op == MFH_GATE_SUM3;
      if (a == 0 || a >= o || b == 0 || b >= o || (three && (c == 0 || c >= o))) {
        ctx->err = fn + "a gate operand is 0 or not below the gate's output wire";
        return MFH_EINVAL;
      }
      if (!three && c != 0) { ctx->err = fn + "a one- or two-input gate with a third operand c != 0"; return MFH_EINVAL; }
      if (op == MFH_GATE_NOT && b != a) { ctx->err = fn + "a NOT gate with b != a"; return MFH_EINVAL; }
      if (is_out(a) || is_out(b) || (three && is_out(c))) { ctx->err = fn + "a gate reads an output wire"; return MFH_EINVAL; }
      if (op == MFH_GATE_SUM3) {
        const uint32_t *m = q - gw;  // gate g - 1
        if (g == 0 || m[0] != MFH_GATE_MAJ) { ctx->err = fn + "a SUM3 gate not directly after a MAJ gate"; return MFH_EINVAL; }
        if (m[1] != a || m[2] != b || m[3] != c) { ctx->err = fn + "a SUM3 gate whose operands differ from its MAJ's"; return MFH_EINVAL; }
      }
      lvl[o] = 1 + std::max(std::max(lvl[a], lvl[b]), three ? lvl[c] : 0u);
    }
    nlev = std::max(nlev, lvl[o]);
  }
  if (run_i < run_n) { ctx->err = fn + "a WSUM head not followed by its WSUM_BIT records in order"; return MFH_EINVAL; }
  for (uint32_t e = 0; e < nasserts; e++) {
    const uint32_t w = h_asserts[2 * e], v = h_asserts[2 * e + 1];
    if (w == 0 || w > nw) { ctx->err = fn + "an assertion on wire 0 or above nin + ngates"; return MFH_EINVAL; }
    if (v > 1) { ctx->err = fn + "an assertion value other than 0 / 1"; return MFH_EINVAL; }
    if (is_out(w)) { ctx->err = fn + "an assertion on an output wire"; return MFH_EINVAL; }
  }
  for (uint32_t e = 0; e < nequal; e++) {
    const uint32_t a = h_equal[2 * e], b = h_equal[2 * e + 1];
    if (a == 0 || a > nw || b == 0 || b > nw) { ctx->err = fn + "an equality on wire 0 or above nin + ngates"; return MFH_EINVAL; }
    if (a == b) { ctx->err = fn + "an equality of a wire with itself"; return MFH_EINVAL; }
    if ((is_out(a) && source[a] != b) || (is_out(b) && source[b] != a)) {
      ctx->err = fn + "an equality on an output wire other than its own pair's";
      return MFH_EINVAL;
    }
  }
  // counting sort by level (stable: creation order within a level; with WSUM gates a level's heads come first, and WSUM_BIT records are dropped)
  const bool sum = nheads != 0;
  const auto opof = [&](uint32_t g) { return h_gates[gw * g]; };
  const auto is_head = [&](uint32_t g) { return sum && opof(g) == MFH_GATE_WSUM; };
  const auto is_bit = [&](uint32_t g) { return sum && opof(g) == MFH_GATE_WSUM_BIT; };
  const uint32_t nrec = ngates - nbitrec;  // device records
  std::vector<uint32_t> lp(nlev + 1, 0), hp(sum ? nlev : 0, 0);
  for (uint32_t g = 0; g < ngates; g++) {
    if (is_bit(g)) continue;
    lp[lvl[nin + 1 + g]]++;  // lp[L] = gates of level L (L >= 1) ...
    if (is_head(g)) hp[lvl[nin + 1 + g] - 1]++;  // hp[L] = heads of level L + 1 ...
  }
  for (uint32_t L = 0, acc = 0; L <= nlev; L++) { const uint32_t n = L < nlev ? lp[L + 1] : 0; lp[L] = acc; acc += n; }  // ... then lp[L] = first gate of level L + 1
  for (uint32_t L = 0; sum && L < nlev; L++) hp[L] += lp[L];                                                           // ... and hp[L] = the end of its heads
  const size_t rec = global || ex ? 4 : 2;  // words per device gate record
  const size_t tail_at = rec * nrec + 2 * (size_t)nasserts + 2 * (size_t)nequal + 2 * (size_t)nout + nlev + 1;
  std::vector<uint32_t> host(tail_at + (sum ? (size_t)nlev + nterms : 0));
  {
    std::vector<uint32_t> pos(lp.begin(), lp.end()), cpos(hp.begin(), hp.end());  // next slot of a level: heads from lp[L], the others from hp[L]
    for (uint32_t g = 0; g < ngates; g++) {
      if (is_bit(g)) continue;
      const uint32_t *q = h_gates + gw * g;
      const uint32_t op = q[0], a = q[1], b = op == MFH_GATE_NOT ? a : q[2], o = nin + 1 + g;
      uint32_t *r = &host[rec * (sum && !is_head(g) ? cpos : pos)[lvl[o] - 1]++];
      if (ex) {
        r[0] = a; r[1] = b; r[2] = q[3]; r[3] = o | op << 24;
      } else if (global) {
        r[0] = a; r[1] = b; r[2] = o; r[3] = op;
      } else {
        r[0] = a | b << 16;
        r[1] = o | op << 16;
      }
    }
    std::copy(h_asserts, h_asserts + (size_t)2 * nasserts, host.begin() + rec * nrec);
    std::copy(h_equal, h_equal + (size_t)2 * nequal, host.begin() + rec * nrec + 2 * nasserts);
    std::copy(h_outputs, h_outputs + (size_t)2 * nout, host.begin() + rec * nrec + 2 * nasserts + 2 * nequal);
    std::copy(lp.begin(), lp.end(), host.begin() + rec * nrec + 2 * nasserts + 2 * nequal + 2 * nout);
    if (sum) {
      std::copy(hp.begin(), hp.end(), host.begin() + tail_at);
      for (uint32_t e = 0; e < nterms; e++) host[tail_at + nlev + e] = h_terms[2 * (size_t)e] | h_terms[2 * (size_t)e + 1] << 24;
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  mfh_circuit *c = new mfh_circuit();
  c->device = ctx->device;
  c->global = global;
  c->ex = ex;
  c->nin = nin;
  c->ngates = ngates;
  c->nasserts = nasserts;
  c->nequal = nequal;
  c->nout = nout;
  c->nlev = nlev;
  c->sum = sum;
  if (hipMalloc(&c->mem, host.size() * 4) != hipSuccess) {
    (void)hipGetLastError();
    delete c;
    ctx->err = fn + "no memory for the gate program";
    return MFH_ENOMEM;
  }
  if (hipMemcpy(c->mem, host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(c->mem);
    delete c;
    ctx->err = fn + "upload failed";
    return MFH_EDEVICE;
  }
  c->gates = c->mem;
  c->asserts = (const uint2 *)((const uint32_t *)c->mem + rec * nrec);
  c->equal = c->asserts + nasserts;
  c->outputs = c->equal + nequal;
  c->lp = (const uint32_t *)(c->outputs + nout);
  if (sum) {
    c->hp = (const uint32_t *)c->mem + tail_at;
    c->terms = c->hp + nlev;
  }
  *out = c;
  return MFH_OK;
}

}  // namespace

extern "C" {

int mfh_circuit_create(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                       mfh_circuit **out) {
  return circuit_create(ctx, "mfh_circuit_create", false, false, nin, ngates, h_gates, nasserts, h_asserts, 0, nullptr, 0, nullptr, out);
}

int mfh_circuit_create_global(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                              mfh_circuit **out) {
  return circuit_create(ctx, "mfh_circuit_create_global", true, false, nin, ngates, h_gates, nasserts, h_asserts, 0, nullptr, 0, nullptr, out);
}

int mfh_circuit_create_ex(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                          uint32_t nequal, const uint32_t *h_equal, uint32_t flags, mfh_circuit **out) {
  if (!ctx || !out) return MFH_EINVAL;
  if (flags & ~MFH_CIRCUIT_GLOBAL) {
    *out = nullptr;
    ctx->err = "mfh_circuit_create_ex: unknown flag bits";
    return MFH_EINVAL;
  }
  return circuit_create(ctx, "mfh_circuit_create_ex", (flags & MFH_CIRCUIT_GLOBAL) != 0, true, nin, ngates, h_gates, nasserts, h_asserts, nequal, h_equal,
                        0, nullptr, out);
}

int mfh_circuit_create_out(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                           uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, uint32_t flags, mfh_circuit **out) {
  if (!ctx || !out) return MFH_EINVAL;
  if (flags & ~MFH_CIRCUIT_GLOBAL) {
    *out = nullptr;
    ctx->err = "mfh_circuit_create_out: unknown flag bits";
    return MFH_EINVAL;
  }
  return circuit_create(ctx, "mfh_circuit_create_out", (flags & MFH_CIRCUIT_GLOBAL) != 0, true, nin, ngates, h_gates, nasserts, h_asserts, nequal, h_equal,
                        nout, h_outputs, out);
}

int mfh_circuit_create_sum(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                           uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, uint32_t nterms_total,
                           const uint32_t *h_terms, uint32_t flags, mfh_circuit **out) {
  if (!ctx || !out) return MFH_EINVAL;
  if (flags & ~MFH_CIRCUIT_GLOBAL) {
    *out = nullptr;
    ctx->err = "mfh_circuit_create_sum: unknown flag bits";
    return MFH_EINVAL;
  }
  return circuit_create(ctx, "mfh_circuit_create_sum", (flags & MFH_CIRCUIT_GLOBAL) != 0, true, nin, ngates, h_gates, nasserts, h_asserts, nequal, h_equal,
                        nout, h_outputs, out, true, nterms_total, h_terms);
}

void mfh_circuit_destroy(mfh_circuit *c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->mem) hipFree(c->mem);
  delete c;
}

int mfh_circuit_assign(mfh_ctx *ctx, const mfh_circuit *c, uint32_t nstmt, const uint8_t *h_inputs, size_t in_stride, uint8_t *h_witness_bits,
                       size_t bits_stride, uint8_t *h_holds) {
  if (!ctx || !c) return MFH_EINVAL;
  if (c->device != ctx->device) { ctx->err = "mfh_circuit_assign: the circuit belongs to another device"; return MFH_EINVAL; }
  const uint64_t nw = (uint64_t)c->nin + c->ngates;
  if (in_stride * 8 < c->nin) { ctx->err = "mfh_circuit_assign: in_stride * 8 < nin"; return MFH_EINVAL; }
  if (bits_stride * 8 < nw) { ctx->err = "mfh_circuit_assign: bits_stride * 8 < nin + ngates"; return MFH_EINVAL; }
  if (!nstmt) return MFH_OK;
  if ((in_stride && !h_inputs) || (bits_stride && !h_witness_bits)) { ctx->err = "mfh_circuit_assign: null row buffer"; return MFH_EINVAL; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // statements per launch: the LDS kind CCHUNK; the global kind as many whole blocks as GPIN_BYTES of staging and GSTATE_BYTES of wire state hold (>= 1 block)
  const size_t colw = (nw + 1 + 31) & ~(size_t)31;  // global kind: words per block's column (128-byte aligned columns)
  uint32_t ch = std::min(nstmt, CCHUNK);
  if (c->global) {
    const size_t by_pin = GPIN_BYTES / (in_stride + bits_stride + 1) / CSTMT, by_state = GSTATE_BYTES / (colw * 4);
    const size_t blocks = std::max<size_t>(1, std::min(by_pin, by_state));
    ch = (uint32_t)std::min<size_t>(nstmt, blocks * CSTMT);
  }
  const size_t in_b = (size_t)ch * in_stride, out_b = (size_t)ch * bits_stride, io_b = in_b + out_b + ch;
  if (int rc = buf_reserve(ctx, ctx->circ_io, ctx->circ_io_bytes, io_b)) return rc;
  if (c->global)
    if (int rc = buf_reserve(ctx, ctx->circ_state, ctx->circ_state_bytes, (size_t)(ch + CSTMT - 1) / CSTMT * colw * 4)) return rc;
  uint8_t *pin_in = in_b ? (uint8_t *)pin_acquire(ctx, ctx->pin_rows, in_b) : nullptr;
  uint8_t *pin_out = (uint8_t *)pin_acquire(ctx, ctx->pin_cw, out_b + ch);
  if ((in_b && !pin_in) || !pin_out) return MFH_ENOMEM;
  uint8_t *d_in = (uint8_t *)ctx->circ_io, *d_out = d_in + in_b, *d_holds = d_out + out_b;
  int rc = MFH_OK;
  for (uint32_t b0 = 0; b0 < nstmt && rc == MFH_OK; b0 += ch) {
    const uint32_t n = std::min(ch, nstmt - b0);
    if (in_b) {
      memcpy(pin_in, h_inputs + (size_t)b0 * in_stride, (size_t)n * in_stride);
      if (hipMemcpyAsync(d_in, pin_in, (size_t)n * in_stride, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = MFH_EDEVICE; break; }
    }
    const dim3 grid((n + CSTMT - 1) / CSTMT);
    const uint32_t *const no_terms = nullptr;
    if (c->sum && c->global) {
      Timer tm(ctx, 23, n);
      if (c->nout)
        hipLaunchKernelGGL((k_circuit_eval_global<true, true, true>), grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts,
                           c->nasserts, c->nin, (uint32_t)nw, (uint32_t *)ctx->circ_state, colw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride,
                           d_holds, c->equal, c->nequal, c->outputs, c->nout, c->terms, c->hp);
      else
        hipLaunchKernelGGL((k_circuit_eval_global<true, false, true>), grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts,
                           c->nasserts, c->nin, (uint32_t)nw, (uint32_t *)ctx->circ_state, colw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride,
                           d_holds, c->equal, c->nequal, (const uint2 *)nullptr, 0u, c->terms, c->hp);
    } else if (c->sum) {
      Timer tm(ctx, 22, n);
      if (c->nout)
        hipLaunchKernelGGL((k_circuit_eval<true, true, true>), grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts,
                           c->nasserts, c->nin, (uint32_t)nw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds, c->equal, c->nequal,
                           c->outputs, c->nout, c->terms, c->hp);
      else
        hipLaunchKernelGGL((k_circuit_eval<true, false, true>), grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts,
                           c->nasserts, c->nin, (uint32_t)nw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds, c->equal, c->nequal,
                           (const uint2 *)nullptr, 0u, c->terms, c->hp);
    } else if (c->global && c->nout) {
      Timer tm(ctx, 21, n);
      hipLaunchKernelGGL((k_circuit_eval_global<true, true>), grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts,
                         c->nasserts, c->nin, (uint32_t)nw, (uint32_t *)ctx->circ_state, colw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride,
                         d_holds, c->equal, c->nequal, c->outputs, c->nout, no_terms, no_terms);
    } else if (c->nout) {
      Timer tm(ctx, 20, n);
      hipLaunchKernelGGL((k_circuit_eval<true, true>), grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts, c->nasserts,
                         c->nin, (uint32_t)nw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds, c->equal, c->nequal, c->outputs, c->nout, no_terms,
                         no_terms);
    } else if (c->global && c->ex) {
      Timer tm(ctx, 19, n);
      hipLaunchKernelGGL(k_circuit_eval_global<true>, grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts, c->nasserts,
                         c->nin, (uint32_t)nw, (uint32_t *)ctx->circ_state, colw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds, c->equal,
                         c->nequal, (const uint2 *)nullptr, 0u, no_terms, no_terms);
    } else if (c->global) {
      Timer tm(ctx, 17, n);
      hipLaunchKernelGGL(k_circuit_eval_global<false>, grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts, c->nasserts,
                         c->nin, (uint32_t)nw, (uint32_t *)ctx->circ_state, colw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds,
                         (const uint2 *)nullptr, 0u, (const uint2 *)nullptr, 0u, no_terms, no_terms);
    } else if (c->ex) {
      Timer tm(ctx, 18, n);
      hipLaunchKernelGGL(k_circuit_eval<true>, grid, dim3(CWG), 0, ctx->stream, (const uint4 *)c->gates, c->lp, c->nlev, c->asserts, c->nasserts, c->nin,
                         (uint32_t)nw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds, c->equal, c->nequal, (const uint2 *)nullptr, 0u, no_terms,
                         no_terms);
    } else {
      Timer tm(ctx, 16, n);
      hipLaunchKernelGGL(k_circuit_eval<false>, grid, dim3(CWG), 0, ctx->stream, (const uint2 *)c->gates, c->lp, c->nlev, c->asserts, c->nasserts, c->nin,
                         (uint32_t)nw, (const uint8_t *)d_in, in_stride, n, d_out, bits_stride, d_holds, (const uint2 *)nullptr, 0u, (const uint2 *)nullptr, 0u,
                         no_terms, no_terms);
    }
    if (hipGetLastError() != hipSuccess) { rc = MFH_EDEVICE; break; }
    if (hipMemcpyAsync(pin_out, d_out, (size_t)n * bits_stride, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(pin_out + out_b, d_holds, n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = MFH_EDEVICE; break; }
    if (bits_stride) memcpy(h_witness_bits + (size_t)b0 * bits_stride, pin_out, (size_t)n * bits_stride);
    if (h_holds) memcpy(h_holds + b0, pin_out + out_b, n);
  }
  if (in_b) pin_release(ctx, ctx->pin_rows);
  pin_release(ctx, ctx->pin_cw);
  if (rc != MFH_OK) {
    (void)hipGetLastError();
    ctx->err = "mfh_circuit_assign: launch or copy failed";
  }
  return rc;
}

}  // extern "C"
