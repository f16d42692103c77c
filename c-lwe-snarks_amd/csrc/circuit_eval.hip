// circuit_eval.hip -- mfh_circuit_create* / mfh_circuit_assign: the witnesses of a Boolean circuit for a batch of statements, bitsliced on the device.
//
// One workgroup serves a block of 32 statements.  It keeps one uint32 word per wire, bit j = statement j of the block, so a gate is one word operation for
// all 32 statements.  The gates are sorted by level on the host (inputs level 0, a gate one more than its highest operand); the workgroup's threads evaluate
// one level at a time, with a barrier between levels, all levels in one launch (a ripple-carry chain has depth ~ ngates).  Both transposes go through wave
// ballots:
//   in:  lanes 0..31 hold 32 input bits of statements 0..31, lanes 32..63 the next 32 bits: ballot t gives wire words of input bits t and t + 32;
//   out: lane l holds the word of wire 64 q + 1 + l: ballot((word >> j) & 1) is bits [64 q, 64 q + 64) of statement j's witness -- 8 output bytes.
// After the last level the computed public outputs are copied (pairs (p, w): st[p] = st[w], so bits [0, lu) of a witness row carry the computed statement
// whatever the caller put at p's input position), then assertions and equalities fold into one holds word per workgroup, then the witness is written.
//
// All of that is circuit_eval<REC, EX, OUT, SUM, UNROLL> on a plain uint32_t *st; the two kernels differ in where st lives:
//   k_circuit_eval         st = a __shared__ array of MFH_CIRCUIT_MAX_WIRES + 1 words (128 KiB of LDS), one gate per thread in flight;
//   k_circuit_eval_global  st = the block's column of colw words of ctx->circ_state, read and written by that block's workgroup alone -- so the workgroup
//                          barrier between levels (workgroup-scope release / acquire) orders everything -- and GUNROLL gates per thread in flight.
// The body is inlined into both, which is where st's address space is recovered: the LDS kernel has no flat access.
//
// Device records, by the program's kind (host records are (op, a, b) or, for extended programs, (op, a, b, c)):
//   kind                                   record                                  ops
//   LDS,           not extended            uint2 {a | b << 16, out | op << 16}     XOR AND OR NOT
//   device memory, not extended            uint4 {a, b, out, op}                   XOR AND OR NOT
//   extended, either state                 uint4 {a, b, c, out | op << 24}         the above, MAJ SUM3 CONST0 CONST1 LUT2(tt) = 16 + tt
//   extended with a WSUM gate: head        uint4 {first_term, nterms, nbits, out | MFH_GATE_WSUM << 24}; WSUM_BIT records have no device record
// and asserts[e] = {wire, value}, equal[e] = {a, b}, outputs[e] = {p, w} (no w is a p, every p once: no order among pairs), terms[e] = wire | shift << 24.
// Level L + 1 is records [lp[L], lp[L + 1]); its WSUM heads are the first of them, [lp[L], hp[L]).
//
// A head is served by one wave, the other way round from every other gate: lane j holds STATEMENT j's sum T_j = sum_e (bit j of term e's word) << shift_e as
// an ordinary integer (T < 2^24), and output wire i's word is the ballot of bit i of T over the lanes.  The wave first gathers up to 64 terms, one per lane
// (the term record and its wire word: one memory latency for 64 terms, in LDS or device memory alike), then walks them with v_readlane: four register
// instructions per term, no memory access in the loop, no counter array.  The heads of a level go to the waves from the last one down, while the level's
// one-word gates fill the threads from the first wave up: a level of the SHA-256 statement (2 - 4 heads, a few hundred cheap gates at most) then has no
// wave that does both.
//
// Which instantiation a program gets (mfh_circuit_assign; these ten exist and no other), and its timing kind 16 + 2 * tier + global:
//   tier 0  not extended (mfh_circuit_create, _global)             <false>               "circuit_assign"      "circuit_assign_global"
//   tier 1  extended, no outputs (_ex; _out, _sum that add none)   <true>                "circuit_assign_ex"   "circuit_assign_global_ex"
//   tier 2  extended with outputs (_out with nout > 0)             <true, true>          "circuit_assign_out"  "circuit_assign_global_out"
//   tier 3  with a WSUM gate (_sum), with outputs or without       <true, OUT, true>     "circuit_assign_sum"  "circuit_assign_global_sum"
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

// A program on the device (the table above): what mfh_circuit holds and the evaluation reads.  equal / outputs / terms, hp are read by the EX / OUT / SUM
// instantiations alone.  The fields are in the order of the kernels' arguments.
struct Program {
  const void *gates; const uint32_t *lp; uint32_t nlev;
  const uint2 *asserts; uint32_t nasserts, nin, nw;  // nw = nin + ngates: the last wire
  const uint2 *equal; uint32_t nequal;
  const uint2 *outputs; uint32_t nout;
  const uint32_t *terms, *hp;
};

// one-word gates: the three record formats decoded, and the gate's word from its operands' words (op = MFH_GATE_*, LUT2: 16 + tt)
struct Gate { uint32_t a, b, c, out, op; };
template <bool EX>
__device__ __forceinline__ Gate decode(const uint2 &r) {
  return {r.x & 0xffff, r.x >> 16, 0, r.y & 0xffff, r.y >> 16};
}
template <bool EX>
__device__ __forceinline__ Gate decode(const uint4 &r) {
  if constexpr (EX) return {r.x, r.y, r.z, r.w & 0xffffff, r.w >> 24};
  return {r.x, r.y, 0, r.z, r.w};
}
template <bool EX>
__device__ __forceinline__ uint32_t gate_word(uint32_t op, uint32_t x, uint32_t y, uint32_t z) {
  if constexpr (!EX) return op == MFH_GATE_XOR ? x ^ y : op == MFH_GATE_AND ? x & y : op == MFH_GATE_OR ? x | y : ~x;
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

// The evaluation of program p for the workgroup's block of statements on the wire words st (wire i at st[i]).  REC = the gate record, UNROLL = one-word
// gates in flight per thread and level (no gate of a level reads another's output).
template <typename REC, bool EX, bool OUT, bool SUM, uint32_t UNROLL>
__device__ __forceinline__ void circuit_eval(uint32_t *__restrict__ st, const Program &p, const uint8_t *__restrict__ in, size_t in_stride, uint32_t nstmt,
                                             uint8_t *__restrict__ out, size_t bits_stride, uint8_t *__restrict__ holds) {
  static_assert(EX || !OUT, "outputs belong to extended programs");
  static_assert(EX || !SUM, "weighted sums belong to extended programs");
  __shared__ uint32_t hw;
  const REC *__restrict__ gates = (const REC *)p.gates;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = CWG / 64;
  const uint32_t s0 = blockIdx.x * CSTMT, j = lane & 31;
  const bool live = s0 + j < nstmt;  // the tail block: statements past nstmt read zeros and write nothing
  if (tid == 0) hw = ~0u;

  // ---- inputs: statement rows -> wire words (wire k + 1 = input bit k)
  const uint8_t *row = in + (size_t)(live ? s0 + j : 0) * in_stride;
  for (uint32_t it = wave; it * 64 < p.nin; it += nwaves) {  // (wave-uniform trip count: every lane takes part in the ballots)
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
    if (k < p.nin) st[k + 1] = mine;
  }
  __syncthreads();

  // ---- gates, level by level
  uint32_t g1 = p.nlev ? p.lp[0] : 0;
  for (uint32_t lv = 0; lv < p.nlev; lv++) {
    uint32_t g0 = g1;
    g1 = p.lp[lv + 1];
    if constexpr (SUM) {  // the level's heads, one wave each, from the last wave down
      const uint32_t h1 = p.hp[lv], uw = __builtin_amdgcn_readfirstlane(nwaves - 1 - wave);
      for (uint32_t h = g0 + uw; h < h1; h += nwaves) {
        const uint4 r = gates[h];
        wsum_head(st, p.terms, __builtin_amdgcn_readfirstlane(r.x), __builtin_amdgcn_readfirstlane(r.y), __builtin_amdgcn_readfirstlane(r.z),
                  __builtin_amdgcn_readfirstlane(r.w & 0xffffff), lane);
      }
      g0 = h1;
    }
    for (uint32_t g = g0 + tid; g < g1; g += UNROLL * CWG) {
      REC r[UNROLL];
      uint32_t x[UNROLL], y[UNROLL], z[UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < UNROLL; u++)
        if (g + u * CWG < g1) r[u] = gates[g + u * CWG];
#pragma unroll
      for (uint32_t u = 0; u < UNROLL; u++)
        if (g + u * CWG < g1) {
          const Gate q = decode<EX>(r[u]);
          x[u] = st[q.a];
          y[u] = st[q.b];
          z[u] = EX ? st[q.c] : 0;
        }
#pragma unroll
      for (uint32_t u = 0; u < UNROLL; u++)
        if (g + u * CWG < g1) {
          const Gate q = decode<EX>(r[u]);
          st[q.out] = gate_word<EX>(q.op, x[u], y[u], z[u]);
        }
    }
    __syncthreads();
  }

  // ---- computed public outputs: the input wire p takes the value of wire w
  if constexpr (OUT) {
    for (uint32_t e = tid; e < p.nout; e += CWG) {
      const uint2 o = p.outputs[e];
      st[o.x] = st[o.y];
    }
    __syncthreads();
  }

  // ---- assertions and equalities
  uint32_t ok = ~0u;
  for (uint32_t e = tid; e < p.nasserts; e += CWG) {
    const uint2 a = p.asserts[e];
    ok &= a.y ? st[a.x] : ~st[a.x];
  }
  if constexpr (EX)
    for (uint32_t e = tid; e < p.nequal; e += CWG) {
      const uint2 q = p.equal[e];
      ok &= ~(st[q.x] ^ st[q.y]);
    }
  if (ok != ~0u) atomicAnd(&hw, ok);

  // ---- witness: wire words -> statement rows, 8 bytes per statement and group of 64 wires; bytes [0, bits_stride) all written
  const uint32_t nq = (uint32_t)((bits_stride + 7) / 8);
  for (uint32_t q = wave; q < nq; q += nwaves) {
    const uint32_t i = q * 64 + 1 + lane;
    const uint32_t word = i <= p.nw ? st[i] : 0;
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

// The kernels take the program's fields as loose arguments and hand the body a Program, which dissolves after inlining.  (As one by-value argument the
// struct shifts the register allocation of the device-memory kernels -- a VGPR less in four of them, three instructions more in <false> -- for no gain.)
template <bool EX, bool OUT = false, bool SUM = false>
__global__ __launch_bounds__(CWG) void k_circuit_eval(const void *__restrict__ gates, const uint32_t *__restrict__ lp, uint32_t nlev,
                                                      const uint2 *__restrict__ asserts, uint32_t nasserts, uint32_t nin, uint32_t nw,
                                                      const uint8_t *__restrict__ in, size_t in_stride, uint32_t nstmt, uint8_t *__restrict__ out,
                                                      size_t bits_stride, uint8_t *__restrict__ holds, const uint2 *__restrict__ equal, uint32_t nequal,
                                                      const uint2 *__restrict__ outputs, uint32_t nout, const uint32_t *__restrict__ terms,
                                                      const uint32_t *__restrict__ hp) {
  __shared__ uint32_t st[CWORDS];
  const Program p{gates, lp, nlev, asserts, nasserts, nin, nw, equal, nequal, outputs, nout, terms, hp};
  circuit_eval<std::conditional_t<EX, uint4, uint2>, EX, OUT, SUM, 1>(st, p, in, in_stride, nstmt, out, bits_stride, holds);
}

template <bool EX, bool OUT = false, bool SUM = false>
__global__ __launch_bounds__(CWG) void k_circuit_eval_global(const void *__restrict__ gates, const uint32_t *__restrict__ lp, uint32_t nlev,
                                                             const uint2 *__restrict__ asserts, uint32_t nasserts, uint32_t nin, uint32_t nw,
                                                             uint32_t *state, size_t colw, const uint8_t *__restrict__ in, size_t in_stride, uint32_t nstmt,
                                                             uint8_t *__restrict__ out, size_t bits_stride, uint8_t *__restrict__ holds,
                                                             const uint2 *__restrict__ equal, uint32_t nequal, const uint2 *__restrict__ outputs,
                                                             uint32_t nout, const uint32_t *__restrict__ terms, const uint32_t *__restrict__ hp) {
  const Program p{gates, lp, nlev, asserts, nasserts, nin, nw, equal, nequal, outputs, nout, terms, hp};
  circuit_eval<uint4, EX, OUT, SUM, GUNROLL>(state + (size_t)blockIdx.x * colw, p, in, in_stride, nstmt, out, bits_stride, holds);
}

}  // namespace

struct mfh_circuit {
  int device = 0;
  bool global = false;  // the wire state: false in LDS (k_circuit_eval), true in ctx->circ_state (k_circuit_eval_global)
  bool ex = false;      // extended: 16-byte {a, b, c, out | op << 24} records and equalities
  bool sum = false;     // has a WSUM gate
  void *mem = nullptr;  // the device image (Layout below); p points into it
  Program p{};
};

namespace {

// What a mfh_circuit_create* call asks for.  ex programs take 4-word gate records (op, a, b, c), the others 3-word (op, a, b); wsum = WSUM / WSUM_BIT
// records are accepted (mfh_circuit_create_sum alone).
struct CircuitDesc {
  const char *name;  // the entry point, for the error texts
  uint32_t nin, ngates; const uint32_t *gates;
  uint32_t nasserts; const uint32_t *asserts;
  uint32_t flags = 0;  // MFH_CIRCUIT_GLOBAL or 0
  bool ex = false, wsum = false;
  uint32_t nequal = 0, nout = 0, nterms = 0;
  const uint32_t *equal = nullptr, *outputs = nullptr, *terms = nullptr;  // pairs (a, b), (p, w), (wire, shift)
};

// Word offsets of a program's device image: gates | asserts | equal | outputs | lp (nlev + 1 words) | with WSUM gates: hp (nlev words) | terms
struct Layout { size_t asserts, equal, outputs, lp, hp, terms, words; };
Layout layout_of(const CircuitDesc &d, size_t rec, uint32_t nrec, uint32_t nlev, bool sum) {
  Layout L;
  L.asserts = rec * nrec;
  L.equal = L.asserts + 2 * (size_t)d.nasserts;
  L.outputs = L.equal + 2 * (size_t)d.nequal;
  L.lp = L.outputs + 2 * (size_t)d.nout;
  L.hp = L.lp + nlev + 1;
  L.terms = L.hp + (sum ? nlev : 0);
  L.words = L.terms + (sum ? d.nterms : 0);
  return L;
}

// source[p] = w for an output wire p (sized nin + 1 when the program has outputs, else empty).  An output wire has no value until the end of the evaluation,
// so nothing reads it but its own pair's equality
bool is_out(const std::vector<uint32_t> &source, uint32_t w) { return w < source.size() && source[w] != 0; }

// The rules of a WSUM head at gate g, q = (op, first_term, nterms, nbits), in the order they are tested: the text of the first one broken, or nullptr and
// *top = the highest level among its terms
const char *wsum_head_defect(const CircuitDesc &d, uint32_t g, const uint32_t *q, const std::vector<uint32_t> &lvl, const std::vector<uint32_t> &source,
                             uint32_t *top) {
  const uint32_t a = q[1], b = q[2], c = q[3], o = d.nin + 1 + g;
  if (b == 0) return "a WSUM gate with nterms = 0";
  if ((uint64_t)a + b > d.nterms) return "a WSUM gate's term range lies outside the term array";
  if (c > 24) return "a WSUM gate with nbits > 24";
  uint64_t tmax = 0;
  uint32_t prev = 0;
  *top = 0;
  for (uint32_t e = 0; e < b; e++) {
    const uint32_t w = d.terms[2 * ((size_t)a + e)], sh = d.terms[2 * ((size_t)a + e) + 1];
    if (w == 0 || w >= o) return "a WSUM term wire is 0 or not below the head's output wire";
    if (is_out(source, w)) return "a WSUM term reads an output wire";
    if (sh >= c) return "a WSUM term with shift >= nbits";
    if (sh < prev) return "WSUM terms not in non-decreasing shift order";
    prev = sh;
    tmax += (uint64_t)1 << sh;
    *top = std::max(*top, lvl[w]);
  }
  uint32_t len = 0;
  while (tmax >> len) len++;
  if (len != c) return "a WSUM gate whose nbits is not the bit length of the sum of 2^shift";
  if ((uint64_t)g + c > d.ngates) return "a WSUM head not followed by its WSUM_BIT records in order";
  return nullptr;
}

// every entry point: validate, level, sort by level, upload.  A mfh_circuit_create_sum program without a WSUM gate comes out as that of mfh_circuit_create_out.
int circuit_create(mfh_ctx *ctx, const CircuitDesc &d, mfh_circuit **out) {
  if (!ctx || !out) return MFH_EINVAL;
  *out = nullptr;
  const auto fail = [&](const char *what, int rc = MFH_EINVAL) { ctx->err = std::string(d.name) + ": " + what; return rc; };
  if (d.flags & ~MFH_CIRCUIT_GLOBAL) return fail("unknown flag bits");
  const bool global = (d.flags & MFH_CIRCUIT_GLOBAL) != 0, ex = d.ex;
  const uint32_t nin = d.nin, ngates = d.ngates;
  if ((ngates && !d.gates) || (d.nasserts && !d.asserts)) return fail("gates / assertions without their array");
  if (d.nequal && !d.equal) return fail("equalities without their array");
  if (d.nout && !d.outputs) return fail("outputs without their array");
  if (d.nterms && !d.terms) return fail("terms without their array");
  const uint64_t nw = (uint64_t)nin + ngates;
  if (nw > ctx->P.m - 1) return fail("nin + ngates > m - 1");
  if (!global && nw > MFH_CIRCUIT_MAX_WIRES) return fail("nin + ngates > MFH_CIRCUIT_MAX_WIRES (the wire state must fit 128 KiB of LDS)");
  if (ex && nw >= (1u << 24)) return fail("nin + ngates >= 2^24 (the records' 24-bit wire field)");
  const size_t gw = ex ? 4 : 3;  // words per input gate record
  std::vector<uint32_t> source(d.nout ? (size_t)nin + 1 : 0, 0);
  for (uint32_t e = 0; e < d.nout; e++) {
    const uint32_t p = d.outputs[2 * e], w = d.outputs[2 * e + 1];
    if (p == 0 || p > nin) return fail("an output wire p that is not an input wire (1 .. nin)");
    if (w == 0 || w > nw) return fail("an output's source wire w is 0 or above nin + ngates");
    if (w == p) return fail("an output wire defined as itself");
    if (source[p]) return fail("an output wire p given twice");
    source[p] = w;
  }
  for (uint32_t e = 0; e < d.nout; e++)
    if (is_out(source, d.outputs[2 * e + 1])) return fail("an output's source wire w is itself an output wire");
  std::vector<uint32_t> lvl(nw + 1, 0);
  uint32_t nlev = 0, nheads = 0, nbitrec = 0;
  uint32_t run_o = 0, run_n = 0, run_i = 0;  // inside a head's run of WSUM_BIT records: the head's output wire, its nbits, the next i
  for (uint32_t g = 0; g < ngates; g++) {
    const uint32_t *q = d.gates + gw * g;
    const uint32_t op = q[0], a = q[1], b = q[2], o = nin + 1 + g;
    if (!ex) {
      if (op > MFH_GATE_NOT) return fail("unknown gate op");
      if (a == 0 || a >= o || b == 0 || b >= o) return fail("a gate operand is 0 or not below the gate's output wire");
      lvl[o] = 1 + std::max(lvl[a], op == MFH_GATE_NOT ? lvl[a] : lvl[b]);
      nlev = std::max(nlev, lvl[o]);
      continue;
    }
    const uint32_t c = q[3];
    if (d.wsum && run_i < run_n) {  // the records after a head
      if (op != MFH_GATE_WSUM_BIT || a != run_i || b != 0 || c != 0) return fail("a WSUM head not followed by its WSUM_BIT records in order");
      lvl[o] = lvl[run_o];
      run_i++;
      nbitrec++;
      continue;
    }
    if (d.wsum && op == MFH_GATE_WSUM_BIT) return fail("a WSUM_BIT record without a head");
    if (d.wsum && op == MFH_GATE_WSUM) {
      uint32_t top = 0;
      if (const char *what = wsum_head_defect(d, g, q, lvl, source, &top)) return fail(what);
      lvl[o] = 1 + top;
      nlev = std::max(nlev, lvl[o]);
      run_o = o; run_n = c; run_i = 1;
      nheads++;
      continue;
    }
    if ((op > MFH_GATE_CONST1 && op < 16) || op >= 32) return fail("unknown gate op");
    if (op == MFH_GATE_CONST0 || op == MFH_GATE_CONST1) {
      if (a | b | c) return fail("a CONST gate with an operand other than 0");
      lvl[o] = 1;
    } else {
      const bool three = op == MFH_GATE_MAJ || op == MFH_GATE_SUM3;
      if (a == 0 || a >= o || b == 0 || b >= o || (three && (c == 0 || c >= o))) return fail("a gate operand is 0 or not below the gate's output wire");
      if (!three && c != 0) return fail("a one- or two-input gate with a third operand c != 0");
      if (op == MFH_GATE_NOT && b != a) return fail("a NOT gate with b != a");
      if (is_out(source, a) || is_out(source, b) || (three && is_out(source, c))) return fail("a gate reads an output wire");
      if (op == MFH_GATE_SUM3) {
        const uint32_t *m = q - gw;  // gate g - 1
        if (g == 0 || m[0] != MFH_GATE_MAJ) return fail("a SUM3 gate not directly after a MAJ gate");
        if (m[1] != a || m[2] != b || m[3] != c) return fail("a SUM3 gate whose operands differ from its MAJ's");
      }
      lvl[o] = 1 + std::max(std::max(lvl[a], lvl[b]), three ? lvl[c] : 0u);
    }
    nlev = std::max(nlev, lvl[o]);
  }
  if (run_i < run_n) return fail("a WSUM head not followed by its WSUM_BIT records in order");
  for (uint32_t e = 0; e < d.nasserts; e++) {
    const uint32_t w = d.asserts[2 * e], v = d.asserts[2 * e + 1];
    if (w == 0 || w > nw) return fail("an assertion on wire 0 or above nin + ngates");
    if (v > 1) return fail("an assertion value other than 0 / 1");
    if (is_out(source, w)) return fail("an assertion on an output wire");
  }
  for (uint32_t e = 0; e < d.nequal; e++) {
    const uint32_t a = d.equal[2 * e], b = d.equal[2 * e + 1];
    if (a == 0 || a > nw || b == 0 || b > nw) return fail("an equality on wire 0 or above nin + ngates");
    if (a == b) return fail("an equality of a wire with itself");
    if ((is_out(source, a) && source[a] != b) || (is_out(source, b) && source[b] != a)) return fail("an equality on an output wire other than its own pair's");
  }
  // counting sort by level (stable: creation order within a level; with WSUM gates a level's heads come first, and WSUM_BIT records are dropped)
  const bool sum = nheads != 0;
  const auto opof = [&](uint32_t g) { return d.gates[gw * g]; };
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
  const Layout at = layout_of(d, rec, nrec, nlev, sum);
  std::vector<uint32_t> host(at.words);
  {
    std::vector<uint32_t> pos(lp.begin(), lp.end()), cpos(hp.begin(), hp.end());  // next slot of a level: heads from lp[L], the others from hp[L]
    for (uint32_t g = 0; g < ngates; g++) {
      if (is_bit(g)) continue;
      const uint32_t *q = d.gates + gw * g;
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
    std::copy(d.asserts, d.asserts + (size_t)2 * d.nasserts, host.begin() + at.asserts);
    std::copy(d.equal, d.equal + (size_t)2 * d.nequal, host.begin() + at.equal);
    std::copy(d.outputs, d.outputs + (size_t)2 * d.nout, host.begin() + at.outputs);
    std::copy(lp.begin(), lp.end(), host.begin() + at.lp);
    std::copy(hp.begin(), hp.end(), host.begin() + at.hp);
    for (uint32_t e = 0; sum && e < d.nterms; e++) host[at.terms + e] = d.terms[2 * (size_t)e] | d.terms[2 * (size_t)e + 1] << 24;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  mfh_circuit *c = new mfh_circuit();
  c->device = ctx->device;
  c->global = global;
  c->ex = ex;
  c->sum = sum;
  if (hipMalloc(&c->mem, host.size() * 4) != hipSuccess) {
    (void)hipGetLastError();
    delete c;
    return fail("no memory for the gate program", MFH_ENOMEM);
  }
  if (hipMemcpy(c->mem, host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(c->mem);
    delete c;
    return fail("upload failed", MFH_EDEVICE);
  }
  const uint32_t *w = (const uint32_t *)c->mem;
  c->p = {w, w + at.lp, nlev, (const uint2 *)(w + at.asserts), d.nasserts, nin, (uint32_t)nw, (const uint2 *)(w + at.equal), d.nequal,
          (const uint2 *)(w + at.outputs), d.nout, sum ? w + at.terms : nullptr, sum ? w + at.hp : nullptr};
  *out = c;
  return MFH_OK;
}

// the description shared by mfh_circuit_create_ex / _out / _sum
CircuitDesc extended(const char *name, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts, uint32_t nequal,
                     const uint32_t *h_equal, uint32_t flags) {
  CircuitDesc d{name, nin, ngates, h_gates, nasserts, h_asserts, flags, true};
  d.nequal = nequal;
  d.equal = h_equal;
  return d;
}

// one chunk of statements of mfh_circuit_assign
struct Chunk { uint32_t n; size_t colw; const uint8_t *in; size_t in_stride; uint8_t *out; size_t bits_stride; uint8_t *holds; };  // n statements
template <bool GLOBAL, bool EX, bool OUT = false, bool SUM = false>
void launch(mfh_ctx *ctx, const mfh_circuit *c, const Chunk &k) {
  Timer tm(ctx, 16 + 2 * (SUM ? 3 : OUT ? 2 : EX ? 1 : 0) + GLOBAL, k.n);  // mfh_timing_kind (mfhip.hip): 16 + 2 * tier + global
  const dim3 grid((k.n + CSTMT - 1) / CSTMT);
  const Program &p = c->p;
  if constexpr (GLOBAL)
    hipLaunchKernelGGL((k_circuit_eval_global<EX, OUT, SUM>), grid, dim3(CWG), 0, ctx->stream, p.gates, p.lp, p.nlev, p.asserts, p.nasserts, p.nin, p.nw, ctx->circ_state.as<uint32_t>(), k.colw, k.in, k.in_stride,
                       k.n, k.out, k.bits_stride, k.holds, p.equal, p.nequal, p.outputs, p.nout, p.terms, p.hp);
  else
    hipLaunchKernelGGL((k_circuit_eval<EX, OUT, SUM>), grid, dim3(CWG), 0, ctx->stream, p.gates, p.lp, p.nlev, p.asserts, p.nasserts, p.nin, p.nw, k.in, k.in_stride, k.n, k.out, k.bits_stride, k.holds, p.equal, p.nequal, p.outputs, p.nout, p.terms, p.hp);
}

}  // namespace

extern "C" {

int mfh_circuit_create(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                       mfh_circuit **out) {
  return circuit_create(ctx, CircuitDesc{"mfh_circuit_create", nin, ngates, h_gates, nasserts, h_asserts}, out);
}

int mfh_circuit_create_global(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                              mfh_circuit **out) {
  return circuit_create(ctx, CircuitDesc{"mfh_circuit_create_global", nin, ngates, h_gates, nasserts, h_asserts, MFH_CIRCUIT_GLOBAL}, out);
}

int mfh_circuit_create_ex(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                          uint32_t nequal, const uint32_t *h_equal, uint32_t flags, mfh_circuit **out) {
  return circuit_create(ctx, extended("mfh_circuit_create_ex", nin, ngates, h_gates, nasserts, h_asserts, nequal, h_equal, flags), out);
}

int mfh_circuit_create_out(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                           uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, uint32_t flags, mfh_circuit **out) {
  CircuitDesc d = extended("mfh_circuit_create_out", nin, ngates, h_gates, nasserts, h_asserts, nequal, h_equal, flags);
  d.nout = nout;
  d.outputs = h_outputs;
  return circuit_create(ctx, d, out);
}

int mfh_circuit_create_sum(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                           uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, uint32_t nterms_total,
                           const uint32_t *h_terms, uint32_t flags, mfh_circuit **out) {
  CircuitDesc d = extended("mfh_circuit_create_sum", nin, ngates, h_gates, nasserts, h_asserts, nequal, h_equal, flags);
  d.nout = nout;
  d.outputs = h_outputs;
  d.wsum = true;
  d.nterms = nterms_total;
  d.terms = h_terms;
  return circuit_create(ctx, d, out);
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
  const uint64_t nw = c->p.nw;
  if (in_stride * 8 < c->p.nin) { ctx->err = "mfh_circuit_assign: in_stride * 8 < nin"; return MFH_EINVAL; }
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
  if (int rc = work_reserve(ctx, ctx->circ_io, io_b)) return rc;
  if (c->global)
    if (int rc = work_reserve(ctx, ctx->circ_state, (size_t)(ch + CSTMT - 1) / CSTMT * colw * 4)) return rc;
  uint8_t *pin_in = in_b ? (uint8_t *)pin_acquire(ctx, ctx->pin_rows, in_b) : nullptr;
  uint8_t *pin_out = (uint8_t *)pin_acquire(ctx, ctx->pin_cw, out_b + ch);
  if ((in_b && !pin_in) || !pin_out) return MFH_ENOMEM;
  uint8_t *d_in = ctx->circ_io.as<uint8_t>(), *d_out = d_in + in_b, *d_holds = d_out + out_b;
  int rc = MFH_OK;
  for (uint32_t b0 = 0; b0 < nstmt && rc == MFH_OK; b0 += ch) {
    const uint32_t n = std::min(ch, nstmt - b0);
    if (in_b) {
      memcpy(pin_in, h_inputs + (size_t)b0 * in_stride, (size_t)n * in_stride);
      if (hipMemcpyAsync(d_in, pin_in, (size_t)n * in_stride, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = MFH_EDEVICE; break; }
    }
    const Chunk k{n, colw, d_in, in_stride, d_out, bits_stride, d_holds};
    switch (c->sum << 3 | (c->p.nout != 0) << 2 | c->ex << 1 | c->global) {  // sum, out, ex, global: the ten kinds of program circuit_create makes
      case 0b0000: launch<false, false>(ctx, c, k); break;
      case 0b0001: launch<true, false>(ctx, c, k); break;
      case 0b0010: launch<false, true>(ctx, c, k); break;
      case 0b0011: launch<true, true>(ctx, c, k); break;
      case 0b0110: launch<false, true, true>(ctx, c, k); break;
      case 0b0111: launch<true, true, true>(ctx, c, k); break;
      case 0b1010: launch<false, true, false, true>(ctx, c, k); break;
      case 0b1011: launch<true, true, false, true>(ctx, c, k); break;
      case 0b1110: launch<false, true, true, true>(ctx, c, k); break;
      case 0b1111: launch<true, true, true, true>(ctx, c, k); break;
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
