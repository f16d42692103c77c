// witness.hip -- the witness pass (reference src/snark.c:141,147-155), the first step of every prover entry point:
//     w_b[k] = delta_b t[k] + sum_i bit_b[i] v_i[k]  (mod p),   k = 0 .. d - 1,
// over the SSP's wire polynomials v_i (slot i + 1; slot 0 = t): a dense uint32 image or the generator of ssp_prg.hpp.  (The row SSP has no
// v_i to sum: the entry points hand it to ssp_rows.hip.)  Four forms, all staging the bits through pinned memory into c->wws, on c->stream:
//   VALU, one statement   k_witness_partial[_prg] sums the selected rows in G shares, k_witness_finish adds delta t: mfh_witness_poly (mfh_prove);
//                         mfh_witness_lanes / _from_lanes (a rank's share of the rows); mfh_ssp_prg_make_t (t of a generated SSP is such a sum)
//   VALU, 12 statements   k_witness_partial_multi[_prg]<12>, a row read or generated once per 12: mfh_witness_poly_multi (batch chain, d % 128 != 0)
//   GEMM, <= 256          bits x SSP bytes on the matrix cores, the rows read once (k_witness_mm<MT> / k_witness_mm8q: B fragments from the image
//                         k_ssp_frag builds per SSP) or generated once (k_witness_mm_prg<MT> / k_witness_mm8q_prg: B fragments hashed in the
//                         kernel): mfh_witness_poly_mm (batch chain), mfh_witness_poly_mm_cols (a rank's coefficient range, row-sharded prover)
//   GEMM, a whole call    SSP bytes x bits, the batch prover's streaming launch (evalmm.hip: mms_plan_ssp) over the A-fragment image k_ssp_image builds per SSP, in groups
//                         of 255 statements: mfh_witness_poly_stream; mfh_prove_batch (snark.hip: batch_witness_stream) shares b_w's digit fragments with it
#include <algorithm>
#include <type_traits>

#include "ctx.hpp"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// sum_g partial[g * d + k] mod p on top of s (< p): the G shares of a coefficient's row sum, each reduced as it is added
__device__ __forceinline__ uint64_t partial_sum(const uint64_t *__restrict__ partial, uint32_t G, uint32_t d, uint32_t k, uint64_t s) {
  for (uint32_t g = 0; g < G; g++) s = (s + partial[(uint64_t)g * d + k] % MFH_P) % MFH_P;
  return s;
}
// byte w of x0 .. x3 as one dword {x0.bw, x1.bw, x2.bw, x3.bw}: two v_perm
__device__ __forceinline__ uint32_t byte_plane(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, int w) {
  return __builtin_amdgcn_perm(x1, x0, 0x0c0c0400u + 0x00000101u * w)    // {x0.bw, x1.bw, 0, 0}
         | __builtin_amdgcn_perm(x3, x2, 0x04000c0cu + 0x01010000u * w);  // {0, 0, x2.bw, x3.bw}
}
// row of a 32x32 MFMA tile (= statement within its tile of 32) that accumulator element e of a lane of half h holds
__device__ __forceinline__ constexpr uint32_t acc_row(uint32_t e, uint32_t h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// partial[g][k] = sum over the g-th share of selected rows of v_row[k]   (uint64, no reduction needed: < 2^32 * rows)
__global__ __launch_bounds__(256) void k_witness_partial(const uint32_t *__restrict__ ssp, const uint32_t *__restrict__ rows, uint32_t nsel,
                                                         uint32_t d, uint64_t *__restrict__ partial) {
  const uint32_t k4 = blockIdx.x * blockDim.x + threadIdx.x;  // group of 4 coefficients
  if (k4 * 4 >= d) return;
  const uint32_t G = gridDim.y, g = blockIdx.y;
  uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (uint32_t i = g; i < nsel; i += G) {
    const uint4 v = *reinterpret_cast<const uint4 *>(ssp + (uint64_t)rows[i] * d + (uint64_t)k4 * 4);
    s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
  }
  uint64_t *o = partial + (uint64_t)g * d + (uint64_t)k4 * 4;
  o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
}

// the same partial sums with generator-defined rows: every thread makes 4 consecutive coefficients of each selected row
__global__ __launch_bounds__(256) void k_witness_partial_prg(uint64_t seed, const uint32_t *__restrict__ rows, uint32_t nsel, uint32_t d,
                                                             uint64_t *__restrict__ partial) {
  const uint32_t k4 = blockIdx.x * blockDim.x + threadIdx.x;
  if (k4 * 4 >= d) return;
  const uint32_t G = gridDim.y, g = blockIdx.y;
  const uint32_t k = k4 * 4;
  uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (uint32_t i = g; i < nsel; i += G) {
    const uint32_t rk = mf::ssp_prg_rowkey(seed, rows[i]);
    s0 += mf::ssp_prg_raw(rk, k);  // raw values: congruent to the coefficients mod p, the sums are reduced by the finish kernels
    s1 += mf::ssp_prg_raw(rk, k + 1);
    s2 += mf::ssp_prg_raw(rk, k + 2);
    s3 += mf::ssp_prg_raw(rk, k + 3);
  }
  uint64_t *o = partial + (uint64_t)g * d + k;
  o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
}
// The witness pass for NB statements at once: every selected SSP row is read ONCE and added into the accumulators of the statements
// whose bit selects it.  list[i] = {slot, mask}: bit b of mask = statement b selects the row (uniform per row: scalar branches).
// partial[(b * G + g) * d + k]: the per-statement layout k_witness_finish reads.
template <int NB>
__global__ __launch_bounds__(256) void k_witness_partial_multi(const uint32_t *__restrict__ ssp, const uint2 *__restrict__ list, uint32_t nsel,
                                                               uint32_t d, uint64_t *__restrict__ partial) {
  const uint32_t k4 = blockIdx.x * blockDim.x + threadIdx.x;
  if (k4 * 4 >= d) return;
  const uint32_t G = gridDim.y, g = blockIdx.y;
  uint64_t acc[NB][4];
#pragma unroll
  for (int b = 0; b < NB; b++) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0;
  auto add = [&](const uint4 &v, uint32_t mask) {
#pragma unroll
    for (int b = 0; b < NB; b++)
      if ((mask >> b) & 1) { acc[b][0] += v.x; acc[b][1] += v.y; acc[b][2] += v.z; acc[b][3] += v.w; }
  };
  const uint32_t *col = ssp + (uint64_t)k4 * 4;
  uint32_t i = g;
  for (; i + 3 * G < nsel; i += 4 * G) {  // four rows in flight
    const uint2 e0 = list[i], e1 = list[i + G], e2 = list[i + 2 * G], e3 = list[i + 3 * G];
    const uint4 v0 = *reinterpret_cast<const uint4 *>(col + (uint64_t)e0.x * d), v1 = *reinterpret_cast<const uint4 *>(col + (uint64_t)e1.x * d);
    const uint4 v2 = *reinterpret_cast<const uint4 *>(col + (uint64_t)e2.x * d), v3 = *reinterpret_cast<const uint4 *>(col + (uint64_t)e3.x * d);
    add(v0, e0.y); add(v1, e1.y); add(v2, e2.y); add(v3, e3.y);
  }
  for (; i < nsel; i += G) {
    const uint2 e = list[i];
    add(*reinterpret_cast<const uint4 *>(col + (uint64_t)e.x * d), e.y);
  }
#pragma unroll
  for (int b = 0; b < NB; b++) {
    uint64_t *o = partial + ((uint64_t)b * G + g) * d + (uint64_t)k4 * 4;
    o[0] = acc[b][0]; o[1] = acc[b][1]; o[2] = acc[b][2]; o[3] = acc[b][3];
  }
}
// the same with generator-defined rows (csrc/ssp_prg.hpp): every selected row is GENERATED once per NB statements
template <int NB>
__global__ __launch_bounds__(256) void k_witness_partial_multi_prg(uint64_t seed, const uint2 *__restrict__ list, uint32_t nsel, uint32_t d,
                                                                   uint64_t *__restrict__ partial) {
  const uint32_t k4 = blockIdx.x * blockDim.x + threadIdx.x;
  if (k4 * 4 >= d) return;
  const uint32_t G = gridDim.y, g = blockIdx.y, k = k4 * 4;
  uint64_t acc[NB][4];
#pragma unroll
  for (int b = 0; b < NB; b++) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0;
  for (uint32_t i = g; i < nsel; i += G) {
    const uint2 e = list[i];
    const uint32_t rk = mf::ssp_prg_rowkey(seed, e.x);
    const uint32_t v0 = mf::ssp_prg_raw(rk, k), v1 = mf::ssp_prg_raw(rk, k + 1), v2 = mf::ssp_prg_raw(rk, k + 2), v3 = mf::ssp_prg_raw(rk, k + 3);
#pragma unroll
    for (int b = 0; b < NB; b++)
      if ((e.y >> b) & 1) { acc[b][0] += v0; acc[b][1] += v1; acc[b][2] += v2; acc[b][3] += v3; }
  }
#pragma unroll
  for (int b = 0; b < NB; b++) {
    uint64_t *o = partial + ((uint64_t)b * G + g) * d + k;
    o[0] = acc[b][0]; o[1] = acc[b][1]; o[2] = acc[b][2]; o[3] = acc[b][3];
  }
}
// materialise generator-defined slots [first, first+nslots) as a dense uint32 image (tests; small instances)
__global__ void k_ssp_prg_fill(uint64_t seed, uint32_t first_slot, uint32_t d, uint64_t total, uint32_t *__restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t slot = first_slot + (uint32_t)(i / d), k = (uint32_t)(i % d);
    out[i] = mf::ssp_prg_coeff(mf::ssp_prg_rowkey(seed, slot), k);
  }
}
// t = v_0 + (summed selected rows) - 1: random_ssp's definition (src/ssp.c:59-71), for a generator-defined SSP
__global__ void k_ssp_prg_make_t(uint64_t seed, const uint64_t *__restrict__ partial, uint32_t G, uint32_t d, uint32_t *__restrict__ t) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d) return;
  uint64_t s = partial_sum(partial, G, d, k, mf::ssp_prg_coeff(mf::ssp_prg_rowkey(seed, 1), k));  // v_0 = slot 1
  if (k == 0) s = (s + MFH_P - 1) % MFH_P;
  t[k] = (uint32_t)s;
}
__global__ void k_witness_finish(const uint32_t *__restrict__ ssp, const uint64_t *__restrict__ partial, uint32_t G, uint32_t d, uint32_t delta,
                                 uint32_t *__restrict__ w) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d) return;
  w[k] = (uint32_t)partial_sum(partial, G, d, k, ((uint64_t)ssp[k] * delta) % MFH_P);  // slot 0 = t
}
__global__ void k_witness_lanes(const uint64_t *__restrict__ partial, uint32_t G, uint32_t d, uint64_t *__restrict__ lanes) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d) return;
  lanes[k] = partial_sum(partial, G, d, k, 0);
}

// ---- the witness pass of up to 32 statements as a GEMM over the SSP rows (one read of the SSP) ---------------------------------------
//   sum_b[k] = sum_i bit_b[i] * v_i[k]:   A = the statements' witness bits (0/1), B = the bytes of v_i[k] (offset by 128), K = rows.
// The SSP is row-major (v_i[k], k fastest) but the MFMA wants 16 consecutive ROWS per lane, so a second image of the SSP in B-fragment
// order is built once per SSP (k_ssp_frag, same size as the uint32 SSP): for row step K (32 rows), coefficient tile kt (32
// coefficients), byte w and lane (k = 32 kt + (l & 31), h = l >> 5): the 16 bytes [byte w of v_{32K+16h+e+1}[k]] ^ 0x80, e = 0..15, at
// frag[(((kt * KS + K) * 4 + w) * 64 + l) * 16 + e] (KS row steps: a coefficient tile's fragments are contiguous, so a wave reads one
// sequential stream -- with the row step outermost, 8 KiB pieces 4 MiB apart, the pass ran at 3.75 TB/s).  The pass is then a pure stream: four 16-byte loads and four 32x32x32 MFMAs
// (M = 32 statements) per wave and row step.
__global__ void k_ssp_frag(const uint32_t *__restrict__ ssp, uint32_t nrowsel, uint32_t d, uint32_t *__restrict__ frag) {
  // one thread = 4 rows x 1 coefficient -> one dword of each of the four byte columns
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t KT = d / 32;
  const uint32_t lane = gid & 63, eg = (gid >> 6) & 3;
  const uint64_t tile = gid >> 8;  // K * KT + kt
  const uint32_t kt = (uint32_t)(tile % KT), K = (uint32_t)(tile / KT);
  const uint32_t KSt = (nrowsel + 31) / 32;
  if (K >= KSt) return;
  const uint32_t k = kt * 32 + (lane & 31), rb = K * 32 + 16 * (lane >> 5) + 4 * eg;
  uint32_t x[4];
#pragma unroll
  for (int e = 0; e < 4; e++) x[e] = rb + e < nrowsel ? ssp[(uint64_t)(rb + e + 2) * d + k] ^ 0x80808080u : 0u;  // row r = v_{r+1} = slot r + 2
#pragma unroll
  for (int w = 0; w < 4; w++) frag[(((((uint64_t)kt * KSt + K) * 4 + w) * 64 + lane) << 2) + eg] = byte_plane(x[0], x[1], x[2], x[3], w);
}
// A third image of the SSP, in the A-fragment order k_mmstream reads (header of expandmm.hip), for the batch prover's streamed witness pass (evalmm.hip:
// mms_plan_ssp): the SSP as the MATRIX of that GEMM and the witness bits as its digit columns -- b_w's own product over the BT+BV image with the SSP in the
// image's place.  "Row" r = 0 .. m - 1 of the K dimension is slot r + 1 (r = 0: v_0, whose digit column holds coefficient 0; r >= 1: v_r, selected by bit
// r - 1: exactly the digit matrix k_mm_digits builds for b_w), "byte position" 4 k + w is byte w of coefficient k, so that a lane's packed record (pk = 1: four
// consecutive byte positions, sum_e acc[e] 2^(8 e)) is the integer sum_r bit_r v_r[k] itself up to the -128 corrections.  For row tile P (16 byte positions =
// coefficients 4 P .. 4 P + 3) and 64-row k-step ks:
//     img[((P * KS + ks) * 64 + lane) * 16 + e] = byte (lane & 3) of v_r[4 P + ((lane & 15) >> 2)] ^ 0x80,   r = 64 ks + 16 (lane >> 4) + e,
// KS = the k-steps of m rows padded to 256-row stages; rows >= m hold 0x80 (A = 0; their digits are zero as well).  (d / 4) x KS KiB: the size of the uint32
// SSP, rounded up to whole stages.  One thread = 16 rows x 1 coefficient -> the 16-byte elements of the four lanes that hold the coefficient's four bytes
// (64 contiguous bytes); consecutive threads take consecutive coefficients, so the reads of a row are coalesced.  d % 64 == 0: a wave has one (ks, lane >> 4).
__global__ __launch_bounds__(256) void k_ssp_image(const uint32_t *__restrict__ ssp, uint32_t m, uint32_t d, uint32_t KS, uint4 *__restrict__ img) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = (uint32_t)(gid % d), rest = (uint32_t)(gid / d), g4 = rest & 3, ks = rest >> 2;
  if (ks >= KS) return;
  const uint32_t r0 = 64 * ks + 16 * g4;
  uint32_t x[16];
#pragma unroll
  for (int e = 0; e < 16; e++) x[e] = (r0 + e < m ? ssp[(uint64_t)(r0 + e + 1) * d + k] : 0u) ^ 0x80808080u;
  uint4 *o = img + (((uint64_t)(k >> 2) * KS + ks) * 64 + 16 * g4 + 4 * (k & 3));
#pragma unroll
  for (int w = 0; w < 4; w++)
    o[w] = uint4{byte_plane(x[0], x[1], x[2], x[3], w), byte_plane(x[4], x[5], x[6], x[7], w), byte_plane(x[8], x[9], x[10], x[11], w),
                 byte_plane(x[12], x[13], x[14], x[15], w)};
}
// The witness kernels work on a RANGE of coefficients [col0, col0 + d) of the polynomials (the whole polynomial: col0 = 0, d = the SSP's
// d; a rank of the row-sharded batch prover computes its slice of every statement's w: mfh_witness_poly_mm_cols): `d` below is the width
// of the range (and of the partial arrays), WCols carries where it starts.
struct WCols {
  uint32_t kt0;      // col0 / 32: first 32-coefficient tile
  uint32_t KS;       // row steps of the whole SSP (the fragment image's tile stride)
  uint64_t wstride;  // coefficients between consecutive statements of the output
};
// grid = (d / 128, row chunks); block = 4 waves, one 32-coefficient tile each; MT = 1, 2 or 4 tiles of 32 statements (the SSP is read
// once per 32 MT statements).  part[((chunk * 4 + w) * 32 MT + stmt) * d + k].
template <int MT>
__global__ __launch_bounds__(256) void k_witness_mm(const v4i *__restrict__ sspfrag, const v4i *__restrict__ bitfrag, uint32_t nrowsel /* m - 1 */,
                                                    uint32_t ksteps_per_chunk, uint32_t d, int *__restrict__ part, WCols wc) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint32_t ktl = blockIdx.x * 4 + wave, kt = wc.kt0 + ktl;
  const uint32_t k = ktl * 32 + r32;  // (within the range)
  const uint32_t K0 = blockIdx.y * ksteps_per_chunk, K1 = min((nrowsel + 31) / 32, K0 + ksteps_per_chunk);
  v16i acc[MT][4];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[t][w][e] = 0;
  if (K0 >= K1) return;  // (uniform)
  // PF row steps of fragments in flight per wave (MT = 4 holds 256 accumulator registers: one wave per SIMD, so the stream has to be
  // kept ahead by hand); loads past the chunk re-read its last step
  constexpr int PF = 3;
  v4i bq[PF][4], aq[PF][MT];
  auto fetch = [&](int slot, uint32_t K) {
    K = min(K, K1 - 1);
    const v4i *src = sspfrag + (((uint64_t)kt * wc.KS + K) * 4) * 64 + lane;
#pragma unroll
    for (int w = 0; w < 4; w++) bq[slot][w] = src[64 * w];
#pragma unroll
    for (int t = 0; t < MT; t++) aq[slot][t] = bitfrag[((uint64_t)K * MT + t) * 64 + lane];
  };
#pragma unroll
  for (int i = 0; i < PF; i++) fetch(i, K0 + i);
  for (uint32_t K = K0; K < K1; K += PF) {
#pragma unroll
    for (int i = 0; i < PF; i++) {
      if (K + i < K1) {
#pragma unroll
        for (int t = 0; t < MT; t++)
#pragma unroll
          for (int w = 0; w < 4; w++) acc[t][w] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[i][t], bq[i][w], acc[t][w], 0, 0, 0);
        fetch(i, K + i + PF);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const uint32_t stmt = 32 * t + acc_row(e, h);
        part[(((uint64_t)blockIdx.y * 4 + w) * (32 * MT) + stmt) * d + k] = acc[t][w][e];
      }
}
// The same pass over a GENERATOR-DEFINED SSP (csrc/ssp_prg.hpp; BASELINE configs 3/4, where the dense SSP would be 5.9 TB): the B
// fragments are not loaded but generated -- lane (coefficient k, row half h) hashes its 16 (row, k) pairs (9 integer operations each; the
// un-reduced 32-bit hash: sums of raw values and sums of coefficients agree mod p) and picks the four byte planes with v_perm -- so that a
// selected row is generated once per 32 MT statements instead of once per 12 (the VALU form, k_witness_partial_multi_prg): at 2^20
// constraints the witness pass of a statement drops from 19 ms to about 2.  rowkeys[r] = ssp_prg_rowkey(seed, slot r + 2), padded to a
// multiple of 32 rows.
__global__ void k_prg_rowkeys(uint64_t seed, uint32_t nrows_pad, uint32_t *__restrict__ rk) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nrows_pad) rk[r] = mf::ssp_prg_rowkey(seed, r + 2);
}
template <int MT>
__global__ __launch_bounds__(256) void k_witness_mm_prg(const uint32_t *__restrict__ rowkeys, const v4i *__restrict__ bitfrag, uint32_t nrowsel /* m - 1 */,
                                                        uint32_t ksteps_per_chunk, uint32_t d, int *__restrict__ part, WCols wc) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint32_t kt = blockIdx.x * 4 + wave;
  const uint32_t k = kt * 32 + r32;  // (within the range)
  const uint32_t K0 = blockIdx.y * ksteps_per_chunk, K1 = min((nrowsel + 31) / 32, K0 + ksteps_per_chunk);
  v16i acc[MT][4];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[t][w][e] = 0;
  if (K0 >= K1) return;  // (uniform)
  const uint32_t kc = wc.kt0 * 32 + k + mf::SSP_PRG_K0;
  // the bit fragments and the row keys of a step are loaded two steps ahead (consumed in the step that issues them, the loads cost their
  // whole latency every step: 0.85 us per step against 0.35 of arithmetic); loads past the chunk re-read its last step
  constexpr int PF = 2;
  v4i aqr[PF][MT];
  uint4 rkr[PF][4];
  auto fetch = [&](uint32_t K, int slot) {
    K = min(K, K1 - 1);
#pragma unroll
    for (int t = 0; t < MT; t++) aqr[slot][t] = bitfrag[((uint64_t)K * MT + t) * 64 + lane];
    const uint4 *rk4 = reinterpret_cast<const uint4 *>(rowkeys + 32 * (uint64_t)K + 16 * h);
#pragma unroll
    for (int q = 0; q < 4; q++) rkr[slot][q] = rk4[q];
  };
  fetch(K0, 0);
  fetch(K0 + 1, 1);
  auto step = [&](uint32_t K, int slot) {
    v4i aq[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) aq[t] = aqr[slot][t];
    uint32_t x[16];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint4 r = rkr[slot][q];
      x[4 * q] = r.x; x[4 * q + 1] = r.y; x[4 * q + 2] = r.z; x[4 * q + 3] = r.w;
    }
    fetch(K + PF, slot);
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = mf::ssp_prg_mix(kc * x[e]);  // mf::ssp_prg_raw(rowkey, k)
    v4i bq[4];
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int j = 0; j < 4; j++) bq[w][j] = (int)(byte_plane(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3], w) ^ 0x80808080u);
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int w = 0; w < 4; w++) acc[t][w] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aq[t], bq[w], acc[t][w], 0, 0, 0);
  };
  uint32_t K = K0;
  for (; K + 2 <= K1; K += 2) {
    step(K, 0);
    step(K + 1, 1);
  }
  if (K < K1) step(K, 0);
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const uint32_t stmt = 32 * t + acc_row(e, h);
        part[(((uint64_t)blockIdx.y * 4 + w) * (32 * MT) + stmt) * d + k] = acc[t][w][e];
      }
}
// 256 statements per generation with TWO waves per SIMD.  The 8 statement tiles x 4 byte planes of a 32-coefficient tile (512 accumulator registers) go to
// four waves, 4 statement tiles x 2 planes each (128 registers; round 4 -- rounds 2-3 gave a wave all 8 statement tiles of ONE plane: 8 KiB of bit fragments
// + 1 KiB of coefficient bytes read from LDS per wave and 32-row step, 72 KiB per CU = 576 clk of the LDS pipe against 512 clk of MFMAs per SIMD: the pass was
// LDS-bound, a build without the MFMAs ran no faster; 4 + 2 KiB per wave are 384 clk).  The four waves SHARE the hashes four ways -- wave j hashes rows
// 4 j .. 4 j + 3 of a lane's 16 and publishes dword j of all four planes' fragments through LDS (a three-slot ring: the hashes of step K + 2 are issued between
// the MFMAs of step K, the fragments of step K + 1 are read during step K; the row keys are loaded four steps ahead), wave (sh, pp) reads the fragments of
// planes 2 pp and 2 pp + 1 with two 16-byte loads and the bit fragments of statement tiles 4 sh .. 4 sh + 3.  4 hashes and 8 MFMAs per wave and step, and
// with two waves per SIMD one wave's hashes run under the other's MFMAs.
// Chunk partials only (k_witness_mm_finish).  grid = (d / 64, row chunks), block = 8 waves = 2 coefficient tiles x (2 statement halves x 2 plane pairs).
__global__ __launch_bounds__(512) void k_witness_mm8q_prg(const uint32_t *__restrict__ rowkeys, const v4i *__restrict__ bitfrag, uint32_t nrowsel /* m - 1 */,
                                                          uint32_t ksteps_per_chunk, uint32_t d, int *__restrict__ part, WCols wc) {
  constexpr int MT = 8, RING = 4;
  __shared__ v4i bits[RING][MT][64];
  __shared__ uint32_t xch[3][2][4][64][4];  // [step % 3][tile][plane][lane][hashing wave]
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint32_t tile = wave >> 2, pl = wave & 3;
  const uint32_t sh = pl >> 1, pp = pl & 1;        // the wave's statement half (tiles 4 sh ..) and plane pair (planes 2 pp, 2 pp + 1)
  // which 4 of a lane's 16 rows this wave hashes = which dword of the lane's fragments it publishes: rotated by the lane's 16-lane group, so that the 64
  // lanes of a ds_write_b32 into the [lane][4 dwords] slots hit 64 different banks (with pos = pl for every lane the addresses are 16 bytes apart: 16
  // distinct banks, every publish a 4-way conflict -- PMC: SQ_LDS_BANK_CONFLICT was 37 % of the LDS cycles of the pass)
  const uint32_t pos = (pl + (lane >> 4)) & 3;
  const uint32_t ktl = blockIdx.x * 2 + tile, kt = wc.kt0 + ktl;
  const uint32_t kc = kt * 32 + r32 + mf::SSP_PRG_K0;
  const uint32_t K0 = blockIdx.y * ksteps_per_chunk, K1 = min((nrowsel + 31) / 32, K0 + ksteps_per_chunk);
  v16i acc[4][2];
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[t][q][e] = 0;
  if (K0 >= K1) return;  // (uniform)
  auto bits_load = [&](uint32_t K) -> v4i { return bitfrag[(uint64_t)min(K, K1 - 1) * MT * 64 + tid]; };  // 512 elements per step: one per thread
  auto bits_store = [&](uint32_t K, v4i st) { (&bits[K % RING][0][0])[tid] = st; };
  auto rk_load = [&](uint32_t K) -> uint4 { return *reinterpret_cast<const uint4 *>(rowkeys + 32 * (uint64_t)min(K, K1 - 1) + 16 * h + 4 * pos); };
  auto hash1 = [&](uint32_t rowkey) -> uint32_t {  // mf::ssp_prg_raw(rowkey, k)
#ifdef WPRG_NOHASH  // timing-only build (wrong results): what the kernel costs without the generator's arithmetic
    return kc ^ rowkey;
#endif
    return mf::ssp_prg_mix(kc * rowkey);
  };
  auto publish = [&](uint32_t K, const uint32_t (&x)[4]) {  // dword `pos` of the four planes' fragments of step K
#pragma unroll
    for (int w = 0; w < 4; w++) xch[K % 3][tile][w][lane][pos] = byte_plane(x[0], x[1], x[2], x[3], w) ^ 0x80808080u;
  };
  auto fragment = [&](uint32_t K, uint32_t q) -> v4i { return *reinterpret_cast<const v4i *>(&xch[K % 3][tile][2 * pp + q][lane][0]); };
  uint4 rkr[4];  // the row keys of steps K + 2 .. K + 5
  v4i sta, stb;  // the bit fragments of steps K + 1 / K + 2 on their way to the ring
  sta = bits_load(K0);
  bits_store(K0, sta);
  sta = bits_load(K0 + 1);
  stb = bits_load(K0 + 2);
  {
    const uint4 r0 = rk_load(K0), r1 = rk_load(K0 + 1);
    const uint32_t x0[4] = {hash1(r0.x), hash1(r0.y), hash1(r0.z), hash1(r0.w)};
    const uint32_t x1[4] = {hash1(r1.x), hash1(r1.y), hash1(r1.z), hash1(r1.w)};
    publish(K0, x0);
    publish(K0 + 1, x1);
  }
#pragma unroll
  for (int i = 2; i <= 5; i++) rkr[i & 3] = rk_load(K0 + i);
  __syncthreads();
  v4i bq0 = fragment(K0, 0), bq1 = fragment(K0, 1);
  uint32_t K = K0;
  auto step = [&](int slot, v4i &st) {  // st: the bit fragment of step K + 1 (loaded two steps ago); refilled with that of step K + 3
    const v4i bn0 = fragment(K + 1, 0), bn1 = fragment(K + 1, 1);  // (published a step ago, before the barrier)
    const uint4 rk = rkr[(slot + 2) & 3];  // step K + 2
    const uint32_t hr[4] = {rk.x, rk.y, rk.z, rk.w};
    uint32_t hx[4];
    bits_store(K + 1, st);
    const v4i *aq = &bits[K % RING][4 * sh][lane];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const v4i a = aq[t * 64];
#ifdef WPRG_NOMFMA  // timing-only build (wrong results): the generation, its LDS exchange and the barriers without the matrix cores
      acc[t][0][0] += a[0] ^ bq0[t];
      acc[t][1][0] += a[1] ^ bq1[t];
#else
      acc[t][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq0, acc[t][0], 0, 0, 0);
      acc[t][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq1, acc[t][1], 0, 0, 0);
#endif
      hx[t] = hash1(hr[t]);
    }
    publish(K + 2, hx);  // (slot last read during step K - 2, two barriers ago)
    rkr[(slot + 2) & 3] = rk_load(K + 6);
    bq0 = bn0;
    bq1 = bn1;
    st = bits_load(K + 3);
#ifndef WPRG_NOSYNC  // (timing-only build without it: wrong results -- what the step barrier costs)
    __syncthreads();
#endif
    K++;
  };
  while (K + 4 <= K1) {  // (K advances inside step)
    step(0, sta);
    step(1, stb);
    step(2, sta);
    step(3, stb);
  }
  if (K < K1) step(0, sta);
  if (K < K1) step(1, stb);
  if (K < K1) step(2, sta);
  uint32_t dd = d;
  asm volatile("" : "+s"(dd));  // (keeps the store addresses from being computed ahead of the loop)
#pragma unroll
  for (int q = 0; q < 2; q++) {
    int *dst = part + (((uint64_t)blockIdx.y * 4 + 2 * pp + q) * (32 * MT) + 128 * sh) * dd + ktl * 32 + r32 + (uint64_t)(4 * h) * dd;
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int e = 0; e < 16; e++) dst[(uint64_t)acc_row(e, 0) * dd] = acc[t][q][e];
      dst += (uint64_t)32 * dd;
    }
  }
}
// 256 statements (a whole super-group of 248) in ONE read of the dense SSP.  8 statement tiles x 4 byte planes are 512 accumulator
// registers per 32-coefficient tile: the four planes go to four waves (128 registers each, two waves per SIMD; a workgroup = 2
// coefficient tiles x 4 planes), the eight bit fragments of a row step -- 8 KiB, the same for all eight waves -- go through a four-slot
// LDS ring (fetched straight from L2 by every wave they made a first version L1-bound: 2.26 ms against 2 x 0.59 for two 124-statement
// passes) and are read from it a step ahead, under the previous step's MFMAs.  Vector-memory operations complete in issue order, so
// EVERY load of the loop is consumed exactly PF steps after its issue (the plane's fragment of step K + PF, the bit fragment of step
// K + 2 + PF, staged in registers and stored to the ring two steps ahead of its use), and the prologue issues its loads in the order
// the loop does, pinned: s_waitcnt vmcnt(n) is a static count of younger loads and the compiler takes the minimum over the paths into
// the loop (with the bit fragments staged two steps ahead, or all of them loaded first, it emitted vmcnt(4..9) where the steady state
// allows 12: the stream was awaited one or two steps after its issue whatever PF).  Timing-only builds split the pass: the stream
// alone 0.53 ms per 248 statements (5.4 TB/s), MFMAs + LDS alone 0.54, together 0.77 -- with one wave per SIMD (wave pairs, two
// planes each: the first version) as with two; the chip does not hold its clock under both.
// part == nullptr (one row chunk, m < 2^16): the four waves exchange their plane sums through LDS, one statement tile per round, and the
// tile's owner writes w_b[k] = delta_b t[k] + the byte sum mod p (what k_witness_mm_finish does from chunk partials: 0.5 GB written and
// read back per 248 statements otherwise).  grid = (d / 64, row chunks), block = 8 waves.
__global__ __launch_bounds__(512) void k_witness_mm8q(const v4i *__restrict__ sspfrag, const v4i *__restrict__ bitfrag, uint32_t nrowsel /* m - 1 */,
                                                      uint32_t ksteps_per_chunk, uint32_t d, int *__restrict__ part, const uint32_t *__restrict__ tpoly /* + col0 */,
                                                      const uint32_t *__restrict__ cnt_delta, uint32_t nstmt, uint32_t *__restrict__ w_out, WCols wc) {
  constexpr int MT = 8, RING = 4, PF = 4;
  __shared__ v4i bits[RING][MT][64];      // 32 KiB
  __shared__ uint32_t xch[2][3][16][64];  // the epilogue's exchange: [coefficient tile][sending wave (owner skipped)][e][lane], 24 KiB
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint32_t tile = wave >> 2, pl = wave & 3;
  const uint32_t ktl = blockIdx.x * 2 + tile, kt = wc.kt0 + ktl;
  const uint32_t K0 = blockIdx.y * ksteps_per_chunk, K1 = min((nrowsel + 31) / 32, K0 + ksteps_per_chunk);
  v16i acc[MT];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[t][e] = 0;
  if (K0 >= K1) return;  // (uniform)
  auto bits_load = [&](uint32_t K) -> v4i { return bitfrag[(uint64_t)min(K, K1 - 1) * MT * 64 + tid]; };  // 512 elements per step: one per thread
  auto bits_store = [&](uint32_t K, v4i st) { (&bits[K % RING][0][0])[tid] = st; };
  auto ssp_load = [&](uint32_t K) -> v4i { return sspfrag[(((uint64_t)kt * wc.KS + min(K, K1 - 1)) * 4 + pl) * 64 + lane]; };
  v4i stg[PF], bq[PF];
  {
    const v4i s0 = bits_load(K0), s1 = bits_load(K0 + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < PF; i++) {  // (in the order the loop issues them)
      bq[i] = ssp_load(K0 + i);
      stg[i] = bits_load(K0 + 2 + i);
      __builtin_amdgcn_sched_barrier(0);
    }
    bits_store(K0, s0);
    bits_store(K0 + 1, s1);
  }
  __syncthreads();
  v4i acur[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) acur[t] = bits[K0 % RING][t][lane];
  uint32_t K = K0;
  auto step = [&](int slot) {
    bits_store(K + 2, stg[slot]);
    v4i anext[MT];
    const v4i *aq = &bits[(K + 1) % RING][0][lane];
#pragma unroll
    for (int t = 0; t < MT; t++) anext[t] = aq[t * 64];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(acur[t], bq[slot], acc[t], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    bq[slot] = ssp_load(K + PF);
    stg[slot] = bits_load(K + 2 + PF);
#pragma unroll
    for (int t = 0; t < MT; t++) acur[t] = anext[t];
    __syncthreads();
    K++;
  };
  while (K + PF <= K1) {  // (K advances inside step)
#pragma unroll
    for (int i = 0; i < PF; i++) step(i);
  }
#pragma unroll
  for (int i = 0; i + 1 < PF; i++)
    if (K < K1) step(i);
  uint32_t dd = d;
  asm volatile("" : "+s"(dd));  // (keeps the store addresses from being computed ahead of the loop)
  if (part) {
    int *dst = part + ((uint64_t)blockIdx.y * 4 + pl) * (32 * MT) * dd + ktl * 32 + r32 + (uint64_t)(4 * h) * dd;
#pragma unroll
    for (int t = 0; t < MT; t++) {
#pragma unroll
      for (int e = 0; e < 16; e++) dst[(uint64_t)acc_row(e, 0) * dd] = acc[t][e];
      dst += (uint64_t)32 * dd;
    }
    return;
  }
  // statement tile t is finished by wave t >> 1 of the coefficient tile: the other three hand over their plane sums (acc + 128 cnt_b:
  // the true byte sum, < 2^24 for m < 2^16), one statement tile per round
  asm volatile("" : "+s"(cnt_delta), "+s"(tpoly));
  const uint32_t k = ktl * 32 + r32;
  const uint64_t tk = tpoly[k], ws = wc.wstride, P = MFH_P;
#pragma unroll
  for (int t = 0; t < MT; t++) {
    const uint32_t owner = t >> 1;
    uint32_t mine[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const uint32_t b = 32 * t + acc_row(e, h);
      mine[e] = (uint32_t)acc[t][e] + (b < nstmt ? 128u * cnt_delta[2 * b] : 0u);
    }
    if (pl != owner) {  // (wave-uniform)
      const uint32_t sidx = pl - (pl > owner);
#pragma unroll
      for (int e = 0; e < 16; e++) xch[tile][sidx][e][lane] = mine[e];
    }
    __syncthreads();
    if (pl == owner) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const uint32_t b = 32 * t + acc_row(e, h);
        if (b < nstmt) {
          uint64_t val = (uint64_t)mine[e] << (8 * owner);
#pragma unroll
          for (int o = 0; o < 4; o++)
            if (o != (int)owner) val += (uint64_t)xch[tile][o - (o > (int)owner)][e][lane] << (8 * o);
          w_out[(uint64_t)b * ws + k] = (uint32_t)((val % P + tk * cnt_delta[2 * b + 1] % P) % P);
        }
      }
    }
    __syncthreads();
  }
}
// bits of nstmt statements (packed, bits_stride bytes apart) -> A fragments: bitfrag[K][t][lane (stmt = 32 t + (l & 31), h)][e] = bit
// (32 K + 16 h + e) of that statement
// (one thread per lane's 16 bytes: two bytes of the statement's bit string in, one 16-byte store out)
__global__ void k_witness_bits(const uint8_t *__restrict__ bits, size_t bits_stride, uint32_t nstmt, uint32_t nrowsel, uint32_t ksteps, uint32_t MT,
                               int8_t *__restrict__ bitfrag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // one lane of one fragment: 16 output bytes
  if (i >= ksteps * MT * 64) return;
  const uint32_t lane = i & 63, t = (i >> 6) % MT, K = (i >> 6) / MT, stmt = 32 * t + (lane & 31), h = lane >> 5;
  const uint32_t r0 = K * 32 + 16 * h;  // rows r0 .. r0 + 15: bits of two consecutive bytes (r0 is a multiple of 16)
  uint32_t w = 0;
  if (stmt < nstmt && r0 < nrowsel) {
    const uint8_t *b = bits + (size_t)stmt * bits_stride + (r0 >> 3);
    w = b[0];
    if (r0 + 8 < nrowsel) w |= (uint32_t)b[1] << 8;
    if (nrowsel - r0 < 16) w &= (1u << (nrowsel - r0)) - 1;  // rows beyond the last selected one contribute nothing
  }
  uint32_t o[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t n4 = (w >> (4 * q)) & 15;  // four bits -> four bytes of 0 / 1
    o[q] = (n4 & 1) | ((n4 & 2) << 7) | ((n4 & 4) << 14) | ((n4 & 8) << 21);
  }
  reinterpret_cast<uint4 *>(bitfrag)[i] = uint4{o[0], o[1], o[2], o[3]};
}
// w_b[k] = delta_b t[k] + sum_i bit_b[i] v_i[k] mod p from the chunk partials: sum_w 256^w (G'_w + 128 cnt_b)
__global__ void k_witness_mm_finish(const int *__restrict__ part, uint32_t nchunks, const uint32_t *__restrict__ t, const uint32_t *__restrict__ cnt_delta,
                                    uint32_t nstmt, uint32_t mrows /* 32 MT */, uint32_t d, uint32_t *__restrict__ w_out, uint64_t wstride) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (k >= d || b >= nstmt) return;
  const uint64_t corr = 128ull * cnt_delta[2 * b];
  const uint32_t delta = cnt_delta[2 * b + 1];
  uint64_t val = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    int64_t g = 0;
    for (uint32_t ch = 0; ch < nchunks; ch++) g += part[(((uint64_t)ch * 4 + w) * mrows + b) * d + k];
    val += (uint64_t)(g + (int64_t)corr) << (8 * w);  // the true byte sum: >= 0
  }
  const uint64_t P = MFH_P;
  w_out[(uint64_t)b * wstride + k] = (uint32_t)((val % P + (uint64_t)t[k] * delta % P) % P);
}

// ---- host side: what the forms share ---------------------------------------------------------------------------------------------------
// What the entry points check of their arguments, in two steps (the registered SSP and the shape are looked at between them): the pointers
// and the statement count against nmax, what the form takes in one pass (`in`: the bits, or the lanes that stand for them); then delta_b < p
bool witness_args_ok(const mfh_ctx *c, uint32_t nstmt, uint32_t nmax, const void *in, const uint32_t *h_delta, const uint32_t *d_w) {
  return c && in && h_delta && d_w && nstmt && nstmt <= nmax;
}
int witness_deltas(mfh_ctx *c, uint32_t nstmt, const uint32_t *h_delta) {
  for (uint32_t b = 0; b < nstmt; b++)
    if (h_delta[b] >= MFH_P) { c->err = "delta must be < p"; return MFH_EINVAL; }
  return MFH_OK;
}
// whether a statement selects v_i (slot i + 1), i = 1 .. m - 1: bit i - 1 of its packed bits
inline uint32_t witness_bit(const uint8_t *h_bits, uint32_t i) { return (h_bits[(i - 1) >> 3] >> ((i - 1) & 7)) & 1u; }
// how many of v_1 .. v_{m-1} it selects: whole bytes by popcount, then the last byte's bits below m - 1 (its padding bits are not looked at)
uint32_t witness_count(const uint8_t *h_bits, uint32_t m) {
  uint32_t cnt = 0, i = 1;
  for (; i + 8 <= m; i += 8) cnt += (uint32_t)__builtin_popcount(h_bits[(i - 1) >> 3]);
  for (; i < m; i++) cnt += witness_bit(h_bits, i);
  return cnt;
}
constexpr size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// c->wws as N areas back to back: area i is bytes [off[i], off[i + 1]) (callers round a size up where the next area wants the alignment)
template <int N> struct WwsCarve {
  size_t off[N + 1] = {0};
  WwsCarve(const size_t (&bytes)[N]) { for (int i = 0; i < N; i++) off[i + 1] = off[i] + bytes[i]; }
  size_t bytes(int i) const { return off[i + 1] - off[i]; }
  int reserve(mfh_ctx *c) const { return wws_reserve(c, off[N]); }
  template <class T> T *at(const mfh_ctx *c, int i) const { return reinterpret_cast<T *>(c->wws.as<uint8_t>() + off[i]); }
};

// VALU, one statement: partial[g][k] sums over this rank's share of the selected SSP rows; finish(partial, G) launches what becomes of them
template <class F> int witness_partials(mfh_ctx *c, const mf::SspSrc &src, const uint8_t *h_bits, uint32_t rank, uint32_t world, F &&finish) {
  const uint32_t d = c->P.d, m = c->P.m;
  if (d % 4) { c->err = "d must be a multiple of 4"; return MFH_EINVAL; }
  uint32_t *rows = (uint32_t *)pin_acquire(c, c->pin_rows, (size_t)m * 4 + 4);
  if (!rows) return MFH_ENOMEM;
  uint32_t nall = 0;
  for (uint32_t i = 1; i < m; i++)
    if (witness_bit(h_bits, i)) rows[nall++] = i + 1;  // slot of v_i
  const mf::Share sel = mf::row_share(nall, rank, world);  // contiguous share of the selected rows
  const uint32_t lo = (uint32_t)sel.lo, nsel = (uint32_t)sel.cnt, G = std::max(1u, std::min(64u, nsel / 8 + 1));
  const WwsCarve<2> ws({up256((size_t)m * 4), (size_t)G * d * 8});
  if (int rc = ws.reserve(c)) return rc;
  uint32_t *d_rows = ws.at<uint32_t>(c, 0);  // the selected rows | the partials
  uint64_t *partial = ws.at<uint64_t>(c, 1);
  if (nsel) HIP_TRY(c, hipMemcpyAsync(d_rows, rows + lo, (size_t)nsel * 4, hipMemcpyHostToDevice, c->stream));
  pin_release(c, c->pin_rows);
  if (src.dense)
    hipLaunchKernelGGL(k_witness_partial, dim3((d / 4 + 255) / 256, G), dim3(256), 0, c->stream, src.dense, d_rows, nsel, d, partial);
  else
    hipLaunchKernelGGL(k_witness_partial_prg, dim3((d / 4 + 255) / 256, G), dim3(256), 0, c->stream, src.seed, d_rows, nsel, d, partial);
  HIP_TRY(c, hipGetLastError());
  finish(partial, G);
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

// The GEMM form's launch plan: nstmt statements over a range of nc coefficients, dense (B fragments loaded) or generated
struct MmPlan {
  uint32_t MT;               // statement tiles of 32: 1, 2, 4 (k_witness_mm[_prg]<MT>) or 8 (k_witness_mm8q[_prg])
  uint32_t nrowsel, ksteps;  // the m - 1 rows a statement may select, in steps of 32
  // (MT = 8, dense: nc / 64 workgroups of one wave per SIMD, so one row chunk fills the chip at nc >= 2^14; small instances: nothing to fill either way)
  bool fused;                // k_witness_mm8q finishes in the kernel: one row chunk, and byte sums that fit 32 bits per plane pair
  uint32_t nchunks, kpc, ychunks;  // row chunks the partials are sized for; row steps per chunk; the chunks these make (the GEMM grid's y, summed by k_witness_mm_finish)
  size_t packed, cd_off;     // the head area: the statements' packed bits, then from cd_off (count of selected rows, delta) per statement
  enum { HEAD, BITFRAG, PART, ROWKEYS };
  WwsCarve<4> ws;            // head | bit fragments | chunk partials | row keys (generated rows only)
  MmPlan(const mfh_ctx *c, bool dense, uint32_t nstmt, size_t bits_stride, uint32_t nc)
      : MT(nstmt > 128 ? 8 : nstmt > 64 ? 4 : nstmt > 32 ? 2 : 1), nrowsel(c->P.m - 1), ksteps((nrowsel + 31) / 32),
        fused(MT == 8 && dense && c->P.m < 65536 && (nc >= 16384 || ksteps <= 64)), nchunks(fused ? 1u : std::min(ksteps, 4u)),
        kpc((ksteps + nchunks - 1) / nchunks), ychunks((ksteps + kpc - 1) / kpc), packed((size_t)nstmt * bits_stride), cd_off(packed + (8 - packed % 8) % 8),
        ws({up256(packed + 8 + 256 * 8), (size_t)ksteps * MT * 1024, (size_t)nchunks * 4 * 32 * MT * nc * 4, dense ? 0 : up256((size_t)ksteps * 32 * 4)}) {}
};
// f(std::integral_constant<int, MT>) for MT = 1, 2 or 4: the one place that turns the plan's tile count into a template argument
template <class F> void with_mt(uint32_t MT, F &&f) {
  if (MT == 1) f(std::integral_constant<int, 1>{});
  else if (MT == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace

// The SSP image of k_ssp_image, built where ssp_frag is built -- on first use per SSP -- and stale where ssp_frag_src is (ssp_images_stale).  Any stream may read it
// afterwards, so the build is awaited here, once per SSP.  No room: nullptr and no error, the caller keeps k_witness_mm8q (as batch_transient_image's callers
// regenerate the keystream).
const uint8_t *ssp_image(mfh_ctx *c, const uint32_t *d_ssp) {
  const uint32_t d = c->P.d, m = c->P.m;
  if (!d_ssp || d % 64 || m < 2) return nullptr;
  const uint32_t KS = (m + 255) / 256 * 4;  // 64-row k-steps, whole 256-row stages (mms_stream)
  const size_t bytes = (size_t)(d / 4) * KS * 1024;
  if (c->ssp_img_src == d_ssp && c->ssp_img.cap >= bytes) return c->ssp_img.as<uint8_t>();
  c->ssp_img_src = nullptr;
  if (c->ssp_img.cap < bytes) {
    if (c->ssp_img.p) {
      (void)hipDeviceSynchronize();
      dev_free(c->ssp_img);
    }
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) mem_free = 0;
    if (bytes > mem_free / 4 * 3 || !dev_alloc(c->ssp_img, bytes)) {
      (void)hipGetLastError();
      return nullptr;
    }
  }
  hipLaunchKernelGGL(k_ssp_image, dim3((uint32_t)((uint64_t)d * KS * 4 / 256)), dim3(256), 0, c->stream, d_ssp, m, d, KS, c->ssp_img.as<uint4>());
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return nullptr;
  c->ssp_img_src = d_ssp;
  return c->ssp_img.as<uint8_t>();
}

extern "C" {

// mfh_witness_poly_mm's results for ANY number of statements by the batch prover's streamed pass (evalmm.hip: mms_plan_ssp): groups of 255 statements, up to
// 8 groups per streaming launch over the SSP image -- k_mmstream1 for one group, the persistent grid k_mmstream_pb for 2, 4 or 8, k_mmstream otherwise --, the
// digit fragments built here (mfh_prove_batch shares b_w's).  Dense SSPs with d % 64 == 0; MFH_EUNSUPPORTED otherwise, MFH_ENOMEM without room for the image.
int mfh_witness_poly_stream(mfh_ctx *c, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta, uint32_t *d_w) {
  if (!witness_args_ok(c, nstmt, 0xffffffffu, h_bits, h_delta, d_w)) return MFH_EINVAL;
  const uint32_t d = c->P.d, m = c->P.m;
  if (!d_ssp || d % 64 || m < 2 || !mms_ssp_ok(c)) { c->err = "mfh_witness_poly_stream: a dense SSP, d a multiple of 64 and packed partial products"; return MFH_EUNSUPPORTED; }
  const uint32_t bstride = (m + 6) / 8;
  if (bits_stride < bstride) { c->err = "bits_stride shorter than the m - 1 witness bits"; return MFH_EINVAL; }
  if (int rc = witness_deltas(c, nstmt, h_delta)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint8_t *img = ssp_image(c, d_ssp);
  if (!img) { c->err = "mfh_witness_poly_stream: no room for the SSP image"; return MFH_ENOMEM; }
  constexpr uint32_t SG = 255, NG = 8;  // statements per group (one digit column each + the ones column), groups per launch
  for (uint32_t s0 = 0; s0 < nstmt; s0 += SG * NG) {
    const uint32_t cnt = std::min(SG * NG, nstmt - s0), ng = (cnt + SG - 1) / SG;
    MmsPlan P;
    if (!mms_plan_ssp(c, img, ng, P)) return MFH_EINVAL;
    // per group the packed bits and the deltas, staged in one copy | the groups' column sums | digit fragments | partial products
    const size_t head_g = up256((size_t)SG * bstride + 3) + up256((size_t)SG * 4), delta_off = up256((size_t)SG * bstride + 3);
    const WwsCarve<4> ws({head_g * ng, (size_t)ng * 2048, P.cd_bytes * ng, P.part_bytes * ng});
    if (int rc = ws.reserve(c)) return rc;
    PinBuf &wpin = c->pin_wring[c->pin_wnext++ % 8];
    uint8_t *stage = (uint8_t *)pin_acquire(c, wpin, head_g * ng);
    if (!stage) return MFH_ENOMEM;
    uint8_t *dev = ws.at<uint8_t>(c, 0);
    MmIo ios[NG];
    uint32_t nvs[NG], *W[NG];
    const uint32_t *dl[NG];
    for (uint32_t g = 0; g < ng; g++) {
      const uint32_t b0 = s0 + g * SG, sg = std::min(SG, nstmt - b0);
      for (uint32_t b = 0; b < sg; b++) memcpy(stage + g * head_g + (size_t)b * bstride, h_bits + (size_t)(b0 + b) * bits_stride, bstride);
      memcpy(stage + g * head_g + delta_off, h_delta + b0, (size_t)sg * 4);
      ios[g] = MmIo{{nullptr, nullptr}, sg, {nullptr, nullptr}, sg, 0, dev + g * head_g, bstride, ws.at<int64_t>(c, 1) + 256 * g};
      nvs[g] = sg;
      dl[g] = (const uint32_t *)(dev + g * head_g + delta_off);
      W[g] = d_w + (size_t)b0 * d;
    }
    HIP_TRY(c, hipMemcpyAsync(dev, stage, head_g * ng, hipMemcpyHostToDevice, c->stream));
    pin_release(c, wpin);
    HIP_TRY(c, hipMemsetAsync(ws.at<uint8_t>(c, 1), 0, (size_t)ng * 2048, c->stream));
    P.cd = ws.at<int8_t>(c, 2);
    P.part = ws.at<int>(c, 3);
    int rc = mms_digits(c, P, ios, nvs);
    if (!rc) rc = mms_stream(c, P);
    if (!rc) rc = mms_witness_finish(c, P, ios, nvs, d_ssp, dl, W);
    if (rc) return rc;
  }
  return MFH_OK;
}

int mfh_ssp_set_prg(mfh_ctx *c, uint64_t seed, const uint32_t *d_t) {
  if (!c) return MFH_EINVAL;
  if (d_t) ssp_rows_free(c, false);  // registering one kind replaces the other
  c->prg_on = d_t != nullptr;
  c->prg_seed = seed;
  c->prg_t = d_t;
  return MFH_OK;
}

int mfh_ssp_prg_fill(mfh_ctx *c, uint64_t seed, size_t first_slot, size_t nslots, uint32_t *d_out) {
  if (!c || !d_out) return MFH_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t total = (uint64_t)nslots * c->P.d;
  if (!total) return MFH_OK;
  hipLaunchKernelGGL(k_ssp_prg_fill, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 4096)), dim3(256), 0, c->stream, seed, (uint32_t)first_slot,
                     c->P.d, total, d_out);
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

int mfh_ssp_prg_make_t(mfh_ctx *c, uint64_t seed, const uint8_t *h_bits, uint32_t *d_t) {
  if (!c || !h_bits || !d_t) return MFH_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  return witness_partials(c, mf::SspSrc{nullptr, d_t, seed}, h_bits, 0, 1, [&](const uint64_t *partial, uint32_t G) {
    hipLaunchKernelGGL(k_ssp_prg_make_t, dim3((c->P.d + 255) / 256), dim3(256), 0, c->stream, seed, partial, G, c->P.d, d_t);
  });
}

int mfh_witness_poly(mfh_ctx *c, const uint32_t *d_ssp, const uint8_t *h_bits, uint32_t delta, uint32_t *d_w) {
  if (!witness_args_ok(c, 1, 1, h_bits, &delta, d_w)) return MFH_EINVAL;
  if (int rc = witness_deltas(c, 1, &delta)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (ssp_is_rows(c, d_ssp)) return ssp_rows_witness(c, 1, h_bits, (c->P.m + 6) / 8, &delta, d_w, c->P.d);
  mf::SspSrc src;
  if (int rc = ssp_src(c, d_ssp, src)) return rc;
  return witness_partials(c, src, h_bits, 0, 1, [&](const uint64_t *partial, uint32_t G) {
    hipLaunchKernelGGL(k_witness_finish, dim3((c->P.d + 255) / 256), dim3(256), 0, c->stream, src.t, partial, G, c->P.d, delta, d_w);
  });
}

// mfh_witness_poly for up to 12 statements in one pass over the SSP (d_ssp == NULL: the rows are generated once per pass): d_w = nstmt
// polynomials of d coefficients
int mfh_witness_poly_multi(mfh_ctx *c, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta, uint32_t *d_w) {
  constexpr int NB = 12;
  if (!witness_args_ok(c, nstmt, NB, h_bits, h_delta, d_w)) return MFH_EINVAL;
  if (ssp_is_rows(c, d_ssp)) return ssp_rows_witness(c, nstmt, h_bits, bits_stride, h_delta, d_w, c->P.d);
  mf::SspSrc src;  // d_ssp == NULL: the registered generator-defined SSP
  if (int rc = ssp_src(c, d_ssp, src)) return rc;
  const uint32_t d = c->P.d, m = c->P.m;
  if (d % 4) { c->err = "d must be a multiple of 4"; return MFH_EINVAL; }
  if (int rc = witness_deltas(c, nstmt, h_delta)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  uint2 *list = (uint2 *)pin_acquire(c, c->pin_rows, (size_t)m * 8 + 8);
  if (!list) return MFH_ENOMEM;
  uint32_t nsel = 0;
  for (uint32_t i = 1; i < m; i++) {
    uint32_t mask = 0;
    for (uint32_t b = 0; b < nstmt; b++) mask |= witness_bit(h_bits + b * bits_stride, i) << b;
    if (mask) list[nsel++] = make_uint2(i + 1, mask);  // slot of v_i
  }
  const uint32_t G = std::max(1u, std::min(16u, nsel / 8 + 1));
  const WwsCarve<2> ws({up256((size_t)m * 8), (size_t)NB * G * d * 8});  // the selected rows and their masks | the partials
  if (int rc = ws.reserve(c)) return rc;
  uint2 *d_list = ws.at<uint2>(c, 0);
  uint64_t *partial = ws.at<uint64_t>(c, 1);
  if (nsel) HIP_TRY(c, hipMemcpyAsync(d_list, list, (size_t)nsel * 8, hipMemcpyHostToDevice, c->stream));
  pin_release(c, c->pin_rows);
  if (src.dense)
    hipLaunchKernelGGL(k_witness_partial_multi<NB>, dim3((d / 4 + 255) / 256, G), dim3(256), 0, c->stream, src.dense, d_list, nsel, d, partial);
  else
    hipLaunchKernelGGL(k_witness_partial_multi_prg<NB>, dim3((d / 4 + 255) / 256, G), dim3(256), 0, c->stream, src.seed, d_list, nsel, d, partial);
  HIP_TRY(c, hipGetLastError());
  for (uint32_t b = 0; b < nstmt; b++)
    hipLaunchKernelGGL(k_witness_finish, dim3((d + 255) / 256), dim3(256), 0, c->stream, src.t, partial + (size_t)b * G * d, G, d, h_delta[b],
                       d_w + (size_t)b * d);
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

// rank's share of sum_{bit} v_i as d uint64 lanes, each already reduced mod p (so `world` of them sum without overflow)
int mfh_witness_lanes(mfh_ctx *c, const uint32_t *d_ssp, const uint8_t *h_bits, uint32_t rank, uint32_t world, uint64_t *d_lanes) {
  if (!c || !h_bits || !d_lanes || world == 0 || rank >= world) return MFH_EINVAL;
  HIP_TRY(c, hipSetDevice(c->device));
  mf::SspSrc src;
  if (int rc = ssp_src(c, d_ssp, src)) return rc;
  return witness_partials(c, src, h_bits, rank, world, [&](const uint64_t *partial, uint32_t G) {
    hipLaunchKernelGGL(k_witness_lanes, dim3((c->P.d + 255) / 256), dim3(256), 0, c->stream, partial, G, c->P.d, d_lanes);
  });
}

// w = delta*t + (summed lanes) mod p
int mfh_witness_from_lanes(mfh_ctx *c, const uint32_t *d_ssp, const uint64_t *d_lanes, uint32_t delta, uint32_t *d_w) {
  if (!witness_args_ok(c, 1, 1, d_lanes, &delta, d_w)) return MFH_EINVAL;
  if (int rc = witness_deltas(c, 1, &delta)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  mf::SspSrc src;
  if (int rc = ssp_src(c, d_ssp, src)) return rc;
  hipLaunchKernelGGL(k_witness_finish, dim3((c->P.d + 255) / 256), dim3(256), 0, c->stream, src.t, d_lanes, 1u, c->P.d, delta, d_w);
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

// mfh_witness_poly for up to 256 statements in ONE read (dense SSP) or one generation (generator-defined SSP) of the selected rows, on the
// matrix cores, restricted to the coefficients [col0, col0 + ncols): d_w[b * w_stride + (k - col0)]
int mfh_witness_poly_mm_cols(mfh_ctx *c, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                             uint32_t col0, uint32_t ncols, uint32_t *d_w, size_t w_stride) {
  if (!witness_args_ok(c, nstmt, 256, h_bits, h_delta, d_w)) return MFH_EINVAL;
  mf::SspSrc src;  // d_ssp == NULL: the registered generator-defined SSP (B fragments generated in the kernel)
  if (int rc = ssp_src(c, d_ssp, src)) return rc;
  const uint32_t d = c->P.d, m = c->P.m, nc = ncols;
  if (d % 128 || m < 2) { c->err = "mfh_witness_poly_mm: d must be a multiple of 128"; return MFH_EUNSUPPORTED; }
  if ((uint64_t)col0 + ncols > d || w_stride < ncols) return MFH_EINVAL;
  if (ncols == 0) return MFH_OK;
  if (col0 % 128 || ncols % 128) { c->err = "mfh_witness_poly_mm_cols: the coefficient range must start and end at multiples of 128"; return MFH_EUNSUPPORTED; }
  if (int rc = witness_deltas(c, nstmt, h_delta)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const MmPlan P(c, src.dense != nullptr, nstmt, bits_stride, nc);
  const WCols wc = {col0 / 32, P.ksteps, (uint64_t)w_stride};
  const uint32_t *tpoly = src.t + col0;
  // the SSP in B-fragment order: built on first use per SSP (mfh_ssp_prepare invalidates it), kept beside the uint32 image
  const size_t sfrag_b = (size_t)P.ksteps * 32 * d * 4;
  if (src.dense && (c->ssp_frag_src != d_ssp || c->ssp_frag.cap < sfrag_b)) {
    if (int rc = dev_reserve(c, c->ssp_frag, sfrag_b)) return rc;
    hipLaunchKernelGGL(k_ssp_frag, dim3(P.ksteps * (d / 32)), dim3(256), 0, c->stream, d_ssp, P.nrowsel, d, c->ssp_frag.as<uint32_t>());  // a block per (row step, tile)
    HIP_TRY(c, hipGetLastError());
    c->ssp_frag_src = d_ssp;
  }
  if (int rc = P.ws.reserve(c)) return rc;
  const size_t head_b = P.ws.bytes(MmPlan::HEAD);
  PinBuf &wpin = c->pin_wring[c->pin_wnext++ % 8];
  uint8_t *stage = (uint8_t *)pin_acquire(c, wpin, head_b);
  if (!stage) return MFH_ENOMEM;
  memcpy(stage, h_bits, P.packed);
  uint32_t *cd = (uint32_t *)(stage + P.cd_off);
  for (uint32_t b = 0; b < nstmt; b++) {
    cd[2 * b] = witness_count(h_bits + (size_t)b * bits_stride, m);
    cd[2 * b + 1] = h_delta[b];
  }
  uint8_t *dev = P.ws.at<uint8_t>(c, MmPlan::HEAD);
  HIP_TRY(c, hipMemcpyAsync(dev, stage, head_b, hipMemcpyHostToDevice, c->stream));
  pin_release(c, wpin);
  const uint32_t *d_cd = (const uint32_t *)(dev + P.cd_off), *d_rk = P.ws.at<uint32_t>(c, MmPlan::ROWKEYS);
  const v4i *bitfrag = P.ws.at<v4i>(c, MmPlan::BITFRAG), *sspfrag = c->ssp_frag.as<const v4i>();
  int *d_part = P.ws.at<int>(c, MmPlan::PART);
  hipLaunchKernelGGL(k_witness_bits, dim3((P.ksteps * P.MT * 64 + 255) / 256), dim3(256), 0, c->stream, dev, bits_stride, nstmt, P.nrowsel, P.ksteps, P.MT, (int8_t *)bitfrag);
  if (!src.dense) hipLaunchKernelGGL(k_prg_rowkeys, dim3((P.ksteps * 32 + 255) / 256), dim3(256), 0, c->stream, src.seed, P.ksteps * 32, (uint32_t *)d_rk);
  const dim3 grid(nc / (P.MT == 8 ? 64 : 128), P.ychunks);  // a workgroup: 8 waves on two coefficient tiles (MT = 8), else 4 waves on four
  if (P.MT == 8 && src.dense)
    hipLaunchKernelGGL(k_witness_mm8q, grid, dim3(512), 0, c->stream, sspfrag, bitfrag, P.nrowsel, P.kpc, nc, P.fused ? (int *)nullptr : d_part, tpoly, d_cd, nstmt,
                       d_w, wc);
  else if (P.MT == 8)
    hipLaunchKernelGGL(k_witness_mm8q_prg, grid, dim3(512), 0, c->stream, d_rk, bitfrag, P.nrowsel, P.kpc, nc, d_part, wc);
  else
    with_mt(P.MT, [&](auto mt) {
      constexpr int M = decltype(mt)::value;
      if (src.dense) hipLaunchKernelGGL(k_witness_mm<M>, grid, dim3(256), 0, c->stream, sspfrag, bitfrag, P.nrowsel, P.kpc, nc, d_part, wc);
      else hipLaunchKernelGGL(k_witness_mm_prg<M>, grid, dim3(256), 0, c->stream, d_rk, bitfrag, P.nrowsel, P.kpc, nc, d_part, wc);
    });
  if (!P.fused)
    hipLaunchKernelGGL(k_witness_mm_finish, dim3((nc + 255) / 256, nstmt), dim3(256), 0, c->stream, d_part, P.ychunks, tpoly, d_cd, nstmt, 32 * P.MT, nc, d_w,
                       (uint64_t)w_stride);
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

int mfh_witness_poly_mm(mfh_ctx *c, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta, uint32_t *d_w) {
  if (!witness_args_ok(c, nstmt, 256, h_bits, h_delta, d_w)) return MFH_EINVAL;  // (what mfh_witness_poly_mm_cols checks first, too)
  if (ssp_is_rows(c, d_ssp)) return ssp_rows_witness(c, nstmt, h_bits, bits_stride, h_delta, d_w, c->P.d);  // one interpolation per statement (ssp_rows.hip)
  return mfh_witness_poly_mm_cols(c, d_ssp, nstmt, h_bits, bits_stride, h_delta, 0, c->P.d, d_w, c->P.d);
}

}  // extern "C"
