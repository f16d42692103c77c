// ntt.hpp -- internal: the three 30-bit NTT primes' arithmetic and the CRT back to F_p, shared by poly.hip (the polynomial step) and
// ssp_rows.hip (the subproduct-tree interpolation of the row SSP).  The kernels and the twiddle tables stay in poly.hip (PolyState); the
// blockwise transforms it exposes are declared at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p32.hpp"

struct mfh_ctx;

namespace mf_ntt {

struct NttPrime {
  uint32_t p, ninv, r2;  // modulus, -p^-1 mod 2^32, 2^64 mod p
};
struct Primes3 {
  NttPrime q[3];
};

__host__ __device__ __forceinline__ uint32_t mont_mul(uint32_t a, uint32_t b, uint32_t p, uint32_t ninv) {
  uint64_t t = (uint64_t)a * b;
  uint32_t m = (uint32_t)t * ninv;
  uint32_t u = (uint32_t)((t + (uint64_t)m * p) >> 32);
  return u >= p ? u - p : u;
}
__host__ __device__ __forceinline__ uint32_t add_mod(uint32_t a, uint32_t b, uint32_t p) {
  uint32_t s = a + b;  // p < 2^31: no overflow
  return s >= p ? s - p : s;
}
__host__ __device__ __forceinline__ uint32_t sub_mod(uint32_t a, uint32_t b, uint32_t p) { return a >= b ? a - b : a + p - b; }

struct Crt {
  uint32_t ninv_std[3];  // N^-1 mod p_i (standard form): mont_mul(xR, ninv_std) = x / N in standard form
  uint32_t inv_p1_p2, inv_p1_p3, inv_p2_p3;  // Montgomery form of p1^-1 mod p2, p1^-1 mod p3, p2^-1 mod p3
  uint32_t p1_mod, p1p2_mod;                 // p1 mod p32, p1*p2 mod p32
};
// the three residues of one coefficient (Montgomery form, as an unscaled inverse transform leaves them) -> the coefficient mod p32
__device__ __forceinline__ uint32_t crt_coeff(uint32_t a1, uint32_t a2, uint32_t a3, const Primes3 &P, const Crt &C) {
  const NttPrime q1 = P.q[0], q2 = P.q[1], q3 = P.q[2];
  uint32_t x1 = mont_mul(a1, C.ninv_std[0], q1.p, q1.ninv);
  uint32_t r2 = mont_mul(a2, C.ninv_std[1], q2.p, q2.ninv);
  uint32_t r3 = mont_mul(a3, C.ninv_std[2], q3.p, q3.ninv);
  // Garner: X = x1 + x2 p1 + x3 p1 p2
  uint32_t x1m2 = x1 >= q2.p ? x1 - q2.p : x1;  // x1 < p1 < 2 p2
  uint32_t x2 = mont_mul(sub_mod(r2, x1m2, q2.p), C.inv_p1_p2, q2.p, q2.ninv);
  uint32_t x1m3 = x1 >= q3.p ? x1 - q3.p : x1;
  uint32_t x2m3 = x2 >= q3.p ? x2 - q3.p : x2;
  uint32_t t3 = mont_mul(sub_mod(r3, x1m3, q3.p), C.inv_p1_p3, q3.p, q3.ninv);
  uint32_t x3 = mont_mul(sub_mod(t3, x2m3, q3.p), C.inv_p2_p3, q3.p, q3.ninv);
  uint64_t acc = (uint64_t)red_p32(x1) + red_p32((uint64_t)x2 * C.p1_mod) + red_p32((uint64_t)x3 * C.p1p2_mod);
  return red_p32(acc);
}

}  // namespace mf_ntt

// ---- blockwise transforms over buffers [nb][3][N] (poly.hip): every contiguous 2^logB block of every prime's row independently, in place.
// Forward leaves Montgomery residues in bit-reversed order; inverse takes them back unscaled (x 2^logB), which ntt_crt_make's constants undo.
// (One plan of passes serves these and the polynomial step's own transforms -- poly.hip: ntt_top_passes; logB = log N is a whole transform per polynomial.)
int ntt_reserve(mfh_ctx *c, uint32_t logmax);  // twiddle tables for lengths up to 2^logmax (poly_init; never shrinks)
const mf_ntt::Primes3 &ntt_primes(const mfh_ctx *c);
mf_ntt::Crt ntt_crt_make(const mfh_ctx *c, uint32_t logB);
void ntt_blocks_forward(mfh_ctx *c, uint32_t *buf, uint32_t N, uint32_t logB, uint32_t nb);
void ntt_blocks_inverse(mfh_ctx *c, uint32_t *buf, uint32_t N, uint32_t logB, uint32_t nb);
