// p32.hpp -- internal: arithmetic modulo p = MFH_P = 2^32 - 5, the SNARK's field, on host and device (2^32 = 5 mod p).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfhip.h"

constexpr uint32_t P32 = MFH_P;

// x mod p for x < 2^64
__host__ __device__ __forceinline__ uint32_t red_p32(uint64_t x) {
  x = (x >> 32) * 5 + (uint32_t)x;  // < 5*2^32 + 2^32
  x = (x >> 32) * 5 + (uint32_t)x;  // < 30 + 2^32
  if (x >= P32) x -= P32;
  if (x >= P32) x -= P32;
  return (uint32_t)x;
}
// a 64-bit product folded once: < 6 * 2^32, so 2^29 of them sum in a uint64
__host__ __device__ __forceinline__ uint64_t fold1(uint64_t x) { return (x >> 32) * 5 + (uint32_t)x; }
__host__ __device__ __forceinline__ uint32_t mulp(uint32_t a, uint32_t b) { return red_p32((uint64_t)a * b); }

inline uint32_t powp(uint32_t a, uint64_t e) {
  uint32_t r = 1;
  for (; e; e >>= 1, a = mulp(a, a))
    if (e & 1) r = mulp(r, a);
  return r;
}
inline uint32_t invp(uint32_t a) { return powp(a, P32 - 2); }  // (a != 0)
