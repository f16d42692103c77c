// sha256_dev.hpp -- one SHA-256 compression (FIPS 180-4 6.2.2) and the padded blocks of a whole message (5.1.1) for the kernels of merkle.hip.
//
// sha256_compress is host and device code: a plain C++ compiler takes this header as it stands (tests/sha256_host_check.cpp), so the rounds, the
// message schedule and the constants are checked on a CPU.  The device pass writes the rotations as v_alignbit_b32 and the three-input Boolean
// functions as one v_bitop3_b32 each (the truth-table byte: bit (a << 2 | b << 1 | c) of it is f(a, b, c), as in aes_dev.hpp):
//   0x96  a ^ b ^ c          the three-way XORs of Sigma0, Sigma1, sigma0, sigma1
//   0xCA  a ? b : c          Ch
//   0xE8  majority           Maj
// hipcc forms only a third of these by itself from ^ & ~ (121 v_bitop3 of 352, 1 795 instructions a compression against 1 466).  The host pass
// uses the plain expressions; the three truth tables are device-only and pinned by the GPU tests of the tree.
// Fully unrolled: a 16-word rolling schedule in registers, the 64 round constants as literals, no table, no LDS, no scratch.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MF_SHA_HD __host__ __device__ __forceinline__
#else
#define MF_SHA_HD inline
#endif

namespace mf {

#if defined(__HIP_DEVICE_COMPILE__)
#define MF_SHA_ROTR(x, n) __builtin_amdgcn_alignbit((x), (x), (n))
#define MF_SHA_XOR3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)
#define MF_SHA_CH(e, f, g) __builtin_amdgcn_bitop3_b32((e), (f), (g), 0xCA)
#define MF_SHA_MAJ(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0xE8)
#else
#define MF_SHA_ROTR(x, n) (((x) >> (n)) | ((x) << (32 - (n))))
#define MF_SHA_XOR3(a, b, c) ((a) ^ (b) ^ (c))
#define MF_SHA_CH(e, f, g) (((e) & (f)) ^ (~(e) & (g)))
#define MF_SHA_MAJ(a, b, c) (((a) & (b)) ^ ((a) & (c)) ^ ((b) & (c)))
#endif

// one round with the working variables where they stand (the caller rotates the names, not the registers)
#define MF_SHA_ROUND(a, b, c, d, e, f, g, h, k, wt)                                                                                              \
  do {                                                                                                                                           \
    const uint32_t t1_ = (h) + MF_SHA_XOR3(MF_SHA_ROTR((e), 6), MF_SHA_ROTR((e), 11), MF_SHA_ROTR((e), 25)) + MF_SHA_CH((e), (f), (g)) + (k) + (wt); \
    const uint32_t t2_ = MF_SHA_XOR3(MF_SHA_ROTR((a), 2), MF_SHA_ROTR((a), 13), MF_SHA_ROTR((a), 22)) + MF_SHA_MAJ((a), (b), (c));              \
    (d) += t1_;                                                                                                                                  \
    (h) = t1_ + t2_;                                                                                                                             \
  } while (0)
// W_t for t >= 16, in place of W_{t-16}: w[t & 15] += sigma1(W_{t-2}) + W_{t-7} + sigma0(W_{t-15})
#define MF_SHA_SCHED(w, t)                                                                                                     \
  ((w)[(t) & 15] += MF_SHA_XOR3(MF_SHA_ROTR((w)[((t) - 2) & 15], 17), MF_SHA_ROTR((w)[((t) - 2) & 15], 19), (w)[((t) - 2) & 15] >> 10) + \
                    (w)[((t) - 7) & 15] +                                                                                      \
                    MF_SHA_XOR3(MF_SHA_ROTR((w)[((t) - 15) & 15], 7), MF_SHA_ROTR((w)[((t) - 15) & 15], 18), (w)[((t) - 15) & 15] >> 3))
// eight rounds t .. t + 7: after them the names a .. h are back in place
#define MF_SHA_8(t, k0, k1, k2, k3, k4, k5, k6, k7)          \
  do {                                                       \
    MF_SHA_ROUND(a, b, c, d, e, f, g, h, k0, MF_SHA_W(t));     \
    MF_SHA_ROUND(h, a, b, c, d, e, f, g, k1, MF_SHA_W(t + 1)); \
    MF_SHA_ROUND(g, h, a, b, c, d, e, f, k2, MF_SHA_W(t + 2)); \
    MF_SHA_ROUND(f, g, h, a, b, c, d, e, k3, MF_SHA_W(t + 3)); \
    MF_SHA_ROUND(e, f, g, h, a, b, c, d, k4, MF_SHA_W(t + 4)); \
    MF_SHA_ROUND(d, e, f, g, h, a, b, c, k5, MF_SHA_W(t + 5)); \
    MF_SHA_ROUND(c, d, e, f, g, h, a, b, k6, MF_SHA_W(t + 6)); \
    MF_SHA_ROUND(b, c, d, e, f, g, h, a, k7, MF_SHA_W(t + 7)); \
  } while (0)

// the initial hash value (FIPS 180-4 5.3.3)
#define MF_SHA256_IV {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u}

// state <- compress(state, block): state = eight words, block = the sixteen big-endian words of the 64 bytes, as values.  block is overwritten (it is the
// rolling schedule).
MF_SHA_HD void sha256_compress(uint32_t state[8], uint32_t w[16]) {
  uint32_t a = state[0], b = state[1], c = state[2], d = state[3], e = state[4], f = state[5], g = state[6], h = state[7];
#define MF_SHA_W(t) w[(t) & 15]
  MF_SHA_8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u);
  MF_SHA_8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u);
#undef MF_SHA_W
#define MF_SHA_W(t) MF_SHA_SCHED(w, (t))
  MF_SHA_8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau);
  MF_SHA_8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u);
  MF_SHA_8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u);
  MF_SHA_8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u);
  MF_SHA_8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u);
  MF_SHA_8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u);
#undef MF_SHA_W
  state[0] += a; state[1] += b; state[2] += c; state[3] += d; state[4] += e; state[5] += f; state[6] += g; state[7] += h;
}

// ---- whole messages: the padded blocks of FIPS 180-4 5.1.1 (message, 0x80, zeros, the bit length as 8 big-endian bytes), one word at a time.  Host and
// device code like sha256_compress; tests/sha256_records_host_check.cpp runs the host pass on exact-fit heap messages under ASan, which is the bound on
// what sha256_block_word reads.  length < 2^32 bytes (the kernel of merkle.hip takes at most 2^20).

// the number of 64-byte blocks of a padded `length`-byte message
MF_SHA_HD uint32_t sha256_blocks(uint32_t length) { return (uint32_t)(((uint64_t)length + 9 + 63) / 64); }

// word t of padded block b, given `data` = the big-endian word of the four bytes at message offset 64 b + 4 t: the bytes of `data` at offsets >= length
// are ignored (whatever they hold), so the padding comes from `length` alone
MF_SHA_HD uint32_t sha256_pad_word(uint32_t data, uint32_t length, uint32_t b, uint32_t t) {
  const uint64_t off = (uint64_t)64 * b + 4 * t;
  uint32_t v = 0;
  if (off + 4 <= length) {
    v = data;
  } else if (off <= length) {  // k = 0 .. 3 message bytes, then 0x80
    const uint32_t k = (uint32_t)(length - off);
    v = (k ? data & (0xFFFFFFFFu << (32 - 8 * k)) : 0u) | (0x80u << (24 - 8 * k));
  }
  if (b + 1 == sha256_blocks(length)) {  // the last block ends with the bit length; 0x80 lies before its word 14
    if (t == 14) v |= length >> 29;
    if (t == 15) v |= length << 3;
  }
  return v;
}

// word t of padded block b of the `length`-byte message at msg: reads no byte outside [msg, msg + length)
MF_SHA_HD uint32_t sha256_block_word(const uint8_t *msg, uint32_t length, uint32_t b, uint32_t t) {
  const uint64_t off = (uint64_t)64 * b + 4 * t;
  uint32_t data = 0;
  for (uint32_t k = 0; k < 4; k++)
    if (off + k < length) data |= (uint32_t)msg[off + k] << (24 - 8 * k);
  return sha256_pad_word(data, length, b, t);
}

#undef MF_SHA_8
#undef MF_SHA_SCHED
#undef MF_SHA_ROUND
#undef MF_SHA_MAJ
#undef MF_SHA_CH
#undef MF_SHA_XOR3
#undef MF_SHA_ROTR

}  // namespace mf
