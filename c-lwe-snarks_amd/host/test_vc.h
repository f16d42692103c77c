/*
 * test_vc.h -- shared by test_shim.c and test_shim_public.c: proofs built by construction for the shim's verifiers, and the verdict they must give.
 * Include after mfuoco/mangiafuoco_api.h.
 */
#ifndef MFUOCO_TEST_VC_H
#define MFUOCO_TEST_VC_H
#include <string.h>

/* verifier()'s four checks (src/snark.c:219-235) on proofs built by construction: with a = 0 a ciphertext decrypts to b mod p (regev_decrypt, src/lwe.c:105-111), so any
 * five field elements can be put in front of them -- each check failing alone and in every combination, which no proof made by prover() does.  The expected verdict is
 * written out below in unsigned __int128 arithmetic; nothing of it calls the shim. */
static uint64_t vc_mul(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % GAMMA_P); }
static uint64_t vc_horner(const uint8_t *slot, uint64_t x)
{ /* one slot of the SSP file layout: GAMMA_D little-endian uint64 coefficients, lowest first */
  uint64_t r = 0;
  for (size_t i = GAMMA_D; i-- > 0;) {
    uint64_t c;
    memcpy(&c, slot + 8 * i, 8);
    r = (vc_mul(r, x) + c % GAMMA_P) % GAMMA_P;
  }
  return r;
}
static uint64_t vc_inv(uint64_t a)
{ /* a^(p - 2) */
  uint64_t r = 1;
  for (uint64_t e = GAMMA_P - 2; e; e >>= 1, a = vc_mul(a, a))
    if (e & 1) r = vc_mul(r, a);
  return r;
}
/* x = h_s, hath_s, hatv_s, w_s, b_s for which exactly the checks in the mask `fail` do not hold (bit 0: first eq-pke, 1: second eq-pke, 2: eq-div, 3: eq-lin): the
 * right value, or the right value plus 1 */
static void vc_values(uint64_t x[5], int fail, uint64_t w_s, uint64_t v_s, uint64_t t_s, uint64_t alpha, uint64_t beta)
{
  x[0] = (vc_mul((vc_mul(v_s, v_s) + GAMMA_P - 1) % GAMMA_P, vc_inv(t_s)) + ((fail >> 2) & 1)) % GAMMA_P;
  x[1] = (vc_mul(x[0], alpha) + (fail & 1)) % GAMMA_P;
  x[2] = (vc_mul(v_s, alpha) + ((fail >> 1) & 1)) % GAMMA_P;
  x[3] = w_s;
  x[4] = (vc_mul(w_s, beta) + ((fail >> 3) & 1)) % GAMMA_P;
}
static int vc_expect(const uint64_t x[5], uint64_t v_s, uint64_t t_s, uint64_t alpha, uint64_t beta)
{
  const unsigned __int128 P = GAMMA_P;
  if ((unsigned __int128)x[0] * alpha % P != x[1]) return 0;                                            /* eq-pke */
  if ((unsigned __int128)v_s * alpha % P != x[2]) return 0;
  if (((unsigned __int128)v_s * v_s + P * P - 1 - (unsigned __int128)x[0] * t_s) % P != 0) return 0;    /* eq-div: v_s^2 - 1 - h_s t(s) = 0 */
  if ((unsigned __int128)x[3] * beta % P != x[4]) return 0;                                             /* eq-lin */
  return 1;
}
/* a = 0, b = value + (2^600 + k) p */
static void vc_craft(mpz_t *ct, uint64_t value, uint64_t k)
{
  for (size_t j = 0; j < GAMMA_N; j++) mpz_set_ui(ct[j], 0);
  mpz_set_ui(ct[GAMMA_N], 1);
  mpz_mul_2exp(ct[GAMMA_N], ct[GAMMA_N], 600);
  mpz_add_ui(ct[GAMMA_N], ct[GAMMA_N], k);
  mpz_mul_ui(ct[GAMMA_N], ct[GAMMA_N], GAMMA_P);
  mpz_add_ui(ct[GAMMA_N], ct[GAMMA_N], value);
}
static void vc_proof(proof_t pi, const uint64_t x[5], uint64_t k)
{
  vc_craft(pi->h, x[0], k);
  vc_craft(pi->hat_h, x[1], k + 1);
  vc_craft(pi->hat_v, x[2], k + 2);
  vc_craft(pi->v_w, x[3], k + 3);
  vc_craft(pi->b_w, x[4], k + 4);
}

#endif
