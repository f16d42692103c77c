/*
 * test_shim_public.c -- the public-input entry points of libmfuoco_gpu (mfuoco_*_public) through the reference's types at the debug parameters (D = 256, M = 64),
 * each against the reference-signature call it extends, on one entropy tape:
 *   - mfuoco_setup_public makes setup()'s draws: same key, same alpha / beta / s, same CRS except rows v[0..lu), which decrypt to 0;
 *   - mfuoco_prover_public(input) is h, hat_h, hat_v of prover(input) and v_w, b_w of prover(input with the statement bits cleared);
 *   - mfuoco_prover_batch_public is the same composition of two mfuoco_prover_batch calls, statement by statement;
 *   - both _public verifiers accept honest proofs, reject a wrong statement, ignore statement bits at lu and above; the forgery a plain CRS lets through
 *     (prover() on the full input, checked against the all-zero statement) is rejected under the setup_public CRS.
 * Exit code 0 = everything holds.  Needs a GPU.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>
#include <unistd.h>

#include "mfuoco/mangiafuoco_api.h"
#include "test_vc.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

/* the entropy tape of test_shim.c: between tape_start(seed) and tape_stop() getrandom() serves a splitmix64 stream (this definition comes before libc's for the shim too) */
#include <sys/syscall.h>
static int tape_on;
static uint64_t tape_state;
static void tape_start(uint64_t seed) { tape_on = 1; tape_state = seed; }
static void tape_stop(void) { tape_on = 0; }
ssize_t getrandom(void *buf, size_t len, unsigned int flags)
{
  if (!tape_on) return syscall(SYS_getrandom, buf, len, flags);
  uint8_t *p = buf;
  for (size_t i = 0; i < len; i += 8) {
    uint64_t z = (tape_state += 0x9e3779b97f4a7c15UL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9UL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebUL;
    z ^= z >> 31;
    memcpy(p + i, &z, len - i < 8 ? len - i : 8);
  }
  return (ssize_t)len;
}

static int cts_equal(mpz_t *a, mpz_t *b)
{
  for (size_t j = 0; j <= GAMMA_N; j++)
    if (mpz_cmp(a[j], b[j])) return 0;
  return 1;
}
/* pub == (h, hat_h, hat_v of full) + (v_w, b_w of zero) */
static int composed(proof_t pub, proof_t full, proof_t zero)
{
  return cts_equal(pub->h, full->h) && cts_equal(pub->hat_h, full->hat_h) && cts_equal(pub->hat_v, full->hat_v) && cts_equal(pub->v_w, zero->v_w) &&
         cts_equal(pub->b_w, zero->b_w);
}
static void clear_low(mpz_t out, mpz_t in, uint32_t lu)
{
  mpz_set(out, in);
  for (uint32_t i = 0; i < lu; i++) mpz_clrbit(out, i);
}

int main(void)
{
  const uint32_t lu = 10;
  uint8_t *ssp = calloc(1, SSP_SIZE);
  mpz_t input, priv, stmt;
  mpz_inits(input, priv, stmt, NULL);
  do random_ssp(input, ssp); /* (random_ssp draws the input: kept when its statement, the low lu bits, is nonzero) */
  while (mpz_fdiv_ui(input, 1u << lu) == 0);
  clear_low(priv, input, lu);

  /* ---- setup: the same draws; the CRS differs in rows v[0..lu) only, which decrypt to 0 */
  crs_t plain, pub;
  crs_init(plain);
  crs_init(pub);
  memcpy(pub->seed, plain->seed, sizeof plain->seed);
  vrs_t vp, vq;
  tape_start(0x7075620001);
  setup(plain, vp, ssp);
  tape_stop();
  tape_start(0x7075620001);
  mfuoco_setup_public(pub, vq, ssp, lu);
  tape_stop();
  CHECK(vp->alpha == vq->alpha && vp->beta == vq->beta && vp->s == vq->s);
  for (size_t j = 0; j < GAMMA_N; j++) CHECK(!mpz_cmp(vp->sk[j], vq->sk[j]));
  CHECK(!memcmp(plain->s, pub->s, (size_t)GAMMA_D * CT_BYTES) && !memcmp(plain->as, pub->as, (size_t)GAMMA_D * CT_BYTES) && !memcmp(plain->t, pub->t, CT_BYTES));
  CHECK(!memcmp(plain->v[lu], pub->v[lu], (size_t)(GAMMA_M - 1 - lu) * CT_BYTES));
  {
    rng_t rs;
    rng_init(rs, pub->seed);
    mpz_t m;
    mpz_init(m);
    ct_t ct;
    ct_init(ct);
    for (uint32_t i = 0; i < lu; i++) {
      CHECK(memcmp(plain->v[i], pub->v[i], CT_BYTES));
      rng_seek(rs, CTR_BV + (uint64_t)i * CTR_CT);
      ct_import(ct, rs, pub->v[i]);
      regev_decrypt(m, vq->sk, ct);
      CHECK(mpz_sgn(m) == 0);
    }
    ct_clear(ct);
    mpz_clear(m);
    rng_clear(rs);
  }

  /* ---- single prover: the composition identity on one tape, under both CRSs */
  proof_t pp, pf, pz;
  proof_init(pp);
  proof_init(pf);
  proof_init(pz);
  crs_t *crss[2] = { &pub, &plain };
  for (int c = 0; c < 2; c++) {
    struct crs *cr = *crss[c];
    tape_start(0x7075620002 + c);
    mfuoco_prover_public(pp, cr, ssp, input, lu);
    tape_stop();
    tape_start(0x7075620002 + c);
    prover(pf, cr, ssp, input);
    tape_stop();
    tape_start(0x7075620002 + c);
    prover(pz, cr, ssp, priv);
    tape_stop();
    CHECK(composed(pp, pf, pz));
  }

  /* ---- verifiers: honest accepted, a flipped statement bit rejected, bits >= lu ignored; the batch verifier agrees */
  tape_start(0x7075620004);
  mfuoco_prover_public(pp, pub, ssp, input, lu);
  tape_stop();
  CHECK(mfuoco_verifier_public(ssp, vq, pp, input, lu));
  mpz_set(stmt, input);
  mpz_combit(stmt, 0);
  CHECK(!mfuoco_verifier_public(ssp, vq, pp, stmt, lu));
  mpz_set(stmt, input);
  mpz_combit(stmt, lu - 1);
  CHECK(!mfuoco_verifier_public(ssp, vq, pp, stmt, lu));
  mpz_fdiv_r_2exp(stmt, input, lu); /* the statement alone */
  mpz_setbit(stmt, lu + 3);        /* ... and a bit the verifier does not read */
  CHECK(mfuoco_verifier_public(ssp, vq, pp, stmt, lu));
  /* the forgery: prover() on the full input, claimed for the all-zero statement -- accepted under the plain CRS, rejected under setup_public's */
  mpz_set_ui(stmt, 0);
  tape_start(0x7075620005);
  prover(pf, plain, ssp, input);
  tape_stop();
  CHECK(mfuoco_verifier_public(ssp, vp, pf, stmt, lu));
  tape_start(0x7075620005);
  prover(pf, pub, ssp, input);
  tape_stop();
  CHECK(!mfuoco_verifier_public(ssp, vq, pf, stmt, lu));

  /* ---- batch prover: statement k = input with some statement bits flipped (those do not satisfy the SSP); the composition of two mfuoco_prover_batch calls on
   * one tape, and the batch verifier's verdicts */
  enum { NB = 40 };
  proof_t *bp = malloc(NB * sizeof *bp), *bf = malloc(NB * sizeof *bf), *bz = malloc(NB * sizeof *bz);
  mpz_t *in = malloc(NB * sizeof *in), *inz = malloc(NB * sizeof *inz);
  for (int k = 0; k < NB; k++) {
    proof_init(bp[k]);
    proof_init(bf[k]);
    proof_init(bz[k]);
    mpz_init_set(in[k], input);
    if (k % 3 == 1) mpz_combit(in[k], k % lu);
    mpz_init(inz[k]);
    clear_low(inz[k], in[k], lu);
  }
  tape_start(0x7075620006);
  mfuoco_prover_batch_public(bp, pub, ssp, in, NB, lu);
  tape_stop();
  tape_start(0x7075620006);
  mfuoco_prover_batch(bf, pub, ssp, in, NB);
  tape_stop();
  tape_start(0x7075620006);
  mfuoco_prover_batch(bz, pub, ssp, inz, NB);
  tape_stop();
  uint8_t ok[NB];
  mfuoco_verifier_batch_public(ssp, vq, bp, in, NB, lu, ok);
  for (int k = 0; k < NB; k++) {
    CHECK(composed(bp[k], bf[k], bz[k]));
    CHECK(ok[k] == (k % 3 != 1));
    CHECK(mfuoco_verifier_public(ssp, vq, bp[k], in[k], lu) == (k % 3 != 1));
  }
  /* each batch proof against statement 0's input: the flipped ones are now checked against a statement they were not made for */
  mpz_t *same = malloc(NB * sizeof *same);
  for (int k = 0; k < NB; k++) mpz_init_set(same[k], input);
  mfuoco_verifier_batch_public(ssp, vq, bp, same, NB, lu, ok);
  for (int k = 0; k < NB; k++) CHECK(ok[k] == (k % 3 != 1));

  /* ---- the checks of the public verifiers on crafted proofs: for the all-zero statement, all lu bits and one bit, v_s = v_0(s) + the statement's v_i(s) + w_s from
   * verification-key values computed here by Horner; all 16 sets of failing checks at w_s = 777 and at the w_s that makes v_s = 0 */
  {
    enum { NS = 3, NV = NS * 32 };
    uint64_t vk[2 + 10];
    CHECK(lu <= 10);
    vk[0] = vc_horner(ssp + ssp_t_offset, vq->s);
    for (uint32_t i = 0; i <= lu; i++) vk[1 + i] = vc_horner(ssp + ssp_v_offset(i), vq->s);
    CHECK(vk[0] != 0);
    const uint64_t sbits[NS] = { 0, (1u << lu) - 1, 1u << 3 };
    proof_t *pv = malloc(NV * sizeof *pv);
    mpz_t *st = malloc(NV * sizeof *st);
    uint8_t want[NV], okv[NV];
    for (int k = 0; k < NV; k++) {
      const int fail = k & 15;
      const uint64_t u = sbits[k >> 5];
      uint64_t base = vk[1];
      for (uint32_t i = 0; i < lu; i++)
        if ((u >> i) & 1) base = (base + vk[2 + i]) % GAMMA_P;
      const uint64_t w_s = (k >> 4) & 1 ? (GAMMA_P - base) % GAMMA_P : 777, v_s = (base + w_s) % GAMMA_P;
      uint64_t x[5];
      vc_values(x, fail, w_s, v_s, vk[0], vq->alpha, vq->beta);
      want[k] = (uint8_t)vc_expect(x, v_s, vk[0], vq->alpha, vq->beta);
      CHECK(want[k] == (fail == 0));
      proof_init(pv[k]);
      vc_proof(pv[k], x, 5 * (uint64_t)k);
      mpz_init_set_ui(st[k], u);
      CHECK(mfuoco_verifier_public(ssp, vq, pv[k], st[k], lu) == (want[k] != 0));
    }
    memset(okv, 9, sizeof okv);
    mfuoco_verifier_batch_public(ssp, vq, pv, st, NV, lu, okv);
    for (int k = 0; k < NV; k++) CHECK(okv[k] == want[k]);
    /* the accepted proof of each statement under another one: the sums differ (v_4(s) != 0), the second eq-pke line and eq-div fail */
    CHECK(vk[2 + 3] != 0);
    CHECK(!mfuoco_verifier_public(ssp, vq, pv[0], st[64], lu) && !mfuoco_verifier_public(ssp, vq, pv[64], st[0], lu));
    for (int k = 0; k < NV; k++) { proof_clear(pv[k]); mpz_clear(st[k]); }
    free(pv); free(st);
    puts("public verifier checks ok");
  }

  for (int k = 0; k < NB; k++) {
    proof_clear(bp[k]);
    proof_clear(bf[k]);
    proof_clear(bz[k]);
    mpz_clears(in[k], inz[k], same[k], NULL);
  }
  free(bp); free(bf); free(bz); free(in); free(inz); free(same);
  proof_clear(pp);
  proof_clear(pf);
  proof_clear(pz);
  crs_clear(plain);
  crs_clear(pub);
  mpz_clears(input, priv, stmt, NULL);
  free(ssp);
  printf("test_shim_public: ok (lu = %u)\n", lu);
  return 0;
}
