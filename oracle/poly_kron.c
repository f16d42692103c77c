/*
 * poly_kron.c -- an exact reference for products and Euclidean quotients in F_p[x], p = 2^32 - 5, at any length the GPU path runs.
 *
 * TEST INFRASTRUCTURE ONLY.  Linked into libmf_gmpcheck.so beside gmp_check.c.  Nothing here comes from the reference: it is GMP plus the
 * definition of polynomial division.
 *
 *   pk_poly_mul_modp   c = a b: Kronecker substitution.  Every coefficient goes into a 128-bit slot of one integer; a single mpz_mul gives
 *                      the integer product; each slot of it IS one coefficient of the integer convolution (below 2^32 * 2^32 * min(la, lb)
 *                      < 2^128, so no slot carries into the next), reduced mod p afterwards.
 *   pk_poly_div_certify  is q the Euclidean quotient of A = v^2 - 1 by t?  R = A - q t must have deg R < deg t and deg q <= deg A - deg t.
 *                      Euclidean division is unique, so the answer does not depend on how q was computed.
 *   pk_poly_div        the quotient itself (all of it), by Newton inversion of rev(t); certified before it is returned.
 *
 * Coefficients cross the boundary as uint32 arrays (canonical residues mod p: inputs above p are taken as integers and reduced with the product).
 * None of these take the Python GIL (they are called through ctypes.CDLL).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <gmp.h>

#define PK_P 0xfffffffbULL

#if GMP_NUMB_BITS != 64
#error "poly_kron.c packs two 64-bit limbs per 128-bit slot"
#endif

typedef unsigned __int128 u128;

static size_t trim(const uint32_t *a, size_t n)
{
  while (n && !a[n - 1]) n--;
  return n;
}

static void pack(mpz_t z, const uint32_t *a, size_t n)
{
  n = trim(a, n);
  if (!n) {
    mpz_set_ui(z, 0);
    return;
  }
  mp_limb_t *d = mpz_limbs_write(z, (mp_size_t)(2 * n));
  for (size_t i = 0; i < n; i++) {
    d[2 * i] = a[i];
    d[2 * i + 1] = 0;
  }
  mpz_limbs_finish(z, (mp_size_t)(2 * n));
}

static uint64_t powmod(uint64_t a, uint64_t e)
{
  uint64_t r = 1;
  a %= PK_P;
  while (e) {
    if (e & 1) r = (uint64_t)((u128)r * a % PK_P);
    a = (uint64_t)((u128)a * a % PK_P);
    e >>= 1;
  }
  return r;
}

/* c[0 .. la + lb - 1) = a b mod p.  Returns 0, or -1 for an empty operand / allocation failure. */
int pk_poly_mul_modp(const uint32_t *a, size_t la, const uint32_t *b, size_t lb, uint32_t *c)
{
  if (!la || !lb) return -1;
  const size_t lc = la + lb - 1;
  memset(c, 0, lc * 4);
  mpz_t x, y;
  mpz_init(x);
  pack(x, a, la);
  if (a == b && la == lb) {
    mpz_mul(x, x, x); /* GMP squares when both operands are the same number */
  } else {
    mpz_init(y);
    pack(y, b, lb);
    mpz_mul(x, x, y);
    mpz_clear(y);
  }
  const size_t sz = mpz_size(x);
  const mp_limb_t *d = mpz_limbs_read(x);
  for (size_t i = 0; 2 * i < sz && i < lc; i++) {
    const u128 s = ((u128)(2 * i + 1 < sz ? d[2 * i + 1] : 0) << 64) | d[2 * i];
    c[i] = (uint32_t)(s % PK_P);
  }
  mpz_clear(x);
  return 0;
}

/* A = v^2 - 1 in F_p[x]: writes 2 lv - 1 coefficients, returns its length after trimming (0 for the zero polynomial) */
static size_t square_minus_one(const uint32_t *v, size_t lv, uint32_t *A)
{
  pk_poly_mul_modp(v, lv, v, lv, A);
  A[0] = A[0] ? A[0] - 1 : (uint32_t)(PK_P - 1);
  return trim(A, 2 * lv - 1);
}

static int certify_A(const uint32_t *A, size_t nA, const uint32_t *t, size_t nt, const uint32_t *q, size_t lq)
{
  const size_t nq = trim(q, lq);
  if (nA < nt) return nq == 0; /* deg A < deg t (or A = 0): the quotient is 0 */
  if (nq > nA - nt + 1) return 0; /* deg q > deg A - deg t */
  if (!nq) {                      /* R = A: deg A >= deg t */
    return 0;
  }
  uint32_t *qt = malloc((nq + nt - 1) * 4);
  if (!qt) return -1;
  pk_poly_mul_modp(q, nq, t, nt, qt);
  int ok = 1;
  /* R = A - q t: every coefficient at index >= deg t must vanish (deg(q t) <= deg A, so q t has no coefficient above A's) */
  for (size_t i = nt - 1; i < nA && ok; i++) {
    const uint32_t y = i < nq + nt - 1 ? qt[i] : 0u;
    ok = A[i] == y;
  }
  free(qt);
  return ok;
}

/* 1 iff q (lq coefficients, trailing zeros allowed) is the Euclidean quotient of v^2 - 1 by t; 0 if not; -1 for t = 0 or no memory */
int pk_poly_div_certify(const uint32_t *v, size_t lv, const uint32_t *t, size_t lt, const uint32_t *q, size_t lq)
{
  const size_t nt = trim(t, lt);
  if (!nt || !lv) return -1;
  uint32_t *A = malloc((2 * lv - 1) * 4);
  if (!A) return -1;
  const size_t nA = square_minus_one(v, lv, A);
  const int ok = certify_A(A, nA, t, nt, q, lq);
  free(A);
  return ok;
}

/* The Euclidean quotient of v^2 - 1 by t into q (room for 2 lv - 1 coefficients; zero filled above the quotient).  Returns its length
 * deg A - deg t + 1 (0 when deg A < deg t); -1 for t = 0 or no memory; -2 if the result fails pk_poly_div_certify (a bug of this file). */
long pk_poly_div(const uint32_t *v, size_t lv, const uint32_t *t, size_t lt, uint32_t *q)
{
  const size_t nt = trim(t, lt);
  if (!nt || !lv) return -1;
  memset(q, 0, (2 * lv - 1) * 4);
  uint32_t *A = malloc((2 * lv - 1) * 4);
  if (!A) return -1;
  const size_t nA = square_minus_one(v, lv, A);
  long ret = 0;
  if (nA >= nt) {
    const size_t n = nA - nt + 1; /* quotient length */
    const size_t lf = nt < n ? nt : n;
    /* f = rev(t)[:n], g = f^-1 mod x^n by Newton: g <- g (2 - f g) mod x^2k */
    uint32_t *f = malloc(lf * 4), *g = calloc(n, 4), *e = malloc(2 * n * 4), *w = malloc(2 * n * 4);
    if (!f || !g || !e || !w) {
      free(f); free(g); free(e); free(w); free(A);
      return -1;
    }
    for (size_t i = 0; i < lf; i++) f[i] = t[nt - 1 - i];
    g[0] = (uint32_t)powmod(f[0], PK_P - 2);
    for (size_t k = 1; k < n;) {
      const size_t k2 = 2 * k < n ? 2 * k : n;
      const size_t lff = lf < k2 ? lf : k2;
      pk_poly_mul_modp(f, lff, g, k, e); /* lff + k - 1 coefficients */
      for (size_t i = lff + k - 1; i < k2; i++) e[i] = 0;
      for (size_t i = 0; i < k2; i++) e[i] = e[i] ? (uint32_t)(PK_P - e[i]) : 0u; /* 2 - e */
      e[0] = (uint32_t)((e[0] + 2ULL) % PK_P);
      pk_poly_mul_modp(g, k, e, k2, w);
      memcpy(g, w, k2 * 4);
      k = k2;
    }
    /* rev(q) = rev(A)[:n] g mod x^n */
    for (size_t i = 0; i < n; i++) e[i] = A[nA - 1 - i];
    pk_poly_mul_modp(e, n, g, n, w);
    for (size_t i = 0; i < n; i++) q[i] = w[n - 1 - i];
    ret = (long)n;
    free(f); free(g); free(e); free(w);
  }
  const int ok = certify_A(A, nA, t, nt, q, 2 * lv - 1);
  free(A);
  return ok == 1 ? ret : ok < 0 ? -1 : -2;
}
