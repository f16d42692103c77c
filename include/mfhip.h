/*
 * mfhip.h -- C ABI of the MI355X-native LWE/SSP-SNARK prover core (libmfhip.so).
 *
 * This is the drop-in boundary for the hot path of mmaker/c-lwe-snarks ("mangiafuoco"):
 * every entry point is `extern "C"`, takes plain pointers and sizes, and cites the reference
 * interface it replaces (file:line relative to the reference tree).  The reference API is
 * one-ciphertext-at-a-time over GMP `mpz_t`; these are the batched, dense-limb equivalents that
 * the reference-signature shim (c-lwe-snarks_amd/host/) calls underneath.
 *
 * Data conventions
 *   value      : L = ceil(logq/64) little-endian uint64 limbs (12 @ logq=736, 23 @ 1472).  Results are
 *                reduced the way the reference's modq() reduces (src/lwe.h:107-118): only the low
 *                K = logq/64 limbs survive (effective modulus 2^704 @ 736, 2^1472 @ 1472).
 *   ciphertext : (n+1) values, coordinate-major: ct[j*L .. j*L+L), j = n is `b`   (ct_t, src/lwe.h:44)
 *   c8         : CT_BYTES = logq/8 little-endian bytes of `b` per ciphertext       (ct_export, src/lwe.c:115-119)
 *   seed       : 40 bytes: [0,8) nonce, [8,40) AES-256 key                         (rseed_t, src/entropy.h:35)
 *   stream     : byte x of the public stream = byte (x&15) of AES256_K(nonce_le64 || le64(x>>4))
 *                (src/aes.c:104-144, src/entropy.c:46-61)
 *   Pointers named d_* are DEVICE pointers (HBM); h_* are host pointers.  All launches go to the
 *   context's HIP stream and are asynchronous unless stated; mfh_sync() waits.
 *
 * Threading: like the reference (no function of which is re-entrant w.r.t. a shared rng_t), a context is NOT thread-safe; use
 * one context per thread / per GPU.  Different contexts are independent.
 *
 * Error behaviour: the reference API is void and asserts preconditions (debug builds only).  Here every
 * function returns 0 on success or a negative MFH_E* code; mfh_last_error() gives the text.  There is no
 * CPU fallback anywhere in the library: without a usable HIP device mfh_ctx_create fails.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFH_P 0xfffffffbu /* GAMMA_P, src/lwe.h:25 */

enum {
  MFH_OK = 0,
  MFH_EINVAL = -1,  /* bad argument (the reference would assert or misbehave) */
  MFH_EDEVICE = -2, /* HIP runtime error / no device */
  MFH_ENOMEM = -3,
  MFH_EUNSUPPORTED = -4 /* parameter set not compiled in (logq must be 736 or 1472) */
};

typedef struct {
  uint32_t n;    /* GAMMA_N,    src/lwe.h:23 (1470) */
  uint32_t logq; /* GAMMA_LOGQ, src/lwe.h:24 (736; 1472 for the doubled-modulus stress config) */
  uint32_t d;    /* GAMMA_D,    src/lwe.h:15,19 */
  uint32_t m;    /* GAMMA_M,    src/lwe.h:17,20 */
} mfh_params;

typedef struct mfh_ctx mfh_ctx;

/* ---- context ------------------------------------------------------------------------------------ */
int mfh_ctx_create(mfh_ctx **out, int device, const mfh_params *P);
void mfh_ctx_destroy(mfh_ctx *ctx);
/* run on an existing hipStream_t (e.g. torch's current stream).  NULL means HIP's default (null) stream,
 * NOT the context's own stream (a fresh context runs on its own non-blocking stream until this is called).
 * Switching rule: the context's scratch, pinned staging and side-stream events are ordered by the stream the previous calls ran on, so the caller
 * waits for the context's work (mfh_sync, or its own wait on the old stream) BEFORE it switches; calls queued on the new stream otherwise race the
 * ones still running on the old.  The one exception is mfh_sample_rows, which orders its kept buffer across streams itself: a switch may follow it at once. */
int mfh_set_stream(mfh_ctx *ctx, void *hip_stream);
int mfh_sync(mfh_ctx *ctx);
/* The prover entry points stage what the host contributes -- witness bits, deltas (src/snark.c:140) and the smudging terms u p (src/lwe.c:65-76) -- in pinned host
 * buffers the context keeps.  This waits for their copies and zeroes them: a caller whose proofs must stay zero-knowledge against a later reader of its memory calls
 * it when the proofs are out (the shim's prover() / mfuoco_prover_batch() do; the reference, single-threaded on the CPU, leaves delta and u in freed mpz limbs). */
int mfh_scrub_staging(mfh_ctx *ctx);
const char *mfh_last_error(const mfh_ctx *ctx);
/* rng_init (src/entropy.c:58-61) + aesctr_init (src/aes.c:49-95): expand the AES-256 key of `seed`
 * and make it the context's current public stream. */
int mfh_set_seed(mfh_ctx *ctx, const uint8_t h_seed[40]);

/* ---- L0/L1: keystream and sampler ---------------------------------------------------------------- */
/* rng_seek + rng_gen / aesctr_prg (src/entropy.c:46-56, src/aes.c:104-144): bytes [off, off+nbytes)
 * of the current stream into d_out. */
int mfh_keystream(mfh_ctx *ctx, uint64_t off, void *d_out, size_t nbytes);
/* mpz2_urandommv(c, rs, GAMMA_LOGQ, GAMMA_N) for `nrows` consecutive ciphertext rows starting at stream
 * offset `off` (src/entropy.h:62-66, src/lwe.c:90,101,124): d_out[row][j][L] limbs, j < n, masked to logq bits. */
int mfh_sample_rows(mfh_ctx *ctx, uint64_t off, size_t nrows, uint64_t *d_out);

/* ---- L2: ciphertext algebra ---------------------------------------------------------------------- */
/* ct_add / ct_mul_ui / ct_addmul_ui on `count` ciphertexts (src/lwe.c:131-157).  In-place allowed. */
int mfh_ct_add(mfh_ctx *ctx, uint64_t *d_rop, const uint64_t *d_a, const uint64_t *d_b, size_t count);
int mfh_ct_mul_ui(mfh_ctx *ctx, uint64_t *d_rop, const uint64_t *d_a, uint32_t b, size_t count);
int mfh_ct_addmul_ui(mfh_ctx *ctx, uint64_t *d_rop, const uint64_t *d_a, uint32_t b, size_t count);

/* eval_poly (src/lwe.c:176-186), fused over one or two coefficient vectors:
 *   rop_k (+)= sum_{i<nrows} coeff_k[i] * Import(c8[i])   with the stream pre-seeked to `off`
 * i.e. row i is expanded from stream bytes [off + i*n*CT_BYTES, ...) exactly as ct_import does
 * (src/lwe.c:122-126), once, and multiply-accumulated into both outputs.  Rows whose coefficients are
 * all zero are not expanded (the reference expands them only to advance its stream).
 * d_coeff1/d_rop1 may be NULL.  accumulate != 0 keeps the previous contents of d_rop* (the reference
 * always accumulates into rop); 0 overwrites.  Coefficients must be < p (the reference asserts). */
int mfh_eval_rows(mfh_ctx *ctx, uint64_t off, size_t nrows, const uint8_t *d_c8, const uint32_t *d_coeff0,
                  const uint32_t *d_coeff1, uint64_t *d_rop0, uint64_t *d_rop1, int accumulate);

/* ---- resident (materialised) CRS: SURVEY 8(d)'s second regime ---------------------------------------------------
 * The reference regenerates the a-vectors of every CRS row from the seed on every use (ct_import, src/lwe.c:122-126).
 * With 288 GB of HBM they can instead be expanded ONCE (11.3 GB for the default CRS) and streamed at HBM speed:
 * mfh_crs_expand writes rows [off/CTR_CT ...) in a limb-plane layout (mfh_resident_row_bytes() per row: only the words that
 * survive modq, coordinate n = the row's b); mfh_eval_rows_resident is eval_poly over rows [first_row, first_row+nrows)
 * of such an image (coefficient i belongs to row first_row + i).  mfh_crs_set_resident(ctx, image) makes
 * mfh_prove / mfh_prove_partial use the image (row index = position in stream order from CTR_S); NULL reverts. */
size_t mfh_resident_row_bytes(const mfh_ctx *ctx);
int mfh_crs_expand(mfh_ctx *ctx, uint64_t off, size_t nrows, const uint8_t *d_c8, void *d_rows_out);
/* d_c8 may be NULL in mfh_crs_expand: the a parts only (they depend on the seed alone, not on the ciphertexts), coordinate n left zero -- so that the 12 ms of AES can run
 * BEFORE the b's exist (the shim's setup() queues it beside the SSP upload); mfh_crs_image_set_b then fills coordinate n of rows [first_row, first_row + nrows)
 * of the image from their compressed ciphertexts (d_c8[0] = row first_row).  Expanding with d_c8 gives the same bytes as expanding without and setting b afterwards. */
int mfh_crs_image_set_b(mfh_ctx *ctx, size_t first_row, size_t nrows, const uint8_t *d_c8, void *d_rows);
int mfh_eval_rows_resident(mfh_ctx *ctx, const void *d_rows, size_t first_row, size_t nrows, const uint32_t *d_coeff0,
                           const uint32_t *d_coeff1, uint64_t *d_rop0, uint64_t *d_rop1, int accumulate);
int mfh_crs_set_resident(mfh_ctx *ctx, const void *d_rows);
/* Partial residency for a CRS whose expansion exceeds HBM (362 GB for the 2^20-constraint CRS): only stream rows
 * [0, nrows_resident) are in the image; mfh_prove* streams those and regenerates the remaining rows from the seed. */
int mfh_crs_set_resident_prefix(mfh_ctx *ctx, const void *d_rows, size_t nrows_resident);
/* Multi-GPU form ("GPU g ... keeps its slice of the expanded CRS resident", 45 GB per GPU for the 2^20-constraint
 * CRS on 8 GPUs): the image holds only rank `rank`'s contiguous shares, in the order S share | AS share | BT+BV share
 * (mfh_resident_share_rows() rows of mfh_resident_row_bytes() each).  mfh_prove_partial* with the same (rank, world) then streams it. */
size_t mfh_resident_share_rows(const mfh_ctx *ctx, uint32_t rank, uint32_t world);
int mfh_crs_expand_share(mfh_ctx *ctx, const uint8_t *d_crs_c8, uint32_t rank, uint32_t world, void *d_image);
int mfh_crs_set_resident_share(mfh_ctx *ctx, const void *d_image, uint32_t rank, uint32_t world);

/* Batched regev_encrypt2 + ct_export (src/lwe.c:78-97,115-119): for i < nrows
 *   b_i = (e_i*p + <sk, a_i> + m_i) mod 2^(64K),  a_i = row at stream offset off + i*n*CT_BYTES
 * d_sk: n values; d_msg: nrows uint32 (< p); d_err: nrows values (the sampled error e, any L-limb value;
 * the reference draws 559 bits from getrandom, src/lwe.c:60-63); d_c8_out: nrows*CT_BYTES bytes. */
int mfh_encrypt_rows(mfh_ctx *ctx, uint64_t off, size_t nrows, const uint64_t *d_sk, const uint32_t *d_msg,
                     const uint64_t *d_err, uint8_t *d_c8_out);
/* Which kernel mfh_encrypt_rows (hence mfh_setup) uses; the results are identical.  0 (default): batches of 4096 rows or more run <sk, a> on
 * the matrix cores -- the dot product as a (rows x keystream bytes) x Toeplitz(sk) int8 GEMM, each lane's AES output block being an MFMA
 * operand as it stands -- when off and n * CT_BYTES are multiples of 8, anything else the VALU kernel; 1: always the VALU kernel;
 * 2: always the matrix-core kernel (MFH_EINVAL from mfh_encrypt_rows if the alignment does not allow it). */
int mfh_set_encrypt_path(mfh_ctx *ctx, int path);

/* Batched regev_decrypt (src/lwe.c:105-111) of `count` explicit ciphertexts: d_out[i] = (b - <a,sk> mod 2^(64K)) mod p */
int mfh_decrypt(mfh_ctx *ctx, const uint64_t *d_sk, const uint64_t *d_cts, size_t count, uint32_t *d_out);
/* mfh_decrypt: 0 (default) = by batch size (from 4096 ciphertexts <a, sk> runs as a Toeplitz int8 GEMM on the matrix cores, HBM-bound), 1 = VALU kernel,
 * 2 = matrix-core kernel.  Same results. */
int mfh_set_decrypt_path(mfh_ctx *ctx, int path);
/* regev_decrypt (src/lwe.c:105-111) of nrows SEED-COMPRESSED ciphertexts -- the form ct_export / the CRS hold (src/lwe.c:115-126): row i's a part is
 * regenerated from the public stream at off + i * n * CT_BYTES (ct_import), d_c8 holds its CT_BYTES little-endian b.  d_out[i] = (b - <a, sk>) mod p.
 * off and n * CT_BYTES must be multiples of 8 (MFH_EUNSUPPORTED otherwise).  AES-bound like mfh_encrypt_rows. */
int mfh_decrypt_rows(mfh_ctx *ctx, uint64_t off, size_t nrows, const uint64_t *d_sk, const uint8_t *d_c8, uint32_t *d_out);

/* mpz_add_dotp (src/lwe.c:20-28): rop = (rop + sum_{j<len} a[j]*b[j]) mod 2^(64K); rop is one value, a and b are len values */
int mfh_add_dotp(mfh_ctx *ctx, uint64_t *d_rop, const uint64_t *d_a, const uint64_t *d_b, size_t len);

/* ct_smudge (src/lwe.c:65-76) with caller-supplied entropy: b += (+/-) u*p on coordinate n of each of `count`
 * ciphertexts; h_mag = count * maglen little-endian bytes of u, h_sign[i]&1 selects the minus sign. */
int mfh_ct_smudge(mfh_ctx *ctx, uint64_t *d_cts, size_t count, const uint8_t *h_mag, size_t maglen, const uint8_t *h_sign);

/* ---- L3: SSP witness polynomial ------------------------------------------------------------------- */
/* Device SSP layout: uint32 d_ssp[(m+3)][d], slot 0 = t, slot i+1 = v_i, coefficients reduced mod p
 * (reference host layout: uint64 little-endian, src/ssp.h:6-9; mfh_ssp_upload converts and reduces as
 * nmod_poly_import does, src/ssp.c:28-34). */
int mfh_ssp_upload(mfh_ctx *ctx, const void *h_ssp_u64, uint32_t *d_ssp, size_t first_slot, size_t nslots);
/* w(x) = delta*t(x) + sum_{i=1..m-1, witness bit i-1 set} v_i(x) mod p   (src/snark.c:141,147-155);
 * h_witness_bits: little-endian bit string, bit i-1 <-> v_i (mpz_tstbit).  d_w: d uint32. */
int mfh_witness_poly(mfh_ctx *ctx, const uint32_t *d_ssp, const uint8_t *h_witness_bits, uint32_t delta, uint32_t *d_w);

/* Generator-defined SSP (BASELINE configs 4/5; SURVEY 8(d): "SSP coefficients defined by a counter-based PRG (not stored)").
 * The dense buffer of src/ssp.h:6-9 is 5.9 TB at 2^20 constraints; here v_i[k] = f(seed, slot i+1, k) (a 32-bit integer hash
 * reduced into [0,p), csrc/ssp_prg.hpp) and only slot 0 (t, d uint32) is stored.  mfh_ssp_prg_make_t builds
 * t = v_0 + sum_{witness bit} v_i - 1 as random_ssp does (src/ssp.c:59-71); mfh_ssp_set_prg(ctx, seed, d_t) registers the SSP,
 * after which EVERY entry point that takes `d_ssp` accepts NULL to mean "the registered generator-defined SSP"
 * (mfh_witness_poly, mfh_witness_lanes, mfh_ssp_prepare, mfh_setup_messages, mfh_setup, mfh_prove*, mfh_verify).
 * mfh_ssp_prg_fill materialises slots [first_slot, first_slot+nslots) (slots >= 1) as a dense uint32 image (tests). */
int mfh_ssp_set_prg(mfh_ctx *ctx, uint64_t seed, const uint32_t *d_t);
int mfh_ssp_prg_make_t(mfh_ctx *ctx, uint64_t seed, const uint8_t *h_witness_bits, uint32_t *d_t);
int mfh_ssp_prg_fill(mfh_ctx *ctx, uint64_t seed, size_t first_slot, size_t nslots, uint32_t *d_out);

/* A constraint system given row by row, written as the device SSP (the layout above) by interpolation on the device.
 * Points: r_j = j + 2, j = 0 .. d - 2 (d - 1 of them).  Row j < nrows asks  v_0(r_j) + sum_i a_i v_i(r_j)  in {-1, +1}, where its entries
 * (h_wire[e], h_coef[e]), e in [h_row_ptr[j], h_row_ptr[j + 1]), give the values v_i(r_j) = coef (wire 0 = the constant v_0; entries of one row with the same
 * wire add; a wire absent from a row is 0 there).  Padding rows j >= nrows have v_0(r_j) = 1 and no wire: every input satisfies them.
 * Written: slot 0 = t(x) = prod_j (x - r_j) (monic, degree d - 1; no root at +-1, so a satisfying batch takes the exact-division path of mfh_poly_h_multi),
 * slot i + 1 = v_i, the interpolant of degree < d - 1 of its column (i = 0 .. m - 1), slots m + 1 and m + 2 = 0.
 * Bits: input (witness) bit i - 1 is wire i (mfh_witness_poly); with public inputs, bits [0, lu) -- wires 1 .. lu -- are the statement.
 * h_row_ptr: nrows + 1 entries (only [h_row_ptr[0], h_row_ptr[nrows]) of h_wire / h_coef is read); wires in [0, m), coefficients in [0, p).
 * MFH_EINVAL, with nothing written, for nrows > d - 1, a wire >= m, a coefficient >= p or a decreasing h_row_ptr; then MFH_EUNSUPPORTED for d > 2^22.
 * d_ssp is written in full, derived images of an earlier SSP are dropped as by mfh_ssp_upload; call mfh_ssp_prepare afterwards.  Per context the call keeps
 * a seed table of (d - 1) * ceil(d / 32) words (134 MB at d = 2^15), built on its first call, and the tree of t of mfh_ssp_set_rows (below; 7.3 MB at
 * d = 2^15), built when the context has none; the call synchronises the context's stream. */
int mfh_ssp_from_rows(mfh_ctx *ctx, uint32_t nrows, const uint32_t *h_row_ptr, const uint32_t *h_wire, const uint32_t *h_coef, uint32_t *d_ssp);

/* The same constraint system registered as its ROWS (the row SSP): no dense image exists, so circuits fill any d mfh_ssp_from_rows accepts up to 2^22,
 * including d = 2^20 where the dense SSP would be 2.9 TB.  Input, points, padding rows and every MFH_EINVAL case as mfh_ssp_from_rows (an MFH_EINVAL leaves
 * the previous registration in place); lu_max < m is the largest number of public wires the prover will be asked for.  Afterwards d_ssp == NULL means the row
 * SSP in mfh_ssp_prepare, mfh_setup_messages, mfh_setup, mfh_setup_image, mfh_setup_public, mfh_vk_derive, mfh_verify, mfh_witness_poly, mfh_witness_poly_multi,
 * mfh_witness_poly_mm, mfh_prove, mfh_prove_public, mfh_prove_batch, mfh_prove_batch_public and mfh_batch_chain, and every one of them returns exactly what it
 * returns for the dense SSP mfh_ssp_from_rows writes from the same rows.  A public call with lu > lu_max returns MFH_EINVAL.  mfh_witness_lanes,
 * mfh_witness_from_lanes, mfh_witness_poly_mm_cols, mfh_batch_witness_cols and mfh_prove_partial* with world > 1 return MFH_EUNSUPPORTED in row mode.
 * The prover interpolates w - delta t from the statement's row sums by the subproduct tree of t (csrc/ssp_rows.hip); setup evaluates v_i(s) from the rows.
 * Registering replaces a generator-defined SSP (and mfh_ssp_set_prg replaces the row SSP); mfh_ssp_set_rows(ctx, 0, NULL, NULL, NULL, 0) unregisters and frees.
 * Derived images of an earlier SSP are dropped as by mfh_ssp_from_rows; call mfh_ssp_prepare(ctx, NULL) afterwards.  The call synchronises the stream.
 * Device memory: per context (d alone, kept across registrations) the tree of t, (6 log2(Np / 64) + 1) Np + 2 d words with Np = 2^ceil(log2 d) -- 7.3 MB at
 * d = 2^15, 0.37 GB at 2^20 -- plus the NTT tables of the polynomial step for length Np; per registration the rows (nrows + 1 + 2 nnz words), the dense
 * prefix t, v_0 .. v_lu_max ((lu_max + 2) d words) and the interpolation scratch: 8 Np words per statement in flight, chunks of at most 128 MB.
 * mfh_ssp_rows_fill writes slots [first_slot, first_slot + nslots) of the dense layout by interpolation (tests; slot 0 = t, slots m + 1, m + 2 = 0). */
int mfh_ssp_set_rows(mfh_ctx *ctx, uint32_t nrows, const uint32_t *h_row_ptr, const uint32_t *h_wire, const uint32_t *h_coef, uint32_t lu_max);
int mfh_ssp_rows_fill(mfh_ctx *ctx, size_t first_slot, size_t nslots, uint32_t *d_out);

/* The row check: which rows of the registered row SSP does a witness violate?  What a prover otherwise learns only from a rejected proof, with no location.
 * Statement b is h_bits + b * bits_stride in the layout of mfh_prove_batch: bit i - 1 is wire i (with public inputs the statement is bits [0, lu)).
 * Row j < nrows has  E_j = (the coefficients of its wire-0 entries) + sum of coef(e) over its entries e whose wire i >= 1 has its bit set,  mod p; entries of
 * one row on one wire add.  The row is satisfied iff E_j is 1 or p - 1.  h_count[b] = the number of violated rows of statement b; h_first[b] (h_first may
 * be NULL) = the smallest violated row index, 0xFFFFFFFF when there is none.  Padding rows j >= nrows hold for every input and are not examined; an empty
 * row has E_j = 0 and counts as violated.  A witness with h_count[b] = 0 is one the prover's h = (v^2 - 1) / t is exact for.
 * One thread per (row, statement) (k_rows_violations, csrc/ssp_rows.hip) reads the packed bits as the prover's bottom level does; the bits are staged like
 * the prover's, compacted to (m + 6) / 8 bytes per statement in pinned memory that mfh_scrub_staging zeroes, in chunks of statements of at most 64 MiB
 * (at least one statement), their device copy in the witness scratch.  The call synchronises the stream.
 * MFH_EINVAL, each with its own text and nothing written: no row SSP registered; bits_stride < (m + 6) / 8; nstmt > 0 with h_bits or h_count NULL.
 * nstmt = 0 does nothing. */
int mfh_ssp_rows_violations(mfh_ctx *ctx, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, uint32_t *h_count, uint32_t *h_first);

/* Witnesses of a Boolean circuit for a batch of statements, evaluated on the device.  What random_ssp(mpz_t input, ...) (src/ssp.c:37) is to a random SSP --
 * the reference's only source of a witness -- this is to the SSP of mfh_ssp_from_rows: the input bits of mfh_prove / mfh_prove_batch for each statement.
 * Wires (mfh_ssp_from_rows): wire 0 is the constant, wires 1 .. nin are the inputs (public first, then private), and gate g writes wire nin + 1 + g.
 * A program is validated, ordered by level (inputs are level 0, a gate one more than the highest level of the operands it uses; CONST: 1; SUM3 shares its
 * MAJ's level; a WSUM head and its WSUM_BIT records: 1 + the highest level of its terms) and uploaded once by one of five entry points; it belongs to
 * ctx's device; destroy it (mfh_circuit_destroy, every kind) before the context.
 *
 * Arguments.
 *   h_gates    ngates records of uint32: (op, a, b) for mfh_circuit_create / _global, (op, a, b, c) for _ex / _out / _sum (extended programs)
 *   h_asserts  nasserts records (wire, value): wire in [1, nin + ngates], value 0 or 1
 *   h_equal    nequal pairs (a, b) asserting wire a = wire b                                                       (_ex, _out, _sum)
 *   h_outputs  nout pairs (p, w): the input wire p (a public input of the statement, wires 1 .. lu) is DEFINED as wire w   (_out, _sum)
 *   h_terms    nterms_total pairs (wire, shift), the terms of the WSUM gates                                         (_sum)
 *   flags      0: wire state in LDS; MFH_CIRCUIT_GLOBAL: in device memory                                           (_ex, _out, _sum)
 * The wire state.  LDS (mfh_circuit_create, flags 0): one uint32 word per wire, (MFH_CIRCUIT_MAX_WIRES + 1) * 4 bytes = 128 KiB of the 160 KiB of a CU,
 * so nin + ngates <= MFH_CIRCUIT_MAX_WIRES (every circuit of mf.DEFAULT, m - 1 = 21 844 wires, fits).  Device memory (mfh_circuit_create_global,
 * MFH_CIRCUIT_GLOBAL): nin + ngates <= m - 1 alone (699 049 wires at d = 2^20, m = 699 050; gate records are 16 bytes with 32-bit wire numbers, 7.5 MB for
 * 470 000 gates); one column of (nin + ngates + 1) words, rounded up to 32, per block of 32 statements in a context buffer reused across calls.  Witness
 * rows and holds are byte for byte the same in both kinds.
 *
 * Gates and their operands (g = the gate's index; extended programs only below the line; c = 0 where it is not named).
 *   XOR, AND, OR          a, b in [1, nin + g]
 *   NOT                   a in [1, nin + g], b = a
 *   ------------------------------------------------------------------------------------------------------------------------------------------------
 *   LUT2(tt)              a, b in [1, nin + g]: out = (tt >> (a + 2b)) & 1
 *   MAJ, SUM3             a, b, c in [1, nin + g]; SUM3 is sound only next to the MAJ that forces its carry k: gate g - 1 must be a MAJ with the same (a, b, c)
 *   CONST0, CONST1        a = b = c = 0
 *   WSUM (_sum only)      (a, b, c) = (first_term, nterms, nbits): its terms are h_terms[first_term .. first_term + nterms), and it has nbits =
 *                         bitlength(sum_e 2^shift_e) output wires; output wire i carries bit i of T = sum_e 2^shift_e * x_e, x_e the bit on term e's wire (a
 *                         wire may occur in several terms).  The rule "gate g writes wire nin + 1 + g" stays: the head at gate g is followed by exactly
 *                         nbits - 1 records (MFH_GATE_WSUM_BIT, i, 0, 0), i = 1 .. nbits - 1, and writes wires nin + 1 + g .. nin + g + nbits.
 * Every extended gate and every equality adds one SSP row that is +-1 mod p exactly when its output is right, given bit operands (circuit.py compiles them;
 * wire w keeps its bit row 2w - 1):
 *   MAJ(a, b, c)     k = 1 iff a + b + c >= 2                          2a + 2b + 2c - 4k - 1
 *   SUM3(a, b, c)    s = a ^ b ^ c (k = the wire of gate g - 1)         1 - a - b - c + 2k - s
 *   CONST0 / CONST1  0 / 1                                              1 - c / c
 *   LUT2(tt)(a, b)   c = (tt >> (a + 2b)) & 1                          by the class of tt (circuit.py); XOR, AND, OR, NOT rows for those functions
 *   equality (a, b)  a = b (no wire)                                     1 - a - b
 *   output (p, w)    p = w                                               1 - p - w, an equality: list it in h_equal and it holds by construction
 *   WSUM             two rows 2X - 1 and 2X + 1 with X = T - sum_i 2^i o_i: the first is +-1 mod p iff X in {0, 1}, the second iff X in {0, -1}, so X = 0
 *                    mod p, and with nbits <= 24 and every operand and output wire a bit, |X| < 2^24 < p gives O = T over the integers
 *
 * MFH_EINVAL, with its own mfh_last_error text (named after the function called) and nothing allocated:
 *   every entry point     nin + ngates > m - 1; in the LDS kind nin + ngates > MFH_CIRCUIT_MAX_WIRES; an unknown op (not extended: above NOT; _ex, _out:
 *                         8 .. 15 and >= 32; _sum: 10 .. 15 and >= 32); an operand of 0 or not below the gate's output wire; an assertion on wire 0 or above
 *                         nin + ngates; an assertion value other than 0 / 1; a count > 0 with its array null
 *   _ex, _out, _sum       unknown flag bits; nin + ngates >= 2^24; a violation of the operand table above (a third operand c != 0 on a one- or two-input
 *                         gate, NOT with b != a, CONST with an operand, SUM3 not directly after its MAJ or with other operands); an equality on wire 0 or
 *                         above nin + ngates, or with a = b
 *   _out, _sum            p = 0 or p > nin; w = 0 or w > nin + ngates; w = p; a p given twice; a w that is the p of another pair; a gate operand or an
 *                         assertion on an output wire (it has no value until the end); an equality touching an output wire other than (p, w) / (w, p) of
 *                         its own pair
 *   _sum                  a term range outside the array; nterms = 0; a term wire that is 0, not below the head's output wire, or an output wire; a
 *                         shift >= nbits; terms not in non-decreasing shift order; nbits other than the bit length of sum 2^shift; nbits > 24; a head not
 *                         followed by its WSUM_BIT records in order; a WSUM_BIT record without a head
 *
 * What mfh_circuit_assign runs: circuit_eval.hip's k_circuit_eval<EX, OUT, SUM> (LDS) or k_circuit_eval_global<EX, OUT, SUM> (device memory), by what the
 * program holds, whichever entry point made it (so nout = 0 gives exactly the program of mfh_circuit_create_ex, and a _sum program without a WSUM gate
 * exactly that of mfh_circuit_create_out).  Kernel timing kinds (mfh_timing_kind):
 *   not extended (mfh_circuit_create / _global)          <false>             "circuit_assign"      / "circuit_assign_global"
 *   extended, no outputs, no WSUM gate                   <true>              "circuit_assign_ex"   / "circuit_assign_global_ex"
 *   extended with outputs (nout > 0), no WSUM gate       <true, true>        "circuit_assign_out"  / "circuit_assign_global_out"
 *   with a WSUM gate, outputs or none                    <true, OUT, true>   "circuit_assign_sum"  / "circuit_assign_global_sum"
 * Device gate records are 8 bytes {a | b << 16, out | op << 16} for LDS programs that are not extended, 16 bytes {a, b, out, op} for device-memory ones,
 * 16 bytes {a, b, c, out | op << 24} for extended programs of either kind.  A WSUM head is evaluated by one wave, lane j summing statement j's terms as an
 * integer, the output words formed by ballots. */
#define MFH_GATE_XOR 0u /* c = a ^ b */
#define MFH_GATE_AND 1u /* c = a & b */
#define MFH_GATE_OR 2u  /* c = a | b */
#define MFH_GATE_NOT 3u /* c = 1 - a */
#define MFH_GATE_MAJ 4u    /* out = maj(a, b, c) */
#define MFH_GATE_SUM3 5u   /* out = a ^ b ^ c; gate g - 1 must be MFH_GATE_MAJ with the same (a, b, c) */
#define MFH_GATE_CONST0 6u /* a = b = c = 0 */
#define MFH_GATE_CONST1 7u
#define MFH_GATE_WSUM 8u     /* head: (a, b, c) = (first_term, nterms, nbits) */
#define MFH_GATE_WSUM_BIT 9u /* (a, b, c) = (i, 0, 0): output bit i of the head i records before */
#define MFH_GATE_LUT2(tt) (16u + (tt)) /* out = (tt >> (a + 2b)) & 1, tt in [0, 16) */
#define MFH_CIRCUIT_MAX_WIRES 32767u
#define MFH_CIRCUIT_GLOBAL 1u
typedef struct mfh_circuit mfh_circuit;
int mfh_circuit_create(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                       mfh_circuit **out);
int mfh_circuit_create_global(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                              mfh_circuit **out);
int mfh_circuit_create_ex(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                          uint32_t nequal, const uint32_t *h_equal, uint32_t flags, mfh_circuit **out);
int mfh_circuit_create_out(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                           uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, uint32_t flags, mfh_circuit **out);
int mfh_circuit_create_sum(mfh_ctx *ctx, uint32_t nin, uint32_t ngates, const uint32_t *h_gates, uint32_t nasserts, const uint32_t *h_asserts,
                           uint32_t nequal, const uint32_t *h_equal, uint32_t nout, const uint32_t *h_outputs, uint32_t nterms_total,
                           const uint32_t *h_terms, uint32_t flags, mfh_circuit **out);
void mfh_circuit_destroy(mfh_circuit *c);
/* nstmt statements: row b of h_inputs (in_stride bytes) holds the nin input bits, LSB first (bits >= nin are ignored, and so is input bit p - 1 of an
 * output wire p).  Row b of h_witness_bits (bits_stride bytes) becomes the witness bit string of statement b: bit i - 1 = wire i, bits >= nin + ngates
 * zero -- the layout mfh_prove_batch reads; after the last level and before the assertions and equalities are folded, wire w's value is written onto
 * wire p for every output pair, so bits [0, lu) of a witness row carry the computed statement.  h_holds[b] = 1 if every value assertion and every
 * equality holds on statement b, else 0.  Bitsliced: one workgroup serves 32 statements, one word per wire; one launch per chunk of statements whatever the
 * circuit's depth.  A chunk is 8 192 statements in the LDS kind; in the device-memory kind the most whole blocks whose staging, chunk x (in_stride +
 * bits_stride + 1) bytes, fits 64 MiB and whose columns fit 256 MiB, at least one block (736 statements at d = 2^20 with 2 508-byte input rows).
 * MFH_EINVAL for in_stride * 8 < nin or bits_stride * 8 < nin + ngates; nstmt = 0 does nothing.  Staged through the context's pinned buffers
 * (mfh_scrub_staging zeroes them); the call synchronises the context's stream. */
int mfh_circuit_assign(mfh_ctx *ctx, const mfh_circuit *c, uint32_t nstmt, const uint8_t *h_inputs, size_t in_stride, uint8_t *h_witness_bits,
                       size_t bits_stride, uint8_t *h_holds);

/* ---- Merkle trees (merkle.hip): what words.MerklePath(depth) proves membership in, kept in device memory ------------------------------
 * The node function is parent = compress(IV, left || right): ONE SHA-256 compression of the 64 bytes from the constant initial hash value, no padding
 * block.  The tree is one device allocation of 2^(depth + 1) nodes of 32 bytes in heap order: node 1 is the root, the children of node k are 2k and
 * 2k + 1, slot 0 is unused; node j of level l (0 = the leaves, depth = the root) is heap index 2^(depth - l) + j.  A node is stored as its 32 digest
 * bytes (the big-endian words of FIPS 180-4, what hashlib prints).  The tree belongs to ctx's device and may be used by every context of that device;
 * its memory is its own (hipMalloc at create).  Destroy it before the context that created it.
 *   create      1 <= depth <= 24 (1 GiB of nodes at 24).  The tree of all-zero leaves with every level computed; waits for the stream.
 *   set_leaves  d_leaves = count x 32 bytes ON THE DEVICE, copied to leaves [first, first + count); then parents [first >> l, (first + count - 1) >> l] of
 *               level l = 1 .. depth are recomputed, one launch of k_merkle_level per level, and nothing else.  Queue-only on the context's stream (no
 *               host wait): d_leaves must stay valid until the stream has passed the call.  count = 0 does nothing.
 *   root        the root's 32 bytes to the host; synchronises the stream.
 *   nodes       the device pointer of level `level`'s first node (2^(depth - level) nodes of 32 bytes follow), 0 <= level <= depth; touches no stream:
 *               the caller orders its reads behind the context's stream.  Its error text goes to the creating context.
 *   paths       row b of h_inputs (in_stride bytes) becomes the packed input row of MerklePath(depth) for the leaf of index h_index[b] -- what
 *               mfh_circuit_assign takes: 32 zero bytes where the root is computed; the leaf's 8 words; for l = 0 .. depth - 1 the 8 words of the sibling,
 *               heap node ((2^depth + index) >> l) ^ 1; each word a little-endian uint32 holding the word's value (the node's 4 bytes reversed); then
 *               ceil(depth / 8) bytes holding the index, little-endian (direction bit l = bit l of the index).  nin = 256 + 256 (depth + 1) + depth bits;
 *               exactly ceil(nin / 8) bytes of a row are written, the rest of a wider row is left alone.  Indices may repeat.  One launch of
 *               k_merkle_paths per chunk of statements, a chunk being the most statements whose rows fit 64 MiB (at least one); staged through the
 *               context's pinned buffers (mfh_scrub_staging zeroes them); synchronises the stream.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing allocated, queued or written: depth 0 or above 24; a null tree or a null
 * required pointer; a tree of another device; first + count > 2^depth; an index >= 2^depth; in_stride < ceil(nin / 8); level > depth.
 * Kernel timing kinds: "merkle_level" (total_rows = parents computed, one count per launch: depth launches and 2^depth - 1 rows for a full build) and
 * "merkle_paths" (total_rows = statements). */
typedef struct mfh_merkle mfh_merkle;
int mfh_merkle_create(mfh_ctx *ctx, uint32_t depth, mfh_merkle **out);
void mfh_merkle_destroy(mfh_merkle *t);
int mfh_merkle_set_leaves(mfh_ctx *ctx, mfh_merkle *t, uint32_t first, uint32_t count, const uint8_t *d_leaves);
int mfh_merkle_root(mfh_ctx *ctx, const mfh_merkle *t, uint8_t h_root[32]);
int mfh_merkle_nodes(const mfh_merkle *t, uint32_t level, const uint8_t **d_nodes);
int mfh_merkle_paths(mfh_ctx *ctx, const mfh_merkle *t, uint32_t nstmt, const uint32_t *h_index, uint8_t *h_inputs, size_t in_stride);

/* ---- SHA-256 of whole records (merkle.hip: k_sha256_records): the leaves of a tree from the data they stand for --------------------------------
 * A record is `length` bytes ON THE DEVICE at d_records + r * stride, stride >= length, any byte alignment of d_records and of stride; length <= 2^20.
 * Its digest is SHA-256 of exactly those bytes with the padding of FIPS 180-4 5.1.1 (0x80, zeros, the 64-bit big-endian bit length), which is made
 * from `length` alone and never read: what hashlib.sha256(record).digest() gives and what words.Sha256Message(length) states.  Nothing outside
 * [d_records, d_records + (count - 1) * stride + length) is read; a byte of a gap between two records may be read and enters no digest.
 *   sha256_records   d_digests[32 r, 32 r + 32) <- the digest of record r, r < count; d_digests is 16-byte aligned device memory of 32 count bytes.
 *   set_records      leaves [first, first + count) of the tree <- the digests of the records, hashed straight into the tree's leaves (no buffer in
 *                    between); then their ancestors are recomputed as by mfh_merkle_set_leaves (one launch of k_merkle_level per level).
 * Both are queue-only on the context's stream (no host wait): d_records must stay valid until the stream has passed the call.  count = 0 does nothing.
 * One launch of k_sha256_records, one thread per record.  The range arithmetic is done in 64 bits.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued or written: a null tree; a null d_digests, or a null d_records
 * with length > 0 (count > 0); stride < length; length > 2^20; first + count > 2^depth; a tree of another device; d_digests not 16-byte aligned.
 * Kernel timing kind: "sha256_records" (total_rows = records, one count per launch). */
int mfh_sha256_records(mfh_ctx *ctx, const uint8_t *d_records, size_t stride, uint32_t length, uint32_t count, uint8_t *d_digests);
int mfh_merkle_set_records(mfh_ctx *ctx, mfh_merkle *t, uint32_t first, uint32_t count, const uint8_t *d_records, size_t stride, uint32_t length);

/* ---- Sequential updates of a tree as statements (merkle.hip: k_merkle_update_level, k_merkle_update_store): what words.MerkleUpdate(depth) proves --
 * "I changed one leaf, and that change alone takes the tree from root R to root R'".  For k = 0 .. nupd - 1 IN ORDER: row k of h_inputs (in_stride bytes)
 * becomes the packed input row of MerkleUpdate(depth) taken from the tree as it stands before update k; then leaf h_index[k] becomes
 * d_new_leaves[32 k, 32 k + 32) (ON THE DEVICE, 16-byte aligned) and its ancestors are recomputed.  Indices may repeat, and later updates may be the
 * siblings, cousins or the same leaf as earlier ones: update k sees everything updates 0 .. k - 1 did.  Afterwards the tree is what nupd one-leaf
 * mfh_merkle_set_leaves calls would have left.
 *   roots    h_roots is NULL or (nupd + 1) x 32 bytes: the roots R_0 .. R_nupd; statement k is (R_k, R_k+1), MerkleUpdate.statement's bytes.
 *   rows     64 zero bytes where the two roots are computed; the 8 words of the old leaf; the 8 words of the new leaf; for l = 0 .. depth - 1 the 8 words
 *            of the sibling at level l; each word a little-endian uint32 holding the word's value (mfh_merkle_paths' convention); then ceil(depth / 8)
 *            bytes holding the index.  nin = 512 + 512 + 256 depth + depth bits; exactly 128 + 32 depth + ceil(depth / 8) bytes of a row are written,
 *            the rest of a wider row is left alone.
 *   how      level-synchronous, not a loop over updates: the host makes, in O(nupd log nupd + nupd depth), the tables "the last earlier update at my
 *            leaf / at my sibling of level l" and "I am the last update at this node" (merkle_sched.hpp); then one launch of k_merkle_update_level per
 *            level, one thread per update, computes every update's value of its node from its own value and its sibling's below -- an earlier update's
 *            value or the tree's stored node -- and writes the sibling into the row; one launch of k_merkle_update_store then writes each touched node's
 *            last value into the tree, after every read of the stored nodes.  depth + 1 launches per chunk of updates, a chunk being the most updates
 *            whose rows fit 64 MiB (at least one); chunks run in order.  Rows, roots and tables are staged through the context's pinned buffers
 *            (mfh_scrub_staging zeroes them); d_new_leaves is read in place and in stream order (it must not overlap the tree's own nodes); the call
 *            synchronises the stream.  nupd = 0 does nothing.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued, written or changed in the tree: a null tree; a tree of another
 * device; nupd > 0 with h_index, d_new_leaves or h_inputs null; an index >= 2^depth; in_stride below the row's bytes; d_new_leaves not 16-byte aligned.
 * Kernel timing kind: "merkle_updates" (one count per launch: depth + 1 per chunk; total_rows = compressions, nupd x depth over the call). */
int mfh_merkle_update_rows(mfh_ctx *ctx, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, const uint8_t *d_new_leaves, uint8_t *h_inputs, size_t in_stride,
                           uint8_t *h_roots);

/* ---- Sequential updates of a table of records and its tree as statements (merkle.hip: k_sha256_records, k_record_gather, the level and store kernels of
 * mfh_merkle_update_rows, k_record_store): what words.MerkleRecordUpdate(length, depth) proves -- "I changed one record, and that change alone takes the tree
 * from root R to root R'".  d_table holds the 2^depth records of the tree ON THE DEVICE, record i at d_table + i * table_stride (table_stride >= length; any
 * byte alignment of base and stride, as mfh_sha256_records takes them).  PRECONDITION, NOT CHECKED: leaf i of the tree is SHA-256 of record i -- the state
 * after mfh_merkle_set_records(ctx, t, 0, 2^depth, d_table, table_stride, length).  Where table and tree disagree, the old root mfh_circuit_assign computes
 * from a row is not R_k.
 * For k = 0 .. nupd - 1 IN ORDER: row k of h_inputs becomes the packed input row of MerkleRecordUpdate(length, depth) taken from the table and the tree as
 * they stand before update k; then record h_index[k] becomes the `length` bytes at d_new_records + k * new_stride (on the device, any alignment) and its leaf
 * and the leaf's ancestors are recomputed.  Indices may repeat: the old record of update k is then the new record of the last earlier update at that index.
 *   rows     64 zero bytes where the two roots are computed; the old record's `length` bytes; the new record's; for l = 0 .. depth - 1 the 8 words of the
 *            sibling at level l, each a little-endian uint32 holding the word's value (mfh_merkle_update_rows' order); ceil(depth / 8) bytes holding the
 *            index.  Exactly 64 + 2 length + 32 depth + ceil(depth / 8) bytes of a row are written, the rest of a wider row is left alone.
 *   after    the table holds each touched record's last new value and nothing outside a touched record's `length` bytes was written (the gap bytes of a
 *            wider stride stay); the tree holds the final nodes; h_roots, when not NULL, the (nupd + 1) x 32 bytes R_0 .. R_nupd.
 *   how      per chunk, on the context's stream: one launch of k_sha256_records hashes the chunk's new records; k_record_gather copies every update's old
 *            record -- out of the table, or out of d_new_records where the schedule of merkle_sched.hpp names an earlier update at that leaf -- and new
 *            record into the row heads; the depth + 1 launches of mfh_merkle_update_rows run on the digests; k_record_store writes the new record of the
 *            last update at each leaf into the table, behind the gather's reads.  A chunk is the most updates whose rows fit 64 MiB (at least one); chunks
 *            run in order, a later chunk reads the table and the tree the earlier ones stored.  Rows, roots and tables are staged through the context's
 *            pinned buffers (mfh_scrub_staging zeroes them), the host splices the heads and the siblings into the rows; the call synchronises the stream.
 *            d_new_records must not overlap the table, and neither may overlap the tree's nodes (not checked).  nupd = 0 does nothing.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued, written or changed in tree or table: a null tree; a tree of another
 * device; nupd > 0 with h_index, h_inputs or d_table null, or d_new_records null with length > 0; an index >= 2^depth; table_stride or new_stride below
 * length; length > 2^20; in_stride below the row's bytes.
 * Kernel timing kinds: "sha256_records" (1 per chunk, rows = the chunk's updates), "merkle_record_rows" (2 per chunk: the gather with rows = the chunk's
 * updates, the table store with 0), "merkle_updates" (depth + 1 per chunk, as mfh_merkle_update_rows). */
int mfh_merkle_update_records(mfh_ctx *ctx, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, uint8_t *d_table, size_t table_stride, uint32_t length,
                              const uint8_t *d_new_records, size_t new_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots);
/* Non-membership in an INDEXED table: for every query key the record whose range holds it, and the packed input row of words.MerkleAbsent(key_bytes, length,
 * depth) -- "this key is not in the set behind this root".
 *   layout     a key is key_bytes bytes, 1 <= key_bytes <= 32, compared as a big-endian unsigned integer (memcmp order); the all-zero and the all-0xFF key
 *              are sentinels, never members and never queries.  Record i of the table (at d_table + i * table_stride, any byte alignment of base and
 *              stride, as mfh_merkle_update_records takes it) is length >= 2 key_bytes bytes: lo = its own key at [0, key_bytes) | hi = the next larger
 *              key of the set at [key_bytes, 2 key_bytes) | an opaque payload.
 *   invariant  NOT CHECKED, and the statement is sound relative to it: the 2^depth records hold, in ANY positions, the sentinel record (0...0, k_1), one
 *              record (k_i, k_i+1) per member k_1 < k_2 < ..., the last of them with hi = FF...FF, and in every other slot lo >= hi (an all-zero slot
 *              qualifies), which makes the slot inert.  The open ranges (lo, hi) of the live records then partition the keys that are neither members
 *              nor sentinels.  Inserting k into the range of record p is two updates of mfh_merkle_update_records: record p with hi <- k, and the record
 *              (k, the old hi) into any inert slot.  Leaf i of the tree is SHA-256 of record i (the state after mfh_merkle_set_records), not checked
 *              either: the root mfh_circuit_assign computes from a row shows it.
 *   results    query j is the key_bytes bytes at h_keys + j * key_stride.  h_status[j] = 0, absent, with h_index[j] = the record with lo < q < hi; 1,
 *              present, with the record whose lo == q; 2, no record (only in a malformed table), with 0xFFFFFFFF.  Where several records of a malformed
 *              table qualify, the lowest index is reported.
 *   rows       h_inputs = NULL means locate only: no row work is launched.  Else row j (at h_inputs + j * in_stride): 32 zero bytes where the root is
 *              computed | q | the record's `length` bytes | the 32 depth sibling bytes in mfh_merkle_paths' word convention | ceil(depth / 8) index bytes.
 *              Exactly 32 + key_bytes + length + 32 depth + ceil(depth / 8) bytes of a row are written, the rest of a wider row is left alone.  A status 1
 *              row is written in full (its witness violates the statement's lo < q); a status 2 row gets the 32 zero bytes and q only.
 *   how        the host sorts the queries, drops duplicates and turns them into big-endian words; ONE launch of k_key_locate, one thread per record
 *              whatever nq, binary-searches them for the record's range (a range holding several queries is filled in by the whole wave) and leaves
 *              the lowest record per query by atomic minimum; the results come back through the sort's permutation.  Then per chunk (the most queries
 *              whose rows fit 64 MiB, at least one) k_merkle_paths runs on the located indices and k_absent_gather copies the located records; the host
 *              splices q, record and siblings.  Staging goes through the context's pinned buffers (mfh_scrub_staging zeroes them); the call synchronises
 *              the stream.  Neither the tree nor the table is modified.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued or written: a null tree; a tree of another device; key_bytes 0 or above
 * 32; length < 2 key_bytes or length > 2^20; table_stride < length; key_stride < key_bytes; nq > 0 with d_table, h_keys, h_index or h_status null; in_stride
 * below the row's bytes when h_inputs is given; a query that is all-zero or all-0xFF.  nq = 0 does nothing.
 * Kernel timing kinds: "merkle_locate" (1 per call, rows = 2^depth), "merkle_absent_rows" (1 per chunk: the gather, rows = the chunk's queries),
 * "merkle_paths" (1 per chunk, as mfh_merkle_paths). */
int mfh_merkle_absent_rows(mfh_ctx *ctx, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nq,
                           const uint8_t *h_keys, size_t key_stride, uint8_t *h_inputs, size_t in_stride, uint32_t *h_index, uint8_t *h_status);
/* nk sequential key inserts into an INDEXED table (the data model: mfh_merkle_absent_rows) and its tree in ONE call, and the packed input row of
 * words.MerkleInsert(key_bytes, length, depth) of every insert -- "key j was inserted, and that alone takes the tree from R_j to R_j+1".
 *   semantics  byte for byte what this gives, run once per key in order: mfh_merkle_absent_rows (locate) for the record p whose range holds the key; the two
 *              updates of an insert -- record p with hi <- key, and (key | the old hi | payload, zero-padded) into the LOWEST inert slot s of the table as it
 *              then stands -- through mfh_merkle_update_records.  That covers the table in place, every node of the tree, the roots and row j, which describes
 *              table and tree as they stood before insert j.  A later key may fall into a range an earlier key of the batch has split: it is resolved in order.
 *   arguments  key j is the key_bytes bytes at h_keys + j * key_stride; its payload the length - 2 key_bytes bytes at h_payloads + j * payload_stride, or all
 *              zero with h_payloads = NULL.  h_inputs = NULL: insert, no rows.  h_roots (may be NULL) receives the nk + 1 roots R_0 .. R_nk.  h_index
 *              receives nk pairs (p, s): the slot whose hi changed and the slot that received the new record.  h_status receives the status of each key
 *              against the table BEFORE the batch (mfh_merkle_absent_rows').
 *   rows       row j (at h_inputs + j * in_stride): 64 zero bytes where the roots are computed | the key | the old record of p | the old record of s | the new
 *              record of s | the 32 depth sibling bytes of p | those of s, from the tree after p's update | ceil(2 depth / 8) index bytes, bit l < depth =
 *              bit l of p, bit depth + l = bit l of s.  Exactly 64 + key_bytes + 3 length + 64 depth + ceil(2 depth / 8) bytes are written.
 *   how        k_key_locate as mfh_merkle_absent_rows runs it; three launches (k_inert_flags, k_inert_scan, k_inert_select) find the lowest nk inert slots
 *              and their total on the device, and nk + 1 words come back; the host plans predecessors and successors within the batch (merkle_insert.hpp);
 *              ONE launch of k_insert_records builds the 2 nk new records; they go through mfh_merkle_update_records' machinery in chunks of whole inserts
 *              (the most whose rows fit 64 MiB, at least one).  The call synchronises the stream behind the search, the inert search and every chunk.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued: a null tree; a tree of another device; key_bytes 0 or above 32; length
 * < 2 key_bytes or > 2^20; table_stride < length; key_stride < key_bytes; payload_stride < length - 2 key_bytes with h_payloads given; nk > 0 with d_table,
 * h_keys, h_index or h_status null; nk > 2^depth; in_stride below the row's bytes when h_inputs is given; a sentinel key; a key given twice.
 * MFH_EINVAL after the search, with h_status and the first element of every pair of h_index (the located record) filled, table and tree unwritten: a key that
 * is already a member (status 1); a key that no record holds (status 2); fewer inert slots than nk.  The call is all or nothing.  nk = 0 does nothing.
 * Kernel timing kinds: "merkle_locate" (1 per call), "merkle_inert" (3 per call, rows = 2^depth), "merkle_insert_records" (1 per call, rows = 2 nk), then per
 * chunk of 2 k updates "sha256_records" (1), "merkle_record_rows" (2; 1 without rows) and "merkle_updates" (depth + 1). */
int mfh_merkle_insert_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk,
                           const uint8_t *h_keys, size_t key_stride, const uint8_t *h_payloads, size_t payload_stride, uint8_t *h_inputs, size_t in_stride,
                           uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status);
/* ---- The three update calls above with the PATH CUT into level ranges, for trees deeper than one circuit: what words.MerkleSegment proves per range.
 * h_cuts holds ncuts >= 1 levels 1 <= c_0 < c_1 < .. < c_G-1 < depth (G = ncuts); segment 0 covers levels [0, c_0), segment g >= 1 levels [c_g-1, c_g) with
 * c_G = depth.  In place of (h_inputs, in_stride) the calls take h_rows and h_strides, arrays of ncuts + 1 row pointers and strides, one per segment:
 *   segment 0   the parent call's row over the subtree of height c_0 that holds the leaf: the same head, the first c_0 siblings, ceil(c_0 / 8) bytes holding
 *               the index mod 2^c_0 -- the packed input row of MerkleUpdate(c_0) (mfh_merkle_update_rows_cut: 128 + 32 c_0 + ceil(c_0 / 8) bytes), of
 *               MerkleRecordUpdate(length, c_0) (mfh_merkle_update_records_cut: 64 + 2 length + ..) or, ONE ROW PER INSERT, of MerkleInsert(key_bytes, length, c_0,
 *               joined=False) (mfh_merkle_insert_keys_cut: 128 zero bytes | key | old p | old s | new s | c_0 siblings of p | c_0 of s | ceil(2 c_0 / 8) index
 *               bytes of p mod 2^c_0 and s mod 2^c_0).  The values its circuit computes are the old and new node of level c_0 on the path.
 *   segment g   the packed input row of MerkleSegment(levels = c_g - c_g-1), ONE ROW PER UPDATE (an insert is two updates: 2 nk rows, p's then s's of each
 *               insert): the old node of level c_g-1 on the update's path as 8 words | the new node as 8 words | 64 zero bytes where the two tops are computed
 *               | the siblings of levels c_g-1 .. c_g - 1 in mfh_merkle_paths' word convention | ceil(levels / 8) bytes holding (index >> c_g-1) mod
 *               2^levels.  Exactly 128 + 32 levels + ceil(levels / 8) bytes of a row are written, the rest of a wider row is left alone.
 * The published node pairs of an update are the heads of its rows: (X_g, X_g') for g < G are bytes [0, 64) of its segment g + 1 row (words: swap each
 * word's bytes for the digest), (X_G, X_G') = (R_k, R_k+1) from h_roots.  mfh_merkle_insert_keys_cut writes ALL 2 nk + 1 roots to h_roots, so the root
 * between an insert's two updates, from which the upper chain of s starts, is there.  Tree, table, h_index, h_status and the order of events are the
 * parent call's; so are its kernels, with ONE more launch per chunk, k_merkle_cut_rows, behind the last k_merkle_update_level and before the write-back
 * (it reads stored nodes of the cut levels that the write-back may replace).  A chunk is the most updates (or whole inserts) whose rows, all segments
 * together, fit 64 MiB, at least one.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued, written or changed: everything the parent call refuses, and ncuts = 0
 * or h_cuts null; cuts that are not 1 <= c_0 < .. < c_G-1 < depth; h_rows or h_strides null; a null pointer in h_rows with rows to write; a stride below
 * its segment's row bytes.  mfh_merkle_insert_keys_cut has no "no rows" mode.
 * Kernel timing kinds: the parent call's, and "merkle_segments" (1 per chunk, rows = the chunk's updates x ncuts). */
int mfh_merkle_update_rows_cut(mfh_ctx *ctx, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, const uint8_t *d_new_leaves, uint32_t ncuts,
                               const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots);
int mfh_merkle_update_records_cut(mfh_ctx *ctx, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, uint8_t *d_table, size_t table_stride, uint32_t length,
                                  const uint8_t *d_new_records, size_t new_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                                  const size_t *h_strides, uint8_t *h_roots);
int mfh_merkle_insert_keys_cut(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk,
                               const uint8_t *h_keys, size_t key_stride, const uint8_t *h_payloads, size_t payload_stride, uint32_t ncuts, const uint32_t *h_cuts,
                               uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status);
/* ---- The two READ calls with the path cut into level ranges: what words.MerkleClimb proves per range.  h_cuts, h_rows and h_strides follow the conventions of
 * the mfh_merkle_*_cut calls above (ncuts >= 1 levels 1 <= c_0 < .. < c_G-1 < depth; ncuts + 1 row pointers and strides, nstmt or nq rows a segment).
 *   segment 0   the parent call's row over the subtree of height c_0 that holds the leaf: the same head, the first c_0 siblings, ceil(c_0 / 8) bytes holding
 *               the index mod 2^c_0 -- the packed input row of MerklePath(c_0) (mfh_merkle_paths_cut: 64 + 32 c_0 + ceil(c_0 / 8) bytes) or of
 *               MerkleAbsent(key_bytes, length, c_0) (mfh_merkle_absent_rows_cut: 32 + key_bytes + length + 32 c_0 + ceil(c_0 / 8) bytes).  The value its
 *               circuit computes is X_0, the node of level c_0 on the path.
 *   segment g   the packed input row of MerkleClimb(levels = c_g - c_g-1), c_G = depth: the stored node X_g-1 of level c_g-1 on the path as 8 words | 32 zero
 *               bytes where the top X_g is computed | the siblings of levels c_g-1 .. c_g - 1 in mfh_merkle_paths' word convention | ceil(levels / 8) bytes
 *               holding (index >> c_g-1) mod 2^levels.  Exactly 64 + 32 levels + ceil(levels / 8) bytes of a row are written, the rest of a wider row is left
 *               alone.
 * The published nodes of a statement are the heads of its rows: X_g for g < G is bytes [0, 32) of its segment g + 1 row (words: swap each word's bytes for the
 * digest), X_G the root (mfh_merkle_root).
 * mfh_merkle_absent_rows_cut: the search, the gather of the located records, h_index and h_status are exactly mfh_merkle_absent_rows'.  A status 1 row set is
 * written in full (segment 0 does not hold); a status 2 query gets the 32 zero bytes and its key alone in segment 0 and all-zero rows above it.  There is
 * no "locate only" mode: mfh_merkle_absent_rows has it.
 *   how        per chunk (the most statements whose rows of ALL segments fit 64 MiB, at least one) the indices go up and ONE launch of k_merkle_climb_rows
 *              writes every segment's staged rows straight from the tree's nodes -- no k_merkle_paths, no staged full path; mfh_merkle_absent_rows_cut adds
 *              k_absent_gather, and the host splices key and record into segment 0.  Staging goes through the context's pinned buffers; the calls run on
 *              the context's stream, synchronise it, and modify neither the tree nor the table.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued or written: everything the uncut call refuses but its in_stride (a null
 * tree; a tree of another device; statements without h_index; an index not below 2^depth; for the absent call key_bytes 0 or above 32, length < 2 key_bytes or
 * > 2^20, table_stride < length, key_stride < key_bytes, nq > 0 with d_table, h_keys, h_index or h_status null, a sentinel query), and ncuts = 0 or h_cuts
 * null; cuts that are not 1 <= c_0 < .. < c_G-1 < depth; h_rows or h_strides null; a null pointer in h_rows with rows to write; a stride below its
 * segment's row bytes.  nstmt = 0 or nq = 0 does nothing.
 * Kernel timing kinds: "merkle_climb_rows" (1 per chunk, rows = the chunk's statements x (ncuts + 1)); the absent call also "merkle_locate" (1 per call) and
 * "merkle_absent_rows" (1 per chunk).  Neither launches "merkle_paths". */
int mfh_merkle_paths_cut(mfh_ctx *ctx, const mfh_merkle *t, uint32_t nstmt, const uint32_t *h_index, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                         const size_t *h_strides);
int mfh_merkle_absent_rows_cut(mfh_ctx *ctx, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nq,
                               const uint8_t *h_keys, size_t key_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides,
                               uint32_t *h_index, uint8_t *h_status);
/* ---- RANGE reads of an indexed table (the data model: mfh_merkle_absent_rows): the links of the key range [lo, hi] in key order, and the packed input row of
 * words.MerkleLink(key_bytes, length, depth) -- MerkleRecord's row: 32 zero bytes | the record | depth siblings as words | ceil(depth / 8) index bytes -- of
 * every link.  A LINK of [lo, hi] is a live record (record.lo < record.hi) with record.hi >= lo and record.lo <= hi.  In a well-formed table the links are
 * (p, k_1), (k_1, k_2), .., (k_n, s), where k_1 < .. < k_n are exactly the members inside [lo, hi], p is the largest key below lo (a member or the all-zero
 * sentinel) and s the smallest key above hi: n + 1 links, at least one.  A present-key lookup is the range [k, k]: link 1 is (k, successor) with k's payload.
 *   h_lo, h_hi  the bounds, key_bytes bytes each, lo <= hi, neither a sentinel
 *   max_links   the most links the caller has room for, at most 2^16 (the ordering is quadratic in the links).  0 with null outputs is the COUNT query
 *   *h_count    always the number of links of the whole table
 *   *h_status   0: count <= max_links and the links chain across the range (link 0's lo < lo, every link's hi is the next link's lo, the last link's hi >
 *               hi) -- h_index, h_keys and the rows are written, count entries each.  1: count > max_links, nothing but *h_count is written.  2: the
 *               selected records do not chain (or there is none): the table is malformed; h_index and h_keys are written, the rows are not.
 *   h_index     max_links slots: the links' slots, ordered by (record.lo, slot)
 *   h_keys      max_links x 2 key_bytes bytes, or null: lo | hi of every link, in that order
 *   h_inputs    max_links rows at in_stride, or null for no rows: row i the MerkleLink row of link i (its first 2 key_bytes + reveal record bytes are the
 *               statement's public prefix, whatever `reveal` the statement was built with: the row does not depend on it)
 *   how         three launches select the links in table order (flags and popcounts per workgroup, one-workgroup scan, select: the inert search of
 *               mfh_merkle_insert_keys with another predicate), two put them into key order on the device (a dense array of their keys, then every link's
 *               rank among all of them); count | slots | keys come back in one copy under one wait; the host checks the chain; on status 0 the rows are
 *               mfh_merkle_absent_rows' -- per chunk k_merkle_paths and the gather of the records, spliced on the host.  No atomics: the result does not depend
 *               on the order in which threads run.  Both calls run on the context's stream, synchronise it, stage through the context's pinned buffers
 *               (mfh_scrub_staging covers them) and modify neither the tree nor the table.  One range a call.
 * mfh_merkle_range_rows_cut: the same with the path cut (the conventions of the cut reads above): segment 0's row i, to h_rows[0], is the packed input row of
 * MerkleLink(key_bytes, length, c_0) of link i, 32 + length + 32 c_0 + ceil(c_0 / 8) bytes, and segment g >= 1 a MerkleClimb row; max_links rows a segment.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued or written: a null tree; a tree of another device; key_bytes 0 or above
 * 32; length < 2 key_bytes or > 2^20; table_stride < length; max_links > 2^16; in_stride below the row's bytes (with h_inputs), or for the cut call what the
 * cut conventions refuse (ncuts = 0 or h_cuts null; cuts that are not 1 <= c_0 < .. < c_G-1 < depth; h_rows or h_strides null; a null pointer in h_rows with
 * max_links > 0; a stride below its segment's row bytes); d_table, h_lo, h_hi, h_count or h_status null; max_links > 0 with h_index null; a bound that is the
 * all-zero or the all-0xFF key; lo > hi.
 * Kernel timing kinds: "merkle_range" (flags, scan, select: 3 per call, 2 for the count query; rows = 2^depth on the first), "merkle_range_order" (keys and
 * order: 2 per call with max_links > 0; rows = max_links), then per chunk "merkle_paths" and "merkle_absent_rows", or for the cut call "merkle_climb_rows" and
 * "merkle_absent_rows" and no "merkle_paths". */
int mfh_merkle_range_rows(mfh_ctx *ctx, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, const uint8_t *h_lo,
                          const uint8_t *h_hi, uint32_t max_links, uint32_t *h_count, uint32_t *h_index, uint8_t *h_keys, uint8_t *h_inputs, size_t in_stride,
                          uint8_t *h_status);
int mfh_merkle_range_rows_cut(mfh_ctx *ctx, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes,
                              const uint8_t *h_lo, const uint8_t *h_hi, uint32_t max_links, uint32_t *h_count, uint32_t *h_index, uint8_t *h_keys, uint32_t ncuts,
                              const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_status);
/* nk sequential key REMOVES from an indexed table (the data model: mfh_merkle_absent_rows) and its tree in ONE call, and the packed input row of
 * words.MerkleRemove(key_bytes, length, depth) of every remove -- "key j was removed, and that alone takes the tree from R_j to R_j+1".  The inverse of
 * mfh_merkle_insert_keys: with all-zero inert slots, inserting a batch and removing the same keys restores the table's bytes and the root.
 *   semantics  byte for byte what this gives, run once per key in order: find s, the lowest live record whose own key (lo) is the key, and P, the lowest live
 *              record whose hi is the key, in the table as it then stands; the two updates of a remove -- record P with hi <- the hi of record s, then the
 *              all-zero record into slot s -- through mfh_merkle_update_records.  That covers the table in place, every node of the tree, the roots and row
 *              j, which describes table and tree as they stood before remove j.  Adjacent members may both be in the batch: resolved in order.
 *   arguments  key j is the key_bytes bytes at h_keys + j * key_stride.  h_inputs = NULL: remove, no rows.  h_roots (may be NULL) receives the nk + 1 roots
 *              R_0 .. R_nk.  h_index receives nk pairs (P, s): the slot whose hi changed and the slot that was zeroed.  h_status receives the status of each
 *              key against the table BEFORE the batch: 1 = a member, both records found; 0 = no live record has this key as its own, it is not a member; 2 =
 *              a member, but no live record has it as hi: the table is malformed.
 *   rows       row j (at h_inputs + j * in_stride): 64 zero bytes where the roots are computed | the key | the old record of P | the old record of s | the 32
 *              depth sibling bytes of P | those of s, from the tree after P's update | ceil(2 depth / 8) index bytes, bit l < depth = bit l of P, bit depth +
 *              l = bit l of s.  Exactly 64 + key_bytes + 2 length + 64 depth + ceil(2 depth / 8) bytes are written.
 *   how        ONE launch of k_key_owners (one thread per record, at most two atomic minima each: the lowest index wins on a malformed table) finds own and
 *              prev of every key, and 2 nk words come back; the host plans the slots and the inherited hi within the batch (merkle_remove.hpp); ONE launch
 *              of k_remove_records builds the 2 nk new records; they go through mfh_merkle_update_records' machinery in chunks of whole removes (the most
 *              whose rows fit 64 MiB, at least one).  The call synchronises the stream behind the search and every chunk.
 * mfh_merkle_remove_keys_cut is the same with the path cut (above): segment 0's row, ONE PER REMOVE, is that of MerkleRemove(key_bytes, length, c_0,
 * joined=False) -- 128 zero bytes | key | old P | old s | c_0 siblings of P | c_0 of s | ceil(2 c_0 / 8) index bytes of P mod 2^c_0 and s mod 2^c_0 -- the upper
 * segments have one MerkleSegment row per UPDATE (2 nk), and h_roots receives ALL 2 nk + 1 roots; it has no "no rows" mode.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued: a null tree; a tree of another device; key_bytes 0 or above 32; length
 * < 2 key_bytes or > 2^20; table_stride < length; key_stride < key_bytes; nk > 0 with d_table, h_keys, h_index or h_status null; nk > 2^depth; in_stride
 * below the row's bytes when h_inputs is given; a sentinel key; a key given twice; for the cut call, what the cut calls above refuse.
 * MFH_EINVAL after the search, with h_status and h_index (the located P and s of the table before the batch, 0xFFFFFFFF = none) filled, table and tree
 * unwritten and no record or tree kernel launched: any key of status 0 or 2.  The call is all or nothing.  nk = 0 does nothing.
 * Kernel timing kinds: "merkle_owners" (1 per call, rows = 2^depth), "merkle_remove_records" (1 per call, rows = 2 nk), then per chunk of 2 k updates
 * "sha256_records" (1), "merkle_record_rows" (2; 1 without rows) and "merkle_updates" (depth + 1), the cut call also "merkle_segments" (1). */
int mfh_merkle_remove_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk,
                           const uint8_t *h_keys, size_t key_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots, uint32_t *h_index,
                           uint8_t *h_status);
int mfh_merkle_remove_keys_cut(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk,
                               const uint8_t *h_keys, size_t key_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                               const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status);
/* nk sequential TRANSFERS between the accounts of an indexed table (the data model: mfh_merkle_absent_rows) and its tree in ONE call, and the packed input row
 * of words.MerkleTransfer(key_bytes, length, depth, amount_bytes) of every transfer -- "amount j moved from the account with key from_j to the account with key
 * to_j, and that alone takes the tree from R_j to R_j+1".  A record's BALANCE is its bytes [2 key_bytes, 2 key_bytes + amount_bytes), an unsigned big-endian
 * integer, 1 <= amount_bytes <= 8; a transfer changes nothing else of a record.
 *   semantics  byte for byte what this gives, run once per transfer in order: find p, the lowest live record whose own key (lo) is from_j, and s, that of
 *              to_j; record p with its balance less the amount, then record s with its balance plus the amount, through mfh_merkle_update_records.  That
 *              covers the table in place, every node of the tree, the roots and row j, which describes table and tree as they stood before transfer j.  An
 *              account may occur in ANY number of steps, as sender and as receiver -- the one batch in which a key may be given many times -- and a step sees
 *              the balances the earlier steps left: it may spend what an earlier step of the batch delivered.
 *   arguments  sender j is the key_bytes bytes at h_from + j * key_stride, receiver j those at h_to + j * key_stride, h_amounts[j] the amount, below
 *              2^(8 amount_bytes).  h_inputs = NULL: transfer, no rows.  h_roots (may be NULL) receives the nk + 1 roots R_0 .. R_nk.  h_index receives nk
 *              pairs (p, s), 0xFFFFFFFF for a key that is no member.  h_status receives per step the first that applies: 0 = fine; 1 = the sender is not a
 *              member; 2 = the receiver is not a member; 3 = an overdraft, the amount exceeds the sender's balance AT THAT STEP; 4 = an overflow, the
 *              receiver's balance at that step plus the amount exceeds 2^(8 amount_bytes) - 1.  A step with a status is left out of the balances the later
 *              steps are judged by.
 *   rows       row j (at h_inputs + j * in_stride): 64 zero bytes where the roots are computed | from_j | to_j | the amount as amount_bytes big-endian bytes |
 *              the old record of p | the old record of s | the 32 depth sibling bytes of p | those of s, from the tree after p's update | ceil(2 depth / 8)
 *              index bytes, bit l < depth = bit l of p, bit depth + l = bit l of s.  Exactly 64 + 2 key_bytes + amount_bytes + 2 length + 64 depth +
 *              ceil(2 depth / 8) bytes are written.
 *   how        ONE launch of k_key_locate over the sorted unique keys of all 2 nk senders and receivers and, behind it on the stream, ONE launch of
 *              k_balance_gather (one thread per unique key: the located record's balance as a uint64); 2 words and one balance per unique key come back under
 *              ONE wait.  The host walks the steps in order over a running balance per account (merkle_transfer.hpp); ONE launch of k_refield_records
 *              builds the 2 nk new records from the table before the batch and the uploaded new balances; they go through mfh_merkle_update_records'
 *              machinery in chunks of whole transfers (the most whose rows fit 64 MiB, at least one).  The call synchronises the stream behind the search
 *              and every chunk.
 * mfh_merkle_transfer_keys_cut is the same with the path cut (above): segment 0's row, ONE PER TRANSFER, is that of MerkleTransfer(key_bytes, length, c_0,
 * amount_bytes, joined=False) -- 128 zero bytes | from | to | amount | old p | old s | c_0 siblings of p | c_0 of s | ceil(2 c_0 / 8) index bytes of p mod
 * 2^c_0 and s mod 2^c_0 -- the upper segments have one MerkleSegment row per UPDATE (2 nk), and h_roots receives ALL 2 nk + 1 roots; it has no "no rows" mode.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued: a null tree; a tree of another device; key_bytes 0 or above 32;
 * amount_bytes 0 or above 8; length < 2 key_bytes + amount_bytes or > 2^20; table_stride < length; key_stride < key_bytes; nk > 0 with d_table, h_from, h_to,
 * h_amounts, h_index or h_status null (nk may exceed 2^depth: accounts repeat); in_stride below the row's bytes when h_inputs is given; a sentinel key as sender or receiver; a transfer
 * from an account to itself (from_j == to_j: a no-op, which the statement allows and the call has nothing to do for); an amount of 2^(8 amount_bytes) or more;
 * for the cut call, what the cut calls above refuse.
 * MFH_EINVAL after the search, with h_status and h_index filled, table and tree unwritten and no record or tree kernel launched: any step with a status
 * other than 0.  The call is all or nothing.  nk = 0 does nothing.
 * Kernel timing kinds: "merkle_locate" (1 per call, rows = 2^depth), "merkle_balances" (1 per call, rows = the unique keys), "merkle_transfer_records" (1 per
 * call, rows = 2 nk), then per chunk of 2 k updates "sha256_records" (1), "merkle_record_rows" (2; 1 without rows) and "merkle_updates" (depth + 1), the
 * cut call also "merkle_segments" (1). */
int mfh_merkle_transfer_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                             uint32_t nk, const uint8_t *h_from, const uint8_t *h_to, size_t key_stride, const uint64_t *h_amounts, uint8_t *h_inputs,
                             size_t in_stride, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status);
int mfh_merkle_transfer_keys_cut(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                                 uint32_t nk, const uint8_t *h_from, const uint8_t *h_to, size_t key_stride, const uint64_t *h_amounts, uint32_t ncuts,
                                 const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index,
                                 uint8_t *h_status);

/* nk sequential DEPOSITS and WITHDRAWALS on the accounts of an indexed table whose records carry a balance (the data model: mfh_merkle_transfer_keys) and its
 * tree in ONE call, and the packed input row of words.MerkleAdjust(key_bytes, length, depth, amount_bytes) of every step -- "the balance of the account with key
 * k_j went up (side 0) or down (side 1) by amount j, and that alone takes the tree from R_j to R_j+1".  What funds and drains the ledger that the transfers
 * move value within; an adjust changes nothing of a record but its balance.
 *   semantics  byte for byte what this gives, run once per step in order: find the lowest live record whose own key (lo) is k_j; that record with its balance
 *              plus or less the amount, through mfh_merkle_update_records.  That covers the table in place, every node of the tree, the roots and row j, which
 *              describes table and tree as they stood before step j.  A key may occur in ANY number of steps, and a step sees the balance the earlier steps
 *              left: a withdrawal may spend what an earlier deposit of the batch delivered.
 *   arguments  key j is the key_bytes bytes at h_keys + j * key_stride, h_amounts[j] the amount, below 2^(8 amount_bytes), h_sides[j] the direction, 0 = deposit,
 *              1 = withdrawal; h_sides = NULL: all deposits.  h_inputs = NULL: adjust, no rows.  h_roots (may be NULL) receives the nk + 1 roots R_0 .. R_nk.
 *              h_index receives the nk records, 0xFFFFFFFF for a key that is no member.  h_status receives per step the first that applies: 0 = fine; 1 = the
 *              key is not a member; 3 = an overdraft, a withdrawal above the account's balance AT THAT STEP; 4 = an overflow, a deposit that takes the balance
 *              at that step past 2^(8 amount_bytes) - 1 (2 is unused: the numbers mean what mfh_merkle_transfer_keys' mean).  A step with a status is left
 *              out of the balances the later steps are judged by.
 *   rows       row j (at h_inputs + j * in_stride): 64 zero bytes where the roots are computed | k_j | the amount as amount_bytes big-endian bytes | the side
 *              byte | the old record | the 32 depth sibling bytes | ceil(depth / 8) index bytes.  Exactly 64 + key_bytes + amount_bytes + 1 + length +
 *              32 depth + ceil(depth / 8) bytes are written.
 *   how        ONE launch of k_key_locate over the sorted unique keys and, behind it on the stream, ONE launch of k_balance_gather; 2 words and one balance
 *              per unique key come back under ONE wait.  The host walks the steps in order over a running balance per account (merkle_adjust.hpp); ONE launch
 *              of k_refield_records builds the nk new records from the table before the batch and the uploaded new balances; they go through
 *              mfh_merkle_update_records' machinery in its chunks (the most updates whose rows fit 64 MiB, at least one).  The call synchronises the stream
 *              behind the search and every chunk.
 * mfh_merkle_adjust_keys_cut is the same with the path cut (above), exactly as mfh_merkle_update_records_cut for nk updates: segment 0's row is that of
 * MerkleAdjust(key_bytes, length, c_0, amount_bytes) -- 64 zero bytes | k | amount | side | old record | c_0 siblings | ceil(c_0 / 8) index bytes of the record
 * mod 2^c_0 -- every upper segment has ONE MerkleSegment row per step, and h_roots (may be NULL) receives the nk + 1 roots; it has no "no rows" mode.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued: a null tree; a tree of another device; key_bytes 0 or above 32;
 * amount_bytes 0 or above 8; length < 2 key_bytes + amount_bytes or > 2^20; table_stride < length; key_stride < key_bytes; nk > 0 with d_table, h_keys,
 * h_amounts, h_index or h_status null (nk may exceed 2^depth: keys repeat); in_stride below the row's bytes when h_inputs is given; a sentinel key; a side
 * above 1; an amount of 2^(8 amount_bytes) or more; for the cut call, what the cut calls above refuse.
 * MFH_EINVAL after the search, with h_status and h_index filled, table and tree unwritten and no record or tree kernel launched: any step with a status
 * other than 0.  The call is all or nothing.  nk = 0 does nothing.
 * Kernel timing kinds: "merkle_locate" (1 per call, rows = 2^depth), "merkle_balances" (1 per call, rows = the unique keys), "merkle_adjust_records" (1 per
 * call, rows = nk), then per chunk of k updates "sha256_records" (1), "merkle_record_rows" (2; 1 without rows) and "merkle_updates" (depth + 1), the cut call
 * also "merkle_segments" (1). */
int mfh_merkle_adjust_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                           uint32_t nk, const uint8_t *h_keys, size_t key_stride, const uint64_t *h_amounts, const uint8_t *h_sides, uint8_t *h_inputs,
                           size_t in_stride, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status);
int mfh_merkle_adjust_keys_cut(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                               uint32_t nk, const uint8_t *h_keys, size_t key_stride, const uint64_t *h_amounts, const uint8_t *h_sides, uint32_t ncuts,
                               const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index,
                               uint8_t *h_status);
/* nk sequential WRITES BY KEY on an indexed table and its tree in ONE call, plain or compare-and-set, and the packed input row of
 * words.MerkleWrite(key_bytes, length, depth, (field_lo, field_hi), expect) of every step -- "bytes [field_lo, field_hi) of the record of key k_j were set to
 * v_j [, having been e_j], and that alone takes the tree from R_j to R_j+1".  The put of the keyed store: the field is any part of the payload, 2 key_bytes <=
 * field_lo < field_hi <= length, F = field_hi - field_lo bytes, one field for the whole call; the keys are never writable.
 *   semantics  byte for byte what this gives, run once per step in order: find the lowest live record whose own key (lo) is k_j; if expectations are given and
 *              its field is not e_j the step fails; else that record with the field set to v_j, through mfh_merkle_update_records.  That covers the table in
 *              place, every node of the tree, the roots and row j, which describes table and tree as they stood before step j.  A key may occur in ANY number
 *              of steps, and a step sees what the earlier steps of the batch left: an expectation may be met by an earlier write alone, or broken by one.
 *   arguments  key j is the key_bytes bytes at h_keys + j * key_stride, v_j the F bytes at h_values + j * value_stride, e_j the F bytes at h_expect + j *
 *              expect_stride.  h_expect = NULL: every step is unconditional (expect_stride is ignored); a call is all-conditional or all-plain, as a circuit
 *              is.  h_inputs = NULL: write, no rows.  h_roots (may be NULL) receives the nk + 1 roots R_0 .. R_nk.  h_index receives the nk records, 0xFFFFFFFF
 *              for a key that is no member.  h_status receives per step the first that applies: 0 = fine; 1 = the key is not a member; 5 = the field is not
 *              what was expected AT THAT STEP (2 to 4 are unused: the numbers keep their meaning across the key calls).  A step with a status is left out of
 *              the values the later steps are judged by.
 *   rows       row j (at h_inputs + j * in_stride): 64 zero bytes where the roots are computed | k_j | with h_expect e_j | v_j | the old record | the 32 depth
 *              sibling bytes | ceil(depth / 8) index bytes.  Exactly 64 + key_bytes + F (2 F with h_expect) + length + 32 depth + ceil(depth / 8) bytes are
 *              written.
 *   how        ONE launch of k_key_locate over the sorted unique keys; with h_expect, behind it on the stream, ONE launch of k_field_gather (a slot of
 *              ceil(F / 16) 16-byte units per unique key); the results come back under ONE wait.  The host walks the steps in order over a running field value
 *              per unique key (merkle_write.hpp); ONE launch of k_refield_records builds the nk new records from the table before the batch and the uploaded
 *              values; they go through mfh_merkle_update_records' machinery in its chunks (the most updates whose rows fit 64 MiB, at least one).  The call
 *              synchronises the stream behind the search and every chunk.
 * mfh_merkle_write_keys_cut is the same with the path cut (above), exactly as mfh_merkle_adjust_keys_cut: segment 0's row is that of MerkleWrite(key_bytes,
 * length, c_0, field, expect) -- 64 zero bytes | k | [e |] v | old record | c_0 siblings | ceil(c_0 / 8) index bytes of the record mod 2^c_0 -- every upper
 * segment has ONE MerkleSegment row per step, and h_roots (may be NULL) receives the nk + 1 roots; it has no "no rows" mode.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued: what mfh_merkle_adjust_keys refuses of the arguments the two share;
 * field_lo < 2 key_bytes; field_hi <= field_lo; field_hi > length; value_stride < F; expect_stride < F with h_expect; nk > 0 with h_values null; in_stride
 * below the row's bytes when h_inputs is given; for the cut call, what the cut calls above refuse.
 * MFH_EINVAL after the search, with h_status and h_index filled, table and tree unwritten and no record or tree kernel launched: any step with a status
 * other than 0.  The call is all or nothing.  nk = 0 does nothing.
 * Kernel timing kinds: "merkle_locate" (1 per call, rows = 2^depth), "merkle_fields" (1 per call with h_expect, none without; rows = the unique keys),
 * "merkle_write_records" (1 per call, rows = nk), then per chunk as mfh_merkle_adjust_keys. */
int mfh_merkle_write_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t field_lo,
                          uint32_t field_hi, uint32_t nk, const uint8_t *h_keys, size_t key_stride, const uint8_t *h_values, size_t value_stride,
                          const uint8_t *h_expect, size_t expect_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots, uint32_t *h_index,
                          uint8_t *h_status);
int mfh_merkle_write_keys_cut(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t field_lo,
                              uint32_t field_hi, uint32_t nk, const uint8_t *h_keys, size_t key_stride, const uint8_t *h_values, size_t value_stride,
                              const uint8_t *h_expect, size_t expect_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                              const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status);
/* A BLOCK: nk sequential steps of MIXED kinds -- transfers, adjusts and writes in any order -- on an indexed table whose records carry a balance and its tree
 * in ONE call, and every step's packed input row: that of words.MerkleTransfer, words.MerkleAdjust or words.MerkleWrite, as the three calls above write it.
 * key_bytes and amount_bytes hold for the whole call; a write's field is PER STEP.  A write may cover balance bytes: a later transfer or adjust of the block
 * then reads the balance those bytes spell.  No step changes membership (inserts and removes are no kinds of a block), so one search serves all steps.
 *   semantics  byte for byte what the three calls give, run once per step in order on the same table and tree: the table's whole allocation, every node of
 *              the tree, the roots and row j, which describes table and tree as they stood before step j.  A key may occur in ANY number of steps of any
 *              kind, and a step sees what the earlier steps of the block left.
 *   arguments  h_kinds[j]: 0 = a transfer, 1 = an adjust, 2 = a write.  Key j, the key_bytes bytes at h_keys + j * key_stride, is the sender, the account or
 *              the written key; h_keys_to + j * key_stride is a transfer's receiver (read for transfers only; NULL in a block without one).  h_amounts[j]
 *              (transfers and adjusts; NULL in a block of writes) is below 2^(8 amount_bytes); h_sides[j] (adjusts) is 0 = a deposit or 1 = a withdrawal,
 *              h_sides = NULL: all deposits.  A write's field is bytes [h_fields[2 j], h_fields[2 j + 1]) of the record, 2 key_bytes <= lo < hi <= length,
 *              its value the hi - lo bytes at h_values + h_value_at[j] (inside the buffer's values_bytes bytes) and its expectation, if it has one, those
 *              at h_expect + h_expect_at[j] (inside expect_bytes); h_expect_at[j] = MFH_BLOCK_NO_EXPECT or h_expect_at = NULL: a plain write.  These
 *              arrays have nk entries each and are read at the steps of their kinds alone.  skip_failed: the policy, below.
 *   outputs    h_rows (may be NULL: no rows) is ONE buffer: row j is written at h_rows + h_row_at[j], and h_row_at has nk + 1 entries, the slot of row j
 *              being [h_row_at[j], h_row_at[j + 1]) -- at least mfh_merkle_block_row_bytes of the step.  h_index receives nk PAIRS: (the sender's
 *              record, the receiver's) of a transfer, (the record, 0xFFFFFFFF) of a one-record step, 0xFFFFFFFF for a key that is no member.  h_status
 *              receives per step the first that applies, with the numbers of the three calls: 0 = fine; 1 = the key (a transfer's sender) is not a member; 2 =
 *              a transfer's receiver is not a member; 3 = an overdraft against the RUNNING balance; 4 = an overflow of the running balance; 5 = the RUNNING
 *              field is not what the step expects.  A step with a status is not applied, and the steps behind it are judged without it.
 *              h_first_update receives nk + 1 entries: step j's record updates are [h_first_update[j], h_first_update[j + 1]), none, one or two, and nupd =
 *              h_first_update[nk].  h_roots (may be NULL; room for 2 nk + 1 roots) receives the nupd + 1 roots, one behind EVERY update: the root before
 *              step j is root h_first_update[j], the root behind it root h_first_update[j + 1].
 *   policy     skip_failed = 0, fail-fast: any status other than 0 returns MFH_EINVAL after the search with h_status, h_index and h_first_update (all zero)
 *              filled, table and tree unwritten and no record or tree kernel launched.  skip_failed = 1: the steps with a status are left out -- no update,
 *              their row's slot is not touched, R_j+1 = R_j -- every other step is applied as if the block had been given without them, and the call
 *              returns MFH_OK with the statuses.
 *   how        ONE launch of k_key_locate over the sorted unique keys of all steps and behind it ONE of k_window_gather: unique key u has a WINDOW of its
 *              record, the hull of what its steps touch (the balance field for transfers and adjusts, every written field), gathered into a slot of
 *              ceil(window bytes / 16) 16-byte units; both come back under ONE wait.  The host walks the steps in order over the running window bytes
 *              (merkle_block.hpp); ONE launch of k_window_records builds all nupd new records from the table before the block, per-update descriptors and
 *              the uploaded window bytes; they go through mfh_merkle_update_records' machinery in uniform chunks of updates (the most whose rows fit 64 MiB
 *              when every update is charged the most row bytes an update of any step stands for, at least one).  A transfer whose two updates fall into two
 *              chunks is spliced from a host copy of its first update's pieces.  The call synchronises the stream behind the search and every chunk.
 * mfh_merkle_block_keys_cut is the same with the path cut (above): h_rows[0] is the one buffer of the segment-0 rows, addressed through h_row_at -- a
 * transfer's is that of MerkleTransfer(.., c_0, joined=False), 128 zero bytes in front, an adjust's and a write's the statement's own at depth c_0 -- and
 * h_strides[0] is not read; every upper segment g has ONE MerkleSegment row per UPDATE, update r's at h_rows[g] + r * h_strides[g], so its array has room
 * for the updates of all steps.  It has no "no rows" mode.
 * MFH_EINVAL, with its own mfh_last_error text naming the function and nothing queued: what mfh_merkle_adjust_keys refuses of the table, the keys and
 * amount_bytes; nk > 0 with h_kinds, h_first_update or, with rows, h_row_at null; a kind above 2; a transfer without h_keys_to, with a sentinel receiver or
 * to its own sender; a transfer or an adjust without h_amounts or with an amount above 2^(8 amount_bytes) - 1; a side above 1; a write without h_fields,
 * h_value_at or h_values, with lo < 2 key_bytes, hi <= lo or hi > length, with a value outside h_values or an expectation outside h_expect; a row slot
 * shorter than the step's row; 2^32 or more window bytes summed over the updates of all steps, one window of its key an update (the new records' units are
 * bounded as in mfh_merkle_adjust_keys, which bounds the gather's units too); for the cut call, what the cut calls above refuse.  nk = 0 does nothing.
 * Kernel timing kinds: "merkle_locate" (1 per call, rows = 2^depth), "merkle_block_windows" (1 per call, rows = the unique keys), "merkle_block_records" (1
 * per call with an update, rows = nupd), then per chunk as mfh_merkle_adjust_keys on nupd updates. */
#define MFH_BLOCK_NO_EXPECT (~(uint64_t)0)
int mfh_merkle_block_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                          uint32_t nk, const uint8_t *h_kinds, const uint8_t *h_keys, const uint8_t *h_keys_to, size_t key_stride, const uint64_t *h_amounts,
                          const uint8_t *h_sides, const uint32_t *h_fields, const uint64_t *h_value_at, const uint8_t *h_values, size_t values_bytes,
                          const uint64_t *h_expect_at, const uint8_t *h_expect, size_t expect_bytes, uint32_t skip_failed, uint8_t *h_rows,
                          const uint64_t *h_row_at, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status, uint32_t *h_first_update);
int mfh_merkle_block_keys_cut(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                              uint32_t nk, const uint8_t *h_kinds, const uint8_t *h_keys, const uint8_t *h_keys_to, size_t key_stride,
                              const uint64_t *h_amounts, const uint8_t *h_sides, const uint32_t *h_fields, const uint64_t *h_value_at, const uint8_t *h_values,
                              size_t values_bytes, const uint64_t *h_expect_at, const uint8_t *h_expect, size_t expect_bytes, uint32_t skip_failed,
                              uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, const uint64_t *h_row_at,
                              uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status, uint32_t *h_first_update);
/* the bytes of a block step's row: kind as h_kinds has it, a write's field (field_lo, field_hi) and whether it has an expectation (both ignored for the other
 * kinds), over `depth` levels; cut != 0: a segment-0 row of a cut call, depth = c_0.  0 for a kind above 2 */
size_t mfh_merkle_block_row_bytes(uint32_t kind, uint32_t key_bytes, uint32_t amount_bytes, uint32_t length, uint32_t depth, uint32_t field_lo,
                                  uint32_t field_hi, uint32_t expect, uint32_t cut);
/* The SUPPLY of such a table: h_sum[0] | h_sum[1] << 64 = the sum of the balances (bytes [2 key_bytes, 2 key_bytes + amount_bytes), big-endian) of all LIVE
 * records (lo < hi) of the 2^depth records at d_table, *h_live (may be NULL) their number.  What is in the balance bytes of a record that is not live does
 * not count.  The table is only read; the tree is used for its depth alone.  Transfers leave the sum as it is, a batch of adjusts changes it by its deposits
 * less its withdrawals.
 *   how        ONE launch of k_balance_sum (one thread per record, a 128-bit sum reduced per wave by shuffles and per workgroup through LDS, one partial a
 *              workgroup) and ONE of k_balance_fold (one workgroup), no atomics; 20 bytes come back under ONE wait.
 * MFH_EINVAL with the function's name in mfh_last_error: a null tree; a tree of another device; key_bytes 0 or above 32; amount_bytes 0 or above 8; length <
 * 2 key_bytes + amount_bytes or > 2^20; table_stride < length; d_table or h_sum null.
 * Kernel timing kind: "merkle_balance_sum" (2 per call, rows = 2^depth on the first and 0 on the fold). */
int mfh_merkle_balance_sum(mfh_ctx *ctx, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes,
                           uint32_t amount_bytes, uint64_t h_sum[2], uint32_t *h_live);
/* LOAD a whole indexed table from a key set that is on the device, and its tree: the genesis of a ledger, where mfh_merkle_insert_keys is for increments.
 * d_keys: nk x key_bytes packed bytes, in ANY order; d_payloads: nk x payload_bytes packed bytes in the order of the keys, or NULL (zero payloads).
 * On status 0 the WHOLE table and the WHOLE tree are written: slot 0 <- the sentinel record (00..00 | the smallest key), slots 1 .. nk <- one record (key |
 * next larger key | payload, zero-padded to length) per member in ascending key order, the last with hi = FF..FF, slots nk + 1 .. 2^depth - 1 <- all zero;
 * bytes [length, table_stride) of a slot are left as they were; the tree <- what mfh_merkle_set_records(t, 0, 2^depth, d_table, table_stride, length) gives.
 * nk = 0 gives the single record (00..00 | FF..FF).  h_status = {status, where0, where1}:
 *   0  loaded (where0 = where1 = 0xFFFFFFFF)
 *   2  a key is a sentinel, all-zero or all-0xFF over its bytes: where0 = the lowest input index of such a key.  Goes before status 1
 *   1  a key is given twice: where0 < where1 = the two lowest input indices of the SMALLEST duplicated key
 * and with a status other than 0 NOTHING of the table or the tree is written.
 *   how        k_load_entries (the keys' words and the tag = input index; the sentinel check), key_sort -- k_sort_tiles (tiles of 1 024 entries sorted in LDS)
 *              and ceil(log2(ceil(nk / 1024))) launches of k_sort_merge (merge-path partition, one pass a launch between two buffers), no atomics, ONE
 *              permutation whatever the scheduling --, k_load_dups and k_load_dup_tags on the sorted neighbours, ONE wait for 16 bytes of status, then
 *              k_load_records (every record of the table, at any byte alignment and stride), k_sha256_records and the depth launches of k_merkle_level.
 *              Scratch: two buffers of nk (ceil(key_bytes / 4) + 1) words in the context's growable scratch.  Queued on the context's stream behind whatever
 *              produced d_keys there.
 * MFH_EINVAL with the function's name in mfh_last_error, nothing launched and nothing written: a null tree; a tree of another device; nk > 2^depth - 1;
 * key_bytes 0 or above 32; length < 2 key_bytes + payload_bytes or > 2^20; table_stride < length; d_table null; d_keys null with nk > 0; d_payloads given
 * with payload_bytes = 0; h_status null.
 * Kernel timing kinds: "merkle_sort" (1 + the merge passes; rows = nk each), "merkle_load" (3 in front of the wait, none for nk = 0, and the build launch,
 * rows = 2^depth), then "sha256_records" (1) and "merkle_level" (depth). */
int mfh_merkle_load_keys(mfh_ctx *ctx, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk,
                         const uint8_t *d_keys, const uint8_t *d_payloads, uint32_t payload_bytes, uint32_t h_status[3]);
/* CHECK the invariant every key statement is sound relative to: the live records (lo < hi) of the 2^depth records at d_table tile the key space in ONE chain
 * from 00..00 to FF..FF, the tree's leaves are the records' SHA-256 and every node is the compression of its children.  Only reads table and tree.
 * h_out = {status, live, where0, where1}, live = the number of live records:
 *   0  all good
 *   1  the chain: with the live records sorted by (lo, slot), where0 = the slot of the first record at which it breaks -- sorted record 0 when its lo is not
 *      00..00, sorted record i + 1 at the lowest i with hi_i != lo_i+1, the last record when its hi is not FF..FF --, 0xFFFFFFFF when no record is live
 *   2  the leaves (the chain is good): where0 = the lowest slot whose record does not hash to its leaf, inert slots included
 *   3  the nodes (chain and leaves are good): where0 = the lowest level with a wrong node, the leaves' parents being level 1, where1 = the lowest index there
 *   how        k_range_flags (bounds 00..00 and FF..FF), k_inert_scan, k_inert_select, k_range_keys with max_links = 2^depth; one wait for the count; then
 *              k_check_entries, key_sort of (lo, rank in table order), k_chain_check, k_sha256_records into scratch, k_leaf_check and one k_node_check a
 *              level, all queued whatever the chain says, and ONE wait for 32 bytes of results.  Scratch: the range reads' with max_links = 2^depth, the
 *              sort's two buffers and 32 bytes a slot of digests.
 * MFH_EINVAL as above: a null tree; a tree of another device; key_bytes 0 or above 32; length < 2 key_bytes or > 2^20; table_stride < length; d_table or
 * h_out null.
 * Kernel timing kinds: "merkle_check" (4, and with a live record 3 + depth more), "merkle_sort" (as above, n = live), "sha256_records" (1). */
int mfh_merkle_check_table(mfh_ctx *ctx, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes,
                           uint32_t h_out[4]);
/* GROW a tree and its table: *out <- a NEW tree of new_depth > depth whose leftmost subtree of height depth is t and whose other leaves are all the inert
 * leaf E_0 = SHA-256 of `length` zero bytes; records [0, 2^depth) of d_new_table <- those of d_table and records [2^depth, 2^new_depth) <- all zero (bytes
 * [0, length) of each; bytes [length, new_stride) and everything outside the new table's span are left as they were).  An all-zero record has lo >= hi: the
 * new slots are inert, the grown pair has the invariant of mfh_merkle_check_table exactly when the old pair had it, and every key call and cut call runs on
 * it unchanged.  No record is hashed: with E_l+1 = node(E_l, E_l), the root of every subtree of height l right of the old tree is the constant E_l, and the
 * nodes above the old root R are S_depth = R, S_l+1 = node(S_l, E_l) -- the new root R' = S_new_depth is new_depth - depth compressions of PUBLIC values, which
 * a verifier following a chain of roots evaluates himself (words.grown_root): the jump R -> R' needs no proof.
 * t and d_table are only read and stay valid and unchanged; *out is destroyed by mfh_merkle_destroy like a created tree.
 * d_table and d_new_table may BOTH be NULL: the tree alone is grown, for a table kept elsewhere (the strides are then unused).
 * h_roots: NULL, or 64 bytes <- R | R'.  With NULL the call is queue-only on the context's stream and does not wait; with h_roots it waits once.
 *   how        the host computes E_0 .. E_new_depth (csrc/merkle_grow.hpp: microseconds) and hands them to the kernels as an argument; the nodes are
 *              allocated and NOT built as a zero tree first; k_grow_nodes (one launch over the whole memory of the new tree, a 16-byte unit a lane: a copy of
 *              an old node or a constant), k_grow_spine (one thread: the new_depth - depth nodes above the old root, from the old tree and the constants
 *              alone) and k_grow_table (16-byte windows of the destination's dword grid: any byte alignment and stride on either side); no atomics, no LDS,
 *              no scratch.
 * MFH_EINVAL with the function's name in mfh_last_error, nothing queued and *out untouched: a null tree; a tree of another device; out null; new_depth <=
 * depth or > 24; length > 2^20; table_stride or new_stride < length; one of d_table, d_new_table without the other; a new table whose span [d_new_table,
 * d_new_table + (2^new_depth - 1) new_stride + length) overlaps the old table's; 2^new_depth ceil((length + 3) / 16) >= 2^32.  MFH_ENOMEM: no memory for the
 * nodes.
 * Kernel timing kind: "merkle_grow" (3 per call with the tables, 2 without; rows = the 2^(new_depth + 1) nodes, the new_depth - depth spine nodes, the
 * 2^new_depth records); no "sha256_records" and no "merkle_level" launch. */
int mfh_merkle_grow(mfh_ctx *ctx, const mfh_merkle *t, uint32_t new_depth, const uint8_t *d_table, size_t table_stride, uint32_t length,
                    uint8_t *d_new_table, size_t new_stride, mfh_merkle **out, uint8_t *h_roots);
/* ... the same for a tree of LEAVES (mfh_merkle_set_leaves): E_0 = 32 zero bytes, the leaf of mfh_merkle_create, whose fresh root of depth D is E_D. */
int mfh_merkle_grow_leaves(mfh_ctx *ctx, const mfh_merkle *t, uint32_t new_depth, mfh_merkle **out, uint8_t *h_roots);

/* ---- L3/L4: polynomial step, setup, prover ------------------------------------------------------------ */
/* c = a*b over F_p[x] (la+lb-1 canonical coefficients).  What nmod_poly_mul/pow compute (src/snark.c:167).
 * Limit: la + lb - 1 <= 2^23 (the NTT primes have 2-adicity 23); longer products fail with MFH_EUNSUPPORTED.  A product longer than the
 * transforms the context has prepared rebuilds them and forgets the prepared t: mfh_poly_h* then fail until mfh_poly_prepare_t is called again. */
int mfh_poly_mul(mfh_ctx *ctx, const uint32_t *d_a, size_t la, const uint32_t *d_b, size_t lb, uint32_t *d_c);
int mfh_poly_add(mfh_ctx *ctx, const uint32_t *d_a, const uint32_t *d_b, size_t count, uint32_t *d_out);
/* Per-SSP precomputation for the quotient by t(x): power-series inverse of rev(t) (and its transform).
 * d_t = d coefficients (slot 0 of the device SSP).  Fails (MFH_EINVAL) for t = 0, where nmod_poly_div raises.
 * Limit: 4 d - deg t <= 2^23, i.e. d <= 2 796 202 when deg t = d - 1 and d <= 2^21 when deg t is small; beyond it MFH_EUNSUPPORTED.
 * A call that fails leaves no t prepared (mfh_poly_h* fail until a call succeeds). */
int mfh_poly_prepare_t(mfh_ctx *ctx, const uint32_t *d_t);
int mfh_ssp_prepare(mfh_ctx *ctx, const uint32_t *d_ssp); /* = mfh_poly_prepare_t(slot 0) */
/* h = floor((v^2 - 1) / t), first d coefficients (nmod_poly_pow/sub/div, src/snark.c:166-169).  v: d coefficients. */
int mfh_poly_h(mfh_ctx *ctx, const uint32_t *d_v, uint32_t *d_h);
/* the same for nb polynomials side by side (v_k at d_v + k d, h_k at d_h + k d): one set of launches for the whole batch.
 * Limit: 1 <= nb <= 21845 (three grid rows per polynomial, 65535 at most); MFH_EINVAL outside. */
int mfh_poly_h_multi(mfh_ctx *ctx, const uint32_t *d_v, uint32_t *d_h, uint32_t nb);
/* A batch (nb >= 4) takes the exact-division path when the prepared t has degree d - 1 and is a unit modulo x^N - 1 (N = the power of two >= d): a prover with a valid
 * witness divides exactly (src/ssp.c:37-77), and then h = (v^2 - 1 mod x^N - 1) t^-1 mod x^N - 1 -- two cyclic products of length N instead of two linear ones of
 * length 2N.  Every result is CHECKED on the device (h(r) t(r) = v(r)^2 - 1 at four points drawn per preparation from the kernel's entropy, so that a wrong h for a
 * v chosen without knowledge of them survives with probability <= (2d / p)^4 < 2^-64); the statements that fail -- a witness that does not satisfy the SSP
 * -- are recomputed by the Euclidean division above, by kernels queued behind the check (no host round trip; a batch with k such statements pays that path for k):
 * the output is nmod_poly_div's but for that probability.  mode 1 (the default): as described, except that after a batch in which the check has failed the next
 * 64 batches take the Euclidean path alone before the exact path is tried again (a caller whose statements do not satisfy the SSP would pay both; the failure is
 * noticed through a word in host memory whenever the device gets there -- a hint, nothing is waited for).  mode 2: every batch tries the exact path (A/B, tests).
 * mode 0: never.  Setting a mode forgets what earlier batches have taught.  The points: mfh_poly_exact_points, mfh_set_poly_exact_points below. */
int mfh_set_poly_exact(mfh_ctx *ctx, int mode);
/* statements that failed that check (and were recomputed) since the last call; waits for the stream.  -1: the prepared t has no exact-division path */
long mfh_poly_exact_fallbacks(mfh_ctx *ctx);
/* the four points of that check for the prepared t (out[4]).  MFH_EINVAL: no t prepared, or it has no exact-division path. */
int mfh_poly_exact_points(mfh_ctx *ctx, uint32_t *out);
/* pin the check points (tests, reproducible runs): pts = four distinct values in [2, p - 1), used from the next mfh_poly_prepare_t on until unpinned; pts = NULL
 * unpins (the next preparation draws them again).  MFH_EINVAL for a value out of range or a repeated one (and the setting is left as it was). */
int mfh_set_poly_exact_points(mfh_ctx *ctx, const uint32_t *pts);

/* The 2d+m plaintexts setup() encrypts, in stream order: s^i | alpha s^i | beta t(s) | beta v_i(s), i=1..m-1
 * (src/snark.c:73-110; the Horner values nmod_poly_evaluate_nmod are computed as dot products with the powers of s). */
int mfh_setup_messages(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t alpha, uint32_t beta, uint32_t s, uint32_t *d_msg);
/* setup() (src/snark.c:57-115) with caller-supplied secrets: d_sk = n values (key_gen, src/lwe.c:30-34),
 * d_err = (2d+m) error values in encryption order (errdist_uniform, src/lwe.c:60-63).  The public seed is the one
 * given to mfh_set_seed (crs->seed).  Output: the device CRS, (2d+m)*CT_BYTES bytes in stream order
 * s[0..d) | as[0..d) | t | v[0..m-1)  (struct crs, src/snark.h:27-33, keeps them in four arrays). */
int mfh_setup(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t alpha, uint32_t beta, uint32_t s, const uint64_t *d_sk,
              const uint64_t *d_err, uint8_t *d_crs_c8);
/* The same, leaving the expanded rows behind as a by-product ("writing the expanded rows to HBM as a by-product, so the prover starts with a materialised
 * CRS"): d_rows_image (may be NULL: then this is mfh_setup) receives all 2d+m rows in the layout of mfh_crs_expand -- (2d+m) x mfh_resident_row_bytes() bytes, what
 * mfh_crs_set_resident registers and mfh_prove streams -- so that the first proof under the new CRS does not regenerate a single a-vector.  The rows are written by a second
 * pass over the stream (the expansion kernel of mfh_crs_expand, queued behind the encryptions); the encryption kernel itself keeps the keystream in its MFMA operand
 * registers (csrc/encmm.hip) and would have to scatter it in 4-byte pieces to lay it out. */
int mfh_setup_image(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t alpha, uint32_t beta, uint32_t s, const uint64_t *d_sk,
                    const uint64_t *d_err, uint8_t *d_crs_c8, void *d_rows_image);
/* prover() (src/snark.c:117-190) with caller-supplied entropy: delta (< p; the reference draws 8 bytes % p) and the
 * five smudging draws in call order h, hat_h, hat_v, v_w, v_w (sic: v_w twice, b_w never; src/snark.c:185-189):
 * h_smudge_mag = 5*maglen bytes, h_smudge_sign = 5 bytes.  Needs mfh_set_seed(crs seed) and mfh_ssp_prepare.
 * d_proof = 5 ciphertexts in struct order h | hat_h | hat_v | v_w | b_w (struct proof, src/snark.h:14-20).
 * Every CRS row is expanded once: S rows feed v_w and h, AS rows feed hat_v and hat_h (the reference expands each twice). */
int mfh_prove(mfh_ctx *ctx, const uint8_t *d_crs_c8, const uint32_t *d_ssp, const uint8_t *h_witness_bits, uint32_t delta,
              const uint8_t *h_smudge_mag, size_t maglen, const uint8_t *h_smudge_sign, uint64_t *d_proof);

/* verifier() (src/snark.c:192-250) for `count` proofs (5 ciphertexts each) entirely on the device: t(s), v_0(s), the 5*count
 * decryptions and the eq-pke / eq-div / eq-lin checks.  d_ok[i] = 1 iff proof i is accepted.  (The reference's final
 * "test-error" bound never rejects: SIZ of a non-positive value is <= 0, src/snark.c:238-241.) */
int mfh_verify(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t alpha, uint32_t beta, uint32_t s, const uint64_t *d_sk,
               const uint64_t *d_proofs, size_t count, uint8_t *d_ok);

/* ---- public inputs: proofs bound to a statement of lu public wires ----------------------------------------------------------------
 * The reference defines GAMMA_LU 10 (src/lwe.h:26) but fixes l_u = 0 ("Assume l_u = 0 . So v(x) = v_0(x) + w(x)", src/snark.c:160): its proofs carry no
 * statement.  Here, with 0 <= lu <= m - 1, the m - 1 input bits of a statement are split: bits [0, lu) are the statement u (public), bits [lu, m - 1) the
 * private witness.  lu is a property of the CRS: a proof made or checked with another lu than the CRS was set up with is in general rejected (accepted
 * only when the wires on which the two lu disagree are all zero).  lu = 0 gives exactly the bytes of mfh_setup_image / mfh_prove / mfh_prove_batch /
 * mfh_verify; lu >= m is MFH_EINVAL.  The row-sharded provers (mfh_prove_partial*, mfh_prove_batch_partial, mfh_batch_chain*) stay at lu = 0.
 *
 * mfh_setup_public: setup() (src/snark.c:100-108) with the messages of rows v[0..lu) zeroed -- they encrypt 0 instead of beta v_i(s), at the same stream
 * rows with the same errors; the layout is that of mfh_setup.  Required for soundness: with Enc(beta v_i(s)) of a public wire in the CRS a prover could move
 * (u - u') v_i into w and prove a false statement u'.  d_rows_image may be NULL; otherwise it receives the expanded rows as mfh_setup_image writes them. */
int mfh_setup_public(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t alpha, uint32_t beta, uint32_t s, uint32_t lu, const uint64_t *d_sk,
                     const uint64_t *d_err, uint8_t *d_crs_c8, void *d_rows_image);
/* prover() (src/snark.c:141-174) with a statement: h_bits as for mfh_prove (m - 1 bits, bits [0, lu) the statement):
 *   w_priv = delta t + sum_{i > lu, bit} v_i,  v = v_0 + sum_{i <= lu, u_i} v_i + w_priv,  b_w = delta ct_t + sum_{i > lu, bit} ct_{v_i},
 *   v_w = eval(S, w_priv), hat_v = eval(AS, v), h = (v^2 - 1) / t, hat_h, and the smudging of mfh_prove (src/snark.c:185-189).
 * Equivalently: h, hat_h, hat_v are those of mfh_prove(bits); v_w, b_w those of mfh_prove(bits with [0, lu) cleared) (same delta and smudging). */
int mfh_prove_public(mfh_ctx *ctx, const uint8_t *d_crs_c8, const uint32_t *d_ssp, uint32_t lu, const uint8_t *h_bits, uint32_t delta,
                     const uint8_t *h_smudge_mag, size_t maglen, const uint8_t *h_smudge_sign, uint64_t *d_proof);
/* mfh_prove_batch with a statement per proof (same layout, regimes and queue-only behaviour; proof b is bit-identical to mfh_prove_public of statement b).
 * The witness GEMM and the b_w launches receive the bits with the statement cleared; the statements (ceil(lu / 8) bytes each) are staged beside them and the
 * V = W + v_0 step adds the selected public rows (up to 64 public wires read once per 16 statements through L2; more by a second witness pass with delta 0). */
int mfh_prove_batch_public(mfh_ctx *ctx, const uint8_t *d_crs_c8, const uint32_t *d_ssp, uint32_t lu, uint32_t nproofs, const uint8_t *h_bits,
                           size_t bits_stride, const uint32_t *h_delta, const uint8_t *h_smudge_mag, size_t maglen, const uint8_t *h_smudge_sign,
                           uint64_t *d_proofs);
/* The verification key: d_vk = [t(s), v_0(s), v_1(s) .. v_lu(s)] mod p, lu + 2 uint32 (the Horner values of src/snark.c:201,213 and of the public wires).
 * With alpha, beta and sk it is all the verifier needs: no SSP on the device. */
int mfh_vk_derive(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t s, uint32_t lu, uint32_t *d_vk);
/* verifier() (src/snark.c:192-250) with statements: the 5 count decryptions of mfh_verify, then its four checks with
 * v_s = v_0(s) + sum_{i <= lu, u_i} u_i v_i(s) + w_s mod p (src/snark.c:213-217).  Proof i's statement: h_statements + i * stmt_stride (stmt_stride >=
 * ceil(lu / 8); bits lu and above are ignored).  d_ok[i] = 1 iff proof i is accepted. */
int mfh_verify_public(mfh_ctx *ctx, const uint32_t *d_vk, uint32_t lu, uint32_t alpha, uint32_t beta, const uint64_t *d_sk, const uint64_t *d_proofs,
                      const uint8_t *h_statements, size_t stmt_stride, size_t count, uint8_t *d_ok);

/* The CRS expanded ONCE for the matrix-core path (the resident regime of the batch prover): mfh_crs_expand_mm writes the S, AS and
 * BT+BV regions in MFMA A-fragment order (mfh_crs_mm_image_bytes bytes: 11.3 GB at the default instance); while an image is
 * registered with mfh_crs_set_resident_mm (NULL clears it), mfh_eval_rows_multi over exactly one of those regions -- hence
 * mfh_prove_batch -- streams it from HBM instead of regenerating the keystream.  Results are identical. */
size_t mfh_crs_mm_image_bytes(const mfh_ctx *ctx);
int mfh_crs_expand_mm(mfh_ctx *ctx, const uint8_t *d_crs_c8, uint8_t *d_image);
int mfh_crs_set_resident_mm(mfh_ctx *ctx, const uint8_t *d_image);
/* Which kernel writes the image (same bytes for every row tile and row that exists; tuning / A-B): 0 (default) the barrier-free writer
 * (lane = row, 16 x 16 byte transposition on the matrix cores, csrc/expandmm.hip), 1 the LDS-tile writer (k_evalmm16<MODE 1>). */
int mfh_set_expand_path(mfh_ctx *ctx, int path);
/* Periods (of 23 AES blocks) a workgroup of the barrier-free writer walks per chunk: 0 (default) picked from the region's row count, 2 .. 10 forced; anything else is
 * MFH_EINVAL.  The image's bytes do not depend on it (tests: regions small enough for a test select 2 on their own).  Holds for every expansion of the context, the
 * transient image of mfh_prove_batch included. */
int mfh_set_expand_periods(mfh_ctx *ctx, uint32_t periods);
/* prover() for nproofs statements under ONE CRS and SSP.  The S and AS regions are expanded (or streamed from the image, below) once per group of up to 31 proofs, the
 * BT+BV region once per up to 255 (the S / AS launches of the streaming regime: 255 proofs per two passes over a region), and the multiply-accumulate of the coefficient vectors runs on the matrix cores (mfh_eval_rows_multi); proof b is bit-identical to
 * mfh_prove(witness b, delta b, smudging b).  h_witness_bits: nproofs bit strings, bits_stride bytes apart; h_delta: nproofs values
 * < p; h_smudge_mag: nproofs x 5 x maglen bytes; h_smudge_sign: nproofs x 5 bytes; d_proofs: nproofs x 5 ciphertexts.
 * The single-proof resident image (mfh_crs_set_resident) must not be set; the matrix-core image (mfh_crs_set_resident_mm) may.
 * With more than 31 proofs and no image registered, the call first expands the CRS into a transient image of
 * mfh_crs_mm_image_bytes bytes (scratch kept by the context; expanded again by every call) and streams it for every group instead of
 * running AES once per group; if that scratch cannot be allocated, or after mfh_set_batch_image(ctx, 0) (which also frees it), every
 * group regenerates the keystream.  Same proofs either way.  The call only QUEUES its work (about 2.5 ms of host time per 1020 statements at the default instance, for calls of up to 8
 * super-groups = 2040 statements: the witness pass stages through a ring of 8 pinned buffers, and a longer call waits for the copy of super-group k - 8 before it stages k): it returns
 * long before the proofs exist -- mfh_sync, or mfh_prove_batch_stream_wait below, before d_proofs is read. */
int mfh_set_batch_image(mfh_ctx *ctx, int enabled);
/* Row slabs of mfh_prove_batch.  A call whose matrix-core image does not fit the GPU's memory (363 GB at 2^20 constraints) cuts the CRS
 * rows into slabs -- the row shares of the multi-GPU prover, one after the other on one GPU --, expands a slab's image once and streams it
 * for every group of the call, accumulating mod 2^(64K): the keystream is generated once per call instead of once per group of 31 proofs.
 * 0 (default): slabs only when needed, their number from the free memory; n: always n slabs (tests, tuning).  Same proofs. */
int mfh_set_batch_slabs(mfh_ctx *ctx, uint32_t nslabs);
/* tuning knobs (results do not depend on them; MFH_EINVAL outside the range): column chunks per row of the matrix-core encryption kernel
 * (0 = picked from the batch size, at most 64); statements per witness GEMM pass of the batch chain (0 = one pass per super-group of up to 255, else 32..256). */
int mfh_set_encrypt_chunks(mfh_ctx *ctx, uint32_t chunks);
/* mfh_eval_rows / mfh_prove*: 0 (default) = tile kernel (k_eval: two 512-coordinate row tiles per workgroup), 1 = at logq = 736 the wave-autonomous
 * kernel (k_eval_w: a wave owns 64 coordinates and a private keystream tile, no workgroup barriers; measured 4 % slower).  Same results (A/B, tests). */
int mfh_set_eval_path(mfh_ctx *ctx, int path);
int mfh_set_witness_per(mfh_ctx *ctx, uint32_t statements);
/* launch shape of the streaming regime of mfh_prove_batch* (tuning; results do not depend on it): groups of 31 proofs served by one pass
 * over a region's image (1..8, default 4), and whether the S and AS groups of a round share ONE launch (default) or run as two
 * launches on two streams. */
int mfh_set_batch_launch(mfh_ctx *ctx, uint32_t groups_per_launch, int merge_regions);
/* b_w (src/snark.c:143-155) of all super-groups of a streaming mfh_prove_batch call in ONE launch per up to 8 super-groups over the BT+BV image (default), or one
 * launch per super-group (0; rounds 1 - 3).  Tuning; results do not depend on it. */
int mfh_set_batch_bw(mfh_ctx *ctx, int merged);
/* The witness pass of a streaming mfh_prove_batch call (single GPU, dense SSP, d % 64 == 0, no public inputs, no row slabs, 2 .. 8 super-groups with b_w merged) as ONE
 * streaming launch over an image of the SSP in the CRS image's fragment order (mfh_witness_poly_stream below), sharing b_w's digit fragments (default), or
 * k_witness_mm8q once per super-group (0; every other caller's pass).  The image is a per-SSP constant the size of the SSP, built on first use and rebuilt after
 * mfh_ssp_upload / mfh_ssp_prepare; without room for it the call keeps the per-super-group pass.  Tuning; results do not depend on it. */
int mfh_set_batch_witness(mfh_ctx *ctx, int streamed);
/* how a streaming launch with several groups is laid out on the chip (tuning; results do not depend on it).  map: 0 = a tile group's workgroups for all
 * groups of both regions are neighbours, 1 = the 32 workgroups an XCD runs at a time are 32 / g tile groups x the g groups of ONE region (a group's digit
 * fragments are then shared by twice as many workgroups of the XCD).  persistent: 1 = one workgroup per CU looping over its XCD's items instead of one workgroup
 * per item (default), 2 = the same grid with the one-wave-per-SIMD body (k_mmstream_w: 256 accumulators per wave in AccVGPRs, half the LDS reads; measured the same time); sync_mode (persistent only): 0 = none, 1 = the workgroups that stream the same fragments begin every item together, 2 = all workgroups of an XCD
 * do -- a speed-only rendezvous bounded by spin_max polls (a workgroup never waits longer, so the grid drains whatever is resident). */
int mfh_set_mm_stream(mfh_ctx *ctx, int map, int persistent, int sync_mode, uint32_t spin_max);
/* Width of the persistent S / AS launch: workgroups per XCD (1..32; 32 = one per CU, the default).  Fewer leave CUs of every XCD free; with early_chain != 0
 * mfh_prove_batch then queues the chain of super-group k + 1 and the epilogue of super-group k on side streams beside the streaming launches instead of between them
 * (the round-5 experiment on the power finding, EXPERIMENTS.md).  Tuning; results do not depend on it. */
int mfh_set_mm_width(mfh_ctx *ctx, uint32_t per_xcd, int early_chain);
/* How the workgroups of the persistent grid come by their items (tuning; results do not depend on it).  mode 0: every workgroup walks its fixed list, so a launch
 * ends when the slowest CU has finished its list.  mode 1 (default): every XCD has a queue over its items in the static walk's order; a workgroup claims from its own XCD's queue
 * (one atomic add per item) and, when that is exhausted, from the queues of the XCDs x + 1, x + 2, ... (mod 8), and returns after eight exhausted queues -- it never waits
 * for another workgroup.  prefix: rounds of the static list every workgroup runs before it claims (the claim's latency is then paid for the last items only); >= 0 that
 * many (at most the whole list), < 0 all but the last -prefix rounds (default -8).  start_shift (0..7, tests): workgroups of XCD x begin in the queue of XCD
 * (x + start_shift) mod 8 and run no static prefix, so whatever a workgroup takes before its first queue is exhausted is a foreign XCD's item (its own XCD's queue
 * is its (8 - start_shift)-th).  Every launch has counters of its own: the two launches mfh_prove_batch keeps in flight together (mfh_set_batch_launch, merge_regions 0)
 * do not share any.  The rendezvous modes of mfh_set_mm_stream and the one-wave body keep
 * the static walk. */
int mfh_set_mm_queue(mfh_ctx *ctx, int mode, uint32_t start_shift, int prefix);
/* Tests: a device array of `words` zeroed 32-bit words in which the persistent launches of the following calls record who ran which item (NULL: none, the default).
 * Launch l of the calls since this one takes the next 2 x nchunks x 8 x 32 nblk words: per (chunk, XCD, slot) how often the item was taken, and
 * blockIdx.x + 1 | from << 16 of the workgroup that took it (from: 0xff = its static list, else the ordinal 0..7 of the queue it claimed from).
 * mfh_mm_claim_log_launches copies 12 words per launch -- first word of its section, nchunks, nblk, groups, groups per region, map, tile groups, workgroups per XCD,
 * coefficient bytes, queue mode, static prefix, start shift -- for up to max_launches launches and returns how many there were (16 at most per log). */
int mfh_set_mm_claim_log(mfh_ctx *ctx, uint32_t *d_log, size_t words);
uint32_t mfh_mm_claim_log_launches(const mfh_ctx *ctx, uint32_t *desc, uint32_t max_launches);
/* rows per row chunk of the matrix-core launches (mfh_eval_rows_multi, mfh_prove_batch): the int32 accumulators hold at most
 * 131071 rows (the default; 0 restores it); smaller values split every region into more chunks -- same results (tuning, tests). */
int mfh_set_mm_chunk_rows(mfh_ctx *ctx, uint32_t rows);
/* How the streaming kernels (k_mmstream*) hand the partial products sum_i A'[i][m] C'[i][n] to the epilogue: on (default) recombined in the kernel -- the four byte
 * positions a lane holds and, for four-byte coefficient vectors, the vector's four digit columns: a 16-byte record per (byte-position quad, vector) instead of sixteen
 * int32, a quarter of the bytes written and read back (2.1 GB per super-group launch otherwise) --; off: the int32 layout of rounds 1 - 5.  Exact integer arithmetic either
 * way: same results (tuning, tests). */
int mfh_set_mm_pack(mfh_ctx *ctx, int on);
int mfh_prove_batch(mfh_ctx *ctx, const uint8_t *d_crs_c8, const uint32_t *d_ssp, uint32_t nproofs, const uint8_t *h_witness_bits,
                    size_t bits_stride, const uint32_t *h_delta, const uint8_t *h_smudge_mag, size_t maglen, const uint8_t *h_smudge_sign,
                    uint64_t *d_proofs);
/* Draining a call while it runs.  mfh_prove_batch queues its work super-group by super-group (mfh_prove_batch_supergroup() statements each: 255 when the
 * call streams an image, 248 when every group regenerates the keystream; 0 before the first call) and statement k's five ciphertexts are final in d_proofs
 * once super-group k / size has been smudged.  mfh_prove_batch_stream_wait makes `hip_stream` (a stream of the caller's, not the context's) wait until statements
 * [0, upto) of the LAST mfh_prove_batch call are final: a device-to-host copy queued on it afterwards runs under the following super-groups' kernels (the host shim's
 * mfuoco_prover_batch converts super-group k to mpz_t while the GPU works on k + 1).  Row-slab calls complete all statements together. */
uint32_t mfh_prove_batch_supergroup(const mfh_ctx *ctx);
int mfh_prove_batch_stream_wait(mfh_ctx *ctx, uint32_t upto, void *hip_stream);
/* ---- multi-GPU: row-sharded BATCH prover (BASELINE configs 3/4: "ciphertexts sharded across 8 x MI355X + RCCL reduce") ------
 * The loops that shard are src/snark.c:147-155 (b_w over the BT+BV rows) and :157-174 (the four eval_poly passes over the S / AS rows):
 * rank r of `world` owns rows [R r / world, R (r+1) / world) of each region (R = d, d, m) and, for the steps that do not touch the CRS,
 * a contiguous slice of the STATEMENTS.  One step over nstmt statements:
 *   1. mfh_batch_chain on the rank's own statements: w = delta t + sum_bits v_i, v = w + v_0, h = (v^2 - 1) / t   (src/snark.c:141-169)
 *   2. exchange (all-to-all): rank r receives rows [d r / world, ...) of w | h | v of ALL statements
 *   3. mfh_prove_batch_partial: the rank's row shares of all five ciphertexts of all statements (no delta ct_t term, un-smudged),
 *      streamed from the rank's share of the matrix-core image (mfh_crs_expand_mm_share: 45 GB per GPU for the 2^20-constraint CRS on 8)
 *   4. mfh_ct_to_lanes -> ONE reduce-scatter (sum) of uint64 lanes per step: every rank receives the summed lanes of its own statements
 *   5. mfh_ct_from_lanes (carries + modq) -> mfh_prove_batch_finish: + delta ct_t on b_w, smudging.
 * Proofs are bit-identical to mfh_prove_batch's (sums mod 2^(64K) do not depend on the order).  world = 1 degenerates to mfh_prove_batch.
 * c-lwe-snarks_amd/dist.py (prove_batch_sharded) drives the sequence over torch.distributed (backend nccl = RCCL); for a generator-defined
 * SSP it runs step 1 in two halves (mfh_batch_witness_cols / mfh_batch_chain_from_w below, one more all-to-all). */
size_t mfh_crs_mm_share_bytes(const mfh_ctx *ctx, uint32_t rank, uint32_t world);
int mfh_crs_expand_mm_share(mfh_ctx *ctx, const uint8_t *d_crs_c8, uint32_t rank, uint32_t world, uint8_t *d_image);
int mfh_crs_set_resident_mm_share(mfh_ctx *ctx, const uint8_t *d_image, uint32_t rank, uint32_t world);
/* step 1: d_w, d_h, d_v = nstmt x d coefficients each (statement-major) */
int mfh_batch_chain(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_witness_bits, size_t bits_stride, const uint32_t *h_delta,
                    uint32_t *d_w, uint32_t *d_h, uint32_t *d_v);
/* step 1 in two halves, for SSPs whose witness pass dominates the chain (generator-defined: 2^20 constraints): (1a) every rank computes
 * the coefficients [col0, col0 + ncols) of w of ALL nstmt statements -- 1 / world of the generation (or read) of the selected rows, no
 * reduction -- into d_w[b * w_stride + (k - col0)] (col0, ncols multiples of 128, else MFH_EUNSUPPORTED: use mfh_batch_chain);
 * the slices are exchanged (all-to-all by statement owner); (1b) the owner finishes the chain of its statements from their whole w:
 * d_v = d_w + v_0, d_h = (d_v^2 - 1) / t. */
int mfh_batch_witness_cols(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_witness_bits, size_t bits_stride, const uint32_t *h_delta,
                           uint32_t col0, uint32_t ncols, uint32_t *d_w, size_t w_stride);
int mfh_batch_chain_from_w(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint32_t *d_w, uint32_t *d_h, uint32_t *d_v);
/* step 3: statement b's coefficients for the rank's S / AS rows [d rank / world, d (rank+1) / world) at d_w / d_h / d_v + b * coef_stride
 * (uint32 words; with the whole polynomials in memory: d_w = W + d rank / world, coef_stride = d).  The witness bits select the rank's
 * share of the BT+BV rows.  d_partial = nstmt x 5 partial ciphertexts (struct proof order).  With more than 31 statements and no image
 * registered the call expands the rank's shares into a transient image first (see mfh_prove_batch). */
int mfh_prove_batch_partial(mfh_ctx *ctx, const uint8_t *d_crs_c8, uint32_t rank, uint32_t world, uint32_t nstmt, const uint8_t *h_witness_bits,
                            size_t bits_stride, const uint32_t *d_w, const uint32_t *d_h, const uint32_t *d_v, size_t coef_stride, uint64_t *d_partial);
/* step 5: d_proofs = nstmt summed proofs (after mfh_ct_from_lanes): b_w += delta_b ct_t (src/snark.c:143-145), then the five smudging
 * draws per proof in the order of mfh_prove (src/snark.c:185-189).  Queue-only: the host's contribution (deltas, smudging terms, signs) is staged once in pinned memory and
 * the call returns without waiting for the GPU to reach it (a pipelined caller queues it behind work that has not run yet: host/mfuoco_dist.c). */
int mfh_prove_batch_finish(mfh_ctx *ctx, const uint8_t *d_crs_c8, uint32_t nstmt, const uint32_t *h_delta, const uint8_t *h_smudge_mag, size_t maglen,
                           const uint8_t *h_smudge_sign, uint64_t *d_proofs);

/* ---- multi-GPU: row-sharded prover -------------------------------------------------------------
 * Every proof element is sum_i coeff_i * row_i and the public stream is seekable, so the CRS rows of each region are
 * split into `world` contiguous shares.  mfh_prove_partial computes rank `rank`'s share of the five (un-smudged)
 * ciphertexts; the shares are summed with ONE all-reduce of uint64 lanes (mfh_ct_to_lanes -> RCCL sum ->
 * mfh_ct_from_lanes propagates the carries and applies modq), then mfh_prove_finish smudges.  world = 1 is mfh_prove. */
int mfh_prove_partial(mfh_ctx *ctx, const uint8_t *d_crs_c8, const uint32_t *d_ssp, const uint8_t *h_witness_bits, uint32_t delta,
                      uint32_t rank, uint32_t world, uint64_t *d_partial);
int mfh_prove_finish(mfh_ctx *ctx, uint64_t *d_proof, const uint8_t *h_smudge_mag, size_t maglen, const uint8_t *h_smudge_sign);
/* mfh_witness_poly for nstmt <= 12 statements in ONE pass over the SSP: every selected v_i is read (d_ssp == NULL: generated) once and
 * added into the polynomials of the statements whose bit selects it.  h_bits: nstmt bit strings bits_stride bytes apart; d_w: nstmt x d coefficients. */
int mfh_witness_poly_multi(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                           uint32_t *d_w);
/* The same for nstmt <= 256 statements (dense and generator-defined SSP alike) in ONE read of the SSP, as a GEMM on the matrix cores (bits x SSP bytes, exact); d a multiple
 * of 128 (d_ssp == NULL, the generator-defined SSP: the SSP bytes are generated in the kernel).  Keeps a second image of the SSP in MFMA fragment order (same size), built on first use and rebuilt after
 * mfh_ssp_upload / mfh_ssp_prepare.  Used by mfh_prove_batch. */
int mfh_witness_poly_mm(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                        uint32_t *d_w);
/* The same restricted to the coefficients [col0, col0 + ncols) of the polynomials: d_w[b * w_stride + (k - col0)] (col0 and ncols
 * multiples of 128, else MFH_EUNSUPPORTED).  The cost is the range's share of the read / generation of the selected rows. */
int mfh_witness_poly_mm_cols(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                             uint32_t col0, uint32_t ncols, uint32_t *d_w, size_t w_stride);
/* mfh_witness_poly_mm for ANY number of statements of a dense SSP with d a multiple of 64, as the batch prover's streaming GEMM (SSP bytes x witness-bit digit columns, exact):
 * groups of 255 statements, up to 8 groups per launch over a third image of the SSP, in the CRS image's A-fragment order (same size, built on first use and rebuilt
 * after mfh_ssp_upload / mfh_ssp_prepare).  MFH_EUNSUPPORTED for other SSPs or with mfh_set_mm_pack(ctx, 0); MFH_ENOMEM without room for the image. */
int mfh_witness_poly_stream(mfh_ctx *ctx, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                            uint32_t *d_w);
/* Optional second exchange that also shards the witness polynomial (the SSP pass, 1.4 GB per proof at the default size):
 * mfh_witness_lanes = this rank's share of sum_{bit} v_i as d uint64 lanes (each < p) -> all-reduce (sum) ->
 * mfh_prove_partial_w takes the summed lanes instead of recomputing w on every rank.  mfh_witness_from_lanes: w = delta t + lanes mod p. */
int mfh_witness_lanes(mfh_ctx *ctx, const uint32_t *d_ssp, const uint8_t *h_witness_bits, uint32_t rank, uint32_t world, uint64_t *d_lanes);
int mfh_witness_from_lanes(mfh_ctx *ctx, const uint32_t *d_ssp, const uint64_t *d_lanes, uint32_t delta, uint32_t *d_w);
int mfh_prove_partial_w(mfh_ctx *ctx, const uint8_t *d_crs_c8, const uint32_t *d_ssp, const uint8_t *h_witness_bits, uint32_t delta,
                        uint32_t rank, uint32_t world, const uint64_t *d_wlanes, uint64_t *d_partial);
/* count ciphertexts <-> count * (n+1) * mfh_lanes_per_value uint64 lanes: lane j of a value = its bits [56 j, 56 j + 56) (13 lanes per 704-bit value, 27 at
 * logq 1472): sums of up to 256 ranks' lanes fit 64 bits; mfh_ct_from_lanes propagates the carries and applies modq (src/lwe.h:107-118). */
uint32_t mfh_lanes_per_value(const mfh_ctx *ctx);
int mfh_ct_to_lanes(mfh_ctx *ctx, const uint64_t *d_cts, size_t count, uint64_t *d_lanes);
int mfh_ct_from_lanes(mfh_ctx *ctx, const uint64_t *d_lanes, size_t count, uint64_t *d_cts);

/* ---- library info -------------------------------------------------------------------------------- */
const char *mfh_version(void);
/* 128-bit digest of nbytes at d_buf (4-byte aligned), copied to the host: a cache key for "has this device buffer changed" (the host shim keeps the expanded
 * CRS image across prover calls while the compressed CRS it was made from is unchanged), not a cryptographic hash.  Synchronises the context's stream. */
int mfh_digest128(mfh_ctx *ctx, const void *d_buf, size_t nbytes, uint64_t h_digest[2]);
/* size in bytes the context's scratch currently occupies on the device */
size_t mfh_workspace_bytes(const mfh_ctx *ctx);
/* eval_poly (src/lwe.c:160-178) for MANY coefficient vectors over the same nrows CRS rows -- the S / AS / BV regions of a batch of
 * proofs under one CRS: the rows are expanded once and the multiply-accumulate runs on the matrix cores (i8 MFMA over 8-bit
 * keystream bytes x coefficient bytes; exact integer arithmetic, same result as nvec calls of mfh_eval_rows).
 * d_coeffs = nvec vectors of nrows uint32, vector-major; coeff_bytes = 4: any uint32 value, nvec <= 63; coeff_bytes = 1: the caller
 * guarantees every coefficient < 256 (only the low byte is used), nvec <= 255.  More than 128 digit columns (nvec * coeff_bytes + 1)
 * select the 256-column kernel, which needs off and the row length n * CT_BYTES to be multiples of 8 (true for every CRS region).  d_rops = nvec ciphertexts, vector-major.
 * At logq = 1472 every call uses the 256-column kernel. */
int mfh_eval_rows_multi(mfh_ctx *ctx, uint64_t off, size_t nrows, const uint8_t *d_c8, const uint32_t *d_coeffs, uint32_t nvec,
                        uint32_t coeff_bytes, uint64_t *d_rops, int accumulate);

/* Kernel timing for the roofline leg of bench.py.  With timing enabled every launch of a hot kernel is bracketed by
 * HIP events on the context's stream (no synchronisation is added).  mfh_timing_drain waits for the stream, then
 * reports and forgets the launches of kind `which`: "eval2" / "eval1" (k_eval with 2 / 1 coefficient vectors),
 * "eval" (both), "encrypt", "keystream", "expand", "mac2" / "mac1" (resident MAC), "evalmm" / "evalmm_resident" (mfh_eval_rows_multi from the seed / from the image), "mmstream_rounds" (those of "evalmm_resident" that serve several groups of a batch: the S / AS rounds of mfh_prove_batch; drain it first), "mmstream_bw" (b_w of several super-groups in one launch), "mmstream_rounds_persistent" / "mmstream_bw_persistent" (those of the two that ran the persistent one-workgroup-per-CU grid; drain them before their supersets), "expandmm" (mfh_crs_expand_mm, one launch per region), "ssp_interp" (the gather launches of mfh_ssp_from_rows; total_rows = nonzeros), "circuit_assign" (k_circuit_eval of mfh_circuit_assign; total_rows = statements), "circuit_assign_global" (k_circuit_eval_global of mfh_circuit_assign on a mfh_circuit_create_global program; total_rows = statements), "circuit_assign_ex" / "circuit_assign_global_ex" (k_circuit_eval_ex / k_circuit_eval_global_ex: mfh_circuit_create_ex programs of either kind; total_rows = statements), "circuit_assign_out" / "circuit_assign_global_out" (the same for mfh_circuit_create_out programs with outputs), "circuit_assign_sum" / "circuit_assign_global_sum" (k_circuit_eval<true, OUT, true> / k_circuit_eval_global<true, OUT, true>: mfh_circuit_create_sum programs with a WSUM gate, with or without outputs), "ssp_rows_violations" (k_rows_violations of mfh_ssp_rows_violations; total_rows = rows x statements), "merkle_level" / "merkle_paths" (k_merkle_level / k_merkle_paths of the Merkle tree calls; total_rows = parents computed / statements).  "sha256_records" (k_sha256_records of mfh_sha256_records and mfh_merkle_set_records; total_rows = records).  total_rows = rows handed to those launches (AES blocks for "keystream"). */
int mfh_set_timing(mfh_ctx *ctx, int enabled);
/* prover scheduling: mfh_prove* run the witness pass + polynomial step on an internal stream beside the evaluation of
 * b_w's rows and join before the S / AS regions; results are identical in every mode.  0 = one stream, 1 (default) = two
 * streams, queueing order picked from the size of b_w's share, 2 = b_w's rows queued first, 3 = the chain queued first. */
int mfh_set_overlap(mfh_ctx *ctx, int mode);
int mfh_timing_drain(mfh_ctx *ctx, const char *which, uint64_t *count, double *total_ms, uint64_t *total_rows, float *last_ms);
float mfh_last_kernel_ms(mfh_ctx *ctx, const char *which); /* = last_ms of mfh_timing_drain; < 0 if none */
/* Union of the [start, end) spans of the launches the last mfh_timing_drain matched, in ms: equals total_ms when the launches
 * ran one after the other, less when launches of two streams overlapped (mfh_prove_batch). */
double mfh_timing_busy_ms(const mfh_ctx *ctx);
/* rows x evaluations served by the launches the last mfh_timing_drain matched: a streaming launch of mfh_prove_batch serves 4 groups of
 * coefficient vectors from one pass over its rows (= total_rows for every other kind) */
uint64_t mfh_timing_work_rows(const mfh_ctx *ctx);

#ifdef __cplusplus
}
#endif
