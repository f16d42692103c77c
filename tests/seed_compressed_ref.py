"""Reference for the seed-compressed ciphertext calls (mfh_encrypt_rows, mfh_decrypt_rows) and for the launch plan of k_encrypt_mm, for the tests.

regev_decrypt (src/lwe.c:105-111) of a seed-compressed ciphertext, in Python integers: row i of a region at stream offset `off` has its a part
at off + i * CTR_CT, and b is the CT_BYTES of ct_export taken whole (ct_import, src/lwe.c:122-126, does not reduce it):

    dot = sum_j sk_j a_j  mod 2^(64 K)          m = (b - dot) mod p

A second statement of what oracle.decrypt(oracle.ct_import(...)) computes in C limbs; tests/test_seed_compressed_ref_cpu.py holds the two
against each other before either judges a kernel.

enc_plan() restates the column-chunk arithmetic of csrc/encmm.hip (enc_plan) so that a test can say which plan a forced chunk count
selects and how much workspace that plan reserves.
"""
import numpy as np

import oracle_lib as ol

P = ol.P


def key_ints(sk) -> list:
    return [ol.limbs_to_int(v) for v in sk]


def row_dots(oracle, p, seed, off, nrows, sk_ints) -> list:
    """<sk, a_i> mod 2^(64 K) for rows i < nrows of the region at stream offset off"""
    mod, vb = 1 << (64 * p.K), 8 * p.L
    out = []
    for i in range(nrows):
        raw = oracle.sample_rows(p, seed, off + i * p.ctr_ct, 1)[0].tobytes()  # n values of L little-endian limbs
        out.append(sum(s * int.from_bytes(raw[vb * j: vb * j + vb], "little") for j, s in enumerate(sk_ints)) % mod)
    return out


def decrypt_b(b: bytes, dot: int) -> int:
    return (int.from_bytes(b, "little") - dot) % P


def extreme_key(rng, p):
    """random key values with the extreme balanced digits among them: all-ones (every digit carries), zero, 0x80.. (the most negative digit) and 0x7f.."""
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    sk[0] = ol.int_to_limbs((1 << p.logq) - 1, p.L)
    sk[1] = 0
    sk[2] = ol.int_to_limbs(int.from_bytes(b"\x80" * p.ctb, "little"), p.L)
    sk[3] = ol.int_to_limbs(int.from_bytes(b"\x7f" * p.ctb, "little"), p.L)
    return sk


# ---- the launch plan of k_encrypt_mm (csrc/encmm.hip: EG<>, enc_plan, key_operands) ---------------------------------------------------------
_SBY = {736: 88, 1472: 184}   # result byte positions
_NQ = {736: 6, 1472: 12}      # 16-column tiles
_SLOTS = {736: 512, 1472: 256}  # workgroup slots: 256 CUs x 2 workgroups at logq 736, x 1 at 1472


def enc_plan(p, nrows: int, forced: int = 0, honour_kc_min: bool = True):
    """(ksteps, kc, kpc): k-steps of a row, column chunks, k-steps per chunk.  honour_kc_min = False is the plan a library would run that dropped the
    int32 floor under a forced chunk count: what the plan assertions must be able to tell apart."""
    rowlen = p.n * p.ctb
    ksteps = (rowlen + 8 + 63) // 64
    nblk = 2 * ((nrows + 511) // 512)
    kc_min = 1
    if p.n * _SBY[p.logq] > 131071:
        kc_min = (ksteps * 64 + 131070) // 131071
    slots = _SLOTS[p.logq]
    k_lo = max(kc_min, (4 * slots + nblk - 1) // nblk)
    k_hi = max(k_lo, min(3 * k_lo, max(1, ksteps // 32)))
    kc, best = min(k_lo, k_hi), 0.0
    for k in range(kc, k_hi + 1):
        wg = nblk * k
        rounds = (wg + slots - 1) // slots
        eff = wg / (slots * rounds)
        if eff > best + 1e-9:
            best, kc = eff, k
    kc = max(kc_min, kc)
    if forced:
        kc = max(kc_min, forced) if honour_kc_min else forced
    kpc = (ksteps + kc - 1) // kc
    kc = (ksteps + kpc - 1) // kpc
    return ksteps, kc, kpc


def enc_workspace_bytes(p, nrows: int, kc: int) -> int:
    """bytes k_encrypt_mm's host side reserves for one call: key digits | prefix and column sums | Toeplitz fragments for both heads | partial products;
    the workspace grows to this rounded up to 1 MiB (and never shrinks)"""
    ksteps = (p.n * p.ctb + 8 + 63) // 64
    sb_b = (p.n * _SBY[p.logq] + 255) & ~255
    total = sb_b + 2 * 256 * 8 + 2 * ksteps * _NQ[p.logq] * 1024 + nrows * kc * 16 * _NQ[p.logq] * 4
    return (total + (1 << 20) - 1) & ~((1 << 20) - 1)


def refreshes(kpc: int) -> int:
    """how often a full chunk of kpc k-steps runs the counter-span refresh (every 64 k-steps, not at the chunk's first)"""
    return (kpc - 1) // 64
