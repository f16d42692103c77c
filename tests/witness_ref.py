"""The witness pass and the SSP generator, restated for the tests with numpy and Python integers only: no GPU, no project code.

    w_b[k] = delta_b t[k] + sum_{i = 1 .. m - 1} bit_b[i - 1] v_i[k]  mod p,    t = slot 0, v_i = slot i + 1, p = 2^32 - 5

(csrc/witness.hip) and the counter-based generator that defines the SSP of BASELINE configs 4/5 (csrc/ssp_prg.hpp): row key, raw hash, coefficient,
the inverse of its mixing function and seeds crafted so that a chosen (slot, k) hashes to a chosen raw value -- the five raw values in [p, 2^32) that
a coefficient must not show are otherwise never met (5 of 2^32 inputs).  tests/test_witness_ref_cpu.py holds this file against the compiled header,
recorded numbers and the oracle; tests/test_gpu_witness_exact.py holds every form of the witness pass against it."""
import numpy as np

P = 0xFFFFFFFB
M32 = 0xFFFFFFFF
RAW_AT_OR_ABOVE_P = (P, P + 1, P + 2, P + 3, P + 4)

# ---- csrc/ssp_prg.hpp ----------------------------------------------------------------------------------------------------------------------
SSP_PRG_K0 = 0x632BE5AB
ROWKEY_GOLD, ROWKEY_MUL = 0x9E3779B1, 0x2C1B3C6D
MIX_MUL1, MIX_MUL2 = 0x7FEB352D, 0x846CA68B


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _rowkey_pre(seed, slot):
    """ssp_prg_rowkey before its XOR with the seed's high word (and before the `| 1`)"""
    m = np.uint64(M32)
    r = (np.uint64(seed & M32) + (_u64(slot) & m) * np.uint64(ROWKEY_GOLD)) & m
    r ^= r >> np.uint64(15)
    return (r * np.uint64(ROWKEY_MUL)) & m


def prg_rowkey(seed, slot):
    """ssp_prg_rowkey(seed, slot) for a 64-bit seed and a slot or an array of slots -> uint32"""
    r = _rowkey_pre(seed, slot) ^ np.uint64((seed >> 32) & M32)
    return (r | np.uint64(1)).astype(np.uint32)


def prg_mix(x):
    m = np.uint64(M32)
    x = _u64(x) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(MIX_MUL1)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(MIX_MUL2)) & m
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def prg_unmix(x):
    """the inverse of prg_mix: every step of the mix is an xor-shift or a multiply by an odd constant, so it is a bijection on 32 bits"""
    m = np.uint64(M32)
    x = _u64(x) & m
    x = x ^ (x >> np.uint64(16))                       # y = x ^ x >> 16 is its own inverse (shift >= half the width)
    x = (x * np.uint64(pow(MIX_MUL2, -1, 1 << 32))) & m
    x = x ^ (x >> np.uint64(15)) ^ (x >> np.uint64(30))  # y = x ^ x >> 15  =>  x = y ^ y >> 15 ^ y >> 30
    x = (x * np.uint64(pow(MIX_MUL1, -1, 1 << 32))) & m
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def prg_raw(rowkey, k):
    """ssp_prg_raw(rowkey, k): the un-reduced hash, for arrays of row keys and / or k (broadcast) -> uint32"""
    m = np.uint64(M32)
    return prg_mix((((_u64(k) & m) + np.uint64(SSP_PRG_K0)) & m) * _u64(rowkey) & m)


def prg_coeff(rowkey, k):
    """ssp_prg_coeff(rowkey, k) = raw mod p -> uint32 in [0, p)"""
    x = prg_raw(rowkey, k).astype(np.uint64)
    return (x - np.uint64(P) * (x >= np.uint64(P)).astype(np.uint64)).astype(np.uint32)  # x >= p ? x - p : x


def prg_image(seed, first_slot, nslots, d):
    """slots [first_slot, first_slot + nslots) of the generator-defined SSP as uint32 [nslots, d] (what mfh_ssp_prg_fill writes)"""
    slots = np.arange(first_slot, first_slot + nslots, dtype=np.uint64)
    return prg_coeff(prg_rowkey(seed, slots)[:, None], np.arange(d, dtype=np.uint64)[None, :])


def prg_craft_seed(slot, k, raw, lo32):
    """a 64-bit seed whose low word is lo32 with prg_raw(prg_rowkey(seed, slot), k) == raw.

    y = unmix(raw) has to equal (k + K0) * rowkey mod 2^32 for an odd rowkey, so y and k + K0 must hold the same power 2^a of two; then
    rowkey = (y >> a) * ((k + K0) >> a)^-1 mod 2^(32 - a) (odd; its top a bits are free and left 0).  The seed's high word is that row key XOR the value
    ssp_prg_rowkey has for (lo32, slot) before it XORs the high word in.  a = 0 (k even: K0 is odd) reaches the raw values p, p + 2 and p + 3,
    a = 1 (k = 3 mod 4) reaches p + 1, a = 2 (k = 1 mod 8) reaches 2^32 - 1.  ValueError where the powers of two differ."""
    y = int(prg_unmix(raw))
    kk = (k + SSP_PRG_K0) & M32
    a = (y & -y).bit_length() - 1 if y else 32
    b = (kk & -kk).bit_length() - 1 if kk else 32
    if a != b or a >= 31:
        raise ValueError(f"raw {raw:#x} (preimage {y:#x}) is not reachable at k = {k}: 2-adic orders {a} and {b}")
    mod = 1 << (32 - a)
    rowkey = (y >> a) * pow(kk >> a, -1, mod) % mod
    assert rowkey & 1
    hi = rowkey ^ int(_rowkey_pre(lo32, slot))
    seed = (hi << 32) | (lo32 & M32)
    assert int(prg_raw(prg_rowkey(seed, slot), k)) == raw
    return seed


CRAFT_LO32 = 0x89ABCDEF
CRAFT_K = {P: 70, P + 1: 71, P + 2: 70, P + 3: 70, P + 4: 73}  # a k < 128 with the 2-adic order of each raw value's preimage


def crafted_seeds(slot):
    """[(seed, slot, k, raw)] for all five raw values in [p, 2^32): the generator's coefficient at (slot, k) under that seed is raw - p"""
    return [(prg_craft_seed(slot, CRAFT_K[raw], raw, CRAFT_LO32), slot, CRAFT_K[raw], raw) for raw in RAW_AT_OR_ABOVE_P]


# ---- the witness pass ----------------------------------------------------------------------------------------------------------------------
def bit_matrix(bits_list, m):
    """[nstmt, m - 1] of 0 / 1: column i - 1 = whether the statement selects v_i (bit (i - 1) & 7 of byte (i - 1) >> 3); bits at and above m - 1 ignored"""
    nbytes = (m - 1 + 7) // 8
    rows = [np.unpackbits(np.frombuffer(bytes(b[:nbytes]).ljust(nbytes, b"\0"), dtype=np.uint8), bitorder="little")[: m - 1] for b in bits_list]
    return np.stack(rows) if rows else np.zeros((0, m - 1), dtype=np.uint8)


def w_polys(ssp_u32, bits_list, deltas, m, col_block=4096):
    """uint64 [nstmt, d]: w_b[k] = delta_b t[k] + sum_{i=1..m-1} bit_b[i-1] v_i[k] mod p, exactly.

    ssp_u32: [(m + 3), d] coefficients in [0, 2^32) (slots beyond m are not looked at).  The rows are split into 16-bit halves, each half is multiplied
    by the 0 / 1 bit matrix in float64 (BLAS) and the two products are recombined in integers.  Every product entry -- and every partial sum BLAS
    forms on the way -- is a sum of at most m - 1 integers below 2^16, so it is an integer < 2^16 (m - 1); float64 holds integers up to 2^53 exactly,
    hence the assertion m - 1 < 2^37 (the sizes used here stay below 2^16 (m - 1) <= 2^48)."""
    assert 2 <= m and m - 1 < (1 << 37)
    ssp = np.asarray(ssp_u32)
    assert ssp.ndim == 2 and ssp.shape[0] >= m + 1 and ssp.dtype in (np.uint32, np.uint64)
    d = ssp.shape[1]
    nstmt = len(bits_list)
    assert len(deltas) == nstmt
    a = bit_matrix(bits_list, m).astype(np.float64)
    delta = np.array([int(x) for x in deltas], dtype=np.uint64)[:, None]
    assert (delta < np.uint64(P)).all()
    out = np.empty((nstmt, d), dtype=np.uint64)
    p64 = np.uint64(P)
    for c0 in range(0, d, col_block):
        rows = ssp[2: m + 1, c0: c0 + col_block].astype(np.uint64)  # v_1 .. v_{m-1}
        assert (rows <= np.uint64(M32)).all()
        lo = a @ (rows & np.uint64(0xFFFF)).astype(np.float64)
        hi = a @ (rows >> np.uint64(16)).astype(np.float64)
        s = ((hi.astype(np.uint64) % p64) * np.uint64(65536) + lo.astype(np.uint64)) % p64  # (< 2^48 + 2^48)
        t = ssp[0, c0: c0 + col_block].astype(np.uint64)[None, :] % p64
        out[:, c0: c0 + col_block] = (s + delta * t % p64) % p64  # delta, t < 2^32: the product fits 64 bits
    return out


def w_polys_plain(ssp_rows, bits_list, deltas, m):
    """the definition in Python integers, a loop per statement, row and coefficient: the check of w_polys (small shapes only)"""
    d = len(ssp_rows[0])
    out = []
    for bits, delta in zip(bits_list, deltas):
        w = [int(delta) * int(ssp_rows[0][k]) % P for k in range(d)]
        for i in range(1, m):
            if (bits[(i - 1) >> 3] >> ((i - 1) & 7)) & 1:
                row = ssp_rows[i + 1]
                for k in range(d):
                    w[k] = (w[k] + int(row[k])) % P
        out.append(w)
    return out
