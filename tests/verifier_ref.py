"""The verifier's four equations in Python integers, and proofs built by construction instead of by the prover.

verifier() (reference src/snark.c:192-250) decrypts the five ciphertexts of a proof to h_s, hath_s, hatv_s, w_s, b_s, forms v_s = v_0(s) + w_s (plus the
statement's v_i(s) with public inputs) and asks four things (src/snark.c:219-235):
    first eq-pke   h_s alpha = hath_s          second eq-pke   v_s alpha = hatv_s
    eq-div         v_s^2 - 1 - h_s t(s) = 0    eq-lin          w_s beta = b_s          (all mod p)
The "test-error" bound behind them (src/snark.c:238-241) can never reject -- it takes SIZ of a non-positive value, which is <= 0 < 80 -- as csrc/snark.hip
(verify_checks), host/mfuoco_gpu.c (verifier) and oracle/mf_oracle.c (mfo_verifier) each say where they leave it out; it is left out here too.

A proof made by the prover from a random instance fails these checks in few ways and never sits at an edge of the field.  A ciphertext whose decryption the test
chooses puts any five field elements in front of them: with a = 0 it decrypts to b mod p, and with any a and b = (<a, sk> mod 2^(64 K)) + value + k p to value
(regev_decrypt, src/lwe.c:105-111: (b - modq(<a, sk>)) mod p, b as it stands in memory).  No CRS, no prover, no setup.

tests/test_verifier_ref_cpu.py pins this file against the oracle; tests/test_gpu_verifier_checks.py rests on it."""
import itertools

import numpy as np

import oracle_lib as ol

P = ol.P
CHECK_NAMES = ("eq-pke h", "eq-pke v", "eq-div", "eq-lin")
KINDS = ("zero", "above", "below", "unreduced")
SUBSETS = [frozenset(c) for r in range(5) for c in itertools.combinations(range(4), r)]  # the 16 sets of failing checks, the empty one first

# (s, alpha, beta) of the parameter sets the matrix is run at; "root" is run with t = x - s, so that t(s) = 0
PARAM_SETS = {"random": (12345, 7, 9), "pm1": (P - 1, P - 1, P - 1), "zero": (0, 0, 0), "one": (1, 1, 1), "root": (12345, 7, 9)}


def checks(h_s, hath_s, hatv_s, w_s, b_s, t_s, v_s, alpha, beta):
    """(first eq-pke, second eq-pke, eq-div, eq-lin) of src/snark.c:219-235, each True where the reference goes on to the next line"""
    return ((h_s * alpha) % P == hath_s,
            (v_s * alpha) % P == hatv_s,
            (v_s * v_s - 1 - h_s * t_s) % P == 0,
            (w_s * beta) % P == b_s)


def accept(*args):
    return all(checks(*args))


def v_s(vk, lu, u_bytes, w_s):
    """vk = [t(s), v_0(s), v_1(s) .. v_lu(s)]: v_0(s) + w_s + the v_i(s) of the statement's set bits, mod p; bits at lu and above are not read"""
    acc = int(vk[1]) + w_s
    for i in range(lu):
        if (u_bytes[i >> 3] >> (i & 7)) & 1:
            acc += int(vk[i + 2])
    return acc % P


def horner(coeffs, x):
    r = 0
    for c in reversed(coeffs):
        r = (r * x + int(c)) % P
    return r


def w_list(v0_s):
    """w_s at the edges: v_s = v_0(s) + w_s takes the values v_0(s), v_0(s) + 1, v_0(s) - 1 (wraps past p for most v_0(s)), 1, -1, 0, and an ordinary one"""
    return [0, 1, P - 1, (1 - v0_s) % P, (-1 - v0_s) % P, (-v0_s) % P, 777]


def matrix(t_s, v0_s, alpha, beta, w_values):
    """(values, failing) for every w_s and every set of failing checks: values = (h_s, hath_s, hatv_s, w_s, b_s), failing = the frozenset of indices into
    CHECK_NAMES that do not hold for them.  A failing check is the right value plus 1.  With t(s) = 0 eq-div does not depend on h_s: it holds for v_s = +-1 and
    fails otherwise, so only the subsets that agree with that exist there (h_s arbitrary)."""
    for w in w_values:
        for failing in SUBSETS:
            values = row(t_s, v0_s, alpha, beta, w, failing)
            if values is not None:
                yield values, failing


def row(t_s, v0_s, alpha, beta, w, failing=frozenset()):
    """the values (h_s, hath_s, hatv_s, w_s, b_s) at w_s = w for which exactly the checks in `failing` do not hold; None where t(s) = 0 rules the subset out"""
    vs = (v0_s + w) % P
    if t_s:
        h = ((vs * vs - 1) * pow(t_s, P - 2, P) + (2 in failing)) % P
    else:
        if (2 in failing) == (vs in (1, P - 1)):
            return None
        h = (0x9E3779B1 * (w + 1) + len(failing)) % P
    return (h, (h * alpha + (0 in failing)) % P, (vs * alpha + (1 in failing)) % P, w, (w * beta + (3 in failing)) % P)


def single_failures(t_s, v0_s, alpha, beta, w):
    """five value tuples at one w_s: all checks hold, then each check failing alone (t(s) != 0)"""
    return [row(t_s, v0_s, alpha, beta, w)] + [row(t_s, v0_s, alpha, beta, w, frozenset([k])) for k in range(4)]


# ---- ciphertexts with a chosen decryption -----------------------------------------------------------------------------------------------
def shared_a(p, sk, rng):
    """one random a of full logq bits per coordinate and <a, sk> mod 2^(64 K) in Python integers, for a whole batch: (a as (n, L) uint64, dot)"""
    a = ol.rand_values(rng, p.n, p.L, p.logq)
    mod = 1 << (64 * p.K)
    dot = sum(ol.limbs_to_int(a[j]) * ol.limbs_to_int(sk[j]) for j in range(p.n)) % mod
    return a, dot


def _rand_below(rng, bound):
    """a random integer in [0, bound), bound >= 1"""
    nb = (bound.bit_length() + 7) // 8 + 8
    return int.from_bytes(rng.bytes(nb), "little") % bound


def craft_b(p, a_kind, value, rng, dot=0):
    """the b coordinate (a Python integer below 2^(64 L)) that makes a ciphertext with <a, sk> mod 2^(64 K) = dot decrypt to value"""
    assert 0 <= value < P
    mod = 1 << (64 * p.K)
    if a_kind == "zero":  # a = 0: b = value + k p below 2^(64 K)
        return value + P * _rand_below(rng, (mod - value) // P)
    if a_kind == "above":  # b >= dot: the difference is reduced as it stands
        room = (mod - 1 - dot - value) // P
        assert room >= 0
        return dot + value + P * _rand_below(rng, room + 1)
    if a_kind == "below":  # a small b under a large dot product: the difference is negative before the reduction
        return dot + value - P * (dot // P)
    if a_kind == "unreduced":
        # b as a raw ct_import leaves it (src/lwe.c:125): a random non-zero part above 2^(64 K), read by regev_decrypt at its full L limbs.  At logq 1472
        # L = K and memory has no such bits: there the top limb is the random part (its top bit set, so b sits at the full width of its storage).
        split = 64 * p.K if p.L > p.K else 64 * (p.K - 1)
        width = 64 * p.L - split
        hi = _rand_below(rng, (1 << width) - 1) + 1
        if p.L == p.K:
            hi |= 1 << (width - 1)
        low = (value + dot - (hi << split)) % P
        return (hi << split) + low + P * _rand_below(rng, ((1 << split) - low) // P)
    raise ValueError(a_kind)


def craft_ct(p, sk, a_kind, value, rng, shared=None):
    """an (n + 1, L) uint64 ciphertext that decrypts to value under sk ((n, L) uint64); shared = shared_a(...) to form the dot product once for many"""
    ct = np.zeros((p.n + 1, p.L), dtype=np.uint64)
    dot = 0
    if a_kind != "zero":
        a, dot = shared if shared is not None else shared_a(p, sk, rng)
        ct[:p.n] = a
    ct[p.n] = ol.int_to_limbs(craft_b(p, a_kind, value, rng, dot), p.L)
    return ct


def craft_proof(p, sk, a_kinds, values, rng, shared=None, out=None):
    """five ciphertexts in the order h, hat_h, hat_v, v_w, b_w decrypting to values: (5, n + 1, L) uint64"""
    out = np.empty((5, p.n + 1, p.L), dtype=np.uint64) if out is None else out
    for j in range(5):
        out[j] = craft_ct(p, sk, a_kinds[j], values[j], rng, shared)
    return out


def mixed_kinds(i):
    """the kinds of proof i's five ciphertexts: every kind reaches every position within four consecutive proofs"""
    return [KINDS[(i + j) % 4] for j in range(5)]


def craft_batch(p, sk, rows, rng, shared, kinds=mixed_kinds):
    """rows: value 5-tuples -> (len(rows), 5, n + 1, L) uint64"""
    out = np.empty((len(rows), 5, p.n + 1, p.L), dtype=np.uint64)
    for i, values in enumerate(rows):
        craft_proof(p, sk, kinds(i), values, rng, shared, out=out[i])
    return out


def ssp_with(p, t, v0):
    """a host SSP in the file layout ((m + 3) slots of d little-endian uint64) with the given slots 0 (t) and 1 (v_0), the rest zero"""
    ssp = np.zeros((p.m + 3) * p.d, dtype=np.uint64)
    ssp[:len(t)] = np.asarray(t, dtype=np.uint64)
    ssp[p.d:p.d + len(v0)] = np.asarray(v0, dtype=np.uint64)
    return ssp


def instance(p, name, rng):
    """(s, alpha, beta, t, v0) of a parameter set: arbitrary coefficients below p in slots 0 and 1; t = x - s for "root" """
    s, alpha, beta = PARAM_SETS[name]
    v0 = [int(x) for x in rng.integers(0, P, size=p.d, dtype=np.uint64)]
    t = [(-s) % P, 1] + [0] * (p.d - 2) if name == "root" else [int(x) for x in rng.integers(0, P, size=p.d, dtype=np.uint64)]
    return s, alpha, beta, t, v0
