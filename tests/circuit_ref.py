"""Python-integer restatement of mfh_ssp_from_rows (include/mfhip.h) for the tests: the SSP of a constraint system given row by row.

Points r_j = j + 2 (j < n = d - 1), t = prod_j (x - r_j), w_j = 1 / ((-1)^(n-1-j) j! (n-1-j)!), Q_j = t / (x - r_j) by synthetic division, and
v_i = sum_j V_ij w_j Q_j.  Rows j >= nrows are padding: v_0(r_j) = 1.  Everything mod p with numpy uint64 (no product exceeds 64 bits)."""
import numpy as np

P = 0xFFFFFFFB


def t_poly(d):
    """t = prod_{j < d-1} (x - r_j): d coefficients, low first"""
    n = d - 1
    t = np.zeros(d, dtype=np.uint64)
    t[0] = 1
    for j in range(n):
        r = np.uint64(j + 2)
        nt = np.zeros(d, dtype=np.uint64)
        nt[1:] = t[:-1]
        nt = (nt + (np.uint64(P) - (t * r) % np.uint64(P))) % np.uint64(P)
        t = nt
    return t


def weights(d):
    n = d - 1
    fact = [1] * (n + 1)
    for i in range(1, n + 1):
        fact[i] = fact[i - 1] * i % P
    return [pow((-1) ** (n - 1 - j) * fact[j] * fact[n - 1 - j] % P, P - 2, P) for j in range(n)]


def values(d, m, rows):
    """V (m x (d-1)): V[i][j] = v_i(r_j), with the padding rows"""
    row_ptr, wire, coef = (np.asarray(a, dtype=np.int64) for a in rows)
    n, nrows = d - 1, len(row_ptr) - 1
    V = np.zeros((m, n), dtype=np.uint64)
    for j in range(nrows):
        for e in range(int(row_ptr[j]), int(row_ptr[j + 1])):
            V[wire[e], j] = (int(V[wire[e], j]) + int(coef[e])) % P
    V[0, nrows:] = 1
    return V


def q_matrix(t):
    """Q[j][k] = coefficient k of t / (x - r_j), k < d"""
    d = len(t)
    n = d - 1
    r = np.arange(n, dtype=np.uint64) + np.uint64(2)
    Q = np.zeros((n, d), dtype=np.uint64)
    q = np.zeros(n, dtype=np.uint64)  # q_{j, d-1} = 0
    for k in range(d - 1, 0, -1):
        q = (t[k] + r * q) % np.uint64(P)
        Q[:, k - 1] = q
    return Q


def _matmul_mod(A, B):
    """A @ B mod p for uint64 matrices of residues (16-bit halves of B keep every partial sum below 2^64 for inner sizes < 2^16)"""
    lo = B & np.uint64(0xFFFF)
    hi = B >> np.uint64(16)
    return ((A @ hi) % np.uint64(P) * np.uint64(1 << 16) + (A @ lo) % np.uint64(P)) % np.uint64(P)


def ssp(d, m, rows, t=None):
    """the device SSP as mfh_ssp_from_rows writes it: (m + 3) x d uint64"""
    t = t_poly(d) if t is None else t
    w = np.array(weights(d), dtype=np.uint64)
    C = values(d, m, rows) * w % np.uint64(P)
    out = np.zeros((m + 3, d), dtype=np.uint64)
    out[0] = t
    out[1:m + 1] = _matmul_mod(C, q_matrix(t))
    return out


def horner(poly, x):
    """poly(x) mod p for a vector of points x (numpy uint64 Horner)"""
    x = np.asarray(x, dtype=np.uint64)
    acc = np.zeros_like(x)
    for c in np.asarray(poly, dtype=np.uint64)[::-1]:
        acc = (acc * x % np.uint64(P) + c) % np.uint64(P)
    return acc


def row_values(rows, bits: bytes):
    """value of every row on an input: v_0 term + sum_i a_i coef, mod p (bit i - 1 = wire i)"""
    row_ptr, wire, coef = (np.asarray(a, dtype=np.int64) for a in rows)
    out = []
    for j in range(len(row_ptr) - 1):
        acc = 0
        for e in range(int(row_ptr[j]), int(row_ptr[j + 1])):
            w = int(wire[e])
            if w == 0 or (bits[(w - 1) >> 3] >> ((w - 1) & 7)) & 1:
                acc += int(coef[e])
        out.append(acc % P)
    return out


def satisfied(rows, bits: bytes):
    return all(v in (1, P - 1) for v in row_values(rows, bits))
