"""CPU: the algorithm of the row SSP (csrc/ssp_rows.hip) restated with Python integers at small d -- the subproduct tree of t padded with factors x,
bottom nodes by the synthetic-division recurrence, upper levels N_parent = N_L T_R' + N_R T_L' + x^L (N_L + N_R), the root shifted down -- equals direct
Lagrange interpolation and circuit_ref.ssp; and the setup scalars lambda_j(s) = w_j t(s) / (s - r_j) are the Lagrange basis at s, the indicator at a point."""
import random

import numpy as np
import pytest

import circuit_ref as cr

P = cr.P


def pmul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % P
    return out


def weights(n):
    pts = [j + 2 for j in range(n)]
    w = []
    for j in range(n):
        den = 1
        for l in range(n):
            if l != j:
                den = den * (pts[j] - pts[l]) % P
        w.append(pow(den, P - 2, P))
    return w


def tree_interp(d, vals, G=64):
    """coefficients (degree < d - 1) of the interpolant of vals[j] at r_j = j + 2, the way ssp_rows.hip computes them"""
    n = d - 1
    Np = 1
    while Np < d:
        Np <<= 1
    G = min(G, Np)
    w = weights(n)
    r = [j + 2 if j < n else 0 for j in range(Np)]
    c = [vals[j] * w[j] % P if j < n else 0 for j in range(Np)]
    T, N = [], []  # level vectors: node k of degree L at [kL, (k+1)L), low coefficients
    for node in range(Np // G):
        t = [1]
        for l in range(G):
            t = pmul(t, [(-r[node * G + l]) % P, 1])
        T += t[:G]
        acc = [0] * G
        for l in range(G):
            j = node * G + l
            q = 1
            for k in range(G - 1, -1, -1):
                acc[k] = (acc[k] + c[j] * q) % P
                if k:
                    q = (t[k] + r[j] * q) % P
        N += acc
    L = G
    while L < Np:
        T2, N2 = [], []
        for k in range(Np // (2 * L)):
            tl, tr = T[2 * k * L:(2 * k + 1) * L], T[(2 * k + 1) * L:(2 * k + 2) * L]
            nl, nr = N[2 * k * L:(2 * k + 1) * L], N[(2 * k + 1) * L:(2 * k + 2) * L]
            pt = pmul(tl, tr) + [0]
            pn = [(x + y) % P for x, y in zip(pmul(nl, tr) + [0], pmul(nr, tl) + [0])]
            for i in range(L):
                pt[L + i] = (pt[L + i] + tl[i] + tr[i]) % P
                pn[L + i] = (pn[L + i] + nl[i] + nr[i]) % P
            T2 += pt
            N2 += pn
        T, N, L = T2, N2, 2 * L
    t = [T[k + Np - n] for k in range(n)] + [1]
    return [N[k + Np - n] for k in range(n)] + [0], t


def lagrange(d, vals):
    n = d - 1
    pts = [j + 2 for j in range(n)]
    out = [0] * d
    for j in range(n):
        basis, den = [1], 1
        for l in range(n):
            if l != j:
                basis = pmul(basis, [(-pts[l]) % P, 1])
                den = den * (pts[j] - pts[l]) % P
        f = vals[j] * pow(den, P - 2, P) % P
        for k, x in enumerate(basis):
            out[k] = (out[k] + f * x) % P
    return out


@pytest.mark.parametrize("d", [64, 130, 192])
def test_tree_equals_lagrange(d):
    rng = random.Random(d)
    vals = [rng.randrange(P) for _ in range(d - 1)]
    got, t = tree_interp(d, vals)
    assert got == lagrange(d, vals)
    exp_t = [1]
    for j in range(d - 1):
        exp_t = pmul(exp_t, [(-(j + 2)) % P, 1])
    assert t == exp_t


@pytest.mark.parametrize("G", [4, 8, 16])
def test_bottom_ntt_seam(G):
    """the same result whatever the height of the bottom nodes: the recurrence and the product levels meet anywhere"""
    d = 130
    rng = random.Random(G)
    vals = [rng.randrange(P) for _ in range(d - 1)]
    assert tree_interp(d, vals, G)[0] == tree_interp(d, vals, 64)[0]


def test_tree_equals_circuit_ref_ssp_1152():
    d, m = 1152, 6
    rng = np.random.default_rng(5)
    nrows = 700
    rows = [[(int(rng.integers(0, m)), int(rng.integers(0, P))) for _ in range(2)] for _ in range(nrows)]
    rp = np.zeros(nrows + 1, dtype=np.uint32)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    csr = (rp, np.array([x for r in rows for x, _ in r], dtype=np.uint32), np.array([a for r in rows for _, a in r], dtype=np.uint32))
    exp = cr.ssp(d, m, csr)
    for i in (0, 3):
        vals = [sum(a for x, a in rows[j] if x == i) % P if j < nrows else int(i == 0) for j in range(d - 1)]
        got, t = tree_interp(d, vals)
        assert got == [int(x) for x in exp[i + 1]]
        assert t == [int(x) for x in exp[0]]


def lam(d, s):
    n = d - 1
    w = weights(n)
    if 2 <= s < n + 2:
        return [int(j == s - 2) for j in range(n)]
    ts = 1
    for j in range(n):
        ts = ts * (s - j - 2) % P
    return [w[j] * ts * pow((s - j - 2) % P, P - 2, P) % P for j in range(n)]


@pytest.mark.parametrize("s", [123456789, 0, 1, 2, 2 + 70, 2 + 128])
def test_lambda_is_the_lagrange_basis(s):
    d = 130
    rng = random.Random(s)
    vals = [rng.randrange(P) for _ in range(d - 1)]
    coef = lagrange(d, vals)
    at_s = sum(x * pow(s, k, P) for k, x in enumerate(coef)) % P
    assert sum(v * l for v, l in zip(vals, lam(d, s))) % P == at_s
