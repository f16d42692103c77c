"""A statement aimed at the exact-division check of the batch prover's polynomial step (c-lwe-snarks_amd/csrc/poly.hip): a v with t NOT dividing v^2 - 1 whose
cyclic quotient g -- the unique h of degree < N with h t = v^2 - 1 (mod x^N - 1), N = 2^ceil(log2 d), what the exact path computes -- satisfies
g(c) t(c) = v(c)^2 - 1 at four given points c.  Points known in advance are blind to it; points drawn after v is fixed see it but for a probability ~ (2d / p)^4.

Construction, C = prod (x - c_i), k >= N - d + 5 roots s_j of t (not 0, +-1 or a c_i):  t = T_J T_S, T_S = prod (x - s_j);  K = lambda C T_J and v = 1 + T_J u with
deg u < k and, at every s_j, T_J(s_j) u^2 + 2 u + lambda (s_j^N - 1) C(s_j) = 0 (u = (sigma - 1) / T_J(s_j), sigma^2 = 1 - lambda T_J(s_j) (s_j^N - 1) C(s_j): lambda is
drawn until all k are squares; p = 3 mod 4, so sigma = D^((p + 1) / 4)).  Then F = v^2 - 1 + (x^N - 1) K vanishes on T_J (v = 1 there, K = 0) and at every s_j, so
t | F and g = F / t has degree <= max(d - 3, N + 4 - k) < d: g t = v^2 - 1 (mod x^N - 1), and at the c_i, where K = 0, g t = v^2 - 1 exactly.  But t does not divide
v^2 - 1 ((x^N - 1) K is not 0 modulo T_S), so g is not nmod_poly_div's quotient.  deg v = d - 2, and v + delta t keeps every property (g becomes
g + 2 delta v + delta^2 t): the defect survives the prover's w = ... + delta t.

Everything but g is O(d k) in numpy (uint64, every product of two residues below 2^64, sums of residues exact below 2^64 for 2^32 terms); g itself is an O(d N) division
in Python integers, for small d only."""
from dataclasses import dataclass

import numpy as np

P = 2**32 - 5
M64 = (1 << 64) - 1


def splitmix_points():
    """the four check points poly.hip used before they were drawn per preparation: 2 + splitmix64(j + 1) mod (p - 2), j < 4 -- public constants"""
    out = []
    for j in range(4):
        z = (0x9E3779B97F4A7C15 * (j + 1)) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out.append(2 + (z ^ (z >> 31)) % (P - 2))
    return out


def powers(x, n):
    """x^0 .. x^(n - 1) mod p (uint64), by doubling"""
    pw = np.ones(max(n, 1), dtype=np.uint64)
    filled = 1
    while filled < n:
        cnt = min(filled, n - filled)
        pw[filled:filled + cnt] = pw[:cnt] * np.uint64(pow(x, filled, P)) % np.uint64(P)
        filled += cnt
    return pw[:n]


def evaluate(f, x):
    f = np.ascontiguousarray(f, dtype=np.uint64)
    return int((f * powers(int(x) % P, len(f)) % np.uint64(P)).sum(dtype=np.uint64) % np.uint64(P))


def mul_short(a, b):
    """a (long, uint64 residues) times b (a short sequence of ints)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    out = np.zeros(len(a) + len(b) - 1, dtype=np.uint64)
    for j, c in enumerate(b):
        c = int(c) % P
        if c:
            out[j:j + len(a)] = (out[j:j + len(a)] + a * np.uint64(c) % np.uint64(P)) % np.uint64(P)
    return out


def from_roots(roots):
    f = np.ones(1, dtype=np.uint64)
    for r in roots:
        f = mul_short(f, [(-int(r)) % P, 1])
    return f


def div_linear(a, s):
    """a / (x - s), exact (asserted): q_i = sum_{l > i} a_l s^(l - i - 1), as suffix sums of a_l s^l scaled by s^-(i + 1)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    n = len(a)
    suffix = np.cumsum((a * powers(s, n) % np.uint64(P))[::-1], dtype=np.uint64)[::-1] % np.uint64(P)  # (< 2^32 terms below 2^32: exact)
    assert suffix[0] == 0, "s is not a root"
    return suffix[1:] * powers(pow(s, P - 2, P), n)[1:] % np.uint64(P)


def _mul_int(a, b):
    c = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                c[i + j] += x * y
    return [x % P for x in c]


@dataclass
class Defect:
    t: np.ndarray     # d coefficients, deg t = d - 1
    v: np.ndarray     # d coefficients, deg v <= d - 2
    g: np.ndarray     # d coefficients: the cyclic quotient (None unless asked for)
    N: int
    k: int
    s: list           # the k roots of t that carry the defect
    lam: int
    TJ: np.ndarray    # t / T_S
    u: list           # v = 1 + T_J u, deg u < k
    K: np.ndarray     # lambda C T_J: (v^2 - 1 + (x^N - 1) K) = t g


def craft(d, points, k=None, t=None, roots=None, rng=None, want_g=False):
    """The construction above for d coefficients, aimed at `points` (four distinct values, not 0 or +-1).  t, roots: a given t of degree d - 1 and k of its roots
    (the row SSP's t); else t = T_J T_S with T_J = x^(d - 1 - k) + a x + b and k random roots.  k: at least N - d + 5 (the default)."""
    N = 1 << (d - 1).bit_length()
    kmin = N - d + 5
    rng = rng if rng is not None else np.random.default_rng(d)
    cs = [int(c) % P for c in points]
    assert len(cs) == 4 and len(set(cs)) == 4 and not set(cs) & {0, 1, P - 1}
    C = from_roots(cs)
    if t is None:
        k = kmin if k is None else k
        assert d - 1 - k >= 2
        s = set()
        while len(s) < k:
            x = int(rng.integers(2, P - 1))
            if x not in cs:
                s.add(x)
        s = sorted(s)
        while True:
            TJ = np.zeros(d - k, dtype=np.uint64)
            TJ[-1], TJ[1], TJ[0] = 1, int(rng.integers(1, P)), int(rng.integers(1, P))
            if all(evaluate(TJ, x) for x in s):
                break
        t = mul_short(TJ, from_roots(s))
    else:
        t = np.ascontiguousarray(t, dtype=np.uint64)
        s = [int(x) % P for x in roots]
        k = len(s)
        assert len(set(s)) == k and not set(s) & ({0, 1, P - 1} | set(cs))
        TJ = t
        for x in s:
            TJ = div_linear(TJ, x)
    assert len(t) == d and t[-1] != 0 and k >= kmin
    tj = [evaluate(TJ, x) for x in s]
    assert all(tj), "a root of T_S is a root of T_J too"
    e = [(pow(x, N, P) - 1) * evaluate(C, x) % P for x in s]
    while True:
        lam = int(rng.integers(1, P))
        sig = []
        for a, b in zip(tj, e):
            D = (1 - lam * a * b) % P
            r = pow(D, (P + 1) // 4, P)
            if r * r % P != D:
                break
            sig.append(r)
        else:
            break
    uval = [(sg - 1) * pow(a, P - 2, P) % P for sg, a in zip(sig, tj)]
    u = [0] * k  # Lagrange interpolation through (s_j, u_j)
    for i, x in enumerate(s):
        L, den = [1], 1
        for j, y in enumerate(s):
            if j != i:
                L = _mul_int(L, [(-y) % P, 1])
                den = den * (x - y) % P
        w = uval[i] * pow(den, P - 2, P) % P
        u = [(a + w * b) % P for a, b in zip(u, L)]
    v = np.zeros(d, dtype=np.uint64)
    v[:d - 1] = mul_short(TJ, u)
    v[0] = (v[0] + np.uint64(1)) % np.uint64(P)
    K = mul_short(TJ, [lam * int(c) % P for c in C])
    g = None
    if want_g:
        vi, ti, Ki = [int(x) for x in v], [int(x) for x in t], [int(x) for x in K]
        F = _mul_int(vi, vi) + [0] * max(0, N + len(Ki) - (2 * d - 1))
        F[0] -= 1
        for i, x in enumerate(Ki):
            F[i + N] += x
            F[i] -= x
        F = [x % P for x in F]
        while F and F[-1] == 0:
            F.pop()
        q, inv = [0] * (len(F) - d + 1), pow(ti[-1], P - 2, P)
        for i in range(len(q) - 1, -1, -1):  # F / t, long division
            c = F[i + d - 1] * inv % P
            q[i] = c
            if c:
                for j, y in enumerate(ti):
                    F[i + j] = (F[i + j] - c * y) % P
        assert not any(F[:d - 1]), "t does not divide v^2 - 1 + (x^N - 1) K"
        assert len(q) <= d
        g = np.zeros(d, dtype=np.uint64)
        g[:len(q)] = q
    return Defect(t=t, v=v, g=g, N=N, k=k, s=s, lam=lam, TJ=TJ, u=u, K=K)
