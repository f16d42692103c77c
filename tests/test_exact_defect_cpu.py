"""CPU: the crafted statement of tests/exact_defect_ref.py defeats an exact-division check whose four points are known in advance -- here the splitmix64 constants
poly.hip used to check at.  At small d in plain Python integers, against the oracle's Euclidean division: t is a unit modulo x^N - 1; the cyclic product the exact path
computes, (v^2 - 1 mod x^N - 1) t^-1 mod x^N - 1, is the crafted g; g t = v^2 - 1 holds at the four points; yet t does not divide v^2 - 1, the oracle's quotient is not
g, and the identity fails at random points.  At the sizes the product runs (2^15, 2^20) the O(d) construction is checked by evaluation identities alone."""
import numpy as np
import pytest

import exact_defect_ref as xd
from test_exact_division_math import cyc_inv, cyc_mul, evaluate

P = xd.P


def _cyclic_quotient(v, t, N):
    v2 = cyc_mul(v, v, N)
    v2[0] = (v2[0] - 1) % P
    tinv = cyc_inv(t + [0] * (N - len(t)))
    assert tinv is not None, "t is not a unit modulo x^N - 1"
    return cyc_mul(v2, tinv, N)


@pytest.mark.parametrize("d", [64, 61, 256])
def test_crafted_v_passes_the_fixed_points(oracle, d):
    pts = xd.splitmix_points()
    D = xd.craft(d, pts, want_g=True)
    assert D.k == D.N - d + 5
    t, v, g = [int(x) for x in D.t], [int(x) for x in D.v], [int(x) for x in D.g]
    assert t[-1] != 0 and v[-1] == 0 and len(t) == len(v) == len(g) == d
    h = _cyclic_quotient(v, t, D.N)
    assert h[:d] == g and not any(h[d:]), "the cyclic product is not the crafted g"
    for c in pts:
        assert evaluate(g, c) * evaluate(t, c) % P == (evaluate(v, c) ** 2 - 1) % P, f"the identity fails at the fixed point {c}"
    assert not oracle.poly_divides(D.v, D.t)
    assert not np.array_equal(oracle.poly_h(D.v, D.t), D.g), "g is the Euclidean quotient"
    rng = np.random.default_rng(d + 1)
    for z in (int(x) for x in rng.integers(2, P - 1, size=8)):
        assert evaluate(g, z) * evaluate(t, z) % P != (evaluate(v, z) ** 2 - 1) % P, f"the identity holds at the random point {z}"
    # v + delta t: the same defect, the quotient g + 2 delta v + delta^2 t
    delta = 0x12345677
    vd = [(a + delta * b) % P for a, b in zip(v, t)]
    gd = [(a + 2 * delta * b + delta * delta * c) % P for a, b, c in zip(g, v, t)]
    assert _cyclic_quotient(vd, t, D.N)[:d] == gd
    assert not oracle.poly_divides(np.array(vd, dtype=np.uint64), D.t)


@pytest.mark.parametrize("d", [1 << 15, 1 << 20])
def test_crafted_v_at_product_sizes(d):
    """t = T_J T_S, F = v^2 - 1 + (x^N - 1) K vanishes at every root of T_S and on T_J (v = 1 + T_J u, K = lambda C T_J), deg F - deg t < N; K vanishes at the four
    points (the check passes there) and not at random points (it fails there); v^2 = 1 fails at a root of t (t does not divide v^2 - 1)."""
    pts = xd.splitmix_points()
    D = xd.craft(d, pts)
    N, t, v, K = D.N, D.t, D.v, D.K
    assert N == d and D.k == 5 and len(t) == d and t[-1] == 1 and v[-1] == 0
    assert len(K) - 1 + N - (d - 1) < N  # deg g
    rng = np.random.default_rng(d)
    for z in (int(x) for x in rng.integers(2, P - 1, size=3)):
        assert xd.evaluate(t, z) == xd.evaluate(D.TJ, z) * xd.evaluate(xd.from_roots(D.s), z) % P
        assert (xd.evaluate(v, z) - 1) % P == xd.evaluate(D.TJ, z) * evaluate(D.u, z) % P  # v = 1 on T_J
        assert xd.evaluate(K, z) == D.lam * xd.evaluate(D.TJ, z) * xd.evaluate(xd.from_roots(pts), z) % P
        assert (pow(z, N, P) - 1) * xd.evaluate(K, z) % P != 0, "the check would hold at a random point"
    for c in pts:
        assert xd.evaluate(K, c) == 0
    ok = []
    for s in D.s:
        assert xd.evaluate(t, s) == 0
        vs = xd.evaluate(v, s)
        assert (vs * vs - 1 + (pow(s, N, P) - 1) * xd.evaluate(K, s)) % P == 0
        ok.append((vs * vs - 1) % P == 0)
    assert not all(ok), "t divides v^2 - 1"


def test_crafted_v_for_a_given_t(oracle):
    """the branch the row SSP's test takes: t = prod (x - r_j), r_j = j + 2 (ssp_rows.hip), T_J = t / T_S for k of its roots"""
    d = 64
    pts = xd.splitmix_points()
    t = xd.from_roots([j + 2 for j in range(d - 1)])
    D = xd.craft(d, pts, t=t, roots=[5, 17, 18, 40, 64], want_g=True)
    assert np.array_equal(D.t, t)
    tl, v, g = [int(x) for x in t], [int(x) for x in D.v], [int(x) for x in D.g]
    assert _cyclic_quotient(v, tl, D.N)[:d] == g
    for c in pts:
        assert evaluate(g, c) * evaluate(tl, c) % P == (evaluate(v, c) ** 2 - 1) % P
    assert not oracle.poly_divides(D.v, D.t)
