"""CPU: the exact polynomial reference the GPU polynomial step is compared with at full size (oracle/poly_kron.c, tests/oracle_lib.PolyKron) -- its
products against integer convolution and against closed forms, its quotients against the O(d^2) oracle (mfo_poly_h) and sympy, and its certificate
against quotients that are wrong by one coefficient or one term."""
import numpy as np
import pytest

import oracle_lib as ol

P = ol.P


@pytest.fixture(scope="module")
def kron():
    return ol.PolyKron()  # fails (does not skip) when libmf_gmpcheck.so is missing


def _conv(a, b):
    return [int(x) % P for x in np.convolve(np.asarray(a, dtype=np.uint64).astype(object), np.asarray(b, dtype=np.uint64).astype(object))]


@pytest.mark.parametrize("seed", range(12))
def test_mul_matches_integer_convolution(kron, seed):
    rng = np.random.default_rng(seed + 9100)
    la, lb = (int(x) for x in rng.integers(1, 3001, size=2))
    if seed == 0:
        la = 1
    if seed == 1:
        lb = 1
    if seed == 2:
        la = lb = 1
    a = rng.integers(0, P, size=la, dtype=np.uint64)
    b = rng.integers(0, P, size=lb, dtype=np.uint64)
    a[0], b[-1] = P - 1, P - 1
    assert kron.mul(a, b).tolist() == _conv(a, b)
    assert kron.mul(a).tolist() == _conv(a, a)  # the squaring call
    assert kron.mul(a, a.copy()).tolist() == _conv(a, a)  # ... equals the product of two equal operands


@pytest.mark.parametrize("logn", [16, 20])
def test_mul_matches_closed_forms(kron, logn):
    """all-(p - 1) operands: every slot holds a coefficient of up to 2^logn (p - 1)^2 (2^84 at 2^20) before the reduction"""
    n = 1 << logn
    top = np.full(n, P - 1, dtype=np.uint32)
    assert np.array_equal(kron.mul(top), ol.product_of_constants(P - 1, n, P - 1, n))
    assert np.array_equal(kron.mul(top, top[: n // 2 + 1]), ol.product_of_constants(P - 1, n, P - 1, n // 2 + 1))
    c = np.full(n - 3, 2**31, dtype=np.uint32)
    assert np.array_equal(kron.mul(c, top[:5]), ol.product_of_constants(2**31, n - 3, P - 1, 5))
    a = np.zeros(n, dtype=np.uint32)
    b = np.zeros(n + 1, dtype=np.uint32)
    a[n - 7], b[n] = P - 2, P - 1
    assert np.array_equal(kron.mul(a, b), ol.product_of_monomials(n - 7, P - 2, n, n, P - 1, n + 1))


def _case(case, d, seed):
    """the statements of test_gpu_snark.test_poly_h_matches_oracle, at any d"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, P, size=d, dtype=np.uint64)
    t = rng.integers(0, P, size=d, dtype=np.uint64)
    if case == "low_deg_t":
        t[d - 5:] = 0
    if case == "small_v":
        v[10:] = 0
    if case == "constant_t":
        t[1:] = 0
    if case == "valid_ssp":
        import c_lwe_snarks_amd as mf

        p = mf.Params(d=d, m=12)
        bits = rng.integers(0, 256, size=(p.m + 7) // 8, dtype=np.uint8).tobytes()
        ssp = ol.Oracle().ssp_from_tape(p, rng.integers(0, 256, size=p.m * 8 * d, dtype=np.uint8), bits).reshape(p.m + 3, d)
        t = ssp[0].copy()
        v = ssp[1].copy()
        for i in range(1, p.m):
            if (bits[(i - 1) >> 3] >> ((i - 1) & 7)) & 1:
                v = (v + ssp[i + 1]) % np.uint64(P)
    return v, t


CASES = ["dense", "low_deg_t", "small_v", "valid_ssp", "constant_t"]


@pytest.mark.parametrize("case,d", [(c, d) for c in CASES for d in [1, 2, 256, 1152, 4096] if d >= 16 or c in ("dense", "constant_t")])
def test_div_and_certify_match_the_oracle(kron, oracle, case, d):
    v, t = _case(case, d, CASES.index(case) * 7 + d)
    q = kron.div(v, t)
    assert np.array_equal(q[:d].astype(np.uint64), oracle.poly_h(v, t))
    assert kron.div_certify(v, t, q)
    # deg t = d - 1: the first d coefficients (what the GPU returns) are the whole quotient; a shorter t leaves some above them
    assert kron.div_certify(v, t, q[:d]) == (t[d - 1] != 0 or not np.any(q[d:]))
    if case == "valid_ssp":
        assert oracle.poly_divides(v, t)


@pytest.mark.parametrize("case", ["dense", "low_deg_t", "valid_ssp", "constant_t"])
def test_certify_rejects_a_quotient_off_by_one(kron, case):
    d = 512
    v, t = _case(case, d, 31 + CASES.index(case))
    q = kron.div(v, t)
    n = int(np.flatnonzero(q)[-1]) + 1  # deg A - deg t + 1
    rng = np.random.default_rng(5)
    for i in [0, n - 1, int(rng.integers(1, n - 1))]:
        for delta in (1, P - 1):
            bad = q.copy()
            bad[i] = (int(bad[i]) + delta) % P
            assert not kron.div_certify(v, t, bad), (i, delta)
    assert not kron.div_certify(v, t, q[: n - 1])  # one coefficient too short
    assert not kron.div_certify(v, t, np.zeros(n, dtype=np.uint32))
    longer = np.zeros(n + 1, dtype=np.uint32)
    longer[:n] = q[:n]
    assert kron.div_certify(v, t, longer)  # (a trailing zero is the same polynomial)
    longer[n] = 1
    assert not kron.div_certify(v, t, longer)  # one term too many


def test_certify_of_a_zero_quotient(kron):
    """deg A < deg t: the quotient is 0 and nothing else; A = 0 (v = +-1): the same"""
    t = np.arange(1, 41, dtype=np.uint32)
    v = np.array([3, 5], dtype=np.uint32)
    assert kron.div_certify(v, t, np.zeros(4, dtype=np.uint32)) and not kron.div_certify(v, t, np.array([1], dtype=np.uint32))
    assert not np.any(kron.div(v, t))
    for one in (1, P - 1):
        v = np.array([one, 0, 0], dtype=np.uint32)
        assert not np.any(kron.div(v, t[:1]))
        assert kron.div_certify(v, t[:1], np.zeros(1, dtype=np.uint32))


@pytest.mark.parametrize("seed", range(6))
def test_div_matches_sympy(kron, seed):
    sympy = pytest.importorskip("sympy")
    rng = np.random.default_rng(seed + 600)
    d = int(rng.integers(1, 24))
    dt = int(rng.integers(0, d))
    v = rng.integers(0, P, size=d, dtype=np.uint64)
    t = np.zeros(d, dtype=np.uint64)
    t[: dt + 1] = rng.integers(1, P, size=dt + 1, dtype=np.uint64)
    x = sympy.symbols("x")
    fv = sympy.Poly([int(c) for c in v[::-1]], x, modulus=P)
    ft = sympy.Poly([int(c) for c in t[::-1]], x, modulus=P)
    qs, _ = sympy.div(fv * fv - sympy.Poly(1, x, modulus=P), ft)
    exp = [int(c) % P for c in qs.all_coeffs()[::-1]]
    exp = (exp + [0] * (2 * d))[: 2 * d - 1]
    assert kron.div(v, t).tolist() == exp
