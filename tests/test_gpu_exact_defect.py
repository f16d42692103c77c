"""GPU: the exact-division check of the batch polynomial step (csrc/poly.hip, k_exact_check) against statements crafted to pass it at points known in advance
(tests/exact_defect_ref.py: t does not divide v^2 - 1, yet the cyclic quotient g satisfies g t = v^2 - 1 at those four points).

1. the points are drawn per preparation and per context, and the getter / pinning setter (mfh_poly_exact_points, mfh_set_poly_exact_points) check their arguments;
2. positive control: with the points pinned to the constants poly.hip used to check at, the crafted statements pass the check -- h is g and nothing is counted --
   so the statements are aimed at the check, and a check that missed them with drawn points would be blind;
3. with drawn points, a batch of 8 (crafted statements at 0, 3 and 7, satisfying ones elsewhere) in modes 1, 2 and 0 at every shape of the exact path -- generic
   cyclic products (d = 256, 2^17, 2^20), k_exact_seam<1> (d = 4093), <4> (2^15), <5> (2^16), and the row SSP's t at 2^20 -- equals the Euclidean quotients (the
   oracle's nmod_poly_div restatement, or GMP with a certificate above 4096) and counts the 3 crafted statements;
4. the prover: an SSP whose v_0 is crafted and v_1 = 1 - v_0, so that witness bit 0 selects a satisfying statement: mfh_prove_batch equals the oracle's prover
   (DEBUG) and mfh_prove statement by statement (d = 2^15, where a single proof takes the Euclidean path)."""
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import exact_defect_ref as xd
import oracle_lib as ol

pytestmark = pytest.mark.gpu

P = ol.P
MFH_EINVAL = -1
CRAFTED = (0, 3, 7)
SEED = bytes((11 * i + 3) & 0xFF for i in range(40))


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def kron():
    return ol.PolyKron()


def _dev(c, arr):
    return c.to_device(np.ascontiguousarray(arr, dtype=np.uint32))


def _rc(err):
    return int(re.search(r"libmfhip error (-?\d+)", str(err)).group(1))


def _scale(f, a):
    """a f mod p (uint64: a product of two residues is below 2^64)"""
    return np.ascontiguousarray(f, dtype=np.uint64) * np.uint64(a % P) % np.uint64(P)


def _batch(D, rng):
    """8 statements: v + a t (crafted) at CRAFTED, 1 + a t (t | v^2 - 1, quotient 2a + a^2 t) elsewhere.  Returns them, the satisfying ones' quotients and the a's."""
    V, honest, scal = [], {}, []
    for b in range(8):
        a = int(rng.integers(1, P))
        scal.append(a)
        if b in CRAFTED:
            V.append((D.v + _scale(D.t, a)) % np.uint64(P))
        else:
            V.append(_scale(D.t, a))
            V[-1][0] = (V[-1][0] + np.uint64(1)) % np.uint64(P)
            q = _scale(D.t, a * a % P)
            q[0] = (q[0] + np.uint64(2 * a % P)) % np.uint64(P)
            honest[b] = q
    return np.stack(V), honest, scal


# ------------------------------------------------------------------ 1. the points
def test_points_are_drawn_per_preparation(gpu_ctx_factory, mf):
    p = mf.DEBUG
    rng = np.random.default_rng(1)
    D = xd.craft(p.d, xd.splitmix_points(), rng=rng)
    a, b = gpu_ctx_factory(p), gpu_ctx_factory(p)
    with pytest.raises(mf.MfhError) as e:
        a.exact_points()  # nothing prepared
    assert _rc(e.value) == MFH_EINVAL
    seen = []
    for c in (a, b, a):
        c.poly_prepare_t(_dev(c, D.t))
        pts = c.exact_points()
        assert len(set(pts)) == 4 and all(2 <= x < P - 1 for x in pts), pts
        assert all(xd.evaluate(D.t, x) for x in pts), "a check point is a root of t"
        seen.append(tuple(pts))
    assert len(set(seen)) == 3, f"the same points twice: {seen}"
    assert not set(seen[0]) & set(xd.splitmix_points())
    # pinned: from the next preparation on, until unpinned
    pin = [2, 3, P - 2, 0x12345678]
    a.set_exact_points(pin)
    assert a.exact_points() == list(seen[2])
    for _ in range(2):
        a.poly_prepare_t(_dev(a, D.t))
        assert a.exact_points() == pin
    for bad in ([0, 3, 4, 5], [1, 3, 4, 5], [2, 3, 4, P - 1], [2, 3, 4, P], [2, 3, 4, 2**32 - 1], [2, 3, 2, 5], [9, 9, 9, 9]):
        with pytest.raises(mf.MfhError) as e:
            a.set_exact_points(bad)
        assert _rc(e.value) == MFH_EINVAL, bad
    a.poly_prepare_t(_dev(a, D.t))
    assert a.exact_points() == pin, "a refused setting changed the pinned points"
    a.set_exact_points(None)
    a.poly_prepare_t(_dev(a, D.t))
    assert a.exact_points() != pin
    # no exact path for this t (deg t < d - 1): no points
    t_short = D.t.copy()
    t_short[-1] = 0
    a.poly_prepare_t(_dev(a, t_short))
    with pytest.raises(mf.MfhError) as e:
        a.exact_points()
    assert _rc(e.value) == MFH_EINVAL


# ------------------------------------------------------------------ 2. positive control
def test_pinned_constants_are_blind_to_the_crafted_statements(gpu_ctx_factory, oracle, mf):
    p = mf.DEBUG
    rng = np.random.default_rng(2)
    D = xd.craft(p.d, xd.splitmix_points(), rng=rng, want_g=True)
    V, honest, scal = _batch(D, rng)
    c = gpu_ctx_factory(p)
    c.set_exact_points(xd.splitmix_points())
    c.poly_prepare_t(_dev(c, D.t))
    assert c.exact_points() == xd.splitmix_points()
    c.set_poly_exact(2)
    assert c.poly_exact_fallbacks() == 0
    got = c.to_host(c.poly_h_many(_dev(c, V.reshape(-1)), 8), np.uint32).astype(np.uint64).reshape(8, p.d)
    assert c.poly_exact_fallbacks() == 0, "the pinned check caught a crafted statement: the construction does not aim at it"
    t, v, g = D.t.astype(object), D.v.astype(object), D.g.astype(object)
    for b in range(8):
        if b in CRAFTED:
            a = scal[b]
            exp = ((g + 2 * a * v + a * a * t) % P).astype(np.uint64)  # the cyclic quotient of v + a t
            assert np.array_equal(got[b], exp), f"statement {b} is not the crafted cyclic quotient"
            assert not np.array_equal(got[b], oracle.poly_h(V[b], D.t))
        else:
            assert np.array_equal(got[b], honest[b]), f"statement {b}"


# ------------------------------------------------------------------ 3. drawn points
def _rows_t(c, p):
    """the row SSP's t (ssp_rows.hip: prod (x - r_j), r_j = j + 2, j < d - 1), from the tree of t of a registration without rows"""
    c.ssp_set_rows([])
    t = c.to_host(c.ssp_rows_fill(0, 1), np.uint32).astype(np.uint64)
    c.ssp_set_rows(None)
    return t


@pytest.mark.parametrize("d,kind", [(256, "sparse"), (4093, "sparse"), (1 << 15, "sparse"), (1 << 16, "sparse"), (1 << 17, "sparse"), (1 << 20, "rows")])
def test_drawn_points_catch_the_crafted_statements(gpu_ctx_factory, oracle, kron, mf, d, kind):
    p = mf.Params(d=d, m=4)
    c = gpu_ctx_factory(p)
    rng = np.random.default_rng(d)
    if kind == "rows":
        t = _rows_t(c, p)
        assert t[-1] == 1
        roots = [int(j) + 2 for j in rng.choice(d - 1, size=5, replace=False)]
        D = xd.craft(d, xd.splitmix_points(), t=t, roots=roots, rng=rng)
    else:
        D = xd.craft(d, xd.splitmix_points(), rng=rng)
    V, honest, _ = _batch(D, rng)
    if d <= 4096:
        exp = {b: oracle.poly_h(V[b], D.t) for b in CRAFTED}
    else:
        with ThreadPoolExecutor(max_workers=3) as ex:
            exp = dict(zip(CRAFTED, ex.map(lambda b: kron.div(V[b], D.t)[:d].astype(np.uint64), CRAFTED)))
    c.poly_prepare_t(_dev(c, D.t))
    d_v = _dev(c, V.reshape(-1))
    c.poly_exact_fallbacks()
    for mode, counted in ((1, 3), (2, 3), (0, 0)):
        c.set_poly_exact(mode)
        got = c.to_host(c.poly_h_many(d_v, 8), np.uint32).astype(np.uint64).reshape(8, d)
        fb = c.poly_exact_fallbacks()
        for b in range(8):
            want = exp[b] if b in CRAFTED else honest[b]
            assert np.array_equal(got[b], want), f"mode {mode}, statement {b} ({'crafted' if b in CRAFTED else 'satisfying'}): fallbacks {fb}"
        assert fb == counted, f"mode {mode}: {fb} statements recomputed"
        if d > 4096:
            assert kron.div_certify(V[0], D.t, got[0])


# ------------------------------------------------------------------ 4. the prover
def _ssp(D, m, rng):
    """slot 0 = t, v_0 = the crafted v, v_1 = 1 - v, v_2 .. v_(m-1) and the last two slots: multiples of t"""
    ssp = np.zeros((m + 3, len(D.t)), dtype=np.uint64)
    ssp[0] = D.t
    ssp[1] = D.v
    ssp[2] = (np.uint64(P) - D.v) % np.uint64(P)
    ssp[2][0] = (ssp[2][0] + np.uint64(1)) % np.uint64(P)
    for i in range(3, m + 3):
        ssp[i] = _scale(D.t, int(rng.integers(0, P)))
    return ssp


def _statements(rng, m, nb):
    nbytes = (m + 7) // 8
    bits = []
    for b in range(nb):
        w = bytearray(rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes())
        w[0] = (w[0] & 0xFE) | (0 if b in CRAFTED else 1)  # bit 0: v_1 = 1 - v_0, a satisfying witness
        bits.append(bytes(w))
    deltas = [int(x) for x in rng.integers(0, P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    return bits, deltas, mags, signs


def test_prove_batch_with_crafted_statements_matches_the_oracle(gpu_ctx_factory, oracle, mf):
    p = mf.DEBUG
    rng = np.random.default_rng(4)
    D = xd.craft(p.d, xd.splitmix_points(), rng=rng)
    ssp = _ssp(D, p.m, rng)
    flat = ssp.reshape(-1)
    c = gpu_ctx_factory(p)
    c.set_seed(SEED)
    alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    etape = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    crs = oracle.setup(p, SEED, flat, alpha, beta, s, sk, etape)
    d_ssp = c.ssp_upload(flat)
    c.ssp_prepare(d_ssp)
    d_crs = c.to_device(np.concatenate([crs["s"], crs["as_"], crs["t"], crs["v"][: (p.m - 1) * p.ctb]]))
    nb = 8
    bits, deltas, mags, signs = _statements(rng, p.m, nb)
    refs = []
    for b in range(nb):
        stape = b"".join(mags[b][80 * k: 80 * k + 80] + signs[b][k: k + 1] for k in range(5))
        refs.append(oracle.prover(p, crs, flat, bits[b], deltas[b], stape, 80))
        w = c.to_host(c.witness_poly(d_ssp, bits[b], deltas[b]), np.uint32).astype(np.uint64)
        assert np.array_equal(w, refs[b]["w"]), f"witness polynomial of statement {b}"
        assert oracle.poly_divides((w + D.v) % np.uint64(P), D.t) == (b not in CRAFTED)
    c.set_poly_exact(1)
    c.poly_exact_fallbacks()
    got = c.to_host(c.prove_batch(d_crs, d_ssp, bits, deltas, mags, signs), np.uint64).reshape(nb, 5, p.n + 1, p.L)
    assert c.poly_exact_fallbacks() == len(CRAFTED)
    for b in range(nb):
        assert np.array_equal(got[b], np.stack(refs[b]["proof"])), f"proof {b} differs from the oracle's prover"


def test_prove_batch_with_crafted_statements_at_the_default_d(gpu_ctx_factory, mf):
    p = mf.Params(d=1 << 15, m=16)
    rng = np.random.default_rng(5)
    D = xd.craft(p.d, xd.splitmix_points(), rng=rng)
    ssp = _ssp(D, p.m, rng)
    c = gpu_ctx_factory(p)
    c.set_seed(SEED)
    d_ssp = c.ssp_upload(ssp.reshape(-1))
    c.ssp_prepare(d_ssp)
    alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    etape = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    d_crs = c.setup(d_ssp, alpha, beta, s, c.to_device(sk), c.to_device(etape))
    nb = 8
    bits, deltas, mags, signs = _statements(rng, p.m, nb)
    c.set_poly_exact(1)
    c.poly_exact_fallbacks()
    got = c.prove_batch(d_crs, d_ssp, bits, deltas, mags, signs).view(nb, -1)
    assert c.poly_exact_fallbacks() == len(CRAFTED)
    for b in range(nb):
        one = c.prove(d_crs, d_ssp, bits[b], deltas[b], mags[b], signs[b])
        assert bool((got[b] == one).all()), f"proof {b} of the batch differs from the single-proof path"
