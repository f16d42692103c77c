"""GPU: the polynomial step (csrc/poly.hip) against EXACT products and quotients at the sizes the product runs -- every NTT length from 2^1 to 2^23, every
split of the register passes, every k_exact_seam<K> shape and the generic cyclic path beyond it, the Euclidean path at large d with a short t, Garner's CRT at its
largest magnitude, and the size limits.  The reference is GMP (oracle/poly_kron.c through oracle_lib.PolyKron: one mpz_mul per product, quotients certified by
R = v^2 - 1 - q t with deg R < deg t) and closed forms where the inputs are structured; the O(d^2) oracle cannot reach these sizes.  Large batches are checked on
a few threads (the GMP calls release the GIL)."""
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

P = ol.P
Q = (998244353, 897581057, 880803841)  # the three NTT primes of poly.hip (kPrimes)
CONSTS = [P - 1, Q[0] - 1, Q[1] - 1, Q[2] - 1, 2**31, 1]  # every residue of each NTT prime at its maximum, 2^31, 1
MAX_LOG = 23  # the largest transform: 2^23 points
MFH_EINVAL, MFH_EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def kron():
    return ol.PolyKron()  # fails (does not skip) when libmf_gmpcheck.so is missing


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=8) as ex:
        yield ex


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory, mf):
    return gpu_ctx_factory(mf.DEBUG)


def _dev(c, arr):
    return c.to_device(np.ascontiguousarray(arr, dtype=np.uint32))


def _host(c, t, shape=None):
    h = c.to_host(t, np.uint32)
    return h.reshape(shape) if shape else h


def _rand(rng, n):
    a = rng.integers(0, P, size=n, dtype=np.uint64).astype(np.uint32)
    a[0], a[-1] = P - 1, P - 1  # nonzero ends: the lengths are exact
    return a


def _rc(err):
    return int(re.search(r"libmfhip error (-?\d+)", str(err)).group(1))


def _mul(c, a, b=None):
    """c.poly_mul on fresh device copies; b = None: the same tensor as both operands (the squaring path)"""
    da = _dev(c, a)
    if b is None:
        return _host(c, c.poly_mul(da, len(a), da, len(a)))
    return _host(c, c.poly_mul(da, len(a), _dev(c, b), len(b)))


# ------------------------------------------------------------------ a. mfh_poly_mul at every transform length
@pytest.mark.parametrize("k", range(1, MAX_LOG + 1))
def test_poly_mul_at_every_transform_length(ctx, kron, pool, k):
    """la + lb - 1 = 2^k exactly and 2^k + 1 (the padding step to the next length), distinct operands (k_ntt_lds_mul) and squares (k_ntt_lds_mul8 at 2^11 points
    and up): random coefficients against GMP, and at every k constant and monomial operands against closed forms.  This walks every ntt_top_passes
    split of the register passes (one pass of 1..5 stages, 4 + 3, 5 + 3, 3 + 3, 5 + 5, 5 + 3 + 3, 5 + 4 + 3)."""
    n = 1 << k
    rng = np.random.default_rng(7000 + k)
    jobs = []
    for L in [n, n + 1] if k < MAX_LOG else [n]:
        la = (L + 1) // 2
        a, b = _rand(rng, la), _rand(rng, L + 1 - la)
        jobs.append((f"{la} x {len(b)}", _mul(ctx, a, b), pool.submit(kron.mul, a, b)))
    for la in [max(n // 2, 1), n // 2 + 1] if k < MAX_LOG else [n // 2]:
        a = _rand(rng, la)
        jobs.append((f"square of {la}", _mul(ctx, a), pool.submit(kron.mul, a)))
    la = (n + 1) // 2
    lb = n + 1 - la
    sq = max(n // 2, 1)
    for cst in CONSTS:
        got = _mul(ctx, np.full(la, cst, np.uint32), np.full(lb, cst, np.uint32))
        assert np.array_equal(got, ol.product_of_constants(cst, la, cst, lb)), f"constant {cst}: {la} x {lb}"
        got = _mul(ctx, np.full(sq, cst, np.uint32))
        assert np.array_equal(got, ol.product_of_constants(cst, sq, cst, sq)), f"constant {cst}: square of {sq}"
    i, j = la - 1, int(rng.integers(0, lb))
    a, b = np.zeros(la, np.uint32), np.zeros(lb, np.uint32)
    a[i], b[j] = P - 1, Q[2] + 7
    assert np.array_equal(_mul(ctx, a, b), ol.product_of_monomials(i, P - 1, la, j, Q[2] + 7, lb)), "monomials"
    for name, got, fut in jobs:
        assert np.array_equal(got, fut.result()), name


@pytest.mark.parametrize("la,lb", [(1, 1 << 23), (1 << 23, 1), (3 << 21, (1 << 21) + 1)])
def test_poly_mul_unbalanced_at_2_23(ctx, kron, la, lb):
    rng = np.random.default_rng(la + 3 * lb)
    a, b = _rand(rng, la), _rand(rng, lb)
    assert np.array_equal(_mul(ctx, a, b), kron.mul(a, b))


# ------------------------------------------------------------------ b. limits
def test_poly_mul_size_limit(ctx, kron, mf):
    """2^23 coefficients with every one p - 1: accepted and exact -- coefficients up to 2^22 (p - 1)^2 ~ 2^86, Garner's largest top digit (p1 p2 p3 ~ 2^89.35).
    2^23 + 1: refused with the limit in the message, and the context still multiplies correctly after it."""
    h = 1 << 22
    top = np.full(h + 1, P - 1, np.uint32)
    d_top = _dev(ctx, top)
    got = _host(ctx, ctx.poly_mul(d_top, h, d_top, h + 1))
    assert np.array_equal(got, ol.product_of_constants(P - 1, h, P - 1, h + 1))
    got = _host(ctx, ctx.poly_mul(d_top, h, d_top, h))  # the square: 2^23 - 1 coefficients
    assert np.array_equal(got, ol.product_of_constants(P - 1, h, P - 1, h))
    for la, lb in [(h + 1, h + 1), (2 * h, 2)]:
        with pytest.raises(mf.MfhError) as e:
            ctx.poly_mul(d_top, la, d_top, lb)
        assert _rc(e.value) == MFH_EUNSUPPORTED and "max 2^23" in str(e.value)
    rng = np.random.default_rng(23)
    a, b = _rand(rng, 100), _rand(rng, 37)
    assert np.array_equal(_mul(ctx, a, b), kron.mul(a, b))


def test_prepare_t_at_the_largest_d(gpu_ctx_factory, kron, pool, mf):
    """4 d - deg t <= 2^23: with deg t = d - 1 the largest d is 2 796 202.  d = 2 796 200: a batch of 4 random statements -- the exact path's check fails for
    every one (cyclic products of 2^22 points), the Euclidean path recomputes them (transforms of 2^23) -- each quotient certified."""
    d, nb = 2796200, 4
    c = gpu_ctx_factory(mf.Params(d=d, m=4))
    rng = np.random.default_rng(d)
    t = _rand(rng, d)
    V = np.stack([_rand(rng, d) for _ in range(nb)])
    c.poly_prepare_t(_dev(c, t))
    got = _host(c, c.poly_h_many(_dev(c, V), nb), (nb, d))
    assert c.poly_exact_fallbacks() == nb
    for k, ok in enumerate(pool.map(kron.div_certify, V, [t] * nb, got)):
        assert ok, k
    c.close()


@pytest.mark.parametrize("d,dt", [(2796204, 2796203), ((1 << 21) + 4, 3)])
def test_prepare_t_beyond_the_limit_is_refused(gpu_ctx_factory, mf, d, dt):
    """4 d - deg t > 2^23: MFH_EUNSUPPORTED, not a wrong answer -- and a t prepared before the refused one is not used for the statements behind it"""
    c = gpu_ctx_factory(mf.Params(d=d, m=4))
    rng = np.random.default_rng(dt)
    if d < 2796202:  # a t this context can take: prepared first
        c.poly_prepare_t(_dev(c, _rand(rng, d)))
    t = np.zeros(d, np.uint32)
    t[: dt + 1] = _rand(rng, dt + 1)
    with pytest.raises(mf.MfhError) as e:
        c.poly_prepare_t(_dev(c, t))
    assert _rc(e.value) == MFH_EUNSUPPORTED
    with pytest.raises(mf.MfhError):
        c.poly_h(_dev(c, _rand(rng, d)))
    c.close()


def test_poly_h_many_at_the_largest_batch(gpu_ctx_factory, oracle, kron, pool, mf):
    """nb <= kMaxBatch = 21845 (grid.y = 3 nb <= 65535): a full batch at d = 256 with a non-dividing statement in the last position is exact; 21846 is refused"""
    d, nb = 256, 21845
    rng = np.random.default_rng(nb)
    p, t, v_ok = _ssp(oracle, mf, d, 8, rng)
    V = _valid(v_ok, t, rng.integers(0, P, size=nb, dtype=np.uint64))
    V[-1, 100] = (V[-1, 100] + 1) % P
    c = gpu_ctx_factory(p)
    c.poly_prepare_t(_dev(c, t))
    d_v = _dev(c, V)
    got = _host(c, c.poly_h_many(d_v, nb), (nb, d))
    assert c.poly_exact_fallbacks() == 1
    bad = [k for k, ok in enumerate(pool.map(kron.div_certify, V, [t] * nb, got, chunksize=256)) if not ok]
    assert bad == []
    with pytest.raises(mf.MfhError) as e:
        c.poly_h_many(d_v, nb + 1)
    assert _rc(e.value) == MFH_EINVAL
    c.close()


# ------------------------------------------------------------------ c. the exact-division path at every seam shape and beyond
def _ssp(oracle, mf, d, m, rng):
    """a valid SSP: t, and the v of its witness (t | v^2 - 1)"""
    p = mf.Params(d=d, m=m)
    bits = rng.integers(0, 256, size=(m + 7) // 8, dtype=np.uint8).tobytes()
    ssp = oracle.ssp_from_tape(p, rng.integers(0, 256, size=m * 8 * d, dtype=np.uint8), bits).reshape(m + 3, d)
    t, v = ssp[0].copy(), ssp[1].copy()
    for i in range(1, m):
        if (bits[(i - 1) >> 3] >> ((i - 1) & 7)) & 1:
            v = (v + ssp[i + 1]) % np.uint64(P)
    assert t[-1] != 0  # deg t = d - 1: the GPU's d coefficients are the whole quotient
    return p, t.astype(np.uint32), v.astype(np.uint32)


def _valid(v_ok, t, deltas):
    """v_ok + delta t: (v + delta t)^2 - 1 = v^2 - 1 + t (2 delta v + delta^2 t), still divisible by t"""
    return ((v_ok.astype(np.uint64)[None, :] + deltas.astype(np.uint64)[:, None] * t.astype(np.uint64)[None, :] % np.uint64(P)) % np.uint64(P)).astype(np.uint32)


class _Quotients:
    """the first quotient of each statement is certified (on the pool); every later one must equal it"""

    def __init__(self, kron, pool, t):
        self.kron, self.pool, self.t = kron, pool, t
        self.first, self.jobs = {}, []

    def check(self, sid, v, h, where):
        if sid in self.first:
            assert np.array_equal(h, self.first[sid]), f"statement {sid}, {where}: differs from its earlier quotient"
        else:
            self.first[sid] = h.copy()
            self.jobs.append((sid, where, self.pool.submit(self.kron.div_certify, v, self.t, self.first[sid])))

    def finish(self):
        for sid, where, fut in self.jobs:
            assert fut.result(), f"statement {sid}, {where}: not the Euclidean quotient"


@pytest.mark.parametrize("d", [4100, 8192, 12288, 32768, 40000, 65536, 1 << 17, 1 << 20])
def test_exact_path_at_every_seam_shape(gpu_ctx_factory, oracle, kron, pool, mf, d):
    """k_exact_seam<K>, K = logNc - 11: d = 4100 (K = 2, d not a power of two), 8192 (2), 12288 (3), 32768 (4, the default size), 40000 and 65536 (5); then the
    generic cyclic products at 2^17 and 2^20.  Batches of 6 with non-dividing statements at position 0, at nb - 1, at two adjacent positions, everywhere and
    everywhere but one, in modes 0 (Euclidean only), 1 (backs off after a failed check) and 2 (always tries): every quotient certified, the fallbacks counted."""
    nb = 6
    rng = np.random.default_rng(d + 31)
    p, t, v_ok = _ssp(oracle, mf, d, 3, rng)
    good = _valid(v_ok, t, rng.integers(0, P, size=nb, dtype=np.uint64))
    bad = good.copy()
    for i in range(nb):
        j = (d // 3 + 17 * i) % d
        bad[i, j] = (int(bad[i, j]) + 1) % P
    bad[0] = _rand(rng, d)
    c = gpu_ctx_factory(p)
    c.poly_prepare_t(_dev(c, t))
    assert c.poly_exact_fallbacks() == 0  # the exact path exists for this t
    layouts = [set(), {0}, {nb - 1}, {2, 3}, set(range(nb)), set(range(nb)) - {1}]
    qs = _Quotients(kron, pool, t)
    for mode in (0, 1, 2):
        c.set_poly_exact(mode)
        failed_before = False
        for badpos in layouts:
            V = np.stack([bad[i] if i in badpos else good[i] for i in range(nb)])
            got = _host(c, c.poly_h_many(_dev(c, V), nb), (nb, d))
            fb = c.poly_exact_fallbacks()
            tried = mode == 2 or (mode == 1 and not failed_before)
            assert fb == (len(badpos) if tried else 0), f"mode {mode}, non-dividing at {sorted(badpos)}"
            failed_before |= bool(badpos)
            for i in range(nb):
                qs.check(i + nb * (i in badpos), V[i], got[i], f"mode {mode}, non-dividing at {sorted(badpos)}, position {i}")
    qs.finish()
    c.close()


def test_exact_path_super_group_of_255(gpu_ctx_factory, oracle, kron, pool, mf):
    """the shape the headline runs: 255 statements (snark.hip's super-group) at d = 32768, k_exact_seam<4>; then the same with the last one non-dividing"""
    d, nb = 32768, 255
    rng = np.random.default_rng(255)
    p, t, v_ok = _ssp(oracle, mf, d, 3, rng)
    V = _valid(v_ok, t, rng.integers(0, P, size=nb, dtype=np.uint64))
    c = gpu_ctx_factory(p)
    c.poly_prepare_t(_dev(c, t))
    c.set_poly_exact(2)
    got = _host(c, c.poly_h_many(_dev(c, V), nb), (nb, d))
    assert c.poly_exact_fallbacks() == 0
    assert [k for k, ok in enumerate(pool.map(kron.div_certify, V, [t] * nb, got)) if not ok] == []
    V[-1, 5] = (V[-1, 5] + 1) % P
    got2 = _host(c, c.poly_h_many(_dev(c, V), nb), (nb, d))
    assert c.poly_exact_fallbacks() == 1
    assert np.array_equal(got2[:-1], got[:-1])
    assert kron.div_certify(V[-1], t, got2[-1])
    c.close()


# ------------------------------------------------------------------ d. the Euclidean path at large d
@pytest.mark.parametrize("d,dt", [(1 << 15, 0), (1 << 15, 1), (1 << 15, (1 << 15) - 6), (1 << 20, 0), (1 << 20, 1), (1 << 20, (1 << 20) - 6)])
def test_euclidean_path_with_a_short_t(gpu_ctx_factory, kron, pool, mf, d, dt):
    """deg t < d - 1: no exact path, and the quotient has more than d coefficients -- the GPU keeps the first d of the whole quotient"""
    nb = 4 if d <= 1 << 15 else 2
    rng = np.random.default_rng(d + dt)
    t = np.zeros(d, np.uint32)
    t[: dt + 1] = _rand(rng, dt + 1)
    V = np.stack([_rand(rng, d) for _ in range(nb)])
    futs = [pool.submit(kron.div, v, t) for v in V]
    c = gpu_ctx_factory(mf.Params(d=d, m=4))
    c.poly_prepare_t(_dev(c, t))
    assert c.poly_exact_fallbacks() == -1
    got = _host(c, c.poly_h_many(_dev(c, V), nb), (nb, d))
    assert np.array_equal(_host(c, c.poly_h(_dev(c, V[-1]))), got[-1])
    for k, fut in enumerate(futs):
        assert np.array_equal(got[k], fut.result()[:d]), k
    c.close()


def test_euclidean_path_at_2_20_random_statements(gpu_ctx_factory, kron, pool, mf):
    """d = 2^20 (configs 4 / 5), dense t, statements that do not divide: one alone (Euclidean path) and four in a batch (exact path, its check fails for all)"""
    d, nb = 1 << 20, 4
    rng = np.random.default_rng(20)
    t = _rand(rng, d)
    V = np.stack([_rand(rng, d) for _ in range(nb)])
    c = gpu_ctx_factory(mf.Params(d=d, m=4))
    c.poly_prepare_t(_dev(c, t))
    one = _host(c, c.poly_h(_dev(c, V[2])))
    got = _host(c, c.poly_h_many(_dev(c, V), nb), (nb, d))
    assert c.poly_exact_fallbacks() == nb
    assert np.array_equal(one, got[2])
    for k, ok in enumerate(pool.map(kron.div_certify, V, [t] * nb, got)):
        assert ok, k
    c.close()


# ------------------------------------------------------------------ e. mfh_poly_add
def test_poly_add_near_p(ctx):
    n = 1000  # not a multiple of 256
    rng = np.random.default_rng(1000)
    a = (P - 1 - rng.integers(0, 4, size=n, dtype=np.uint64)).astype(np.uint32)
    b = (P - 1 - rng.integers(0, 4, size=n, dtype=np.uint64)).astype(np.uint32)
    a[:4], b[:4] = [P - 1, P - 1, 0, 1], [P - 1, 1, 0, P - 1]
    got = _host(ctx, ctx.poly_add(_dev(ctx, a), _dev(ctx, b), n))
    assert np.array_equal(got, ((a.astype(np.uint64) + b) % P).astype(np.uint32))


# ------------------------------------------------------------------ f. the prepared t across other calls
def test_growing_poly_mul_after_prepare_t(gpu_ctx_factory, oracle, kron, mf):
    """mfh_poly_mul longer than the prepared transforms rebuilds the NTT state (and with it the prepared t and the exact path): a poly_h behind it equals the
    reference or raises -- it never divides by something else.  Preparing t again restores both paths."""
    d, nb = 256, 6
    rng = np.random.default_rng(4096)
    p, t, v_ok = _ssp(oracle, mf, d, 8, rng)
    V = _valid(v_ok, t, rng.integers(0, P, size=nb, dtype=np.uint64))
    exp = np.stack([kron.div(v, t)[:d] for v in V])
    c = gpu_ctx_factory(p)
    c.set_poly_exact(2)
    c.poly_prepare_t(_dev(c, t))
    d_v = _dev(c, V)
    assert np.array_equal(_host(c, c.poly_h_many(d_v, nb), (nb, d)), exp)
    a, b = _rand(rng, 3000), _rand(rng, 1097)  # 4096 coefficients: a longer transform than t's preparation made
    assert np.array_equal(_mul(c, a, b), kron.mul(a, b))
    for call in (lambda: _host(c, c.poly_h(d_v)), lambda: _host(c, c.poly_h_many(d_v, nb), (nb, d))[0]):
        try:
            h = call()
        except mf.MfhError:
            continue
        assert np.array_equal(h, exp[0])
    c.poly_prepare_t(_dev(c, t))
    assert np.array_equal(_host(c, c.poly_h_many(d_v, nb), (nb, d)), exp)
    assert c.poly_exact_fallbacks() == 0
    c.close()


def test_prepared_t_across_preparations_in_one_context(gpu_ctx_factory, oracle, kron, mf):
    """The per-SSP buffers of a context only grow, so a preparation finds the buffers of the one before it: nothing of an earlier t may be read.  d = 4100 is the
    smallest shape that takes the fused seam (logNc = 13, K = 2).  A poly_mul of 2^15 coefficients comes first: it sizes the NTT tables for all that follows (the
    degree-3 t needs 2^15, the dense ones 2^14), so no preparation rebuilds the state and the buffers do carry over.  Then a dense t; a t of degree 3 (no exact path,
    a longer quotient and G; the transform of t^-1 and the check powers of step 1 stay behind, unused); another dense t, which writes its own over them and feeds them
    to k_exact_seam / k_exact_check; and a fourth, dense again, over step 3's -- every quotient against GMP's division."""
    d, nb = 4100, 6
    rng = np.random.default_rng(4100)
    p = mf.Params(d=d, m=3)
    c = gpu_ctx_factory(p)
    c.set_poly_exact(2)
    a, b = _rand(rng, 1 << 14), _rand(rng, (1 << 14) + 1)
    assert np.array_equal(_mul(c, a, b), kron.mul(a, b))
    points = []
    for step, seed in ((1, 11), (2, None), (3, 33), (4, 44)):
        if seed is None:  # step 2: deg t = 3, statements that do not divide
            t = np.zeros(d, np.uint32)
            t[:4] = _rand(rng, 4)
            V = np.stack([_rand(rng, d) for _ in range(nb)])
        else:
            _, t, v_ok = _ssp(oracle, mf, d, 3, np.random.default_rng(seed))
            V = _valid(v_ok, t, rng.integers(0, P, size=nb, dtype=np.uint64))
        exp = np.stack([kron.div(v, t)[:d] for v in V])
        c.poly_prepare_t(_dev(c, t))
        assert c.poly_exact_fallbacks() == (-1 if seed is None else 0), step
        assert np.array_equal(_host(c, c.poly_h_many(_dev(c, V), nb), (nb, d)), exp), step
        assert np.array_equal(_host(c, c.poly_h(_dev(c, V[-1]))), exp[-1]), step
        assert c.poly_exact_fallbacks() == (-1 if seed is None else 0), step
        if seed is not None:
            points.append(c.exact_points())
    assert points[0] != points[1] and points[1] != points[2]  # drawn per preparation
    c.close()


def test_poly_h_after_a_refused_prepare_t_raises(gpu_ctx_factory, oracle, mf):
    """a prepare_t that fails (t = 0) leaves no t behind: the statements after it are refused, not divided by the t prepared before"""
    p = mf.DEBUG
    c = gpu_ctx_factory(p)
    rng = np.random.default_rng(0)
    t = _rand(rng, p.d)
    v = _rand(rng, p.d)
    c.poly_prepare_t(_dev(c, t))
    assert np.array_equal(_host(c, c.poly_h(_dev(c, v))).astype(np.uint64), oracle.poly_h(v, t))
    with pytest.raises(mf.MfhError):
        c.poly_prepare_t(c.zeros(p.d * 4))
    with pytest.raises(mf.MfhError):
        c.poly_h(_dev(c, v))
    with pytest.raises(mf.MfhError):
        c.poly_h_many(_dev(c, np.stack([v] * 4)), 4)
    assert c.poly_exact_fallbacks() == -1
    c.close()
