"""GPU: the row SSP (mfh_ssp_set_rows) -- a constraint system registered as its rows and interpolated per statement by the subproduct tree of t.

Every result is compared with the dense SSP that mfh_ssp_from_rows writes from the same rows (the interpolant is unique, so they agree bit for bit),
or with the Python-integer restatement (tests/circuit_ref.py):
1. every slot (ssp_rows_fill); 2. witness polynomials of random bits; 3. setup messages, vk and verify, also at s = a point; 4. default-size batches,
public inputs on both sides of the second-pass split, violating statements; 5. d = 2^20, where the dense SSP cannot exist; 6. errors and registration."""
import numpy as np
import pytest

import circuit_ref as cr
from test_gpu_ssp_interp import CASES, SEED, _draws, _flip, _honest, _keys, _random_circuit, _random_rows

pytestmark = pytest.mark.gpu

P = cr.P
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def C():
    from c_lwe_snarks_amd import circuit

    return circuit


def _fill_all(ctx, p):
    return ctx.to_host(ctx.ssp_rows_fill(0, p.m + 3), np.uint32).reshape(p.m + 3, p.d)


# ------------------------------------------------------------------ 1. every slot
@pytest.mark.parametrize("case", sorted(CASES))
def test_fill_equals_python_reference_debug(gpu_ctx_factory, mf, case):
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(sorted(CASES).index(case) + 1)
    kw = dict(CASES[case])
    rows = _random_rows(rng, p, kw.pop("nrows"), **kw)
    ctx.ssp_set_rows(rows, lu_max=3)
    assert np.array_equal(_fill_all(ctx, p).astype(np.uint64), cr.ssp(p.d, p.m, rows))


@pytest.mark.parametrize("d,m", [(130, 24), (192, 40), (64, 16), (1152, 1000)])
def test_fill_equals_dense_odd_shapes(gpu_ctx_factory, mf, d, m):
    """x-padding of the tree (d not a power of two), d % 4 != 0, a single bottom node (d = 64), and the bottom / NTT seam"""
    p = mf.Params(d=d, m=m)
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(d + m)
    for nrows in (d - 1, d // 3):
        rows = _random_rows(rng, p, nrows, dense_wire=0, dup=True)
        dense = ctx.to_host(ctx.ssp_from_rows(rows), np.uint32).reshape(p.m + 3, p.d)
        ctx.ssp_set_rows(rows, lu_max=2)
        assert np.array_equal(_fill_all(ctx, p), dense)
    ctx.ssp_set_rows(None)  # frees the tree of t that ssp_from_rows shares: the next call rebuilds it
    assert np.array_equal(ctx.to_host(ctx.ssp_from_rows(rows), np.uint32).reshape(p.m + 3, p.d), dense)


def test_fill_default_size_sample(gpu_ctx_factory, mf):
    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(9)
    rows = _random_rows(rng, p, 30000, per_row=3, dense_wire=7)
    dense = ctx.ssp_from_rows(rows)
    ctx.ssp_set_rows(rows)
    for slot in [0, 1, 8] + [int(x) for x in rng.integers(2, p.m + 1, 5)]:
        got = ctx.to_host(ctx.ssp_rows_fill(slot, 1), np.uint32)
        exp = ctx.to_host(dense[slot * p.d * 4:(slot + 1) * p.d * 4], np.uint32)
        assert np.array_equal(got, exp), slot


# ------------------------------------------------------------------ 2. witness polynomials
@pytest.mark.parametrize("shape", ["debug", "1152", "default"])
def test_witness_poly_equals_dense(gpu_ctx_factory, mf, shape):
    p = {"debug": mf.DEBUG, "1152": mf.Params(d=1152, m=1000), "default": mf.DEFAULT}[shape]
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(len(shape))
    rows = _random_rows(rng, p, min(p.d - 1, 30000), per_row=3)
    dense = ctx.ssp_from_rows(rows)
    ctx.ssp_set_rows(rows)
    for delta in (0, int(rng.integers(1, P)), P - 1):
        bits = rng.bytes((p.m + 7) // 8)  # random bits, not a satisfying assignment
        a = ctx.to_host(ctx.witness_poly(None, bits, delta), np.uint32)
        b = ctx.to_host(ctx.witness_poly(dense, bits, delta), np.uint32)
        assert np.array_equal(a, b), delta


# ------------------------------------------------------------------ 3. setup, vk, verify
def test_setup_equals_dense(gpu_ctx_factory, mf, C):
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(41)
    c, gates = _random_circuit(C, rng, 4, 12, 40)
    cc = c.compile(p)
    dense = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_set_rows(cc.rows, lu_max=4)
    K = _keys(ctx, rng, p)
    nrows = cc.nrows
    for s in (K["s"], 2, p.d, nrows + 1, 0, 1):  # random, r_0, r_{d-2}, r_{nrows-1}, 0, 1
        a = ctx.to_host(ctx.setup_messages(None, K["alpha"], K["beta"], s), np.uint32)
        b = ctx.to_host(ctx.setup_messages(dense, K["alpha"], K["beta"], s), np.uint32)
        assert np.array_equal(a, b), s
        va = ctx.to_host(ctx.derive_vk(None, s, 4), np.uint32)
        vb = ctx.to_host(ctx.derive_vk(dense, s, 4), np.uint32)
        assert np.array_equal(va, vb), s
    ctx.ssp_prepare(None)
    crs_r = ctx.setup(None, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"]).clone()
    crs_d = ctx.setup(dense, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"]).clone()
    assert bool((crs_r == crs_d).all())
    stmts = [_honest(c, rng, 4, 12) for _ in range(4)] + [_flip(_honest(c, rng, 4, 12), cc.wire(gates[-1]))]
    deltas, mags, signs = _draws(rng, 5)
    proofs = ctx.prove_batch(crs_r, None, stmts, deltas, mags, signs).clone()
    ok_r = ctx.to_host(ctx.verify(None, K["alpha"], K["beta"], K["s"], K["d_sk"], proofs, 5), np.uint8)
    ok_d = ctx.to_host(ctx.verify(dense, K["alpha"], K["beta"], K["s"], K["d_sk"], proofs, 5), np.uint8)
    assert list(ok_r) == list(ok_d) == [1, 1, 1, 1, 0]


# ------------------------------------------------------------------ 4. default size: bit-identical batches
def test_default_size_batches_bit_identical(gpu_ctx_factory, mf, C):
    p = mf.DEFAULT
    rng = np.random.default_rng(55)
    npub, npriv, ngates = 100, 3000, 13400
    c, gates = _random_circuit(C, rng, npub, npriv, ngates)
    cc = c.compile(p)
    assert cc.nrows > 0.9 * (p.d - 1)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    dense = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_set_rows(cc.rows, lu_max=100)
    ctx.ssp_prepare(None)
    K = _keys(ctx, rng, p)
    d_crs = ctx.setup(None, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"]).clone()
    nb = 255
    bad = {7, 100, 254}
    stmts = [_honest(c, rng, npub, npriv) for _ in range(nb)]
    for k in bad:
        stmts[k] = _flip(stmts[k], cc.wire(gates[-1 - k]))
    deltas, mags, signs = _draws(rng, nb)
    ctx.poly_exact_fallbacks()
    a = ctx.prove_batch(d_crs, None, stmts, deltas, mags, signs).clone()
    assert ctx.poly_exact_fallbacks() == len(bad)
    b = ctx.prove_batch(d_crs, dense, stmts, deltas, mags, signs).clone()
    assert bool((a == b).all())
    ok = ctx.to_host(ctx.verify(None, K["alpha"], K["beta"], K["s"], K["d_sk"], a, nb), np.uint8)
    assert [k for k in range(nb) if not ok[k]] == sorted(bad)
    sz = 5 * p.ct_limbs * 8  # bytes per proof
    one_r = ctx.prove(d_crs, None, stmts[3], deltas[3], mags[3], signs[3]).clone()
    one_d = ctx.prove(d_crs, dense, stmts[3], deltas[3], mags[3], signs[3]).clone()
    assert bool((one_r == one_d).all()) and bool((one_r == a[3 * sz:4 * sz]).all())  # = the batch's row
    for lu in (16, 100):  # 100 > 64: the statement sum by a second witness pass
        crs = ctx.setup_public(None, K["alpha"], K["beta"], K["s"], lu, K["d_sk"], K["d_err"]).clone()
        pa = ctx.prove_batch_public(crs, None, lu, stmts[:40], deltas[:40], mags[:40], signs[:40]).clone()
        pb = ctx.prove_batch_public(crs, dense, lu, stmts[:40], deltas[:40], mags[:40], signs[:40]).clone()
        assert bool((pa == pb).all()), lu
        sa = ctx.prove_public(crs, None, lu, stmts[5], deltas[5], mags[5], signs[5]).clone()
        sb = ctx.prove_public(crs, dense, lu, stmts[5], deltas[5], mags[5], signs[5]).clone()
        assert bool((sa == sb).all()) and bool((sa == pa[5 * sz:6 * sz]).all()), lu
        vk = ctx.derive_vk(None, K["s"], lu)
        ok = ctx.to_host(ctx.verify_public(vk, lu, K["alpha"], K["beta"], K["d_sk"], pa, stmts[:40]), np.uint8)
        assert [k for k in range(40) if not ok[k]] == [7], lu


# ------------------------------------------------------------------ 5. d = 2^20: the dense SSP cannot be allocated
def test_two_pow_20_interpolation_at_points(gpu_ctx_factory, mf):
    p = mf.Params(d=1 << 20, m=699050)
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(2020)
    nrows = int(0.95 * (p.d - 1))
    k = rng.integers(1, 4, nrows)
    rp = np.zeros(nrows + 1, dtype=np.uint32)
    np.cumsum(k, out=rp[1:])
    nnz = int(rp[-1])
    wire = rng.integers(0, p.m, nnz).astype(np.uint32)
    coef = rng.integers(0, P, nnz, dtype=np.uint64).astype(np.uint32)
    ctx.ssp_set_rows((rp, wire, coef), lu_max=64)
    bits = rng.bytes((p.m + 7) // 8)
    w = ctx.to_host(ctx.witness_poly(None, bits, 0), np.uint32).astype(np.uint64)
    v0 = ctx.to_host(ctx.ssp_rows_fill(1, 1), np.uint32).astype(np.uint64)
    js = np.sort(rng.choice(p.d - 1, 256, replace=False))
    pts = (js + 2).astype(np.uint64)
    gw, gv = cr.horner(w, pts), cr.horner(v0, pts)
    bitarr = np.unpackbits(np.frombuffer(bits, dtype=np.uint8), bitorder="little")
    for q, j in enumerate(js):
        if j >= nrows:
            ew, ev = 0, 1
        else:
            e = slice(int(rp[j]), int(rp[j + 1]))
            ws, cs = wire[e].astype(np.int64), coef[e].astype(object)
            ew = sum(int(c) for x, c in zip(ws, cs) if x >= 1 and bitarr[x - 1]) % P
            ev = sum(int(c) for x, c in zip(ws, cs) if x == 0) % P
        assert int(gw[q]) == ew and int(gv[q]) == ev, j


def test_two_pow_20_circuit_proved_and_verified(gpu_ctx_factory, mf, C):
    """the issue's instance: a Circuit of 64 public inputs, 20 000 private inputs and 470 000 gates at d = 2^20, m = 699 050 (960 064 rows, 91.6 % of
    d - 1), registered as rows -- mfh_ssp_from_rows cannot allocate its 2.9 TB SSP here -- set up with 64 public wires, 6 honest and 2 violating statements
    proved in one batch, the device verifier deciding each"""
    p = mf.Params(d=1 << 20, m=699050)
    rng = np.random.default_rng(2021)
    npub, npriv, ngates = 64, 20000, 470000
    c, gates = _random_circuit(C, rng, npub, npriv, ngates)
    cc = c.compile(p)
    assert cc.nrows == npub + npriv + 2 * ngates and cc.nrows > 0.9 * (p.d - 1)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    ctx.ssp_set_rows(cc.rows, lu_max=64)
    ctx.ssp_prepare(None)
    K = _keys(ctx, rng, p)
    d_crs = ctx.setup_public(None, K["alpha"], K["beta"], K["s"], 64, K["d_sk"], K["d_err"]).clone()
    nb = 8
    stmts = [_honest(c, rng, npub, npriv) for _ in range(nb)]
    bad = [2, 6]
    for k in bad:
        stmts[k] = _flip(stmts[k], cc.wire(gates[-1 - 1000 * k]))
    deltas, mags, signs = _draws(rng, nb)
    ctx.poly_exact_fallbacks()
    proofs = ctx.prove_batch_public(d_crs, None, 64, stmts, deltas, mags, signs).clone()
    assert ctx.poly_exact_fallbacks() == len(bad)
    vk = ctx.derive_vk(None, K["s"], 64)
    ok = ctx.to_host(ctx.verify_public(vk, 64, K["alpha"], K["beta"], K["d_sk"], proofs, stmts), np.uint8)
    assert [k for k in range(nb) if not ok[k]] == bad
    wrong = [_flip(stmts[0], 1)] + stmts[1:]  # honest proof 0 against its statement with public bit 0 flipped
    ok = ctx.to_host(ctx.verify_public(vk, 64, K["alpha"], K["beta"], K["d_sk"], proofs, wrong), np.uint8)
    assert ok[0] == 0 and ok[1] == 1


# ------------------------------------------------------------------ 6. errors and registration
def test_errors_and_registration(gpu_ctx_factory, mf):
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(6)
    rows = _random_rows(rng, p, 200)
    ctx.ssp_set_rows(rows, lu_max=3)
    first = _fill_all(ctx, p)
    rp, w, c = rows
    lib, h = ctx.lib, ctx._h

    def set_rows(rp, w, c, lu_max=0, nrows=None):
        import ctypes

        rp, w, c = (np.ascontiguousarray(a, dtype=np.uint32) for a in (rp, w, c))
        return lib.mfh_ssp_set_rows(h, len(rp) - 1 if nrows is None else nrows, ctypes.c_void_p(rp.ctypes.data), ctypes.c_void_p(w.ctypes.data),
                                    ctypes.c_void_p(c.ctypes.data), lu_max)

    bad_w = w.copy(); bad_w[3] = p.m
    bad_c = c.copy(); bad_c[4] = P
    bad_rp = rp.copy(); bad_rp[10] = bad_rp[11] + 1
    big = np.zeros(p.d + 1, dtype=np.uint32)
    for args in [(rp, bad_w, c), (rp, w, bad_c), (bad_rp, w, c), (big, w, c), (rp, w, c, p.m)]:
        assert set_rows(*args) == EINVAL
        assert np.array_equal(_fill_all(ctx, p), first)  # the previous registration survives
    # lu > lu_max
    bits = rng.bytes((p.m + 7) // 8)
    assert lib.mfh_vk_derive(h, None, 5, 4, mf._ptr(ctx.empty(24))) == EINVAL
    # entry points that do not take the row SSP
    out = torch.empty(p.d, dtype=torch.int64, device=ctx.device)
    assert lib.mfh_witness_lanes(h, None, bits, 0, 1, mf._ptr(out)) == EUNSUPPORTED
    assert lib.mfh_witness_from_lanes(h, None, mf._ptr(out), 0, mf._ptr(ctx.empty(p.d * 4))) == EUNSUPPORTED
    import ctypes

    dl = (ctypes.c_uint32 * 1)(0)
    stride = (p.m + 6) // 8
    assert lib.mfh_witness_poly_mm_cols(h, None, 1, bits, stride, ctypes.cast(dl, ctypes.c_void_p), 0, 128, mf._ptr(ctx.empty(128 * 4)), 128) == EUNSUPPORTED
    with pytest.raises(mf.MfhError, match="error -4"):
        ctx.batch_witness_cols(None, [bits], [0], 0, 128)
    ctx.set_seed(SEED)
    K = _keys(ctx, rng, p)
    d_crs = ctx.setup(None, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"])
    for world in (2, 3):
        with pytest.raises(mf.MfhError, match="error -4"):
            ctx.prove_partial(d_crs, None, bits, 1, 0, world)
    # a dense d_ssp passed explicitly still works
    dense = ctx.ssp_from_rows(rows)
    assert np.array_equal(ctx.to_host(ctx.witness_poly(dense, bits, 3), np.uint32), ctx.to_host(ctx.witness_poly(None, bits, 3), np.uint32))
    # rows -> generator -> rows
    d_t = ctx.ssp_prg_make_t(123, bits)
    ctx.ssp_set_prg(123, d_t)
    assert lib.mfh_ssp_rows_fill(h, 0, 1, mf._ptr(ctx.empty(p.d * 4))) == EINVAL
    prg = ctx.to_host(ctx.witness_poly(None, bits, 0), np.uint32)
    assert not np.array_equal(prg, ctx.to_host(ctx.witness_poly(dense, bits, 0), np.uint32))  # the generator's SSP, not the rows'
    ctx.ssp_set_rows(rows, lu_max=3)
    assert np.array_equal(_fill_all(ctx, p), first)
    ctx.ssp_set_rows(None)
    assert lib.mfh_witness_poly(h, None, bits, 0, mf._ptr(ctx.empty(p.d * 4))) == EINVAL  # nothing registered


def test_unregister_frees_at_default_size(gpu_ctx_factory, mf):
    """at the default size a registration holds the tree of t (7 MB), the prefix (0.6 MB at lu_max = 3), the rows and the scratch: with nothing run in
    between, free device memory before set_rows and after unregistering agrees within 1 MB.  The first registration of the context also sizes the NTT
    tables the polynomial step shares (PolyState, kept by the context): it runs once before the measurement."""
    import torch

    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(61)
    rows = _random_rows(rng, p, 30000, per_row=3)
    ctx.ssp_set_rows(rows, lu_max=3)
    ctx.ssp_set_rows(None)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ctx.ssp_set_rows(rows, lu_max=3)
    torch.cuda.synchronize()
    held = free0 - torch.cuda.mem_get_info()[0]
    assert held > 7 << 20  # (what the check below would miss if it leaked)
    ctx.ssp_set_rows(None)
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) < (1 << 20)
