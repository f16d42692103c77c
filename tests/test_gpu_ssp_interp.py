"""GPU: mfh_ssp_from_rows -- a constraint system given row by row, interpolated into the dense device SSP -- and proofs of Boolean circuits through it.

1. the SSP equals the Python-integer restatement (tests/circuit_ref.py) in every coefficient of every slot, on edge cases of the row format;
2. at the default size, t and the rows are checked through evaluations at every point (t and the witness polynomial);
3.-6. circuits end to end: proofs equal the oracle's prover on the exported SSP, honest statements verify and violating ones do not, the exact-division path
   takes every satisfying statement, public inputs bind the statement, and recompiling into the same buffer is seen by the batch prover;
7. invalid rows are refused with MFH_EINVAL before anything is written."""
import numpy as np
import pytest

import circuit_ref as cr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

P = cr.P
SEED = bytes((53 * i + 7) & 0xFF for i in range(40))


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def C():
    from c_lwe_snarks_amd import circuit

    return circuit


def _csr(rows):
    lens = [len(r) for r in rows]
    rp = np.zeros(len(rows) + 1, dtype=np.uint32)
    np.cumsum(lens, out=rp[1:])
    w = np.array([x for r in rows for x, _ in r], dtype=np.uint32)
    c = np.array([a for r in rows for _, a in r], dtype=np.uint32)
    return rp, w, c


def _random_rows(rng, p, nrows, per_row=4, dense_wire=None, empty_every=0, extreme=False, dup=False):
    rows = []
    for j in range(nrows):
        if empty_every and j % empty_every == 0:
            rows.append([])
            continue
        k = int(rng.integers(1, per_row + 1))
        r = [(int(rng.integers(0, p.m)), int(rng.integers(0, P))) for _ in range(k)]
        if extreme:
            r += [(int(rng.integers(0, p.m)), 0), (int(rng.integers(0, p.m)), P - 1)]
        if dup and r:
            r.append(r[0])
            r.append((r[0][0], P - 1))
        if dense_wire is not None:
            r.append((dense_wire, int(rng.integers(0, P))))
            if dup:
                r.append((dense_wire, int(rng.integers(0, P))))
        rows.append(r)
    return _csr(rows)


def _bits_of(rng, p):
    return rng.bytes((p.m + 7) // 8)


# ------------------------------------------------------------------ 1. every coefficient of every slot
CASES = {
    "nrows0": dict(nrows=0),
    "full": dict(nrows=255),
    "empty_rows": dict(nrows=200, empty_every=3),
    "extremes": dict(nrows=180, extreme=True),
    "duplicates": dict(nrows=150, dup=True),
    "dense_wire": dict(nrows=255, dense_wire=5, dup=True),  # 510 entries on one wire: a column cut into parts
    "dense_v0": dict(nrows=120, dense_wire=0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_equals_python_reference_debug(gpu_ctx_factory, mf, case):
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(sorted(CASES).index(case) + 1)
    kw = dict(CASES[case])
    rows = _random_rows(rng, p, kw.pop("nrows"), **kw)
    d_ssp = ctx.zeros((p.m + 3) * p.d * 4) - 1  # (every word written: no slot may keep this)
    ctx.ssp_from_rows(rows, d_ssp)
    got = ctx.ssp_to_host_u64(d_ssp).reshape(p.m + 3, p.d)
    exp = cr.ssp(p.d, p.m, rows)
    for i in range(p.m + 3):
        assert np.array_equal(got[i], exp[i]), f"slot {i}"


@pytest.mark.parametrize("d,m", [(130, 24), (192, 40), (64, 16)])
def test_equals_python_reference_odd_shapes(gpu_ctx_factory, mf, d, m):
    """d not a power of two (padding factors in the product tree), d % 4 != 0 (word stores), and a full row space"""
    p = mf.Params(d=d, m=m)
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(d + m)
    for nrows in (d - 1, d // 3):
        rows = _random_rows(rng, p, nrows, dense_wire=0, dup=True)
        got = ctx.ssp_to_host_u64(ctx.ssp_from_rows(rows)).reshape(p.m + 3, p.d)
        assert np.array_equal(got, cr.ssp(p.d, p.m, rows))


# ------------------------------------------------------------------ 2. default size: t and the rows through evaluations
def test_default_size_evaluations(gpu_ctx_factory, mf):
    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(22)
    nrows = 30000
    rp = np.zeros(nrows + 1, dtype=np.uint32)
    k = rng.integers(1, 6, nrows)
    np.cumsum(k + 1, out=rp[1:])
    nnz = int(rp[-1])
    wire = rng.integers(0, p.m, nnz).astype(np.uint32)
    coef = rng.integers(0, P, nnz, dtype=np.uint64).astype(np.uint32)
    wire[rp[1:] - 1] = 17  # one wire in every row (a dense column, cut into parts)
    rows = (rp, wire, coef)
    d_ssp = ctx.ssp_from_rows(rows)
    t = ctx.to_host(d_ssp[: p.d * 4], np.uint32).astype(np.uint64)
    assert t[p.d - 1] == 1
    fact = 1
    for i in range(2, p.d + 1):
        fact = fact * i % P
    assert int(t[0]) == (P - fact) % P  # (-1)^(d-1) d!, d - 1 odd
    pts = np.arange(p.d - 1, dtype=np.uint64) + 2
    assert not cr.horner(t, pts).any()
    tail = ctx.to_host(d_ssp[(p.m + 1) * p.d * 4:(p.m + 3) * p.d * 4], np.uint32)
    assert not tail.any()
    v0 = ctx.to_host(d_ssp[p.d * 4: 2 * p.d * 4], np.uint32).astype(np.uint64)
    rowid = np.repeat(np.arange(nrows), np.diff(rp.astype(np.int64)))
    for b in range(2):
        bits = _bits_of(rng, p)
        w = ctx.to_host(ctx.witness_poly(d_ssp, bits, 0), np.uint32).astype(np.uint64)
        got = cr.horner((w + v0) % P, pts)
        sel = np.array([(bits[(x - 1) >> 3] >> ((x - 1) & 7)) & 1 if x else 1 for x in range(p.m)], dtype=bool)
        take = sel[wire]
        exp = np.zeros(p.d - 1, dtype=object)
        exp[nrows:] = 1
        np.add.at(exp, rowid[take], coef[take].astype(object))
        exp = np.array([int(x) % P for x in exp], dtype=np.uint64)
        assert np.array_equal(got, exp), b


# ------------------------------------------------------------------ circuits
def _draws(rng, nb):
    deltas = [int(x) for x in rng.integers(0, P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    return deltas, mags, signs


def _keys(ctx, rng, p):
    alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    err = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    return dict(alpha=alpha, beta=beta, s=s, sk=sk, err=err, d_sk=ctx.to_device(sk), d_err=ctx.to_device(err))


def _random_circuit(C, rng, npub, npriv, ngates):
    c = C.Circuit()
    ws = c.public(npub) + c.private(npriv)
    gates = []
    for _ in range(ngates):
        kind = ("XOR", "AND", "OR", "NOT")[int(rng.integers(0, 4))]
        a, b = (ws[int(rng.integers(0, len(ws)))] for _ in range(2))
        g = c.NOT(a) if kind == "NOT" else getattr(c, kind)(a, b)
        gates.append(g)
        ws.append(g)
    return c, gates


def _flip(bits, w):
    b = bytearray(bits)
    b[(w - 1) >> 3] ^= 1 << ((w - 1) & 7)
    return bytes(b)


def _honest(c, rng, npub, npriv):
    return c.assign([int(x) for x in rng.integers(0, 2, npub)], [int(x) for x in rng.integers(0, 2, npriv)])


# ------------------------------------------------------------------ 3. end to end at the debug size, against the oracle
def test_circuit_end_to_end_debug(gpu_ctx_factory, oracle, mf, C):
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(31)
    c, gates = _random_circuit(C, rng, 3, 12, 40)
    cc = c.compile(p)
    d_ssp = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_prepare(d_ssp)
    assert ctx.poly_exact_fallbacks() == 0  # t has the exact-division path (degree d - 1, a unit modulo x^N - 1)
    ssp = ctx.ssp_to_host_u64(d_ssp)
    K = _keys(ctx, rng, p)
    crs = oracle.setup(p, SEED, ssp, K["alpha"], K["beta"], K["s"], K["sk"], K["err"])
    d_crs = ctx.setup(d_ssp, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"])
    assert np.array_equal(ctx.to_host(d_crs), np.concatenate([crs["s"], crs["as_"], crs["t"], crs["v"][: (p.m - 1) * p.ctb]]))
    nb = 40
    bad_at = {3: 0, 9: 7, 17: 20, 30: 39, 38: 11}  # statement -> the gate whose output is flipped
    stmts = []
    for b in range(nb):
        bits = _honest(c, rng, 3, 12)
        if b in bad_at:
            bits = _flip(bits, cc.wire(gates[bad_at[b]]))
        stmts.append(bits)
        assert cr.satisfied(cc.rows, bits) == (b not in bad_at)
    deltas, mags, signs = _draws(rng, nb)
    for b in (0, 3):  # single prover, bit for bit the oracle's
        tape = b"".join(mags[b][80 * k: 80 * k + 80] + signs[b][k: k + 1] for k in range(5))
        ref = oracle.prover(p, crs, ssp, stmts[b], deltas[b], tape, 80, want_pre=False)
        got = ctx.to_host(ctx.prove(d_crs, d_ssp, stmts[b], deltas[b], mags[b], signs[b]), np.uint64).reshape(5, p.n + 1, p.L)
        assert np.array_equal(got, ref["proof"]), b
    ctx.set_poly_exact(2)  # every batch tries the exact path: the check counts every statement that fails it
    try:
        ctx.poly_exact_fallbacks()
        proofs = ctx.prove_batch(d_crs, d_ssp, stmts, deltas, mags, signs).clone()
        assert ctx.poly_exact_fallbacks() == len(bad_at)
    finally:
        ctx.set_poly_exact(1)
    pv = proofs.view(nb, -1)
    for b in (0, 3, 4, 38):
        tape = b"".join(mags[b][80 * k: 80 * k + 80] + signs[b][k: k + 1] for k in range(5))
        ref = oracle.prover(p, crs, ssp, stmts[b], deltas[b], tape, 80, want_pre=False)
        assert np.array_equal(ctx.to_host(pv[b], np.uint64).reshape(5, p.n + 1, p.L), ref["proof"]), b
        assert torch.equal(pv[b], ctx.prove(d_crs, d_ssp, stmts[b], deltas[b], mags[b], signs[b]))
    ok = ctx.to_host(ctx.verify(d_ssp, K["alpha"], K["beta"], K["s"], K["d_sk"], proofs, nb))
    assert [int(x) for x in ok] == [0 if b in bad_at else 1 for b in range(nb)]
    assert oracle.verifier(p, ssp, K["alpha"], K["beta"], K["s"], K["sk"], ctx.to_host(pv[0], np.uint64).reshape(5, p.n + 1, p.L))


# ------------------------------------------------------------------ 4. public inputs: an adder with a public sum
def _adder(C, nbits):
    c = C.Circuit()
    z = c.public(nbits + 1)
    x = c.private(nbits)
    y = c.private(nbits)
    carry = None
    for i in range(nbits):
        h = c.XOR(x[i], y[i])
        if carry is None:
            s, carry = h, c.AND(x[i], y[i])
        else:
            s = c.XOR(h, carry)
            carry = c.OR(c.AND(x[i], y[i]), c.AND(carry, h))
        c.assert_equal(c.XOR(s, z[i]), 0)
    c.assert_equal(c.XOR(carry, z[nbits]), 0)
    return c


def _bits(v, n):
    return [(v >> i) & 1 for i in range(n)]


def _clear_low(bits, lu):
    b = bytearray(bits)
    for i in range(lu):
        b[i >> 3] &= ~(1 << (i & 7)) & 0xFF
    return bytes(b)


def test_adder_with_public_sum(gpu_ctx_factory, mf, C):
    import torch

    p = mf.DEBUG
    nbits = 4
    c = _adder(C, nbits)
    cc = c.compile(p)
    lu = cc.lu
    assert lu == nbits + 1
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(44)
    d_ssp = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_prepare(d_ssp)
    K = _keys(ctx, rng, p)
    d_crs = ctx.setup_public(d_ssp, K["alpha"], K["beta"], K["s"], lu, K["d_sk"], K["d_err"])
    nb = 24
    xs = [(int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in range(nb)]
    stmts = [c.assign(_bits(x + y, nbits + 1), _bits(x, nbits) + _bits(y, nbits)) for x, y in xs]
    for b in range(nb):
        assert cr.satisfied(cc.rows, stmts[b])
    deltas, mags, signs = _draws(rng, nb)
    proofs = ctx.prove_batch_public(d_crs, d_ssp, lu, stmts, deltas, mags, signs).clone()
    vk = ctx.derive_vk(d_ssp, K["s"], lu)
    right = [c.statement(_bits(x + y, nbits + 1)) for x, y in xs]
    wrong = [c.statement(_bits((x + y + 1) % 32, nbits + 1)) for x, y in xs]
    assert int(ctx.verify_public(vk, lu, K["alpha"], K["beta"], K["d_sk"], proofs, right).sum()) == nb
    assert int(ctx.verify_public(vk, lu, K["alpha"], K["beta"], K["d_sk"], proofs, wrong).sum()) == 0
    # the composition identity of test_gpu_public_inputs.py on the circuit SSP: (h, hat_h, hat_v) of prove(u || w), (v_w, b_w) of prove(0^lu || w)
    pv = proofs.view(nb, -1)
    for b in (0, 5, nb - 1):
        full = ctx.prove(d_crs, d_ssp, stmts[b], deltas[b], mags[b], signs[b]).clone().view(5, -1)
        zero = ctx.prove(d_crs, d_ssp, _clear_low(stmts[b], lu), deltas[b], mags[b], signs[b]).clone().view(5, -1)
        exp = torch.cat([full[:3], zero[3:]]).reshape(-1)
        assert torch.equal(pv[b], exp), b
        assert torch.equal(ctx.prove_public(d_crs, d_ssp, lu, stmts[b], deltas[b], mags[b], signs[b]), exp)


# ------------------------------------------------------------------ 5. default size: a circuit filling most of the row space, 255 statements
def test_default_size_circuit_batch(gpu_ctx_factory, mf, C):
    p = mf.DEFAULT
    rng = np.random.default_rng(55)
    npub, npriv, ngates = 16, 3000, 13500
    c, _ = _random_circuit(C, rng, npub, npriv, ngates)
    cc = c.compile(p)
    assert cc.nrows == npub + npriv + 2 * ngates and cc.nrows > 0.9 * (p.d - 1)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    d_ssp = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_prepare(d_ssp)
    K = _keys(ctx, rng, p)
    d_crs = ctx.setup(d_ssp, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"])
    nb = 255
    stmts = [_honest(c, rng, npub, npriv) for _ in range(nb)]
    assert len(set(stmts)) == nb
    deltas, mags, signs = _draws(rng, nb)
    ctx.set_poly_exact(2)
    try:
        ctx.poly_exact_fallbacks()
        proofs = ctx.prove_batch(d_crs, d_ssp, stmts, deltas, mags, signs)
        assert ctx.poly_exact_fallbacks() == 0
    finally:
        ctx.set_poly_exact(1)
    assert int(ctx.verify(d_ssp, K["alpha"], K["beta"], K["s"], K["d_sk"], proofs, nb).sum()) == nb


# ------------------------------------------------------------------ 6. recompiling into the same buffer is what the next batch proves
def test_recompile_into_the_same_buffer(gpu_ctx_factory, mf, C):
    """the batch prover keeps an MFMA-fragment image of the SSP, keyed by d_ssp: a second circuit written into the same buffer must drop it.  t depends on d
    alone, so the prepared t stays right and ssp_prepare is NOT called again -- only mfh_ssp_from_rows can tell the prover that the SSP changed"""
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(66)
    K = _keys(ctx, rng, p)
    d_ssp = ctx.zeros((p.m + 3) * p.d * 4)
    nb = 20
    for k in range(2):
        c, _ = _random_circuit(C, rng, 2, 10 + 5 * k, 30 + 7 * k)
        cc = c.compile(p)
        ctx.ssp_from_rows(cc.rows, d_ssp)
        if k == 0:
            ctx.ssp_prepare(d_ssp)
        d_crs = ctx.setup(d_ssp, K["alpha"], K["beta"], K["s"], K["d_sk"], K["d_err"])
        stmts = [_honest(c, rng, 2, 10 + 5 * k) for _ in range(nb)]
        deltas, mags, signs = _draws(rng, nb)
        proofs = ctx.prove_batch(d_crs, d_ssp, stmts, deltas, mags, signs).clone()
        assert int(ctx.verify(d_ssp, K["alpha"], K["beta"], K["s"], K["d_sk"], proofs, nb).sum()) == nb, k
        for b in (0, nb - 1):
            assert torch.equal(proofs.view(nb, -1)[b], ctx.prove(d_crs, d_ssp, stmts[b], deltas[b], mags[b], signs[b])), (k, b)


# ------------------------------------------------------------------ 7. invalid rows
def test_invalid_rows_are_einval_and_write_nothing(gpu_ctx_factory, mf):
    import ctypes

    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    d_ssp = ctx.zeros((p.m + 3) * p.d * 4) + 0x5A
    before = d_ssp.clone()
    good = _csr([[(0, 1), (3, 2)], [(1, P - 1)]])

    def call(rp, w, c):
        rp, w, c = (np.ascontiguousarray(a, dtype=np.uint32) for a in (rp, w, c))
        return ctx.lib.mfh_ssp_from_rows(ctx._h, len(rp) - 1, ctypes.c_void_p(rp.ctypes.data), ctypes.c_void_p(w.ctypes.data),
                                         ctypes.c_void_p(c.ctypes.data), mf._ptr(d_ssp))

    bad = {
        "nrows > d - 1": (np.zeros(p.d + 1), [0], [1]),
        "wire >= m": (good[0], [0, p.m, 1], good[2]),
        "coefficient >= p": (good[0], good[1], [1, P, 2]),
        "coefficient 2^32 - 1": (good[0], good[1], [0xFFFFFFFF, 2, 2]),
        "row_ptr decreases": ([0, 2, 1], good[1], good[2]),
    }
    for name, args in bad.items():
        assert call(*args) == -1, name  # MFH_EINVAL
        ctx.sync()
        assert torch.equal(d_ssp, before), name
    with pytest.raises(mf.MfhError):
        ctx.ssp_from_rows((np.array([0, 1], dtype=np.uint32), np.array([p.m], dtype=np.uint32), np.array([1], dtype=np.uint32)), d_ssp)
    assert call(np.zeros(p.d), [], []) == 0  # nrows = d - 1 empty rows is fine
