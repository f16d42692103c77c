"""GPU: mfh_circuit_create / mfh_circuit_assign -- the witnesses of a compiled circuit for a batch of statements, bitsliced on the device.

1. rows equal Circuit.assign byte for byte and holds equals Circuit.holds: random circuits at mf.DEBUG and mf.DEFAULT, batch sizes around the 32-statement
   block and past one launch's chunk, lu = 0, no gates, gates whose two operands are one wire, rows wider than the witness (zero padding);
2. a 5 000-gate chain (depth 5 000) in one call;
3. the largest circuit at mf.DEFAULT (nin + ngates = m - 1) and at the LDS budget (MFH_CIRCUIT_MAX_WIRES) is accepted and evaluated; one wire more is MFH_EINVAL;
4. every MFH_EINVAL case of create / assign;
5. end to end at the default size: proofs from circuit_assign's witnesses are bit-identical to proofs from Circuit.assign's, holds flags exactly the
   violating statements, the honest statements verify, and an all-honest batch takes the exact-division path with no fallback."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from circuit_program_ref import bitsliced, random_circuit

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFB
SEED = bytes((29 * i + 3) & 0xFF for i in range(40))
EINVAL = -1
MAX_WIRES = 32767  # MFH_CIRCUIT_MAX_WIRES


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def C():
    from c_lwe_snarks_amd import circuit

    return circuit


def _inputs(rng, nb, nin):
    return rng.integers(0, 2, size=(nb, nin), dtype=np.uint8)


def _check(c, cc, bits, witness, holds, m):
    npub = cc.lu
    assert witness.shape == (len(bits), (m + 7) // 8) and witness.dtype == np.uint8
    assert holds.shape == (len(bits),) and holds.dtype == bool
    for b in range(len(bits)):
        pub, priv = bits[b, :npub].tolist(), bits[b, npub:].tolist()
        assert witness[b].tobytes() == c.assign(pub, priv), b
        assert bool(holds[b]) == c.holds(pub, priv), b


# ------------------------------------------------------------------ 1. equal to Circuit.assign / holds
@pytest.mark.parametrize("nb", [1, 31, 32, 33, 255, 1020, 8200])
def test_random_circuit_debug(gpu_ctx_factory, mf, nb):
    p = mf.DEBUG
    rng = np.random.default_rng(nb)
    c = random_circuit(rng, 3, 12, 45, nasserts=3, interleave=True)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    prog = ctx.circuit_load(cc)
    bits = _inputs(rng, nb, 15)
    witness, holds = ctx.circuit_assign(prog, bits)
    _check(c, cc, bits, witness, holds, p.m)
    prog.close()


@pytest.mark.parametrize("nb", [33, 1020])
def test_random_circuit_default(gpu_ctx_factory, mf, nb):
    p = mf.DEFAULT
    rng = np.random.default_rng(100 + nb)
    c = random_circuit(rng, 16, 500, 3000, nasserts=4, interleave=True)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    prog = ctx.circuit_load(cc)
    bits = _inputs(rng, nb, 516)
    witness, holds = ctx.circuit_assign(prog, bits)
    _check(c, cc, bits, witness, holds, p.m)
    prog.close()


def test_lu_zero(gpu_ctx_factory, mf):
    p = mf.DEBUG
    rng = np.random.default_rng(7)
    c = random_circuit(rng, 0, 20, 40, nasserts=2)
    cc = c.compile(p)
    assert cc.lu == 0
    ctx = gpu_ctx_factory(p)
    bits = _inputs(rng, 70, 20)
    witness, holds = ctx.circuit_assign(ctx.circuit_load(cc), bits)
    _check(c, cc, bits, witness, holds, p.m)


def test_no_gates(gpu_ctx_factory, mf, C):
    p = mf.DEBUG
    c = C.Circuit()
    u = c.public(5)
    x = c.private(30)
    c.assert_equal(u[1], 1)
    c.assert_equal(x[7], 0)
    cc = c.compile(p)
    assert len(cc.gates) == 0
    ctx = gpu_ctx_factory(p)
    bits = _inputs(np.random.default_rng(8), 100, 35)
    witness, holds = ctx.circuit_assign(ctx.circuit_load(cc), bits)
    _check(c, cc, bits, witness, holds, p.m)
    # and no assertion at all: every statement holds
    c2 = C.Circuit()
    c2.private(9)
    cc2 = c2.compile(p)
    w2, h2 = ctx.circuit_assign(ctx.circuit_load(cc2), bits[:40, :9])
    assert h2.all()
    _check(c2, cc2, bits[:40, :9], w2, h2, p.m)


def test_same_operand_gates(gpu_ctx_factory, mf, C):
    p = mf.DEBUG
    c = C.Circuit()
    x = c.private(4)
    y = [c.XOR(x[0], x[0]), c.AND(x[1], x[1]), c.OR(x[2], x[2]), c.NOT(x[3])]
    z = [c.XOR(y[1], y[1]), c.AND(y[3], y[3]), c.OR(y[0], y[0])]
    c.assert_equal(c.XOR(z[1], z[1]), 0)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    bits = np.array([[(i >> k) & 1 for k in range(4)] for i in range(16)] * 3, dtype=np.uint8)
    witness, holds = ctx.circuit_assign(ctx.circuit_load(cc), bits)
    _check(c, cc, bits, witness, holds, p.m)
    assert holds.all()


def test_wider_rows_are_zero_padded(gpu_ctx_factory, mf, C):
    """the C call with bits_stride beyond the witness: every byte of every row is written, the bits past nin + ngates zero"""
    p = mf.DEBUG
    rng = np.random.default_rng(12)
    c = random_circuit(rng, 2, 10, 30, nasserts=1)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    prog = ctx.circuit_load(cc)
    nb, istride, ostride = 45, 7, 13  # odd strides: unaligned rows
    bits = _inputs(rng, nb, 12)
    inp = np.zeros((nb, istride), dtype=np.uint8)
    inp[:, :2] = np.packbits(bits, axis=1, bitorder="little")
    inp[:, 1] |= 0xF0  # input bits >= nin are ignored
    inp[:, 2:] = 0xA5
    out = np.full((nb, ostride), 0xFF, dtype=np.uint8)
    holds = np.full(nb, 7, dtype=np.uint8)
    rc = ctx.lib.mfh_circuit_assign(ctx._h, prog._h, nb, ctypes.c_void_p(inp.ctypes.data), istride, ctypes.c_void_p(out.ctypes.data), ostride,
                                    ctypes.c_void_p(holds.ctypes.data))
    assert rc == 0
    for b in range(nb):
        pub, priv = bits[b, :2].tolist(), bits[b, 2:].tolist()
        ref = c.assign(pub, priv)
        assert out[b, :8].tobytes() == ref and not out[b, 8:].any(), b
        assert holds[b] == int(c.holds(pub, priv))


# ------------------------------------------------------------------ 2. depth 5 000
def test_chain_of_5000_gates(gpu_ctx_factory, mf, C):
    p = mf.DEFAULT
    c = C.Circuit()
    x = c.private(64)
    g = x[0]
    for k in range(5000):
        op = k % 4
        g = (c.XOR, c.AND, c.OR)[op](g, x[(k + 1) % 64]) if op < 3 else c.NOT(g)
    c.assert_equal(g, 1)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    prog = ctx.circuit_load(cc)
    bits = _inputs(np.random.default_rng(5), 70, 64)
    witness, holds = ctx.circuit_assign(prog, bits)
    _check(c, cc, bits, witness, holds, p.m)


# ------------------------------------------------------------------ 3. the size limits
def _program(rng, nin, ngates, nasserts=8):
    gates = np.zeros((ngates, 3), dtype=np.uint32)
    for g in range(ngates):
        hi = nin + g  # operands in [1, nin + g]; mostly recent wires, so that the circuit is deep as well as wide
        lo = max(1, hi - 200) if g % 3 else 1
        a, b = (int(v) for v in rng.integers(lo, hi + 1, size=2))
        op = int(rng.integers(0, 4))
        gates[g] = (op, a, a if op == 3 else b)
    asserts = np.array([(int(rng.integers(1, nin + ngates + 1)), int(rng.integers(0, 2))) for _ in range(nasserts)], dtype=np.uint32).reshape(-1, 2)
    return SimpleNamespace(gates=gates, asserts=asserts, nwires=nin + ngates)


def _check_program(ctx, desc, m, nb, rng):
    nin = desc.nwires - len(desc.gates)
    prog = ctx.circuit_load(desc)
    bits = _inputs(rng, nb, nin)
    witness, holds = ctx.circuit_assign(prog, bits)
    ref_w, ref_h = bitsliced(desc, bits, m)
    assert np.array_equal(witness, ref_w)
    assert np.array_equal(holds, ref_h)
    prog.close()


def test_largest_circuit_at_default_size(gpu_ctx_factory, mf):
    p = mf.DEFAULT
    rng = np.random.default_rng(21)
    ctx = gpu_ctx_factory(p)
    nin = 844
    desc = _program(rng, nin, p.m - 1 - nin)
    assert desc.nwires == p.m - 1
    _check_program(ctx, desc, p.m, 40, rng)
    over = _program(rng, nin + 1, p.m - 1 - nin)
    with pytest.raises(mf.MfhError, match="m - 1"):
        ctx.circuit_load(over)


def test_lds_budget(gpu_ctx_factory, mf):
    """with m - 1 above the LDS budget, MFH_CIRCUIT_MAX_WIRES wires are accepted and one more is not"""
    p = mf.Params(d=256, m=40000)
    rng = np.random.default_rng(22)
    ctx = gpu_ctx_factory(p)
    desc = _program(rng, 767, MAX_WIRES - 767)
    assert desc.nwires == MAX_WIRES
    _check_program(ctx, desc, p.m, 33, rng)
    over = _program(rng, 768, MAX_WIRES - 767)
    with pytest.raises(mf.MfhError, match="LDS"):
        ctx.circuit_load(over)


# ------------------------------------------------------------------ 4. MFH_EINVAL
def _create(ctx, nin, gates, asserts):
    gates = np.ascontiguousarray(np.asarray(gates, dtype=np.uint32).reshape(-1, 3))
    asserts = np.ascontiguousarray(np.asarray(asserts, dtype=np.uint32).reshape(-1, 2))
    h = ctypes.c_void_p(12345)
    rc = ctx.lib.mfh_circuit_create(ctx._h, nin, len(gates), ctypes.c_void_p(gates.ctypes.data), len(asserts), ctypes.c_void_p(asserts.ctypes.data),
                                    ctypes.byref(h))
    return rc, h


def test_einval_cases(gpu_ctx_factory, mf):
    p = mf.DEBUG  # m - 1 = 63 wires
    ctx = gpu_ctx_factory(p)
    ok_gates = [(0, 1, 2), (1, 3, 4), (3, 5, 5)]  # nin = 4: wires 5, 6, 7
    rc, h = _create(ctx, 4, ok_gates, [(7, 1)])
    assert rc == 0 and h.value
    ctx.lib.mfh_circuit_destroy(h)
    bad = {
        "unknown op": (4, [(4, 1, 2)], []),
        "operand 0": (4, [(0, 0, 2)], []),
        "second operand 0": (4, [(1, 2, 0)], []),
        "operand = own output": (4, [(0, 1, 5)], []),
        "operand above own output": (4, [(0, 1, 2), (1, 7, 1)], []),
        "NOT of a later wire": (4, [(3, 6, 6), (0, 1, 2)], []),
        "assert on wire 0": (4, ok_gates, [(0, 1)]),
        "assert above nin + ngates": (4, ok_gates, [(8, 0)]),
        "assert value 2": (4, ok_gates, [(5, 2)]),
        "nin + ngates > m - 1": (61, ok_gates, []),
        "nin > m - 1, no gates": (64, [], []),
    }
    for name, (nin, gates, asserts) in bad.items():
        rc, h = _create(ctx, nin, gates, asserts)
        assert rc == EINVAL, name
        assert not h.value, name  # nothing made
    rc, h = _create(ctx, 60, ok_gates, [])  # exactly m - 1
    assert rc == 0
    ctx.lib.mfh_circuit_destroy(h)

    # assign: strides too short for the inputs / for the witness
    rc, h = _create(ctx, 12, [(0, 1, 12), (1, 13, 2)], [])  # 14 wires
    assert rc == 0
    inp = np.zeros((4, 2), dtype=np.uint8)
    out = np.zeros((4, 2), dtype=np.uint8)
    hold = np.zeros(4, dtype=np.uint8)

    def assign(istride, ostride, nb=4):
        return ctx.lib.mfh_circuit_assign(ctx._h, h, nb, ctypes.c_void_p(inp.ctypes.data), istride, ctypes.c_void_p(out.ctypes.data), ostride,
                                          ctypes.c_void_p(hold.ctypes.data))

    assert assign(1, 2) == EINVAL  # 8 < nin = 12
    assert assign(2, 1) == EINVAL  # 8 < nin + ngates = 14
    out[:] = 0x5A
    assert assign(1, 1, nb=0) == EINVAL  # the strides are checked before nstmt
    assert assign(2, 2, nb=0) == 0 and (out == 0x5A).all()  # nstmt = 0: nothing written
    assert assign(2, 2) == 0
    ctx.lib.mfh_circuit_destroy(h)
    # the Python layer: input rows of the wrong width
    prog = ctx.circuit_load(SimpleNamespace(gates=np.array([(0, 1, 12), (1, 13, 2)], dtype=np.uint32), asserts=np.zeros((0, 2), dtype=np.uint32),
                                            nwires=14))
    with pytest.raises(mf.MfhError, match="bits must be"):
        ctx.circuit_assign(prog, np.zeros((3, 11), dtype=np.uint8))
    prog.close()


# ------------------------------------------------------------------ 5. end to end at the default size
def _draws(rng, nb):
    deltas = [int(x) for x in rng.integers(0, P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    return deltas, mags, signs


def test_default_size_end_to_end(gpu_ctx_factory, mf, C):
    import torch
    import oracle_lib as ol

    p = mf.DEFAULT
    rng = np.random.default_rng(55)
    npub, npriv, ngates = 16, 3000, 13500
    c = C.Circuit()  # the circuit of test_gpu_ssp_interp.py::test_default_size_circuit_batch ...
    ws = c.public(npub) + c.private(npriv)
    for _ in range(ngates):
        kind = ("XOR", "AND", "OR", "NOT")[int(rng.integers(0, 4))]
        a, b = (ws[int(rng.integers(0, len(ws)))] for _ in range(2))
        ws.append(c.NOT(a) if kind == "NOT" else getattr(c, kind)(a, b))
    priv = ws[npub: npub + npriv]
    c.assert_equal(priv[0], 1)  # ... with two assertions on its private inputs
    c.assert_equal(c.XOR(priv[1], priv[2]), 1)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    d_ssp = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_prepare(d_ssp)
    alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    d_crs = ctx.setup(d_ssp, alpha, beta, s, d_sk, d_err)

    nb = 255
    bits = _inputs(rng, nb, npub + npriv)
    bits[:, npub] = 1
    bits[:, npub + 2] = 1 - bits[:, npub + 1]
    bad = [4, 77, 128, 254]
    bits[bad[:2], npub] = 0  # x0 = 0
    bits[bad[2:], npub + 2] = bits[bad[2:], npub + 1]  # x1 = x2
    prog = ctx.circuit_load(cc)
    witness, holds = ctx.circuit_assign(prog, bits)
    assert [b for b in range(nb) if not holds[b]] == bad
    ref = [c.assign(bits[b, :npub].tolist(), bits[b, npub:].tolist()) for b in range(nb)]
    assert all(witness[b].tobytes() == ref[b] for b in range(nb))
    assert [c.holds(bits[b, :npub].tolist(), bits[b, npub:].tolist()) for b in range(nb)] == holds.tolist()

    deltas, mags, signs = _draws(rng, nb)
    got = ctx.prove_batch(d_crs, d_ssp, witness, deltas, mags, signs).clone()  # the array as it is
    exp = ctx.prove_batch(d_crs, d_ssp, ref, deltas, mags, signs).clone()
    assert torch.equal(got, exp)
    ok = ctx.to_host(ctx.verify(d_ssp, alpha, beta, s, d_sk, got, nb))
    assert [int(x) for x in ok] == [0 if b in bad else 1 for b in range(nb)]

    honest = [b for b in range(nb) if b not in bad]
    ctx.set_poly_exact(2)
    try:
        ctx.poly_exact_fallbacks()
        hp = ctx.prove_batch(d_crs, d_ssp, list(witness[honest]), [deltas[b] for b in honest], [mags[b] for b in honest],
                             [signs[b] for b in honest]).clone()
        assert ctx.poly_exact_fallbacks() == 0
    finally:
        ctx.set_poly_exact(1)
    assert torch.equal(hp.view(len(honest), -1), got.view(nb, -1)[honest])
    assert int(ctx.verify(d_ssp, alpha, beta, s, d_sk, hp, len(honest)).sum()) == len(honest)
    prog.close()
