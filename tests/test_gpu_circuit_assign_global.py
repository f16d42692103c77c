"""GPU: mfh_circuit_create_global -- circuit witnesses with the wire state in device memory, above the LDS limit MFH_CIRCUIT_MAX_WIRES.

1. the same circuits loaded both ways (mfh_circuit_create / mfh_circuit_create_global) give byte-identical rows and holds: random circuits at mf.DEBUG
   and mf.DEFAULT, batch sizes around the 32-statement block, a count that crosses the global kind's chunk bound, odd strides with zero padding,
   no gates, gates whose two operands are one wire;
2. beyond the LDS limit: MFH_CIRCUIT_MAX_WIRES + 1 and about 200 000 wires against the numpy reference, and state="auto" on both sides of the limit;
3. a 60 000-gate XOR / NOT chain (depth 60 000) against its closed form, in a handful of launches;
4. d = 2^20 end to end: the 470 000-gate circuit of the row-SSP test with assertions, 1 020 statements against the reference and Circuit.assign, a
   mix of holding and failing statements proved through the row SSP and decided by the device verifier;
5. every MFH_EINVAL case of the new create; the LDS kind still stops at MFH_CIRCUIT_MAX_WIRES."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from circuit_levels_ref import evaluate
from circuit_program_ref import random_circuit

pytestmark = pytest.mark.gpu

EINVAL = -1
MAX_WIRES = 32767  # MFH_CIRCUIT_MAX_WIRES
PIN_BYTES = 64 << 20  # pinned staging per chunk of the global kind (include/mfhip.h)


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


def _both(ctx, desc, bits):
    """rows and holds of the LDS program and of the global program of one circuit"""
    out = []
    for state in ("lds", "global"):
        prog = ctx.circuit_load(desc, state=state)
        assert prog.state == state
        out.append(ctx.circuit_assign(prog, bits))
        prog.close()
    return out


def _raw_assign(ctx, prog, inp, ostride, nb):
    """mfh_circuit_assign with explicit strides; the output rows start as 0xFF and holds as 7, so every byte written is seen"""
    out = np.full((nb, ostride), 0xFF, dtype=np.uint8)
    holds = np.full(nb, 7, dtype=np.uint8)
    rc = ctx.lib.mfh_circuit_assign(ctx._h, prog._h, nb, ctypes.c_void_p(inp.ctypes.data), inp.shape[1], ctypes.c_void_p(out.ctypes.data), ostride,
                                    ctypes.c_void_p(holds.ctypes.data))
    assert rc == 0, ctx.lib.mfh_last_error(ctx._h)
    return out, holds


def _chunk(in_stride, bits_stride):
    """statements per launch of the global kind when the wire state is small: whole 32-statement blocks of staging within 64 MiB, at least one"""
    return max(1, PIN_BYTES // (in_stride + bits_stride + 1) // 32) * 32


# ------------------------------------------------------------------ 1. both kinds, byte for byte
@pytest.mark.parametrize("nb", [1, 31, 32, 33, 255, 1020])
@pytest.mark.parametrize("size", ["debug", "default"])
def test_both_kinds_identical(gpu_ctx_factory, mf, size, nb):
    p = mf.DEBUG if size == "debug" else mf.DEFAULT
    rng = np.random.default_rng(nb + (0 if size == "debug" else 7000))
    c = random_circuit(rng, 3, 12, 45, nasserts=3, interleave=True) if size == "debug" else random_circuit(rng, 16, 500, 3000, nasserts=4, interleave=True)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    bits = _inputs(rng, nb, cc.nwires - len(cc.gates))
    (wl, hl), (wg, hg) = _both(ctx, cc, bits)
    assert np.array_equal(wg, wl) and np.array_equal(hg, hl)
    ref_w, ref_h = evaluate(cc, bits, p.m)
    assert np.array_equal(wg, ref_w) and np.array_equal(hg, ref_h)
    for b in range(min(nb, 4)):
        npub = cc.lu
        assert wg[b].tobytes() == c.assign(bits[b, :npub].tolist(), bits[b, npub:].tolist())


def test_across_the_chunk_bound_default(gpu_ctx_factory, mf):
    """mf.DEFAULT rows (16 input bytes, 2 731 witness bytes): the global kind's chunk is 24 416 statements; 132 more take a second launch"""
    p = mf.DEFAULT
    rng = np.random.default_rng(41)
    c = random_circuit(rng, 8, 120, 900, nasserts=2, interleave=True)
    cc = c.compile(p)
    nin = cc.nwires - len(cc.gates)
    stride = (p.m + 7) // 8
    ch = _chunk((nin + 7) // 8, stride)
    nb = ch + 132
    assert ch == 24416
    ctx = gpu_ctx_factory(p)
    bits = _inputs(rng, nb, nin)
    ctx.set_timing(True)
    ctx.timing_drain("circuit_assign_global")
    (wl, hl), (wg, hg) = _both(ctx, cc, bits)
    n, _, rows = ctx.timing_drain("circuit_assign_global")
    assert ctx.timing_drain("circuit_assign")[0] == 3  # the LDS kind: 8 192 statements a launch
    ctx.set_timing(False)
    assert (n, rows) == (2, nb)
    assert np.array_equal(wg, wl) and np.array_equal(hg, hl)
    ref_w, ref_h = evaluate(cc, bits, p.m)
    assert np.array_equal(wg, ref_w) and np.array_equal(hg, ref_h)


def test_across_the_chunk_bound_wide_rows(gpu_ctx_factory, mf):
    """rows of 700 001 bytes (odd, mostly padding): 64 statements a chunk; 100 statements cross it, the padding is zero"""
    p = mf.DEBUG
    rng = np.random.default_rng(42)
    c = random_circuit(rng, 2, 10, 40, nasserts=2)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    nb, istride, ostride = 100, 3, 700001
    assert _chunk(istride, ostride) == 64
    bits = _inputs(rng, nb, 12)
    inp = np.zeros((nb, istride), dtype=np.uint8)
    inp[:, :2] = np.packbits(bits, axis=1, bitorder="little")
    inp[:, 1] |= 0xF0  # input bits >= nin are ignored
    inp[:, 2] = 0x5A
    res = []
    for state in ("lds", "global"):
        prog = ctx.circuit_load(cc, state=state)
        res.append(_raw_assign(ctx, prog, inp, ostride, nb))
        prog.close()
    (ol, hl), (og, hg) = res
    assert np.array_equal(og, ol) and np.array_equal(hg, hl)
    ref_w, ref_h = evaluate(cc, bits, p.m)
    assert np.array_equal(og[:, :8], ref_w) and not og[:, 8:].any()
    assert np.array_equal(hg, ref_h.astype(np.uint8))


def test_odd_strides_zero_padded(gpu_ctx_factory, mf):
    p = mf.DEBUG
    rng = np.random.default_rng(12)
    c = random_circuit(rng, 2, 10, 30, nasserts=1)
    cc = c.compile(p)
    ctx = gpu_ctx_factory(p)
    for nb, istride, ostride in [(45, 7, 13), (33, 3, 9), (70, 5, 11)]:
        bits = _inputs(rng, nb, 12)
        inp = np.zeros((nb, istride), dtype=np.uint8)
        inp[:, :2] = np.packbits(bits, axis=1, bitorder="little")
        inp[:, 1] |= 0xF0
        inp[:, 2:] = 0xA5
        res = []
        for state in ("lds", "global"):
            prog = ctx.circuit_load(cc, state=state)
            res.append(_raw_assign(ctx, prog, inp, ostride, nb))
            prog.close()
        (ol, hl), (og, hg) = res
        assert np.array_equal(og, ol) and np.array_equal(hg, hl)
        ref_w, ref_h = evaluate(cc, bits, p.m)
        assert np.array_equal(og[:, :8], ref_w) and not og[:, 8:].any()
        assert np.array_equal(hg, ref_h.astype(np.uint8))


def test_no_gates_and_same_operands(gpu_ctx_factory, mf, C):
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    c = C.Circuit()
    u = c.public(5)
    x = c.private(30)
    c.assert_equal(u[1], 1)
    c.assert_equal(x[7], 0)
    cc = c.compile(p)
    assert len(cc.gates) == 0
    bits = _inputs(np.random.default_rng(8), 100, 35)
    (wl, hl), (wg, hg) = _both(ctx, cc, bits)
    assert np.array_equal(wg, wl) and np.array_equal(hg, hl) and hg.any() and not hg.all()
    # no gates and no assertion: every statement holds
    c2 = C.Circuit()
    c2.private(9)
    cc2 = c2.compile(p)
    (wl, hl), (wg, hg) = _both(ctx, cc2, bits[:40, :9])
    assert np.array_equal(wg, wl) and hg.all() and hl.all()

    c3 = C.Circuit()
    x = c3.private(4)
    y = [c3.XOR(x[0], x[0]), c3.AND(x[1], x[1]), c3.OR(x[2], x[2]), c3.NOT(x[3])]
    z = [c3.XOR(y[1], y[1]), c3.AND(y[3], y[3]), c3.OR(y[0], y[0])]
    c3.assert_equal(c3.XOR(z[1], z[1]), 0)
    cc3 = c3.compile(p)
    bits3 = np.array([[(i >> k) & 1 for k in range(4)] for i in range(16)] * 3, dtype=np.uint8)
    (wl, hl), (wg, hg) = _both(ctx, cc3, bits3)
    assert np.array_equal(wg, wl) and hg.all() and hl.all()
    for b in range(len(bits3)):
        assert wg[b].tobytes() == c3.assign([], bits3[b].tolist())


# ------------------------------------------------------------------ 2. beyond the LDS limit
def _program(rng, nin, ngates, nasserts=8, window=200):
    """gate g reads two earlier wires, two thirds of them among the last `window` (deep as well as wide), the rest anywhere"""
    hi = nin + np.arange(ngates, dtype=np.int64)  # operands in [1, hi]
    lo = np.where(np.arange(ngates) % 3 == 0, 1, np.maximum(1, hi - window))
    a, b = (lo + (rng.random(ngates) * (hi - lo + 1)).astype(np.int64) for _ in range(2))
    op = rng.integers(0, 4, size=ngates)
    b = np.where(op == 3, a, b)
    gates = np.stack([op, a, b], axis=1).astype(np.uint32)
    asserts = np.stack([rng.integers(1, nin + ngates + 1, size=nasserts), rng.integers(0, 2, size=nasserts)], axis=1).astype(np.uint32).reshape(-1, 2)
    return SimpleNamespace(gates=gates, asserts=asserts, nwires=nin + ngates)


def test_one_wire_over_the_lds_limit(gpu_ctx_factory, mf):
    p = mf.Params(d=256, m=40000)
    rng = np.random.default_rng(22)
    ctx = gpu_ctx_factory(p)
    desc = _program(rng, 768, MAX_WIRES - 767)
    assert desc.nwires == MAX_WIRES + 1
    with pytest.raises(mf.MfhError, match="LDS"):
        ctx.circuit_load(desc)  # the default stays "lds"
    prog = ctx.circuit_load(desc, state="auto")
    assert prog.state == "global"
    bits = _inputs(rng, 70, 768)
    w, h = ctx.circuit_assign(prog, bits)
    ref_w, ref_h = evaluate(desc, bits, p.m)
    assert np.array_equal(w, ref_w) and np.array_equal(h, ref_h)
    prog.close()
    # at the limit "auto" keeps the LDS kind, and both kinds agree
    at = _program(rng, 767, MAX_WIRES - 767)
    prog = ctx.circuit_load(at, state="auto")
    assert prog.state == "lds"
    prog.close()
    bits = _inputs(rng, 40, 767)
    (wl, hl), (wg, hg) = _both(ctx, at, bits)
    assert np.array_equal(wg, wl) and np.array_equal(hg, hl)


@pytest.mark.parametrize("nb", [33, 300])
def test_200k_wires(gpu_ctx_factory, mf, nb):
    p = mf.Params(d=256, m=200001)
    rng = np.random.default_rng(23 + nb)
    ctx = gpu_ctx_factory(p)
    nin = 30000  # tens of thousands of inputs: 3 750-byte rows
    desc = _program(rng, nin, p.m - 1 - nin, nasserts=3)
    assert desc.nwires == 200000
    prog = ctx.circuit_load(desc, state="global")
    bits = _inputs(rng, nb, nin)
    w, h = ctx.circuit_assign(prog, bits)
    ref_w, ref_h = evaluate(desc, bits, p.m)
    assert np.array_equal(w, ref_w) and np.array_equal(h, ref_h)
    prog.close()
    with pytest.raises(mf.MfhError, match="state must be"):
        ctx.circuit_load(desc, state="hbm")


# ------------------------------------------------------------------ 3. deep and narrow
def test_deep_chain(gpu_ctx_factory, mf):
    """g_k = g_(k-1) XOR x_(k+1 mod nin), every fifth gate a NOT instead: depth 60 000, nw = 100 000; the closed form is a prefix parity"""
    nin, ngates, nb = 40000, 60000, 100
    p = mf.Params(d=256, m=nin + ngates + 1)
    gates = np.zeros((ngates, 3), dtype=np.uint32)
    k = np.arange(ngates, dtype=np.int64)
    prev = np.where(k == 0, 1, nin + k)
    nots = k % 5 == 4
    gates[:, 0] = np.where(nots, 3, 0)
    gates[:, 1] = prev
    gates[:, 2] = np.where(nots, prev, 1 + (k + 1) % nin)
    desc = SimpleNamespace(gates=gates, asserts=np.array([[nin + ngates, 1]], dtype=np.uint32), nwires=nin + ngates)
    rng = np.random.default_rng(60)
    bits = _inputs(rng, nb, nin)
    ctx = gpu_ctx_factory(p)
    prog = ctx.circuit_load(desc, state="auto")
    assert prog.state == "global"
    ctx.set_timing(True)
    ctx.timing_drain("circuit_assign_global")
    w, h = ctx.circuit_assign(prog, bits)
    n, ms, rows = ctx.timing_drain("circuit_assign_global")
    ctx.set_timing(False)
    assert rows == nb and 1 <= n < 100, (n, ms)
    # closed form: g_k = x_0 ^ x_1 ^ ... over the XOR steps so far, complemented once per NOT so far
    xs = np.where(nots[:, None], 0, bits[:, (k + 1) % nin].T).T  # [nb, ngates]: the input each step XORs in
    val = (bits[:, :1] ^ np.bitwise_xor.accumulate(xs, axis=1) ^ (np.cumsum(nots) & 1)[None, :]).astype(np.uint8)
    exp = np.zeros((nb, p.m + 7 - (p.m + 7) % 8), dtype=np.uint8)
    exp[:, :nin] = bits
    exp[:, nin: nin + ngates] = val
    assert np.array_equal(w, np.packbits(exp, axis=1, bitorder="little")[:, : (p.m + 7) // 8])
    assert np.array_equal(h, val[:, -1] == 1)
    prog.close()


# ------------------------------------------------------------------ 4. d = 2^20 end to end
def test_two_pow_20_end_to_end(mf, C):
    """the 470 000-gate circuit of test_gpu_ssp_rows.py::test_two_pow_20_circuit_proved_and_verified, with two assertions on private inputs"""
    from test_gpu_ssp_interp import SEED, _draws, _keys, _random_circuit

    p = mf.Params(d=1 << 20, m=699050)
    rng = np.random.default_rng(2021)
    npub, npriv, ngates = 64, 20000, 470000
    c, _ = _random_circuit(C, rng, npub, npriv, ngates)
    priv = [C.Wire(npub + i) for i in range(3)]  # the first private inputs (nodes npub ..)
    c.assert_equal(priv[0], 1)
    c.assert_equal(c.XOR(priv[1], priv[2]), 1)
    cc = c.compile(p)
    nin = npub + npriv
    assert cc.nwires == nin + ngates + 1 and cc.nwires > MAX_WIRES

    nb = 1020
    bits = _inputs(rng, nb, nin)
    bits[:, npub] = 1
    bits[:, npub + 2] = 1 - bits[:, npub + 1]
    bad = sorted(int(x) for x in rng.choice(nb, size=40, replace=False))
    bits[bad[:20], npub] = 0  # x0 = 0
    bits[bad[20:], npub + 2] = bits[bad[20:], npub + 1]  # x1 = x2
    ctx = mf.Context(p, 0)
    try:
        prog = ctx.circuit_load(cc, state="auto")
        assert prog.state == "global"
        witness, holds = ctx.circuit_assign(prog, bits)
        assert [b for b in range(nb) if not holds[b]] == bad
        ref_w, ref_h = evaluate(cc, bits, p.m)
        assert np.array_equal(witness, ref_w) and np.array_equal(holds, ref_h)
        for b in [0, 1, bad[0], 500, bad[-1], 1019, 777, 333]:
            pub, prv = bits[b, :npub].tolist(), bits[b, npub:].tolist()
            assert witness[b].tobytes() == c.assign(pub, prv), b
            assert bool(holds[b]) == c.holds(pub, prv), b
        prog.close()

        # prove 16 of them through the row SSP, 5 failing
        good = [b for b in range(nb) if b not in bad]
        sub = sorted(bad[::9] + good[::90][:11])
        assert len(sub) == 16 and sum(1 for b in sub if not holds[b]) == 5
        ctx.set_seed(SEED)
        ctx.ssp_set_rows(cc.rows, lu_max=npub)
        ctx.ssp_prepare(None)
        K = _keys(ctx, rng, p)
        d_crs = ctx.setup_public(None, K["alpha"], K["beta"], K["s"], npub, K["d_sk"], K["d_err"]).clone()
        stmts = [witness[b].tobytes() for b in sub]
        deltas, mags, signs = _draws(rng, len(sub))
        proofs = ctx.prove_batch_public(d_crs, None, npub, stmts, deltas, mags, signs).clone()
        vk = ctx.derive_vk(None, K["s"], npub)
        ok = ctx.to_host(ctx.verify_public(vk, npub, K["alpha"], K["beta"], K["d_sk"], proofs, stmts), np.uint8)
        assert [bool(x) for x in ok] == [bool(holds[b]) for b in sub]
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. MFH_EINVAL
def _create(ctx, nin, gates, asserts, fn="mfh_circuit_create_global", null_gates=False):
    gates = np.ascontiguousarray(np.asarray(gates, dtype=np.uint32).reshape(-1, 3))
    asserts = np.ascontiguousarray(np.asarray(asserts, dtype=np.uint32).reshape(-1, 2))
    h = ctypes.c_void_p(12345)
    gp = ctypes.c_void_p(0) if null_gates else ctypes.c_void_p(gates.ctypes.data)
    rc = getattr(ctx.lib, fn)(ctx._h, nin, len(gates), gp, len(asserts), ctypes.c_void_p(asserts.ctypes.data), ctypes.byref(h))
    return rc, h


def test_einval_cases(gpu_ctx_factory, mf):
    p = mf.DEBUG  # m - 1 = 63 wires
    ctx = gpu_ctx_factory(p)
    ok_gates = [(0, 1, 2), (1, 3, 4), (3, 5, 5)]  # nin = 4: wires 5, 6, 7
    rc, h = _create(ctx, 4, ok_gates, [(7, 1)])
    assert rc == 0 and h.value
    ctx.lib.mfh_circuit_destroy(h)
    bad = {
        "unknown op": (4, [(4, 1, 2)], [], "unknown gate op"),
        "operand 0": (4, [(0, 0, 2)], [], "operand is 0"),
        "second operand 0": (4, [(1, 2, 0)], [], "operand is 0"),
        "operand = own output": (4, [(0, 1, 5)], [], "not below"),
        "operand above own output": (4, [(0, 1, 2), (1, 7, 1)], [], "not below"),
        "NOT of a later wire": (4, [(3, 6, 6), (0, 1, 2)], [], "not below"),
        "assert on wire 0": (4, ok_gates, [(0, 1)], "assertion on wire 0"),
        "assert above nin + ngates": (4, ok_gates, [(8, 0)], "above nin"),
        "assert value 2": (4, ok_gates, [(5, 2)], "value other than"),
        "nin + ngates > m - 1": (61, ok_gates, [], "m - 1"),
        "nin > m - 1, no gates": (64, [], [], "m - 1"),
    }
    for name, (nin, gates, asserts, text) in bad.items():
        for fn in ("mfh_circuit_create", "mfh_circuit_create_global"):
            rc, h = _create(ctx, nin, gates, asserts, fn=fn)
            assert rc == EINVAL, (name, fn)
            assert not h.value, (name, fn)  # nothing made
            err = ctx.lib.mfh_last_error(ctx._h).decode()
            assert err.startswith(fn + ": ") and text in err, (name, err)
    rc, h = _create(ctx, 4, ok_gates, [], null_gates=True)
    assert rc == EINVAL and not h.value and "without their array" in ctx.lib.mfh_last_error(ctx._h).decode()
    rc, h = _create(ctx, 60, ok_gates, [])  # exactly m - 1
    assert rc == 0
    ctx.lib.mfh_circuit_destroy(h)

    # nw > m - 1 at a size the LDS kind could not hold either; MFH_CIRCUIT_MAX_WIRES + 1 under m - 1 is the LDS kind's error only
    big = mf.Params(d=256, m=40000)
    ctx2 = gpu_ctx_factory(big)
    g = _program(np.random.default_rng(3), 40000 - 100, 100, nasserts=0).gates
    rc, h = _create(ctx2, 40000 - 100, g, [])  # 40 000 wires > m - 1 = 39 999
    assert rc == EINVAL and not h.value and "m - 1" in ctx2.lib.mfh_last_error(ctx2._h).decode()
    g = _program(np.random.default_rng(4), 768, MAX_WIRES - 767, nasserts=0).gates
    rc, h = _create(ctx2, 768, g, [], fn="mfh_circuit_create")
    assert rc == EINVAL and not h.value and "LDS" in ctx2.lib.mfh_last_error(ctx2._h).decode()
    rc, h = _create(ctx2, 768, g, [])
    assert rc == 0 and h.value
    ctx2.lib.mfh_circuit_destroy(h)

    # assign on a global program: the same stride checks and nstmt = 0
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
