"""GPU: mfh_circuit_create_ex -- extended gate programs (MAJ, SUM3, CONST, LUT2, equalities) and the ChaCha20 block statement proved end to end.

1. random programs over every op with assertions and equalities, both kinds (LDS and device memory), nb in {1, 31, 32, 33, 255, 1020}: witness rows
   and holds byte-identical to Circuit.assign / holds, to the numpy reference of Compiled.program, and to each other, padding included;
2. every MFH_EINVAL case of mfh_circuit_create_ex, each by name with its own text, nothing made; the old creates still refuse the new ops;
3. an old-op circuit still loads through mfh_circuit_create (and mfh_circuit_create_global) and gives the same rows as before;
4. mf.DEFAULT, dense SSP: a ChaCha double round with 16 public input and 16 public output words, proved in a batch and decided by verify_public --
   the satisfying statements accepted, four tampered ones rejected;
5. d = 2^16, row SSP: the ChaCha20 block statement (RFC 8439 2.3.2 vector and random keys), witnesses on the device, proved in a batch of 255;
   every honest statement verifies, a statement with one flipped public bit is rejected."""
import ctypes
import time

import numpy as np
import pytest

from circuit_ex_ref import bitsliced_ex, chacha20_block_int, double_round_int, einval_cases, random_ex_circuit

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def C():
    from c_lwe_snarks_amd import circuit

    return circuit


@pytest.fixture(scope="module")
def W():
    from c_lwe_snarks_amd import words

    return words


# ------------------------------------------------------------------ 1. random programs, both kinds
@pytest.fixture(scope="module")
def mixed(C):
    """a random circuit over every op: 24 inputs, 1 500 gates, two equalities and one assertion on inputs (holds on about 1 in 8 statements), one
    equality between gate wires that holds whatever the input (a gate and the same gate again)"""
    rng = np.random.default_rng(1234)
    c = random_ex_circuit(rng, 8, 16, 1500, nasserts=0, nequal=0)
    x = [C.Wire(i) for i in range(24)]
    c.assert_same(x[1], x[9])
    c.assert_same(x[20], x[3])
    c.assert_equal(x[5], 1)
    g = c.MAJ(x[0], x[2], x[4])
    c.assert_same(g, c.MAJ(x[0], x[2], x[4]))
    return c


@pytest.mark.parametrize("nb", [1, 31, 32, 33, 255, 1020])
def test_random_programs_both_kinds(gpu_ctx_factory, mf, mixed, nb):
    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    cc = mixed.compile(p)
    ops = set(cc.program[:, 0].tolist())
    assert {0, 1, 2, 3, 4, 5, 6, 7} <= ops and len([o for o in ops if o >= 16]) >= 8 and len(cc.equal) == 3
    rng = np.random.default_rng(nb)
    bits = rng.integers(0, 2, size=(nb, 24), dtype=np.uint8)
    lds = ctx.circuit_load(cc, state="lds")
    glb = ctx.circuit_load(cc, state="global")
    assert lds.extended and glb.extended and lds.state == "lds" and glb.state == "global"
    w1, h1 = ctx.circuit_assign(lds, bits)
    w2, h2 = ctx.circuit_assign(glb, bits)
    assert np.array_equal(w1, w2) and np.array_equal(h1, h2)
    ref_w, ref_h = bitsliced_ex(cc, bits, p.m)
    assert np.array_equal(w1, ref_w) and np.array_equal(h1, ref_h)
    for b in range(nb):
        pub, prv = bits[b, :8].tolist(), bits[b, 8:].tolist()
        assert w1[b].tobytes() == mixed.assign(pub, prv, p), b
        assert bool(h1[b]) == mixed.holds(pub, prv), b
    if nb >= 255:
        assert 0 < h1.sum() < nb
    lds.close()
    glb.close()


def test_deep_adder_chain_both_kinds(gpu_ctx_factory, mf, W):
    """a chain of 200 dependent 32-bit adds (depth about 6 200) with the result pinned by equalities to a public word"""
    p = mf.DEFAULT
    w = W.Words()
    x, y, r = w.private(), w.private(), w.public()
    acc = x
    for _ in range(200):
        acc = w.add(acc, y)
    w.assert_same_u32(acc, r)
    cc = w.c.compile(p)
    rng = np.random.default_rng(3)
    nb = 100
    xv = rng.integers(0, 1 << 32, size=nb, dtype=np.uint64)
    yv = rng.integers(0, 1 << 32, size=nb, dtype=np.uint64)
    rv = (xv + 200 * yv) & 0xFFFFFFFF
    rv[::7] ^= 1 << 5  # every 7th statement fails
    bits = np.concatenate([W.pack(rv[:, None]), W.pack(xv[:, None]), W.pack(yv[:, None])], axis=1)
    ctx = gpu_ctx_factory(p)
    for state in ("lds", "global"):
        prog = ctx.circuit_load(cc, state=state)
        wit, holds = ctx.circuit_assign(prog, bits)
        assert holds.tolist() == [b % 7 != 0 for b in range(nb)], state
        for b in (0, 1, 50, 99):
            assert wit[b].tobytes() == w.c.assign(bits[b, :32].tolist(), bits[b, 32:].tolist(), p), (state, b)
        prog.close()


# ------------------------------------------------------------------ 2. MFH_EINVAL
def _create_ex(ctx, nin, program, asserts, equal, flags, null=None):
    program = np.ascontiguousarray(np.asarray(program, dtype=np.uint32).reshape(-1, 4))
    asserts = np.ascontiguousarray(np.asarray(asserts, dtype=np.uint32).reshape(-1, 2))
    equal = np.ascontiguousarray(np.asarray(equal, dtype=np.uint32).reshape(-1, 2))
    ptr = {k: ctypes.c_void_p(0 if null == k else a.ctypes.data) for k, a in (("gates", program), ("asserts", asserts), ("equal", equal))}
    h = ctypes.c_void_p(12345)
    rc = ctx.lib.mfh_circuit_create_ex(ctx._h, nin, len(program), ptr["gates"], len(asserts), ptr["asserts"], len(equal), ptr["equal"], flags,
                                       ctypes.byref(h))
    return rc, h


def test_einval_cases(gpu_ctx_factory, mf):
    ctxs = {64: gpu_ctx_factory(mf.DEBUG), 40000: gpu_ctx_factory(mf.Params(d=256, m=40000))}
    ok = [(0, 1, 2, 0), (4, 1, 2, 5), (5, 1, 2, 5), (6, 0, 0, 0), (7, 0, 0, 0), (16 + 13, 8, 9, 0), (3, 10, 10, 0)]
    for flags in (0, 1):
        rc, h = _create_ex(ctxs[64], 4, ok, [(11, 0)], [(1, 11)], flags)
        assert rc == 0 and h.value, flags
        ctxs[64].lib.mfh_circuit_destroy(h)
    cases = einval_cases()
    assert len(cases) >= 25
    for name, (nin, program, asserts, equal, m, flags, text) in cases.items():
        ctx = ctxs[m]
        for fl in (flags,) if flags or name == "LDS limit" else (0, 1):
            rc, h = _create_ex(ctx, nin, program, asserts, equal, fl)
            err = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and not h.value, (name, fl, rc)
            assert err == "mfh_circuit_create_ex: " + text, (name, fl, err)
    # the LDS limit is the LDS kind's alone
    nin, program, asserts, equal, m, _, _ = cases["LDS limit"]
    rc, h = _create_ex(ctxs[40000], nin, program, asserts, equal, 1)
    assert rc == 0 and h.value
    ctxs[40000].lib.mfh_circuit_destroy(h)
    # null arrays
    for null, text in (("gates", "gates / assertions without their array"), ("asserts", "gates / assertions without their array"),
                       ("equal", "equalities without their array")):
        rc, h = _create_ex(ctxs[64], 4, ok, [(11, 0)], [(1, 11)], 0, null=null)
        assert rc == EINVAL and not h.value and ctxs[64].lib.mfh_last_error(ctxs[64]._h).decode() == "mfh_circuit_create_ex: " + text
    # the old creates still refuse op 4 and above
    ctx = ctxs[64]
    gates = np.ascontiguousarray(np.array([(4, 1, 2)], dtype=np.uint32))
    for fn in ("mfh_circuit_create", "mfh_circuit_create_global"):
        h = ctypes.c_void_p(12345)
        rc = getattr(ctx.lib, fn)(ctx._h, 4, 1, ctypes.c_void_p(gates.ctypes.data), 0, ctypes.c_void_p(0), ctypes.byref(h))
        assert rc == EINVAL and not h.value and ctx.lib.mfh_last_error(ctx._h).decode() == fn + ": unknown gate op"


# ------------------------------------------------------------------ 3. old-op circuits keep the old entry points
def test_old_op_circuit_loads_through_the_old_creates(gpu_ctx_factory, mf):
    from circuit_program_ref import bitsliced, random_circuit

    p = mf.DEFAULT
    c = random_circuit(np.random.default_rng(77), 4, 30, 900, nasserts=3)
    cc = c.compile(p)
    assert len(cc.equal) == 0 and (cc.program[:, 0] <= 3).all()
    ctx = gpu_ctx_factory(p)
    bits = np.random.default_rng(78).integers(0, 2, size=(70, 34), dtype=np.uint8)
    ref_w, ref_h = bitsliced(cc, bits, p.m)
    for state in ("lds", "global"):
        prog = ctx.circuit_load(cc, state=state)
        assert not prog.extended and prog.state == state
        ctx.set_timing(True)
        w, h = ctx.circuit_assign(prog, bits)
        kind = "circuit_assign" if state == "lds" else "circuit_assign_global"
        assert ctx.timing_drain(kind)[0] == 1 and ctx.timing_drain(kind + "_ex")[0] == 0, state
        ctx.set_timing(False)
        assert np.array_equal(w, ref_w) and np.array_equal(h, ref_h)
        prog.close()


# ------------------------------------------------------------------ 4. a ChaCha double round at mf.DEFAULT, dense SSP
def _draws(rng, nb, P):
    deltas = [int(x) for x in rng.integers(0, P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    return deltas, mags, signs


def _keys(ctx, rng, p, P):
    import oracle_lib as ol

    alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    return alpha, beta, s, d_sk, d_err


def _flip(stmt: bytes, bit: int) -> bytes:
    b = bytearray(stmt)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def test_double_round_default_dense(gpu_ctx_factory, mf, C, W):
    from test_gpu_ssp_interp import SEED

    p = mf.DEFAULT
    w = W.Words()
    xin, xout = w.public(16), w.public(16)
    y = W.double_round(w, xin)
    for a, b in zip(y, xout):
        w.assert_same_u32(a, b)
    c = w.c
    cc = c.compile(p)
    lu = cc.lu
    assert lu == 1024 and cc.nwires == 1024 + 32 * 64 + 32 * 32 and len(cc.equal) == 512

    rng = np.random.default_rng(808)
    nb = 16
    ins = [[int(v) for v in rng.integers(0, 1 << 32, size=16, dtype=np.uint64)] for _ in range(nb)]
    outs = [double_round_int(v) for v in ins]
    outs[3] = list(outs[3]); outs[3][5] ^= 1 << 17   # two statements whose claimed output is wrong
    outs[9] = list(outs[9]); outs[9][0] ^= 1
    bits = np.stack([W.pack(list(i) + list(o)) for i, o in zip(ins, outs)])
    ctx = gpu_ctx_factory(p)
    prog = ctx.circuit_load(cc)
    witness, holds = ctx.circuit_assign(prog, bits)
    assert [b for b in range(nb) if not holds[b]] == [3, 9]
    for b in (0, 3, 15):
        assert witness[b].tobytes() == c.assign(bits[b], [], p)
    prog.close()

    P = C.P
    ctx.set_seed(SEED)
    d_ssp = ctx.ssp_from_rows(cc.rows)
    ctx.ssp_prepare(d_ssp)
    alpha, beta, s, d_sk, d_err = _keys(ctx, rng, p, P)
    d_crs = ctx.setup_public(d_ssp, alpha, beta, s, lu, d_sk, d_err).clone()
    stmts = [witness[b].tobytes() for b in range(nb)]
    deltas, mags, signs = _draws(rng, nb, P)
    proofs = ctx.prove_batch_public(d_crs, d_ssp, lu, stmts, deltas, mags, signs).clone()
    vk = ctx.derive_vk(d_ssp, s, lu)
    ok = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, stmts), np.uint8)
    assert [bool(x) for x in ok] == [b not in (3, 9) for b in range(nb)]
    # two honest proofs checked against tampered statements: a flipped input bit, a flipped output bit
    tampered = list(stmts)
    tampered[0] = _flip(stmts[0], 7)
    tampered[1] = _flip(stmts[1], 512 + 300)
    ok2 = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, tampered), np.uint8)
    assert [bool(x) for x in ok2] == [b not in (0, 1, 3, 9) for b in range(nb)]


# ------------------------------------------------------------------ 5. the ChaCha20 block at d = 2^16, row SSP
RFC_KEY = bytes(range(32))
RFC_NONCE = bytes.fromhex("000000090000004a00000000")


def test_chacha20_block_two_pow_16(mf, C, W):
    from test_gpu_ssp_interp import SEED

    p = mf.Params(d=1 << 16, m=43690)
    P = C.P
    st = W.ChaCha20Block()
    c = st.circuit
    cc = c.compile(p)
    lu = cc.lu
    assert lu == 640 and cc.nwires == 32642 and cc.nrows == 64900

    rng = np.random.default_rng(20260)
    nb = 255
    rows = []
    for b in range(nb):
        if b == 0:
            key, counter, nonce = RFC_KEY, 1, RFC_NONCE
        else:
            key = bytes(rng.integers(0, 256, size=32, dtype=np.uint8).tolist())
            counter = int(rng.integers(0, 1 << 32, dtype=np.uint64))
            nonce = bytes(rng.integers(0, 256, size=12, dtype=np.uint8).tolist())
        rows.append(st.bits(key, counter, nonce, chacha20_block_int(key, counter, nonce)))
    bits = np.stack(rows)
    assert bits[0, 128:192].tolist() == W.pack(W.le_words(bytes.fromhex("10f1e7e4d13b5915"))).tolist()

    ctx = mf.Context(p, 0)
    try:
        prog = ctx.circuit_load(cc, state="auto")
        assert prog.state == "lds" and prog.extended
        witness, holds = ctx.circuit_assign(prog, bits)
        assert holds.all()
        for b in (0, 1, 254):
            assert witness[b].tobytes() == c.assign(bits[b, :640], bits[b, 640:], p), b
        glb = ctx.circuit_load(cc, state="global")
        w2, h2 = ctx.circuit_assign(glb, bits)
        assert np.array_equal(w2, witness) and np.array_equal(h2, holds)
        bad = bits[:4].copy()
        bad[:, 200] ^= 1  # a flipped block bit: no key gives it
        _, hb = ctx.circuit_assign(prog, bad)
        assert not hb.any()
        prog.close()
        glb.close()

        ctx.set_seed(SEED)
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        ctx.ssp_prepare(None)
        alpha, beta, s, d_sk, d_err = _keys(ctx, rng, p, P)
        d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()
        stmts = [witness[b].tobytes() for b in range(nb)]
        deltas, mags, signs = _draws(rng, nb, P)
        t0 = time.perf_counter()
        proofs = ctx.prove_batch_public(d_crs, None, lu, stmts, deltas, mags, signs).clone()
        ctx.sync()
        print(f"prove_batch_public, {nb} ChaCha20 block statements at d = 2^16: {(time.perf_counter() - t0) * 1e3:.1f} ms (first call)")
        vk = ctx.derive_vk(None, s, lu)
        ok = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, stmts), np.uint8)
        assert all(bool(x) for x in ok)
        tampered = list(stmts)
        tampered[0] = _flip(stmts[0], 128 + 3)  # the RFC statement with one block bit flipped
        tampered[100] = _flip(stmts[100], 5)    # a counter bit
        ok2 = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, tampered), np.uint8)
        assert [bool(x) for x in ok2] == [b not in (0, 100) for b in range(nb)]
    finally:
        ctx.close()
