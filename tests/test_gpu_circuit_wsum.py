"""GPU: weighted-sum gates (mfh_circuit_create_sum, the SUM = true kernels) and the SHA-256 compression statement at d = 2^16.

1. random programs mixing every gate kind with WSUM, both state kinds (LDS and device memory), with and without outputs, nb in {1, 31, 33, 1020}:
   witness rows and holds byte-identical to the numpy restatement (circuit_wsum_ref.bitsliced_sum) and to Circuit.assign / holds; the launches counted
   under "circuit_assign_sum" / "circuit_assign_global_sum";
2. every MFH_EINVAL case of mfh_circuit_create_sum, each with its own text, nothing made; mfh_circuit_create_ex / _out still reject op 8;
3. a program without a WSUM gate through mfh_circuit_create_sum is mfh_circuit_create_out's (same kernels and timing kinds, same bytes);
4. long rows (a wsum gate's rows, 100 and more entries) through both interpolators at d = 1152: mfh_ssp_from_rows and mfh_ssp_rows_fill agree with each
   other, and every slot polynomial takes the row's coefficient sums at the points r_j;
5. d = 2^16, row SSP: 255 SHA-256 statements written with sums, witnesses from the LDS kernel, proved in one batch without an exact-division fallback;
   digests equal hashlib's, every proof accepted, a flipped digest bit rejected, a proof from a witness with one carry wire flipped rejected."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

import circuit_ref as cr
from circuit_wsum_ref import bitsliced_sum, random_sum_circuit

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


# ------------------------------------------------------------------ 1. random programs, both kinds, with and without outputs
NPUB, NPRIV = 8, 16


def _mixed(C, noutputs):
    rng = np.random.default_rng(8642 + noutputs)
    c = random_sum_circuit(rng, NPUB, NPRIV, 3000, nsums=120, noutputs=noutputs, max_terms=150)
    c.assert_equal(C.Wire(NPUB + 1), 1)  # on inputs: they hold on 1 statement in 4
    c.assert_same(C.Wire(2), C.Wire(NPUB + 5))
    return c


@pytest.mark.parametrize("noutputs", [0, 30])
@pytest.mark.parametrize("nb", [1, 31, 33, 1020])
def test_random_programs_with_sums_both_kinds(gpu_ctx_factory, mf, C, nb, noutputs):
    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    c = _mixed(C, noutputs)
    cc = c.compile(p)
    lu, nin = cc.lu, cc.lu + NPRIV
    heads = cc.program[cc.program[:, 0] == C.GATE_WSUM]
    assert lu == NPUB + noutputs and len(heads) == 120 and {0, 1, 2, 3, 4, 5, 6, 7, 8, 9} <= set(cc.program[:, 0].tolist())
    assert int(heads[:, 2].max()) > 128 and int(heads[:, 2].min()) < 8  # more than two gathers of 64 terms, and a short one
    rng = np.random.default_rng(nb)
    bits = rng.integers(0, 2, size=(nb, nin), dtype=np.uint8)  # garbage at the outputs' positions too
    lds = ctx.circuit_load(cc, state="lds")
    glb = ctx.circuit_load(cc, state="global")
    assert lds.sums and glb.sums and lds.extended and lds.outputs == glb.outputs == noutputs and (lds.state, glb.state) == ("lds", "global")
    ctx.set_timing(True)
    w1, h1 = ctx.circuit_assign(lds, bits)
    w2, h2 = ctx.circuit_assign(glb, bits)
    kinds = ("circuit_assign_sum", "circuit_assign_global_sum", "circuit_assign_out", "circuit_assign_global_out", "circuit_assign_ex",
             "circuit_assign_global_ex")
    counts = {k: ctx.timing_drain(k)[0] for k in kinds}
    ctx.set_timing(False)
    assert counts == {k: int(k.endswith("_sum")) for k in kinds}
    assert np.array_equal(w1, w2) and np.array_equal(h1, h2)
    ref_w, ref_h = bitsliced_sum(cc, bits, p.m)
    assert np.array_equal(w1, ref_w) and np.array_equal(h1, ref_h)
    for b in range(nb) if nb <= 33 else (0, 31, 32, 511, 1019):
        pub, prv = bits[b, :lu].tolist(), bits[b, lu:].tolist()
        assert w1[b].tobytes() == c.assign(pub, prv, p), b
        assert bool(h1[b]) == c.holds(pub, prv), b
    if nb >= 1020:
        assert 0 < h1.sum() < nb
    lds.close()
    glb.close()


# ------------------------------------------------------------------ 2. MFH_EINVAL
def _create_sum(ctx, nin, program, asserts, equal, outputs, terms, flags, null_terms=False, nterms=None):
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1, k)) for a, k in ((program, 4), (asserts, 2), (equal, 2), (outputs, 2), (terms, 2))]
    ptr = [ctypes.c_void_p(a.ctypes.data) for a in arrs]
    if null_terms:
        ptr[4] = ctypes.c_void_p(0)
    h = ctypes.c_void_p(12345)
    rc = ctx.lib.mfh_circuit_create_sum(ctx._h, nin, len(arrs[0]), ptr[0], len(arrs[1]), ptr[1], len(arrs[2]), ptr[2], len(arrs[3]), ptr[3],
                                        len(arrs[4]) if nterms is None else nterms, ptr[4], flags, ctypes.byref(h))
    return rc, h


# nin = 4.  An accepted program: XOR -> wire 5; WSUM of 3 terms, 3 bits -> wires 6, 7, 8; AND of a sum bit -> wire 9
_T = [(1, 0), (5, 0), (2, 1), (1, 1)]  # the head uses terms 1 .. 3: Tmax = 1 + 2 + 2 = 5: 3 bits
_OK = [(0, 1, 2, 0), (8, 1, 3, 3), (9, 1, 0, 0), (9, 2, 0, 0), (1, 8, 5, 0)]
_ORDER = "a WSUM head not followed by its WSUM_BIT records in order"
# name -> (program, asserts, equal, outputs, terms, flags, text)
SUM_CASES = {
    "term range past the array": ([(0, 1, 2, 0), (8, 2, 3, 3), (9, 1, 0, 0), (9, 2, 0, 0)], [], [], [], _T, 0, "a WSUM gate's term range lies outside the term array"),
    "first_term past the array": ([(8, 5, 1, 1)], [], [], [], _T, 0, "a WSUM gate's term range lies outside the term array"),
    "first_term + nterms wraps": ([(8, 0xFFFFFFFF, 2, 1)], [], [], [], _T, 0, "a WSUM gate's term range lies outside the term array"),
    "nterms = 0": ([(8, 0, 0, 1)], [], [], [], _T, 0, "a WSUM gate with nterms = 0"),
    "term wire 0": ([(8, 0, 1, 1)], [], [], [], [(0, 0)], 0, "a WSUM term wire is 0 or not below the head's output wire"),
    "term wire = the head's output": ([(8, 0, 1, 1)], [], [], [], [(5, 0)], 0, "a WSUM term wire is 0 or not below the head's output wire"),
    "term wire = a later output bit": ([(8, 0, 2, 2), (9, 1, 0, 0)], [], [], [], [(1, 0), (6, 0)], 0, "a WSUM term wire is 0 or not below the head's output wire"),
    "term reads an output wire": ([(8, 0, 2, 2), (9, 1, 0, 0)], [], [], [(3, 5)], [(1, 0), (3, 1)], 0, "a WSUM term reads an output wire"),
    "shift >= nbits": ([(8, 0, 2, 2), (9, 1, 0, 0)], [], [], [], [(1, 0), (2, 2)], 0, "a WSUM term with shift >= nbits"),
    "shift 40": ([(8, 0, 1, 24)] + [(9, i, 0, 0) for i in range(1, 24)], [], [], [], [(1, 40)], 0, "a WSUM term with shift >= nbits"),
    "shifts out of order": ([(8, 0, 2, 2), (9, 1, 0, 0)], [], [], [], [(1, 1), (2, 0)], 0, "WSUM terms not in non-decreasing shift order"),
    "nbits too large": ([(8, 0, 2, 3), (9, 1, 0, 0), (9, 2, 0, 0)], [], [], [], [(1, 0), (2, 1)], 0,
                        "a WSUM gate whose nbits is not the bit length of the sum of 2^shift"),
    "nbits too small": ([(8, 0, 2, 1)], [], [], [], [(1, 0), (2, 0)], 0, "a WSUM gate whose nbits is not the bit length of the sum of 2^shift"),
    "nbits = 25": ([(8, 0, 1, 25)] + [(9, i, 0, 0) for i in range(1, 25)], [], [], [], [(1, 24)], 0, "a WSUM gate with nbits > 24"),
    "head at the end": ([(0, 1, 2, 0), (8, 1, 3, 3)], [], [], [], _T, 0, _ORDER),
    "a bit record missing": ([(0, 1, 2, 0), (8, 1, 3, 3), (9, 1, 0, 0)], [], [], [], _T, 0, _ORDER),
    "a gate where a bit record belongs": ([(0, 1, 2, 0), (8, 1, 3, 3), (9, 1, 0, 0), (1, 1, 2, 0)], [], [], [], _T, 0, _ORDER),
    "bit records out of order": ([(0, 1, 2, 0), (8, 1, 3, 3), (9, 2, 0, 0), (9, 1, 0, 0)], [], [], [], _T, 0, _ORDER),
    "a bit record with an operand": ([(0, 1, 2, 0), (8, 1, 3, 3), (9, 1, 0, 0), (9, 2, 1, 0)], [], [], [], _T, 0, _ORDER),
    "a second head where a bit record belongs": ([(0, 1, 2, 0), (8, 1, 3, 3), (8, 1, 3, 3), (9, 1, 0, 0)], [], [], [], _T, 0, _ORDER),
    "WSUM_BIT first": ([(9, 1, 0, 0)], [], [], [], _T, 0, "a WSUM_BIT record without a head"),
    "one WSUM_BIT too many": (_OK[:4] + [(9, 3, 0, 0)], [], [], [], _T, 0, "a WSUM_BIT record without a head"),
    "unknown flag": (_OK, [], [], [], _T, 2, "unknown flag bits"),
    "op 10 (a case of mfh_circuit_create_ex)": ([(10, 1, 2, 0)], [], [], [], _T, 0, "unknown gate op"),
    "p twice (a case of mfh_circuit_create_out)": (_OK, [], [], [(3, 5), (3, 6)], _T, 0, "an output wire p given twice"),
    "assertion above nin + ngates": (_OK, [(10, 1)], [], [], _T, 0, "an assertion on wire 0 or above nin + ngates"),
}


def test_einval_cases(gpu_ctx_factory, mf):
    ctx = gpu_ctx_factory(mf.DEBUG)
    last = lambda: ctx.lib.mfh_last_error(ctx._h).decode()  # noqa: E731
    for flags in (0, 1):
        rc, h = _create_sum(ctx, 4, _OK, [(9, 0)], [(6, 7)], [(3, 8), (4, 9)], _T, flags)  # an output may be a sum bit; term 0 is unused
        assert rc == 0 and h.value, (flags, last())
        ctx.lib.mfh_circuit_destroy(h)
    for name, (program, asserts, equal, outputs, terms, flags, text) in SUM_CASES.items():
        for fl in (flags,) if flags else (0, 1):
            rc, h = _create_sum(ctx, 4, program, asserts, equal, outputs, terms, fl)
            assert rc == EINVAL and not h.value, (name, fl, rc)
            assert last() == "mfh_circuit_create_sum: " + text, (name, fl, last())
    rc, h = _create_sum(ctx, 4, _OK, [], [], [], _T, 0, null_terms=True)
    assert rc == EINVAL and not h.value and last() == "mfh_circuit_create_sum: terms without their array"
    # the older creates keep rejecting the new ops
    for op in (8, 9):
        arrs = [np.array([(op, 0, 1, 1)], dtype=np.uint32), np.zeros((0, 2), dtype=np.uint32)]
        h = ctypes.c_void_p(1)
        rc = ctx.lib.mfh_circuit_create_ex(ctx._h, 4, 1, ctypes.c_void_p(arrs[0].ctypes.data), 0, None, 0, None, 0, ctypes.byref(h))
        assert rc == EINVAL and not h.value and last() == "mfh_circuit_create_ex: unknown gate op"
        rc = ctx.lib.mfh_circuit_create_out(ctx._h, 4, 1, ctypes.c_void_p(arrs[0].ctypes.data), 0, None, 0, None, 0, None, 0, ctypes.byref(h))
        assert rc == EINVAL and not h.value and last() == "mfh_circuit_create_out: unknown gate op"


# ------------------------------------------------------------------ 3. no WSUM gate: the program of mfh_circuit_create_out
def test_no_sum_gate_is_create_out(gpu_ctx_factory, mf, C):
    from circuit_ex_ref import random_ex_circuit

    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    c = random_ex_circuit(np.random.default_rng(99), 6, 20, 1200, nasserts=2, nequal=2)
    for k in (40, 300, 900):
        c.output(C.Wire(k))
    cc = c.compile(p)
    nin = cc.lu + 20
    bits = np.random.default_rng(98).integers(0, 2, size=(300, nin), dtype=np.uint8)
    for flags, state, kind in ((0, "lds", "circuit_assign_out"), (1, "global", "circuit_assign_global_out")):
        ref = ctx.circuit_load(cc, state=state)
        assert not ref.sums and ref.outputs == 3
        for null in (False, True):  # nterms_total = 0 does not look at h_terms
            rc, h = _create_sum(ctx, nin, cc.program, cc.asserts, cc.equal, cc.outputs, [], flags, null_terms=null)
            assert rc == 0 and h.value
            prog = mf.CircuitProgram(ctx, nin, len(cc.program), h, state, True, 3)
            ctx.set_timing(True)
            w0, h0 = ctx.circuit_assign(prog, bits)
            assert ctx.timing_drain(kind)[0] == 1 and ctx.timing_drain(kind.replace("_out", "_sum"))[0] == 0  # the kernels of mfh_circuit_create_out
            ctx.set_timing(False)
            w1, h1 = ctx.circuit_assign(ref, bits)
            assert w0.tobytes() == w1.tobytes() and h0.tobytes() == h1.tobytes()
            prog.close()
        ref.close()
    # and a circuit with the gate, but only such a circuit, loads through the new create
    c2 = C.Circuit()
    x = c2.private(3)
    c2.wsum([(x[0], 0), (x[1], 0), (x[2], 1)])
    prog = ctx.circuit_load(c2.compile(p))
    assert prog.sums and prog.extended
    prog.close()


# ------------------------------------------------------------------ 4. long rows through both interpolators
def test_long_rows_through_both_interpolators(gpu_ctx_factory, mf, W):
    p = mf.Params(d=1152, m=1000)
    ctx = gpu_ctx_factory(p)
    w = W.Words()
    xs = w.private(8)
    s = w.sum(xs)                                    # rows of 128 + 19 + 1 and 131 + 19 + 1 entries
    w.sum([s, xs[0], w.const(0xFFFF00FF), xs[3]])    # the one wire 8 and 16 times in a row
    cc = w.c.compile(p)
    rp, wire, coef = cc.rows
    lens = np.diff(rp.astype(np.int64))
    assert int(lens.max()) == 151 and cc.nrows < p.d - 1
    dense = ctx.to_host(ctx.ssp_from_rows(cc.rows), np.uint32).reshape(p.m + 3, p.d)
    ctx.ssp_set_rows(cc.rows, lu_max=2)
    filled = ctx.to_host(ctx.ssp_rows_fill(0, p.m + 3), np.uint32).reshape(p.m + 3, p.d)
    assert np.array_equal(dense, filled)
    V = cr.values(p.d, p.m, cc.rows)  # V[i][j] = the sum of wire i's coefficients in row j (padding rows: v_0 = 1)
    pts = np.arange(p.d - 1, dtype=np.uint64) + np.uint64(2)
    used = sorted(set(wire.tolist()))
    for i in used + [cc.nwires + 1, p.m - 1]:
        assert np.array_equal(cr.horner(dense[1 + i].astype(np.uint64), pts), V[i]), i
    ctx.ssp_set_rows(None)


# ------------------------------------------------------------------ 5. SHA-256 at d = 2^16
def _flip(bits: bytes, bit: int) -> bytes:
    b = bytearray(bits)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def test_sha256_sum_two_pow_16(mf, C, W):
    import oracle_lib as ol
    from test_gpu_ssp_interp import SEED, _draws

    p = mf.Params(d=1 << 16, m=43690)
    st = W.Sha256Compress("iv", adds="sum")
    c = st.circuit
    cc = c.compile(p)
    lu, P = cc.lu, C.P
    assert lu == 256 and cc.nwires == 28114 and cc.nrows == 49588 and len(cc.outputs) == 256

    rng = np.random.default_rng(1604)
    nb = 255
    msgs = [b"abc"] + [bytes(rng.integers(0, 256, size=int(rng.integers(0, 56)), dtype=np.uint8).tolist()) for _ in range(nb - 1)]
    bits = np.stack([st.bits(W.sha256_pad(m)) for m in msgs])
    bits[1::2, :256] = rng.integers(0, 2, size=(len(bits[1::2]), 256), dtype=np.uint8)  # every other statement with garbage where the digest is computed

    ctx = mf.Context(p, 0)
    try:
        ctx.set_seed(SEED)
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        ctx.ssp_prepare(None)
        alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
        d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
        d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
        d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()

        prog = ctx.circuit_load(cc, state="auto")
        assert prog.state == "lds" and prog.sums and prog.outputs == 256
        ctx.set_timing(True)
        t0 = time.perf_counter()
        witness, holds = ctx.circuit_assign(prog, bits)
        call_ms = (time.perf_counter() - t0) * 1e3
        n, kernel_ms, _ = ctx.timing_drain("circuit_assign_sum")
        ctx.set_timing(False)
        print(f"circuit_assign, {nb} SHA-256 statements with sums: {call_ms:.2f} ms the first call, k_circuit_eval<true, true, true> {kernel_ms:.3f} ms in {n} launch")
        assert n == 1 and holds.all()
        for b in range(nb):
            assert st.digest_of(witness[b]) == hashlib.sha256(msgs[b]).digest(), b
        assert st.digest_of(witness[0]).hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
        for b in (0, 1, 254):
            assert witness[b].tobytes() == c.assign(bits[b, :256], bits[b, 256:], p), b
        prog.close()

        stmts = [witness[b].tobytes() for b in range(nb)]
        deltas, mags, signs = _draws(rng, nb)
        ctx.poly_exact_fallbacks()
        t0 = time.perf_counter()
        proofs = ctx.prove_batch_public(d_crs, None, lu, stmts, deltas, mags, signs).clone()
        ctx.sync()
        print(f"prove_batch_public, {nb} SHA-256 statements with sums at d = 2^16: {(time.perf_counter() - t0) * 1e3:.1f} ms (first call)")
        assert ctx.poly_exact_fallbacks() == 0
        vk = ctx.derive_vk(None, s, lu)
        ok = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, stmts), np.uint8)
        assert all(bool(x) for x in ok)
        # the statement with one digest bit flipped: rejected
        tamper = {0: 3, 77: 255}
        tampered = [_flip(x, tamper[b]) if b in tamper else x for b, x in enumerate(stmts)]
        ok2 = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, tampered), np.uint8)
        assert [bool(x) for x in ok2] == [b not in tamper for b in range(nb)]
        # a witness with one carry wire flipped (bit 16 and bit 17 of a lo gate of two rounds): its proof is rejected, its neighbours' are not
        heads = np.flatnonzero(cc.program[:, 0] == C.GATE_WSUM)
        nin = cc.nwires - len(cc.program)
        lo_gates = [int(g) for g in heads if int(cc.program[g, 3]) == 19][::2]  # the sums of 5 .. 8 words: lo, hi, lo, hi, ..
        bad = {1: nin + 1 + lo_gates[10] + 16, 3: nin + 1 + lo_gates[-1] + 17}
        forged = [_flip(stmts[b], bad[b] - 1) if b in bad else stmts[b] for b in range(5)]
        pr = ctx.prove_batch_public(d_crs, None, lu, forged, deltas[:5], mags[:5], signs[:5]).clone()
        ok3 = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, pr, forged), np.uint8)
        assert [bool(x) for x in ok3] == [b not in bad for b in range(5)]
    finally:
        ctx.close()
