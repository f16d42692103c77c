"""GPU: computed public outputs (mfh_circuit_create_out, the OUT = true kernels) and the SHA-256 compression statement proved end to end.

1. random extended programs with outputs, both kinds (LDS and device memory), nb in {1, 31, 32, 33, 255, 8193 (two LDS launches)}: witness rows and
   holds byte-identical to a numpy restatement and to Circuit.assign / holds, padding included, with random garbage at the outputs' input positions;
   the two kinds equal to each other; the launches counted under "circuit_assign_out" / "circuit_assign_global_out";
2. every MFH_EINVAL case of mfh_circuit_create_out, each by name with its own text, nothing made; nout = 0 is mfh_circuit_create_ex byte for byte;
3. circuits without outputs still load through the creates they loaded through before (CircuitProgram attributes and timing kinds);
4. d = 2^17, row SSP: 255 SHA-256 statements (chaining="iv": the "abc" block, then random one-block messages), witnesses and digests on the device, proved
   in one batch; every honest statement verifies, a flipped digest bit is rejected;
5. the same with a public chaining value (lu = 512): the second blocks of 24 two-block messages, chained from the device's own first-block digests;
   a flipped chaining bit and a flipped digest bit are rejected.

Device memory of 4 and 5: Params(d=1 << 17, m=87381) has a CRS of 2d + m = 349 525 rows -- 32 MB seed-compressed, and 47 GB as the expanded image
the batch prover streams (135 332 B a row).  Like the d = 2^16 and d = 2^20 tests these leave the batch image and the row slabs at their defaults:
mfh_prove_batch sizes the slabs from the free memory itself (one slab when 47 GB + 8 GB are free, more otherwise), and the result does not depend on
the count.  The row SSP keeps (lu + 2) d words of dense prefix (0.27 GB at lu = 512) and the rows; the witness kernel one 247 KB column per 32 statements."""
import ctypes
import hashlib
import time
from types import SimpleNamespace

import numpy as np
import pytest

from circuit_ex_ref import bitsliced_ex, random_ex_circuit

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


# ------------------------------------------------------------------ 1. random programs with outputs, both kinds
NPUB, NPRIV = 8, 16


@pytest.fixture(scope="module")
def mixed(C):
    """random_ex_circuit's 8 public and 16 private inputs and 1 500 gates of every kind; then 40 outputs on random gate wires, two on private inputs and
    one on a public input, with two more plain public inputs declared between them; two equalities and an assertion on inputs (they hold on 1 in 8
    statements)"""
    rng = np.random.default_rng(4321)
    c = random_ex_circuit(rng, NPUB, NPRIV, 1500, nasserts=0, nequal=0)
    nodes = len(c.compile(SimpleNamespace(d=1 << 15, m=21845)).wires)  # (fewer than 1 524: the constants are shared wires)
    extra = []
    for k, n in enumerate(rng.choice(np.arange(NPUB + NPRIV, nodes), size=40, replace=False).tolist()):
        c.output(C.Wire(n))
        if k in (7, 23):
            extra.append(c.public())
    c.output(C.Wire(NPUB + 3))
    c.output(C.Wire(NPUB + 3))  # the same source twice
    c.output(C.Wire(2))
    c.assert_same(C.Wire(NPUB + 1), C.Wire(NPUB + 9))
    c.assert_equal(C.Wire(5), 1)
    c.assert_same(extra[0], extra[1])
    return c


def reference(cc, bits, m):
    """witness rows and holds of a program with outputs, from the numpy restatement of the extended kernels: evaluate without the pairs' equalities (the
    input bit at p is garbage), then write wire w's bit at p"""
    pairs = {(int(p), int(w)) for p, w in cc.outputs}
    rest = np.array([e for e in cc.equal.tolist() if tuple(e) not in pairs], dtype=np.uint32).reshape(-1, 2)
    wit, holds = bitsliced_ex(SimpleNamespace(program=cc.program, asserts=cc.asserts, equal=rest), bits, m)
    for p, w in cc.outputs.tolist():
        bit = (wit[:, (w - 1) >> 3] >> ((w - 1) & 7)) & 1
        wit[:, (p - 1) >> 3] = (wit[:, (p - 1) >> 3] & ~np.uint8(1 << ((p - 1) & 7))) | (bit << ((p - 1) & 7)).astype(np.uint8)
    return wit, holds


@pytest.mark.parametrize("nb", [1, 31, 32, 33, 255, 8193])
def test_random_programs_with_outputs_both_kinds(gpu_ctx_factory, mf, mixed, nb):
    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    cc = mixed.compile(p)
    lu, nin = cc.lu, cc.lu + NPRIV
    assert lu == NPUB + 45 and len(cc.outputs) == 43 and len(cc.equal) == 45 and nin == cc.nwires - len(cc.program)
    assert {0, 1, 2, 3, 4, 5, 6, 7} <= set(cc.program[:, 0].tolist())
    rng = np.random.default_rng(nb)
    bits = rng.integers(0, 2, size=(nb, nin), dtype=np.uint8)  # garbage at the outputs' positions too
    lds = ctx.circuit_load(cc, state="lds")
    glb = ctx.circuit_load(cc, state="global")
    assert lds.extended and glb.extended and lds.outputs == glb.outputs == 43 and lds.state == "lds" and glb.state == "global"
    ctx.set_timing(True)
    w1, h1 = ctx.circuit_assign(lds, bits)
    w2, h2 = ctx.circuit_assign(glb, bits)
    counts = {k: ctx.timing_drain(k)[0] for k in ("circuit_assign_out", "circuit_assign_global_out", "circuit_assign_ex", "circuit_assign_global_ex")}
    ctx.set_timing(False)
    assert counts == {"circuit_assign_out": (nb + 8191) // 8192, "circuit_assign_global_out": 1, "circuit_assign_ex": 0, "circuit_assign_global_ex": 0}
    assert np.array_equal(w1, w2) and np.array_equal(h1, h2)
    ref_w, ref_h = reference(cc, bits, p.m)
    assert np.array_equal(w1, ref_w) and np.array_equal(h1, ref_h)
    # the inputs that are not outputs come back as given, the outputs as computed: clearing the garbage changes nothing
    clean = bits.copy()
    clean[:, cc.outputs[:, 0] - 1] = 0
    w3, h3 = ctx.circuit_assign(lds, clean)
    assert np.array_equal(w3, w1) and np.array_equal(h3, h1)
    for b in range(nb) if nb <= 255 else (0, 31, 32, 4095, 8191, 8192):
        pub, prv = bits[b, :lu].tolist(), bits[b, lu:].tolist()
        assert w1[b].tobytes() == mixed.assign(pub, prv, p), b
        assert bool(h1[b]) == mixed.holds(pub, prv), b
        assert mixed.outputs_of(w1[b]) == w1[b, :6].tobytes() + bytes([w1[b, 6] & 0x1F])  # lu = 53
    if nb >= 255:
        assert 0 < h1.sum() < nb
    lds.close()
    glb.close()


# ------------------------------------------------------------------ 2. MFH_EINVAL, and nout = 0
def _create_out(ctx, nin, program, asserts, equal, outputs, flags, null_outputs=False):
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1, k)) for a, k in ((program, 4), (asserts, 2), (equal, 2), (outputs, 2))]
    ptr = [ctypes.c_void_p(a.ctypes.data) for a in arrs]
    if null_outputs:
        ptr[3] = ctypes.c_void_p(0)
    h = ctypes.c_void_p(12345)
    rc = ctx.lib.mfh_circuit_create_out(ctx._h, nin, len(arrs[0]), ptr[0], len(arrs[1]), ptr[1], len(arrs[2]), ptr[2], len(arrs[3]), ptr[3], flags,
                                        ctypes.byref(h))
    return rc, h


_OK = [(0, 1, 2, 0), (4, 1, 2, 5), (5, 1, 2, 5)]  # nin = 4: wires 5, 6, 7; wires 3 and 4 are read by nothing
_P_TEXT = "an output wire p that is not an input wire (1 .. nin)"
_W_TEXT = "an output's source wire w is 0 or above nin + ngates"
# name -> (program, asserts, equal, outputs, flags, text)
OUT_CASES = {
    "p = 0": (_OK, [], [], [(0, 5)], 0, _P_TEXT),
    "p above nin": (_OK, [], [], [(5, 6)], 0, _P_TEXT),
    "w = 0": (_OK, [], [], [(3, 0)], 0, _W_TEXT),
    "w above nin + ngates": (_OK, [], [], [(3, 8)], 0, _W_TEXT),
    "w = p": (_OK, [], [], [(3, 3)], 0, "an output wire defined as itself"),
    "p twice": (_OK, [], [], [(3, 5), (4, 6), (3, 7)], 0, "an output wire p given twice"),
    "w is the p of a later pair": (_OK, [], [], [(4, 3), (3, 5)], 0, "an output's source wire w is itself an output wire"),
    "w is the p of an earlier pair": (_OK, [], [], [(3, 5), (4, 3)], 0, "an output's source wire w is itself an output wire"),
    "a gate reads p (a)": (_OK, [], [], [(1, 5)], 0, "a gate reads an output wire"),
    "a gate reads p (b)": (_OK, [], [], [(2, 7)], 0, "a gate reads an output wire"),
    "a MAJ reads p (c)": ([(4, 1, 2, 3), (5, 1, 2, 3)], [], [], [(3, 5)], 0, "a gate reads an output wire"),
    "a NOT reads p": ([(3, 4, 4, 0)], [], [], [(4, 5)], 0, "a gate reads an output wire"),
    "an assertion on p": (_OK, [(5, 1), (3, 1)], [], [(3, 5)], 0, "an assertion on an output wire"),
    "an equality of p with another wire": (_OK, [], [(3, 5), (3, 6)], [(3, 5)], 0, "an equality on an output wire other than its own pair's"),
    "an equality of another wire with p": (_OK, [], [(7, 3)], [(3, 5)], 0, "an equality on an output wire other than its own pair's"),
    "an equality of two output wires": (_OK, [], [(3, 4)], [(3, 5), (4, 5)], 0, "an equality on an output wire other than its own pair's"),
    "unknown flag": (_OK, [], [], [(3, 5)], 2, "unknown flag bits"),
    "op 8 (a case of mfh_circuit_create_ex)": ([(8, 1, 2, 0)], [], [], [(3, 5)], 0, "unknown gate op"),
    "equality a = b (a case of mfh_circuit_create_ex)": (_OK, [], [(6, 6)], [(3, 5)], 0, "an equality of a wire with itself"),
}


def test_einval_cases(gpu_ctx_factory, mf):
    ctx = gpu_ctx_factory(mf.DEBUG)
    last = lambda: ctx.lib.mfh_last_error(ctx._h).decode()  # noqa: E731
    for flags in (0, 1):  # accepted: the pair's own equality in either order, a source that is an input, one source for two outputs
        rc, h = _create_out(ctx, 4, _OK, [(7, 0)], [(3, 5), (6, 4), (1, 2)], [(3, 5), (4, 6)], flags)
        assert rc == 0 and h.value, (flags, last())
        ctx.lib.mfh_circuit_destroy(h)
        rc, h = _create_out(ctx, 4, _OK, [], [], [(3, 1), (4, 1)], flags)
        assert rc == 0 and h.value, (flags, last())
        ctx.lib.mfh_circuit_destroy(h)
    for name, (program, asserts, equal, outputs, flags, text) in OUT_CASES.items():
        for fl in (flags,) if flags else (0, 1):
            rc, h = _create_out(ctx, 4, program, asserts, equal, outputs, fl)
            assert rc == EINVAL and not h.value, (name, fl, rc)
            assert last() == "mfh_circuit_create_out: " + text, (name, fl, last())
    rc, h = _create_out(ctx, 4, _OK, [], [], [(3, 5)], 0, null_outputs=True)
    assert rc == EINVAL and not h.value and last() == "mfh_circuit_create_out: outputs without their array"
    # the LDS limit is the LDS kind's alone, as for mfh_circuit_create_ex
    big = gpu_ctx_factory(mf.Params(d=256, m=40000))
    for fl, want in ((0, EINVAL), (1, 0)):
        rc, h = _create_out(big, 32767 - 2, _OK, [], [], [(3, 32767 - 1)], fl)
        assert rc == want and bool(h.value) == (want == 0), fl
        if want:
            assert big.lib.mfh_last_error(big._h).decode() == "mfh_circuit_create_out: nin + ngates > MFH_CIRCUIT_MAX_WIRES (the wire state must fit 128 KiB of LDS)"
        else:
            big.lib.mfh_circuit_destroy(h)


def test_nout_zero_is_create_ex(gpu_ctx_factory, mf):
    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    c = random_ex_circuit(np.random.default_rng(99), 6, 20, 1200, nasserts=2, nequal=2)
    cc = c.compile(p)
    nin = 26
    bits = np.random.default_rng(98).integers(0, 2, size=(300, nin), dtype=np.uint8)
    for flags, state, kind in ((0, "lds", "circuit_assign_ex"), (1, "global", "circuit_assign_global_ex")):
        ex = ctx.circuit_load(cc, state=state)
        assert ex.extended and ex.outputs == 0
        for null in (False, True):  # nout = 0 does not look at h_outputs
            rc, h = _create_out(ctx, nin, cc.program, cc.asserts, cc.equal, [], flags, null_outputs=null)
            assert rc == 0 and h.value
            out0 = mf.CircuitProgram(ctx, nin, len(cc.program), h, state, True)
            ctx.set_timing(True)
            w0, h0 = ctx.circuit_assign(out0, bits)
            assert ctx.timing_drain(kind)[0] == 1 and ctx.timing_drain(kind.replace("_ex", "_out"))[0] == 0  # the kernels of mfh_circuit_create_ex
            ctx.set_timing(False)
            w1, h1 = ctx.circuit_assign(ex, bits)
            assert w0.tobytes() == w1.tobytes() and h0.tobytes() == h1.tobytes()
            out0.close()
        ex.close()


# ------------------------------------------------------------------ 3. circuits without outputs load as before
def test_circuits_without_outputs_keep_their_creates(gpu_ctx_factory, mf):
    from circuit_program_ref import bitsliced, random_circuit

    p = mf.DEFAULT
    ctx = gpu_ctx_factory(p)
    old = random_circuit(np.random.default_rng(77), 4, 30, 900, nasserts=3)
    ext = random_ex_circuit(np.random.default_rng(76), 4, 30, 900, nasserts=3, nequal=2)
    bits = np.random.default_rng(78).integers(0, 2, size=(70, 34), dtype=np.uint8)
    kinds = ("circuit_assign", "circuit_assign_global", "circuit_assign_ex", "circuit_assign_global_ex", "circuit_assign_out", "circuit_assign_global_out")
    for c, extended, ref in ((old, False, bitsliced), (ext, True, bitsliced_ex)):
        cc = c.compile(p)
        assert cc.outputs.shape == (0, 2)
        ref_w, ref_h = ref(cc, bits, p.m)
        for state in ("lds", "global"):
            prog = ctx.circuit_load(cc, state=state)
            assert prog.extended == extended and prog.state == state and prog.outputs == 0
            ctx.set_timing(True)
            w, h = ctx.circuit_assign(prog, bits)
            want = "circuit_assign" + ("_global" if state == "global" else "") + ("_ex" if extended else "")
            assert {k: ctx.timing_drain(k)[0] for k in kinds} == {k: int(k == want) for k in kinds}, (extended, state)
            ctx.set_timing(False)
            assert np.array_equal(w, ref_w) and np.array_equal(h, ref_h)
            prog.close()


# ------------------------------------------------------------------ 4, 5. SHA-256 at d = 2^17, row SSP
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


def _prove_and_verify(ctx, mf, C, cc, witness, rng, tamper, what):
    """register cc's rows, set up, prove every witness row in one batch, verify; then verify again with the statements of `tamper` (index -> bit) flipped"""
    from test_gpu_ssp_interp import SEED

    p, P, lu, nb = ctx.params, C.P, cc.lu, len(witness)
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
    print(f"prove_batch_public, {nb} {what} statements at d = 2^17: {(time.perf_counter() - t0) * 1e3:.1f} ms (first call)")
    vk = ctx.derive_vk(None, s, lu)
    ok = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, stmts), np.uint8)
    assert all(bool(x) for x in ok)
    tampered = list(stmts)
    for b, bit in tamper.items():
        assert bit < lu
        tampered[b] = _flip(stmts[b], bit)
    ok2 = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, tampered), np.uint8)
    assert [bool(x) for x in ok2] == [b not in tamper for b in range(nb)]


def test_sha256_two_pow_17(mf, C, W):
    p = mf.Params(d=1 << 17, m=87381)
    st = W.Sha256Compress("iv")
    c = st.circuit
    cc = c.compile(p)
    lu = cc.lu
    assert lu == 256 and cc.nwires == 61698 and cc.nrows == 122884 and len(cc.outputs) == 256

    rng = np.random.default_rng(1804)
    nb = 255
    msgs = [b"abc"] + [bytes(rng.integers(0, 256, size=int(rng.integers(0, 56)), dtype=np.uint8).tolist()) for _ in range(nb - 1)]
    bits = np.stack([st.bits(W.sha256_pad(m)) for m in msgs])
    assert bits.shape == (nb, 768) and not bits[:, :256].any()
    bits[1::2, :256] = rng.integers(0, 2, size=(len(bits[1::2]), 256), dtype=np.uint8)  # every other statement with garbage where the digest is computed

    ctx = mf.Context(p, 0)
    try:
        prog = ctx.circuit_load(cc, state="auto")
        assert prog.state == "global" and prog.extended and prog.outputs == 256
        ctx.set_timing(True)
        t0 = time.perf_counter()
        witness, holds = ctx.circuit_assign(prog, bits)
        call_ms = (time.perf_counter() - t0) * 1e3
        n, kernel_ms, _ = ctx.timing_drain("circuit_assign_global_out")
        ctx.set_timing(False)
        print(f"circuit_assign, {nb} SHA-256 statements: {call_ms:.2f} ms the first call, k_circuit_eval_global<true, true> {kernel_ms:.2f} ms in {n} launch")
        assert n == 1 and holds.all()
        for b in range(nb):
            assert st.digest_of(witness[b]) == hashlib.sha256(msgs[b]).digest(), b
        assert st.digest_of(witness[0]).hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
        for b in (0, 1, 254):
            assert witness[b].tobytes() == c.assign(bits[b, :256], bits[b, 256:], p), b
        prog.close()
        _prove_and_verify(ctx, mf, C, cc, witness, rng, {0: 3, 77: 255}, "SHA-256 (chaining value = IV)")
    finally:
        ctx.close()


def test_sha256_public_chaining_two_pow_17(mf, C, W):
    p = mf.Params(d=1 << 17, m=87381)
    st = W.Sha256Compress("public")
    c = st.circuit
    cc = c.compile(p)
    lu = cc.lu
    assert lu == 512 and cc.nwires == 61954 and cc.nrows == 123140 and len(cc.outputs) == 256

    rng = np.random.default_rng(1805)
    nb = 24
    msgs = [bytes(rng.integers(0, 256, size=int(rng.integers(56, 120)), dtype=np.uint8).tolist()) for _ in range(nb)]
    padded = [W.sha256_pad(m) for m in msgs]
    assert all(len(x) == 128 for x in padded)
    iv = b"".join(v.to_bytes(4, "big") for v in W.SHA256_IV)

    ctx = mf.Context(p, 0)
    try:
        prog = ctx.circuit_load(cc, state="auto")
        assert prog.state == "global" and prog.outputs == 256
        first, h1 = ctx.circuit_assign(prog, np.stack([st.bits(x[:64], iv) for x in padded]))
        mid = [st.digest_of(first[b]) for b in range(nb)]
        bits = np.stack([st.bits(x[64:], h) for x, h in zip(padded, mid)])
        witness, h2 = ctx.circuit_assign(prog, bits)
        assert h1.all() and h2.all()
        for b in range(nb):
            assert st.digest_of(witness[b]) == hashlib.sha256(msgs[b]).digest(), b
            assert c.outputs_of(witness[b])[:32] == np.packbits(W.pack(W.be_words(mid[b])), bitorder="little").tobytes()
        assert witness[5].tobytes() == c.assign(bits[5, :512], bits[5, 512:], p)
        prog.close()
        _prove_and_verify(ctx, mf, C, cc, witness, rng, {2: 9, 11: 256 + 100}, "SHA-256 (public chaining value)")  # a chaining bit, a digest bit
    finally:
        ctx.close()
