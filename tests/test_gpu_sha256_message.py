"""GPU: the whole-message SHA-256 statement and the Merkle path statement at d = 2^17, through the device-memory witness kernel, the row check and
the row SSP.

1. words.Sha256Message(100), 33 statements: the digests circuit_assign computes equal hashlib's; mfh_ssp_rows_violations reports no violated row; with
   one gate wire flipped in one witness row that statement alone reports violations, and count and first equal the numpy reference; then
   setup_public, prove_batch_public on 4 statements and verify_public accept the true digests and reject a digest with one bit changed.
2. the same for words.MerklePath(2): 33 statements at random indices, roots against tests/sha256_ref.py, no violations, 4 statements proved."""
import hashlib

import numpy as np
import pytest

import rows_check_ref as rr
import sha256_ref as ref

pytestmark = pytest.mark.gpu

SEED = bytes((53 * i + 7) & 0xFF for i in range(40))


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def W():
    from c_lwe_snarks_amd import words

    return words


@pytest.fixture(scope="module")
def params(mf):
    return mf.Params(d=1 << 17, m=87381)


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory, params):
    c = gpu_ctx_factory(params)
    c.set_seed(SEED)
    return c


def _flip(bits: bytes, bit: int) -> bytes:
    b = bytearray(bits)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def _check_and_prove(ctx, mf, p, cc, witness, rng, what):
    """the row check on the witnesses (none violated; one flipped gate wire seen in its statement alone, as the reference sees it), then 4 statements
    proved and verified, and rejected with one bit of the public statement changed"""
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    nb, lu = len(witness), cc.lu
    ctx.ssp_set_rows(cc.rows, lu_max=lu)
    ctx.set_timing(True)
    count, first = ctx.ssp_rows_violations(witness)
    n, ms, total = ctx.timing_drain("ssp_rows_violations")
    ctx.set_timing(False)
    print(f"{what}: k_rows_violations, {cc.nrows} rows x {nb} statements: {ms:.3f} ms in {n} launch")
    assert (n, total) == (1, cc.nrows * nb)
    assert not count.any() and (first == rr.NONE).all()

    # one gate wire of statement 7 flipped: the wire in the middle of the program
    nin = cc.nwires - len(cc.program)
    wire = nin + 1 + len(cc.program) // 2
    rows = [witness[b].tobytes() for b in range(nb)]
    rows[7] = _flip(rows[7], wire - 1)
    count, first = ctx.ssp_rows_violations(rows)
    want_count, want_first = rr.violations(cc.rows, [rows[7]])
    print(f"{what}: wire {wire} of statement 7 flipped: count {int(count[7])}, first {int(first[7])} = {cc.row_source(int(first[7]))}")
    assert want_count[0] >= 1
    assert count.tolist() == [int(want_count[0]) if b == 7 else 0 for b in range(nb)]
    assert first.tolist() == [int(want_first[0]) if b == 7 else rr.NONE for b in range(nb)]
    assert cc.row_source(int(first[7]))[0] == "gate"  # (a bit row holds whatever the bit)

    ctx.ssp_prepare(None)
    alpha, beta, s = (int(x) for x in rng.integers(1, C.P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()
    stmts = [witness[b].tobytes() for b in range(4)]
    deltas = [int(x) for x in rng.integers(0, C.P, size=4, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(4)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(4)]
    ctx.poly_exact_fallbacks()
    proofs = ctx.prove_batch_public(d_crs, None, lu, stmts, deltas, mags, signs).clone()
    assert ctx.poly_exact_fallbacks() == 0
    vk = ctx.derive_vk(None, s, lu)
    ok = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, stmts), np.uint8)
    assert all(bool(x) for x in ok)
    tamper = {1: 0, 2: 255}
    tampered = [_flip(x, tamper[b]) if b in tamper else x for b, x in enumerate(stmts)]
    ok2 = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, tampered), np.uint8)
    assert [bool(x) for x in ok2] == [b not in tamper for b in range(4)]


def test_sha256_message_100_bytes(ctx, mf, W, params):
    p = params
    st = W.Sha256Message(100)
    cc = st.circuit.compile(p)
    assert (cc.nwires, cc.nrows, cc.lu) == (55746, 98436, 256)
    rng = np.random.default_rng(1811)
    nb = 33
    msgs = [rng.bytes(100) for _ in range(nb)]
    bits = np.stack([st.bits(m) for m in msgs])
    bits[1::2, :256] = rng.integers(0, 2, size=(len(bits[1::2]), 256), dtype=np.uint8)  # garbage where the digest is computed
    prog = ctx.circuit_load(cc, state="auto")
    assert prog.state == "global" and prog.sums and prog.outputs == 256
    witness, holds = ctx.circuit_assign(prog, bits)
    prog.close()
    assert holds.all()
    for b in range(nb):
        assert st.digest_of(witness[b]) == hashlib.sha256(msgs[b]).digest(), b
    assert witness[0].tobytes() == st.circuit.assign(bits[0, :256], bits[0, 256:], p)
    _check_and_prove(ctx, mf, p, cc, witness, rng, "Sha256Message(100)")


def test_merkle_path_depth_2(ctx, mf, W, params):
    p = params
    st = W.MerklePath(2)
    cc = st.circuit.compile(p)
    assert (cc.nwires, cc.nrows, cc.lu) == (57764, 102502, 256)
    rng = np.random.default_rng(1812)
    nb = 33
    cases = [(rng.bytes(32), [rng.bytes(32), rng.bytes(32)], int(rng.integers(0, 4))) for _ in range(nb)]
    assert {i for _, _, i in cases} == {0, 1, 2, 3}
    bits = np.stack([st.bits(*c) for c in cases])
    prog = ctx.circuit_load(cc, state="auto")
    assert prog.state == "global" and prog.sums and prog.outputs == 256
    witness, holds = ctx.circuit_assign(prog, bits)
    prog.close()
    assert holds.all()
    for b, (leaf, sibs, index) in enumerate(cases):
        assert st.root_of(witness[b]) == ref.merkle_root(leaf, sibs, index), b
    assert witness[0].tobytes() == st.circuit.assign(bits[0, :256], bits[0, 256:], p)
    _check_and_prove(ctx, mf, p, cc, witness, rng, "MerklePath(2)")
