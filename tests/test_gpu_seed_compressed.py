"""Seed-compressed encryption and decryption (k_encrypt_mm with its two finishing kernels, csrc/encmm.hip) against the oracle, bit for bit:

A. every launch plan of k_encrypt_mm -- the column-chunk counts that make a chunk 3 to 2114 k-steps long, so that the counter-span refresh (every 64 k-steps
   of a chunk) runs never, once on the chunk's last k-step (33 chunks at logq 736), and up to 33 times -- through mfh_encrypt_rows and mfh_decrypt_rows, every
   row compared; the plan that ran is read off the workspace the call reserved (it grows in 1 MiB steps: all the resolution there is without a getter);
B. mfh_decrypt_rows on crafted b (equal to, just below and just above the dot product, zero, all ones with bits above 2^(64 K), 2^(64 K) and its
   neighbour, the top word alone) against regev_decrypt in Python integers (seed_compressed_ref, pinned to the oracle on the CPU), and its argument errors;
C. stream block 2^32 (byte 2^36, where the counter's high word changes and the two sets of span constants differ in it) early in a row, deep in a row and
   exactly at a row start, through every call that builds span constants: mfh_encrypt_rows (both kernels), mfh_decrypt_rows, mfh_keystream,
   mfh_sample_rows, mfh_eval_rows (both kernels), mfh_eval_rows_multi (both layouts) and mfh_crs_expand + mfh_eval_rows_resident.

Not covered here: k_expand_mm.  mfh_crs_expand_mm takes no stream offset, but a small share of a large d reaches byte 2^36 through mfh_crs_expand_mm_share:
tests/test_gpu_expand_mm.py::test_counter_block_two_to_the_32 runs the kernel at the boundary.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import seed_compressed_ref as scr

pytestmark = pytest.mark.gpu

SEED = bytes((13 * i + 7) & 0xFF for i in range(40))
ROWS = (1, 2, 3, 33, 70, 513)  # both parities, a ragged 16-row MFMA tile, a ragged 4-row finish block, a second workgroup pair
CHUNKS = {736: (0, 1, 2, 32, 33, 64), 1472: (0, 1, 16, 32, 64)}
KSTEPS_PER_CHUNK = {736: {1: 2114, 2: 1057, 32: 67, 33: 65, 64: 34}, 1472: {1: 1409, 16: 265, 32: 133, 64: 67}}
B36 = 1 << 36


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


class World:
    """one modulus: context, key, messages and errors for up to 513 rows, and the references, each computed once and extended on demand"""

    def __init__(self, mf, ctx, oracle, logq):
        self.p = p = mf.Params(logq=logq, d=64, m=16)
        self.ctx, self.oracle = ctx, oracle
        ctx.set_seed(SEED)
        rng = np.random.default_rng(logq)
        self.sk = scr.extreme_key(rng, p)
        self.ski = scr.key_ints(self.sk)
        nmax = max(ROWS)
        self.msg = rng.integers(0, ol.P, size=nmax, dtype=np.uint64)
        self.msg[:3] = (0, 1, ol.P - 1)
        self.err = ol.rand_values(rng, nmax, p.L, 559)  # GAMMA_LOG_SIGMA + 3 bits (src/lwe.c:62)
        self.err[1] = 0
        self.err[2] = ol.int_to_limbs((1 << 559) - 1, p.L)
        self.b = rng.integers(0, 256, size=nmax * p.ctb, dtype=np.uint8)  # arbitrary b for the decryptions
        self.d_sk, self.d_msg, self.d_err, self.d_b = (ctx.to_device(x) for x in (self.sk, self.msg.astype(np.uint32), self.err, self.b))
        self._enc, self._dot = {}, {}

    def offsets(self, nrows=1):
        """block-aligned | mid-block (at logq 1472 every row then starts mid-block) | the offset of test_gpu_parity's encryption test; every row crosses spans of 256
        blocks.  The 513-row batches (row 512 is the only row of the second workgroup pair) run at the first two: that row's head is 0 at one and 8 at the other."""
        p = self.p
        return (0, 16 * 4099 + 8, 3 * p.ctr_ct + 8 * 1001)[: 2 if nrows > 70 else 3]

    def enc_ref(self, off, nrows):
        """ct_export(regev_encrypt2) of rows 0 .. nrows - 1 at stream offset off, by the oracle"""
        have = self._enc.setdefault(off, [])
        if len(have) < nrows:
            r = self.oracle.rng(SEED, off + len(have) * self.p.ctr_ct)
            for i in range(len(have), nrows):
                have.append(self.oracle.ct_export(self.p, self.oracle.encrypt(self.p, r, self.sk, int(self.msg[i]), self.err[i])))
        return b"".join(have[:nrows])

    def py_dots(self, off, nrows):
        """<sk, a_i> mod 2^(64 K) in Python integers (seed_compressed_ref.row_dots)"""
        have = self._dot.setdefault(off, [])
        if len(have) < nrows:
            have += scr.row_dots(self.oracle, self.p, SEED, off + len(have) * self.p.ctr_ct, nrows - len(have), self.ski)
        return have[:nrows]

    def dots(self, off, nrows):
        """the same numbers out of the oracle's encryptions, b = dot + e p + m mod 2^(64 K): what the batches of hundreds of rows are judged by (the Python sum
        takes milliseconds per row); test_reference_helper_equals_the_oracle holds the two against each other"""
        p, q = self.p, 1 << (64 * self.p.K)
        exp = self.enc_ref(off, nrows)
        return [(int.from_bytes(exp[p.ctb * i: p.ctb * (i + 1)], "little") - ol.limbs_to_int(self.err[i]) * ol.P - int(self.msg[i])) % q for i in range(nrows)]

    def dec_ref(self, off, nrows, b: bytes, dots=None):
        ctb = self.p.ctb
        return [scr.decrypt_b(b[ctb * i: ctb * i + ctb], d) for i, d in enumerate(self.dots(off, nrows) if dots is None else dots)]


@pytest.fixture(scope="module")
def worlds(gpu_ctx_factory, mf, oracle):
    made = {}

    def get(logq):
        if logq not in made:
            made[logq] = World(mf, gpu_ctx_factory(mf.Params(logq=logq, d=64, m=16)), oracle, logq)
        return made[logq]

    return get


def _encrypt(ctx, W, off, nrows, path, chunks=0):
    ctx.set_encrypt_path(path)
    ctx.set_encrypt_chunks(chunks)
    try:
        return ctx.to_host(ctx.encrypt_rows(off, nrows, W.d_sk, W.d_msg, W.d_err)).tobytes()
    finally:
        ctx.set_encrypt_chunks(0)
        ctx.set_encrypt_path(0)


def _decrypt_rows(ctx, W, off, nrows, d_b, chunks=0):
    ctx.set_encrypt_chunks(chunks)
    try:
        return [int(x) for x in ctx.to_host(ctx.decrypt_rows(off, nrows, W.d_sk, d_b), np.uint32)]
    finally:
        ctx.set_encrypt_chunks(0)


def _first_bad_row(got: bytes, exp: bytes, ctb):
    return next((i for i in range(len(exp) // ctb) if got[ctb * i: ctb * i + ctb] != exp[ctb * i: ctb * i + ctb]), None)


# ---------------------------------------------------------------- the judge, once more where it judges
@pytest.mark.parametrize("logq", [736, 1472])
def test_reference_helper_equals_the_oracle(worlds, oracle, logq):
    """regev_decrypt in Python integers == oracle.decrypt(oracle.ct_import(...)) on this file's key and offsets (tests/test_seed_compressed_ref_cpu.py holds the crafted cases)"""
    W = worlds(logq)
    p = W.p
    for off in W.offsets():
        assert W.py_dots(off, 3) == W.dots(off, 3)
        for i, dot in enumerate(W.py_dots(off, 2)):
            b = W.b[p.ctb * i: p.ctb * (i + 1)].tobytes()
            want = oracle.decrypt(p, W.sk, oracle.ct_import(p, oracle.rng(SEED, off + i * p.ctr_ct), b))
            assert scr.decrypt_b(b, dot) == want


# ---------------------------------------------------------------- A. every launch plan
@pytest.mark.parametrize("logq,chunks", [(q, c) for q in (736, 1472) for c in CHUNKS[q]])
def test_every_launch_plan_matches_the_oracle(gpu_ctx_factory, worlds, mf, logq, chunks):
    """mfh_encrypt_rows on the matrix-core kernel and mfh_decrypt_rows under a forced column-chunk count: every row of every batch equals the oracle's.
    The calls run in a context of their own, smallest batch first, so that after each call the workspace is exactly what the expected plan reserves."""
    W = worlds(logq)
    p = W.p
    if chunks:
        ksteps, kc, kpc = scr.enc_plan(p, max(ROWS), chunks)
        assert kpc == KSTEPS_PER_CHUNK[logq][chunks] and (kc == 3 if (logq, chunks) == (1472, 1) else kc >= chunks - 1)
        # what the workspace can tell apart at 513 rows: this plan from the default one, and the int32 floor (3 chunks at logq 1472) from its absence
        assert scr.enc_workspace_bytes(p, 513, kc) != scr.enc_workspace_bytes(p, 513, scr.enc_plan(p, 513)[1])
        if logq == 1472 and chunks < 3:
            assert scr.enc_workspace_bytes(p, 513, kc) != scr.enc_workspace_bytes(p, 513, scr.enc_plan(p, 513, chunks, honour_kc_min=False)[1])
    ctx = gpu_ctx_factory(p)
    try:
        ctx.set_seed(SEED)
        assert ctx.workspace_bytes() == 0
        want_ws = 0
        for nrows in ROWS:
            kc = scr.enc_plan(p, nrows, chunks)[1]
            want_ws = max(want_ws, scr.enc_workspace_bytes(p, nrows, kc))
            for off in W.offsets(nrows):
                got = _encrypt(ctx, W, off, nrows, 2, chunks)
                assert ctx.workspace_bytes() == want_ws, f"{nrows} rows: not the plan of {kc} chunks"
                exp = W.enc_ref(off, nrows)
                assert got == exp, f"encrypt: {nrows} rows at {off}: row {_first_bad_row(got, exp, p.ctb)}"
                dec = _decrypt_rows(ctx, W, off, nrows, W.d_b, chunks)
                assert ctx.workspace_bytes() == want_ws
                assert dec == W.dec_ref(off, nrows, W.b.tobytes()), f"decrypt: {nrows} rows at {off}"
    finally:
        ctx.set_encrypt_chunks(0)
        ctx.set_encrypt_path(0)
        ctx.close()


@pytest.mark.parametrize("logq", [736, 1472])
def test_valu_kernel_gives_the_same_bytes(worlds, logq):
    """k_encrypt on the inputs of the plan test: the oracle's bytes, hence the matrix-core kernel's"""
    W = worlds(logq)
    for nrows in ROWS:
        for off in W.offsets(nrows):
            got = _encrypt(W.ctx, W, off, nrows, 1)
            exp = W.enc_ref(off, nrows)
            assert got == exp, f"{nrows} rows at {off}: row {_first_bad_row(got, exp, W.p.ctb)}"


# ---------------------------------------------------------------- B. mfh_decrypt_rows on crafted b
def _crafted(p, dot, rnd: bytes):
    top, q = 1 << (8 * p.ctb), 1 << (64 * p.K)
    return [dot, (dot - 1) % top, dot + ol.P - 1, dot + ol.P, 0, top - 1, q, q - 1, 0xFFFFFFFF << (8 * p.ctb - 32), int.from_bytes(rnd, "little")]


@pytest.mark.parametrize("nrows", [1, 5, 37])
@pytest.mark.parametrize("logq", [736, 1472])
def test_decrypt_rows_on_crafted_b(worlds, logq, nrows):
    """b = the dot product (must give 0), one below it (negative before mod p), p - 1 and p above it, 0, all ones (bits above 2^704 at logq 736: b is taken
    whole), 2^(64 K) and 2^(64 K) - 1, the top word alone, random bytes -- rotated through the rows, so that every kind meets both parities and, at 37 rows, the ragged
    last finish block.  Expected values: regev_decrypt in Python integers."""
    W = worlds(logq)
    p, ctx = W.p, W.ctx
    off = W.offsets()[1]
    dots = W.py_dots(off, nrows)
    rng = np.random.default_rng(nrows)
    top = 1 << (8 * p.ctb)
    nk = len(_crafted(p, 0, b""))
    for shift in range(nk):
        rows = [(_crafted(p, dots[i], rng.bytes(p.ctb))[(i + shift) % nk] % top).to_bytes(p.ctb, "little") for i in range(nrows)]
        got = _decrypt_rows(ctx, W, off, nrows, ctx.to_device(np.frombuffer(b"".join(rows), dtype=np.uint8)))
        exp = [scr.decrypt_b(rows[i], dots[i]) for i in range(nrows)]
        assert got == exp, f"shift {shift}: rows {[i for i in range(nrows) if got[i] != exp[i]]}"
        for i in range(nrows):
            if (i + shift) % nk == 0:
                assert got[i] == 0  # b equal to the dot product


@pytest.mark.parametrize("logq", [736, 1472])
def test_decrypt_rows_recovers_edge_messages_and_agrees_with_full_ciphertexts(worlds, mf, logq):
    """messages {0, 1, p - 1} x errors {0, 2^559 - 1}, encrypted on the device: mfh_decrypt_rows returns them, and so does mfh_decrypt (both kernels) on the same rows
    assembled into full ciphertexts (the a part from mfh_sample_rows)"""
    import torch

    W = worlds(logq)
    p, ctx = W.p, W.ctx
    off = W.offsets()[2]
    msg = np.array([0, 1, ol.P - 1] * 2, dtype=np.uint32)
    err = np.zeros((6, p.L), dtype=np.uint64)
    err[3:] = ol.int_to_limbs((1 << 559) - 1, p.L)
    n = len(msg)
    for path in (1, 2):
        ctx.set_encrypt_path(path)
        try:
            c8 = ctx.encrypt_rows(off, n, W.d_sk, ctx.to_device(msg), ctx.to_device(err))
        finally:
            ctx.set_encrypt_path(0)
        assert _decrypt_rows(ctx, W, off, n, c8) == [int(x) for x in msg]
    cts = torch.zeros((n, p.n + 1, p.L * 8), dtype=torch.uint8, device=ctx.device)
    cts[:, : p.n] = ctx.sample_rows(off, n).view(n, p.n, p.L * 8)
    cts[:, p.n, : p.ctb] = c8.view(n, p.ctb)
    for path in (1, 2):
        ctx.set_decrypt_path(path)
        try:
            got = ctx.to_host(ctx.decrypt(W.d_sk, cts.reshape(-1), n), np.uint32)
        finally:
            ctx.set_decrypt_path(0)
        assert [int(x) for x in got] == [int(x) for x in msg], f"mfh_decrypt path {path}"


def test_decrypt_rows_argument_errors(gpu_ctx_factory, worlds, mf):
    W = worlds(736)
    p, ctx = W.p, W.ctx
    lib = mf.load_library()
    out = ctx.zeros(16)
    sk, b, o = (ctypes.c_void_p(t.data_ptr()) for t in (W.d_sk, W.d_b, out))
    EINVAL, EUNSUPPORTED = -1, -4
    assert lib.mfh_decrypt_rows(ctx._h, 0, 2, None, b, o) == EINVAL
    assert lib.mfh_decrypt_rows(ctx._h, 0, 2, sk, None, o) == EINVAL
    assert lib.mfh_decrypt_rows(ctx._h, 0, 2, sk, b, None) == EINVAL
    assert lib.mfh_decrypt_rows(None, 0, 2, sk, b, o) == EINVAL
    assert lib.mfh_decrypt_rows(ctx._h, 0, 0, None, None, None) == 0
    for off in (4, 1, 8 * 1001 + 7):
        assert lib.mfh_decrypt_rows(ctx._h, off, 2, sk, b, o) == EUNSUPPORTED
        assert b"multiples of 8" in lib.mfh_last_error(ctx._h)
    assert not ctx.to_host(out).any()  # none of the refused calls wrote
    unseeded = gpu_ctx_factory(p)
    try:
        assert lib.mfh_decrypt_rows(unseeded._h, 0, 2, sk, b, o) == EINVAL
        assert b"mfh_set_seed" in lib.mfh_last_error(unseeded._h)
        with pytest.raises(mf.MfhError, match="mfh_set_seed"):
            unseeded.decrypt_rows(0, 2, W.d_sk, W.d_b)
    finally:
        unseeded.close()


# ---------------------------------------------------------------- C. block 2^32 inside a row
NB = 5  # rows around the boundary; row 2 holds it
# bytes from the start of row 2 to byte 2^36: block 100 of the row, the row starting mid-block | block 1317 (k-step 329: five refreshes into a single chunk) | the row start
POSITIONS = {"early_head8": 16 * 100 + 8, "deep": 16 * (256 * 5 + 37), "row_start": 0}


def _boundary_off(p, pos):
    off = B36 - POSITIONS[pos] - 2 * p.ctr_ct
    assert off % 8 == 0 and off < B36 - p.ctr_ct and B36 - POSITIONS[pos] == off + 2 * p.ctr_ct < off + NB * p.ctr_ct
    return off


@pytest.mark.parametrize("pos", list(POSITIONS))
@pytest.mark.parametrize("logq", [736, 1472])
def test_block_2pow32_inside_a_row_encrypt_decrypt(worlds, logq, pos):
    W = worlds(logq)
    p, ctx = W.p, W.ctx
    off = _boundary_off(p, pos)
    if pos == "early_head8":
        assert (off + 2 * p.ctr_ct) % 16 == 8
    exp = W.enc_ref(off, NB)
    want = W.dec_ref(off, NB, W.b.tobytes(), W.py_dots(off, NB))
    for chunks in (0, 1, 33):  # the boundary in a chunk's first pair of constant sets | after refreshes of a whole-row chunk | 33: in a chunk of 65 k-steps
        got = _encrypt(ctx, W, off, NB, 2, chunks)
        assert got == exp, f"matrix-core kernel, {chunks} chunks: row {_first_bad_row(got, exp, p.ctb)}"
        assert _decrypt_rows(ctx, W, off, NB, W.d_b, chunks) == want, f"decrypt_rows, {chunks} chunks"
    got = _encrypt(ctx, W, off, NB, 1)
    assert got == exp, f"VALU kernel: row {_first_bad_row(got, exp, p.ctb)}"


@pytest.mark.parametrize("pos", list(POSITIONS))
@pytest.mark.parametrize("logq", [736, 1472])
def test_block_2pow32_inside_a_row_stream_and_eval(worlds, oracle, logq, pos):
    W = worlds(logq)
    p, ctx = W.p, W.ctx
    off = _boundary_off(p, pos)
    # the raw stream and the sampler
    lo = off + 2 * p.ctr_ct - 5000
    assert ctx.to_host(ctx.keystream(lo, p.ctr_ct + 10000)).tobytes() == oracle.keystream(SEED, lo, p.ctr_ct + 10000)
    assert ctx.to_host(ctx.keystream(B36 - 3, 40)).tobytes() == oracle.keystream(SEED, B36 - 3, 40)
    got = ctx.to_host(ctx.sample_rows(off, NB), np.uint64).reshape(NB, p.n, p.L)
    assert np.array_equal(got, oracle.sample_rows(p, SEED, off, NB))
    # eval_poly: the row kernels
    rng = np.random.default_rng(logq + len(pos))
    c8 = rng.integers(0, 256, size=NB * p.ctb, dtype=np.uint8)
    co = rng.integers(1, ol.P, size=(40, NB), dtype=np.uint64)
    co[1] = ol.P - 1
    d_c8, d_co = ctx.to_device(c8), ctx.to_device(co.astype(np.uint32))
    exp = {v: oracle.eval_poly(p, SEED, off, c8.tobytes(), co[v]) for v in (0, 1, 2, 39)}
    shape = exp[0].shape
    for path in ((0, 1) if logq == 736 else (0,)):
        ctx.set_eval_path(path)
        try:
            r0, r1 = ctx.eval_rows(off, NB, d_c8, d_co[: 4 * NB], d_co[4 * NB: 8 * NB])
        finally:
            ctx.set_eval_path(0)
        assert np.array_equal(ctx.to_host(r0, np.uint64).reshape(shape), exp[0]), f"eval path {path}"
        assert np.array_equal(ctx.to_host(r1, np.uint64).reshape(shape), exp[1]), f"eval path {path}"
    # ... the matrix-core kernels, regenerating the rows: 3 vectors (the 128-column layout at logq 736) and 40 (the 256-column layout)
    for nvec in (3, 40):
        got = ctx.to_host(ctx.eval_rows_multi(off, NB, d_c8, d_co, nvec), np.uint64).reshape(nvec, *shape)
        for v in (0, 1, 2, nvec - 1):
            assert np.array_equal(got[v], exp[v]), f"eval_rows_multi, {nvec} vectors: vector {v}"
    # ... and out of a row image expanded at this offset
    image = ctx.crs_expand(off, NB, d_c8)
    r0, r1 = ctx.eval_rows_resident(image, 0, NB, d_co[: 4 * NB], d_co[4 * NB: 8 * NB])
    assert np.array_equal(ctx.to_host(r0, np.uint64).reshape(shape), exp[0])
    assert np.array_equal(ctx.to_host(r1, np.uint64).reshape(shape), exp[1])
