"""GPU: the library on a caller's stream, on its own stream, moved between streams, after other work in the same context, and after mfh_scrub_staging.

Every other GPU test runs on the legacy null stream of a context that has done little before: there the host-side copies and `.cpu()` calls order everything
against everything, and a launch or copy that slipped onto stream 0, a missing join of a side stream, a pointer kept across a regrow of the device scratch or
a scratch invariant lost by a reallocation all go unnoticed.  Here
  A. a context made on a non-blocking torch stream runs every entry point with inputs that a few milliseconds of unrelated work on that stream produce, and the
     results are read back on that stream alone (no device-wide wait anywhere);
  B. a context that keeps the library's own non-blocking stream (what a C caller gets) runs the headline calls;
  C. one context alternates between two non-blocking streams and the null stream (mfh_sync before each switch; mfh_sample_rows alone without);
  D. one context per stream kind runs each call-sized entry point at small, large, small, larger sizes, the entry points interleaved, so every shared scratch
     is regrown and handed back and forth;
  E. mfh_scrub_staging between two identical calls.
Expected values are the oracle's (oracle_lib.Oracle; proofs: oracle.prover at mf.DEBUG), the GMP products of oracle_lib.PolyKron, and the Python restatements
of the row SSP and the circuit program (circuit_ref, circuit_program_ref, Circuit.assign); every comparison is of bytes."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import circuit_ref
import oracle_lib as ol
from circuit_program_ref import bitsliced, random_circuit
from test_gpu_public_inputs import _clear_low

pytestmark = pytest.mark.gpu

SEED = bytes((17 * i + 9) & 0xFF for i in range(40))
NAMES = ["h", "hat_h", "hat_v", "v_w", "b_w"]
LU = 5
NPOOL = 64        # statements of the shared instance (the largest batch of section D)
EV_ROWS = 1400    # rows of the shared eval_rows operands (the largest size of section D)
ENC_ROWS = 600    # rows of the shared encryption operands: two parities, more than one 512-row workgroup pair
DEC_CTS = 300     # ciphertexts of the shared decryption operands: more than one 256-row workgroup
KS_CASES = [(0, 48), (0, 16), (92, 8), (5, 1), (15, 2), (16, 4096), (135240, 135240), (8863223880, 92 * 7), ((1 << 36) + 3, 1000), (12, 92 * 1470 + 5)]


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def threads():
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:  # (the oracle's calls release the GIL)
        yield ex


# ---------------------------------------------------------------------------------------------------------------- the reference side, computed once
def _bit(bits, i):
    return (bits[i >> 3] >> (i & 7)) & 1


class _Prims:
    """operands and oracle results of the primitives at one parameter set, each computed on first use and never changed"""

    def __init__(self, oracle, threads, p, tag):
        self.o, self.ex, self.p = oracle, threads, p
        rng = np.random.default_rng(7000 + tag)
        self.ev_off = p.ctr_as + 3 * p.ctr_ct
        self.ev_c8 = rng.integers(0, 256, size=EV_ROWS * p.ctb, dtype=np.uint8)
        self.ev_co = rng.integers(0, ol.P, size=(2, EV_ROWS), dtype=np.uint64)
        self.ev_co[0, 1::7] = 0
        self.ev_co[:, 3] = 0          # a row with all-zero coefficients: skipped on the GPU
        self.ev_co[1, 2] = ol.P - 1
        self.ev_co[:, 0] |= 1         # (the one-row evaluation has something to do)
        self.acc = ol.rand_values(rng, 2 * (p.n + 1), p.L, 64 * p.K).reshape(2, p.n + 1, p.L)  # reduced accumulators
        self.sk = ol.rand_values(rng, p.n, p.L, p.logq)
        self.sk[0] = ol.int_to_limbs((1 << p.logq) - 1, p.L)
        self.sk[1] = 0
        self.enc_off = 3 * p.ctr_ct + 8 * 1001  # 8 mod 16, and the rows cross a 256-block counter span
        self.msg = rng.integers(0, ol.P, size=ENC_ROWS, dtype=np.uint64)
        self.err = ol.rand_values(rng, ENC_ROWS, p.L, 559)
        self.cts = ol.rand_values(rng, DEC_CTS * (p.n + 1), p.L, p.logq).reshape(DEC_CTS, p.n + 1, p.L)  # unreduced b, as after a raw ct_import
        self.cts[0, : p.n] = ol.int_to_limbs((1 << p.logq) - 1, p.L)
        self.cts[1, : p.n] = 0
        self._eval, self._enc, self._dec, self._decrows = {}, None, None, None

    def eval(self, nrows, nvec):
        """eval_poly of rows [0, nrows) of the shared operands for coefficient vectors 0 .. nvec - 1"""
        p = self.p
        todo = [(nrows, v) for v in range(nvec) if (nrows, v) not in self._eval]
        for k, r in zip(todo, self.ex.map(lambda k: self.o.eval_poly(p, SEED, self.ev_off, self.ev_c8[: k[0] * p.ctb].tobytes(), self.ev_co[k[1], : k[0]]), todo)):
            self._eval[k] = r
        return [self._eval[(nrows, v)] for v in range(nvec)]

    def eval_one(self, row, coef, seed=SEED):
        """the shared operands' row `row` alone, times coef"""
        p = self.p
        return self.o.eval_poly(p, seed, self.ev_off + row * p.ctr_ct, self.ev_c8[row * p.ctb:(row + 1) * p.ctb].tobytes(), np.array([coef], dtype=np.uint64))

    def enc(self, nrows):
        """regev_encrypt2 + ct_export of rows [0, nrows): a prefix of the ENC_ROWS rows (row i depends on i alone)"""
        p = self.p
        if self._enc is None:
            r = self.o.rng(SEED, self.enc_off)
            self._enc = np.frombuffer(b"".join(self.o.ct_export(p, self.o.encrypt(p, r, self.sk, int(self.msg[i]), self.err[i])) for i in range(ENC_ROWS)),
                                      dtype=np.uint8)
        return self._enc[: nrows * p.ctb]

    def dec(self, count):
        if self._dec is None:
            self._dec = np.array(list(self.ex.map(lambda i: self.o.decrypt(self.p, self.sk, self.cts[i]), range(DEC_CTS))), dtype=np.uint32)
        return self._dec[:count]

    def dec_rows(self, nrows):
        """regev_decrypt of the imported rows of enc(): ct_import regenerates a from the stream"""
        p = self.p
        if self._decrows is None:
            r = self.o.rng(SEED, self.enc_off)
            c8 = self.enc(ENC_ROWS).tobytes()
            self._decrows = np.array([self.o.decrypt(p, self.sk, self.o.ct_import(p, r, c8[i * p.ctb:(i + 1) * p.ctb])) for i in range(ENC_ROWS)], dtype=np.uint32)
            assert np.array_equal(self._decrows.astype(np.uint64), self.msg)  # (the oracle's own round trip)
        return self._decrows[:nrows]


class _Instance:
    """one mf.DEBUG instance (SSP, keys, the oracle's CRS) with NPOOL statements; the oracle's proofs are computed on first use, on threads"""

    def __init__(self, oracle, threads, p):
        self.o, self.ex, self.p = oracle, threads, p
        rng = np.random.default_rng(20261)
        nbytes = (p.m + 7) // 8
        self.wit = rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()
        self.ssp = oracle.ssp_from_tape(p, rng.integers(0, 256, size=p.m * 8 * p.d, dtype=np.uint8), self.wit)
        self.alpha, self.beta, self.s = (int(x) for x in rng.integers(1, ol.P, size=3, dtype=np.uint64))
        self.sk = ol.rand_values(rng, p.n, p.L, p.logq)
        self.etape = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
        self.crs = oracle.setup(p, SEED, self.ssp, self.alpha, self.beta, self.s, self.sk, self.etape)
        self.c8 = np.concatenate([self.crs["s"], self.crs["as_"], self.crs["t"], self.crs["v"][: (p.m - 1) * p.ctb]])  # stream order
        # every third statement is a random input that does not satisfy the SSP (Euclidean division behind the failed exact-division check)
        self.bits = [self.wit if b % 3 != 2 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for b in range(NPOOL)]
        self.deltas = [int(x) for x in rng.integers(0, ol.P, size=NPOOL, dtype=np.uint64)]
        self.mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(NPOOL)]
        self.signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(NPOOL)]
        self._proofs, self._zero = {}, {}

    def args(self, idx):
        idx = list(idx)
        return [self.bits[b] for b in idx], [self.deltas[b] for b in idx], [self.mags[b] for b in idx], [self.signs[b] for b in idx]

    def _prove(self, b, bits):
        tape = b"".join(self.mags[b][80 * k: 80 * k + 80] + self.signs[b][k: k + 1] for k in range(5))
        return self.o.prover(self.p, self.crs, self.ssp, bits, self.deltas[b], tape, 80, want_pre=False)["proof"]

    def proofs(self, idx):
        """the oracle's prover() for the statements idx: [len(idx)][5][n + 1][L]"""
        idx = list(idx)
        todo = [b for b in idx if b not in self._proofs]
        for b, r in zip(todo, self.ex.map(lambda b: self._prove(b, self.bits[b]), todo)):
            self._proofs[b] = r
        return np.stack([self._proofs[b] for b in idx])

    def public_proofs(self, idx):
        """the proofs with bits [0, LU) public, by the composition identity of test_gpu_public_inputs.py on the oracle's proofs: h, hat_h, hat_v of the
        oracle's prover() on the full bits, v_w and b_w of the oracle's prover() on the bits with the public ones cleared (neither reads rows v[0, LU))"""
        idx = list(idx)
        full = self.proofs(idx)
        todo = [b for b in idx if b not in self._zero]
        for b, r in zip(todo, self.ex.map(lambda b: self._prove(b, _clear_low(self.bits[b], LU)), todo)):
            self._zero[b] = r
        return np.stack([np.concatenate([full[k][:3], self._zero[b][3:]]) for k, b in enumerate(idx)])

    def accepts(self, proof):
        return self.o.verifier(self.p, self.ssp, self.alpha, self.beta, self.s, self.sk, np.ascontiguousarray(proof))

    def vk(self):
        ssp = self.ssp.reshape(self.p.m + 3, self.p.d)
        return [self.o.poly_eval(ssp[0], self.s)] + [self.o.poly_eval(ssp[1 + i], self.s) for i in range(LU + 1)]

    def accepts_public(self, u, proof):
        """verifier() with the statement u (src/snark.c:192-250 with the public wires' v_i(s) added into v(s)), on the oracle's decryptions"""
        h_s, hath_s, hatv_s, w_s, b_s = (self.o.decrypt(self.p, self.sk, np.ascontiguousarray(proof[k])) for k in range(5))
        vk = self.vk()
        v_s = (vk[1] + w_s + sum(vk[1 + i] for i in range(1, LU + 1) if _bit(u, i - 1))) % ol.P
        return (h_s * self.alpha % ol.P == hath_s and v_s * self.alpha % ol.P == hatv_s and (v_s * v_s - 1 - h_s * vk[0]) % ol.P == 0
                and w_s * self.beta % ol.P == b_s)


@pytest.fixture(scope="module")
def inst(oracle, threads, mf):
    return _Instance(oracle, threads, mf.DEBUG)


@pytest.fixture(scope="module")
def prims(oracle, threads, mf):
    return {"debug": _Prims(oracle, threads, mf.DEBUG, 0), "wide": _Prims(oracle, threads, mf.Params(logq=1472, d=64, m=16), 1)}


@pytest.fixture(scope="module")
def circ(mf):
    """a circuit of 45 gates with three assertions (some statements violate them) and 70 + 8193 random inputs, with the Python results"""
    p = mf.DEBUG
    rng = np.random.default_rng(45)
    c = random_circuit(rng, 3, 12, 45, nasserts=3, interleave=True)
    cc = c.compile(p)
    bits = rng.integers(0, 2, size=(8193, 15), dtype=np.uint8)
    wit, holds = bitsliced(cc, bits, p.m)
    for b in list(range(40)) + [8191, 8192]:  # the numpy restatement against Circuit.assign / holds itself
        assert wit[b].tobytes() == c.assign(bits[b, :3].tolist(), bits[b, 3:].tolist()) and bool(holds[b]) == c.holds(bits[b, :3].tolist(), bits[b, 3:].tolist())
    assert holds.any() and not holds.all()
    return dict(c=c, cc=cc, bits=bits, wit=wit, holds=holds)


# ---------------------------------------------------------------------------------------------------------------- streams
class _Run:
    """a context and the torch stream it runs on (None: the null stream)"""

    def __init__(self, ctx, stream):
        self.ctx, self.stream = ctx, stream


@contextlib.contextmanager
def _on(run):
    """torch's current stream is the run's; a non-blocking run asserts its premise first, so that no test silently degenerates to the null stream"""
    import torch

    if run.stream is None:
        assert torch.cuda.current_stream().cuda_stream == 0
        yield run.ctx
        return
    with torch.cuda.stream(run.stream):
        assert run.stream.cuda_stream != 0
        assert torch.cuda.current_stream() == run.stream
        yield run.ctx


_DELAY = {}  # stream handle -> the 128 MB tensor the delay passes run over; owned by the fixture below


@pytest.fixture(scope="module", autouse=True)
def _delay_buffers():
    """the delay tensors live as long as this module's tests and are freed with them"""
    yield
    _DELAY.clear()


def _busy(ctx):
    """queue unrelated work on the current stream: 48 passes over 128 MB (by HBM bandwidth an estimated 3 ms; not a measured figure).  Returns the tensor
    the passes ran over.  A call queued behind it on the same stream starts late; one that slipped onto another stream runs and ends ahead of it."""
    import torch

    key = torch.cuda.current_stream().cuda_stream
    if key not in _DELAY:
        _DELAY[key] = torch.zeros(1 << 25, dtype=torch.float32, device=ctx.device)
    x = _DELAY[key]
    for _ in range(24):
        x.mul_(0.5).add_(1.0)  # (stays in [0, 2])
    return x


def _late(ctx, arr):
    """arr on the device as the OUTPUT of unrelated work on the current stream: the tensor is first filled with 0x5A, then _busy's passes run, then a
    device op that depends on their result writes the bytes.  A kernel or copy that ignores the stream's order reads the filler."""
    import torch

    t = ctx.to_device(arr)
    out = torch.full_like(t, 0x5A)
    x = _busy(ctx)
    gate = (x[:1] < 0).to(torch.uint8)  # 0, known when the passes are done
    torch.bitwise_xor(t, gate, out=out)
    return out


def _u32(ctx, arr):
    return _late(ctx, np.ascontiguousarray(arr, dtype=np.uint32))


def _make_run(factory, p, stream, seed=SEED):
    import torch

    if stream is None:
        c = factory(p)
    else:
        with torch.cuda.stream(stream):
            c = factory(p)
    c.set_seed(seed)
    return _Run(c, stream)


@pytest.fixture(scope="module")
def run(gpu_ctx_factory, mf):
    """section A: mf.DEBUG on a non-blocking stream; Context.__init__ picks torch's current stream up"""
    import torch

    return _make_run(gpu_ctx_factory, mf.DEBUG, torch.cuda.Stream())


@pytest.fixture(scope="module")
def runs(run, gpu_ctx_factory, mf):
    import torch

    return {"debug": run, "wide": _make_run(gpu_ctx_factory, mf.Params(logq=1472, d=64, m=16), torch.cuda.Stream())}


@pytest.fixture(scope="module")
def ssp_on(run, inst):
    """the instance's SSP uploaded and prepared on the run's stream"""
    with _on(run) as ctx:
        d_ssp = ctx.ssp_upload(inst.ssp)
        ctx.ssp_prepare(d_ssp)
    return d_ssp


def _ct(ctx, t, shape):
    return ctx.to_host(t, np.uint64).reshape(shape)


def _check_proofs(got, exp, what=""):
    assert got.shape == exp.shape
    for b in range(len(exp)):
        for k in range(5):
            assert np.array_equal(got[b, k], exp[b, k]), f"{what}: proof {b}, {NAMES[k]} differs from the oracle's"


def _prove(ctx, inst, d_crs, d_ssp, b):
    p = inst.p
    return _ct(ctx, ctx.prove(d_crs, d_ssp, inst.bits[b], inst.deltas[b], inst.mags[b], inst.signs[b]), (1, 5, p.n + 1, p.L))


def _prove_batch(ctx, inst, d_crs, d_ssp, n, sync=False):
    p = inst.p
    out = ctx.prove_batch(d_crs, d_ssp, *inst.args(range(n)))
    if sync:
        ctx.sync()
    return _ct(ctx, out, (n, 5, p.n + 1, p.L))


# ================================================================================================================ A. a caller's non-blocking stream
@pytest.mark.parametrize("which", ["debug", "wide"])
def test_a_keystream_and_sampler(runs, prims, oracle, which):
    R = prims[which]
    p = R.p
    with _on(runs[which]) as ctx:
        # (no device input to delay: the unrelated work is queued in front of the call itself, so a launch that slipped onto another stream would be
        # overtaken or overwritten by the stream's own work rather than simply finish before the readback)
        for off, n in KS_CASES:
            _busy(ctx)
            assert ctx.to_host(ctx.keystream(off, n)).tobytes() == oracle.keystream(SEED, off, n), (off, n)
        for off, nrows in [(0, 1), (p.ctr_ct, 3), (8863223880, 1)]:
            _busy(ctx)
            got = ctx.to_host(ctx.sample_rows(off, nrows), np.uint64).reshape(nrows, p.n, p.L)
            assert np.array_equal(got, oracle.sample_rows(p, SEED, off, nrows)), (off, nrows)


@pytest.mark.parametrize("which", ["debug", "wide"])
def test_a_ciphertext_algebra(runs, prims, oracle, which):
    R = prims[which]
    p = R.p
    rng = np.random.default_rng(31)
    a, b = R.cts[5], R.cts[6]
    shape = a.shape
    with _on(runs[which]) as ctx:
        assert np.array_equal(_ct(ctx, ctx.ct_add(_late(ctx, a), _late(ctx, b)), shape), oracle.ct_add(p, a, b))
        for x in (1, 0xFFFFFFFA):
            assert np.array_equal(_ct(ctx, ctx.ct_mul_ui(_late(ctx, a), x), shape), oracle.ct_mul_ui(p, a, x)), x
            rop = _late(ctx, R.acc[0])
            ctx.ct_addmul_ui(rop, _late(ctx, a), x)
            assert np.array_equal(_ct(ctx, rop, shape), oracle.ct_addmul_ui(p, R.acc[0], a, x)), x
        # mpz_add_dotp at length 257: one lane of the 256 takes two terms
        va, vb = ol.rand_values(rng, 257, p.L, p.logq), ol.rand_values(rng, 257, p.L, p.logq)
        va[0] = vb[0] = ol.int_to_limbs((1 << p.logq) - 1, p.L)
        rop0 = ol.rand_values(rng, 1, p.L, p.logq)[0]
        d_rop = _late(ctx, rop0)
        ctx.add_dotp(d_rop, _late(ctx, va), _late(ctx, vb), 257)
        assert np.array_equal(ctx.to_host(d_rop, np.uint64), oracle.add_dotp(p, rop0, va, vb))
        # ct_smudge: the smudging terms go through the context's pinned staging
        cts = R.acc.copy()
        mags = rng.integers(0, 256, size=2 * 80, dtype=np.uint8).tobytes()
        d = _late(ctx, cts)
        ctx.ct_smudge(d, 2, mags, 80, bytes([1, 0]))
        got = _ct(ctx, d, cts.shape)
        for i in range(2):
            exp, _ = oracle.ct_smudge(p, cts[i], mags[80 * i: 80 * i + 80], [1, 0][i])
            assert np.array_equal(got[i], exp), i


def _eval_case(ctx, R, oracle, nrows, nvec, acc):
    p = R.p
    shape = (p.n + 1, p.L)
    exp = R.eval(nrows, nvec)
    d_c8 = _late(ctx, R.ev_c8[: nrows * p.ctb])
    d_co = [_u32(ctx, R.ev_co[v, :nrows]) for v in range(nvec)]
    rops = [_late(ctx, R.acc[v]) if acc else None for v in range(2)]
    r = ctx.eval_rows(R.ev_off, nrows, d_c8, d_co[0], d_co[1] if nvec > 1 else None, rop0=rops[0], rop1=rops[1] if nvec > 1 else None, accumulate=acc)
    for v in range(nvec):
        want = oracle.ct_add(p, R.acc[v], exp[v]) if acc else exp[v]  # eval_poly accumulates into rop (src/lwe.c:183)
        assert np.array_equal(_ct(ctx, r[v], shape), want), f"{nrows} rows, vector {v} of {nvec}, accumulate={acc}"


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("nvec", [1, 2])
@pytest.mark.parametrize("nrows", [37, 700])
@pytest.mark.parametrize("path", [0, 1])  # 0 = tile kernel (k_eval), 1 = wave-autonomous kernel (k_eval_w)
def test_a_eval_rows(run, prims, oracle, path, nrows, nvec, acc):
    with _on(run) as ctx:
        ctx.set_eval_path(path)
        try:
            _eval_case(ctx, prims["debug"], oracle, nrows, nvec, acc)
        finally:
            ctx.set_eval_path(0)


@pytest.mark.parametrize("nrows", [37, 700])
def test_a_eval_rows_logq1472(runs, prims, oracle, nrows):
    with _on(runs["wide"]) as ctx:
        _eval_case(ctx, prims["wide"], oracle, nrows, 2, False)
        _eval_case(ctx, prims["wide"], oracle, nrows, 2, True)


def test_a_resident_rows(run, prims):
    """mfh_crs_expand + mfh_eval_rows_resident: the rows expanded once, then multiplied out of the image"""
    R = prims["debug"]
    p = R.p
    nrows = 37
    exp = R.eval(nrows, 2)
    with _on(run) as ctx:
        image = ctx.crs_expand(R.ev_off, nrows, _late(ctx, R.ev_c8[: nrows * p.ctb]))
        r0, r1 = ctx.eval_rows_resident(image, 0, nrows, _u32(ctx, R.ev_co[0, :nrows]), _u32(ctx, R.ev_co[1, :nrows]))
        assert np.array_equal(_ct(ctx, r0, exp[0].shape), exp[0]) and np.array_equal(_ct(ctx, r1, exp[1].shape), exp[1])


@pytest.fixture(scope="module")
def as_region(inst, oracle, threads):
    """three coefficient vectors over the instance's AS region and the oracle's eval_poly of each"""
    p = inst.p
    co = np.random.default_rng(3).integers(0, ol.P, size=(3, p.d), dtype=np.uint64)
    co[0, 5] = 0
    exp = list(threads.map(lambda v: oracle.eval_poly(p, SEED, p.ctr_as, inst.crs["as_"].tobytes(), co[v]), range(3)))
    return co.astype(np.uint32), np.stack(exp)


@pytest.mark.parametrize("image", [False, True])
def test_a_eval_rows_multi(run, inst, as_region, image):
    """three vectors over p.d rows on the matrix cores: regenerating the rows, and (image) streaming them out of mfh_crs_expand_mm's image"""
    p = inst.p
    co, exp = as_region
    with _on(run) as ctx:
        d_crs = _late(ctx, inst.c8)
        if image:
            ctx.set_resident_mm(ctx.crs_expand_mm(d_crs))
        try:
            got = _ct(ctx, ctx.eval_rows_multi(p.ctr_as, p.d, d_crs[p.d * p.ctb:], _late(ctx, co), 3), (3, p.n + 1, p.L))
        finally:
            ctx.set_resident_mm(None)
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("which,path,nrows", [("debug", 1, 33), ("debug", 2, 33), ("debug", 1, ENC_ROWS), ("debug", 2, ENC_ROWS), ("wide", 1, 33), ("wide", 2, 33)])
def test_a_encrypt_rows(runs, prims, which, path, nrows):
    """path 1 = VALU kernel, 2 = matrix-core kernel"""
    R = prims[which]
    with _on(runs[which]) as ctx:
        ctx.set_encrypt_path(path)
        try:
            got = ctx.to_host(ctx.encrypt_rows(R.enc_off, nrows, _late(ctx, R.sk), _u32(ctx, R.msg[:nrows]), _late(ctx, R.err[:nrows])))
        finally:
            ctx.set_encrypt_path(0)
        assert np.array_equal(got, R.enc(nrows))


@pytest.mark.parametrize("count", [37, DEC_CTS])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("which", ["debug", "wide"])
def test_a_decrypt(runs, prims, which, path, count):
    R = prims[which]
    with _on(runs[which]) as ctx:
        ctx.set_decrypt_path(path)
        try:
            got = ctx.to_host(ctx.decrypt(_late(ctx, R.sk), _late(ctx, R.cts[:count]), count), np.uint32)
        finally:
            ctx.set_decrypt_path(0)
        assert np.array_equal(got, R.dec(count))


def test_a_decrypt_rows(run, prims):
    R = prims["debug"]
    with _on(run) as ctx:
        got = ctx.to_host(ctx.decrypt_rows(R.enc_off, 70, _late(ctx, R.sk), _late(ctx, R.enc(70))), np.uint32)
        assert np.array_equal(got, R.dec_rows(70))


def test_a_ssp_upload_and_polynomials(run, ssp_on, inst, oracle):
    """mfh_ssp_upload of arbitrary uint64 values (reduced mod p on the way), mfh_witness_poly, mfh_poly_mul, mfh_poly_h"""
    p = inst.p
    rng = np.random.default_rng(61)
    raw = rng.integers(0, 1 << 63, size=(p.m + 3) * p.d, dtype=np.uint64)
    red = (raw % np.uint64(ol.P)).reshape(p.m + 3, p.d)
    bits = rng.integers(0, 256, size=(p.m + 7) // 8, dtype=np.uint8).tobytes()
    delta = 0xDEADBEE
    w = (red[0].astype(object) * delta) % ol.P
    for i in range(1, p.m):
        if _bit(bits, i - 1):
            w = (w + red[i + 1].astype(object)) % ol.P
    a = rng.integers(0, ol.P, size=100, dtype=np.uint64)
    b = rng.integers(0, ol.P, size=511, dtype=np.uint64)
    a[0] = b[-1] = ol.P - 1
    v = rng.integers(0, ol.P, size=p.d, dtype=np.uint64)
    t = rng.integers(0, ol.P, size=p.d, dtype=np.uint64)
    with _on(run) as ctx:
        d_ssp = ctx.ssp_upload(raw)
        assert np.array_equal(ctx.to_host(d_ssp, np.uint32).reshape(p.m + 3, p.d), red.astype(np.uint32))
        assert np.array_equal(ctx.to_host(ctx.witness_poly(d_ssp, bits, delta), np.uint32).astype(np.uint64), np.array(w, dtype=np.uint64))
        got = ctx.to_host(ctx.poly_mul(_u32(ctx, a), 100, _u32(ctx, b), 511), np.uint32)
        assert np.array_equal(got, ol.PolyKron().mul(a, b))
        try:
            ctx.poly_prepare_t(_u32(ctx, t))
            assert np.array_equal(ctx.to_host(ctx.poly_h(_u32(ctx, v)), np.uint32).astype(np.uint64), oracle.poly_h(v, t))
        finally:
            ctx.ssp_prepare(ssp_on)  # (the shared context proves over the instance's SSP again)


@pytest.fixture(scope="module")
def small_circuit(mf, oracle):
    """a circuit of 30 gates without assertions (every input is honest), its SSP restated in Python (circuit_ref.ssp), keys and the oracle's CRS for it"""
    p = mf.DEBUG
    rng = np.random.default_rng(77)
    c = random_circuit(rng, 3, 12, 30)
    cc = c.compile(p)
    ssp = circuit_ref.ssp(p.d, p.m, cc.rows)
    stmts = [c.assign(x[:3].tolist(), x[3:].tolist()) for x in rng.integers(0, 2, size=(3, 15), dtype=np.uint8)]
    bad = bytearray(stmts[0])
    bad[(cc.nwires - 1) >> 3] ^= 1 << ((cc.nwires - 1) & 7)  # the last gate's wire flipped: its row no longer holds
    assert all(circuit_ref.satisfied(cc.rows, s) for s in stmts) and not circuit_ref.satisfied(cc.rows, bytes(bad))
    alpha, beta, s = (int(x) for x in rng.integers(1, ol.P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    etape = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    flat = np.ascontiguousarray(ssp.reshape(-1))
    crs = oracle.setup(p, SEED, flat, alpha, beta, s, sk, etape)
    return dict(p=p, cc=cc, ssp=ssp, flat=flat, stmts=stmts, bad=bytes(bad), alpha=alpha, beta=beta, s=s, sk=sk, etape=etape, crs=crs,
                c8=np.concatenate([crs["s"], crs["as_"], crs["t"], crs["v"][: (p.m - 1) * p.ctb]]))


def _v_of(ssp, bits, delta, m):
    """v = v_0 + delta t + sum of the v_i of the set bits (src/snark.c:141-164), mod p"""
    v = (ssp[1].astype(object) + delta * ssp[0].astype(object)) % ol.P
    for i in range(1, m):
        if _bit(bits, i - 1):
            v = (v + ssp[i + 1].astype(object)) % ol.P
    return np.array(v, dtype=np.uint64)


def test_a_poly_h_many_exact_division_and_fallback(run, ssp_on, small_circuit, oracle, mf):
    """four polynomials side by side on a mfh_ssp_from_rows SSP: satisfying statements take the exact-division path with its queued check; with one
    unsatisfying statement among them the Euclidean kernels run behind the failed check"""
    Z = small_circuit
    p = Z["p"]
    t = Z["ssp"][0]
    good = np.stack([_v_of(Z["ssp"], Z["stmts"][k % 3], 1000 + k, p.m) for k in range(4)])
    mixed = good.copy()
    mixed[2] = _v_of(Z["ssp"], Z["bad"], 5, p.m)
    assert all(oracle.poly_divides(v, t) for v in good) and not oracle.poly_divides(mixed[2], t)
    with _on(run) as ctx:
        d_ssp = ctx.ssp_from_rows(Z["cc"].rows)
        assert np.array_equal(ctx.to_host(d_ssp, np.uint32).reshape(p.m + 3, p.d), Z["ssp"].astype(np.uint32))
        ctx.ssp_prepare(d_ssp)
        ctx.set_poly_exact(2)
        try:
            assert ctx.poly_exact_fallbacks() == 0
            for V, nfall in ((good, 0), (mixed, 1), (good, 0)):
                got = ctx.to_host(ctx.poly_h_many(_u32(ctx, V.reshape(-1)), 4), np.uint32).astype(np.uint64).reshape(4, p.d)
                assert np.array_equal(got, np.stack([oracle.poly_h(v, t) for v in V]))
                assert ctx.poly_exact_fallbacks() == nfall
        finally:
            ctx.set_poly_exact(1)
            ctx.ssp_prepare(ssp_on)


def test_a_setup(run, ssp_on, inst, oracle):
    """mfh_setup_messages, mfh_setup, mfh_setup_image; the row image setup_image leaves is proved over"""
    p = inst.p
    ssp = inst.ssp.reshape(p.m + 3, p.d)
    msgs, x = [], 1
    for _ in range(p.d):
        msgs.append(x)
        x = x * inst.s % ol.P
    msgs += [e * inst.alpha % ol.P for e in msgs[: p.d]]
    msgs.append(oracle.poly_eval(ssp[0], inst.s) * inst.beta % ol.P)
    msgs += [oracle.poly_eval(ssp[i + 1], inst.s) * inst.beta % ol.P for i in range(1, p.m)]
    with _on(run) as ctx:
        assert ctx.to_host(ctx.setup_messages(ssp_on, inst.alpha, inst.beta, inst.s), np.uint32).tolist() == msgs
        d_crs = ctx.setup(ssp_on, inst.alpha, inst.beta, inst.s, _late(ctx, inst.sk), _late(ctx, inst.etape))
        assert np.array_equal(ctx.to_host(d_crs), inst.c8)
        d_crs, rows = ctx.setup_image(ssp_on, inst.alpha, inst.beta, inst.s, _late(ctx, inst.sk), _late(ctx, inst.etape))
        assert np.array_equal(ctx.to_host(d_crs), inst.c8)
        ctx.set_resident(rows)
        try:
            got = _prove(ctx, inst, d_crs, ssp_on, 0)
        finally:
            ctx.set_resident(None)
        _check_proofs(got, inst.proofs([0]), "over setup_image's rows")


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_a_prove_side_stream_fork_and_join(run, ssp_on, inst, mode):
    """mfh_prove with the witness pass and polynomial step on the side stream: both queueing orders and the automatic pick"""
    with _on(run) as ctx:
        ctx.set_overlap(mode)
        try:
            for b in (0, 2):  # a satisfying statement and a random one
                _check_proofs(_prove(ctx, inst, _late(ctx, inst.c8), ssp_on, b), inst.proofs([b]), f"overlap {mode}")
        finally:
            ctx.set_overlap(1)


def test_a_public_inputs(run, ssp_on, inst):
    """mfh_prove_public, mfh_vk_derive, mfh_verify_public with 5 public wires"""
    p = inst.p
    idx = [0, 1, 2]
    exp = inst.public_proofs(idx)
    ub = (LU + 7) // 8
    with _on(run) as ctx:
        for k, b in enumerate(idx):
            got = _ct(ctx, ctx.prove_public(_late(ctx, inst.c8), ssp_on, LU, inst.bits[b], inst.deltas[b], inst.mags[b], inst.signs[b]), (1, 5, p.n + 1, p.L))
            _check_proofs(got, exp[k: k + 1], f"public statement {b}")
        vk = ctx.derive_vk(ssp_on, inst.s, LU)
        assert ctx.to_host(vk, np.uint32).tolist() == inst.vk()
        # the proofs against their own statements, then each against the next one's
        for shift in (0, 1):
            stmts = [inst.bits[idx[(k + shift) % 3]][:ub] for k in range(3)]
            ok = ctx.to_host(ctx.verify_public(vk, LU, inst.alpha, inst.beta, _late(ctx, inst.sk), _late(ctx, exp), stmts))
            want = [inst.accepts_public(stmts[k], exp[k]) for k in range(3)]
            assert [bool(x) for x in ok] == want
            if shift == 0:
                assert want == [True, True, False]


@pytest.mark.parametrize("count", [1, 7])
def test_a_verify(run, ssp_on, inst, count):
    proofs = inst.proofs(range(count)).copy()
    if count > 3:
        proofs[3, 4, inst.p.n, 0] ^= np.uint64(2)  # b_w of a valid proof tampered with
    want = [inst.accepts(pr) for pr in proofs]
    with _on(run) as ctx:
        ok = ctx.to_host(ctx.verify(ssp_on, inst.alpha, inst.beta, inst.s, _late(ctx, inst.sk), _late(ctx, proofs), count))
    assert [bool(x) for x in ok] == want
    assert want[0] and (count == 1 or want == [True, True, False, False, True, False, True])


@pytest.mark.parametrize("n,transient_image", [(3, True), (33, True), (33, False)])
def test_a_prove_batch(run, ssp_on, inst, n, transient_image):
    """3 proofs: one group; 33: more than 31 proofs take the transient CRS image, the streaming launches and the event vectors (or, image off, run AES per group)"""
    with _on(run) as ctx:
        ctx.set_batch_image(transient_image)
        try:
            got = _prove_batch(ctx, inst, _late(ctx, inst.c8), ssp_on, n)
        finally:
            ctx.set_batch_image(True)
    _check_proofs(got, inst.proofs(range(n)), f"batch of {n}")


def test_a_prove_batch_public(run, ssp_on, inst):
    p = inst.p
    n = 33
    with _on(run) as ctx:
        got = _ct(ctx, ctx.prove_batch_public(_late(ctx, inst.c8), ssp_on, LU, *inst.args(range(n))), (n, 5, p.n + 1, p.L))
    _check_proofs(got, inst.public_proofs(range(n)), "public batch of 33")


def test_a_circuit_rows_ssp_and_prove(run, gpu_ctx_factory, small_circuit, oracle, mf):
    """mfh_ssp_from_rows (dense) and mfh_ssp_set_rows (the rows registered, d_ssp = NULL): setup and a proof under either equal the oracle's for the SSP
    restated in Python"""
    Z = small_circuit
    p = Z["p"]
    delta, mags, signs = 424242, bytes(range(200)) * 2, bytes([1, 0, 0, 1, 1])
    tape = b"".join(mags[80 * k: 80 * k + 80] + signs[k: k + 1] for k in range(5))
    exp = oracle.prover(p, Z["crs"], Z["flat"], Z["stmts"][1], delta, tape, 80, want_pre=False)["proof"][None]
    own = _make_run(gpu_ctx_factory, p, run.stream)  # (its own context: the registration stays out of the shared one)
    with _on(own) as ctx:
        dense = ctx.ssp_from_rows(Z["cc"].rows)
        assert np.array_equal(ctx.to_host(dense, np.uint32).reshape(p.m + 3, p.d), Z["ssp"].astype(np.uint32))
        ctx.ssp_set_rows(Z["cc"].rows, lu_max=3)
        try:
            for d_ssp in (dense, None):
                ctx.ssp_prepare(d_ssp)
                d_crs = ctx.setup(d_ssp, Z["alpha"], Z["beta"], Z["s"], _late(ctx, Z["sk"]), _late(ctx, Z["etape"]))
                assert np.array_equal(ctx.to_host(d_crs), Z["c8"]), "rows" if d_ssp is None else "dense"
                got = _ct(ctx, ctx.prove(_late(ctx, Z["c8"]), d_ssp, Z["stmts"][1], delta, mags, signs), (1, 5, p.n + 1, p.L))
                _check_proofs(got, exp, "rows" if d_ssp is None else "dense")
        finally:
            ctx.ssp_set_rows(None)
    own.ctx.close()


@pytest.mark.parametrize("state", ["lds", "global"])
def test_a_circuit_assign(run, circ, mf, state):
    with _on(run) as ctx:
        prog = ctx.circuit_load(circ["cc"], state=state)
        _busy(ctx)  # (host inputs only: the call itself starts behind queued work)
        wit, holds = ctx.circuit_assign(prog, circ["bits"][:70])
        prog.close()
    assert np.array_equal(wit, circ["wit"][:70]) and np.array_equal(holds, circ["holds"][:70])


# ================================================================================================================ B. the library's own stream
def test_b_own_stream(inst, prims, oracle, mf):
    """a context that is never handed a stream runs on its own non-blocking one: inputs made on torch's stream and awaited, the calls, mfh_sync, read back"""
    import torch

    p = inst.p
    R = prims["debug"]
    ctx = mf.Context(p, 0, own_stream=True)
    try:
        ctx.set_seed(SEED)
        d_ssp_in = ctx.empty((p.m + 3) * p.d * 4)
        d_c8, d_co = ctx.to_device(R.ev_c8[: 700 * p.ctb]), [ctx.to_device(R.ev_co[v, :700].astype(np.uint32)) for v in range(2)]
        d_sk, d_msg, d_err = ctx.to_device(R.sk), ctx.to_device(R.msg.astype(np.uint32)), ctx.to_device(R.err)
        d_crs = ctx.to_device(inst.c8)
        torch.cuda.synchronize()
        ks = ctx.keystream(16, 4096)
        r0, r1 = ctx.eval_rows(R.ev_off, 700, d_c8, d_co[0], d_co[1])
        ctx.set_encrypt_path(2)
        enc = ctx.encrypt_rows(R.enc_off, ENC_ROWS, d_sk, d_msg, d_err)
        ctx.set_encrypt_path(0)
        d_ssp = ctx.ssp_upload(inst.ssp, d_ssp_in)
        ctx.ssp_prepare(d_ssp)
        one = ctx.prove(d_crs, d_ssp, inst.bits[1], inst.deltas[1], inst.mags[1], inst.signs[1])
        batch = ctx.prove_batch(d_crs, d_ssp, *inst.args(range(33)))
        ctx.sync()
        assert ctx.to_host(ks).tobytes() == oracle.keystream(SEED, 16, 4096)
        exp = R.eval(700, 2)
        assert np.array_equal(_ct(ctx, r0, exp[0].shape), exp[0]) and np.array_equal(_ct(ctx, r1, exp[1].shape), exp[1])
        assert np.array_equal(ctx.to_host(enc), R.enc(ENC_ROWS))
        _check_proofs(_ct(ctx, one, (1, 5, p.n + 1, p.L)), inst.proofs([1]), "own stream")
        _check_proofs(_ct(ctx, batch, (33, 5, p.n + 1, p.L)), inst.proofs(range(33)), "own stream, batch of 33")
    finally:
        ctx.close()


# ================================================================================================================ C. moving a context between streams
def test_c_alternating_streams_with_a_sync_before_each_switch(gpu_ctx_factory, inst, prims, mf):
    import torch

    p = inst.p
    R = prims["debug"]
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    d_ssp = ctx.ssp_upload(inst.ssp)
    ctx.ssp_prepare(d_ssp)
    d_c8, d_co = ctx.to_device(R.ev_c8[: 700 * p.ctb]), [ctx.to_device(R.ev_co[v, :700].astype(np.uint32)) for v in range(2)]
    d_crs = ctx.to_device(inst.c8)
    torch.cuda.synchronize()  # the operands are final whichever stream reads them
    exp_ev, exp_one, exp_batch = R.eval(700, 2), inst.proofs([4]), inst.proofs(range(33))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    calls = ["eval", "prove", "batch"]
    # a Latin square with k % 3: eval_rows on s1, s2, null; prove on s2, null, s1; prove_batch on null, s1, s2 -- every call on every stream, and every
    # call is preceded by a switch from another stream
    for k, st in enumerate([s1, s2, None, s2, None, s1, None, s1, s2]):
        ctx.sync()
        ctx.set_stream(st)
        with _on(_Run(ctx, st)):
            what = calls[k % 3]
            if what == "eval":
                r0, r1 = ctx.eval_rows(R.ev_off, 700, d_c8, d_co[0], d_co[1])
                assert np.array_equal(_ct(ctx, r0, exp_ev[0].shape), exp_ev[0]) and np.array_equal(_ct(ctx, r1, exp_ev[1].shape), exp_ev[1]), k
            elif what == "prove":
                _check_proofs(_prove(ctx, inst, d_crs, d_ssp, 4), exp_one, f"step {k}")
            else:
                _check_proofs(_prove_batch(ctx, inst, d_crs, d_ssp, 33), exp_batch, f"step {k}")
    ctx.sync()
    ctx.set_stream(None)


def test_c_sample_rows_may_be_followed_by_a_switch_at_once(gpu_ctx_factory, oracle, mf):
    """mfh_sample_rows keeps its raw-bytes buffer in the context and orders it across streams itself (ev_sample): the one call after which the stream may be
    switched without a wait.  No other unsynchronised switch is promised, and none is tested.  This pins the RESULTS of the documented usage, not the
    event wait itself: whether the kernels of two calls overlap is up to the scheduler, and a missing wait would show only if they did.  The requests
    are near the kept buffer's 16 MiB limit (about 120 rows), so that one call's repack is long enough for the next call's keystream to catch up with it."""
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    offs = [(0, 110), (5 * p.ctr_ct, 110), (135240, 97), (8863223880, 110)]  # the first is the largest: the kept buffer is not regrown (a regrow waits)
    outs = []
    for k, (off, nrows) in enumerate(offs):
        st = (s1, s2)[k % 2]
        ctx.set_stream(st)
        with _on(_Run(ctx, st)):
            outs.append(ctx.sample_rows(off, nrows))
    for k, (off, nrows) in enumerate(offs):
        with _on(_Run(ctx, (s1, s2)[k % 2])):
            got = ctx.to_host(outs[k], np.uint64).reshape(nrows, p.n, p.L)
        assert np.array_equal(got, oracle.sample_rows(p, SEED, off, nrows)), k
    ctx.sync()
    ctx.set_stream(None)
    torch.cuda.synchronize()


# ================================================================================================================ D. history of the context
@pytest.mark.parametrize("kind", ["null", "stream"])
def test_d_results_do_not_depend_on_what_the_context_did_before(gpu_ctx_factory, inst, prims, circ, as_region, oracle, mf, kind):
    """Each call-sized entry point at a small, a large, a small and (some) a larger size in ONE context, the entry points interleaved step by step, so that
    every grow-only scratch is regrown while others hold pointers into theirs and the shared ones (ws, aux, wws, pin_rows, pin_cw) change hands at
    different sizes.  After each growth of an eval_rows size an accumulate = False evaluation with one non-zero coefficient must be exact (the lazy-carry
    image is all zero after its reallocation); after the matrix-core encrypt and decrypt calls, whose key wipe zeroes a region of the workspace, the next
    eval_rows must be exact.  mfh_workspace_bytes never shrinks and stays a multiple of 1 MiB."""
    import torch

    p = inst.p
    R = prims["debug"]
    run = _make_run(gpu_ctx_factory, p, torch.cuda.Stream() if kind == "stream" else None)
    shape = (p.n + 1, p.L)
    late = _late if kind == "stream" else (lambda c, a: c.to_device(a))
    u32 = lambda c, a: late(c, np.ascontiguousarray(a, dtype=np.uint32))  # noqa: E731
    wsb = []

    with _on(run) as ctx:
        d_ssp = ctx.ssp_upload(inst.ssp)
        ctx.ssp_prepare(d_ssp)
        progs = {state: ctx.circuit_load(circ["cc"], state=state) for state in ("lds", "global")}
        rng = np.random.default_rng(9)
        smudge_cts = ol.rand_values(rng, 50 * (p.n + 1), p.L, 64 * p.K).reshape(50, p.n + 1, p.L)
        smudge_mags = rng.integers(0, 256, size=50 * 80, dtype=np.uint8).tobytes()
        smudge_signs = bytes(rng.integers(0, 2, size=50, dtype=np.uint8).tolist())
        co10 = rng.integers(0, ol.P, size=(3, 10), dtype=np.uint64)

        def one_row(nrows):
            row = nrows - 1
            co = np.zeros(nrows, dtype=np.uint32)
            co[row] = 0xFFFFFFFA
            r0, _ = ctx.eval_rows(R.ev_off, nrows, late(ctx, R.ev_c8[: nrows * p.ctb]), u32(ctx, co))
            assert np.array_equal(_ct(ctx, r0, shape), R.eval_one(row, 0xFFFFFFFA)), f"one non-zero coefficient over {nrows} rows"

        def ev(nrows):
            exp = R.eval(nrows, 2)
            r0, r1 = ctx.eval_rows(R.ev_off, nrows, late(ctx, R.ev_c8[: nrows * p.ctb]), u32(ctx, R.ev_co[0, :nrows]), u32(ctx, R.ev_co[1, :nrows]))
            assert np.array_equal(_ct(ctx, r0, shape), exp[0]) and np.array_equal(_ct(ctx, r1, shape), exp[1]), f"eval_rows, {nrows} rows"
            one_row(nrows)

        def ev_multi(nrows):
            if nrows == p.d:
                (co, exp), off, c8 = as_region, p.ctr_as, inst.crs["as_"]
            else:
                co, off, c8 = co10, R.ev_off, R.ev_c8[: nrows * p.ctb]
                exp = [oracle.eval_poly(p, SEED, off, c8.tobytes(), co[v]) for v in range(3)]
            got = _ct(ctx, ctx.eval_rows_multi(off, nrows, late(ctx, c8), u32(ctx, co), 3), (3, p.n + 1, p.L))
            for v in range(3):
                assert np.array_equal(got[v], exp[v]), f"eval_rows_multi, {nrows} rows, vector {v}"

        def enc(nrows):
            ctx.set_encrypt_path(2)
            try:
                got = ctx.to_host(ctx.encrypt_rows(R.enc_off, nrows, late(ctx, R.sk), u32(ctx, R.msg[:nrows]), late(ctx, R.err[:nrows])))
            finally:
                ctx.set_encrypt_path(0)
            assert np.array_equal(got, R.enc(nrows)), f"encrypt_rows, {nrows} rows"
            ev(2)

        def dec(count):
            ctx.set_decrypt_path(2)
            try:
                got = ctx.to_host(ctx.decrypt(late(ctx, R.sk), late(ctx, R.cts[:count]), count), np.uint32)
            finally:
                ctx.set_decrypt_path(0)
            assert np.array_equal(got, R.dec(count)), f"decrypt, {count} ciphertexts"
            ev(2)

        def dec_rows(nrows):
            got = ctx.to_host(ctx.decrypt_rows(R.enc_off, nrows, late(ctx, R.sk), late(ctx, R.enc(nrows))), np.uint32)
            assert np.array_equal(got, R.dec_rows(nrows)), f"decrypt_rows, {nrows} rows"

        def sample(nrows):
            got = ctx.to_host(ctx.sample_rows(7 * p.ctr_ct, nrows), np.uint64).reshape(nrows, p.n, p.L)
            assert np.array_equal(got, oracle.sample_rows(p, SEED, 7 * p.ctr_ct, nrows)), f"sample_rows, {nrows} rows"

        def verify(count):
            proofs = inst.proofs(range(count))
            ok = ctx.to_host(ctx.verify(d_ssp, inst.alpha, inst.beta, inst.s, late(ctx, inst.sk), late(ctx, proofs), count))
            assert [bool(x) for x in ok] == [inst.accepts(pr) for pr in proofs] == [b % 3 != 2 for b in range(count)], f"verify, {count} proofs"

        def smudge(count):
            d = late(ctx, smudge_cts[:count])
            ctx.ct_smudge(d, count, smudge_mags[: 80 * count], 80, smudge_signs[:count])
            got = _ct(ctx, d, (count, p.n + 1, p.L))
            for i in range(count):
                assert np.array_equal(got[i], oracle.ct_smudge(p, smudge_cts[i], smudge_mags[80 * i: 80 * i + 80], smudge_signs[i])[0]), f"ct_smudge {i} of {count}"

        def batch(n):
            _check_proofs(_prove_batch(ctx, inst, late(ctx, inst.c8), d_ssp, n), inst.proofs(range(n)), f"prove_batch of {n}")

        def batch_public(n):
            got = _ct(ctx, ctx.prove_batch_public(late(ctx, inst.c8), d_ssp, LU, *inst.args(range(n))), (n, 5, p.n + 1, p.L))
            _check_proofs(got, inst.public_proofs(range(n)), f"prove_batch_public of {n}")

        def assign(nb):
            for state, prog in progs.items():
                wit, holds = ctx.circuit_assign(prog, circ["bits"][:nb])
                assert np.array_equal(wit, circ["wit"][:nb]) and np.array_equal(holds, circ["holds"][:nb]), f"circuit_assign ({state}), {nb} statements"

        ladders = [(ev, [1, 700, 2, EV_ROWS]), (ev_multi, [10, p.d, 10]), (enc, [3, ENC_ROWS, 5]), (dec, [1, DEC_CTS, 16]), (dec_rows, [5, ENC_ROWS, 5]),
                   (sample, [1, 3, 1]), (verify, [1, 40, 2]), (smudge, [1, 50, 1]), (batch, [2, 33, 3, NPOOL]), (batch_public, [2, 33, 2]),
                   (assign, [1, 70, 8193, 1])]  # 8193: one statement past the LDS kind's 8192-statement chunk
        for step in range(4):
            for fn, sizes in ladders:  # step k of every entry point, then step k + 1: each is followed by a step of another
                if step < len(sizes):
                    fn(sizes[step])
                    wsb.append(ctx.workspace_bytes())
        for prog in progs.values():
            prog.close()
    assert all(b % (1 << 20) == 0 for b in wsb), wsb
    assert all(a <= b for a, b in zip(wsb, wsb[1:])), wsb
    assert wsb[-1] > 0


# ================================================================================================================ E. mfh_scrub_staging
def test_e_scrub_on_a_fresh_context(gpu_ctx_factory, mf):
    ctx = gpu_ctx_factory(mf.DEBUG)
    assert ctx.scrub_staging() == 0
    assert ctx.scrub_staging() == 0


def test_e_calls_after_a_scrub_reacquire_their_staging(run, ssp_on, inst, circ, oracle):
    """mfh_scrub_staging resets what the pinned staging buffers remember (bytes in use, copy pending): after it, the same call with the same entropy must stage
    everything again and give the first call's bytes, which are the oracle's.  (That the staging is ZEROED cannot be observed through the ABI -- the buffers
    are the context's own, and no accessor exists for them; only the re-acquisition is pinned here.)"""
    p = inst.p
    rng = np.random.default_rng(13)
    cts = ol.rand_values(rng, 3 * (p.n + 1), p.L, 64 * p.K).reshape(3, p.n + 1, p.L)
    mags = rng.integers(0, 256, size=3 * 80, dtype=np.uint8).tobytes()
    signs = bytes([0, 1, 1])
    with _on(run) as ctx:
        prog = ctx.circuit_load(circ["cc"])

        def prove():
            return _prove(ctx, inst, _late(ctx, inst.c8), ssp_on, 3), inst.proofs([3])

        def prove_public():
            b = 1
            got = ctx.prove_public(_late(ctx, inst.c8), ssp_on, LU, inst.bits[b], inst.deltas[b], inst.mags[b], inst.signs[b])
            return _ct(ctx, got, (1, 5, p.n + 1, p.L)), inst.public_proofs([b])

        def batch():
            return _prove_batch(ctx, inst, _late(ctx, inst.c8), ssp_on, 33), inst.proofs(range(33))

        def assign():
            wit, holds = ctx.circuit_assign(prog, circ["bits"][:70])
            return np.concatenate([wit.reshape(-1), holds.astype(np.uint8)]), np.concatenate([circ["wit"][:70].reshape(-1), circ["holds"][:70].astype(np.uint8)])

        def smudge():
            d = _late(ctx, cts)
            ctx.ct_smudge(d, 3, mags, 80, signs)
            return _ct(ctx, d, cts.shape), np.stack([oracle.ct_smudge(p, cts[i], mags[80 * i: 80 * i + 80], signs[i])[0] for i in range(3)])

        for call in (prove, prove_public, batch, assign, smudge):
            first, exp = call()
            assert ctx.scrub_staging() == 0
            second, _ = call()
            assert np.array_equal(first, second), f"{call.__name__}: the call after the scrub differs from the one before"
            assert np.array_equal(first, exp), f"{call.__name__}: differs from the reference"
        prog.close()


def test_e_scrub_waits_for_the_copies_of_a_queued_batch(run, ssp_on, inst):
    """scrub directly behind a mfh_prove_batch that is only queued: it must wait for the pending copies out of the staging itself before it zeroes them"""
    p = inst.p
    with _on(run) as ctx:
        out = ctx.prove_batch(_late(ctx, inst.c8), ssp_on, *inst.args(range(33)))
        assert ctx.scrub_staging() == 0
        got = _ct(ctx, out, (33, 5, p.n + 1, p.L))
    _check_proofs(got, inst.proofs(range(33)), "scrubbed behind the queued call")
