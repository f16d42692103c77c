"""GPU: every form of the witness pass (csrc/witness.hip) against exact integers.

    w_b[k] = delta_b t[k] + sum_{i = 1 .. m - 1} bit_b[i - 1] v_i[k]  mod p

Every assertion compares all nstmt x d coefficients with tests/witness_ref.py (numpy on 16-bit halves and Python integers, no project code; held
against the definition, the oracle and the compiled generator header by tests/test_witness_ref_cpu.py), never with another GPU result alone.  A
failure names the first (statement, k), the kernel form that ran and got / want; the launch plan of the GEMM form is recomputed here from MmPlan's
formulas (mm_plan) and stands in the test id.

A. forms x plan seams over random SSPs in [0, p): statement tiles (MT 1 / 2 / 4 / 8), a ragged last row step with every padding width of the last
   byte, the chunk planner, k_witness_mm8q's prologue, rounds and tails with both of its epilogues, the seam between them, m >= 2^16, coefficient
   ranges, the VALU forms, and the pass as the batch chain calls it.  Statement 0 is all-zero, statement 1 all 0xFF bytes (padding bits set on
   purpose), delta_0 = 0, delta_1 = p - 1.
B. crafted operands.  The GEMM multiplies the 0 / 1 witness bits with the BYTES of the coefficients, offset by 128 (stored byte ^ 0x80, read as
   int8), and adds 128 cnt_b back per byte plane.  Constant rows put one value on every MFMA B operand:
       byte 0x00 -> -128 (rows 0, and the planes of 0xFF << 8w that are not w),   byte 0xFF -> +127 (p - 1's three upper planes, plane w of 0xFF << 8w),
       byte 0x80 ->    0 (0x80808080),   byte 0x7F -> -1 (0x7F7F7F7F),   p - 1's low byte 0xFA -> +122,
   so an int32 accumulator of a statement that selects cnt rows holds -128 cnt, +127 cnt, 0 or -cnt: the correction 128 cnt_b and the signs are what
   these cases are about.  |accumulator| <= 128 (m - 1) <= 2^23 here, nowhere near 2^31: these are sign and correction cases, not overflow cases.
   The expected values have the closed form cnt_b value + delta_b t[k] mod p, asserted beside the reference.
C. the generator (csrc/ssp_prg.hpp): mfh_ssp_prg_fill equals the restatement, and seeds crafted so that one (slot, k) hashes to each raw value in
   [p, 2^32) -- which ssp_prg_coeff reduces and the GEMM / VALU kernels sum unreduced -- go through every generated form, the setup messages,
   the verification key, the chain's V step and the public-input batch prover."""
import ctypes
import functools

import numpy as np
import pytest

import witness_ref as wr

pytestmark = pytest.mark.gpu
P = wr.P
PRG_SEED = 0x0123456789ABCDEF  # (the seed of tests/test_gpu_prg_ssp.py)
SEED = bytes((17 * i + 9) & 0xFF for i in range(40))


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


# ---- the launch plan, from MmPlan's formulas (csrc/witness.hip) ----------------------------------------------------------------------------
class Plan:
    def __init__(self, m, nstmt, nc, dense):
        self.dense = dense
        self.MT = 8 if nstmt > 128 else 4 if nstmt > 64 else 2 if nstmt > 32 else 1
        self.ksteps = (m - 1 + 31) // 32
        self.fused = self.MT == 8 and dense and m < 65536 and (nc >= 16384 or self.ksteps <= 64)
        self.nchunks = 1 if self.fused else min(self.ksteps, 4)
        self.kpc = (self.ksteps + self.nchunks - 1) // self.nchunks
        self.ychunks = (self.ksteps + self.kpc - 1) // self.kpc

    @property
    def form(self):
        if self.MT == 8:
            body = "k_witness_mm8q" if self.dense else "k_witness_mm8q_prg"
        else:
            body = f"k_witness_mm<{self.MT}>" if self.dense else f"k_witness_mm_prg<{self.MT}>"
        return body + (" (finished in the kernel)" if self.fused else " + k_witness_mm_finish")

    def __str__(self):
        body = ("mm8q" if self.dense else "mm8q_prg") if self.MT == 8 else ("mm" if self.dense else "mm_prg") + str(self.MT)
        return f"{body}-MT{self.MT}-ksteps{self.ksteps}-{'fused' if self.fused else 'partials'}-nchunks{self.nchunks}-kpc{self.kpc}-ychunks{self.ychunks}"


def mm_plan(m, nstmt, nc, dense):
    return Plan(m, nstmt, nc, dense)


def mm_case(d, m, nstmt, dense, nc=None):
    """a pytest.param whose id shows the shape and the plan that runs"""
    return pytest.param(d, m, nstmt, dense, id=f"d{d}-m{m}-n{nstmt}-{mm_plan(m, nstmt, nc or d, dense)}")


# ---- inputs and the comparison --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def random_ssp(m, d, seed=0):
    """uint32 [(m + 3), d], every coefficient uniform in [0, p); shared between the cases of a shape, read-only"""
    a = np.random.default_rng([m, d, seed]).integers(0, P, size=(m + 3, d), dtype=np.uint64).astype(np.uint32)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=2)
def generated_ssp(seed, m, d):
    """uint32 [(m + 3), d]: slot 0 = a random t in [0, p), slots 1 .. m + 2 by the restated generator; read-only"""
    t = np.random.default_rng([m, d, seed & 0xFFFFFFFF, seed >> 32]).integers(0, P, size=(1, d), dtype=np.uint64).astype(np.uint32)
    a = np.concatenate([t, wr.prg_image(seed, 1, m + 2, d)])
    a.flags.writeable = False
    return a


def statements(rng, m, nstmt):
    """statement 0 all-zero, statement 1 all 0xFF bytes (padding bits set), the rest random bytes; delta_0 = 0, delta_1 = p - 1, the rest random"""
    nbytes = (m + 6) // 8
    bits = [bytes(nbytes), b"\xff" * nbytes][:nstmt] + [rng.bytes(nbytes) for _ in range(nstmt - 2)]
    deltas = [0, P - 1][:nstmt] + [int(x) for x in rng.integers(0, P, size=max(0, nstmt - 2), dtype=np.uint64)]
    return bits, deltas


def register(c, ssp, dense, seed=PRG_SEED):
    """the SSP on the device: a dense image through mfh_ssp_upload (which invalidates the cached fragment image), or slot 0 registered with the generator's seed"""
    if dense:
        return c.ssp_upload(ssp.astype(np.uint64).reshape(-1))
    c.ssp_set_prg(seed, c.to_device(np.ascontiguousarray(ssp[0])))
    return None


def assert_exact(got, want, form, what=""):
    got = np.asarray(got).view(np.uint32).reshape(want.shape).astype(np.uint64)
    if np.array_equal(got, want):
        return
    bad = got != want
    b, k = (int(x) for x in np.argwhere(bad)[0])
    raise AssertionError(f"{form}{what}: first difference at statement {b}, k = {k}: got {int(got[b, k]):#010x}, want {int(want[b, k]):#010x} "
                         f"({int(bad.sum())} of {want.size} coefficients differ, in {int(bad.any(axis=1).sum())} of {want.shape[0]} statements)")


def run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense, ssp=None, bits=None, deltas=None, seed=PRG_SEED):
    """mfh_witness_poly_mm of nstmt statements at (d, m) against the reference, all coefficients"""
    plan = mm_plan(m, nstmt, d, dense)
    if ssp is None:
        ssp = random_ssp(m, d) if dense else generated_ssp(seed, m, d)
    if bits is None:
        bits, deltas = statements(np.random.default_rng([d, m, nstmt, int(dense)]), m, nstmt)
    want = wr.w_polys(ssp, bits, deltas, m)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp = register(c, ssp, dense, seed)
        got = c.to_host(c.witness_poly_many(d_ssp, bits, deltas, mm=True), np.uint32)
    finally:
        c.close()
    assert_exact(got, want, plan.form, f" [{plan}]")
    return want


# ================================================================================ A. forms x plan seams ======================================
TILE_NSTMT = [1, 31, 32, 33, 64, 65, 128, 129, 255, 256]


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(128, 100, n, dense) for dense in (True, False) for n in TILE_NSTMT])
def test_statement_tiles(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """MT = 1 / 2 / 4 / 8 on both sides of every threshold, the last statement tile full, one short and one over"""
    assert mm_plan(m, nstmt, d, dense).MT == (1 if nstmt <= 32 else 2 if nstmt <= 64 else 4 if nstmt <= 128 else 8)
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)
    if nstmt == 1:  # (the all-zero statement alone has w = 0: one random statement with a random delta as well)
        rng = np.random.default_rng(int(dense))
        run_mm(mf, gpu_ctx_factory, d, m, 1, dense, bits=[rng.bytes((m + 6) // 8)], deltas=[int(rng.integers(1, P))])


RAGGED_ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65] + [18, 35, 44, 53, 62]  # (the edges are 0, 1 or 7 mod 8: five more for 2 .. 6)


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(128, r + 1, n, dense) for dense in (True, False) for n in (33, 129) for r in RAGGED_ROWS])
def test_ragged_last_row_step(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """m - 1 on both sides of 16, 32 and 64 rows: the half-step and step edges of k_witness_bits and k_ssp_frag; m - 1 mod 8 takes every value, so the
    all-0xFF statement has every width of padding in its last byte"""
    assert {r % 8 for r in RAGGED_ROWS} == set(range(8))
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)


CHUNK_KSTEPS = [1, 2, 3, 4, 5, 9, 13]


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(128, 32 * ks - 4, n, dense) for n, dense in ((33, False), (129, False), (100, True)) for ks in CHUNK_KSTEPS])
def test_chunk_planner(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """chunk partials summed by k_witness_mm_finish: 1 .. 4 chunks of one step, 5 steps -> kpc 2 and 3 chunks where the partials are sized for 4,
    13 steps -> chunks of 4, 4, 4, 1"""
    plan = mm_plan(m, nstmt, d, dense)
    assert not plan.fused
    five, thirteen = mm_plan(32 * 5 - 4, nstmt, d, dense), mm_plan(32 * 13 - 4, nstmt, d, dense)
    assert (five.kpc, five.ychunks, five.nchunks) == (2, 3, 4) and (thirteen.kpc, thirteen.ychunks) == (4, 4) and 13 - 3 * 4 == 1
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(128, 32 * ks + 1, 200, True) for ks in (1, 2, 3, 4, 5, 6, 7, 8, 64)])
def test_mm8q_finished_in_the_kernel(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """k_witness_mm8q with its own epilogue: fewer steps than the prologue prefetches (PF = 4), whole rounds of 4, tails of 1 - 3, and 64 steps (m - 1 = 2048:
    the most the `ksteps <= 64` branch takes)"""
    plan = mm_plan(m, nstmt, d, dense)
    assert plan.fused and plan.ychunks == 1 and plan.ksteps == (m - 1) // 32
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(128, r + 1, 200, True) for r in (2049, 2080)])
def test_mm8q_seam_to_partials(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """one row more than the fused maximum: 65 steps at d = 128 go through chunk partials, chunks of 17, 17, 17, 14"""
    plan = mm_plan(m, nstmt, d, dense)
    assert not plan.fused and (plan.ksteps, plan.nchunks, plan.kpc, plan.ychunks) == (65, 4, 17, 4) and 65 - 3 * 17 == 14
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(16384, 2082, n, True) for n in (256, 130)])
def test_mm8q_fused_by_width(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """the branch the default instance takes: more than 64 row steps in ONE chunk, fused because the range is at least 16384 coefficients wide
    (66 steps: 16 rounds and a tail of 2; a 137 MB SSP)"""
    plan = mm_plan(m, nstmt, d, dense)
    assert plan.fused and plan.ksteps == 66 and plan.ychunks == 1
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(128, 65537, n, dense) for dense in (True, False) for n in (129, 20)])
def test_m_at_65537(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """m >= 2^16: k_witness_mm8q never finishes in the kernel (a byte-plane sum may pass 2^24), and row indices pass 16 bits; 2048 steps in 4 chunks of 512"""
    plan = mm_plan(m, nstmt, d, dense)
    assert not plan.fused and (plan.ksteps, plan.kpc, plan.ychunks) == (2048, 512, 4)
    run_mm(mf, gpu_ctx_factory, d, m, nstmt, dense)


def witness_cols(mf, c, d_ssp, bits, deltas, col0, ncols, w_stride, fill):
    """mfh_batch_witness_cols with an output whose statements are w_stride > ncols apart -> int32 [nstmt, w_stride], pre-filled with `fill`"""
    import torch

    nb = len(bits)
    out = torch.full((nb, w_stride), fill, dtype=torch.int32, device=c.device)
    packed, stride = c._pack_bits(bits)
    dl = (ctypes.c_uint32 * nb)(*deltas)
    c._chk(c.lib.mfh_batch_witness_cols(c._h, mf._ptr(d_ssp), nb, packed, stride, ctypes.cast(dl, ctypes.c_void_p), col0, ncols, mf._ptr(out), w_stride))
    return out


@pytest.mark.parametrize("d,m,nstmt,dense", [mm_case(512, 100, 200, True, nc=128), mm_case(512, 100, 100, True, nc=128), mm_case(512, 100, 200, False, nc=128),
                                             mm_case(512, 100, 40, False, nc=128)])
def test_coefficient_ranges(gpu_ctx_factory, mf, d, m, nstmt, dense):
    """mfh_witness_poly_mm_cols through mfh_batch_witness_cols: ranges that start at 0, in the middle and end at d, two widths, the statements of the
    output further apart than the range is wide (what lies between them stays untouched); k_witness_mm8q finishing in the kernel, k_witness_mm<4> through
    partials, both generated forms (which add the range's start to k before they hash)"""
    ssp = random_ssp(m, d) if dense else generated_ssp(PRG_SEED, m, d)
    bits, deltas = statements(np.random.default_rng([d, m, nstmt, int(dense)]), m, nstmt)
    want = wr.w_polys(ssp, bits, deltas, m)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp = register(c, ssp, dense)
        for col0, ncols in ((0, 128), (128, 256), (384, 128)):
            plan, fill, w_stride = mm_plan(m, nstmt, ncols, dense), 0x5A5A5A5A, ncols + 96
            assert plan.fused == (dense and nstmt > 128)
            got = c.to_host(witness_cols(mf, c, d_ssp, bits, deltas, col0, ncols, w_stride, fill), np.uint32).reshape(nstmt, w_stride)
            assert_exact(np.ascontiguousarray(got[:, :ncols]), want[:, col0: col0 + ncols], plan.form, f" [{plan}] coefficients [{col0}, {col0 + ncols})")
            assert (got[:, ncols:] == fill).all(), f"{plan.form}: wrote between the statements of the output, range [{col0}, {col0 + ncols})"
    finally:
        c.close()


def valu_statements(rng, m, nstmt, nsel):
    """nsel of the m - 1 rows selected by statement 0 and, each, by a random subset of the others; the padding bits of every last byte set"""
    nbytes = (m + 6) // 8
    sel = np.zeros((nstmt, nbytes * 8), dtype=np.uint8)
    rows = rng.choice(m - 1, size=nsel, replace=False)
    sel[0, rows] = 1
    for b in range(1, nstmt):
        sel[b, rows[rng.integers(0, 2, size=nsel).astype(bool)]] = 1
    sel[:, m - 1:] = 1
    bits = [np.packbits(sel[b], bitorder="little").tobytes() for b in range(nstmt)]
    deltas = [0, P - 1][:nstmt] + [int(x) for x in rng.integers(0, P, size=max(0, nstmt - 2), dtype=np.uint64)]
    return bits, deltas


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "generated"])
@pytest.mark.parametrize("nsel", [0, 1, 7, 8, 9, 600])
@pytest.mark.parametrize("d", [4, 132, 1028])
def test_valu_forms(gpu_ctx_factory, mf, d, nsel, dense):
    """mfh_witness_poly (k_witness_partial[_prg] + k_witness_finish) and mfh_witness_poly_multi with 1, 11 and 12 statements
    (k_witness_partial_multi[_prg]<12>), d not a multiple of 128 (one thread, a part of a block, more than one block), the selected rows in
    G = 1, 2 and 64 (16) shares: none, one, 7 | 8 | 9 around the first split, and 600 (the four-rows-in-flight loop of _multi and its tail)"""
    m = 700
    assert (m - 1) % 8 and d % 128 and d % 4 == 0
    ssp = random_ssp(m, d) if dense else generated_ssp(PRG_SEED, m, d)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp = register(c, ssp, dense)
        for nstmt in (1, 11, 12):
            bits, deltas = valu_statements(np.random.default_rng([d, nsel, nstmt]), m, nstmt, nsel)
            assert int(wr.bit_matrix(bits, m).any(axis=0).sum()) == nsel == int(wr.bit_matrix(bits[:1], m).sum())
            want = wr.w_polys(ssp, bits, deltas, m)
            got = c.to_host(c.witness_poly_many(d_ssp, bits, deltas, mm=False), np.uint32)
            assert_exact(got, want, f"k_witness_partial_multi{'' if dense else '_prg'}<12> + k_witness_finish, {nstmt} statements, {nsel} rows, G = {max(1, min(16, nsel // 8 + 1))}")
            for b in sorted({0, nstmt - 1}):
                delta = deltas[b] if nstmt > 1 else 31337
                got = c.to_host(c.witness_poly(d_ssp, bits[b], delta), np.uint32)
                assert_exact(got, wr.w_polys(ssp, [bits[b]], [delta], m), f"k_witness_partial{'' if dense else '_prg'} + k_witness_finish, statement {b} of {nstmt}, {nsel} rows in the union")
    finally:
        c.close()


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "generated"])
@pytest.mark.parametrize("d,nstmt,pers", [(128, 255, (0, 32, 124)), (192, 25, (0,))], ids=["d128-n255-gemm-per0,32,124", "d192-n25-valu-12,12,1"])
def test_through_the_batch_chain(gpu_ctx_factory, mf, d, nstmt, pers, dense):
    """w and v = w + v_0 of mfh_batch_chain, every statement with its own delta: the GEMM in pass windows of 255 | 7 x 32 + 31 | 124 + 124 + 7
    statements (mfh_set_witness_per), and at d % 128 != 0 the VALU form in passes of 12 + 12 + 1"""
    m = 100
    ssp = random_ssp(m, d) if dense else generated_ssp(PRG_SEED, m, d)
    bits, deltas = statements(np.random.default_rng([d, nstmt]), m, nstmt)
    assert len(set(deltas)) == nstmt
    want = wr.w_polys(ssp, bits, deltas, m)
    want_v = (want + ssp[1].astype(np.uint64)[None, :]) % np.uint64(P)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp = register(c, ssp, dense)
        c.ssp_prepare(d_ssp)
        for per in pers:
            c.set_witness_per(per)
            whv = c.to_host(c.batch_chain(d_ssp, bits, deltas), np.uint32).reshape(3, nstmt, d)
            windows = [min(per or 256, nstmt - b0) for b0 in range(0, nstmt, per or 256)] if d % 128 == 0 else [min(12, nstmt - b0) for b0 in range(0, nstmt, 12)]
            forms = sorted({mm_plan(m, n, d, dense).form for n in windows}) if d % 128 == 0 else [f"k_witness_partial_multi{'' if dense else '_prg'}<12>"]
            assert_exact(whv[0], want, " | ".join(forms), f", pass windows {windows}: w")
            assert_exact(whv[2], want_v, "k_add_slot_multi", f", pass windows {windows}: v = w + v_0")
    finally:
        c.close()


# ================================================================================ B. crafted operands ========================================
PATTERNS = {"zero": 0, "p-1": P - 1, "0x80808080": 0x80808080, "0x7f7f7f7f": 0x7F7F7F7F, "ff-plane0": 0xFF, "ff-plane1": 0xFF00, "ff-plane2": 0xFF0000,
            "ff-plane3": 0xFF000000, "alternating-0-p-1": None}
B_SHAPES = [(2049, 256), (65537, 129), (300, 20), (300, 40), (300, 100)]  # the fused maximum (m - 1 = 2048), the unfused m >= 2^16, MT = 1, 2, 4


@pytest.mark.parametrize("m,nstmt", B_SHAPES, ids=[f"m{m}-n{n}-{mm_plan(m, n, 128, True)}" for m, n in B_SHAPES])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_crafted_operands(gpu_ctx_factory, mf, pattern, m, nstmt):
    """(see B in the module docstring) every row v_1 .. v_{m-1} the same constant, or rows alternating 0 / p - 1; statements all-ones, all-zero, only
    bit 0, only bit m - 2, the rest random; t, v_0 and the two slots past v_{m-1} random (the pass must not look at them)"""
    d = 128
    rng = np.random.default_rng([m, nstmt, list(PATTERNS).index(pattern)])
    ssp = rng.integers(0, P, size=(m + 3, d), dtype=np.uint64).astype(np.uint32)
    value = PATTERNS[pattern]
    if value is None:
        ssp[2: m + 1] = 0
        ssp[2: m + 1: 2] = P - 1  # v_1, v_3, ... = p - 1; v_2, v_4, ... = 0
    else:
        ssp[2: m + 1] = value
    nbytes = (m + 6) // 8

    def only(i):
        return bytes((1 << (i & 7)) if j == i >> 3 else 0 for j in range(nbytes))

    bits = ([b"\xff" * nbytes, bytes(nbytes), only(0), only(m - 2)] + [rng.bytes(nbytes) for _ in range(nstmt - 4)])[:nstmt]
    deltas = [P - 1, 0, 1] + [int(x) for x in rng.integers(0, P, size=nstmt - 3, dtype=np.uint64)]
    want = run_mm(mf, gpu_ctx_factory, d, m, nstmt, True, ssp=ssp, bits=bits, deltas=deltas)
    # the closed form, in Python integers
    sel = wr.bit_matrix(bits, m)
    assert [int(x) for x in sel.sum(axis=1)[:4]] == [m - 1, 0, 1, 1]
    for b in range(nstmt):
        s = int(sel[b].sum()) * value if value is not None else int(sel[b, 0::2].sum()) * (P - 1)
        assert [int(x) for x in want[b]] == [(s + deltas[b] * int(t)) % P for t in ssp[0]], f"the reference misses the closed form at statement {b}"


# ================================================================================ C. the generator ===========================================
def all_crafted(slots):
    return [c for slot in slots for c in wr.crafted_seeds(slot)]


def craft_id(c):
    return f"slot{c[1]}-k{c[2]}-raw{c[3]:#x}"


def test_prg_fill_equals_the_restatement(gpu_ctx_factory, mf):
    """mfh_ssp_prg_fill, slots 1 .. m + 1: the seed of the other tests, 0, 2^64 - 1, and every crafted seed (whose image holds the coefficient raw - p
    at its (slot, k), a value below 5); the last slots a 2^20-constraint instance has, too"""
    d, m = 128, 100
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        for seed, slot, k, raw in [(PRG_SEED, None, None, None), (0, None, None, None), ((1 << 64) - 1, None, None, None)] + all_crafted((1, 2, 3, 5)):
            got = c.to_host(c.ssp_prg_fill(seed, 1, m + 1), np.uint32).reshape(m + 1, d)
            want = wr.prg_image(seed, 1, m + 1, d)
            assert_exact(got, want.astype(np.uint64), "k_ssp_prg_fill", f" seed {seed:#x} (statement = slot - 1)")
            assert int(got.max()) < P
            if slot is not None:
                assert int(got[slot - 1, k]) == raw - P
        got = c.to_host(c.ssp_prg_fill(PRG_SEED, 1 << 20, 3), np.uint32).reshape(3, d)
        assert_exact(got, wr.prg_image(PRG_SEED, 1 << 20, 3, d).astype(np.uint64), "k_ssp_prg_fill", " slots 2^20 .. 2^20 + 2")
    finally:
        c.close()


@pytest.mark.parametrize("crafted", wr.crafted_seeds(5), ids=craft_id)
def test_raw_values_at_and_above_p_through_every_generated_form(gpu_ctx_factory, mf, crafted):
    """slot 5 is v_4 (bit 3).  Statement 0 selects only that row with delta = 0, so w_0[k] at the crafted k is the coefficient raw - p itself: a kernel that
    lets the raw value through shows 0xfffffffb .. 0xffffffff there.  Statement 1 selects every row, the others are random: the forms that sum RAW
    values and reduce once (all but k_ssp_prg_fill) must come out congruent.  The VALU form alone and for 12 statements, k_witness_mm_prg<1, 2, 4> and
    k_witness_mm8q_prg."""
    seed, slot, k, raw = crafted
    d, m = 128, 100
    ssp = generated_ssp(seed, m, d)
    assert int(ssp[slot, k]) == raw - P and int(wr.prg_raw(wr.prg_rowkey(seed, slot), k)) == raw
    nbytes = (m + 6) // 8
    rng = np.random.default_rng(raw & 0xFF)
    only_v4 = bytes([1 << 3]) + bytes(nbytes - 1)
    bits = [only_v4, b"\xff" * nbytes] + [rng.bytes(nbytes) for _ in range(127)]
    deltas = [0, P - 1] + [int(x) for x in rng.integers(0, P, size=127, dtype=np.uint64)]
    want = wr.w_polys(ssp, bits, deltas, m)
    assert int(want[0, k]) == raw - P
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        register(c, ssp, False, seed)
        for b in (0, 1):
            assert_exact(c.to_host(c.witness_poly(None, bits[b], deltas[b]), np.uint32), want[b: b + 1], "k_witness_partial_prg + k_witness_finish", f" statement {b}")
        for n in (2, 12):
            assert_exact(c.to_host(c.witness_poly_many(None, bits[:n], deltas[:n], mm=False), np.uint32), want[:n], f"k_witness_partial_multi_prg<12>, {n} statements")
        for n in (2, 33, 65, 129):
            plan = mm_plan(m, n, d, False)
            assert_exact(c.to_host(c.witness_poly_many(None, bits[:n], deltas[:n], mm=True), np.uint32), want[:n], plan.form, f" [{plan}]")
    finally:
        c.close()


def evals(rows, s):
    """[row(s) mod p] in Python integers"""
    pw = [pow(s, k, P) for k in range(len(rows[0]))]
    return [sum(int(a) * b for a, b in zip(row, pw)) % P for row in rows]


@pytest.mark.parametrize("crafted", all_crafted((1, 2, 3)), ids=craft_id)
def test_raw_values_at_and_above_p_in_setup_vk_and_v(gpu_ctx_factory, mf, crafted):
    """seeds crafted at slot 1 (v_0) and at slots 2 and 3 (v_1, v_2: the public rows of lu = 2): the setup messages s^k | alpha s^k | beta t(s), beta v_r(s) and
    the verification key t(s), v_0(s), v_1(s), v_2(s) equal powers and dot products in Python integers at s = 0, 1, p - 1 and a random s; v of the batch chain
    equals w + v_0"""
    seed, slot, k, raw = crafted
    d, m = 128, 24
    ssp = generated_ssp(seed, m, d)
    assert int(ssp[slot, k]) == raw - P
    rng = np.random.default_rng(raw & 0xFF)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        register(c, ssp, False, seed)
        rows = [ssp[0].tolist()] + [ssp[r + 1].tolist() for r in range(1, m)]  # message 2d + r: t for r = 0, v_r for r >= 1
        vk_rows = [ssp[i].tolist() for i in range(4)]
        for s in (0, 1, P - 1, int(rng.integers(2, P - 1))):
            alpha, beta = (int(x) for x in rng.integers(1, P, size=2, dtype=np.uint64))
            got = [int(x) for x in c.to_host(c.setup_messages(None, alpha, beta, s), np.uint32)]
            pw = [pow(s, i, P) for i in range(d)]
            assert got[:d] == pw and got[d: 2 * d] == [alpha * x % P for x in pw], f"s = {s}: powers"
            want = [beta * e % P for e in evals(rows, s)]
            assert got[2 * d:] == want, f"s = {s}: beta v_r(s) differs first at r = {[g == w for g, w in zip(got[2 * d:], want)].index(False)}"
            assert [int(x) for x in c.to_host(c.derive_vk(None, s, 2), np.uint32)] == evals(vk_rows, s), f"s = {s}: verification key"
        nstmt = 14
        bits, deltas = statements(rng, m, nstmt)
        want = wr.w_polys(ssp, bits, deltas, m)
        c.ssp_prepare(None)
        whv = c.to_host(c.batch_chain(None, bits, deltas), np.uint32).reshape(3, nstmt, d)
        assert_exact(whv[0], want, mm_plan(m, nstmt, d, False).form, ": w of the chain")
        assert_exact(whv[2], (want + ssp[1].astype(np.uint64)[None, :]) % np.uint64(P), "k_add_slot_multi", ": v = w + v_0 of the chain")
    finally:
        c.close()


@pytest.mark.parametrize("crafted", all_crafted((1, 2, 3)), ids=craft_id)
def test_raw_values_at_and_above_p_in_the_public_v_step(gpu_ctx_factory, mf, crafted):
    """mfh_prove_batch_public with lu = 2 under the crafted seeds: its V step adds v_0 and the selected public rows v_1, v_2 (slots 1 - 3) from the
    generator.  The binding exposes no chain-level output of it, so this goes through the composition identity of tests/test_gpu_public_inputs.py:
    (h, hat_h, hat_v) of mfh_prove on (u || w), (v_w, b_w) of mfh_prove on (0^lu || w) -- mfh_prove's own w and v under these seeds are what the
    tests above hold against the reference."""
    import torch

    import oracle_lib as ol

    seed, slot, k, raw = crafted
    d, m, lu = 128, 24, 2
    rng = np.random.default_rng(raw & 0xFF)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    p = c.params
    try:
        c.set_seed(SEED)
        nbytes = (m + 7) // 8
        sat = rng.bytes(nbytes)
        d_t = c.ssp_prg_make_t(seed, sat)
        c.ssp_set_prg(seed, d_t)
        c.ssp_prepare(None)
        alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
        d_sk, d_err = c.to_device(ol.rand_values(rng, p.n, p.L, p.logq)), c.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
        d_crs = c.setup_public(None, alpha, beta, s, lu, d_sk, d_err)
        stmts = [bytes([x[0] & 0xFC | u]) + x[1:] for u, x in enumerate([sat, rng.bytes(nbytes), rng.bytes(nbytes), sat])]  # every statement u = 0 .. 3
        nb = len(stmts)
        deltas = [int(x) for x in rng.integers(0, P, size=nb, dtype=np.uint64)]
        mags = [rng.bytes(400) for _ in range(nb)]
        signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
        got = c.prove_batch_public(d_crs, None, lu, stmts, deltas, mags, signs).clone().view(nb, -1)
        for b in range(nb):
            full = c.prove(d_crs, None, stmts[b], deltas[b], mags[b], signs[b]).clone().view(5, -1)
            zero = c.prove(d_crs, None, bytes([stmts[b][0] & 0xFC]) + stmts[b][1:], deltas[b], mags[b], signs[b]).clone().view(5, -1)
            assert torch.equal(got[b], torch.cat([full[:3], zero[3:]]).reshape(-1)), f"statement {b} (u = {b})"
    finally:
        c.close()


@pytest.mark.parametrize("seed", [PRG_SEED] + [c[0] for c in all_crafted((1, 5))], ids=lambda s: f"{s:#x}")
def test_prg_make_t(gpu_ctx_factory, mf, seed):
    """mfh_ssp_prg_make_t: t = v_0 + sum of the selected rows - 1 (random_ssp's definition), for a statement that selects no row, one row, every row and
    random ones; with seeds whose v_0 (slot 1) or v_4 (slot 5) holds a raw value >= p (the sum is formed from raw values, v_0 from the coefficient)"""
    d, m = 132, 100
    ssp = generated_ssp(seed, m, d)
    nbytes = (m + 6) // 8
    rng = np.random.default_rng(seed & 0xFFFF)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        for what, bits in (("no row", bytes(nbytes)), ("only v_4", bytes([8]) + bytes(nbytes - 1)), ("every row", b"\xff" * nbytes), ("random", rng.bytes(nbytes))):
            zero_t = np.concatenate([np.zeros((1, d), dtype=np.uint32), ssp[1:]])
            want = (wr.w_polys(zero_t, [bits], [0], m)[0] + ssp[1].astype(np.uint64)) % np.uint64(P)
            want[0] = (int(want[0]) - 1) % P
            assert_exact(c.to_host(c.ssp_prg_make_t(seed, bits), np.uint32), want[None, :], "k_witness_partial_prg + k_ssp_prg_make_t", f": {what}")
    finally:
        c.close()
