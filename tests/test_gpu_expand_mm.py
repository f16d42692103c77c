"""The matrix-core CRS image (k_expand_mm, csrc/expandmm.hip; mfh_crs_expand_mm*) against the keystream, byte for byte.

The expected image is tests/expand_mm_ref.py: the layout of DESIGN 3 stated in numpy (pinned on the CPU by test_expand_mm_ref_cpu.py), fed with the oracle's AES-CTR
stream.  Every comparison is for EQUALITY OF BYTES; n = 1470 and the seed of test_gpu_evalmm.py throughout.  An image is expanded into a buffer with 4 KiB guard bands on
both sides, prefilled with a pattern that holds neither 0 nor 0x80: afterwards the guards and every UNWRITTEN byte must still hold the pattern, DATA must be the reference,
and under the barrier-free writer (path 0) PAD must be 0x80.  The DATA bytes compared are counted in every case and must be nrows (n + 1) 88 (logq 736) or 184 (1472).
Two rows of b per region are crafted: all 0x00 (stored 0x80) and all 0xFF (stored 0x7F).

a. shapes, periods per chunk automatic, both logq, both writers (the LDS-tile writer, path 1, is held to DATA and the guards only: it writes whole 256-row stages):
   (d, m) = (256, 64) whole, as rank 1 of 3, as rank 5 of 256 (single rows that start at odd absolute rows 5 and 261: at logq 736 the opposite block phase to a row-0
   start, one live lane); (320, 321) whole (320 rows: 5 k-steps written, 3 unwritten; 321: 6 written, 63 spill rows) and as rank 1 of 3 (the BT+BV share starts at odd
   row 2 d + 107, 107 rows, 21 spill rows).
b. every period chunk: mfh_set_expand_periods 2 .. 10 on the whole (256, 64) image, and 3 and 10 on the odd-row shares of rank 5 of 256.  Regions this small select 2 on
   their own; 10 periods are the 231 consecutive counter blocks per lane that the kernel's two sets of span constants are sized for (configs 4 / 5).  256 rows of 8452.5
   blocks each spread the first block of a chunk over every residue mod 256, so the span crossing falls on every block position; 368 / 736 periods per row are no multiple
   of 3, 6, 7, 9, 10: the last chunk of a row is short.
c. stream byte 2^36 (counter block 2^32): Params(d = 2^20, m = 64) as world 4096, so that every S share is 256 rows; the rank whose S share holds the row in which byte 2^36
   falls (1984 at logq 736, 992 at 1472, computed here), and the next rank, whose rows lie wholly beyond; periods automatic and 10.  (Span constants built from the
   counter's low word alone fail here and nowhere else in this file.)
d. what the consumers may depend on: at (256, 300) with 70 statements, mfh_prove_batch, and mfh_eval_rows_multi over the AS region (3 and 40 vectors) and the BT+BV region
   (300 rows, a ragged stage: one-byte columns, and 3 and 40 four-byte vectors), from an image expanded into zeros, into 0x7F (A' = +127 wherever the writer leaves a byte),
   into random bytes, and from the reference image with every byte that is not DATA random: the same bytes as without an image, each time.  The last one ties the
   reference's classes to the consumer: a byte the reference calls free is free.  (A DATA byte is not: one flipped bit changes the proofs.)
e. the knob end to end: mfh_prove_batch with its transient image under 10 periods per chunk and under 2 returns the same bytes; the setter's argument errors.
"""
import os
import sys

import numpy as np
import pytest

import expand_mm_ref as xr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes((5 * i + 9) & 0xFF for i in range(40))  # the seed of test_gpu_evalmm.py
GUARD = 4096
STREAM_ROWS = 961  # rows 0 .. 960 of the stream hold every region of (256, 64), (256, 300) and (320, 321)


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


@pytest.fixture(scope="module")
def contexts(gpu_ctx_factory):
    made = {}

    def get(p):
        if p not in made:
            made[p] = gpu_ctx_factory(p)
            made[p].set_seed(SEED)
        return made[p]

    return get


@pytest.fixture(scope="module")
def stream(oracle):
    """the oracle's keystream of rows [row0, row0 + nrows): one call per logq for the head of the stream, one per region elsewhere; never changed"""
    head, far = {}, {}

    def get(p, row0, nrows):
        if row0 + nrows <= STREAM_ROWS:
            if p.logq not in head:
                head[p.logq] = np.frombuffer(oracle.keystream(SEED, 0, STREAM_ROWS * p.ctr_ct), dtype=np.uint8)
            return head[p.logq][row0 * p.ctr_ct: (row0 + nrows) * p.ctr_ct]
        if (p.logq, row0, nrows) not in far:
            far[p.logq, row0, nrows] = np.frombuffer(oracle.keystream(SEED, row0 * p.ctr_ct, nrows * p.ctr_ct), dtype=np.uint8)
        return far[p.logq, row0, nrows]

    return get


def share_regions(p, rank, world):
    """[(first absolute row, rows)] of the S, AS and BT+BV shares of a rank (include/mfhip.h: mfh_crs_expand_mm_share)"""
    lo_s, lo_b = p.d * rank // world, p.m * rank // world
    n_s, n_b = p.d * (rank + 1) // world - lo_s, p.m * (rank + 1) // world - lo_b
    return [(lo_s, n_s), (p.d + lo_s, n_s), (2 * p.d + lo_b, n_b)]


def region_bytes(p, nrows):
    return xr.geometry(p)[2] * xr.ksteps(nrows)[0] * 1024


def crafted_crs(p, regions, seed):
    """random compressed ciphertexts for the whole CRS; in every region the first row all 0x00 and the last all 0xFF (a single-row region: one of the two)"""
    c8 = np.random.default_rng(seed).integers(0, 256, size=((2 * p.d + p.m), p.ctb), dtype=np.uint8)
    for k, (row0, nrows) in enumerate(regions):
        if nrows >= 2:
            c8[row0], c8[row0 + nrows - 1] = 0x00, 0xFF
        elif nrows == 1:
            c8[row0] = 0xFF if k & 1 else 0x00
    return c8


class Ref:
    """the reference image and the classes of one region, on the device"""

    def __init__(self, torch, dev, p, keystream, c8_rows, nrows):
        image, cls = xr.image_ref(p, keystream, c8_rows, nrows)
        self.nrows, self.nbytes = nrows, image.size
        self.want_data = nrows * (p.n + 1) * (88 if p.logq == 736 else 184)
        self.image = torch.from_numpy(image.reshape(-1)).to(dev)
        self.cls = torch.from_numpy(cls.reshape(-1)).to(dev)


def share_refs(torch, ctx, stream, regions, c8):
    p = ctx.params
    return [Ref(torch, ctx.device, p, stream(p, row0, nrows), c8[row0: row0 + nrows], nrows) if nrows else None for row0, nrows in regions]


def pattern(torch, dev, nbytes):
    """1 .. 113, repeating: never 0 (a cleared buffer), never 0x80 (A = 0)"""
    return (torch.arange(nbytes, device=dev, dtype=torch.int32) % 113 + 1).to(torch.uint8)


def _none(torch, wrong, what):
    bad = int(wrong.sum())
    assert bad == 0, f"{what}: {bad} bytes differ, the first at {int(torch.nonzero(wrong)[0])}"


def expand_and_check(torch, ctx, d_crs, rank, world, refs, path=0):
    """one expansion into a guarded, patterned buffer, and the byte checks of every region"""
    nbytes = sum(r.nbytes for r in refs if r)
    assert nbytes == int(ctx.lib.mfh_crs_mm_share_bytes(ctx._h, rank, world))
    pat = pattern(torch, ctx.device, nbytes + 2 * GUARD)
    buf = pat.clone()
    ctx.set_expand_path(path)
    try:
        ctx.crs_expand_mm_share(d_crs, rank, world, out=buf[GUARD: GUARD + nbytes])
    finally:
        ctx.set_expand_path(0)
    assert torch.equal(buf[:GUARD], pat[:GUARD]), "the guard band in front of the image was written"
    assert torch.equal(buf[GUARD + nbytes:], pat[GUARD + nbytes:]), "the guard band behind the image was written"
    base = GUARD
    for k, r in enumerate(refs):
        if not r:
            continue
        got, was = buf[base: base + r.nbytes], pat[base: base + r.nbytes]
        base += r.nbytes
        data = r.cls == xr.DATA
        assert int(data.sum()) == r.want_data
        _none(torch, (got != r.image) & data, f"region {k}, data")
        if path == 0:
            _none(torch, (got != 0x80) & (r.cls == xr.PAD), f"region {k}, padding")
            _none(torch, (got != was) & (r.cls == xr.UNWRITTEN), f"region {k}, unwritten k-steps")
    return buf[GUARD: GUARD + nbytes]


# ---- a. shapes ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logq", [736, 1472])
@pytest.mark.parametrize("d,m,rank,world", [(256, 64, 0, 1), (256, 64, 1, 3), (256, 64, 5, 256), (320, 321, 0, 1), (320, 321, 1, 3)])
def test_shapes_under_both_writers(mf, torch, contexts, stream, logq, d, m, rank, world):
    p = mf.Params(logq=logq, d=d, m=m)
    ctx = contexts(p)
    regions = share_regions(p, rank, world)
    if world == 256:  # single rows at odd absolute rows: at logq 736 they start at byte 8 of an AES block
        assert regions == [(5, 1), (261, 1), (513, 0)] and (logq == 1472 or all((row0 * p.ctr_ct) % 16 == 8 for row0, _ in regions[:2]))
    if (d, world) == (320, 1):
        assert [(xr.ksteps(n)[1], 64 * xr.ksteps(n)[1] - n, xr.ksteps(n)[0]) for _, n in regions] == [(5, 0, 8), (5, 0, 8), (6, 63, 8)]
    if (d, world) == (320, 3):
        assert regions[2] == (2 * d + 107, 107) and 64 * xr.ksteps(107)[1] - 107 == 21
    c8 = crafted_crs(p, regions, 100 * d + world)
    d_crs = ctx.to_device(c8)
    refs = share_refs(torch, ctx, stream, regions, c8)
    for path in (0, 1):
        expand_and_check(torch, ctx, d_crs, rank, world, refs, path)


# ---- b. every period chunk ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logq", [736, 1472])
def test_every_period_chunk(mf, torch, contexts, stream, logq):
    p = mf.Params(logq=logq, d=256, m=64)
    ctx = contexts(p)
    whole, odd = share_regions(p, 0, 1), share_regions(p, 5, 256)
    c8 = crafted_crs(p, whole + odd, 4000 + logq)
    d_crs = ctx.to_device(c8)
    refs = share_refs(torch, ctx, stream, whole, c8)
    refs_odd = share_refs(torch, ctx, stream, odd, c8)
    first = None
    try:
        for periods in range(2, 11):
            ctx.set_expand_periods(periods)
            image = expand_and_check(torch, ctx, d_crs, 0, 1, refs)
            if first is None:
                first = image
            else:  # 256-row regions have no spill and no unwritten byte: the whole image is pinned, and identical for every value
                assert torch.equal(image, first), periods
        for periods in (3, 10):
            ctx.set_expand_periods(periods)
            expand_and_check(torch, ctx, d_crs, 5, 256, refs_odd)
    finally:
        ctx.set_expand_periods(0)


# ---- c. stream byte 2^36 -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logq", [736, 1472])
def test_counter_block_two_to_the_32(mf, torch, contexts, stream, logq):
    p = mf.Params(logq=logq, d=1 << 20, m=64)
    world = 4096
    rstar = (1 << 36) // p.ctr_ct  # the row in which stream byte 2^36 falls
    rank = rstar // 256
    assert rank == (1984 if logq == 736 else 992)
    ctx = contexts(p)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(36 + logq)
    d_crs = torch.randint(0, 256, ((2 * p.d + p.m) * p.ctb,), dtype=torch.uint8, device=ctx.device, generator=g)  # (only the shares' rows are read)
    try:
        for rk in (rank, rank + 1):
            regions = share_regions(p, rk, world)
            row0, nrows = regions[0]
            assert nrows == 256 and regions[1] == (p.d + row0, 256)
            if rk == rank:
                assert row0 < rstar < row0 + nrows - 1 and row0 * p.ctr_ct < 1 << 36 < (row0 + nrows) * p.ctr_ct
            else:
                assert row0 * p.ctr_ct > 1 << 36
            c8 = ctx.to_host(d_crs[row0 * p.ctb: (row0 + nrows) * p.ctb]).reshape(nrows, p.ctb)
            ref = Ref(torch, ctx.device, p, stream(p, row0, nrows), c8, nrows)
            for periods in (0, 10):
                ctx.set_expand_periods(periods)
                nbytes = int(ctx.lib.mfh_crs_mm_share_bytes(ctx._h, rk, world))
                assert nbytes == 2 * ref.nbytes + sum(region_bytes(p, n) for _, n in regions[2:])
                pat = pattern(torch, ctx.device, nbytes + 2 * GUARD)
                buf = pat.clone()
                ctx.crs_expand_mm_share(d_crs, rk, world, out=buf[GUARD: GUARD + nbytes])
                assert torch.equal(buf[:GUARD], pat[:GUARD]) and torch.equal(buf[GUARD + nbytes:], pat[GUARD + nbytes:])
                got = buf[GUARD: GUARD + ref.nbytes]  # the S share
                data = ref.cls == xr.DATA
                assert int(data.sum()) == ref.want_data
                _none(torch, (got != ref.image) & data, f"rank {rk}, periods {periods}, data")
                _none(torch, (got != 0x80) & (ref.cls == xr.PAD), f"rank {rk}, periods {periods}, padding")
    finally:
        ctx.set_expand_periods(0)


# ---- d, e. the consumers -----------------------------------------------------------------------------------------------------------------------------------------------
class _Batch:
    """(d, m) = (256, 300), 70 statements; what the prover and the evaluations return WITHOUT an image (keystream regenerated per group): once per module, never changed"""

    def __init__(self, mf, torch, ctx, stream):
        sys.path.insert(0, ROOT)
        import bench

        self.ctx, self.p = ctx, ctx.params
        p = self.p
        inst = bench.build_instance(mf, ctx, torch, p, 7 * p.d + p.m)
        ctx.ssp_prepare(inst["d_ssp"])
        self.d_ssp = inst["d_ssp"]
        self.d_crs = ctx.setup(inst["d_ssp"], inst["alpha"], inst["beta"], inst["s"], inst["sk"], inst["err"])
        rng = np.random.default_rng(p.d + 70)
        nbytes = (p.m + 7) // 8
        bits = [inst["bits"] if b % 3 != 2 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for b in range(70)]
        self.stmts = (bits, [int(x) for x in rng.integers(0, ol.P, size=70, dtype=np.uint64)],
                      [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(70)],
                      [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(70)])
        co = rng.integers(0, ol.P, size=(40, max(p.d, p.m)), dtype=np.uint64).astype(np.uint32)
        co[0, :] = 0xFFFFFFFA  # p - 1 everywhere: the largest digits
        co[1, :] = 0xFFFFFFFF
        self.evals = []  # (stream offset, rows, c8, coefficients, vectors, coefficient bytes)
        as_c8, bt_c8 = self.d_crs[p.d * p.ctb:], self.d_crs[2 * p.d * p.ctb:]
        for nvec in (3, 40):
            self.evals.append((p.ctr_as, p.d, as_c8, ctx.to_device(np.ascontiguousarray(co[:nvec, : p.d])), nvec, 4))
            self.evals.append((p.ctr_bt, p.m, bt_c8, ctx.to_device(np.ascontiguousarray(co[:nvec, : p.m])), nvec, 4))
        cb = rng.integers(0, 256, size=(7, p.m), dtype=np.uint32)
        cb[0, :] = 255
        self.evals.append((p.ctr_bt, p.m, bt_c8, ctx.to_device(cb), 7, 1))
        ctx.set_resident_mm(None)
        ctx.set_batch_image(False)
        try:
            self.want = self.prove().clone()
        finally:
            ctx.set_batch_image(True)
        self.want_evals = [self.eval(e).clone() for e in self.evals]
        self.regions = share_regions(p, 0, 1)
        c8 = ctx.to_host(self.d_crs).reshape(2 * p.d + p.m, p.ctb)
        self.refs = [xr.image_ref(p, stream(p, row0, nrows), c8[row0: row0 + nrows], nrows) for row0, nrows in self.regions]

    def prove(self):
        return self.ctx.prove_batch(self.d_crs, self.d_ssp, *self.stmts)

    def eval(self, e):
        off, nrows, c8, co, nvec, cb = e
        return self.ctx.eval_rows_multi(off, nrows, c8, co, nvec, coeff_bytes=cb)


@pytest.fixture(scope="module")
def batch(mf, torch, contexts, stream):
    return _Batch(mf, torch, contexts(mf.Params(d=256, m=300)), stream)


@pytest.mark.parametrize("kind", ["zeros", "x7f", "random", "reference"])
def test_no_result_depends_on_a_byte_that_is_not_data(torch, batch, kind):
    b, ctx = batch, batch.ctx
    nbytes = int(ctx.lib.mfh_crs_mm_image_bytes(ctx._h))
    assert nbytes == sum(im.size for im, _ in b.refs)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(len(kind))
    noise = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=ctx.device, generator=g)
    if kind == "reference":  # built on the host: DATA from the reference, every other byte random
        ref = torch.cat([torch.from_numpy(im.reshape(-1)) for im, _ in b.refs]).to(ctx.device)
        data = torch.cat([torch.from_numpy(cl.reshape(-1)) for _, cl in b.refs]).to(ctx.device) == xr.DATA
        assert int(data.sum()) == (2 * b.p.d + b.p.m) * (b.p.n + 1) * 88
        image = torch.where(data, ref, noise)
    else:
        image = {"zeros": torch.zeros_like(noise), "x7f": torch.full_like(noise, 0x7F), "random": noise}[kind]
        ctx.crs_expand_mm(b.d_crs, out=image)
    ctx.set_resident_mm(image)
    try:
        assert torch.equal(b.prove(), b.want), "prove_batch"
        for e, want in zip(b.evals, b.want_evals):
            assert torch.equal(b.eval(e), want), ("eval_rows_multi", e[0], e[1], e[4], e[5])
        if kind == "reference":  # the image is what every one of these calls read: one bit of one DATA byte of a region changes what is computed from that region
            base = 0
            for region, (im, _) in enumerate(b.refs):
                at = base + 1024 + 17  # row tile 0, k-step 1 of the region: position 1 of row 65
                base += im.size
                assert bool(data[at])
                image[at] ^= 1
                assert not torch.equal(b.prove(), b.want), region  # (row 65 of BT+BV is wire 64: set in some of the 70 statements)
                for e, want in zip(b.evals, b.want_evals):
                    assert torch.equal(b.eval(e), want) == (e[0] != (0, b.p.ctr_as, b.p.ctr_bt)[region]), (region, e[0], e[4], e[5])
                image[at] ^= 1
    finally:
        ctx.set_resident_mm(None)


def test_prove_batch_under_forced_periods(torch, batch):
    """the transient image of mfh_prove_batch (70 statements: more than 31, so the call expands the CRS into scratch and streams it) is written under the knob too"""
    b, ctx = batch, batch.ctx
    ctx.set_resident_mm(None)
    ctx.set_batch_image(True)
    try:
        for periods in (10, 2):
            ctx.set_expand_periods(periods)
            assert torch.equal(b.prove(), b.want), periods
    finally:
        ctx.set_expand_periods(0)


def test_the_setter_checks_its_range(mf, contexts):
    ctx = contexts(mf.Params(d=256, m=64))
    for bad in (1, 11, 12, 256, 1 << 31, (1 << 32) - 1):
        with pytest.raises(mf.MfhError):
            ctx.set_expand_periods(bad)
    with pytest.raises(mf.MfhError):
        ctx.set_expand_periods(-1)
    for ok in (2, 10, 0):
        ctx.set_expand_periods(ok)
    assert ctx.lib.mfh_set_expand_periods(None, 2) != 0
