"""The exact-integer kernels driven to the bounds their correctness arguments rest on, against Python integers.

Every kernel on the proof path does exact multi-word arithmetic that is right only because of a bound: int32 MFMA accumulators of at most
131 071 rows (csrc/evalmm.hip), the recombined records of the streaming kernels (|T| < 2^56, |U| < 2^80), 22- or 46-word carry chains
with the modq wrap at 2^(64 K), 56-bit lanes with 8 bits of headroom for 256 ranks.  Random or AES operands stay far from all of them
(A' = A - 128 averages zero), so the operands here are crafted: constant matrix-core images, all-ones limb planes, coefficients chosen
from the signs of the keystream bytes.  Expected values are closed forms or exact numpy byte sums recombined with Python integers,
never another GPU kernel alone.  Each test's docstring says which bound it reaches and how close it gets.
(The witness GEMM's offset-by-128 bytes and its 128 cnt_b correction: tests/test_gpu_witness_exact.py, part B.)
"""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

SEED = bytes((11 * i + 3) & 0xFF for i in range(40))
PM1 = ol.P - 1  # 0xFFFFFFFA


def _mod(p):
    return 1 << (64 * p.K)


def _rep(byte, nbytes):
    """the value whose nbytes little-endian bytes all equal `byte`"""
    return int.from_bytes(bytes([byte]) * nbytes, "little")


def _limbs(x, p):
    return ol.int_to_limbs(x % _mod(p), p.L)


def _release(c):
    """close a large context and hand its memory back (the caller has dropped its own references first)"""
    import torch

    c.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ A. streaming matrix-core path
def _mm_vectors(rng, nvec, nrows):
    """coefficient vectors at the digit extremes: all 0 (C' = -128 in every digit column: every product with A' = -128 is +16384),
    all p - 1, every byte 255, one digit set, 0 / p - 1 alternating by row, random"""
    kinds = [np.zeros(nrows, np.uint32), np.full(nrows, PM1, np.uint32), np.full(nrows, 0xFFFFFFFF, np.uint32)]
    kinds += [np.full(nrows, 1 << (8 * w), np.uint32) for w in range(4)]
    alt = np.zeros(nrows, np.uint32)
    alt[1::2] = PM1
    kinds.append(alt)
    co = np.stack([kinds[v % (len(kinds) + 1)] if v % (len(kinds) + 1) < len(kinds) else
                   rng.integers(0, ol.P, size=nrows, dtype=np.uint64).astype(np.uint32) for v in range(nvec)])
    co[nvec - 1] = rng.integers(0, ol.P, size=nrows, dtype=np.uint64).astype(np.uint32)
    return co


def _check_const(got, co, X, p, base=None, what=""):
    """got: nvec x (n + 1) x L; every coordinate (b included) of vector v must be base + (sum_i c_v[i]) X mod 2^(64 K)"""
    for v in range(co.shape[0]):
        want = (int(co[v].astype(np.uint64).sum()) * X + (base or 0)) % _mod(p)
        ok = (got[v] == _limbs(want, p)[None, :]).all(axis=1)
        assert ok.all(), f"{what} vector {v}: coordinates {np.flatnonzero(~ok)[:8]} differ from the closed form"


@pytest.mark.parametrize("logq,d", [(736, 131072), (1472, 131072), (736, 130816)])
def test_streaming_path_on_a_constant_image(logq, d):
    """k_mmstream1 + k_evalmm_finish (packed records on and off) over a registered matrix-core image of one constant byte.  A' = -128 with
    all-zero coefficients (C' = -128) makes every product +16384, so an accumulator of r rows holds exactly 16384 r:
      d = 131 072 rows (one region, past one chunk): correct chunking makes two chunks of 65 536 and holds every accumulator at exactly
        2^30, half the bound; the regression of a single 131 072-row chunk would put it at exactly 2^31, where it wraps, and this test
        catches that;
      d = 130 816 rows (the largest whole number of 256-row stages below 131 071): ONE chunk holds every row, and every accumulator sits
        at 2^31 - 2^22, within 0.2 % of the bound -- the closest correct chunking gets to it.
    Also A' = +127 and A' = 0 (stored bytes 0xFF, 0x00: the image holds A - 128), chunk limits 0 / 131 071 / 40 001 / 16 384 (8 chunks),
    1, 63 and 255 (one-byte) vectors and an accumulating call.  Expected: every coordinate, b included, is (sum_i c_v[i]) X mod 2^(64 K)
    with X the value whose significant bytes all equal A.  (The image is 34 GB at logq 736 and 74 GB at 1472; the context is closed
    here, not left to the session.)"""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=d, m=64)
    c = mf.Context(p, 0)
    img = out = None
    try:
        c.set_seed(SEED)
        c.set_timing(True)
        nb = int(c.lib.mfh_crs_mm_image_bytes(c._h))
        img = c.empty(nb)
        c.set_resident_mm(img)
        dummy_c8 = c.zeros(256)
        rng = np.random.default_rng(logq)
        sbytes = 8 * p.K
        cases = [(0x80, 0), (0x7F, 255), (0x00, 128)]  # (stored byte, A): the stored byte is A' = A - 128 as int8
        co63 = _mm_vectors(rng, 63, p.d)
        co1 = co63[:1].copy()
        cb1 = np.stack([np.zeros(p.d, np.uint32), np.full(p.d, 255, np.uint32)] * 127 + [rng.integers(0, 256, p.d).astype(np.uint32)])
        d63, d1, dcb1 = c.to_device(co63), c.to_device(co1), c.to_device(cb1)
        for stored, A in cases:
            img.fill_(stored)
            X = A * _rep(1, sbytes)
            runs = [(0, True, d63, co63, 63, 4), (0, False, d63, co63, 63, 4), (131071, False, d1, co1, 1, 4), (40001, True, d63, co63, 63, 4),
                    (16384, True, d1, co1, 1, 4), (0, True, dcb1, cb1, 255, 1), (40001, False, dcb1, cb1, 255, 1)]
            if stored != 0x80:
                runs = runs[:2] + runs[5:6]
            for chunk, pack, dco, co, nvec, cb in runs:
                c.set_mm_chunk_rows(chunk)
                c.set_mm_pack(pack)
                c.timing_drain("evalmm_resident")
                c.timing_drain("evalmm")
                out = c.eval_rows_multi(p.ctr_s, p.d, dummy_c8, dco, nvec, coeff_bytes=cb)
                got = c.to_host(out, np.uint64).reshape(nvec, p.n + 1, p.L)
                assert c.timing_drain("evalmm_resident")[0] == 1 and c.timing_drain("evalmm")[0] == 0, "the image did not serve the call"
                _check_const(got, co, X, p, what=f"byte {stored:#x} chunk {chunk} pack {pack} nvec {nvec} cb {cb}:")
        # accumulate onto an all-ones output: (2^(64K) - 1) + sum X
        img.fill_(0x80)
        c.set_mm_chunk_rows(0)
        c.set_mm_pack(True)
        out = c.to_device(np.tile(_limbs(-1, p), 63 * (p.n + 1)))
        c.eval_rows_multi(p.ctr_s, p.d, dummy_c8, d63, 63, out=out, accumulate=True)
        _check_const(c.to_host(out, np.uint64).reshape(63, p.n + 1, p.L), co63, 0, p, base=-1, what="accumulate:")
        img.fill_(0x7F)
        c.eval_rows_multi(p.ctr_s, p.d, dummy_c8, d63, 63, out=out, accumulate=True)
        _check_const(c.to_host(out, np.uint64).reshape(63, p.n + 1, p.L), co63, 255 * _rep(1, sbytes), p, base=-1, what="accumulate 0x7f:")
    finally:
        c.set_resident_mm(None)
        img = out = None
        _release(c)


def test_batch_prover_on_constant_images(gpu_ctx_factory, oracle):
    """mfh_prove_batch streaming a constant matrix-core image (k_mmstream_p / k_evalmm_finish_groups) against mfh_prove over a limb-plane
    row image of the same constant (k_mac_resident): stored byte 0x7F (A' = +127) <-> every limb byte 0xFF, i.e. every coordinate of every
    row is 2^(64 K) - 1 and every product has the largest positive MFMA operand.  Satisfying, all-ones and random witnesses, 70 statements
    (a full S / AS group and a partial one), at the DEBUG shape: every product at its largest positive magnitude, 256 rows per region
    (far below the chunk bound, which test_streaming_path_on_a_constant_image comes within 0.2 % of).  delta = 0: the batch prover takes ct_t from
    the compressed CRS (keystream a), which a constant row image cannot encode."""
    import c_lwe_snarks_amd as mf

    p = mf.DEBUG
    c = gpu_ctx_factory(p)
    c.set_seed(SEED)
    rng = np.random.default_rng(3)
    nbytes = (p.m + 7) // 8
    wit = rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()
    ssp = oracle.ssp_from_tape(p, rng.integers(0, 256, size=p.m * 8 * p.d, dtype=np.uint8), wit)
    d_ssp = c.ssp_upload(ssp)
    c.ssp_prepare(d_ssp)
    d_crs = c.to_device(np.full((2 * p.d + p.m) * p.ctb, 0xFF, np.uint8))
    nb = 70
    stmts = [wit if b % 2 == 0 else (b"\xff" * nbytes if b % 4 == 1 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()) for b in range(nb)]
    deltas = [0] * nb
    mags = [(b"\xff" * 400) if b % 5 == 0 else rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for b in range(nb)]
    signs = [bytes([b & 1] * 5) for b in range(nb)]
    image = c.empty(int(c.lib.mfh_crs_mm_image_bytes(c._h))).fill_(0x7F)
    c.set_resident_mm(image)
    try:
        got = c.to_host(c.prove_batch(d_crs, d_ssp, stmts, deltas, mags, signs), np.uint64).reshape(nb, 5, p.n + 1, p.L).copy()
    finally:
        c.set_resident_mm(None)
    rows = c.empty((2 * p.d + p.m) * c.resident_row_bytes()).fill_(0xFF)
    c.set_resident(rows)
    try:
        for b in range(nb):
            one = c.to_host(c.prove(d_crs, d_ssp, stmts[b], deltas[b], mags[b], signs[b]), np.uint64).reshape(5, p.n + 1, p.L)
            assert np.array_equal(got[b], one), f"statement {b}"
    finally:
        c.set_resident(None)


# ------------------------------------------------------------------------------------------------ B. regenerating matrix-core path
def _targets(p, nvec, rng):
    """(coordinate, byte) target of every digit column (v, w): column- and row-tile edges of the 128- and 256-column kernels, and b"""
    j_edges = [0, 1, 2, 3, 4, 5, 7, 8, 511, 512, 735, 736, 1467, 1468, 1469, p.n]
    u_edges = [0, 15, 16, 31, 32, 63, 64, 79, 80, 87]
    return [(j_edges[(4 * v + w) % len(j_edges)], u_edges[(7 * v + 3 * w) % len(u_edges)] if (4 * v + w) % 3 else int(rng.integers(0, 88)))
            for v in range(nvec) for w in range(4)]


def _sign_coeffs(rowbytes, targets, nvec):
    """digit w of c_v[i] = 255 where the target byte of row i has A' >= 0 (A >= 128), else 0; the low digit capped so that c < p"""
    nrows = rowbytes[targets[0]].shape[0]
    co = np.zeros((nvec, nrows), np.uint64)
    for v in range(nvec):
        for w in range(4):
            j, u = targets[4 * v + w]
            co[v] |= np.where(rowbytes[(j, u)] >= 128, 255, 0).astype(np.uint64) << np.uint64(8 * w)
    co[co >= ol.P] = PM1
    return co.astype(np.uint32)


def _byte_sums(co, A):
    """S[v][u] = sum_i co[v][i] A[i][u] exactly: the coefficients split in 16-bit halves, so that every float64 partial sum of the
    matrix products stays below 2^16 x 2^8 x rows <= 2^53 (exact in any summation order) for up to 2^29 rows"""
    assert A.shape[0] <= 1 << 29
    Af = A.astype(np.float64)
    lo = (co & 0xFFFF).astype(np.float64) @ Af
    hi = (co >> 16).astype(np.float64) @ Af
    return (hi.astype(np.uint64) << np.uint64(16)) + lo.astype(np.uint64)


@pytest.mark.parametrize("nrows", [131071, 2 * 131071, 3 * 131071])
def test_regenerating_path_with_sign_matched_coefficients(nrows):
    """k_evalmm<4> (31 vectors) and k_evalmm16<0> (63 vectors) with each digit column's coefficients chosen from the sign of one target
    byte position's keystream byte, so that every product A'C' of that (byte position, digit column) is >= 0, 8160 on average (A
    cannot be crafted here).  With correct chunking the targeted accumulators reach about a quarter of the int32 bound: two chunks of
    65 536 rows at 131 071 rows (about 2^29), three of about 87 500 at 2 x 131 071 and four of 98 304 at 3 x 131 071 (about 2^29.4 -
    2^29.6).  A 256-column launch that lost its row chunking would put 3 x 131 071 rows in one accumulator, about 3.2e9 > 2^31, and
    this test catches that; a chunk of up to about 263 000 rows stays below 2^31 on average, so a merely doubled chunk is not caught here
    (test_streaming_path_on_a_constant_image catches the chunking errors of the image path exactly).  The int32-path epilogue terms
    (sum_i A C of true bytes) reach about 2^31.6, 2^32.6 and 2^33.2.  Targets lie on column- and row-tile edges and on b.  Every
    coordinate against eval_rows (k_eval); the targeted coordinates against exact numpy byte sums recombined with Python integers."""
    import c_lwe_snarks_amd as mf

    p = mf.DEBUG
    c = mf.Context(p, 0)
    try:
        _sign_matched_rows(c, p, nrows)
    finally:
        _release(c)


def _sign_matched_rows(c, p, nrows):
    c.set_seed(SEED)
    rng = np.random.default_rng(nrows)
    c8 = rng.integers(0, 256, size=nrows * p.ctb, dtype=np.uint8)
    d_c8 = c.to_device(c8)
    off = p.ctr_s
    for nvec in (31, 63):
        targets = _targets(p, nvec, rng)
        want_j = sorted({j for j, _ in targets})
        # the significant bytes of the targeted coordinates of every row, from the keystream (b from c8), in slabs of rows
        rowbytes = {}
        slab = 16384
        per_j = {j: [] for j in want_j}
        for r0 in range(0, nrows, slab):
            r1 = min(nrows, r0 + slab)
            ks = c.keystream(off + r0 * p.ctr_ct, (r1 - r0) * p.ctr_ct).view(r1 - r0, p.n, p.ctb)
            for j in want_j:
                if j < p.n:
                    per_j[j].append(c.to_host(ks[:, j, :8 * p.K].contiguous()).reshape(r1 - r0, 8 * p.K))
            del ks
        for j in want_j:
            A = np.concatenate(per_j[j]) if j < p.n else c8.reshape(nrows, p.ctb)[:, :8 * p.K]
            for u in range(8 * p.K):
                rowbytes[(j, u)] = A[:, u]
            rowbytes[("all", j)] = A
        co = _sign_coeffs(rowbytes, targets, nvec)
        got = c.to_host(c.eval_rows_multi(off, nrows, d_c8, c.to_device(co), nvec), np.uint64).reshape(nvec, p.n + 1, p.L)
        for v in range(0, nvec, 2):
            refs = c.eval_rows(off, nrows, d_c8, c.to_device(co[v]), c.to_device(co[v + 1]) if v + 1 < nvec else None)
            for k, ref in enumerate(refs[: min(2, nvec - v)]):
                assert np.array_equal(got[v + k], c.to_host(ref, np.uint64).reshape(p.n + 1, p.L)), f"{nvec} vectors: vector {v + k} differs from k_eval"
        for j in want_j:
            vs = sorted({v for v in range(nvec) for w in range(4) if targets[4 * v + w][0] == j})
            S = _byte_sums(co[vs], rowbytes[("all", j)])
            for k, v in enumerate(vs):
                want = sum(int(S[k, u]) << (8 * u) for u in range(8 * p.K)) % _mod(p)
                assert ol.limbs_to_int(got[v, j]) == want, f"{nvec} vectors: vector {v} coordinate {j}"


# ------------------------------------------------------------------------------------------------ C. VALU carry chains
@pytest.mark.parametrize("logq", [736, 1472])
def test_resident_mac_full_ripple(logq):
    """k_mac_resident + k_eval_reduce_*: a limb-plane row image of 0xFF (every word 0xFFFFFFFF: every 32 x 32 product carries through every
    word of the accumulator) with coefficients p - 1 on all 32 768 rows, one and two accumulators; and 0x00 / 0xFF accumulated onto an
    all-ones output.  Full ripple: every coordinate must be (-(sum c) + base) mod 2^(64 K)."""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=32768, m=64)
    c = mf.Context(p, 0)
    rows = None
    try:
        nrows = p.d
        rows = c.empty(nrows * c.resident_row_bytes())
        co = np.full(nrows, PM1, np.uint32)
        co2 = co.copy()
        co2[::3] = 1
        dco, dco2 = c.to_device(co), c.to_device(co2)
        s1, s2 = nrows * PM1, int(co2.astype(np.uint64).sum())
        ones = np.tile(_limbs(-1, p), p.n + 1)
        for fill in (0xFF, 0x00):
            rows.fill_(fill)
            X = -1 if fill == 0xFF else 0
            r0, r1 = c.eval_rows_resident(rows, 0, nrows, dco, dco2)
            (a,) = c.eval_rows_resident(rows, 0, nrows, dco)[:1]
            for got, s in ((r0, s1), (r1, s2), (a, s1)):
                g = c.to_host(got, np.uint64).reshape(p.n + 1, p.L)
                assert (g == _limbs(s * X, p)[None, :]).all(), f"fill {fill:#x}, sum {s}"
            acc0, acc1 = c.to_device(ones), c.to_device(ones)
            c.eval_rows_resident(rows, 0, nrows, dco, dco2, rop0=acc0, rop1=acc1, accumulate=True)
            for got, s in ((acc0, s1), (acc1, s2)):
                g = c.to_host(got, np.uint64).reshape(p.n + 1, p.L)
                assert (g == _limbs(s * X - 1, p)[None, :]).all(), f"accumulate, fill {fill:#x}"
    finally:
        rows = None
        _release(c)


@pytest.mark.parametrize("logq,path", [(736, 0), (736, 1), (1472, 0)])
def test_eval_all_ones_b_and_expanded_rows(gpu_ctx_factory, logq, path):
    """k_eval / k_eval_w with c8 all 0xFF and coefficients p - 1: coordinate n (b = 2^(64 K) - 1 after modq, full ripple in every
    product) against its closed form -(sum c) mod 2^(64 K); the keystream coordinates against k_mac_resident over the crs_expand image of
    the same rows."""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=64, m=16)
    c = gpu_ctx_factory(p)
    c.set_seed(SEED)
    nrows = 3000
    d_c8 = c.to_device(np.full(nrows * p.ctb, 0xFF, np.uint8))
    co = np.full(nrows, PM1, np.uint32)
    co2 = co.copy()
    co2[1::2] = 0xFFFFFFFA - 1
    dco, dco2 = c.to_device(co), c.to_device(co2)
    off = p.ctr_as + 5 * p.ctr_ct
    c.set_eval_path(path)
    try:
        r0, r1 = c.eval_rows(off, nrows, d_c8, dco, dco2)
    finally:
        c.set_eval_path(0)
    img = c.crs_expand(off, nrows, d_c8)
    e0, e1 = c.eval_rows_resident(img, 0, nrows, dco, dco2)
    for got, ref, cv in ((r0, e0, co), (r1, e1, co2)):
        g = c.to_host(got, np.uint64).reshape(p.n + 1, p.L)
        assert ol.limbs_to_int(g[p.n]) == (-int(cv.astype(np.uint64).sum())) % _mod(p)
        assert np.array_equal(g, c.to_host(ref, np.uint64).reshape(p.n + 1, p.L))


# ------------------------------------------------------------------------------------------------ D. element-wise, reduction, decryption
@pytest.mark.parametrize("logq", [736, 1472])
def test_elementwise_full_ripple(gpu_ctx_factory, oracle, logq):
    """ct_add / ct_mul_ui / ct_addmul_ui on all-ones values (with the bits above 2^(64 K) set in memory): (2^(64K) - 1) + 1 carries through
    every word to 0; all-ones x (p - 1) and rop + all-ones x (p - 1) ripple their high halves through every word.  Full ripple, against
    Python integers and the oracle."""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=64, m=16)
    c = gpu_ctx_factory(p)
    full = np.full((p.n + 1, p.L), 0xFFFFFFFFFFFFFFFF, np.uint64)  # every limb, those above K included
    one = np.zeros_like(full)
    one[:, 0] = 1
    M = _mod(p)
    cases = [(full, one, 0), (full, full, -2 % M), (one, full, 0)]
    for a, b, want in cases:
        g = c.to_host(c.ct_add(c.to_device(a), c.to_device(b)), np.uint64).reshape(full.shape)
        assert (g == _limbs(want, p)[None, :]).all()
        assert np.array_equal(g, oracle.ct_add(p, a, b))
    g = c.to_host(c.ct_mul_ui(c.to_device(full), PM1), np.uint64).reshape(full.shape)
    assert (g == _limbs(-PM1, p)[None, :]).all()
    assert np.array_equal(g, oracle.ct_mul_ui(p, full, PM1))
    rop = full.copy()
    rop[:, p.K:] = 0  # accumulators are reduced values
    d = c.to_device(rop)
    c.ct_addmul_ui(d, c.to_device(full), PM1)
    g = c.to_host(d, np.uint64).reshape(full.shape)
    assert (g == _limbs(-1 - PM1, p)[None, :]).all()
    assert np.array_equal(g, oracle.ct_addmul_ui(p, rop, full, PM1))


@pytest.mark.parametrize("logq", [736, 1472])
def test_add_dotp_every_term_all_ones(gpu_ctx_factory, oracle, logq):
    """k_add_dotp with all 1470 terms all-ones x all-ones (the truncated 32 x 32 products at their maximum, every partial word of every
    lane carrying) onto an all-ones rop: 1470 (2^(64K) - 1)^2 + 2^(64K) - 1 = 1469 mod 2^(64 K).  Full ripple."""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=64, m=16)
    c = gpu_ctx_factory(p)
    n = 1470
    a = np.tile(_limbs(-1, p), n)
    rop = _limbs(-1, p)
    d = c.to_device(rop)
    c.add_dotp(d, c.to_device(a), c.to_device(a), n)
    g = c.to_host(d, np.uint64)
    assert ol.limbs_to_int(g) == (n - 1) % _mod(p)
    assert np.array_equal(g, oracle.add_dotp(p, rop, a.reshape(n, p.L), a.reshape(n, p.L)))


@pytest.mark.parametrize("logq", [736, 1472])
def test_smudge_borrow_and_wrap(gpu_ctx_factory, oracle, logq):
    """k_smudge: b = 2^(64K - 1) minus p (a borrow through every word), all-ones b plus u p with u all-ones over 80 bytes (a wrap past
    2^(64 K)), b = 0 minus p (the negative result: the oracle flags it, the device reduces it mod 2^(64 K)).  Full ripple."""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=64, m=16)
    c = gpu_ctx_factory(p)
    M = _mod(p)
    rng = np.random.default_rng(logq)
    cases = [(1 << (64 * p.K - 1), 1, 1), (M - 1, _rep(255, 80), 0), (M - 1, 1, 0), (0, 1, 1), (5, _rep(255, 80), 1)]
    cts = ol.rand_values(rng, len(cases) * (p.n + 1), p.L, 64 * p.K).reshape(len(cases), p.n + 1, p.L)
    mags = b""
    for i, (b, u, s) in enumerate(cases):
        cts[i, p.n] = _limbs(b, p)
        mags += u.to_bytes(80, "little")
    signs = bytes(s for _, _, s in cases)
    d = c.to_device(cts)
    c.ct_smudge(d, len(cases), mags, 80, signs)
    got = c.to_host(d, np.uint64).reshape(cts.shape)
    for i, (b, u, s) in enumerate(cases):
        want = (b - u * ol.P if s else b + u * ol.P) % M
        assert ol.limbs_to_int(got[i, p.n]) == want, f"case {i}"
        assert np.array_equal(got[i, :p.n], cts[i, :p.n])
        exp, neg = oracle.ct_smudge(p, cts[i], mags[80 * i: 80 * i + 80], s)
        assert neg == (s == 1 and b < u * ol.P)
        assert np.array_equal(got[i], exp)


@pytest.mark.parametrize("logq", [736, 1472])
def test_decrypt_extreme_keys_and_ciphertexts(gpu_ctx_factory, oracle, logq):
    """k_decrypt and k_decrypt_mm (300 ciphertexts: more than one 256-row workgroup; at 1472 the Toeplitz GEMM splits its columns so that no
    accumulator sees more than 131 071 products) with every key coordinate of balanced digits all -128, then all +127, against ciphertexts
    all 0xFF and all 0x00: every balanced-digit product at its largest magnitude and the same sign in every column.  Exact: Python integers
    and the oracle."""
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=64, m=16)
    c = gpu_ctx_factory(p)
    count, M, nb = 300, _mod(p), 8 * p.K
    rng = np.random.default_rng(logq + 1)
    cts = np.zeros((count, p.n + 1, p.L), np.uint64)
    cts[0::2, :p.n] = 0xFFFFFFFFFFFFFFFF
    cts[:, p.n] = ol.rand_values(rng, count, p.L, 64 * p.L)
    cts[3::4, p.n] = 0xFFFFFFFFFFFFFFFF
    d_ct = c.to_device(cts)
    for digit in (-128, 127):
        S = (digit * _rep(1, nb)) % M
        sk = np.tile(_limbs(S, p), p.n).reshape(p.n, p.L)
        d_sk = c.to_device(sk)
        res = []
        for path in (1, 2):
            c.set_decrypt_path(path)
            try:
                res.append(c.to_host(c.decrypt(d_sk, d_ct, count), np.uint32).copy())
            finally:
                c.set_decrypt_path(0)
        for i in range(count):
            a = ol.limbs_to_int(cts[i, 0])
            dot = (p.n * (a % M) * S) % M
            want = (ol.limbs_to_int(cts[i, p.n]) - dot) % ol.P
            assert int(res[0][i]) == want and int(res[1][i]) == want, f"digit {digit}, ciphertext {i}: VALU {res[0][i]} MM {res[1][i]} want {want}"
        for i in (0, 1, 2, 3, count - 1):
            assert oracle.decrypt(p, sk, cts[i]) == int(res[1][i])


# ------------------------------------------------------------------------------------------------ E. multi-GPU lane conversion
@pytest.mark.parametrize("logq", [736, 1472])
def test_lanes_carry_256_rank_sums(gpu_ctx_factory, logq):
    """k_ct_to_lanes / k_ct_from_lanes at the headroom the lanes are sized for: 256 copies of all-ones values summed lane-wise on the
    device (int64 wraps like ncclUint64: each lane sum is 2^64 - 256, the carry into the next lane 255, the 8-bit maximum), and 255 copies
    plus one random value.  Exactly the 256-rank bound; against Python integers."""
    import torch

    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=logq, d=64, m=16)
    c = gpu_ctx_factory(p)
    M = _mod(p)
    count = 2
    rng = np.random.default_rng(logq + 2)
    full = np.tile(_limbs(-1, p), count * (p.n + 1)).reshape(count, p.n + 1, p.L)
    rnd = ol.rand_values(rng, count * (p.n + 1), p.L, 64 * p.K).reshape(full.shape)
    lf = c.ct_to_lanes(c.to_device(full), count)
    lr = c.ct_to_lanes(c.to_device(rnd), count)
    lanes1 = np.array([((M - 1) >> (56 * k)) & ((1 << 56) - 1) for k in range(p.lanes)], np.uint64)  # the top lane is partial
    assert (c.to_host(lf, np.uint64).reshape(-1, p.lanes) == lanes1[None, :]).all()
    s256 = lf.unsqueeze(0).expand(256, -1).sum(0)
    s255 = lf.unsqueeze(0).expand(255, -1).sum(0) + lr
    for lanes, base in ((s256, [[256 * (M - 1)] * (p.n + 1)] * count),
                        (s255, [[255 * (M - 1) + ol.limbs_to_int(rnd[k, j]) for j in range(p.n + 1)] for k in range(count)])):
        assert lanes.dtype == torch.int64
        got = c.to_host(c.ct_from_lanes(lanes, count), np.uint64).reshape(full.shape)
        for k in range(count):
            for j in range(p.n + 1):
                assert ol.limbs_to_int(got[k, j]) == base[k][j] % M, f"ciphertext {k}, coordinate {j}"
                assert not got[k, j, p.K:].any()


def test_witness_from_lanes_at_256_rank_sums(gpu_ctx_factory):
    """mfh_witness_from_lanes: w = delta t + lanes mod p with every lane 256 (p - 1) (256 ranks' largest shares) and delta = p - 1,
    t all p - 1 and random; against Python integers."""
    import c_lwe_snarks_amd as mf

    p = mf.DEBUG
    c = gpu_ctx_factory(p)
    rng = np.random.default_rng(9)
    ssp = rng.integers(0, ol.P, size=(p.m + 3) * p.d, dtype=np.uint64)
    ssp[: p.d // 2] = PM1
    d_ssp = c.ssp_upload(ssp)
    t = c.to_host(c.witness_poly(d_ssp, bytes((p.m + 7) // 8), 1), np.uint32).astype(np.uint64)  # w of the empty witness = t
    lanes = np.full(p.d, 256 * PM1, np.uint64)
    lanes[1::2] = rng.integers(0, 256 * ol.P, size=p.d // 2, dtype=np.uint64)
    out = c.empty(p.d * 4)
    c._chk(c.lib.mfh_witness_from_lanes(c._h, mf._ptr(d_ssp), mf._ptr(c.to_device(lanes)), PM1, mf._ptr(out)))
    got = c.to_host(out, np.uint32)
    want = [(PM1 * int(t[k]) + int(lanes[k])) % ol.P for k in range(p.d)]
    assert [int(x) for x in got] == want
