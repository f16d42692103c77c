"""GPU: the device row check (mfh_ssp_rows_violations, k_rows_violations) against the numpy reference tests/rows_check_ref.py.

1. random row systems at d = 1152, m = 1000: rows of 0 .. 6 entries and one of 200, repeated wires within a row, wire-0 entries, wire m - 1 (the last bit
   of a statement's row); nrows in {0, 1, 64, 257, 1151}, 1 and 33 statements: count and first equal the reference exactly, one launch is timed;
2. crafted positions: a system every row of which holds on a witness (XOR gate rows and bit rows), one witness bit flipped so that exactly one known row
   fails -- rows 0, 63, 64, 255, 256 and nrows - 1, the wave and workgroup seams and both ends -- then two rows, first the lower one;
   and 770 statements at m = 699 050, where a chunk of staged bits holds 767: the second chunk's statements against the reference;
3. every MFH_EINVAL case with its own text and nothing written; nstmt = 0 does nothing;
4. mfh_scrub_staging after the call: returns 0, and the same call afterwards stages again and returns the same;
5. agreement with h_holds of mfh_circuit_assign: 64 statements, half of them failing an assertion or an equality: count == 0 exactly where holds, and the
   first violated row of a failing statement is an "assert" or "equal" row (Compiled.row_source)."""
import ctypes

import numpy as np
import pytest

import rows_check_ref as rr

pytestmark = pytest.mark.gpu

EINVAL = -1
P = rr.P


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def C():
    from c_lwe_snarks_amd import circuit

    return circuit


@pytest.fixture(scope="module")
def params(mf):
    return mf.Params(d=1152, m=1000)


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory, params):
    return gpu_ctx_factory(params)


def _witnesses(rng, p, nb):
    """nb random witness rows of (m + 7) // 8 bytes; the bits past wire m - 1 are set too (the check must not read them as wires)"""
    return [rng.bytes((p.m + 7) // 8) for _ in range(nb)]


# ------------------------------------------------------------------ 1. random systems
def _random_system(rng, p, nrows, w0):
    """rows of 0 .. 6 entries, row nrows // 2 of 200; about half of the non-empty rows are completed by a wire-0 entry so that they hold on witness w0"""
    bits0 = np.unpackbits(np.frombuffer(w0, dtype=np.uint8), bitorder="little")
    rows = []
    for j in range(nrows):
        k = 200 if (j == nrows // 2 and nrows > 1) else int(rng.integers(0, 7))
        r = [(int(rng.integers(0, p.m)), int(rng.integers(0, P))) for _ in range(k)]
        if k >= 2 and j % 3 == 0:
            r[1] = (r[0][0], r[1][1])  # a repeated wire: its entries add
        if k >= 1 and j % 5 == 0:
            r[-1] = (p.m - 1, r[-1][1])  # the last wire: bit m - 2, the last of the statement's row
        if k >= 1 and j % 7 == 0:
            r[0] = (0, r[0][1])  # a wire-0 entry among the others
        if k and j % 2 == 0:  # complete the row to +1 or -1 on w0
            e = sum(c for w, c in r if w == 0 or bits0[w - 1]) % P
            r.append((0, ((1 if j % 4 == 0 else P - 1) - e) % P))
        rows.append(r)
    return rows


@pytest.mark.parametrize("nb", [1, 33])
@pytest.mark.parametrize("nrows", [0, 1, 64, 257, 1151])
def test_random_systems_equal_reference(ctx, params, nrows, nb):
    rng = np.random.default_rng(7000 + 40 * nrows + nb)
    ws = _witnesses(rng, params, nb)
    rows = rr.csr(_random_system(rng, params, nrows, ws[0]))
    ctx.ssp_set_rows(rows, lu_max=0)
    ctx.set_timing(True)
    count, first = ctx.ssp_rows_violations(ws)
    n, ms, total = ctx.timing_drain("ssp_rows_violations")
    ctx.set_timing(False)
    want_count, want_first = rr.violations(rows, ws)
    print(f"nrows {nrows}, {nb} statements: count {count.tolist()[:4]}.. first {first.tolist()[:4]}.. kernel {ms:.3f} ms")
    assert count.dtype == np.uint32 and first.dtype == np.uint32
    assert np.array_equal(count, want_count) and np.array_equal(first, want_first)
    assert (n, total) == ((1, nrows * nb) if nrows else (0, 0))
    if nrows >= 64:  # the case is not vacuous: statement 0 holds on about half of its rows, and violates others
        assert 0 < int(count[0]) < nrows


def test_two_chunks_of_statements(gpu_ctx_factory, mf):
    """the bits are staged in chunks of statements of at most 64 MiB: at m = 699 050 a statement is 87 382 bytes and a chunk holds 767, so statements
    767 .. 769 of 770 go through a second chunk (its own staging, counters and launch); d is small, the chunk depends on m alone"""
    p = mf.Params(d=1152, m=699050)
    bs = (p.m + 6) // 8
    assert (64 << 20) // bs == 767
    ctx = gpu_ctx_factory(p)
    rng = np.random.default_rng(61)
    nb = 770
    raw = rng.integers(0, 256, size=(nb, bs), dtype=np.uint8)
    rows = rr.csr(_random_system(rng, p, 300, raw[769].tobytes()))  # about half of the rows hold on the last statement
    ctx.ssp_set_rows(rows, lu_max=0)
    ctx.set_timing(True)
    count, first = ctx.ssp_rows_violations(raw)
    n, _, total = ctx.timing_drain("ssp_rows_violations")
    ctx.set_timing(False)
    assert (n, total) == (2, 300 * nb)
    want = rr.violations(rows, [raw[b].tobytes() for b in range(nb)])
    print("two chunks: count", count[765:].tolist(), "first", first[765:].tolist())
    assert np.array_equal(count, want[0]) and np.array_equal(first, want[1])
    assert 0 < int(count[769]) < 300 and int(count[768]) > int(count[769])
    ctx.ssp_set_rows(None)


# ------------------------------------------------------------------ 2. crafted positions
NIN, NG, HEAD = 40, 300, 257  # gate rows 0 .. 256, then the 340 bit rows, then gate rows 257 .. 299: 640 rows


def _xor_system(rng):
    """(rows, witness, row index of each gate): gate g writes wire NIN + 1 + g = XOR of two INPUT wires, so flipping its output violates its row alone"""
    ops = [(int(rng.integers(1, NIN + 1)), int(rng.integers(1, NIN + 1))) for _ in range(NG)]
    gate = [[(a, 1), (b, 1), (NIN + 1 + g, 1), (0, P - 1)] for g, (a, b) in enumerate(ops)]
    bit = [[(w, 2), (0, P - 1)] for w in range(1, NIN + NG + 1)]
    rows = gate[:HEAD] + bit + gate[HEAD:]
    row_of = list(range(HEAD)) + [HEAD + len(bit) + k for k in range(NG - HEAD)]
    val = np.zeros(NIN + NG, dtype=np.uint8)
    val[:NIN] = rng.integers(0, 2, size=NIN, dtype=np.uint8)
    for g, (a, b) in enumerate(ops):
        val[NIN + g] = val[a - 1] ^ val[b - 1]
    return rows, val, row_of


def test_crafted_single_rows(ctx, params):
    rng = np.random.default_rng(31)
    rows, val, row_of = _xor_system(rng)
    nrows = len(rows)
    assert nrows == 640 and row_of[-1] == nrows - 1
    targets = [0, 63, 64, 255, 256, nrows - 1]
    gate_at = {r: g for g, r in enumerate(row_of)}
    stride = (params.m + 7) // 8

    def witness(flipped_rows):
        v = val.copy()
        for r in flipped_rows:
            v[NIN + gate_at[r]] ^= 1
        return np.packbits(v, bitorder="little").tobytes().ljust(stride, b"\0")

    ws = [witness([])] + [witness([r]) for r in targets] + [witness([255, 64]), witness([nrows - 1, 0, 256])]
    csr = rr.csr(rows)
    ctx.ssp_set_rows(csr, lu_max=0)
    count, first = ctx.ssp_rows_violations(ws)
    print("crafted: count", count.tolist(), "first", first.tolist())
    assert count.tolist() == [0] + [1] * len(targets) + [2, 3]
    assert first.tolist() == [rr.NONE] + targets + [64, 0]
    want = rr.violations(csr, ws)
    assert np.array_equal(count, want[0]) and np.array_equal(first, want[1])


# ------------------------------------------------------------------ 3. MFH_EINVAL
def test_einval_cases_write_nothing(ctx, params, mf):
    lib, h = ctx.lib, ctx._h
    bs = (params.m + 6) // 8
    bits = bytes(2 * bs)
    count = np.full(2, 0xABCD, dtype=np.uint32)
    first = np.full(2, 0xABCD, dtype=np.uint32)
    pc, pf = ctypes.c_void_p(count.ctypes.data), ctypes.c_void_p(first.ctypes.data)

    def err():
        return lib.mfh_last_error(h).decode()

    ctx.ssp_set_rows(None)
    assert lib.mfh_ssp_rows_violations(h, 2, bits, bs, pc, pf) == EINVAL and "no row SSP registered" in err()
    with pytest.raises(mf.MfhError, match="no row SSP registered"):
        ctx.ssp_rows_violations([bits[:bs]])
    ctx.ssp_set_rows(rr.csr([[(0, 1)], [(1, 1)]]), lu_max=0)
    assert lib.mfh_ssp_rows_violations(h, 2, bits, bs - 1, pc, pf) == EINVAL and "bits_stride" in err()
    assert lib.mfh_ssp_rows_violations(h, 2, None, bs, pc, pf) == EINVAL and "h_bits / h_count" in err()
    assert lib.mfh_ssp_rows_violations(h, 2, bits, bs, None, pf) == EINVAL and "h_bits / h_count" in err()
    assert count.tolist() == [0xABCD] * 2 and first.tolist() == [0xABCD] * 2
    # nstmt = 0 does nothing, whatever the pointers
    assert lib.mfh_ssp_rows_violations(h, 0, None, bs, None, None) == 0
    assert lib.mfh_ssp_rows_violations(h, 0, bits, bs, pc, pf) == 0
    assert count.tolist() == [0xABCD] * 2 and first.tolist() == [0xABCD] * 2
    c0, f0 = ctx.ssp_rows_violations([])
    assert c0.shape == (0,) and f0.shape == (0,)
    # h_first may be NULL; a larger stride is the caller's layout
    wide = bytes(bs + 3) + b"\x01" + bytes(bs + 2)
    assert lib.mfh_ssp_rows_violations(h, 2, wide, bs + 3, pc, None) == 0
    assert count.tolist() == [1, 0] and first.tolist() == [0xABCD] * 2  # row 1 = wire 1: 0 on statement 0, 1 on statement 1
    assert lib.mfh_ssp_rows_violations(h, 2, wide, bs + 3, pc, pf) == 0
    assert first.tolist() == [1, rr.NONE]
    ctx.ssp_set_rows(None)


# ------------------------------------------------------------------ 4. scrub
def test_scrub_after_the_call(ctx, params):
    rng = np.random.default_rng(41)
    ws = _witnesses(rng, params, 5)
    rows = rr.csr(_random_system(rng, params, 300, ws[0]))
    ctx.ssp_set_rows(rows, lu_max=0)
    before = ctx.ssp_rows_violations(ws)
    assert ctx.scrub_staging() == 0
    assert ctx.scrub_staging() == 0  # nothing left in use: a second scrub has nothing to zero
    after = ctx.ssp_rows_violations(ws)  # stages again into the zeroed buffer
    assert ctx.scrub_staging() == 0
    want = rr.violations(rows, ws)
    for got in (before, after):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------ 5. h_holds
def test_agrees_with_holds_of_circuit_assign(ctx, params, C):
    c = C.Circuit()
    pub = c.public(2)
    x = c.private(10)
    acc = x[0]
    for k in range(1, 8):
        acc = c.XOR(acc, c.AND(x[k], x[k - 1]))
    s = c.wsum([(x[k], k % 3) for k in range(8)])
    c.assert_equal(c.XOR(x[8], acc), 1)      # x8 = NOT acc
    c.assert_same(c.OR(x[9], s[0]), pub[0])  # pub0 = x9 | s0
    c.assert_same(s[2], pub[1])
    cc = c.compile(params)
    nb = 64
    rng = np.random.default_rng(51)
    bits = np.zeros((nb, 12), dtype=np.uint8)
    for b in range(nb):
        xs = rng.integers(0, 2, size=10, dtype=np.uint8)
        val = c.evaluate([0, 0], xs.tolist())
        xs[8] = 1 - val[acc.node]
        val = c.evaluate([0, 0], xs.tolist())
        pubs = [val[x[9].node] | val[s[0].node], val[s[2].node]]
        if b % 2:  # fail: the assertion, one equality or the other
            if b % 6 == 1:
                xs[8] ^= 1
            else:
                pubs[(b // 2) % 2] ^= 1
        bits[b] = pubs + xs.tolist()
    prog = ctx.circuit_load(cc)
    witness, holds = ctx.circuit_assign(prog, bits)
    prog.close()
    assert holds.tolist() == [b % 2 == 0 for b in range(nb)]
    ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)
    count, first = ctx.ssp_rows_violations(witness)
    want = rr.violations(cc.rows, [witness[b].tobytes() for b in range(nb)])
    assert np.array_equal(count, want[0]) and np.array_equal(first, want[1])
    assert ((count == 0) == holds).all()
    kinds = set()
    for b in range(nb):
        if not holds[b]:
            src = cc.row_source(int(first[b]))
            assert src[0] in ("assert", "equal"), (b, src)
            kinds.add(src)
        else:
            assert first[b] == rr.NONE
    assert kinds == {("assert", 0), ("equal", 0), ("equal", 1)}
