"""CPU: the weighted-sum gate (Circuit.wsum), Words.sum and Sha256Compress(adds="sum").

1. by enumeration mod p, for small term sets with repeated wires and mixed shifts: over every operand assignment, both rows are +-1 for exactly one
   assignment of the output wires, the binary expansion of the sum;
2. nbits and its bound, the CircuitError cases, the row order and layout, Compiled.terms / program;
3. evaluate / assign / holds, and the numpy restatement of the program format, on random circuits that mix every gate kind;
4. Words.sum for k = 2 .. 8 against Python integers, on random and extreme words, constants folded; its wire and row counts;
5. Sha256Compress(adds="sum"), both chainings, against hashlib; the pinned counts; every compiled row +-1 on an honest witness and one of a gate's two
   rows not +-1 with a sum bit or a carry bit flipped; the default circuit unchanged."""
import hashlib
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

from circuit_wsum_ref import bitsliced_sum, random_sum_circuit, row_values_int

P = C.P
BIG = SimpleNamespace(d=1 << 16, m=43690)
PM1 = (1, P - 1)

# (operand wire index, shift) lists: repeated wires, mixed shifts, a gap in the shifts, one term, all on one shift
TERM_SETS = {
    "two bits": [(0, 0), (1, 0)],
    "one term, shifted": [(0, 2)],
    "a wire twice": [(0, 0), (0, 0), (1, 1)],
    "mixed shifts": [(0, 0), (1, 0), (2, 1), (3, 1), (0, 2)],
    "gap": [(0, 0), (1, 3), (2, 3)],
    "five on one shift": [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)],
    "a wire at every shift": [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2)],
}


@pytest.mark.parametrize("name", sorted(TERM_SETS))
def test_rows_force_the_binary_expansion(name):
    terms = TERM_SETS[name]
    nops = 1 + max(a for a, _ in terms)
    c = C.Circuit()
    x = c.private(nops)
    out = c.wsum([(x[a], sh) for a, sh in terms])
    cc = c.compile(SimpleNamespace(d=256, m=64))
    nbits = sum(1 << sh for _, sh in terms).bit_length()
    assert len(out) == nbits and cc.nwires == nops + nbits and cc.nrows == cc.nwires + 2
    rp, wire, coef = cc.rows
    two = [list(zip(wire[rp[j]: rp[j + 1]].tolist(), coef[rp[j]: rp[j + 1]].tolist())) for j in (cc.nwires, cc.nwires + 1)]
    for ops in itertools.product((0, 1), repeat=nops):
        total = sum(ops[a] << sh for a, sh in terms)
        good = []
        for outs in itertools.product((0, 1), repeat=nbits):
            val = (1,) + ops + outs  # wire 0, operands 1 .. nops, outputs after them
            if all(sum(k * val[w] for w, k in row) % P in PM1 for row in two):
                good.append(outs)
        assert good == [tuple((total >> i) & 1 for i in range(nbits))], (ops, good)


def test_nbits_bound_and_errors():
    c = C.Circuit()
    x = c.private(4)
    assert len(c.wsum([(x[0], 23)])) == 24
    assert len(c.wsum([(x[0], 0)])) == 1
    assert len(c.wsum([(x[0], 0)] * 255)) == 8 and len(c.wsum([(x[0], 0)] * 256)) == 9
    with pytest.raises(C.CircuitError, match="needs 25 bits"):
        c.wsum([(x[0], 24)])
    with pytest.raises(C.CircuitError, match="needs 25 bits"):
        c.wsum([(x[0], 23), (x[1], 23)])
    with pytest.raises(C.CircuitError, match="no terms"):
        c.wsum([])
    with pytest.raises(C.CircuitError, match="non-negative"):
        c.wsum([(x[0], -1)])
    with pytest.raises(C.CircuitError, match="not a wire"):
        c.wsum([(C.Wire(999), 0)])
    p = c.output(x[1])
    with pytest.raises(C.CircuitError, match="computed public output"):
        c.wsum([(x[0], 0), (p, 1)])
    n = len(c._nodes)
    with pytest.raises(C.CircuitError):
        c.wsum([(x[0], 0), (x[1], 30)])
    assert len(c._nodes) == n  # a refused gate leaves no node behind


def test_layout_rows_program_and_terms():
    c = C.Circuit()
    z = c.public()
    x = c.private(3)
    g0 = c.XOR(x[0], x[1])
    s = c.wsum([(x[2], 2), (x[0], 0), (g0, 1), (x[0], 2), (z, 0)])  # sorted by shift, stably: x0, z | g0 | x2, x0;  Tmax = 2 + 2 + 8 = 12: 4 bits
    g1 = c.AND(s[3], g0)
    t = c.wsum([(s[0], 0), (g1, 0)])
    c.assert_equal(g1, 0)
    cc = c.compile(SimpleNamespace(d=256, m=64))
    assert len(s) == 4 and len(t) == 2 and [cc.wire(w) for w in s] == [6, 7, 8, 9] and cc.wire(g1) == 10 and [cc.wire(w) for w in t] == [11, 12]
    assert cc.program.tolist() == [[0, 2, 3, 0], [8, 0, 5, 4], [9, 1, 0, 0], [9, 2, 0, 0], [9, 3, 0, 0], [1, 9, 5, 0], [8, 5, 2, 2], [9, 1, 0, 0]]
    assert cc.terms.tolist() == [[2, 0], [1, 0], [5, 1], [4, 2], [2, 2], [6, 0], [10, 0]]
    assert np.array_equal(cc.gates, cc.program[:, :3]) and cc.terms.dtype == np.uint32
    # rows: 12 bit rows, XOR, the first sum's two, AND, the second sum's two, the assertion
    assert cc.nwires == 12 and cc.nrows == 12 + 1 + 2 + 1 + 2 + 1
    rp, wire, coef = cc.rows
    row = lambda j: list(zip(wire[rp[j]: rp[j + 1]].tolist(), coef[rp[j]: rp[j + 1]].tolist()))  # noqa: E731
    x2 = [(2, 2), (1, 2), (5, 4), (4, 8), (2, 8), (6, P - 2), (7, P - 4), (8, P - 8), (9, P - 16)]
    assert row(13) == x2 + [(0, P - 1)] and row(14) == x2 + [(0, 1)]
    assert row(15) == [(9, 2), (5, 2), (10, P - 4), (0, P - 1)]
    y2 = [(6, 2), (10, 2), (11, P - 2), (12, P - 4)]
    assert row(16) == y2 + [(0, P - 1)] and row(17) == y2 + [(0, 1)] and row(18) == [(10, P - 1), (0, 1)]
    # a circuit without the gate has no terms, and its arrays are what they were
    c2 = C.Circuit()
    a = c2.private(2)
    c2.XOR(a[0], a[1])
    cc2 = c2.compile(SimpleNamespace(d=256, m=64))
    assert cc2.terms.shape == (0, 2) and cc2.program.tolist() == [[0, 1, 2, 0]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_circuits_evaluate_and_restate(seed):
    rng = np.random.default_rng(seed)
    npub, npriv = 5, 14
    c = random_sum_circuit(rng, npub, npriv, 600, nsums=25, noutputs=6)
    c.assert_equal(C.Wire(npub + 1), 1)  # on inputs: they hold for 1 statement in 4
    c.assert_same(C.Wire(2), C.Wire(npub + 5))
    p = SimpleNamespace(d=1 << 12, m=2000)
    cc = c.compile(p)
    assert (cc.program[:, 0] == C.GATE_WSUM).sum() == 25 and {0, 1, 2, 3, 4, 5, 8, 9} <= set(cc.program[:, 0].tolist())
    heads = cc.program[cc.program[:, 0] == C.GATE_WSUM]
    assert heads[:, 1].tolist() == np.cumsum([0] + heads[:-1, 2].tolist()).tolist() and heads[:, 2].sum() == len(cc.terms)
    for first, n, nbits in heads[:, 1:].tolist():
        sh = cc.terms[first: first + n, 1]
        assert (np.diff(sh.astype(np.int64)) >= 0).all() and nbits == int(sum(1 << int(s) for s in sh)).bit_length()
    nin = cc.lu + npriv
    bits = rng.integers(0, 2, size=(70, nin), dtype=np.uint8)
    wit, holds = bitsliced_sum(cc, bits, p.m)
    seen = set()
    for b in range(70):
        pub, prv = bits[b, :cc.lu].tolist(), bits[b, cc.lu:].tolist()
        row = c.assign(pub, prv, p)
        assert wit[b].tobytes() == row, b
        assert bool(holds[b]) == c.holds(pub, prv), b
        ok = all(v in PM1 for v in row_values_int(cc.rows, row))
        assert ok == c.holds(pub, prv), b  # every row +-1 exactly when the assertions and equalities hold
        seen.add(ok)
    assert seen == {True, False}


def _word(v):
    return [(v >> i) & 1 for i in range(32)]


@pytest.mark.parametrize("k", range(2, 9))
def test_words_sum(k):
    rng = np.random.default_rng(k)
    w = W.Words()
    xs = w.private(k)
    before = len(w.c._nodes)
    out = w.sum(xs)
    wires = len(w.c._nodes) - before
    cc = w.c.compile(BIG)
    assert (wires, cc.nrows - cc.nwires) == {2: (34, 4), 3: (36, 4), 4: (36, 4)}.get(k, (38, 4))  # 4 rows beyond the wires' bit rows
    cases = [[W.MASK] * k, [0] * k, [W.MASK] + [0] * (k - 1), [0x0000FFFF] * k, [0xFFFF0000] * k, [1] * k]
    cases += [[int(v) for v in rng.integers(0, 1 << 32, size=k)] for _ in range(40)]
    for vals in cases:
        val = w.c.evaluate([], [b for v in vals for b in _word(v)])
        got = sum(val[o.node] << i for i, o in enumerate(out))
        assert got == sum(vals) & W.MASK, vals
        row = w.c.assign([], [b for v in vals for b in _word(v)], BIG)
        assert all(v in PM1 for v in row_values_int(cc.rows, row))


def test_words_sum_constants_and_bounds():
    rng = np.random.default_rng(11)
    for consts in ([0xFFFFFFFF], [0x00010001, 0x80000000], [0], [0x428A2F98, 0, 0xFFFF]):
        w = W.Words()
        xs = w.private(2)
        plain = W.Words()
        ys = plain.private(2 + len(consts))
        n_plain = len(plain.c._nodes)
        plain.sum(ys)
        before = len(w.c._nodes)
        out = w.sum(xs[:1] + [w.const(v) for v in consts] + xs[1:])
        nconst = len(w.c._const)
        # constants cost no wire of their own beyond the shared constant wires, and never more output bits than as many variable words
        assert len(w.c._nodes) - before - nconst <= len(plain.c._nodes) - n_plain
        head = next(n for n in w.c._nodes if n[0] == "wsum")
        one = w.c._const.get(1)
        ones_lo = sum(bin(v & 0xFFFF).count("1") for v in consts)
        assert sum(1 for a, _ in head[2] if a == one) == ones_lo and len(head[2]) == 32 + ones_lo  # zero bits left out, one bits on the shared wire
        for _ in range(20):
            vals = [int(v) for v in rng.integers(0, 1 << 32, size=2)]
            val = w.c.evaluate([], [b for v in vals for b in _word(v)])
            assert sum(val[o.node] << i for i, o in enumerate(out)) == (sum(vals) + sum(consts)) & W.MASK
        vals = [W.MASK, W.MASK]
        val = w.c.evaluate([], [b for v in vals for b in _word(v)])
        assert sum(val[o.node] << i for i, o in enumerate(out)) == (sum(vals) + sum(consts)) & W.MASK
    w = W.Words()
    x = w.private()
    assert len(w.sum([x] * 255)) == 32  # 255 words: hi sums to at most 255 * 65535 + 254 < 2^24
    with pytest.raises(C.CircuitError, match="more than 24 bits"):
        w.sum([x] * 256)
    with pytest.raises(C.CircuitError):
        w.sum([])
    only = w.sum([w.const(5), w.const(0xFFFFFFFF)])  # constants alone still go through the gates, on the one wire
    val = w.c.evaluate([], _word(0))
    assert sum(val[o.node] << i for i, o in enumerate(only)) == 4


SHA_COUNTS = {"iv": (28114, 49588, 256), "public": (28370, 49844, 512)}


@pytest.fixture(scope="module", params=["iv", "public"])
def sha(request):
    st = W.Sha256Compress(chaining=request.param, adds="sum")
    return st, st.circuit.compile(BIG)


def _sha_case(st, rng, i):
    msg = b"abc" if i == 0 else bytes(rng.integers(0, 256, size=int(rng.integers(0, 56)), dtype=np.uint8).tolist())
    if st.chaining == "iv":
        return st.bits(W.sha256_pad(msg)), hashlib.sha256(msg).digest()
    # public chaining: the second block of a two-block message, chained from the first block's value computed by the default circuit's reference
    long = msg + bytes(rng.integers(0, 256, size=64, dtype=np.uint8).tolist())
    padded = W.sha256_pad(long)
    assert len(padded) == 128
    mid = _compress_int(W.SHA256_IV, padded[:64])
    return st.bits(padded[64:], b"".join(v.to_bytes(4, "big") for v in mid)), hashlib.sha256(long).digest()


def _compress_int(H, block):
    """FIPS 180-4 6.2.2 on Python integers"""
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & W.MASK  # noqa: E731
    w = W.be_words(block)
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & W.MASK)
    a, b, c, d, e, f, g, h = H
    for t in range(64):
        t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + W.SHA256_K[t] + w[t]
        t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))
        a, b, c, d, e, f, g, h = (t1 + t2) & W.MASK, a, b, c, (d + t1) & W.MASK, e, f, g
    return [(x + y) & W.MASK for x, y in zip(H, (a, b, c, d, e, f, g, h))]


def test_sha256_sum_counts_and_fit(sha):
    st, cc = sha
    nw, nrows, lu = SHA_COUNTS[st.chaining]
    assert (cc.nwires, cc.nrows, cc.lu) == (nw, nrows, lu) and len(cc.outputs) == 256
    assert cc.nwires <= 32767 and cc.nrows <= (1 << 16) - 1 and cc.nwires <= BIG.m - 1  # MFH_CIRCUIT_MAX_WIRES, d - 1, m - 1
    heads = cc.program[cc.program[:, 0] == C.GATE_WSUM]
    assert len(heads) == 2 * 184 and int(heads[:, 3].max()) == 19 and len(cc.terms) == int(heads[:, 2].sum())
    with pytest.raises(C.CircuitError, match="rows"):
        st.circuit.compile(SimpleNamespace(d=1 << 15, m=43690))
    with pytest.raises(C.CircuitError, match="adds"):
        W.Sha256Compress(adds="carry-save")


def test_sha256_sum_against_hashlib_and_rows(sha):
    st, cc = sha
    c = st.circuit
    rng = np.random.default_rng(len(st.chaining))
    lu = cc.lu
    for i in range(4):
        bits, digest = _sha_case(st, rng, i)
        if i & 1:
            bits[st.digest_at: st.digest_at + 256] = rng.integers(0, 2, size=256, dtype=np.uint8)  # garbage where the result is computed
        assert c.holds(bits[:lu], bits[lu:])
        row = c.assign(bits[:lu], bits[lu:], BIG)
        assert st.digest_of(row) == digest, i
        if i < 2:
            assert all(v in PM1 for v in row_values_int(cc.rows, row))
    # one sum bit, one carry bit (a lo gate's bit 16 and up) and one discarded bit (a hi gate's) flipped: one of that gate's two rows is not +-1
    heads = np.flatnonzero(cc.program[:, 0] == C.GATE_WSUM)
    nin = cc.nwires - len(cc.program)
    rp = cc.rows[0]
    # the gate rows follow the nwires bit rows in gate order: a head's rows are at nwires + (non-WSUM_BIT records before it) + (heads before it)
    plain_before = np.cumsum(cc.program[:, 0] != C.GATE_WSUM_BIT) - 1
    for k, bit in ((0, 3), (0, 16), (101, 17), (len(heads) - 2, 16), (len(heads) - 1, 16), (200, 0)):
        g = int(heads[k])
        assert bit < cc.program[g, 3]
        wire = nin + 1 + g + bit
        bad = bytearray(row)
        bad[(wire - 1) >> 3] ^= 1 << ((wire - 1) & 7)
        vals = row_values_int(cc.rows, bytes(bad))
        j = cc.nwires + int(plain_before[g]) + k
        assert rp[j + 1] - rp[j] == cc.program[g, 2] + cc.program[g, 3] + 1  # the head's first row: terms, outputs, the constant
        assert not (vals[j] in PM1 and vals[j + 1] in PM1), (k, bit)
        assert vals[wire - 1] in PM1  # the flipped wire is still a bit


def test_default_sha256_is_unchanged():
    big = SimpleNamespace(d=1 << 17, m=87381)
    a = W.Sha256Compress().circuit.compile(big)
    b = W.Sha256Compress(adds="ripple").circuit.compile(big)
    assert (a.nwires, a.nrows) == (61698, 122884) and a.terms.shape == (0, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a.rows, b.rows)) and np.array_equal(a.program, b.program)
    assert not ((a.program[:, 0] == C.GATE_WSUM) | (a.program[:, 0] == C.GATE_WSUM_BIT)).any()
