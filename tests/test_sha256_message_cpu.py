"""CPU: the whole-message SHA-256 statement (words.Sha256Message), the Merkle path statement (words.MerklePath) and Compiled.row_source.

1. tests/sha256_ref.py (a compression function written from FIPS 180-4, the Merkle reference) against hashlib on padded one- and two-block messages;
2. Sha256Message for 0, 3 ("abc"), 55, 56, 64 and 119 bytes: digest_of(assign(...)) = hashlib, wires and rows as documented, 55 bytes compile at
   d = 2^16 and 56 do not, a negative length is refused; the arrays Sha256Compress compiles to are what they were before the new classes existed;
3. MerklePath of depth 1, 2, 3: the root equals the reference for every index at depth 1 and 2 and for three indices at depth 3, the sizes follow
   28 625 depth + 514 wires and 50 865 depth + 772 rows;
4. row_source on a small circuit with every kind of row (a WSUM among them, an assertion, an equality, an output): every row index maps back to the
   object whose row compile emitted there, checked by rebuilding that row's entries from the object."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P16 = mf.Params(d=1 << 16, m=43690)
P17 = mf.Params(d=1 << 17, m=87381)
P18 = mf.Params(d=1 << 18, m=174762)
ABC_DIGEST = "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"  # FIPS 180-4 / NIST example, SHA-256("abc")


def _message(n):
    return b"abc" if n == 3 else bytes(np.random.default_rng(1000 + n).integers(0, 256, size=n, dtype=np.uint8).tolist())


# ------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("n", [0, 3, 55, 56, 64, 119])
def test_reference_compression_equals_hashlib(n):
    m = _message(n)
    padded = ref.pad(m)
    assert len(padded) == (64 if n < 56 else 128) and padded == W.sha256_pad(m)
    assert ref.digest_of_padded(padded) == hashlib.sha256(m).digest()
    assert ref.IV == W.SHA256_IV and ref.K == W.SHA256_K


def test_reference_abc():
    assert ref.digest_of_padded(ref.pad(b"abc")).hex() == ABC_DIGEST


# ------------------------------------------------------------------ 2. Sha256Message
SIZES = {0: (27588, 49062), 55: (28042, 49516), 56: (55382, 98072), 100: (55746, 98436), 119: (55898, 98588), 120: (83238, 147144)}


@pytest.mark.parametrize("n", [0, 3, 55, 56, 64, 119])
def test_message_digest_equals_hashlib(n):
    st = W.Sha256Message(n)
    p = P16 if n < 56 else P17
    cc = st.circuit.compile(p)
    assert st.lu == cc.lu == 256 and len(cc.outputs) == 256 and len(cc.equal) == 256 and len(cc.asserts) == 0
    assert st.blocks == (1 if n < 56 else 2)
    assert cc.nwires - len(cc.program) == 256 + 8 * n  # the padding is no input
    m = _message(n)
    bits = st.bits(m)
    assert bits.shape == (256 + 8 * n,) and not bits[:256].any()
    assert np.array_equal(bits[256:], np.unpackbits(np.frombuffer(m, dtype=np.uint8), bitorder="little"))
    row = st.circuit.assign(bits[:256], bits[256:], p)
    assert st.digest_of(row) == hashlib.sha256(m).digest()
    if n == 3:
        assert st.digest_of(row).hex() == ABC_DIGEST
    assert st.circuit.holds(bits[:256], bits[256:])
    # garbage where the digest is computed changes nothing
    junk = bits.copy()
    junk[:256] = 1
    assert st.circuit.assign(junk[:256], junk[256:], p) == row
    # another message of the same length: another digest; a message of another length is refused
    if n:
        other = bytes([m[0] ^ 1]) + m[1:]
        ob = st.bits(other)
        assert st.digest_of(st.circuit.assign(ob[:256], ob[256:], p)) == hashlib.sha256(other).digest() != hashlib.sha256(m).digest()
    with pytest.raises(C.CircuitError):
        st.bits(m + b"x")


@pytest.mark.parametrize("n", sorted(SIZES))
def test_message_sizes(n):
    cc = W.Sha256Message(n).circuit.compile(P18)
    assert (cc.nwires, cc.nrows) == SIZES[n] == W.SHA256_MESSAGE_SIZES[n]


def test_message_size_limits():
    W.Sha256Message(55).circuit.compile(P16)
    with pytest.raises(C.CircuitError):
        W.Sha256Message(56).circuit.compile(P16)
    W.Sha256Message(119).circuit.compile(P17)
    with pytest.raises(C.CircuitError):
        W.Sha256Message(120).circuit.compile(P17)
    with pytest.raises(C.CircuitError):
        W.Sha256Message(-1)


def _arrays_digest(cc):
    h = hashlib.sha256()
    for a in (*cc.rows, cc.program, cc.equal, cc.outputs, cc.terms, cc.asserts):
        h.update(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
    return h.hexdigest()


# the arrays of Sha256Compress as the commit before Sha256Message / MerklePath compiled them
COMPRESS_DIGESTS = {
    ("iv", "sum", 16): "6a7b4033c7baded07701617f4655939b251d63a2ec2bc16b4378cbb6a1042b07",
    ("public", "sum", 16): "d7820ab9c60981c822fc20d1d4b8db602140688bdb259d28c3798ee63673fbd6",
    ("iv", "ripple", 17): "dc31b63fa2aa9886dfdbd70ce797c2ca0d9bbd5d31bd537a4e1a65790d9a0188",
}


@pytest.mark.parametrize("chaining,adds,logd", sorted(COMPRESS_DIGESTS))
def test_compress_arrays_unchanged(chaining, adds, logd):
    p = P16 if logd == 16 else P17
    before = _arrays_digest(W.Sha256Compress(chaining, adds=adds).circuit.compile(p))
    # building the new statements in between leaves no trace in the next circuit (no shared state in words.py)
    W.Sha256Message(3).circuit.compile(p)
    W.MerklePath(1).circuit.compile(P17)
    after = _arrays_digest(W.Sha256Compress(chaining, adds=adds).circuit.compile(p))
    assert before == after == COMPRESS_DIGESTS[(chaining, adds, logd)]


# ------------------------------------------------------------------ 3. MerklePath
@pytest.fixture(scope="module")
def paths():
    out = {}
    for depth in (1, 2, 3):
        st = W.MerklePath(depth)
        out[depth] = (st, st.circuit.compile(P18))
    return out


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_merkle_sizes(paths, depth):
    st, cc = paths[depth]
    assert (cc.nwires, cc.nrows) == (28625 * depth + 514, 50865 * depth + 772) == W.MERKLE_PATH_SIZES[depth]
    assert W.MERKLE_PATH_SIZES[20] == (28625 * 20 + 514, 50865 * 20 + 772)
    assert W.MERKLE_PATH_SIZES[20][0] <= 699050 - 1 and W.MERKLE_PATH_SIZES[20][1] <= (1 << 20) - 1
    assert st.lu == cc.lu == 256 and len(cc.outputs) == 256
    assert cc.nwires - len(cc.program) == 256 + 256 * (depth + 1) + depth


@pytest.mark.parametrize("depth,indices", [(1, [0, 1]), (2, [0, 1, 2, 3]), (3, [0, 5, 7])])
def test_merkle_root_equals_reference(paths, depth, indices):
    st, cc = paths[depth]
    rng = np.random.default_rng(40 + depth)
    leaf = rng.bytes(32)
    sibs = [rng.bytes(32) for _ in range(depth)]
    roots = set()
    for index in indices:
        bits = st.bits(leaf, sibs, index)
        assert bits.shape == (256 + 256 * (depth + 1) + depth,)
        row = st.circuit.assign(bits[:256], bits[256:], P18)
        want = ref.merkle_root(leaf, sibs, index)
        assert st.root_of(row) == want, index
        roots.add(want)
    assert len(roots) == len(indices)  # the direction bits matter
    # the node function is ONE compression of left || right, not SHA-256 of the 64 bytes
    assert ref.merkle_parent(leaf, sibs[0]) != hashlib.sha256(leaf + sibs[0]).digest()
    with pytest.raises(C.CircuitError):
        st.bits(leaf, sibs, 1 << depth)
    with pytest.raises(C.CircuitError):
        st.bits(leaf, sibs[:-1], 0)


def test_merkle_depth_zero_refused():
    with pytest.raises(C.CircuitError):
        W.MerklePath(0)


# ------------------------------------------------------------------ 4. row_source
def _gate_rows(cc, g):
    """the rows compile emits for program[g], rebuilt from the record: a list of rows of (wire, coef mod p)"""
    nin = cc.nwires - len(cc.program)
    op, a, b, c = (int(x) for x in cc.program[g])
    o, p, m1 = nin + 1 + g, C.P, C.P - 1
    if op == C.GATE_XOR:
        return [[(a, 1), (b, 1), (o, 1), (0, m1)]]
    if op == C.GATE_AND:
        return [[(a, 2), (b, 2), (o, p - 4), (0, m1)]]
    if op == C.GATE_OR:
        return [[(a, p - 2), (b, p - 2), (o, 4), (0, m1)]]
    if op == C.GATE_NOT:
        return [[(a, 1), (o, 1)]]
    if op == C.GATE_MAJ:
        return [[(a, 2), (b, 2), (c, 2), (o, p - 4), (0, m1)]]
    if op == C.GATE_SUM3:
        return [[(a, m1), (b, m1), (c, m1), (o - 1, 2), (o, m1), (0, 1)]]
    if op == C.GATE_CONST0:
        return [[(o, m1), (0, 1)]]
    if op == C.GATE_CONST1:
        return [[(o, 1)]]
    if op == C.GATE_WSUM:
        x2 = [(int(w), (2 << int(sh)) % p) for w, sh in cc.terms[a: a + b]] + [(o + k, p - (2 << k)) for k in range(c)]
        return [x2 + [(0, m1)], x2 + [(0, 1)]]
    if op == C.GATE_WSUM_BIT:
        return []
    terms, const = C.lut2_row(op - 16, a, b, o)
    return [[(w, x % p) for w, x in terms] + ([(0, const % p)] if const % p else [])]


def test_row_source_names_every_row():
    c = C.Circuit()
    pub = c.public(2)
    x = c.private(6)
    g1 = c.XOR(x[0], x[1])
    g2 = c.AND(g1, pub[0])
    s, k = c.full_add(x[2], x[3], g2)
    sums = c.wsum([(x[0], 0), (x[1], 0), (s, 1), (k, 3), (x[4], 3)])
    n1 = c.NOT(sums[2])
    o1 = c.OR(n1, c.const(1))
    l1 = c.ANDN(o1, x[5])
    sums2 = c.wsum([(l1, 0), (sums[0], 0)])
    z = c.const(0)
    c.assert_equal(o1, 1)
    c.assert_equal(z, 0)
    c.assert_same(sums2[1], pub[1])
    c.output(sums[4])
    cc = c.compile(mf.DEBUG)
    assert {C.GATE_XOR, C.GATE_AND, C.GATE_OR, C.GATE_NOT, C.GATE_MAJ, C.GATE_SUM3, C.GATE_CONST0, C.GATE_CONST1, C.GATE_WSUM, C.GATE_WSUM_BIT,
            C.GATE_LUT2(C.TT_ANDN)} == set(cc.program[:, 0].tolist())
    rp, wire, coef = cc.rows
    seen = {"bit": 0, "gate": 0, "assert": 0, "equal": 0}
    per_gate = {}
    for j in range(cc.nrows):
        kind, idx = cc.row_source(j)
        got = list(zip(wire[rp[j]: rp[j + 1]].tolist(), coef[rp[j]: rp[j + 1]].tolist()))
        if kind == "bit":
            assert idx == j + 1 and got == [(idx, 2), (0, C.P - 1)]
        elif kind == "gate":
            nth = per_gate.get(idx, 0)  # a WSUM head has two rows, in this order
            per_gate[idx] = nth + 1
            assert got == _gate_rows(cc, idx)[nth], (j, idx)
        elif kind == "assert":
            w, v = (int(t) for t in cc.asserts[idx])
            assert got == ([(w, 1)] if v else [(w, C.P - 1), (0, 1)])
        else:
            assert kind == "equal"
            a, b = (int(t) for t in cc.equal[idx])
            assert got == [(a, C.P - 1), (b, C.P - 1), (0, 1)]
        seen[kind] += 1
    assert seen == {"bit": cc.nwires, "gate": cc.nrows - cc.nwires - 4, "assert": 2, "equal": 2}
    # every record got exactly the rows it is owed: two per head, none per WSUM_BIT, one otherwise
    for g, op in enumerate(cc.program[:, 0].tolist()):
        assert per_gate.get(g, 0) == (2 if op == C.GATE_WSUM else 0 if op == C.GATE_WSUM_BIT else 1), g
    for j in (-1, cc.nrows):
        with pytest.raises(C.CircuitError):
            cc.row_source(j)


def test_rows_reference_agrees_with_holds():
    """the numpy reference of the row check (tests/rows_check_ref.py, the GPU tests' reference): a witness of assign violates no row exactly when the
    circuit holds, and then the first violated row is an assertion's or an equality's; a flipped gate wire violates that gate's row"""
    import rows_check_ref as rr

    c = C.Circuit()
    pub = c.public(2)
    x = c.private(4)
    g = c.XOR(x[0], x[1])
    s = c.wsum([(x[0], 0), (x[1], 0), (x[2], 1), (g, 1)])
    c.assert_equal(c.AND(g, x[3]), 1)
    c.assert_same(s[1], pub[0])
    cc = c.compile(mf.DEBUG)
    some_fail = some_hold = False
    for v in range(64):
        bits = [(v >> i) & 1 for i in range(6)]
        row = c.assign(bits[:2], bits[2:])
        count, first = rr.violations(cc.rows, [row])
        holds = c.holds(bits[:2], bits[2:])
        assert (count[0] == 0) == holds, v
        if holds:
            some_hold = True
            assert first[0] == rr.NONE
            flipped = bytearray(row)
            flipped[(cc.wire(g) - 1) >> 3] ^= 1 << ((cc.wire(g) - 1) & 7)
            count2, first2 = rr.violations(cc.rows, [bytes(flipped)])
            assert count2[0] >= 1 and cc.row_source(int(first2[0])) == ("gate", cc.wire(g) - 6 - 1)
        else:
            some_fail = True
            assert cc.row_source(int(first[0]))[0] in ("assert", "equal")
    assert some_fail and some_hold
