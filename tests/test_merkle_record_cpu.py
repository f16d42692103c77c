"""CPU: the record-membership statement words.MerkleRecord(length, depth) and Sha256Message.statement.

1. sizes: (0, 1), (55, 1), (56, 1) and (3, 2) are compiled and equal MERKLE_RECORD_SIZES and the formula "Sha256Message(length) plus 28 625 depth wires
   and 50 865 depth rows"; the rest of the table is checked by the formula (the sizes of Sha256Message: SHA256_MESSAGE_SIZES, and the compiled
   Sha256Message(3)); the capacity at d = 2^20, m = 699 050: (55, 19) and (119, 18) fit, (55, 20) does not.
2. roots: root_of(assign(...)) equals tests/sha256_ref.py's merkle_parent chain over the hashlib leaf at (3, 2, 2), (0, 1, 1), (56, 1, 0), and for every
   index at (3, 2); a record with one bit flipped gives another root; a wrong-length record, a wrong sibling count and an index out of range are refused.
3. statements: statement(root) equals the statement bytes of the assigned row (the inverse of root_of) and MerklePath.statement(root);
   Sha256Message.statement(hashlib digest) equals bits [0, 256) of the assigned row for lengths 0, 3 and 56."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P17 = mf.Params(d=1 << 17, m=87381)
P18 = mf.Params(d=1 << 18, m=174762)
P20 = mf.Params(d=1 << 20, m=699050)

# the issue's table: (length, depth) -> (wires, rows)
TABLE = {(0, 1): (56213, 99927), (55, 1): (56667, 100381), (56, 1): (84007, 148937), (119, 1): (84523, 149453), (120, 1): (111863, 198009),
         (3, 2): (84865, 150819), (55, 2): (85292, 151246), (56, 2): (112632, 199802)}
COMPILED = [(0, 1), (55, 1), (56, 1), (3, 2)]


def _record(n, salt=0):
    return bytes(np.random.default_rng(7000 + 16 * n + salt).integers(0, 256, size=n, dtype=np.uint8).tolist())


@pytest.fixture(scope="module")
def statements():
    out = {}
    for key in COMPILED:
        st = W.MerkleRecord(*key)
        out[key] = (st, st.circuit.compile(P18))
    return out


@pytest.fixture(scope="module")
def message3():
    """(wires, rows) of Sha256Message(3), which SHA256_MESSAGE_SIZES does not list"""
    cc = W.Sha256Message(3).circuit.compile(P17)
    return cc.nwires, cc.nrows


def _formula(message_size, depth):
    return message_size[0] + 28625 * depth, message_size[1] + 50865 * depth


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("key", COMPILED)
def test_compiled_sizes(statements, message3, key):
    st, cc = statements[key]
    length, depth = key
    assert (cc.nwires, cc.nrows) == TABLE[key] == W.MERKLE_RECORD_SIZES[key]
    assert TABLE[key] == _formula(message3 if length == 3 else W.SHA256_MESSAGE_SIZES[length], depth)
    assert st.lu == cc.lu == 256 and len(cc.outputs) == 256 and len(cc.equal) == 256 and len(cc.asserts) == 0
    assert cc.nwires - len(cc.program) == 256 + 8 * length + 257 * depth  # the padding and the leaf are no inputs
    assert st.blocks == (1 if length < 56 else 2)


def test_table_by_formula():
    for (length, depth), size in TABLE.items():
        assert W.MERKLE_RECORD_SIZES[(length, depth)] == size
        if length in W.SHA256_MESSAGE_SIZES:
            assert size == _formula(W.SHA256_MESSAGE_SIZES[length], depth), (length, depth)


def test_capacity_at_two_to_the_twenty():
    fits = lambda size: size[0] <= P20.m - 1 and size[1] <= P20.d - 1  # noqa: E731  (Circuit.compile's two limits)
    a = _formula(W.SHA256_MESSAGE_SIZES[55], 19)
    b = _formula(W.SHA256_MESSAGE_SIZES[119], 18)
    c = _formula(W.SHA256_MESSAGE_SIZES[55], 20)
    assert a == (571917, 1015951) == W.MERKLE_RECORD_SIZES[(55, 19)] and fits(a)
    assert b == (571148, 1014158) == W.MERKLE_RECORD_SIZES[(119, 18)] and fits(b)
    assert c[1] == 1066816 and not fits(c)
    assert not fits(_formula(W.SHA256_MESSAGE_SIZES[119], 19))
    # one-block records are the longest that reach depth 19, two-block records the longest that reach depth 18
    assert not fits(_formula(W.SHA256_MESSAGE_SIZES[56], 19)) and not fits(_formula(W.SHA256_MESSAGE_SIZES[120], 18))


def test_bad_shapes_refused():
    for length, depth in [(-1, 1), (3, 0), (3.0, 1), (3, 1.5)]:
        with pytest.raises(C.CircuitError):
            W.MerkleRecord(length, depth)


# ------------------------------------------------------------------ 2. roots
def _root(statements, key, record, sibs, index):
    st, _ = statements[key]
    bits = st.bits(record, sibs, index)
    length, depth = key
    assert bits.shape == (256 + 8 * length + 257 * depth,) and not bits[:256].any()
    row = st.circuit.assign(bits[:256], bits[256:], P18)
    assert st.circuit.holds(bits[:256], bits[256:])
    return st.root_of(row), row


@pytest.mark.parametrize("length,depth,index", [(3, 2, 2), (0, 1, 1), (56, 1, 0)])
def test_root_equals_reference(statements, length, depth, index):
    rng = np.random.default_rng(50 + length)
    record = _record(length)
    sibs = [rng.bytes(32) for _ in range(depth)]
    root, _ = _root(statements, (length, depth), record, sibs, index)
    assert root == ref.merkle_root(hashlib.sha256(record).digest(), sibs, index)


def test_every_index_and_a_flipped_bit(statements):
    key = (3, 2)
    st, _ = statements[key]
    rng = np.random.default_rng(61)
    record = _record(3)
    sibs = [rng.bytes(32) for _ in range(2)]
    leaf = hashlib.sha256(record).digest()
    roots = []
    for index in range(4):
        root, _ = _root(statements, key, record, sibs, index)
        assert root == ref.merkle_root(leaf, sibs, index), index
        roots.append(root)
    assert len(set(roots)) == 4  # the direction bits matter
    # the layout of the private bits: record byte k's bit b at 8 k + b, then the siblings' words, then the direction bits
    bits = st.bits(record, sibs, 2)
    assert np.array_equal(bits[256: 280], np.unpackbits(np.frombuffer(record, dtype=np.uint8), bitorder="little"))
    assert np.array_equal(bits[280: 280 + 512], W.pack(W.be_words(sibs[0] + sibs[1])))
    assert bits[-2:].tolist() == [0, 1]
    for bit in (0, 13, 23):
        other = bytearray(record)
        other[bit >> 3] ^= 1 << (bit & 7)
        root, _ = _root(statements, key, bytes(other), sibs, 2)
        assert root == ref.merkle_root(hashlib.sha256(bytes(other)).digest(), sibs, 2) != roots[2], bit
    for bad_record, bad_sibs, bad_index in [(record + b"x", sibs, 0), (record[:2], sibs, 0), (record, sibs[:1], 0), (record, sibs + [sibs[0]], 0),
                                            (record, [sibs[0], sibs[1][:31]], 0), (record, sibs, 4), (record, sibs, -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(bad_record, bad_sibs, bad_index)


# ------------------------------------------------------------------ 3. statements
def test_statement_is_the_inverse_of_root_of(statements):
    st, _ = statements[(3, 2)]
    rng = np.random.default_rng(62)
    sibs = [rng.bytes(32) for _ in range(2)]
    root, row = _root(statements, (3, 2), _record(3, 1), sibs, 1)
    assert st.statement(root) == bytes(row[:32]) == W.MerklePath.statement(root) == W.MerkleRecord.statement(bytearray(root))
    assert W.MerkleRecord.statement(bytes(range(32)))[:8] == bytes([3, 2, 1, 0, 7, 6, 5, 4])
    for bad in (b"", root[:31], root + b"\0"):
        with pytest.raises(C.CircuitError):
            W.MerkleRecord.statement(bad)


@pytest.mark.parametrize("n", [0, 3, 56])
def test_message_statement(n):
    st = W.Sha256Message(n)
    m = _record(n, 2)
    bits = st.bits(m)
    row = st.circuit.assign(bits[:256], bits[256:], P17)
    digest = hashlib.sha256(m).digest()
    assert W.Sha256Message.statement(digest) == bytes(row[:32])
    assert st.statement(bytearray(digest)) == bytes(row[:32]) and st.digest_of(row) == digest
    assert W.Sha256Message.statement(digest) == W.MerklePath.statement(digest)
    for bad in (b"", digest[:31], digest + b"\0"):
        with pytest.raises(C.CircuitError):
            W.Sha256Message.statement(bad)
