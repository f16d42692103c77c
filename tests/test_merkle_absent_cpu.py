"""CPU: the non-membership statement words.MerkleAbsent(key_bytes, length, depth), its comparator and the host helpers of indexed tables.

1. Words.less_than against Python integers: exhaustive at 3 bits; at 8, 32 and 256 bits on crafted pairs -- equal values, values that differ in the top
   bit only, in the bottom bit only, 0 against the maximum, and the byte-order trap 00 00 01 00 against 00 00 00 FF; its cost, 2 wires and 4 rows a bit.
2. MerkleAbsent(4, 8, 1) and MerkleAbsent(8, 21, 2) against hashlib and tests/sha256_ref.py: a row holds for lo < q < hi with root_of the model's root;
   it does not hold for q == lo, q == hi, q < lo, q > hi (the root is still the model's), with a flipped record byte (another root) or a flipped direction
   bit; keys that differ from lo or hi in the first byte only or in the last bit only compare as big-endian integers; statement(root, key) is bits
   [0, lu) of the assigned row; lu; the argument errors.
3. MERKLE_ABSENT_SIZES against compile and against "MerkleRecord plus 40 K wires and 72 K + 2 rows"; (8, 55, 19) fits Params(d=1 << 20, m=699050) and
   (8, 55, 20) does not.
4. indexed_records / indexed_insert: the invariant checked by brute force (every key of a small key space is in exactly one live range or is a member),
   the errors, and an insert applied to the table keeps the invariant."""
import hashlib
import itertools

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P17 = mf.Params(d=1 << 17, m=87381)
P18 = mf.Params(d=1 << 18, m=174762)
P20 = mf.Params(d=1 << 20, m=699050)


# ------------------------------------------------------------------ 1. the comparator
def _less(n):
    w = W.Words()
    a, b = w.c.private(n), w.c.private(n)
    out = w.less_than(a, b)
    node = out.node
    return w, lambda x, y: w.c.evaluate([], [(x >> i) & 1 for i in range(n)] + [(y >> i) & 1 for i in range(n)])[node]


def test_less_than_exhaustive_at_three_bits():
    _, lt = _less(3)
    for x, y in itertools.product(range(8), repeat=2):
        assert lt(x, y) == int(x < y), (x, y)


@pytest.mark.parametrize("n", [8, 32, 256])
def test_less_than_crafted_pairs(n):
    w, lt = _less(n)
    top, mx = 1 << (n - 1), (1 << n) - 1
    rng = np.random.default_rng(11000 + n)
    r = int.from_bytes(rng.bytes(n // 8), "big") | 2  # (neither 0 nor 1)
    pairs = [(0, 0), (mx, mx), (r, r), (r & ~top, r | top), (top, 0), (top - 1, top), (r & ~1, r | 1), (0, 1), (mx - 1, mx), (0, mx)]
    if n >= 32:  # the byte-order trap: as big-endian integers 00 00 01 00 is the larger one, byte by byte from the wrong end it is not
        pairs.append((int.from_bytes(bytes([0, 0, 1, 0]), "big") << (n - 32), int.from_bytes(bytes([0, 0, 0, 0xFF]), "big") << (n - 32)))
        pairs.append((0x0100, 0x00FF))
    for x, y in pairs:
        assert lt(x, y) == int(x < y) and lt(y, x) == int(y < x), (n, hex(x), hex(y))
    cc = w.c.compile(P17)
    assert cc.nwires == 2 * n + 1 + 2 * n and cc.nrows == cc.nwires + 2 * n + 1  # inputs, const(0), a NOT and a MAJ a bit; a row per wire and per gate


def test_less_than_refuses_bad_operands():
    w = W.Words()
    a = w.c.private(3)
    for x, y in [([], []), (a, a[:2])]:
        with pytest.raises(C.CircuitError):
            w.less_than(x, y)


# ------------------------------------------------------------------ 2. the statement
SHAPES = [(4, 8, 1), (8, 21, 2)]


@pytest.fixture(scope="module")
def statements():
    return {key: W.MerkleAbsent(*key) for key in SHAPES}


def _case(key):
    """(lo, hi, record, siblings, index) with room on both sides of lo and hi and between them"""
    K, length, depth = key
    rng = np.random.default_rng(11100 + length)
    mid = rng.bytes(K - 2)
    lo, hi = bytes([0x40]) + mid + bytes([0x80]), bytes([0x41]) + mid + bytes([0x7F])
    return lo, hi, lo + hi + rng.bytes(length - 2 * K), [rng.bytes(32) for _ in range(depth)], (1 << depth) - 1


def _add(key: bytes, x: int) -> bytes:
    return (int.from_bytes(key, "big") + x).to_bytes(len(key), "big")


def _run(st, q, record, sibs, index):
    bits = st.bits(q, record, sibs, index)
    lu = st.lu
    assert bits.shape == (lu + 8 * st.length + 257 * st.depth,) and not bits[:256].any()
    assert np.array_equal(bits[256: lu], np.unpackbits(np.frombuffer(q, dtype=np.uint8), bitorder="little"))
    row = st.circuit.assign(bits[:lu], bits[lu:], P18)
    return st.circuit.holds(bits[:lu], bits[lu:]), st.root_of(row), row


@pytest.mark.parametrize("key", SHAPES)
def test_holds_exactly_inside_the_range(statements, key):
    st = statements[key]
    K, length, depth = key
    lo, hi, record, sibs, index = _case(key)
    root = ref.merkle_root(hashlib.sha256(record).digest(), sibs, index)
    assert st.lu == st.circuit.lu == 256 + 8 * K
    first_byte = bytes([hi[0]]) + lo[1:]  # differs from lo in byte 0 only and from hi in the last byte only (0x80 > 0x7F): above hi
    inside = [_add(lo, 1), _add(hi, -1), bytes([lo[0]]) + b"\xff" * (K - 1), bytes([hi[0]]) + bytes(K - 1)]
    outside = [lo, hi, _add(lo, -1), _add(hi, 1), bytes([lo[0] - 1]) + b"\xff" * (K - 1), bytes([hi[0] + 1]) + bytes(K - 1), first_byte]
    for q in inside:
        ok, got, row = _run(st, q, record, sibs, index)
        assert ok and got == root, q.hex()
        assert st.statement(root, q) == bytes(row[: st.lu // 8]) == W.MerklePath.statement(root) + q
    for q in outside:
        ok, got, _ = _run(st, q, record, sibs, index)
        assert not ok and got == root, q.hex()
    q = inside[0]
    other = bytearray(record)
    other[length - 1] ^= 0x10
    ok, got, _ = _run(st, q, bytes(other), sibs, index)
    assert ok and got == ref.merkle_root(hashlib.sha256(bytes(other)).digest(), sibs, index) != root  # holds, but for another root
    ok, got, _ = _run(st, q, record, sibs, index ^ 1)
    assert got == ref.merkle_root(hashlib.sha256(record).digest(), sibs, index ^ 1) != root


def test_argument_errors(statements):
    st = statements[(4, 8, 1)]
    lo, hi, record, sibs, index = _case((4, 8, 1))
    q = _add(lo, 1)
    for k, length, depth in [(0, 8, 1), (33, 66, 1), (4, 7, 1), (4, 8, 0), (4.0, 8, 1), (4, 8.0, 1)]:
        with pytest.raises(C.CircuitError):
            W.MerkleAbsent(k, length, depth)
    for bad in [(q[:3], record, sibs, 0), (q + b"\0", record, sibs, 0), (bytes(4), record, sibs, 0), (b"\xff" * 4, record, sibs, 0), (q, record[:7], sibs, 0),
                (q, record, [], 0), (q, record, [sibs[0][:31]], 0), (q, record, sibs, 2), (q, record, sibs, -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(*bad)
    root = bytes(range(32))
    for bad_root, bad_key in [(root[:31], q), (root, q[:3]), (root, bytes(4)), (root, b"\xff" * 4)]:
        with pytest.raises(C.CircuitError):
            st.statement(bad_root, bad_key)
    assert st.statement(root, q) == W.MerklePath.statement(root) + q and len(st.statement(root, q)) == st.lu // 8


# ------------------------------------------------------------------ 3. sizes
def _formula(K, length, depth):
    """MerkleRecord(length, depth)'s sizes (Sha256Message(length) plus 28 625 depth wires and 50 865 depth rows) plus 40 K wires and 72 K + 2 rows"""
    wires, rows = W.SHA256_MESSAGE_SIZES[length]
    return wires + 28625 * depth + 40 * K, rows + 50865 * depth + 72 * K + 2


def test_compiled_sizes(statements):
    cc = statements[(4, 8, 1)].circuit.compile(P17)
    assert (cc.nwires, cc.nrows) == W.MERKLE_ABSENT_SIZES[(4, 8, 1)] and cc.lu == 288 and len(cc.outputs) == 256 and len(cc.asserts) == 2
    assert cc.nwires - len(cc.program) == 288 + 64 + 257
    record = W.MerkleRecord(8, 1).circuit.compile(P17)
    assert (cc.nwires, cc.nrows) == (record.nwires + 40 * 4, record.nrows + 72 * 4 + 2)
    cc = W.MerkleAbsent(8, 16, 1).circuit.compile(P17)
    assert (cc.nwires, cc.nrows) == W.MERKLE_ABSENT_SIZES[(8, 16, 1)]
    cc = W.MerkleAbsent(32, 64, 1).circuit.compile(P18)
    record = W.MerkleRecord(64, 1).circuit.compile(P18)
    assert (cc.nwires, cc.nrows) == W.MERKLE_ABSENT_SIZES[(32, 64, 1)] == (record.nwires + 40 * 32, record.nrows + 72 * 32 + 2)
    with pytest.raises(C.CircuitError):
        W.MerkleAbsent(32, 64, 1).circuit.compile(P17)


def test_deepest_at_two_to_the_twenty():
    st = W.MerkleAbsent(8, 55, 19)
    cc = st.circuit.compile(P20)
    assert (cc.nwires, cc.nrows) == W.MERKLE_ABSENT_SIZES[(8, 55, 19)] == _formula(8, 55, 19) == (572237, 1016529)
    deeper = _formula(8, 55, 20)
    assert deeper[1] == 1067394 > P20.d - 1
    with pytest.raises(C.CircuitError):
        W.MerkleAbsent(8, 55, 20).circuit.compile(P20)


# ------------------------------------------------------------------ 4. indexed tables
def _invariant(table, K):
    """every non-sentinel key of the K-byte key space (K = 1) is a member or in exactly one live range; returns the sorted members"""
    assert K == 1
    live = [(int(r[0]), int(r[1])) for r in table if r[0] < r[1]]
    members = sorted(lo for lo, _ in live if lo != 0)
    assert sorted(lo for lo, _ in live) == [0] + members and sorted(hi for _, hi in live) == members + [0xFF]
    for q in range(1, 0xFF):
        holding = [(lo, hi) for lo, hi in live if lo < q < hi]
        assert len(holding) == (0 if q in members else 1), q
    return members


def test_indexed_records_and_insert():
    keys = [bytes([x]) for x in (0x80, 0x03, 0xFE, 0x7F, 0x01)]
    pay = [bytes([i, i]) for i in range(5)]
    table = W.indexed_records(keys, 3, length=5, payloads=pay)
    assert table.dtype == np.uint8 and table.shape == (8, 5)
    assert _invariant(table, 1) == [0x01, 0x03, 0x7F, 0x80, 0xFE]
    assert table[0].tolist() == [0, 1, 0, 0, 0] and table[1].tolist() == [0x01, 0x03, 4, 4, 0] and table[5].tolist() == [0xFE, 0xFF, 2, 2, 0]
    assert not table[6:].any()
    # the empty set: the sentinel record alone
    empty = W.indexed_records(np.zeros((0, 2), dtype=np.uint8), 1)
    assert empty.tolist() == [[0, 0, 0xFF, 0xFF], [0, 0, 0, 0]]
    # longer keys are ordered as big-endian integers
    t2 = W.indexed_records([bytes([1, 0]), bytes([0, 0xFF])], 2)
    assert t2[:3].tolist() == [[0, 0, 0, 0xFF], [0, 0xFF, 1, 0], [1, 0, 0xFF, 0xFF]]
    full = [bytes([x]) for x in range(1, 8)]
    assert _invariant(W.indexed_records(full, 3), 1) == list(range(1, 8))
    for bad in [dict(keys=full + [b"\x09"], depth=3), dict(keys=[b"\x01", b"\x01"], depth=3), dict(keys=[b"\x00"], depth=3), dict(keys=[b"\xff"], depth=3),
                dict(keys=[b"\x01", b"\x01\x02"], depth=3), dict(keys=[], depth=3), dict(keys=[b"\x01"], depth=0), dict(keys=[b"\x01"], depth=3, length=1),
                dict(keys=[b"\x01"], depth=3, length=3, payloads=[b"ab"]), dict(keys=[b"\x01"], depth=3, payloads=[]),
                dict(keys=np.zeros((1, 33), dtype=np.uint8) + 1, depth=3)]:
        with pytest.raises(C.CircuitError):
            W.indexed_records(**bad)
    # an insert: record 3 = (0x7F, 0x80) has no room; 0x40 goes into the range of record 2 = (0x03, 0x7F)
    idx, new = W.indexed_insert(table[2].tobytes(), 2, b"\x40", 7, payload=b"\x09")
    assert idx == [2, 7] and new.dtype == np.uint8
    assert new.tolist() == [[0x03, 0x40, 1, 1, 0], [0x40, 0x7F, 9, 0, 0]]
    for i, r in zip(idx, new):
        table[i] = r
    assert _invariant(table, 1) == [0x01, 0x03, 0x40, 0x7F, 0x80, 0xFE]
    for bad in [(table[3].tobytes(), 3, b"\x7f", 6), (table[3].tobytes(), 3, b"\x80", 6), (table[3].tobytes(), 3, b"\x10", 6), (table[3].tobytes(), 3, b"", 6),
                (table[2].tobytes(), 2, b"\x10", 2), (table[2].tobytes(), 2, b"\x10", 6, b"abcd"), (b"\x01", 2, b"\x10", 6)]:
        with pytest.raises(C.CircuitError):
            W.indexed_insert(*bad)
