"""CPU: words.MerkleWrite(key_bytes, length, depth, field, expect) -- "bytes [lo, hi) of the record of key k were set to v [, having been e], and that alone
takes the tree from root R to root R'" -- on MerkleWrite(4, 16, 1, (8, 16)), (4, 16, 2, (8, 16)) and (4, 16, 1, (9, 10)), each with expect on and off, against
the brute-force model of tests/merkle_write_model.py (a list of records, hashlib leaves, ref_tree; rows put together byte by byte).

1. the row's sizes and lu; a correct write holds: roots_of is the model's root before and after and MerkleRecordUpdate(16, depth)'s for the same record pair;
   statement(R, R', k, [e,] v) is bits [0, lu) of the assigned row; bits() packed is the model's row; a no-op write (v = the field's bytes) has R' = R.
2. each of these ALONE breaks it.  Circuit.holds is false for: another k, a dead record (lo == hi, lo > hi), a wrong expectation.  The two roots are COMPUTED
   outputs, so a byte changed outside the field (a new record that is not the old one with v), a flipped sibling, a flipped direction bit, another v in the
   statement and a wrong new root break no assertion by themselves: there the test asks what a proof needs (_proves) -- holds, and the circuit arrives at the
   statement's R and R' -- and that is false.  A flipped bit of the statement is another statement.
3. MERKLE_WRITE_SIZES is what compile counts, including (8, 55, 9, (16, 55), True) at d = 2^20, and depth 10 does not fit; the formulas relative to
   MerkleAdjust; the existing size tables and programs are what they were.
4. the argument errors; indexed_write against the model, and its refusals."""
import hashlib
import json

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from merkle_write_model import WriteModel, packed_row, row_bytes, table_of

P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)
K, LENGTH = 4, 16
A_KEY, B_KEY, C_KEY = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("c1aa557f")
SHAPES = [(4, 16, depth, field, expect) for depth, field in ((1, (8, 16)), (2, (8, 16)), (1, (9, 10))) for expect in (False, True)]


@pytest.fixture(scope="module")
def statements():
    return {key: W.MerkleWrite(*key) for key in SHAPES}


@pytest.fixture(scope="module")
def record_updates():
    return {depth: W.MerkleRecordUpdate(16, depth) for depth in (1, 2)}


def _records(depth, length=LENGTH):
    """the well-formed table of the members A_KEY and B_KEY (depth 2: and C_KEY); at depth 1 there is no room for the sentinel record, so the two records close
    the ring by hand: (A, B) and (B, FF..FF)"""
    pay = lambda x: bytes(range(x, x + length - 2 * K))  # noqa: E731
    if depth == 1:
        return [A_KEY + B_KEY + pay(0x30), B_KEY + b"\xff" * K + pay(0x50)]
    return table_of(W, {A_KEY: pay(0x30), B_KEY: pay(0x50), C_KEY: pay(0x70)}, K, depth, length, np.random.default_rng(5))


def _witness(records, field, value, expect, key=A_KEY, public=None, slot=None):
    """the arguments of bits() for the step on the record `slot` FORCED (by default the key's own), without the model's checks; expect: the bytes, or None for
    a plain statement; public: the public pieces where they differ from what is done"""
    m = WriteModel(records, K, field)
    i = m.own(key) if slot is None else slot
    pub = public or ((key,) + (() if expect is None else (expect,)) + (value,))
    return pub + (m.records[i], m.siblings(i), i)


def _holds(st, args):
    bits = st.bits(*args)
    assert bits.shape == (st.nin,) and not bits[:512].any()
    return st.circuit.holds(bits[: st.lu], bits[st.lu:])


def _proves(st, args, roots):
    """the witness holds AND the circuit arrives at the roots (R, R') of the statement: what a proof against statement(R, R', k, [e,] v) needs"""
    bits = st.bits(*args)
    if not st.circuit.holds(bits[: st.lu], bits[st.lu:]):
        return False
    return st.roots_of(st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)) == tuple(roots)


def _value(field, seed=0xA0):
    return bytes((seed + 7 * j) & 0xFF for j in range(field[1] - field[0]))


@pytest.mark.parametrize("key", SHAPES)
def test_sizes_of_the_row(statements, key):
    st = statements[key]
    kb, length, depth, (lo, hi), expect = key
    F = hi - lo
    pub = 8 * (kb + (2 * F if expect else F))
    assert st.lu == st.circuit.lu == 512 + pub and st.field == (lo, hi) and st.field_bytes == F and st.expect is expect
    assert st.nin == 512 + pub + 8 * length + 257 * depth
    assert st.row_bytes == row_bytes(kb, length, depth, F, expect) == 64 + kb + (2 * F if expect else F) + length + 32 * depth + (depth + 7) // 8


@pytest.mark.parametrize("key", SHAPES)
def test_a_correct_write_holds_and_a_no_op_keeps_the_root(statements, record_updates, key):
    st = statements[key]
    _, length, depth, field, expect = key
    lo, hi = field
    ru = record_updates[depth]
    records = _records(depth)
    for value in (_value(field), b"\0" * (hi - lo), b"\xff" * (hi - lo), records[WriteModel(records, K, field).own(A_KEY)][lo:hi]):  # the last: a no-op
        model = WriteModel(records, K, field)
        before = model.root()
        e = model.field(model.own(A_KEY)) if expect else None
        i, args = model.write(A_KEY, value, e)
        assert args == _witness(records, field, value, e)
        assert model.records[i] == records[i][:lo] + value + records[i][hi:] and [r for j, r in enumerate(model.records) if j != i] == [r for j, r in enumerate(records) if j != i]
        bits = st.bits(*args)
        row = packed_row(A_KEY, e, value, args[-3], args[-2], i)
        assert np.array_equal(np.packbits(bits, bitorder="little"), row) and len(row) == st.row_bytes
        public = np.unpackbits(np.frombuffer(A_KEY + (e or b"") + value, dtype=np.uint8), bitorder="little")
        assert np.array_equal(bits[512: st.lu], public)
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:]), value
        assigned = st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)
        assert st.roots_of(assigned) == (before, model.root()) and (before == model.root()) == (value == records[i][lo:hi])
        stmt = st.statement(before, model.root(), A_KEY, *(() if e is None else (e,)), value)
        assert stmt == bytes(assigned[: st.lu // 8]) == W.MerkleUpdate.statement(before, model.root()) + A_KEY + (e or b"") + value
        ubits = ru.bits(args[-3], model.records[i], args[-2], i)  # MerkleRecordUpdate for the same record pair: the same two roots
        assert ru.roots_of(ru.circuit.assign(ubits[:512], ubits[512:], P20)) == st.roots_of(assigned)


@pytest.mark.parametrize("key", SHAPES)
def test_each_defect_alone_breaks_it(statements, key):
    st = statements[key]
    _, length, depth, field, expect = key
    lo, hi = field
    records = _records(depth)
    value = _value(field)
    m = WriteModel(records, K, field)
    i = m.own(A_KEY)
    e = m.field(i) if expect else None
    pub = lambda k=A_KEY, x=e, v=value: (k,) + (() if x is None else (x,)) + (v,)  # noqa: E731
    good = _witness(records, field, value, e)
    done = WriteModel(records, K, field)
    roots = (done.root(), (done.write(A_KEY, value, e), done.root())[1])
    assert _holds(st, good) and _proves(st, good, roots)
    other = A_KEY[:3] + bytes([A_KEY[3] ^ 1])
    assert not _holds(st, _witness(records, field, value, e, public=pub(k=other)))  # another k
    assert not _holds(st, _witness(records, field, value, e, public=pub(k=B_KEY)))
    assert not _holds(st, _witness(records, field, value, m.field(m.own(B_KEY)) if expect else None, slot=m.own(B_KEY)))  # k's statement on another live record
    for dead_hi in (A_KEY, bytes(K)):  # a dead record: lo == hi, lo > hi
        dead = list(records)
        dead[i] = A_KEY + dead_hi + records[i][2 * K:]
        assert not _holds(st, _witness(dead, field, value, e, slot=i))
    if expect:  # a wrong expectation: every single flipped bit of e, and the value in e's place
        for bit in range(8 * (hi - lo)):
            bad = bytearray(e)
            bad[bit // 8] ^= 1 << (bit % 8)
            assert not _holds(st, _witness(records, field, value, e, public=pub(x=bytes(bad)))), bit
        assert not _holds(st, _witness(records, field, value, e, public=pub(x=value)))
    # a byte changed outside the field: the transition to such a record is not what the circuit arrives at, whatever the witness
    for at in [b for b in (2 * K, lo - 1, hi, length - 1) if 2 * K <= b < length and not lo <= b < hi]:
        forged = bytearray(done.records[i])
        forged[at] ^= 0x01
        tampered = WriteModel(records, K, field)
        tampered.set(i, bytes(forged))
        assert not _proves(st, good, (roots[0], tampered.root())), at
    wrong = bytes([value[0] ^ 0x10]) + value[1:]
    assert not _proves(st, pub(v=wrong) + good[-3:], roots)  # another v in the statement: another R'
    assert not _proves(st, good[:-1] + (good[-1] ^ 1,), roots)  # a direction bit: other roots ...
    sibs = [bytearray(x) for x in good[-2]]
    sibs[-1][7] ^= 0x10
    assert not _proves(st, good[:-2] + ([bytes(x) for x in sibs], good[-1]), roots)  # ... a sibling bit: other roots
    assert not _proves(st, good, (roots[0], hashlib.sha256(roots[1]).digest())) and not _proves(st, good, (roots[1], roots[0]))  # a wrong new root
    if depth == 2:
        assert not _proves(st, good[:-1] + (good[-1] ^ 2,), roots)  # the direction bit of the upper level
        assert _holds(st, _witness(records, field, value, m.field(m.own(C_KEY)) if expect else None, key=C_KEY))


@pytest.mark.parametrize("expect", [False, True])
def test_a_flipped_bit_of_the_statement_is_another_statement(statements, expect):
    """the verifier's side of item 2: with the roots of what was done, a statement with any one bit of k, e or v flipped is not the assigned row's"""
    field = (8, 16)
    st = statements[(4, 16, 2, field, expect)]
    records = _records(2)
    model = WriteModel(records, K, field)
    before = model.root()
    e = model.field(model.own(A_KEY)) if expect else None
    _, args = model.write(A_KEY, _value(field), e)
    bits = st.bits(*args)
    row = bytes(st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)[: st.lu // 8])
    pieces = (A_KEY,) + (() if e is None else (e,)) + (_value(field),)
    assert row == st.statement(before, model.root(), *pieces)
    for which, piece in enumerate(pieces):
        for bit in range(8 * len(piece)):
            bad = bytearray(piece)
            bad[bit // 8] ^= 1 << (bit % 8)
            if bytes(bad) in (bytes(K), b"\xff" * K):
                continue
            assert st.statement(before, model.root(), *pieces[:which], bytes(bad), *pieces[which + 1:]) != row, (which, bit)
    assert st.statement(model.root(), before, *pieces) != row


def test_compiled_sizes(statements):
    sizes = W.MERKLE_WRITE_SIZES
    cases = [((4, 16, 1, (8, 16), False), P18), ((4, 16, 1, (8, 16), True), P18), ((4, 16, 1, (9, 10), True), P18), ((4, 16, 2, (8, 16), True), P19),
             ((8, 55, 1, (16, 24), False), P18), ((8, 55, 1, (16, 24), True), P18), ((8, 55, 9, (16, 55), True), P20)]
    assert sorted(sizes) == sorted(c[0] for c in cases)
    for key, params in cases:
        st = statements.get(key) or W.MerkleWrite(*key)
        cc = st.circuit.compile(params)
        kb, length, depth, (lo, hi), expect = key
        F = hi - lo
        assert (cc.nwires, cc.nrows) == sizes[key], key
        assert cc.lu == 512 + 8 * (kb + (2 * F if expect else F)) and len(cc.outputs) == 512 and len(cc.asserts) == 1  # the comparison
        assert cc.nwires - len(cc.program) == st.nin == cc.lu + 8 * length + 257 * depth
    deepest = (8, 55, 9, (16, 55), True)
    assert sizes[deepest][0] <= P20.m - 1 and sizes[deepest][1] <= P20.d - 1
    diff = lambda a, b: tuple(x - y for x, y in zip(a, b))  # noqa: E731
    level = diff(sizes[(4, 16, 2, (8, 16), True)], sizes[(4, 16, 1, (8, 16), True)])
    assert level == diff(W.MERKLE_RECORD_UPDATE_SIZES[(55, 2)], W.MERKLE_RECORD_UPDATE_SIZES[(55, 1)]) == (56993, 101473)  # a level: MerkleRecordUpdate's
    # relative to MerkleAdjust with amount_bytes = F: 8 + 24 F wires and 16 + 48 F rows below it, plain
    for write, adjust in (((4, 16, 1, (8, 16), False), (4, 16, 1, 8)), ((8, 55, 1, (16, 24), False), (8, 55, 1, 8))):
        assert diff(W.MERKLE_ADJUST_SIZES[adjust], sizes[write]) == (8 + 24 * 8, 16 + 48 * 8)
    assert diff(sizes[(4, 16, 1, (8, 16), True)], sizes[(4, 16, 1, (8, 16), False)]) == (8 * 8, 16 * 8)  # expect: 8 F wires, 16 F rows
    assert diff(sizes[(8, 55, 1, (16, 24), True)], sizes[(8, 55, 1, (16, 24), False)]) == (8 * 8, 16 * 8)
    assert diff(sizes[(4, 16, 1, (8, 16), True)], sizes[(4, 16, 1, (9, 10), True)]) == (7 * 16, 7 * 24)  # a field byte: 8 wires and 8 rows, as many again with expect ...
    assert sizes[deepest] == tuple(a + 8 * b + c * (39 - 8) for a, b, c in zip(sizes[(8, 55, 1, (16, 24), True)], level, (16, 24)))  # ... and 8 levels
    with pytest.raises(C.CircuitError):
        statements[(4, 16, 2, (8, 16), True)].circuit.compile(P18)


def test_depth_ten_does_not_fit_two_to_the_twenty():
    sizes = W.MERKLE_WRITE_SIZES
    need = sizes[(8, 55, 9, (16, 55), True)][1] + 101473
    assert need > P20.d - 1
    with pytest.raises(C.CircuitError) as e:
        W.MerkleWrite(8, 55, 10, (16, 55), True).circuit.compile(P20)
    assert str(need) in str(e.value)


def test_the_existing_sizes_and_programs_are_what_they_were():
    import test_merkle_programs_cpu as G

    assert W.MERKLE_ADJUST_SIZES == {(4, 16, 1, 8): (112677, 200400), (4, 16, 1, 1): (112453, 200008), (4, 16, 1, 3): (112517, 200120), (8, 55, 1, 8): (113091, 200910),
                                     (4, 16, 2, 8): (169670, 301873), (8, 55, 9, 8): (569035, 1012694)}
    assert W.MERKLE_RECORD_UPDATE_SIZES[(55, 1)] == (113075, 200501) and W.MERKLE_UPDATE_SIZES[10] == (570956, 1016270)
    assert W.MERKLE_TRANSFER_SIZES[(4, 16, 1, 8)] == (224697, 399808) and W.MERKLE_SEGMENT_SIZES[1] == (58019, 103013)
    want = json.load(open(G.GOLDEN))
    for name in ("MerkleRecordUpdate(8, 1)", "MerkleAbsent(4, 8, 1)"):
        assert G.program_digest(G.STATEMENTS[name](), G.P18) == want[name], name
    cc = W.MerkleAdjust(4, 16, 1, 8).circuit.compile(P18)
    assert (cc.nwires, cc.nrows) == W.MERKLE_ADJUST_SIZES[(4, 16, 1, 8)]


def test_argument_errors(statements):
    for bad in [(0, 16, 1, (8, 16)), (33, 80, 1, (66, 70)), (4, 8, 1, (8, 9)), (4, 16, 0, (8, 16)), (4.0, 16, 1, (8, 16)), (4, 16, 1, (7, 16)), (4, 16, 1, (8, 17)),
                (4, 16, 1, (8, 8)), (4, 16, 1, (12, 10)), (4, 16, 1, (8.0, 16)), (4, 16, 1, 8), (4, 16, 1, (8, 12, 16)), (4, 16, 1, None), (4, 16, 1, (8, 16), 1),
                (4, 16, 1, (8, 16), None)]:
        with pytest.raises(C.CircuitError) as e:
            W.MerkleWrite(*bad)
        assert str(e.value).startswith("MerkleWrite: "), str(e.value)
    assert W.MerkleWrite(4, 9, 1, (8, 9)).field_bytes == 1  # 2K + 1 exactly: the whole payload is one byte
    field = (8, 16)
    records = _records(1)
    e = records[0][8:16]
    for expect in (False, True):
        st = statements[(4, 16, 1, field, expect)]
        good = _witness(records, field, _value(field), e if expect else None)
        n = len(good)
        bad_args = [(0, A_KEY[:3]), (0, bytes(4)), (0, b"\xff" * 4), (n - 4, _value(field)[:7]), (n - 4, _value(field) + b"\0"), (n - 3, good[n - 3][:15]),
                    (n - 3, good[n - 3] + b"\0"), (n - 2, []), (n - 2, [good[n - 2][0][:31]]), (n - 1, 2), (n - 1, -1)]
        if expect:
            bad_args += [(1, e[:7]), (1, e + b"\0")]
        for at, bad in bad_args:
            with pytest.raises(C.CircuitError) as err:
                st.bits(*good[:at], bad, *good[at + 1:])
            assert str(err.value).startswith("MerkleWrite: "), (at, str(err.value))
        for short in (good[:-1], good + (0,)):  # e missing or one piece too many
            with pytest.raises(C.CircuitError) as err:
                st.bits(*short)
            assert str(err.value).startswith("MerkleWrite: ")
        root = bytes(range(32))
        pieces = (A_KEY,) + ((e,) if expect else ()) + (_value(field),)
        for bad in [(root[:31], root) + pieces, (root, root[:31]) + pieces, (root, root, bytes(4)) + pieces[1:], (root, root, b"\xff" * 4) + pieces[1:],
                    (root, root) + pieces[:-1] + (b"x" * 7,), (root, root) + pieces[:-1], (root, root) + pieces + (b"x" * 8,)]:
            with pytest.raises(C.CircuitError) as err:
                st.statement(*bad)
            assert str(err.value).startswith("MerkleWrite: "), str(err.value)
        assert len(st.statement(root, root[::-1], *pieces)) == st.lu // 8


def test_indexed_write():
    rec = bytes([0x03, 0x40, 1, 2, 3, 4, 9])  # K = 1
    new = W.indexed_write(rec, (3, 5), b"\xaa\xbb", 1)
    assert new.dtype == np.uint8 and new.tolist() == [0x03, 0x40, 1, 0xAA, 0xBB, 4, 9]
    assert W.indexed_write(rec, (2, 7), bytes(5), 1).tolist() == [0x03, 0x40, 0, 0, 0, 0, 0]  # the whole payload
    assert W.indexed_write(rec, (6, 7), [7], 1).tolist() == [0x03, 0x40, 1, 2, 3, 4, 7]  # the last byte alone
    assert W.indexed_write(rec, (3, 5), b"\x02\x03", 1).tobytes() == rec  # a no-op
    assert W.indexed_write(rec, (3, 5), b"\xaa\xbb", 1, expect=b"\x02\x03").tolist() == new.tolist()
    rng = np.random.default_rng(3)
    field = (9, 14)
    records = table_of(W, {k: rng.bytes(LENGTH - 2 * K) for k in (A_KEY, B_KEY, C_KEY)}, K, 2, LENGTH, rng)
    model = WriteModel(records, K, field)
    for key, expect in ((A_KEY, False), (B_KEY, True), (A_KEY, True), (C_KEY, False)):
        i = model.own(key)
        v, e = rng.bytes(5), model.field(i) if expect else None
        want = W.indexed_write(model.records[i], field, v, K, expect=e)
        model.write(key, v, e)
        assert want.tobytes() == model.records[i]
    for bad in [(rec, (3, 5), b"\xaa"), (rec, (3, 5), b"\xaa\xbb\xcc"),  # a value of the wrong length
                (rec, (1, 5), bytes(4)), (rec, (3, 8), bytes(5)), (rec, (3, 3), b""), (rec, (5, 3), b""), (rec, (3.0, 5), bytes(2)), (rec, 3, bytes(2)),  # a bad field
                (bytes([0x40, 0x40, 1, 2, 3, 4, 9]), (3, 5), bytes(2)), (bytes([0x80, 0x40, 1, 2, 3, 4, 9]), (3, 5), bytes(2)),  # a record that is not live
                (rec[:2], (2, 3), b"")]:
        with pytest.raises(C.CircuitError) as e:
            W.indexed_write(*bad, 1)
        assert str(e.value).startswith("indexed_write: "), str(e.value)
    for exp in (b"\x02\x04", b"\x02", b"\x02\x03\x04"):  # an expectation the record does not meet, or of the wrong length
        with pytest.raises(C.CircuitError) as e:
            W.indexed_write(rec, (3, 5), b"\xaa\xbb", 1, expect=exp)
        assert str(e.value).startswith("indexed_write: "), str(e.value)
    for kb in (0, 33, 4, 1.0):  # (4: the record has no payload behind two keys of 4 bytes)
        with pytest.raises(C.CircuitError):
            W.indexed_write(rec, (3, 5), bytes(2), kb)
