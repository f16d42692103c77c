"""CPU: words.MerkleAdjust(key_bytes, length, depth, amount_bytes) -- "the balance of the account k went up (side 0) or down (side 1) by v, and that alone takes
the tree from root R to root R'" -- on MerkleAdjust(4, 16, 1, 8), (4, 16, 2, 8), (4, 16, 1, 1) and (4, 16, 1, 3), against the brute-force model of
tests/merkle_adjust_model.py (a list of records, hashlib leaves, ref_tree; rows put together byte by byte).

1. a correct witness holds: both sides, v = 0 on both, the whole balance withdrawn, a deposit up to exactly 2^(8A) - 1, carries and borrows across every byte
   and the 32-bit boundary (0x00000000FFFFFFFF + 1, 0x0100000000000000 - 1); roots_of is the model's root before and after and MerkleRecordUpdate(16, depth)'s
   for the same record pair; statement(R, R', k, v, side) is bits [0, lu) of the assigned row; bits() packed is the model's row; nin, lu, row_bytes.
2. each of these ALONE breaks it.  Circuit.holds is false for: another k, a nonzero bit 1 .. 7 of the side byte, a withdrawal of b + 1, a deposit of 1 onto
   2^(8A) - 1, an inert record.  The two roots are COMPUTED outputs, so v off by one in the statement, the side flipped in the statement, a flipped direction
   bit and a flipped sibling bit break no assertion by themselves: there the test asks what a proof needs (_proves) -- holds, and the circuit arrives at the
   statement's R and R' -- and that is false: the circuit arrives at other roots, or (v > b, b + v past the limit) holds is false as well.
3. MERKLE_ADJUST_SIZES is what compile counts; (8, 55, 9, 8) fits Params(d=1 << 20, m=699050) and (8, 55, 10, 8) does not; the existing statements' programs
   are what tests/golden/merkle_programs.json says (a sample here; tests/test_merkle_programs_cpu.py has them all).
4. indexed_adjust against the model, and its refusals; the argument errors."""
import json

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from merkle_adjust_model import AdjustModel, ledger, packed_row, row_bytes

P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)
K, LENGTH = 4, 16
A_KEY, B_KEY, C_KEY = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("c1aa557f")
SHAPES = [(4, 16, 1, 8), (4, 16, 2, 8), (4, 16, 1, 1), (4, 16, 1, 3)]


@pytest.fixture(scope="module")
def statements():
    return {key: W.MerkleAdjust(*key) for key in SHAPES}


@pytest.fixture(scope="module")
def record_updates():
    return {depth: W.MerkleRecordUpdate(16, depth) for depth in (1, 2)}


def _records(depth, balance, A=8, length=LENGTH, other=5):
    """the well-formed table of the accounts A_KEY and B_KEY (depth 2: and C_KEY); at depth 1 there is no room for the sentinel record, so the two records close
    the ring by hand: (A, B) and (B, FF..FF)"""
    pay = lambda b: b.to_bytes(A, "big") + bytes(range(0x30, 0x30 + length - 2 * K - A))  # noqa: E731
    if depth == 1:
        return [A_KEY + B_KEY + pay(balance), B_KEY + b"\xff" * K + pay(other)]
    return ledger(W, {A_KEY: balance, B_KEY: other, C_KEY: 77}, K, depth, length, A, np.random.default_rng(5))


def _witness(records, v, side, A=8, key=A_KEY, public=None, slot=None):
    """the arguments of bits() for the step on the record `slot` FORCED (by default the account's own), without the model's checks; public: the three public
    pieces where they differ from what is done"""
    m = AdjustModel(records, K, A)
    i = m.own(key) if slot is None else slot
    return (public or (key, v, side)) + (m.records[i], m.siblings(i), i)


def _holds(st, args):
    bits = st.bits(*args)
    assert bits.shape == (st.nin,) and not bits[:512].any()
    return st.circuit.holds(bits[: st.lu], bits[st.lu:])


def _proves(st, args, roots):
    """the witness holds AND the circuit arrives at the roots (R, R') of the statement: what a proof against statement(R, R', k, v, side) needs.  The two roots
    are computed outputs, so a public piece or a sibling that differs from what was done need not break an assertion: it gives another R or R', and that
    statement is then not the one proved"""
    bits = st.bits(*args)
    if not st.circuit.holds(bits[: st.lu], bits[st.lu:]):
        return False
    return st.roots_of(st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)) == tuple(roots)


@pytest.mark.parametrize("key", SHAPES)
def test_sizes_of_the_row(statements, key):
    st = statements[key]
    kb, length, depth, A = key
    assert st.lu == st.circuit.lu == 512 + 8 * (kb + A + 1)
    assert st.nin == 512 + 8 * (kb + A + 1) + 8 * length + 257 * depth
    assert st.row_bytes == row_bytes(kb, length, depth, A) == 64 + kb + A + 1 + length + 32 * depth + (depth + 7) // 8


@pytest.mark.parametrize("key", [(4, 16, 1, 8), (4, 16, 2, 8)])
def test_a_correct_adjust_holds(statements, record_updates, key):
    st = statements[key]
    _, length, depth, A = key
    ru = record_updates[depth]
    for side, v, b in ((0, 300, 1000), (1, 300, 1000), (0, 0, 1000), (1, 0, 1000), (1, 1000, 1000), (0, (1 << 64) - 1 - 1000, 1000)):
        records = _records(depth, b)
        model = AdjustModel(records, K, A)
        before = model.root()
        i, args = model.adjust(A_KEY, v, side)
        assert args == _witness(records, v, side)
        assert model.balance(i) == (b - v if side else b + v)
        assert [r[: 2 * K] + r[2 * K + A:] for r in model.records] == [r[: 2 * K] + r[2 * K + A:] for r in records]  # nothing but the balance
        bits = st.bits(*args)
        assert np.array_equal(np.packbits(bits, bitorder="little"), packed_row(*args, A)) and len(packed_row(*args, A)) == st.row_bytes
        public = np.unpackbits(np.frombuffer(A_KEY + v.to_bytes(A, "big") + bytes([side]), dtype=np.uint8), bitorder="little")
        assert np.array_equal(bits[512: st.lu], public)
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:]), (side, v)
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)
        assert st.roots_of(row) == (before, model.root()) and (before == model.root()) == (v == 0)
        assert st.statement(before, model.root(), A_KEY, v, side) == bytes(row[: st.lu // 8]) \
            == W.MerkleUpdate.statement(before, model.root()) + A_KEY + v.to_bytes(A, "big") + bytes([side])
        ubits = ru.bits(args[3], model.records[i], args[4], i)  # MerkleRecordUpdate for the same record pair: the same two roots
        assert ru.roots_of(ru.circuit.assign(ubits[:512], ubits[512:], P20)) == st.roots_of(row)


@pytest.mark.parametrize("A", [1, 3, 8])
def test_amount_widths_carries_and_edges(statements, A):
    st = statements[(4, 16, 1, A)]
    top = (1 << (8 * A)) - 1
    cases = [(0, 0, top), (0, top, 0), (1, top, top), (1, 0, 0), (0, top - 5, 5), (1, 5, 5), (0, top // 3, top // 5), (1, top // 3, top // 7), (1, top, 1), (0, 0, 1)]  # (side, b, v)
    if A == 8:
        cases += [(0, 0x00000000FFFFFFFF, 1), (1, 0x0100000000000000, 1),  # the carry across the 32-bit boundary, the borrow through seven bytes
                  (1, 0x0000000100000000, 1), (0, 0x00FFFFFFFFFFFFFF, 1), (0, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000), (1, 0x8000000000000000, 0x8000000000000000)]
    if A == 3:
        cases += [(0, 0x00FFFF, 1), (1, 0x010000, 1), (0, 0x0000FF, 1), (1, 0x000100, 1)]  # across every byte
    for side, b, v in cases:
        records = _records(1, b, A)
        model = AdjustModel(records, K, A)
        before = model.root()
        i, args = model.adjust(A_KEY, v, side)
        assert model.balance(i) == (b - v if side else b + v)
        bits = st.bits(*args)
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:]), (A, side, b, v)
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P19)
        assert st.roots_of(row) == (before, model.root()), (A, side, b, v)
        assert st.statement(before, model.root(), A_KEY, v, side) == bytes(row[: st.lu // 8])


@pytest.mark.parametrize("key", SHAPES)
def test_each_defect_alone_breaks_it(statements, key):
    st = statements[key]
    depth, A = key[2], key[3]
    top = (1 << (8 * A)) - 1
    records = _records(depth, 200, A, other=top)  # B_KEY's account stands at the limit
    for side in (0, 1):
        good = _witness(records, 50, side, A)
        done = AdjustModel(records, K, A)
        roots = (done.root(), (done.adjust(A_KEY, 50, side), done.root())[1])
        assert _holds(st, good) and _proves(st, good, roots)
        other = A_KEY[:3] + bytes([A_KEY[3] ^ 1])
        assert not _holds(st, _witness(records, 50, side, A, public=(other, 50, side)))  # another k
        assert not _holds(st, _witness(records, 50, side, A, public=(B_KEY, 50, side)))
        for off in (49, 51):  # v off by one in the statement, the record pair being the one of 50: the circuit arrives at ANOTHER R'
            assert not _proves(st, (A_KEY, off, side) + good[3:], roots)
        assert not _proves(st, (A_KEY, 50, side ^ 1) + good[3:], roots)  # the side flipped in the statement
        for bit in range(1, 8):  # a nonzero bit 1 .. 7 of the side byte
            bits = st.bits(*good)
            bits[512 + 8 * (K + A) + bit] = 1
            assert not st.circuit.holds(bits[: st.lu], bits[st.lu:]), bit
        assert not _proves(st, good[:5] + (good[5] ^ 1,), roots)  # a direction bit: other roots ...
        sibs = [bytearray(x) for x in good[4]]
        sibs[-1][7] ^= 0x10
        assert not _proves(st, good[:4] + ([bytes(x) for x in sibs], good[5]), roots)  # ... a sibling bit: other roots
    assert _holds(st, _witness(records, 200, 1, A))  # the whole balance ...
    assert not _holds(st, _witness(records, 201, 1, A))  # ... and one more: an overdraft
    if A == 8:
        assert not _holds(st, _witness(records, top, 1, A)) and not _holds(st, _witness(_records(depth, 0, A), 1, 1, A))
    assert _holds(st, _witness(records, 0, 0, A, key=B_KEY)) and _holds(st, _witness(records, 0, 1, A, key=B_KEY))
    assert not _holds(st, _witness(records, 1, 0, A, key=B_KEY))  # a deposit of 1 onto 2^(8A) - 1: an overflow
    assert _holds(st, _witness(records, top - 200, 0, A)) and not _holds(st, _witness(records, top - 199, 0, A))
    m = AdjustModel(records, K, A)
    i = m.own(A_KEY)
    for hi in (A_KEY, bytes(K)):  # an inert record: lo == hi, lo > hi
        inert = list(records)
        inert[i] = A_KEY + hi + records[i][2 * K:]
        assert not _holds(st, _witness(inert, 50, 0, A, slot=i)) and not _holds(st, _witness(inert, 50, 1, A, slot=i))
    if depth == 2:
        good = _witness(records, 50, 0, A)
        done = AdjustModel(records, K, A)
        roots = (done.root(), (done.adjust(A_KEY, 50, 0), done.root())[1])
        assert _proves(st, good, roots) and not _proves(st, good[:5] + (good[5] ^ 2,), roots)  # the direction bit of the upper level
        assert not _holds(st, _witness(records, 50, 0, A, slot=m.own(C_KEY)))  # another account's record
        assert _holds(st, _witness(records, 7, 1, A, key=C_KEY))


def test_a_flipped_bit_of_the_statement_is_another_statement(statements):
    """the verifier's side of item 2: with the roots of what was done, a statement with another k, v or side is not the assigned row's"""
    st = statements[(4, 16, 2, 8)]
    records = _records(2, 200)
    model = AdjustModel(records, K, 8)
    before = model.root()
    _, args = model.adjust(A_KEY, 50, 1)
    bits = st.bits(*args)
    row = bytes(st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)[: st.lu // 8])
    assert row == st.statement(before, model.root(), A_KEY, 50, 1)
    for bad in ((B_KEY, 50, 1), (A_KEY, 51, 1), (A_KEY, 49, 1), (A_KEY, 50, 0)):
        assert st.statement(before, model.root(), *bad) != row
    assert st.statement(model.root(), before, A_KEY, 50, 1) != row


def test_compiled_sizes(statements):
    sizes = W.MERKLE_ADJUST_SIZES
    assert sorted(sizes) == [(4, 16, 1, 1), (4, 16, 1, 3), (4, 16, 1, 8), (4, 16, 2, 8), (8, 55, 1, 8), (8, 55, 9, 8)]
    for key, params in [((4, 16, 1, 8), P18), ((4, 16, 2, 8), P19), ((4, 16, 1, 1), P18), ((4, 16, 1, 3), P18), ((8, 55, 1, 8), P18), ((8, 55, 9, 8), P20)]:
        st = statements.get(key) or W.MerkleAdjust(*key)
        cc = st.circuit.compile(params)
        kb, length, depth, A = key
        assert (cc.nwires, cc.nrows) == sizes[key], key
        assert cc.lu == 512 + 8 * (kb + A + 1) and len(cc.outputs) == 512 and len(cc.asserts) == 8  # the side's seven bits and the comparison
        assert cc.nwires - len(cc.program) == st.nin == 512 + 8 * (kb + A + 1) + 8 * length + 257 * depth
    assert sizes[(8, 55, 9, 8)][0] <= P20.m - 1 and sizes[(8, 55, 9, 8)][1] <= P20.d - 1
    level = tuple(a - b for a, b in zip(sizes[(4, 16, 2, 8)], sizes[(4, 16, 1, 8)]))
    assert level == tuple(a - b for a, b in zip(W.MERKLE_RECORD_UPDATE_SIZES[(55, 2)], W.MERKLE_RECORD_UPDATE_SIZES[(55, 1)]))  # a level: MerkleRecordUpdate's
    assert sizes[(8, 55, 9, 8)] == tuple(a + 8 * b for a, b in zip(sizes[(8, 55, 1, 8)], level))
    assert tuple(a - b for a, b in zip(sizes[(4, 16, 1, 3)], sizes[(4, 16, 1, 1)])) == (2 * 32, 2 * 56)  # an amount byte: 8 x (4 wires, 7 rows)
    with pytest.raises(C.CircuitError):
        statements[(4, 16, 2, 8)].circuit.compile(P18)


def test_depth_ten_does_not_fit_two_to_the_twenty():
    sizes = W.MERKLE_ADJUST_SIZES
    level = tuple(a - b for a, b in zip(sizes[(4, 16, 2, 8)], sizes[(4, 16, 1, 8)]))
    assert sizes[(8, 55, 9, 8)][1] + level[1] > P20.d - 1
    with pytest.raises(C.CircuitError) as e:
        W.MerkleAdjust(8, 55, 10, 8).circuit.compile(P20)
    assert str(sizes[(8, 55, 9, 8)][1] + level[1]) in str(e.value)


def test_the_existing_programs_are_what_they_were():
    import test_merkle_programs_cpu as G

    want = json.load(open(G.GOLDEN))
    for name in ("MerkleRecordUpdate(8, 1)", "MerkleAbsent(4, 8, 1)"):
        assert G.program_digest(G.STATEMENTS[name](), G.P18) == want[name], name
    for name in ("MerkleInsert(4, 8, 1)", "MerkleRemove(4, 8, 1)"):
        assert G.program_digest(G.STATEMENTS[name](), G.P19) == want[name], name
    cc = W.MerkleTransfer(4, 16, 1, 8).circuit.compile(P19)  # Words.ripple is what it was
    assert (cc.nwires, cc.nrows) == W.MERKLE_TRANSFER_SIZES[(4, 16, 1, 8)]


def test_argument_errors(statements):
    st = statements[(4, 16, 1, 8)]
    for bad in [(0, 16, 1), (33, 80, 1), (4, 15, 1), (4, 16, 0), (4.0, 16, 1), (4, 16, 1, 0), (4, 16, 1, 9), (4, 16, 1, 8.0), (4, 10, 1, 3)]:
        with pytest.raises(C.CircuitError) as e:
            W.MerkleAdjust(*bad)
        assert str(e.value).startswith("MerkleAdjust: "), str(e.value)
    assert W.MerkleAdjust(4, 11, 1, 3).length == 11  # 2K + A exactly
    good = _witness(_records(1, 9), 1, 0)
    for at, bad in [(0, A_KEY[:3]), (0, bytes(4)), (0, b"\xff" * 4), (1, -1), (1, 1 << 64), (1, 1.0), (2, 2), (2, -1), (2, 1.0), (3, good[3][:15]), (3, good[3] + b"\0"),
                    (4, []), (4, [good[4][0][:31]]), (5, 2), (5, -1)]:
        with pytest.raises(C.CircuitError) as e:
            st.bits(*good[:at], bad, *good[at + 1:])
        assert str(e.value).startswith("MerkleAdjust: "), (at, str(e.value))
    root = bytes(range(32))
    for bad in [(root[:31], root, A_KEY, 1, 0), (root, root[:31], A_KEY, 1, 0), (root, root, bytes(4), 1, 0), (root, root, b"\xff" * 4, 1, 0), (root, root, A_KEY, 1 << 64, 0),
                (root, root, A_KEY, -1, 0), (root, root, A_KEY, 1, 2), (root, root, A_KEY, 1, -1)]:
        with pytest.raises(C.CircuitError) as e:
            st.statement(*bad)
        assert str(e.value).startswith("MerkleAdjust: "), str(e.value)
    assert len(st.statement(root, root[::-1], A_KEY, 5, 1)) == st.lu // 8
    with pytest.raises(C.CircuitError):
        statements[(4, 16, 1, 1)].statement(root, root, A_KEY, 256, 0)


def test_indexed_adjust():
    rec = bytes([0x03, 0x40, 0x01, 0x00, 9])  # K = 1, A = 2: the balance is 256
    new = W.indexed_adjust(rec, 1, 1, 1, amount_bytes=2)
    assert new.dtype == np.uint8 and new.tolist() == [0x03, 0x40, 0x00, 0xFF, 9]
    assert W.indexed_adjust(rec, 255, 0, 1, amount_bytes=2).tolist() == [0x03, 0x40, 0x01, 0xFF, 9]
    assert W.indexed_adjust(rec, 256, 1, 1, amount_bytes=2).tolist() == [0x03, 0x40, 0, 0, 9]  # the whole balance
    assert W.indexed_adjust(rec, 0xFEFF, 0, 1, amount_bytes=2).tolist() == [0x03, 0x40, 0xFF, 0xFF, 9]  # up to the limit
    for side in (0, 1):
        assert W.indexed_adjust(rec, 0, side, 1, amount_bytes=2).tobytes() == rec
    wide = bytes([0x03, 0x40]) + ((1 << 63) - 1).to_bytes(8, "big")
    assert W.indexed_adjust(wide, 1 << 63, 0, 1)[2:].tobytes() == b"\xff" * 8  # amount_bytes defaults to 8
    rng = np.random.default_rng(3)
    records = ledger(W, {A_KEY: 1000, B_KEY: 5, C_KEY: 77}, K, 2, LENGTH, 8, rng)
    model = AdjustModel(records, K, 8)
    for key, v, side in ((A_KEY, 300, 1), (B_KEY, 300, 0), (A_KEY, 700, 1), (C_KEY, 0, 0)):
        i = model.own(key)
        want = W.indexed_adjust(model.records[i], v, side, K)
        model.adjust(key, v, side)
        assert want.tobytes() == model.records[i]
    for bad in [(rec, 257, 1), (rec, 0xFF00, 0),  # an overdraft, an overflow
                (bytes([0x40, 0x40, 1, 0, 9]), 1, 0), (bytes([0x80, 0x40, 1, 0, 9]), 1, 1),  # a record that is not live
                (rec, -1, 0), (rec, 1 << 16, 0), (rec, 1.0, 0), (rec, 1, 2), (rec, 1, -1), (rec[:3], 1, 0)]:
        with pytest.raises(C.CircuitError) as e:
            W.indexed_adjust(*bad, 1, amount_bytes=2)
        assert str(e.value).startswith("indexed_adjust: "), str(e.value)
    for kb, ab in ((0, 2), (33, 2), (1, 0), (1, 9), (1, 4), (1.0, 2)):  # (1, 4): the record is shorter than 2K + A
        with pytest.raises(C.CircuitError):
            W.indexed_adjust(rec, 1, 0, kb, amount_bytes=ab)
