"""CPU: words.MerkleTransfer(key_bytes, length, depth, amount_bytes) -- "v moved from the account k_from to the account k_to, and that alone takes the tree from
root R to root R'" -- on MerkleTransfer(4, 16, 1, 8) and (4, 16, 2, 8), against the brute-force model of tests/merkle_transfer_model.py (a list of records,
hashlib leaves, ref_tree).

1. a correct witness holds, roots_of is the model's root before and after, statement(R, R', k_from, k_to, v) is bits [0, lu) of the assigned row; amount_bytes
   1, 3 and 8; carries and borrows across every byte and the 32-bit boundary (0x00000000FFFFFFFF + 1, 0x0100000000000000 - 1); v = 0; v = the whole balance.
2. each of these ALONE makes holds false: another k_from, another k_to, v off by one in the statement, v = b_p + 1, a receiver at 2^(8A) - 1 with v = 1, an
   inert p, an inert s, the siblings of s taken from the tree BEFORE p's update, a flipped direction bit of p and of s.
3. joined=False over a deeper model tree, p and s in one height-1 subtree and in two: tops_of and the statement bytes.
4. MERKLE_TRANSFER_SIZES / MERKLE_TRANSFER_SPLIT_SIZES are what compile counts, nin, the cost of a level, the (8, 55, 4, 8) fit at d = 2^20 and the depth-5
   refusal; MerkleInsert's and MerkleRemove's programs are what they were (tests/golden/merkle_programs.json is test_merkle_statements_cpu.py's).
5. Words.ripple against Python integers at widths that are no multiple of 8; Circuit.public_last; the argument errors; indexed_transfer and its refusals.
6. k_from = k_to: the no-op the docstring argues -- the witness holds and R' = R."""
import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from merkle_transfer_model import TransferModel, ledger, row_bytes

P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)
K, LENGTH = 4, 16
A_KEY, B_KEY, C_KEY = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("c1aa557f")


@pytest.fixture(scope="module")
def statements():
    return {key: W.MerkleTransfer(*key) for key in [(4, 16, 1, 8), (4, 16, 2, 8), (4, 16, 1, 1), (4, 16, 1, 3)]}


def _records(depth, b_from, b_to, A=8, length=LENGTH):
    """the well-formed table of the accounts A_KEY and B_KEY (depth 2: and C_KEY) with these balances; at depth 1 there is no room for the sentinel record, so
    the two records close the ring by hand: (A, B) and (B, FF..FF)"""
    pay = lambda b: b.to_bytes(A, "big") + bytes(range(0x30, 0x30 + length - 2 * K - A))  # noqa: E731
    if depth == 1:
        return [A_KEY + B_KEY + pay(b_from), B_KEY + b"\xff" * K + pay(b_to)]
    return ledger(W, {A_KEY: b_from, B_KEY: b_to, C_KEY: 77}, K, depth, length, A, np.random.default_rng(5))


def _witness(records, v, A=8, k_from=A_KEY, k_to=B_KEY, public=None, stale=False, p=None, s=None):
    """the arguments of bits() for the transfer with records p and s FORCED (by default the accounts' own), built as the model builds them but without its
    checks; public: the three public pieces where they differ from what is done"""
    m = TransferModel(records, K, A)
    p = m.own(k_from) if p is None else p
    s = m.own(k_to) if s is None else s
    mod = 1 << (8 * A)
    old_p, sibs_p, before = m.records[p], m.siblings(p), m.siblings(s)
    m.set(p, m.with_balance(p, (m.balance(p) - v) % mod))
    old_s, sibs_s = m.records[s], before if stale else m.siblings(s)
    return (public or (k_from, k_to, v % mod)) + (old_p, old_s, sibs_p, p, sibs_s, s)


def _holds(st, args):
    bits = st.bits(*args)
    assert bits.shape == (st.lu + 16 * st.length + 514 * st.depth,) == (st.nin,) and not bits[:512].any()
    return st.circuit.holds(bits[: st.lu], bits[st.lu:])


@pytest.mark.parametrize("key", [(4, 16, 1, 8), (4, 16, 2, 8)])
def test_a_correct_transfer_holds(statements, key):
    st = statements[key]
    _, length, depth, A = key
    assert st.lu == st.circuit.lu == 512 + 16 * K + 8 * A and st.row_bytes == row_bytes(K, length, depth, A)
    records = _records(depth, 1000, 5)
    model = TransferModel(records, K, A)
    before = model.root()
    p, s, args = model.transfer(A_KEY, B_KEY, 300)
    assert args == _witness(records, 300) and p != s
    assert (model.balance(p), model.balance(s)) == (700, 305)
    assert [r[: 2 * K] + r[2 * K + A:] for r in model.records] == [r[: 2 * K] + r[2 * K + A:] for r in records]  # nothing but the balances
    bits = st.bits(*args)
    public = np.unpackbits(np.frombuffer(A_KEY + B_KEY + (300).to_bytes(A, "big"), dtype=np.uint8), bitorder="little")
    assert np.array_equal(bits[512: st.lu], public)
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)
    assert st.roots_of(row) == (before, model.root()) and before != model.root()
    assert st.statement(before, model.root(), A_KEY, B_KEY, 300) == bytes(row[: st.lu // 8]) == W.MerkleUpdate.statement(before, model.root()) + A_KEY + B_KEY + (300).to_bytes(A, "big")
    assert len(np.packbits(bits, bitorder="little")) == st.row_bytes


@pytest.mark.parametrize("A", [1, 3, 8])
def test_amount_widths_carries_and_edges(statements, A):
    st = statements[(4, 16, 1, A)]
    top = (1 << (8 * A)) - 1
    cases = [(top, 0, top), (top, 0, 0), (5, top - 5, 5), (1, top - 1, 1), (0, top, 0), (0, 0, 0), (top // 3, top // 5, top // 7)]  # v = 0, v = the whole balance, up to the limit
    if A == 8:
        cases += [(0x0100000000000000, 0x00000000FFFFFFFF, 1),  # the borrow runs through seven bytes, the carry across the 32-bit boundary
                  (0x0000000100000000, 0x00FFFFFFFFFFFFFF, 1), (0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000)]
    if A == 3:
        cases += [(0x010000, 0x00FFFF, 1), (0x000100, 0x00FF, 1)]  # across every byte
    for b_from, b_to, v in cases:
        records = _records(1, b_from, b_to, A)
        model = TransferModel(records, K, A)
        before = model.root()
        p, s, args = model.transfer(A_KEY, B_KEY, v)
        assert (model.balance(p), model.balance(s)) == (b_from - v, b_to + v)
        bits = st.bits(*args)
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:]), (A, b_from, b_to, v)
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P19)
        assert st.roots_of(row) == (before, model.root()), (A, b_from, b_to, v)
        assert st.statement(before, model.root(), A_KEY, B_KEY, v) == bytes(row[: st.lu // 8])


@pytest.mark.parametrize("key", [(4, 16, 1, 8), (4, 16, 2, 8), (4, 16, 1, 1)])
def test_each_defect_alone_breaks_it(statements, key):
    st = statements[key]
    depth, A = key[2], key[3]
    top = (1 << (8 * A)) - 1
    records = _records(depth, 200, 5, A)
    good = _witness(records, 100, A)
    assert _holds(st, good)
    other = bytes([A_KEY[0]]) + A_KEY[1:3] + bytes([A_KEY[3] ^ 1])
    assert not _holds(st, _witness(records, 100, A, public=(other, B_KEY, 100)))  # another k_from
    assert not _holds(st, _witness(records, 100, A, public=(A_KEY, other, 100)))  # another k_to
    assert not _holds(st, _witness(records, 100, A, public=(B_KEY, A_KEY, 100)))  # the two swapped
    for off in (99, 101):  # v off by one in the statement: what was done is 100
        assert not _holds(st, _witness(records, 100, A, public=(A_KEY, B_KEY, off)))
    assert _holds(st, _witness(records, 200, A))  # the whole balance ...
    assert not _holds(st, _witness(records, 201, A))  # ... and one more: the borrow (the model's records wrap mod 2^(8A), as the subtractor's wires do)
    at_top = _records(depth, 200, top, A)
    assert _holds(st, _witness(at_top, 0, A)) and not _holds(st, _witness(at_top, 1, A))  # a receiver at 2^(8A) - 1 with v = 1: the carry
    assert _holds(st, _witness(_records(depth, 200, top - 1, A), 1, A))
    m = TransferModel(records, K, A)
    p, s = m.own(A_KEY), m.own(B_KEY)
    for hi in (A_KEY, bytes(K)):  # an inert p: lo == hi, lo > hi
        inert = list(records)
        inert[p] = A_KEY + hi + records[p][2 * K:]
        assert not _holds(st, _witness(inert, 100, A, p=p, s=s))
    for hi in (B_KEY, bytes(K)):  # an inert s
        inert = list(records)
        inert[s] = B_KEY + hi + records[s][2 * K:]
        assert not _holds(st, _witness(inert, 100, A, p=p, s=s))
    assert not _holds(st, _witness(records, 100, A, stale=True))  # s's siblings from the tree before p's update: the middle roots differ
    assert not _holds(st, good[:6] + (good[6] ^ 1,) + good[7:])  # a direction bit of p
    assert not _holds(st, good[:8] + (good[8] ^ 1,))  # ... of s
    if depth == 2:
        assert not _holds(st, good[:6] + (good[6] ^ 2,) + good[7:]) and not _holds(st, good[:8] + (good[8] ^ 2,))
        c = m.own(C_KEY)
        assert not _holds(st, _witness(records, 100, A, p=c)) and not _holds(st, _witness(records, 100, A, s=c))  # another account's record as p, as s
        assert _holds(st, _witness(records, 7, A, k_from=C_KEY, k_to=A_KEY))


def test_a_transfer_to_oneself_is_a_no_op(statements):
    st = statements[(4, 16, 2, 8)]
    records = _records(2, 200, 5)
    args = _witness(records, 150, k_from=A_KEY, k_to=A_KEY)
    assert args[6] == args[8]  # s is p, opened after p's update
    bits = st.bits(*args)
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    old, new = st.roots_of(st.circuit.assign(bits[: st.lu], bits[st.lu:], P20))
    assert old == new == TransferModel(records, K).root()
    assert not _holds(st, _witness(records, 201, k_from=A_KEY, k_to=A_KEY))  # ... that still demands v <= b_p


def test_split_form_in_one_subtree_and_in_two():
    A = 8
    st = W.MerkleTransfer(4, 16, 1, A, joined=False)
    assert st.lu == st.circuit.lu == 1024 + 16 * K + 8 * A and st.nin == st.lu + 16 * 16 + 514 and st.row_bytes == row_bytes(K, 16, 1, A, zeros=128)
    with pytest.raises(C.CircuitError):
        W.MerkleTransfer(4, 16, 1).tops_of(bytes(300))
    records = ledger(W, {A_KEY: 900, B_KEY: 10, C_KEY: 33}, K, 2, 16, A, np.random.default_rng(6))  # slots 0 .. 3: the sentinel, A, B, C
    for (k_from, k_to), shared in (((B_KEY, C_KEY), True), ((A_KEY, B_KEY), False)):  # B, C under one level-1 node; A, B under two
        m = TransferModel(records, K, A)
        node = lambda i: m.levels[1][i >> 1]  # noqa: E731
        p, s = m.own(k_from), m.own(k_to)
        assert ((p >> 1) == (s >> 1)) == shared
        x_p = node(p)
        _, _, (_, _, v, old_p, old_s, sibs_p, _, sibs_s, _) = TransferModel(records, K, A).transfer(k_from, k_to, 1)
        m.set(p, m.with_balance(p, m.balance(p) - 1))
        x_p2, x_s = node(p), node(s)
        m.set(s, m.with_balance(s, m.balance(s) + 1))
        x_s2 = node(s)
        assert (x_p2 == x_s) == shared
        args = (k_from, k_to, 1, old_p, old_s, sibs_p[:1], p & 1, sibs_s[:1], s & 1)
        bits = st.bits(*args)
        assert bits.shape == (st.nin,) and not bits[:1024].any()
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P19)
        assert st.tops_of(row) == (x_p, x_p2, x_s, x_s2)
        assert st.statement(x_p, x_p2, x_s, x_s2, k_from, k_to, 1) == bytes(row[: st.lu // 8])
        assert len(st.statement(x_p, x_p2, x_s, x_s2, k_from, k_to, 1)) == 128 + 2 * K + A
        with pytest.raises(C.CircuitError):
            st.statement(x_p, x_s2, k_from, k_to, 1)
        bad = st.bits(k_from, k_to, 2, *args[3:])
        assert st.circuit.holds(bad[: st.lu], bad[st.lu:])  # another amount: ANOTHER pair of new tops, which the upper segments' statements refuse, not this one
        tops = st.tops_of(st.circuit.assign(bad[: st.lu], bad[st.lu:], P19))
        assert (tops[0], tops[2]) == (x_p, x_s) and tops[1] != x_p2 and tops[3] != x_s2
        bad = st.bits(k_to, k_from, 1, *args[3:])  # the defects that do not need the middle roots
        assert not st.circuit.holds(bad[: st.lu], bad[st.lu:])
        bad = st.bits(k_from, k_to, m.balance(p) + 2, *args[3:])  # (m is past the transfer of 1: one more than the sender had)
        assert not st.circuit.holds(bad[: st.lu], bad[st.lu:])


LEVEL = (113986, 202946)


def test_compiled_sizes(statements):
    sizes = W.MERKLE_TRANSFER_SIZES
    assert sorted(sizes) == [(4, 16, 1, 1), (4, 16, 1, 3), (4, 16, 1, 8), (4, 16, 2, 8), (8, 55, 1, 8), (8, 55, 4, 8)]
    assert sorted(W.MERKLE_TRANSFER_SPLIT_SIZES) == [(4, 16, 1, 8), (8, 55, 1, 8), (8, 55, 4, 8)]
    for key, params in [((4, 16, 1, 8), P19), ((4, 16, 2, 8), P20), ((4, 16, 1, 1), P19), ((4, 16, 1, 3), P19), ((8, 55, 1, 8), P19), ((8, 55, 4, 8), P20)]:
        st = statements.get(key) or W.MerkleTransfer(*key)
        cc = st.circuit.compile(params)
        kb, length, depth, A = key
        assert (cc.nwires, cc.nrows) == sizes[key], key
        assert cc.lu == 512 + 16 * kb + 8 * A and len(cc.outputs) == 512 and len(cc.asserts) == 4
        assert cc.nwires - len(cc.program) == st.nin == 512 + 16 * kb + 8 * A + 16 * length + 514 * depth
    for key, params in [((4, 16, 1, 8), P19), ((8, 55, 1, 8), P19), ((8, 55, 4, 8), P20)]:
        st = W.MerkleTransfer(*key, joined=False)
        cc = st.circuit.compile(params)
        assert (cc.nwires, cc.nrows) == W.MERKLE_TRANSFER_SPLIT_SIZES[key] == (sizes[key][0] + 512, sizes[key][1] + 768), key
        kb, length, depth, A = key
        assert cc.lu == 1024 + 16 * kb + 8 * A and len(cc.outputs) == 1024 and cc.nwires - len(cc.program) == st.nin == 1024 + 16 * kb + 8 * A + 16 * length + 514 * depth
    assert tuple(a - b for a, b in zip(sizes[(4, 16, 2, 8)], sizes[(4, 16, 1, 8)])) == LEVEL  # a level: MerkleInsert's
    assert sizes[(8, 55, 4, 8)] == tuple(a + 3 * b for a, b in zip(sizes[(8, 55, 1, 8)], LEVEL)) == (567483, 1009666)
    assert tuple(a - b for a, b in zip(sizes[(4, 16, 1, 3)], sizes[(4, 16, 1, 1)])) == (2 * 48, 2 * 88)  # an amount byte: 8 x (6 wires, 11 rows)
    assert sizes[(8, 55, 4, 8)][0] <= P20.m - 1 and sizes[(8, 55, 4, 8)][1] <= P20.d - 1  # about 1.01 M rows: fits d = 2^20
    with pytest.raises(C.CircuitError):
        statements[(4, 16, 1, 8)].circuit.compile(P18)
    with pytest.raises(C.CircuitError):
        statements[(4, 16, 2, 8)].circuit.compile(P19)


def test_depth_five_does_not_fit_two_to_the_twenty():
    assert W.MERKLE_TRANSFER_SIZES[(8, 55, 4, 8)][1] + LEVEL[1] == 1212612 > P20.d - 1
    with pytest.raises(C.CircuitError) as e:
        W.MerkleTransfer(8, 55, 5, 8).circuit.compile(P20)
    assert "1212612" in str(e.value)


def test_the_other_key_steps_are_what_they_were():
    for cls, sizes in ((W.MerkleInsert, W.MERKLE_INSERT_SIZES), (W.MerkleRemove, W.MERKLE_REMOVE_SIZES)):
        st = cls(4, 8, 1)
        cc = st.circuit.compile(P19)
        assert (cc.nwires, cc.nrows) == sizes[(4, 8, 1)] and st.lu == cc.lu == 512 + 32
        assert st._piece_bytes() == (4,)
    root = bytes(range(32))
    assert W.MerkleRemove(4, 8, 1).statement(root, root, A_KEY) == W.MerkleUpdate.statement(root, root) + A_KEY


def test_ripple_and_public_last():
    rng = np.random.default_rng(9)
    for n in (1, 5, 13):
        w = W.Words()
        a, b = w.c.private(n), w.c.private(n)
        total, carry = w.ripple(a, b)
        diff, borrow = w.ripple(a, b, subtract=True)
        wires = [x.node for x in total + [carry] + diff + [borrow]]
        for t in range(40):
            x, y = (int(v) for v in rng.integers(0, 1 << n, size=2))
            if t % 4 == 0:
                y = x
            val = w.c.evaluate([], [(x >> i) & 1 for i in range(n)] + [(y >> i) & 1 for i in range(n)])
            got = [val[i] for i in wires]
            assert sum(v << i for i, v in enumerate(got[: n + 1])) == x + y
            assert sum(v << i for i, v in enumerate(got[n + 1: 2 * n + 1])) == (x - y) % (1 << n) and got[-1] == int(x < y)
    with pytest.raises(C.CircuitError):
        W.Words().ripple([], [])
    c = C.Circuit()
    early = c.public(2)
    gate = c.AND(*early)
    out = c.output(gate)
    c.public_last(early[::-1])
    assert c._pub == [out.node, early[1].node, early[0].node] and c.lu == 3
    assert c.evaluate([0, 1, 1], [])[gate.node] == 1 and c.evaluate([0, 1, 0], [])[gate.node] == 0  # (the output's position, then early[1], early[0])
    for bad in ([early[0], early[0]], [gate], [out]):
        with pytest.raises(C.CircuitError):
            c.public_last(bad)


def test_argument_errors(statements):
    st = statements[(4, 16, 1, 8)]
    for bad in [(0, 16, 1), (33, 80, 1), (4, 15, 1), (4, 16, 0), (4.0, 16, 1), (4, 16, 1, 0), (4, 16, 1, 9), (4, 16, 1, 8.0), (4, 10, 1, 3)]:
        with pytest.raises(C.CircuitError) as e:
            W.MerkleTransfer(*bad)
        assert str(e.value).startswith("MerkleTransfer: "), str(e.value)
    assert W.MerkleTransfer(4, 11, 1, 3).length == 11  # 2K + A exactly
    good = _witness(_records(1, 9, 9), 1)
    for at, bad in [(0, A_KEY[:3]), (0, bytes(4)), (0, b"\xff" * 4), (1, B_KEY + b"\0"), (1, bytes(4)), (2, -1), (2, 1 << 64), (2, 1.0), (3, good[3][:15]), (4, good[4] + b"\0"),
                    (5, []), (5, [good[5][0][:31]]), (6, 2), (8, -1)]:
        with pytest.raises(C.CircuitError) as e:
            st.bits(*good[:at], bad, *good[at + 1:])
        assert str(e.value).startswith("MerkleTransfer: "), (at, str(e.value))
    root = bytes(range(32))
    for bad in [(root[:31], root, A_KEY, B_KEY, 1), (root, root, A_KEY, bytes(4), 1), (root, root, A_KEY, B_KEY, 1 << 64), (root, root, A_KEY, B_KEY), (root, root, root, root, A_KEY, B_KEY, 1)]:
        with pytest.raises(C.CircuitError) as e:
            st.statement(*bad)
        assert str(e.value).startswith("MerkleTransfer: "), str(e.value)
    assert len(st.statement(root, root[::-1], A_KEY, B_KEY, 5)) == st.lu // 8
    with pytest.raises(C.CircuitError):
        statements[(4, 16, 1, 1)].statement(root, root, A_KEY, B_KEY, 256)


def test_indexed_transfer():
    rec_p, rec_s = bytes([0x03, 0x40, 0x01, 0x00, 9]), bytes([0x40, 0x80, 0x00, 0xFF, 7])  # K = 1, A = 2: balances 256 and 255
    idx, new = W.indexed_transfer(rec_p, 5, rec_s, 2, 1, 1, amount_bytes=2)
    assert idx == [5, 2] and new.dtype == np.uint8 and new.tolist() == [[0x03, 0x40, 0x00, 0xFF, 9], [0x40, 0x80, 0x01, 0x00, 7]]
    idx, new = W.indexed_transfer(rec_p, 5, rec_s, 2, 256, 1, amount_bytes=2)  # the whole balance
    assert new.tolist() == [[0x03, 0x40, 0, 0, 9], [0x40, 0x80, 0x01, 0xFF, 7]]
    assert W.indexed_transfer(rec_p, 5, rec_s, 2, 0, 1, amount_bytes=2)[1].tolist() == [list(rec_p), list(rec_s)]
    full = bytes([0x40, 0x80, 0xFF, 0xFF, 7])
    assert W.indexed_transfer(rec_p, 5, full, 2, 0, 1, amount_bytes=2)[1][1].tobytes() == full
    wide = bytes([0x03, 0x40]) + (1 << 63).to_bytes(8, "big"), bytes([0x40, 0x80]) + ((1 << 63) - 1).to_bytes(8, "big")
    assert W.indexed_transfer(wide[0], 0, wide[1], 1, 1 << 63, 1)[1][1, 2:].tobytes() == b"\xff" * 8  # amount_bytes defaults to 8
    for bad in [(rec_p, 5, rec_s, 2, 257), (rec_p, 5, full, 2, 1),  # an overdraft, an overflow
                (rec_p, 2, rec_s, 2, 1), (rec_p, -1, rec_s, 2, 1),  # p == s
                (bytes([0x40, 0x40, 1, 0, 9]), 5, rec_s, 2, 1), (rec_p, 5, bytes([0x80, 0x40, 0, 0, 7]), 2, 1),  # a record that is not live
                (rec_p, 5, rec_s[:4], 2, 1), (rec_p, 5, rec_s, 2, -1), (rec_p, 5, rec_s, 2, 1 << 16), (rec_p, 5, rec_s, 2, 1.0)]:
        with pytest.raises(C.CircuitError) as e:
            W.indexed_transfer(*bad, 1, amount_bytes=2)
        assert str(e.value).startswith("indexed_transfer: "), str(e.value)
    for kb, ab in ((0, 2), (33, 2), (1, 0), (1, 9), (1, 4), (1.0, 2)):  # (1, 4): the record is shorter than 2K + A
        with pytest.raises(C.CircuitError):
            W.indexed_transfer(rec_p, 5, rec_s, 2, 1, kb, amount_bytes=ab)
