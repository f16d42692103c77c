"""CPU: words.MerkleRemove(key_bytes, length, depth) -- "key k was removed, and that alone takes the tree from root R to root R'" -- on MerkleRemove(4, 8, 1)
and MerkleRemove(4, 8, 2), against the brute-force model of tests/merkle_remove_model.py (a list of records, hashlib leaves, ref_tree).

1. a correct witness holds, roots_of is the model's root before and after, statement(R, R', k) is bits [0, lu) of the assigned row.
2. each of these ALONE makes holds false: another key in the statement, a p whose hi is not k, an s whose lo is not k, s == p, the siblings of s taken from
   the tree BEFORE p's update, a flipped direction bit of p and of s, lo_p == k and lo_p > k, hi_s == k and hi_s < k.
3. joined=False over a deeper model tree, p and s in one height-1 subtree and in two: tops_of, the statement bytes, and that it refuses what 2 refuses.
4. MERKLE_REMOVE_SIZES / MERKLE_REMOVE_SPLIT_SIZES are what compile counts, nin, the cost of a level, the (8, 55, 4) fit and the depth-5 refusal.
5. the argument errors; indexed_remove and its refusals.
6. removes applied to a model table keep test_merkle_absent_cpu.py's brute-force invariant and are indexed_remove's two updates; inserting a batch and removing
   the same keys restores the table's bytes and the root."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from merkle_remove_model import RemoveModel, row_bytes
from test_merkle_absent_cpu import _add, _invariant

P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)
SHAPES = [(4, 8, 1), (4, 8, 2)]
K = 4
LO, KEY, HI = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("41aa557f")


@pytest.fixture(scope="module")
def statements():
    return {key: W.MerkleRemove(*key) for key in SHAPES}


def _records(depth, p_rec=None, s_rec=None):
    """(records, p, s): the well-formed table of the members KEY and HI (depth 1: KEY alone, with lo_p the zero sentinel and hi_s = FF..FF) in which KEY is to
    be removed, records p and s replaced on request"""
    if depth == 1:
        records, p, s = [bytes(K) + KEY, KEY + b"\xff" * K], 0, 1
    else:
        records, p, s = [bytes(K) + LO, HI + b"\xff" * K, KEY + HI, LO + KEY], 3, 2
    records[p] = records[p] if p_rec is None else p_rec
    records[s] = records[s] if s_rec is None else s_rec
    return records, p, s


def _witness(records, p, s, public=KEY, stale=False):
    """the arguments of bits() for the remove with records p and s FORCED, built as the model builds them but without its search"""
    m = RemoveModel(records, K)
    old_p, sibs_p, before = m.records[p], m.siblings(p), m.siblings(s)
    m.set(p, old_p[:K] + m.records[s][K: 2 * K] + old_p[2 * K:])
    old_s, sibs_s = m.records[s], before if stale else m.siblings(s)
    return (public, old_p, old_s, sibs_p, p, sibs_s, s)


def _holds(st, args):
    bits = st.bits(*args)
    assert bits.shape == (st.lu + 16 * st.length + 514 * st.depth,) == (st.nin,) and not bits[:512].any()
    return st.circuit.holds(bits[: st.lu], bits[st.lu:])


@pytest.mark.parametrize("key", SHAPES)
def test_a_correct_remove_holds(statements, key):
    st = statements[key]
    _, length, depth = key
    assert st.lu == st.circuit.lu == 512 + 8 * K and st.row_bytes == row_bytes(K, length, depth) == 64 + K + 2 * length + 64 * depth + (2 * depth + 7) // 8
    records, p, s = _records(depth)
    model = RemoveModel(records, K)
    before = model.root()
    got_p, got_s, args = model.remove(KEY)
    assert (got_p, got_s) == (p, s) and args == _witness(records, p, s)
    assert model.records[s] == bytes(length) and model.records[p] == records[p][:K] + records[s][K:]
    bits = st.bits(*args)
    assert np.array_equal(bits[512: st.lu], np.unpackbits(np.frombuffer(KEY, dtype=np.uint8), bitorder="little"))
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)
    assert st.roots_of(row) == (before, model.root()) and before != model.root()
    assert st.statement(before, model.root(), KEY) == bytes(row[: st.lu // 8]) == W.MerkleUpdate.statement(before, model.root()) + KEY
    assert len(np.packbits(bits, bitorder="little")) == st.row_bytes
    # the new leaf of s is the constant digest of the all-zero record
    assert model.levels[0][s] == hashlib.sha256(bytes(length)).digest()


@pytest.mark.parametrize("key", SHAPES)
def test_each_defect_alone_breaks_it(statements, key):
    st = statements[key]
    depth = key[2]
    records, p, s = _records(depth)
    lo_p, hi_s = records[p][:K], records[s][K:]
    good = _witness(records, p, s)
    assert _holds(st, good)
    assert not _holds(st, _witness(records, p, s, public=_add(KEY, 1)))  # another key in the statement
    assert not _holds(st, _witness(*_records(depth, p_rec=lo_p + _add(KEY, 1))))  # a p whose hi is not k
    assert not _holds(st, _witness(*_records(depth, s_rec=_add(KEY, 1) + hi_s)))  # an s whose lo is not k
    assert not _holds(st, _witness(records, p, p))  # s == p: old_s is p's record after its update, whose lo is lo_p
    assert not _holds(st, _witness(records, p, s, stale=True))  # s's siblings from the tree before p's update: the middle roots differ
    assert not _holds(st, good[:4] + (good[4] ^ 1,) + good[5:])  # a direction bit of p
    assert not _holds(st, good[:6] + (good[6] ^ 1,))  # ... of s
    if depth == 2:
        assert not _holds(st, good[:4] + (good[4] ^ 2,) + good[5:]) and not _holds(st, good[:6] + (good[6] ^ 2,))
        for other in (0, 1):  # another live record as s, another as p
            assert not _holds(st, _witness(records, p, other)) and not _holds(st, _witness(records, other, s))
    for bad in (KEY, _add(KEY, 1), b"\xff" * K):  # lo_p == k, lo_p > k
        assert not _holds(st, _witness(*_records(depth, p_rec=bad + KEY))), bad.hex()
    for bad in (KEY, _add(KEY, -1), bytes(K)):  # hi_s == k, hi_s < k
        assert not _holds(st, _witness(*_records(depth, s_rec=KEY + bad))), bad.hex()
    # the byte order of the comparisons: a lo_p above k in the first byte alone, a hi_s below k in the first byte alone
    assert not _holds(st, _witness(*_records(depth, p_rec=bytes([KEY[0] + 1]) + bytes(K - 1) + KEY)))
    assert not _holds(st, _witness(*_records(depth, s_rec=KEY + bytes([KEY[0] - 1]) + b"\xff" * (K - 1))))
    assert _holds(st, _witness(*_records(depth, p_rec=bytes([KEY[0] - 1]) + b"\xff" * (K - 1) + KEY)))
    assert _holds(st, _witness(*_records(depth, s_rec=KEY + bytes([KEY[0] + 1]) + bytes(K - 1))))


def test_split_form_in_one_subtree_and_in_two():
    st = W.MerkleRemove(4, 8, 1, joined=False)
    assert st.lu == st.circuit.lu == 1024 + 8 * K and st.nin == 1024 + 8 * K + 16 * 8 + 514 and st.row_bytes == row_bytes(K, 8, 1, zeros=128)
    with pytest.raises(C.CircuitError):
        W.MerkleRemove(4, 8, 1).tops_of(bytes(200))
    one = ([bytes(K) + KEY, KEY + HI, HI + b"\xff" * K, bytes(8)], 0, 1)  # p and s under one level-1 node
    two = ([bytes(K) + LO, LO + KEY, KEY + HI, HI + b"\xff" * K], 1, 2)  # ... under two
    for (records, p, s), shared in ((one, True), (two, False)):
        m = RemoveModel(records, K)
        node = lambda i: m.levels[1][i >> 1]  # noqa: E731
        x_p = node(p)
        got_p, got_s, (key, old_p, old_s, sibs_p, _, sibs_s, _) = RemoveModel(records, K).remove(KEY)
        assert (got_p, got_s) == (p, s)
        m.set(p, old_p[:K] + records[s][K:])
        x_p2, x_s = node(p), node(s)
        m.set(s, bytes(8))
        x_s2 = node(s)
        assert (x_p2 == x_s) == shared
        args = (key, old_p, old_s, sibs_p[:1], p & 1, sibs_s[:1], s & 1)
        bits = st.bits(*args)
        assert bits.shape == (st.nin,) and not bits[:1024].any()
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P19)
        assert st.tops_of(row) == (x_p, x_p2, x_s, x_s2)
        assert st.statement(x_p, x_p2, x_s, x_s2, KEY) == bytes(row[: st.lu // 8])
        assert len(st.statement(x_p, x_p2, x_s, x_s2, KEY)) == 128 + K
        with pytest.raises(C.CircuitError):
            st.statement(x_p, x_s2, KEY)
        # the defects of the joined form that do not need the middle roots
        bad = st.bits(_add(KEY, 1), *args[1:])
        assert not st.circuit.holds(bad[: st.lu], bad[st.lu:])
        bad = st.bits(*args[:4], args[4] ^ 1, *args[5:])
        assert st.circuit.holds(bad[: st.lu], bad[st.lu:])  # a flipped direction: ANOTHER top, which the upper segment's statement refuses, not this one
        assert st.tops_of(st.circuit.assign(bad[: st.lu], bad[st.lu:], P19))[:2] != (x_p, x_p2)
        bad = st.bits(key, old_p[:K] + _add(KEY, 1), *args[2:])
        assert not st.circuit.holds(bad[: st.lu], bad[st.lu:])


LEVEL = (113986, 202946)


def test_compiled_sizes(statements):
    assert sorted(W.MERKLE_REMOVE_SIZES) == [(4, 8, 1), (4, 8, 2), (8, 55, 1), (8, 55, 4)] and sorted(W.MERKLE_REMOVE_SPLIT_SIZES) == [(4, 8, 1), (8, 55, 1), (8, 55, 4)]
    for key, params in [((4, 8, 1), P19), ((4, 8, 2), P20), ((8, 55, 1), P19), ((8, 55, 4), P20)]:
        st = statements.get(key) or W.MerkleRemove(*key)
        cc = st.circuit.compile(params)
        kb, length, depth = key
        assert (cc.nwires, cc.nrows) == W.MERKLE_REMOVE_SIZES[key], key
        assert cc.lu == 512 + 8 * kb and len(cc.outputs) == 512 and len(cc.asserts) == 2
        assert cc.nwires - len(cc.program) == st.nin == 512 + 8 * kb + 16 * length + 514 * depth
    for key, params in [((4, 8, 1), P19), ((8, 55, 1), P19), ((8, 55, 4), P20)]:
        st = W.MerkleRemove(*key, joined=False)
        cc = st.circuit.compile(params)
        joined = W.MERKLE_REMOVE_SIZES[key]
        assert (cc.nwires, cc.nrows) == W.MERKLE_REMOVE_SPLIT_SIZES[key] == (joined[0] + 512, joined[1] + 768), key
        assert cc.lu == 1024 + 8 * key[0] and len(cc.outputs) == 1024 and cc.nwires - len(cc.program) == st.nin == 1024 + 8 * key[0] + 16 * key[1] + 514 * key[2]
    sizes = W.MERKLE_REMOVE_SIZES
    assert tuple(a - b for a, b in zip(sizes[(4, 8, 2)], sizes[(4, 8, 1)])) == LEVEL  # a level: MerkleInsert's
    assert tuple(a - b for a, b in zip(W.MERKLE_INSERT_SIZES[(8, 55, 4)], W.MERKLE_INSERT_SIZES[(8, 55, 1)])) == tuple(3 * x for x in LEVEL)
    assert sizes[(8, 55, 4)] == tuple(a + 3 * b for a, b in zip(sizes[(8, 55, 1)], LEVEL)) == (539690, 960334)
    assert sizes[(8, 55, 4)][0] <= P20.m - 1 and sizes[(8, 55, 4)][1] <= P20.d - 1
    with pytest.raises(C.CircuitError):
        statements[(4, 8, 1)].circuit.compile(P18)


def test_depth_five_does_not_fit_two_to_the_twenty():
    assert W.MERKLE_REMOVE_SIZES[(8, 55, 4)][1] + LEVEL[1] == 1163280 > P20.d - 1
    with pytest.raises(C.CircuitError) as e:
        W.MerkleRemove(8, 55, 5).circuit.compile(P20)
    assert "1163280" in str(e.value)


def test_argument_errors(statements):
    st = statements[(4, 8, 1)]
    for bad in [(0, 8, 1), (33, 66, 1), (4, 7, 1), (4, 8, 0), (4.0, 8, 1), (4, 8.0, 1), (4, 8, 1.0)]:
        with pytest.raises(C.CircuitError) as e:
            W.MerkleRemove(*bad)
        assert str(e.value).startswith("MerkleRemove: "), str(e.value)
    k, old_p, old_s, sibs_p, p, sibs_s, s = _witness(*_records(1))
    for bad in [(k[:3], old_p, old_s, sibs_p, p, sibs_s, s), (k + b"\0", old_p, old_s, sibs_p, p, sibs_s, s), (bytes(4), old_p, old_s, sibs_p, p, sibs_s, s),
                (b"\xff" * 4, old_p, old_s, sibs_p, p, sibs_s, s), (k, old_p[:7], old_s, sibs_p, p, sibs_s, s), (k, old_p, old_s + b"\0", sibs_p, p, sibs_s, s),
                (k, old_p, old_s, [], p, sibs_s, s), (k, old_p, old_s, sibs_p, p, [sibs_s[0][:31]], s), (k, old_p, old_s, sibs_p + sibs_p, p, sibs_s, s),
                (k, old_p, old_s, sibs_p, 2, sibs_s, s), (k, old_p, old_s, sibs_p, p, sibs_s, -1)]:
        with pytest.raises(C.CircuitError) as e:
            st.bits(*bad)
        assert str(e.value).startswith("MerkleRemove: "), str(e.value)
    root = bytes(range(32))
    for bad in [(root[:31], root, k), (root, root[:31], k), (root, root, k[:3]), (root, root, bytes(4)), (root, root, b"\xff" * 4), (root, root, root, root, k)]:
        with pytest.raises(C.CircuitError) as e:
            st.statement(*bad)
        assert str(e.value).startswith("MerkleRemove: "), str(e.value)
    assert len(st.statement(root, root[::-1], k)) == st.lu // 8


def test_indexed_remove():
    rec_p, rec_s = bytes([0x03, 0x40, 7, 8, 9]), bytes([0x40, 0x80, 1, 2, 3])
    idx, new = W.indexed_remove(rec_p, 5, rec_s, 2, key_bytes=1)
    assert idx == [5, 2] and new.dtype == np.uint8 and new.tolist() == [[0x03, 0x80, 7, 8, 9], [0, 0, 0, 0, 0]]
    idx, new = W.indexed_remove(bytes([0, 3, 0, 9]), 0, bytes([0, 9, 0xFF, 0xFF]), 1)  # key_bytes = half the length
    assert idx == [0, 1] and new.tolist() == [[0, 3, 0xFF, 0xFF], [0, 0, 0, 0]]
    for bad in [(bytes([0x03, 0x41, 7, 8, 9]), 5, rec_s, 2), (rec_p, 5, bytes([0x41, 0x80, 1, 2, 3]), 2),  # record_p[K:2K] != record_s[:K]
                (bytes([0x40, 0x40, 7, 8, 9]), 5, rec_s, 2), (bytes([0x41, 0x40, 7, 8, 9]), 5, rec_s, 2),  # p is not live
                (rec_p, 5, bytes([0x40, 0x40, 1, 2, 3]), 2), (rec_p, 5, bytes([0x40, 0x3F, 1, 2, 3]), 2),  # s is not live
                (rec_p, 2, rec_s, 2), (rec_p, -1, rec_s, 2), (rec_p, 5, rec_s[:4], 2)]:
        with pytest.raises(C.CircuitError) as e:
            W.indexed_remove(*bad, key_bytes=1)
        assert str(e.value).startswith("indexed_remove: "), str(e.value)
    for kb in (0, 3, 33, 1.0):
        with pytest.raises(C.CircuitError):
            W.indexed_remove(rec_p, 5, rec_s, 2, key_bytes=kb)


def test_model_removes_keep_the_invariant_and_undo_inserts():
    keys = [bytes([x]) for x in (0x80, 0x03, 0xFE)]
    table = W.indexed_records(keys, 3, length=5, payloads=[b"ab", b"cd", b"ef"])
    start = [r.tobytes() for r in table]
    model = RemoveModel(start, 1)
    root0 = model.root()
    batch = [0x40, 0x20, 0x60, 0x01]
    for x in batch:
        model.insert(bytes([x]), b"\x09")
    members = sorted([0x03, 0x80, 0xFE] + batch)
    full = list(model.records)
    # the inserted keys out again, in another order: adjacent members (0x20, 0x40, 0x60) both ways round
    for x in (0x40, 0x01, 0x60, 0x20):
        old = list(model.records)
        p, s, args = model.remove(bytes([x]))
        idx, new = W.indexed_remove(old[p], p, old[s], s, key_bytes=1)
        assert idx == [p, s] and [model.records[i] for i in idx] == [r.tobytes() for r in new]
        assert [r for i, r in enumerate(model.records) if i not in idx] == [r for i, r in enumerate(old) if i not in idx]
        members.remove(x)
        assert _invariant(np.array([list(r) for r in model.records], dtype=np.uint8), 1) == members
        assert model.levels[0] == [hashlib.sha256(r).digest() for r in model.records]
    assert model.records == start and model.root() == root0  # the round trip: bytes and root
    # ... and the original members, down to the empty set: the sentinel record alone is left, (00, FF)
    for x in (0x80, 0xFE, 0x03):
        model.remove(bytes([x]))
    assert model.records == [bytes([0, 0xFF, 0, 0, 0])] + [bytes(5)] * 7
    assert full != start
    assert model.own(b"\x03") is None and model.prev(b"\xff") == 0
