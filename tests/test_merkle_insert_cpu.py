"""CPU: words.MerkleInsert(key_bytes, length, depth) -- "key k was inserted, and that alone takes the tree from root R to root R'" -- on MerkleInsert(4, 8, 1)
and MerkleInsert(8, 21, 2), against the brute-force model of tests/merkle_insert_model.py (a list of records, hashlib leaves, ref_tree).

1. a correct witness holds, roots_of is the model's root before and after, statement(R, R', k) is bits [0, lu) of the assigned row.
2. each of these ALONE makes holds false: k == lo_p, k == hi_p, k below and above the range, a live old_s (another live record, and p's own record after its
   update: s == p), new_s.hi != old_p.hi, new_s.lo != k, the siblings of s taken from the tree BEFORE p's update, a flipped direction bit of p and of s.
3. a changed payload of new_s still holds, with another R'; the byte-order trap of tests/test_merkle_absent_cpu.py applies to k.
4. MERKLE_INSERT_SIZES is what compile counts for its four shapes, and the closed form in terms of the other size tables; (8, 55, 5) is refused at d = 2^20.
5. the argument errors.
6. inserts applied to a model table keep test_merkle_absent_cpu.py's brute-force invariant and are indexed_insert's two updates."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from merkle_insert_model import InsertModel
from test_merkle_absent_cpu import _add, _invariant

P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)
SHAPES = [(4, 8, 1), (8, 21, 2)]


@pytest.fixture(scope="module")
def statements():
    return {key: W.MerkleInsert(*key) for key in SHAPES}


def _table(key):
    """records of a table whose record p = 2^depth - 2 is (lo, hi) with room on both sides and between; the last slot is inert (lo == hi != 0), and at depth
    2 record 0 is the sentinel's (live) and record 1 another inert one (lo > hi)"""
    K, length, depth = key
    rng = np.random.default_rng(14100 + length)
    mid = rng.bytes(K - 2)
    lo, hi = bytes([0x40]) + mid + bytes([0x80]), bytes([0x41]) + mid + bytes([0x7F])
    records = [lo + hi + rng.bytes(length - 2 * K), hi + hi + rng.bytes(length - 2 * K)]
    if depth == 2:
        records = [bytes(K) + lo + rng.bytes(length - 2 * K), hi + lo + rng.bytes(length - 2 * K)] + records
    return lo, hi, records


def _witness(key, k, s=None, payload=b"\x5a", public=None, stale=False, new_s=None):
    """the arguments of bits() for the insert of k into record p = 2^depth - 2 and slot s (default: the last), built as the model builds them but with p and
    s forced and no range check; public: another key in the statement; stale: s's siblings from the tree before p's update; new_s: a function of new_s"""
    K, length, depth = key
    lo, hi, records = _table(key)
    m = InsertModel(records, K)
    p = (1 << depth) - 2
    s = (1 << depth) - 1 if s is None else s
    old_p, sibs_p, before = m.records[p], m.siblings(p), m.siblings(s)
    m.set(p, old_p[:K] + k + old_p[2 * K:])
    old_s, sibs_s = m.records[s], before if stale else m.siblings(s)
    rec = (k + old_p[K: 2 * K] + payload[: length - 2 * K]).ljust(length, b"\0")
    rec = new_s(rec) if new_s else rec
    return (k if public is None else public, old_p, old_s, rec, sibs_p, p, sibs_s, s)


def _holds(st, args):
    bits = st.bits(*args)
    assert bits.shape == (st.lu + 24 * st.length + 514 * st.depth,) == (st.nin,) and not bits[:512].any()
    return st.circuit.holds(bits[: st.lu], bits[st.lu:])


@pytest.mark.parametrize("key", SHAPES)
def test_a_correct_insert_holds(statements, key):
    st = statements[key]
    K, length, depth = key
    lo, hi, records = _table(key)
    assert st.lu == st.circuit.lu == 512 + 8 * K and st.row_bytes == 64 + K + 3 * length + 64 * depth + (2 * depth + 7) // 8
    model = InsertModel(records, K)
    k = _add(lo, 5)
    before = model.root()
    p, s, args = model.insert(k, b"\x5a"[: length - 2 * K])
    assert (p, s) == ((1 << depth) - 2, 1) and args == _witness(key, k, s=s)
    bits = st.bits(*args)
    assert np.array_equal(bits[512: st.lu], np.unpackbits(np.frombuffer(k, dtype=np.uint8), bitorder="little"))
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)
    assert st.roots_of(row) == (before, model.root()) and before != model.root()
    assert st.statement(before, model.root(), k) == bytes(row[: st.lu // 8]) == W.MerkleUpdate.statement(before, model.root()) + k
    # the packed row is the bits, eight to a byte
    assert len(np.packbits(bits, bitorder="little")) == st.row_bytes
    # another payload: holds, with another R'
    other = _witness(key, k, s=s, payload=b"\x5b")
    bits = st.bits(*other)
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    if length > 2 * K:
        got = st.roots_of(st.circuit.assign(bits[: st.lu], bits[st.lu:], P20))
        assert got[0] == before and got[1] != model.root()


@pytest.mark.parametrize("key", SHAPES)
def test_each_defect_alone_breaks_it(statements, key):
    st = statements[key]
    K, length, depth = key
    lo, hi, records = _table(key)
    k, p = _add(lo, 5), (1 << depth) - 2
    assert _holds(st, _witness(key, k))  # the last slot (lo == hi != 0) is as inert as the lowest
    for bad in (lo, hi, _add(lo, -1), _add(hi, 1)):  # k == lo_p, k == hi_p, outside
        assert not _holds(st, _witness(key, bad)), bad.hex()
    assert not _holds(st, _witness(key, k, s=p))  # s == p: old_s is p's record after its update, which is live
    if depth == 2:
        assert not _holds(st, _witness(key, k, s=0))  # another live record
        assert _holds(st, _witness(key, k, s=1))  # lo > hi: inert
    flip_hi = lambda r: r[:K] + bytes([r[K] ^ 1]) + r[K + 1:]  # noqa: E731
    assert not _holds(st, _witness(key, k, new_s=flip_hi))  # new_s.hi != old_p.hi
    assert not _holds(st, _witness(key, _add(k, 1), public=k))  # new_s.lo != k: the insert of k + 1, consistent but for the statement's key
    assert _holds(st, _witness(key, _add(k, 1)))
    assert not _holds(st, _witness(key, k, stale=True))  # s's siblings from the tree before p's update: the middle roots differ
    good = _witness(key, k)
    assert not _holds(st, good[:5] + (good[5] ^ 1,) + good[6:])  # a direction bit of p
    assert not _holds(st, good[:7] + (good[7] ^ 1,))  # ... of s
    if depth == 2:
        assert not _holds(st, good[:5] + (good[5] ^ 2,) + good[6:]) and not _holds(st, good[:7] + (good[7] ^ 2,))


def test_byte_order_of_the_key(statements):
    key = (4, 8, 1)
    st = statements[key]
    K = key[0]
    lo, hi, _ = _table(key)
    first_byte = bytes([hi[0]]) + lo[1:]  # differs from lo in byte 0 only and from hi in the last byte only (0x80 > 0x7F): above hi
    for k in (bytes([lo[0]]) + b"\xff" * (K - 1), bytes([hi[0]]) + bytes(K - 1), _add(lo, 1), _add(hi, -1)):
        assert _holds(st, _witness(key, k)), k.hex()
    for k in (first_byte, bytes([lo[0] - 1]) + b"\xff" * (K - 1), bytes([hi[0] + 1]) + bytes(K - 1)):
        assert not _holds(st, _witness(key, k)), k.hex()


def _formula(K, length, depth):
    """twice MerkleRecordUpdate(length, depth)'s sizes less 8 length - 56 K + 514 wires and 8 length - 120 K + 769 rows; MerkleRecordUpdate's from its own form"""
    message = W.SHA256_MESSAGE_SIZES[length]
    update = (56993 * depth + 1026, 101473 * depth + 1540)
    ru = (update[0] + 2 * message[0] - 1028, update[1] + 2 * message[1] - 1544)
    return 2 * ru[0] - 8 * length + 56 * K - 514, 2 * ru[1] - 8 * length + 120 * K - 769


def test_compiled_sizes(statements):
    assert sorted(W.MERKLE_INSERT_SIZES) == [(4, 8, 1), (8, 16, 4), (8, 55, 1), (8, 55, 4)]
    for key, params in [((4, 8, 1), P19), ((8, 55, 1), P19), ((8, 16, 4), P20), ((8, 55, 4), P20)]:
        st = statements.get(key) or W.MerkleInsert(*key)
        cc = st.circuit.compile(params)
        K, length, depth = key
        assert (cc.nwires, cc.nrows) == W.MERKLE_INSERT_SIZES[key], key
        assert cc.lu == 512 + 8 * K and len(cc.outputs) == 512 and len(cc.asserts) == 3
        assert cc.nwires - len(cc.program) == st.nin == 512 + 8 * K + 24 * length + 514 * depth
    ru = W.MERKLE_RECORD_UPDATE_SIZES[(55, 1)]
    assert W.MERKLE_INSERT_SIZES[(8, 55, 1)] == (2 * ru[0] - 440 + 448 - 514, 2 * ru[1] - 440 + 960 - 769) == _formula(8, 55, 1)
    assert W.MERKLE_INSERT_SIZES[(8, 55, 4)] == _formula(8, 55, 4)
    with pytest.raises(C.CircuitError):
        W.MerkleInsert(8, 55, 1).circuit.compile(mf.Params(d=1 << 18, m=174762))


def test_depth_five_does_not_fit_two_to_the_twenty():
    assert _formula(8, 55, 5)[1] == 1212537 > P20.d - 1
    with pytest.raises(C.CircuitError):
        W.MerkleInsert(8, 55, 5).circuit.compile(P20)


def test_argument_errors(statements):
    key = (4, 8, 1)
    st = statements[key]
    lo, hi, _ = _table(key)
    k = _add(lo, 5)
    for bad in [(0, 8, 1), (33, 66, 1), (4, 7, 1), (4, 8, 0), (4.0, 8, 1), (4, 8.0, 1), (4, 8, 1.0)]:
        with pytest.raises(C.CircuitError):
            W.MerkleInsert(*bad)
    key_, old_p, old_s, new_s, sibs_p, p, sibs_s, s = _witness(key, k)
    for bad in [(k[:3], old_p, old_s, new_s, sibs_p, p, sibs_s, s), (k + b"\0", old_p, old_s, new_s, sibs_p, p, sibs_s, s),
                (bytes(4), old_p, old_s, new_s, sibs_p, p, sibs_s, s), (b"\xff" * 4, old_p, old_s, new_s, sibs_p, p, sibs_s, s),
                (k, old_p[:7], old_s, new_s, sibs_p, p, sibs_s, s), (k, old_p, old_s + b"\0", new_s, sibs_p, p, sibs_s, s), (k, old_p, old_s, new_s[:7], sibs_p, p, sibs_s, s),
                (k, old_p, old_s, new_s, [], p, sibs_s, s), (k, old_p, old_s, new_s, sibs_p, p, [sibs_s[0][:31]], s), (k, old_p, old_s, new_s, sibs_p + sibs_p, p, sibs_s, s),
                (k, old_p, old_s, new_s, sibs_p, 2, sibs_s, s), (k, old_p, old_s, new_s, sibs_p, p, sibs_s, -1)]:
        with pytest.raises(C.CircuitError) as e:
            st.bits(*bad)
        assert str(e.value).startswith("MerkleInsert: "), str(e.value)
    root = bytes(range(32))
    for bad in [(root[:31], root, k), (root, root[:31], k), (root, root, k[:3]), (root, root, bytes(4)), (root, root, b"\xff" * 4)]:
        with pytest.raises(C.CircuitError) as e:
            st.statement(*bad)
        assert str(e.value).startswith("MerkleInsert: "), str(e.value)
    assert len(st.statement(root, root[::-1], k)) == st.lu // 8


def test_model_inserts_keep_the_invariant():
    keys = [bytes([x]) for x in (0x80, 0x03, 0xFE)]
    table = W.indexed_records(keys, 3, length=5, payloads=[b"ab", b"cd", b"ef"])
    model = InsertModel([r.tobytes() for r in table], 1)
    members = [0x03, 0x80, 0xFE]
    for x, want_p in ((0x40, 1), (0x20, 1), (0x60, 4), (0x01, 0)):  # 0x20 splits (0x03, 0x40); 0x60 falls into the record 0x40 went to
        old = list(model.records)
        p, s, args = model.insert(bytes([x]), b"\x09")
        idx, new = W.indexed_insert(old[p], p, bytes([x]), s, payload=b"\x09")
        assert p == want_p and idx == [p, s] and [model.records[i] for i in idx] == [r.tobytes() for r in new]
        assert [r for i, r in enumerate(model.records) if i not in idx] == [r for i, r in enumerate(old) if i not in idx]
        members = sorted(members + [x])
        assert _invariant(np.array([list(r) for r in model.records], dtype=np.uint8), 1) == members
        assert model.levels[0] == [hashlib.sha256(r).digest() for r in model.records]
    assert not any(not model.live(i) for i in range(8))  # full: 1 + 7 live records
    with pytest.raises(StopIteration):
        model.insert(b"\x50")
