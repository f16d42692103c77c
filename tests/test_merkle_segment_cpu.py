"""CPU: words.MerkleSegment(levels), the statement of one level range of a deep Merkle transition, words.segment_levels, and segment 0 of an insert,
words.MerkleInsert(joined=False).

1. sizes: levels 1 and 2 are compiled and equal MERKLE_SEGMENT_SIZES and MerkleUpdate's formula; lu = 1024 with 512 given and 512 computed wires; at
   d = 2^20, m = 699 050 ten levels fit and eleven do not.
2. tops: tops_of(assign(bits(...))) equals tests/sha256_ref.py's merkle_root above the old and the new node at every index of levels 1 and 2; the row's
   layout; one bit flipped in a node changes that node's top alone, in a sibling both.
3. statement: statement(...) equals bits [0, 1024) of the assigned row, each quarter MerklePath.statement's bytes.
4. composition on a depth-3 reference tree with cuts [1], [2] and [1, 2]: MerkleUpdate(c_0) and every segment hold on the model's rows, their computed tops
   are the published nodes, and chain(nodes) gives the segments' statement bytes; a segment fed a wrong lower node computes tops that are not the
   published ones.
5. refusals: cuts, sizes, the index range, chain.
6. MerkleInsert(joined=False): the two compiled sizes, lu, the joined sizes unchanged; a correct witness with p and s in one depth-1 subtree of a depth-2
   table and in two; every defect of the joined statement alone -- those the middle roots caught now show as tops that are not the tree's; statement."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from merkle_insert_model import InsertModel
from merkle_segments_model import leaf_batch, segment_row_bytes
from test_merkle_absent_cpu import _add
from test_merkle_insert_cpu import _table

P17 = mf.Params(d=1 << 17, m=87381)
P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)

# the issue's figures: levels -> (wires, rows)
TABLE = {1: (58019, 103013), 2: (115012, 204486)}
SPLIT = {(4, 8, 1): (224776, 399885), (8, 55, 1): (226156, 401521), (8, 55, 4): (568114, 1010359)}


def _formula(levels):
    return 56993 * levels + 1026, 101473 * levels + 1540


def _fits(size, p):
    return size[0] <= p.m - 1 and size[1] <= p.d - 1


@pytest.fixture(scope="module")
def segments():
    out = {}
    for levels in (1, 2):
        st = W.MerkleSegment(levels)
        out[levels] = (st, st.circuit.compile(P18))
    return out


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("levels", [1, 2])
def test_compiled_sizes(segments, levels):
    st, cc = segments[levels]
    assert (cc.nwires, cc.nrows) == TABLE[levels] == W.MERKLE_SEGMENT_SIZES[levels] == _formula(levels) == W.MERKLE_UPDATE_SIZES[levels]
    assert st.lu == cc.lu == 1024 and len(cc.outputs) == 512 and len(cc.equal) == 512 and len(cc.asserts) == 0
    assert cc.nwires - len(cc.program) == st.nin == 1024 + 257 * levels and st.row_bytes == segment_row_bytes(levels)


def test_table_by_formula_and_capacity():
    for levels, size in W.MERKLE_SEGMENT_SIZES.items():
        assert size == _formula(levels), levels
    assert _fits(_formula(10), P20) and W.MERKLE_SEGMENT_SIZES[10] == (570956, 1016270)
    assert not _fits(_formula(11), P20)
    assert _fits(_formula(1), P17) and _fits(_formula(2), P18) and not _fits(_formula(2), P17)


# ------------------------------------------------------------------ 2. tops
def _tops(segments, levels, old, new, sibs, index):
    st, _ = segments[levels]
    bits = st.bits(old, new, sibs, index)
    assert bits.shape == (1024 + 257 * levels,) and bits.dtype == np.uint8 and not bits[512:1024].any()
    assert st.circuit.holds(bits[:1024], bits[1024:])
    row = st.circuit.assign(bits[:1024], bits[1024:], P18)
    return st.tops_of(row), row


@pytest.mark.parametrize("levels", [1, 2])
def test_tops_equal_reference_at_every_index(segments, levels):
    rng = np.random.default_rng(9100 + levels)
    old, new = rng.bytes(32), rng.bytes(32)
    sibs = [rng.bytes(32) for _ in range(levels)]
    seen = set()
    for index in range(1 << levels):
        (t_old, t_new), _ = _tops(segments, levels, old, new, sibs, index)
        assert t_old == ref.merkle_root(old, sibs, index), index
        assert t_new == ref.merkle_root(new, sibs, index), index
        seen |= {t_old, t_new}
    assert len(seen) == 2 << levels
    st, _ = segments[levels]
    bits = st.bits(old, new, sibs, (1 << levels) - 2)
    assert np.array_equal(bits[:512], W.pack(W.be_words(old + new)))
    assert np.array_equal(bits[1024: 1024 + 256 * levels], W.pack(W.be_words(b"".join(sibs))))
    assert bits[-levels:].tolist() == [0] + [1] * (levels - 1)
    # the packed row: old node as words | new node as words | 64 zero bytes | siblings as words | index bytes
    row = np.packbits(bits, bitorder="little").tobytes()
    swap = lambda d: b"".join(d[i: i + 4][::-1] for i in range(0, len(d), 4))  # noqa: E731
    assert row == swap(old) + swap(new) + bytes(64) + swap(b"".join(sibs)) + bytes([(1 << levels) - 2])


def _flip(b: bytes, bit: int) -> bytes:
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


def test_one_flipped_bit_changes_the_right_tops(segments):
    levels, index = 2, 2
    rng = np.random.default_rng(9200)
    old, new = rng.bytes(32), rng.bytes(32)
    sibs = [rng.bytes(32) for _ in range(levels)]
    (t_old, t_new), _ = _tops(segments, levels, old, new, sibs, index)
    (a_old, a_new), _ = _tops(segments, levels, _flip(old, 77), new, sibs, index)
    assert a_old != t_old and a_new == t_new and a_old == ref.merkle_root(_flip(old, 77), sibs, index)
    (b_old, b_new), _ = _tops(segments, levels, old, _flip(new, 200), sibs, index)
    assert b_old == t_old and b_new != t_new and b_new == ref.merkle_root(_flip(new, 200), sibs, index)
    for level in range(levels):
        other = list(sibs)
        other[level] = _flip(sibs[level], 5 + level)
        (c_old, c_new), _ = _tops(segments, levels, old, new, other, index)
        assert c_old != t_old and c_new != t_new, level
        assert (c_old, c_new) == (ref.merkle_root(old, other, index), ref.merkle_root(new, other, index))


# ------------------------------------------------------------------ 3. statement
def test_statement_is_bits_0_to_1024_of_the_row(segments):
    st, _ = segments[1]
    rng = np.random.default_rng(9300)
    old, new, sib = rng.bytes(32), rng.bytes(32), rng.bytes(32)
    (t_old, t_new), row = _tops(segments, 1, old, new, [sib], 1)
    stmt = st.statement(old, new, t_old, t_new)
    assert len(stmt) == 128 and stmt == bytes(row[:128]) == W.MerkleSegment.statement(bytearray(old), new, t_old, bytearray(t_new))
    assert stmt == b"".join(W.MerklePath.statement(x) for x in (old, new, t_old, t_new))
    assert st.statement(new, old, t_old, t_new) != stmt and st.statement(old, new, t_new, t_old) != stmt
    for k in range(4):
        for bad in (b"", old[:31], old + b"\0"):
            args = [old, new, t_old, t_new]
            args[k] = bad
            with pytest.raises(C.CircuitError):
                W.MerkleSegment.statement(*args)


# ------------------------------------------------------------------ 4. composition
@pytest.fixture(scope="module")
def composed():
    """a depth-3 tree and four sequential updates (a leaf twice, a sibling, a cousin) under each cut list: the model's rows, nodes and roots"""
    rng = np.random.default_rng(9400)
    leaves = [rng.bytes(32) for _ in range(8)]
    indices = [5, 4, 5, 1]
    new = [rng.bytes(32) for _ in indices]
    return {tuple(cuts): leaf_batch(leaves, indices, new, cuts)[:3] for cuts in ([1], [2], [1, 2])}


def _assigned(st, packed_row, params=P18):
    bits = np.unpackbits(packed_row, bitorder="little")[: st.nin]
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    return st.circuit.assign(bits[: st.lu], bits[st.lu:], params)


@pytest.mark.parametrize("cuts", [(1,), (2,), (1, 2)])
def test_segments_compose_on_a_depth_3_tree(segments, composed, cuts):
    rows, nodes, roots = composed[cuts]
    ranges = W.segment_levels(3, cuts)
    assert ranges == list(zip((0,) + cuts, cuts + (3,)))
    low = W.MerkleUpdate(cuts[0])
    for k in range(len(nodes)):
        pub = [(nodes[k, g, 0].tobytes(), nodes[k, g, 1].tobytes()) for g in range(len(cuts) + 1)]
        assert pub[-1] == (roots[k].tobytes(), roots[k + 1].tobytes())
        row = _assigned(low, rows[0][k])
        assert low.roots_of(row) == pub[0] and bytes(row[:64]) == W.MerkleUpdate.statement(*pub[0])
        stmts = W.MerkleSegment.chain(pub)
        assert len(stmts) == len(cuts)
        for g, (lo, hi) in enumerate(ranges[1:], start=1):
            st, _ = segments[hi - lo]
            row = _assigned(st, rows[g][k])
            assert st.tops_of(row) == pub[g] and bytes(row[:128]) == stmts[g - 1] == st.statement(*pub[g - 1], *pub[g])
    # adjacent updates chain: the new root of update k is the old root of update k + 1
    assert all(nodes[k, -1, 1].tobytes() == nodes[k + 1, -1, 0].tobytes() for k in range(len(nodes) - 1))


def test_a_wrong_lower_node_gives_other_tops(segments, composed):
    rows, nodes, _ = composed[(1,)]
    st, _ = segments[2]
    k = 2
    bits = np.unpackbits(rows[1][k], bitorder="little")[: st.nin].copy()
    other = np.unpackbits(rows[1][k - 1], bitorder="little")[:256]  # update k - 1's old node in place of update k's
    assert not np.array_equal(bits[:256], other)
    bits[:256] = other
    assert st.circuit.holds(bits[:1024], bits[1024:])  # the circuit computes tops, it asserts nothing: the STATEMENT is what differs
    t_old, t_new = st.tops_of(st.circuit.assign(bits[:1024], bits[1024:], P18))
    assert t_old != nodes[k, 1, 0].tobytes() and t_new == nodes[k, 1, 1].tobytes()


# ------------------------------------------------------------------ 5. refusals
def test_refusals(segments):
    for levels in (0, -1, 1.0, None):
        with pytest.raises(C.CircuitError):
            W.MerkleSegment(levels)
    for depth, cuts in [(3, []), (3, [0]), (3, [3]), (3, [2, 2]), (3, [2, 1]), (3, [1, 4]), (3, [1.0]), (20, [4, 12, 20])]:
        with pytest.raises(C.CircuitError):
            W.segment_levels(depth, cuts)
    assert W.segment_levels(20, [4, 12]) == [(0, 4), (4, 12), (12, 20)] and W.segment_levels(2, (1,)) == [(0, 1), (1, 2)]
    st, _ = segments[2]
    node, sibs = bytes(32), [bytes(32), bytes(32)]
    for old, new, s, index in [(node[:31], node, sibs, 0), (node, node + b"x", sibs, 0), (node, node, sibs[:1], 0), (node, node, sibs + [node], 0),
                               (node, node, [sibs[0], sibs[1][:31]], 0), (node, node, sibs, 4), (node, node, sibs, -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(old, new, s, index)
    assert st.bits(node, node, sibs, 3).shape == (1024 + 514,)
    with pytest.raises(C.CircuitError):
        W.MerkleSegment.chain([(node, node)])
    with pytest.raises(C.CircuitError):
        W.MerkleSegment.chain([(node, node), (node, node[:31])])


# ------------------------------------------------------------------ 6. MerkleInsert(joined=False)
@pytest.fixture(scope="module")
def split():
    st = W.MerkleInsert(4, 8, 1, joined=False)
    return st, st.circuit.compile(P19)


def test_split_insert_sizes(split):
    st, cc = split
    assert (cc.nwires, cc.nrows) == SPLIT[(4, 8, 1)] == W.MERKLE_INSERT_SPLIT_SIZES[(4, 8, 1)]
    assert st.lu == cc.lu == 1024 + 32 and len(cc.outputs) == 1024 and st.row_bytes == 128 + 4 + 24 + 64 + 1
    big = W.MerkleInsert(8, 55, 1, joined=False)
    cb = big.circuit.compile(P19)
    assert (cb.nwires, cb.nrows) == SPLIT[(8, 55, 1)] and big.lu == 1024 + 64
    assert W.MERKLE_INSERT_SPLIT_SIZES == SPLIT
    for key, (wires, rows) in SPLIT.items():
        assert (wires - 512, rows - 768) == W.MERKLE_INSERT_SIZES[key], key
    assert _fits(SPLIT[(8, 55, 4)], P20)
    # the joined statement is today's
    assert W.MERKLE_INSERT_SIZES == {(4, 8, 1): (224264, 399117), (8, 55, 1): (225644, 400753), (8, 16, 4): (566654, 1008643), (8, 55, 4): (567602, 1009591)}
    joined = W.MerkleInsert(4, 8, 1)
    assert joined.joined and joined.lu == 512 + 32 and W.MerkleInsert(4, 8, 1, joined=True).lu == 544
    cj = joined.circuit.compile(P19)
    assert (cj.nwires, cj.nrows) == W.MERKLE_INSERT_SIZES[(4, 8, 1)]
    with pytest.raises(C.CircuitError):
        joined.tops_of(bytes(200))


def _split_witness(k, s, public=None, stale=False, new_s=None, flip_p=0, flip_s=0):
    """the arguments of bits() of MerkleInsert(4, 8, 1, joined=False) for the insert of k into record p = 2 and slot s of the depth-2 table of
    test_merkle_insert_cpu._table, cut at level 1, and the four tops the TREE has: node p >> 1 of level 1 before and after p's update, node s >> 1 after
    p's update and after s's"""
    K, length = 4, 8
    _, _, records = _table((K, length, 2))
    m = InsertModel(records, K)
    p = 2
    old_p, sibs_p, before = m.records[p], m.siblings(p), m.siblings(s)
    x_p = m.levels[1][p >> 1]
    m.set(p, old_p[:K] + k + old_p[2 * K:])
    x_p2, x_s = m.levels[1][p >> 1], m.levels[1][s >> 1]
    old_s, sibs_s = m.records[s], before if stale else m.siblings(s)
    rec = (k + old_p[K: 2 * K]).ljust(length, b"\0")
    rec = new_s(rec) if new_s else rec
    m.set(s, rec)
    x_s2 = m.levels[1][s >> 1]
    args = (k if public is None else public, old_p, old_s, rec, sibs_p[:1], (p & 1) ^ flip_p, sibs_s[:1], (s & 1) ^ flip_s)
    return args, (x_p, x_p2, x_s, x_s2), m


def _split_run(st, args):
    bits = st.bits(*args)
    assert bits.shape == (st.nin,) == (st.lu + 24 * st.length + 514 * st.depth,) and not bits[:1024].any()
    holds = st.circuit.holds(bits[: st.lu], bits[st.lu:])
    row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P19)
    return holds, st.tops_of(row), row


@pytest.mark.parametrize("s", [3, 1])  # p = 2: s = 3 shares its depth-1 subtree, s = 1 lies in the other
def test_split_insert_holds_in_one_subtree_and_in_two(split, s):
    st, _ = split
    lo, hi, _ = _table((4, 8, 2))
    k = _add(lo, 5)
    args, tops, m = _split_witness(k, s)
    holds, got, row = _split_run(st, args)
    assert holds and got == tops and len(set(tops)) == (3 if s == 3 else 4)
    assert (tops[1] == tops[2]) == (s == 3)  # one subtree: s's chain starts where p's ended; two: X_s is the untouched other half
    assert st.statement(*tops, k) == bytes(row[: st.lu // 8]) == b"".join(W.MerklePath.statement(x) for x in tops) + k
    assert np.array_equal(st.bits(*args)[1024: st.lu], np.unpackbits(np.frombuffer(k, dtype=np.uint8), bitorder="little"))
    # the tree afterwards: s's node is X_s'; with two subtrees p's node stayed at X_p', and the two are the root's children
    assert m.levels[1][s >> 1] == tops[3]
    if s == 1:
        assert m.levels[1][1] == tops[1] and ref.merkle_parent(tops[3], tops[1]) == m.root()
    with pytest.raises(C.CircuitError):
        st.statement(tops[0], tops[3], k)
    with pytest.raises(C.CircuitError):
        st.statement(*tops, bytes(4))


def test_split_insert_each_defect_alone(split):
    st, _ = split
    lo, hi, _ = _table((4, 8, 2))
    k, K = _add(lo, 5), 4
    for s in (3, 1):
        assert _split_run(st, _split_witness(k, s)[0])[0]
        for bad in (lo, hi, _add(lo, -1), _add(hi, 1)):  # k == lo_p, k == hi_p, outside
            assert not _split_run(st, _split_witness(bad, s)[0])[0], bad.hex()
        flip_hi = lambda r: r[:K] + bytes([r[K] ^ 1]) + r[K + 1:]  # noqa: E731
        assert not _split_run(st, _split_witness(k, s, new_s=flip_hi)[0])[0]  # new_s.hi != old_p.hi
        assert not _split_run(st, _split_witness(_add(k, 1), s, public=k)[0])[0]  # new_s.lo != k
        assert _split_run(st, _split_witness(_add(k, 1), s)[0])[0]
    assert not _split_run(st, _split_witness(k, 2)[0])[0]  # s == p: old_s is p's record after its update, which is live
    assert not _split_run(st, _split_witness(k, 0)[0])[0]  # another live record
    # what the middle roots caught in the joined statement is now caught by the STATEMENT: the computed tops are not the tree's
    args, tops, _ = _split_witness(k, 3, stale=True)  # s's sibling (record p's leaf) from before p's update
    holds, got, _ = _split_run(st, args)
    assert holds and got[:2] == tops[:2] and got[2] != tops[2] and got[3] != tops[3]
    args, tops, _ = _split_witness(k, 3, flip_p=1)
    holds, got, _ = _split_run(st, args)
    assert holds and got[0] != tops[0] and got[1] != tops[1] and got[2:] == tops[2:]
    args, tops, _ = _split_witness(k, 1, flip_s=1)
    holds, got, _ = _split_run(st, args)
    assert holds and got[:2] == tops[:2] and got[2] != tops[2] and got[3] != tops[3]


def test_split_row_is_the_joined_row_behind_128_zero_bytes(split):
    st, _ = split
    lo, _, _ = _table((4, 8, 2))
    args, _, _ = _split_witness(_add(lo, 5), 1)
    packed = np.packbits(st.bits(*args), bitorder="little").tobytes()
    joined = np.packbits(W.MerkleInsert(4, 8, 1).bits(*args), bitorder="little").tobytes()
    assert len(packed) == st.row_bytes == len(joined) + 64 and packed == bytes(64) + joined and not any(joined[:64])
    assert hashlib.sha256(args[1]).digest() != hashlib.sha256(args[3]).digest()
