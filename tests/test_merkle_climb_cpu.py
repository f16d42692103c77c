"""CPU: words.MerkleClimb(levels), the statement of one level range of a deep Merkle READ, against tests/merkle_climb_model.py.

1. sizes: levels 1 and 2 are compiled and equal MERKLE_CLIMB_SIZES, the issue's figures, MerklePath's table and its formula; lu = 512 with 256 given and
   256 computed wires; every listed entry of the table follows the formula.
2. capacity, by wires <= m - 1 and rows <= d - 1: 20 levels fit d = 2^20, m = 699 050 and 21 do not; 2 fit d = 2^17, m = 87 381 and 3 do not; 10 fit d = 2^19.
3. tops: top_of(assign(bits(...))) equals tests/sha256_ref.py's merkle_root at every index of levels 1 and 2.
4. row bytes: the packed row, byte for byte, is the model's (node as words | 32 zero bytes | siblings as words | index bytes): 97 and 129 bytes.
5. statement: statement(node, top) equals bits [0, 512) of the assigned row, each half MerklePath.statement's.
6. composition on a depth-3 tree with cuts [1], [2] and [1, 2], segment 0 being MerklePath(c_0), MerkleRecord(8, c_0) and MerkleAbsent(4, 8, c_0): segment 0
   and every climb hold on the model's rows, their computed tops are the model's nodes, and chain(nodes) gives the statement bytes.
7. a wrong lower node computes another top, and the statement catches it; so does a flipped direction bit.
8. refusals: levels, bits, statement, chain."""
import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import merkle_climb_model as M
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P17 = mf.Params(d=1 << 17, m=87381)
P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)

# the issue's figures: levels -> (wires, rows)
TABLE = {1: (29139, 51637), 2: (57764, 102502), 3: (86389, 153367)}
CUTS = [(1,), (2,), (1, 2)]
K, LENGTH = 4, 8


def _formula(levels):
    return 28625 * levels + 514, 50865 * levels + 772


def _fits(size, p):
    return size[0] <= p.m - 1 and size[1] <= p.d - 1


@pytest.fixture(scope="module")
def climbs():
    out = {}
    for levels in (1, 2):
        st = W.MerkleClimb(levels)
        out[levels] = (st, st.circuit.compile(P18))
    return out


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("levels", [1, 2])
def test_compiled_sizes(climbs, levels):
    st, cc = climbs[levels]
    assert (cc.nwires, cc.nrows) == TABLE[levels] == W.MERKLE_CLIMB_SIZES[levels] == _formula(levels) == W.MERKLE_PATH_SIZES[levels]
    assert st.lu == cc.lu == 512 and len(cc.outputs) == 256 and len(cc.equal) == 256 and len(cc.asserts) == 0
    assert cc.nwires - len(cc.program) == st.nin == 512 + 257 * levels and st.row_bytes == M.climb_row_bytes(levels)


def test_table_by_formula():
    assert set(W.MERKLE_CLIMB_SIZES) >= {1, 2}
    for levels, size in W.MERKLE_CLIMB_SIZES.items():
        assert size == _formula(levels), levels
        assert TABLE.get(levels, size) == size and W.MERKLE_PATH_SIZES.get(levels, size) == size, levels


# ------------------------------------------------------------------ 2. capacity
def test_capacity():
    assert _formula(20) == (573014, 1018072) == W.MERKLE_PATH_SIZES[20]
    assert _fits(_formula(20), P20) and not _fits(_formula(21), P20)
    assert _fits(_formula(2), P17) and not _fits(_formula(3), P17)
    assert _fits(_formula(10), P19)


# ------------------------------------------------------------------ 3. tops, 4. row bytes
def _top(climbs, levels, node, sibs, index):
    st, _ = climbs[levels]
    bits = st.bits(node, sibs, index)
    assert bits.shape == (512 + 257 * levels,) and bits.dtype == np.uint8 and not bits[256:512].any()
    assert st.circuit.holds(bits[:512], bits[512:])
    row = st.circuit.assign(bits[:512], bits[512:], P18)
    return st.top_of(row), row


@pytest.mark.parametrize("levels", [1, 2])
def test_tops_equal_reference_at_every_index_and_row_bytes(climbs, levels):
    rng = np.random.default_rng(9500 + levels)
    node = rng.bytes(32)
    sibs = [rng.bytes(32) for _ in range(levels)]
    st, _ = climbs[levels]
    seen = set()
    for index in range(1 << levels):
        top, _ = _top(climbs, levels, node, sibs, index)
        assert top == ref.merkle_root(node, sibs, index), index
        seen.add(top)
        packed = np.packbits(st.bits(node, sibs, index), bitorder="little").tobytes()
        assert len(packed) == st.row_bytes == {1: 97, 2: 129}[levels]
        assert packed == M.climb_row(node, sibs, index) == M.swap(node) + bytes(32) + M.swap(b"".join(sibs)) + bytes([index]), index
    assert len(seen) == 1 << levels
    bits = st.bits(node, sibs, (1 << levels) - 2)
    assert np.array_equal(bits[:256], W.pack(W.be_words(node)))
    assert np.array_equal(bits[512: 512 + 256 * levels], W.pack(W.be_words(b"".join(sibs))))
    assert bits[-levels:].tolist() == [0] + [1] * (levels - 1)


# ------------------------------------------------------------------ 5. statement
def test_statement_is_bits_0_to_512_of_the_row(climbs):
    st, _ = climbs[1]
    rng = np.random.default_rng(9600)
    node, sib = rng.bytes(32), rng.bytes(32)
    top, row = _top(climbs, 1, node, [sib], 1)
    stmt = st.statement(node, top)
    assert len(stmt) == 64 and stmt == bytes(row[:64]) == W.MerkleClimb.statement(bytearray(node), bytearray(top))
    assert stmt == W.MerklePath.statement(node) + W.MerklePath.statement(top)
    assert st.statement(top, node) != stmt
    for k in range(2):
        for bad in (b"", node[:31], node + b"\0"):
            args = [node, top]
            args[k] = bad
            with pytest.raises(C.CircuitError):
                W.MerkleClimb.statement(*args)


# ------------------------------------------------------------------ 6. composition
@pytest.fixture(scope="module")
def table():
    """a depth-3 indexed table of (4, 8) records in shuffled positions: five members, the sentinel record and two inert slots"""
    rng = np.random.default_rng(9700)
    members = sorted({rng.bytes(K) for _ in range(5)})
    keys = np.frombuffer(b"".join(members), dtype=np.uint8).reshape(len(members), K)
    records = [r.tobytes() for r in W.indexed_records(keys, 3, length=LENGTH)]
    records = [records[int(i)] for i in rng.permutation(8)]
    return records, members


@pytest.fixture(scope="module")
def lows():
    """segment 0's statements by (kind, c_0), built once"""
    out = {}
    for c0 in (1, 2):
        out["path", c0] = W.MerklePath(c0)
        out["record", c0] = W.MerkleRecord(LENGTH, c0)
        out["absent", c0] = W.MerkleAbsent(K, LENGTH, c0)
    return out


def _assigned(st, packed_row, holds=True):
    bits = np.unpackbits(np.asarray(packed_row, dtype=np.uint8), bitorder="little")[: st.nin]
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:]) == holds
    return st.circuit.assign(bits[: st.lu], bits[st.lu:], P18)


def _check_upper(climbs, rows, nodes, cuts, k):
    """every climb of statement k holds, computes the model's node and carries chain's statement bytes"""
    pub = [nodes[k, g].tobytes() for g in range(len(cuts) + 1)]
    stmts = W.MerkleClimb.chain(pub)
    assert len(stmts) == len(cuts)
    for g, (lo, hi) in enumerate(W.segment_levels(3, cuts)[1:], start=1):
        st, _ = climbs[hi - lo]
        row = _assigned(st, rows[g][k])
        assert st.top_of(row) == pub[g] and bytes(row[:64]) == stmts[g - 1] == st.statement(pub[g - 1], pub[g]), (k, g)
    return pub


@pytest.mark.parametrize("cuts", CUTS)
def test_paths_compose_on_a_depth_3_tree(climbs, lows, cuts):
    rng = np.random.default_rng(9800)
    model = M.ClimbModel([rng.bytes(32) for _ in range(8)])
    indices = [5, 0, 7, 2]
    rows, nodes = M.path_segments(model, indices, cuts)
    assert W.segment_levels(3, cuts) == M.ranges(3, cuts)
    low = lows["path", cuts[0]]
    assert [r.shape[1] for r in rows] == [low.row_bytes] + [M.climb_row_bytes(hi - lo) for lo, hi in M.ranges(3, cuts)[1:]]
    for k, i in enumerate(indices):
        pub = _check_upper(climbs, rows, nodes, cuts, k)
        assert pub[-1] == model.root() and pub[0] == model.node(i, cuts[0])
        row = _assigned(low, rows[0][k])
        assert low.root_of(row) == pub[0] and bytes(row[:32]) == W.MerklePath.statement(pub[0])
        # the segments' tails, one behind the other, are the uncut row's siblings
        whole = M.path_row(model.levels[0][i], model.siblings(i), i)
        assert b"".join(bytes(r[k][64: 64 + 32 * (hi - lo)]) for r, (lo, hi) in zip(rows, M.ranges(3, cuts))) == whole[64: 64 + 96]


@pytest.mark.parametrize("cuts", CUTS)
def test_records_compose_on_a_depth_3_tree(climbs, lows, table, cuts):
    records, _ = table
    indices = [3, 6, 1]
    rows, nodes, model = M.record_segments(records, indices, cuts)
    low = lows["record", cuts[0]]
    for k, i in enumerate(indices):
        pub = _check_upper(climbs, rows, nodes, cuts, k)
        assert pub[-1] == model.root()
        row = _assigned(low, rows[0][k])
        assert low.root_of(row) == pub[0] and bytes(row[:32]) == W.MerkleRecord.statement(pub[0])


@pytest.mark.parametrize("cuts", CUTS)
def test_absent_composes_on_a_depth_3_tree(climbs, lows, table, cuts):
    records, members = table
    rng = np.random.default_rng(9900)
    queries = [rng.bytes(K) for _ in range(3)] + [members[2]]
    rows, nodes, index, status, model = M.absent_segments(records, K, queries, cuts)
    assert status.tolist() == [0, 0, 0, 1] and len(set(index.tolist())) > 1
    low = lows["absent", cuts[0]]
    for k, q in enumerate(queries):
        pub = _check_upper(climbs, rows, nodes, cuts, k)  # the upper segments of a present key's record hold too
        assert pub[-1] == model.root()
        row = _assigned(low, rows[0][k], holds=status[k] == 0)
        assert low.root_of(row) == pub[0]
        assert bytes(row[: low.lu // 8]) == low.statement(pub[0], q) == W.MerklePath.statement(pub[0]) + q


# ------------------------------------------------------------------ 7. defects
def test_a_wrong_lower_node_and_a_flipped_direction_give_other_tops(climbs):
    rng = np.random.default_rng(10000)
    model = M.ClimbModel([rng.bytes(32) for _ in range(8)])
    rows, nodes = M.path_segments(model, [5, 3], (1,))
    st, _ = climbs[2]
    good = st.statement(nodes[0, 0].tobytes(), nodes[0, 1].tobytes())
    assert bytes(_assigned(st, rows[1][0])[:64]) == good
    # statement 1's lower node under statement 0's siblings and directions
    bits = np.unpackbits(rows[1][0], bitorder="little")[: st.nin].copy()
    other = np.unpackbits(rows[1][1], bitorder="little")[:256]
    assert not np.array_equal(bits[:256], other)
    bits[:256] = other
    assert st.circuit.holds(bits[:512], bits[512:])  # the circuit computes a top, it asserts nothing: the STATEMENT is what differs
    row = st.circuit.assign(bits[:512], bits[512:], P18)
    assert st.top_of(row) != model.root() and bytes(row[:64]) != good
    assert bytes(row[:64]) != st.statement(nodes[1, 0].tobytes(), model.root())  # nor does it prove the other node under the root
    # one direction bit flipped
    for level in range(2):
        bits = np.unpackbits(rows[1][0], bitorder="little")[: st.nin].copy()
        bits[512 + 512 + level] ^= 1
        row = st.circuit.assign(bits[:512], bits[512:], P18)
        index = (5 >> 1) ^ (1 << level)
        assert st.top_of(row) == ref.merkle_root(nodes[0, 0].tobytes(), model.siblings(5, 1, 3), index) != model.root(), level
        assert bytes(row[:32]) == good[:32] and bytes(row[:64]) != good


# ------------------------------------------------------------------ 8. refusals
def test_refusals(climbs):
    for levels in (0, -1, 1.0, None, "2"):
        with pytest.raises(C.CircuitError):
            W.MerkleClimb(levels)
    st, _ = climbs[2]
    node, sibs = bytes(32), [bytes(32), bytes(32)]
    for x, s, index in [(node[:31], sibs, 0), (node + b"x", sibs, 0), (node, sibs[:1], 0), (node, sibs + [node], 0), (node, [sibs[0], sibs[1][:31]], 0),
                        (node, sibs, 4), (node, sibs, -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(x, s, index)
    assert st.bits(node, sibs, 3).shape == (512 + 514,)
    for bad in ([], [node], [node, node[:31]], [node + b"x", node], [node, node, b""]):
        with pytest.raises(C.CircuitError):
            W.MerkleClimb.chain(bad)
    assert W.MerkleClimb.chain([node, node]) == [bytes(64)] and len(W.MerkleClimb.chain([node] * 4)) == 3
    assert W.MerkleClimb.chain(np.zeros((3, 32), dtype=np.uint8)) == [bytes(64)] * 2
