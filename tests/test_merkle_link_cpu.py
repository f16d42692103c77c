"""CPU: words.MerkleLink(key_bytes, length, depth, reveal), the statement of one link of a range read, and words.indexed_range, against
tests/merkle_range_model.py.

1. sizes: (4, 8, 1, 0), (8, 55, 1, 8), (4, 9, 1, 1) and (4, 8, 2, 0) are compiled and equal MERKLE_LINK_SIZES, the issue's figures, the compiled
   MerkleRecord(length, depth) wire for wire and row for row, MERKLE_RECORD_SIZES where it has the entry, and the Sha256Message formula for one block.
2. lu = 256 + 8 P, nin = MerkleRecord's, bits() = MerkleRecord.bits(), the packed row = the model's record row byte for byte.
3. statement: the assigned row's statement bytes are MerkleRecord.statement(root) + record[:P]; shown_of reads the prefix; statement refuses lo >= hi.
4. a flipped public key bit computes another root.
5. chain on a depth-3 model table, for every lo <= hi of the probe set (members, members +- 1, 1, max - 1), with reveal 0 and 1: the model's statements.
6. chain refuses each broken inequality on its own, and a wrong `shown` count.
7. chain_cut with MerkleClimb.chain: segment 0 and the climbs hold on the model's cut rows and carry the statements.
8. indexed_range against the model's brute force on shuffled tables with garbage inert slots inside the range.
9. argument refusals."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import merkle_climb_model as CM
import merkle_range_model as M
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P18 = mf.Params(d=1 << 18, m=174762)

# the issue's figures: (key_bytes, length, depth, reveal) -> (wires, rows)
TABLE = {(4, 8, 1, 0): (56284, 99998), (8, 55, 1, 8): (56667, 100381), (4, 9, 1, 1): (56292, 100006)}
COMPILED = list(TABLE) + [(4, 8, 2, 0)]


@pytest.fixture(scope="module")
def links():
    out = {}
    for args in COMPILED:
        st = W.MerkleLink(*args)
        out[args] = (st, st.circuit.compile(P18))
    return out


@pytest.fixture(scope="module")
def records_compiled():
    return {(length, depth): W.MerkleRecord(length, depth).circuit.compile(P18) for length, depth in {(a[1], a[2]) for a in COMPILED}}


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("args", COMPILED)
def test_compiled_sizes(links, records_compiled, args):
    K, length, depth, reveal = args
    st, cc = links[args]
    rc = records_compiled[length, depth]
    assert (cc.nwires, cc.nrows) == W.MERKLE_LINK_SIZES[args] == (rc.nwires, rc.nrows) == TABLE.get(args, (rc.nwires, rc.nrows))
    assert W.MERKLE_RECORD_SIZES.get((length, depth), (cc.nwires, cc.nrows)) == (cc.nwires, cc.nrows)
    if length in W.SHA256_MESSAGE_SIZES:
        w, r = W.SHA256_MESSAGE_SIZES[length]
        assert (cc.nwires, cc.nrows) == (w + 28625 * depth, r + 50865 * depth)
    assert len(cc.outputs) == 256 and len(cc.equal) == 256 and len(cc.asserts) == 0  # no comparator, no equality row beyond the outputs'


def test_table_entries():
    assert set(W.MERKLE_LINK_SIZES) == set(COMPILED)
    assert W.MERKLE_LINK_SIZES[8, 55, 1, 8] == W.MERKLE_RECORD_SIZES[55, 1]
    a, b = W.MERKLE_LINK_SIZES[4, 8, 1, 0], W.MERKLE_LINK_SIZES[4, 8, 2, 0]
    assert (b[0] - a[0], b[1] - a[1]) == (28625, 50865)  # a level costs what MerklePath's does


# ------------------------------------------------------------------ 2. lu, nin, row
def _witness(rng, args, index=None):
    K, length, depth, reveal = args
    lo, hi = sorted((rng.bytes(K), rng.bytes(K)))
    if lo == hi:
        hi = (int.from_bytes(lo, "big") + 1).to_bytes(K, "big")
    record = lo + hi + rng.bytes(length - 2 * K)
    sibs = [rng.bytes(32) for _ in range(depth)]
    return record, sibs, int(rng.integers(1 << depth)) if index is None else index


@pytest.mark.parametrize("args", COMPILED)
def test_lu_nin_bits_and_row_are_merkle_records(links, records_compiled, args):
    K, length, depth, reveal = args
    st, cc = links[args]
    P = 2 * K + reveal
    rec = W.MerkleRecord(length, depth)
    assert st.shown_bytes == P and st.lu == cc.lu == 256 + 8 * P
    assert st.nin == rec.nin == cc.nwires - len(cc.program) == 256 + 8 * length + 257 * depth and st.row_bytes == rec.row_bytes
    rng = np.random.default_rng(11000 + length)
    for index in range(1 << depth):
        record, sibs, _ = _witness(rng, args)
        bits = st.bits(record, sibs, index)
        assert bits.dtype == np.uint8 and np.array_equal(bits, rec.bits(record, sibs, index))
        packed = np.packbits(bits, bitorder="little").tobytes()
        assert packed == CM.record_row(record, sibs, index) == bytes(32) + record + CM.swap(b"".join(sibs)) + bytes([index])


# ------------------------------------------------------------------ 3. statement, 4. a flipped public bit
def _assign(st, bits):
    assert st.circuit.holds(bits[: st.lu], bits[st.lu:])
    return st.circuit.assign(bits[: st.lu], bits[st.lu:], P18)


@pytest.mark.parametrize("args", COMPILED)
def test_statement_bytes(links, args):
    K, length, depth, reveal = args
    st, _ = links[args]
    P = 2 * K + reveal
    rng = np.random.default_rng(11100 + length)
    record, sibs, index = _witness(rng, args)
    row = _assign(st, st.bits(record, sibs, index))
    root = ref.merkle_root(hashlib.sha256(record).digest(), sibs, index)
    assert st.root_of(row) == root and st.shown_of(row) == record[:P]
    stmt = st.statement(root, record[:P])
    assert len(stmt) == 32 + P == st.lu // 8 and stmt == bytes(row[: 32 + P]) == W.MerkleRecord.statement(root) + record[:P]
    assert stmt == st.statement(bytearray(root), bytearray(record[:P]))
    for shown in (record[:K] + record[:K] + record[2 * K: P], record[K: 2 * K] + record[:K] + record[2 * K: P]):  # lo == hi, lo > hi
        with pytest.raises(C.CircuitError, match="not a live record"):
            st.statement(root, shown)
    for shown in (record[: P - 1], record[:P] + b"x", b""):
        with pytest.raises(C.CircuitError):
            st.statement(root, shown)
    with pytest.raises(C.CircuitError):
        st.statement(root[:31], record[:P])


def test_a_flipped_public_key_bit_computes_another_root(links):
    args = (4, 9, 1, 1)
    st, _ = links[args]
    rng = np.random.default_rng(11200)
    record, sibs, index = _witness(rng, args)
    good = bytes(_assign(st, st.bits(record, sibs, index))[: st.lu // 8])
    for bit in (0, 31, 32, 63, 64, 71):  # both keys' ends and the revealed byte's
        bits = st.bits(record, sibs, index).copy()
        bits[256 + bit] ^= 1
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P18)  # the circuit computes a root, it asserts nothing: the STATEMENT differs
        assert st.root_of(row) != st.root_of(good) and bytes(row[:32]) != good[:32]
        flipped = bytearray(record)
        flipped[bit // 8] ^= 1 << (bit % 8)
        assert st.shown_of(row) == bytes(flipped[:9])
        assert st.root_of(row) == ref.merkle_root(hashlib.sha256(bytes(flipped)).digest(), sibs, index)


# ------------------------------------------------------------------ 5. chain
@pytest.fixture(scope="module")
def tables():
    """depth-3 model tables by reveal: 5 members in shuffled slots, 2 garbage inert slots; (4, 8) and (4, 9) records"""
    out = {}
    for reveal in (0, 1):
        table, members = M.make_table(np.random.default_rng(11300 + reveal), 4, 8 + reveal, 3, 5)
        out[reveal] = (table, members, CM.ClimbModel([hashlib.sha256(bytes(r)).digest() for r in table]))
    return out


def _claim(table, K, reveal, order):
    """(keys, shown) of the links `order` as a prover publishes them"""
    recs = [bytes(table[s]) for s in order]
    keys = [recs[0][:K]] + [r[K: 2 * K] for r in recs]
    return keys, ([r[2 * K: 2 * K + reveal] for r in recs] if reveal else None)


@pytest.mark.parametrize("reveal", [0, 1])
def test_chain_gives_the_models_statements_for_every_probe_pair(tables, reveal):
    table, members, model = tables[reveal]
    K = 4
    st = W.MerkleLink(K, 8 + reveal, 3, reveal)
    probes = M.probes(members, K)
    assert len(probes) >= 12
    sizes = set()
    for i, lo in enumerate(probes):
        for hi in probes[i:]:
            order = M.links(table, K, lo, hi)
            assert M.status(table, K, lo, hi, order) == 0
            inside = [m for m in members if lo <= m <= hi]
            keys, shown = _claim(table, K, reveal, order)
            assert keys[1:-1] == inside and len(order) == len(inside) + 1
            got = st.chain(model.root(), lo, hi, keys, shown)
            assert got == M.statements([model.root()] * len(order), table, order, K, reveal), (lo, hi)
            sizes.add(len(got))
    assert sizes == {1, 2, 3, 4, 5, 6}  # from the absence of a whole interval to the whole set


def test_chain_refuses_each_broken_inequality(tables):
    table, members, model = tables[1]
    K, root = 4, model.root()
    st = W.MerkleLink(K, 9, 3, 1)
    lo, hi = members[1], members[3]
    order = M.links(table, K, lo, hi)
    keys, shown = _claim(table, K, 1, order)
    assert keys == members[0:5] and len(st.chain(root, lo, hi, keys, shown)) == 4

    def dec(k):
        return (int.from_bytes(k, "big") - 1).to_bytes(K, "big")

    def inc(k):
        return (int.from_bytes(k, "big") + 1).to_bytes(K, "big")

    def refused(lo_, hi_, keys_, shown_=shown, match=None):
        with pytest.raises(C.CircuitError, match=match):
            st.chain(root, lo_, hi_, keys_, shown_)

    refused(keys[0], hi, keys, match="p < lo")                                            # p >= lo
    refused(dec(keys[0]), hi, keys, match="p < lo")
    refused(inc(lo), hi, keys, match="lo <= k_1")                                     # k_1 < lo
    refused(lo, hi, [keys[0], keys[2], keys[1], keys[3], keys[4]], match="ascending")     # an unsorted pair
    refused(lo, hi, [keys[0], keys[1], keys[1], keys[3], keys[4]], match="ascending")     # a duplicate
    refused(lo, dec(hi), keys, match="k_n <= hi")                                         # k_n > hi
    refused(lo, keys[4], keys, match="hi < s")                                            # s <= hi
    refused(lo, inc(keys[4]), keys, match="hi < s")
    refused(hi, lo, keys)                                                                 # lo > hi
    refused(lo, hi, keys, shown[:-1], match="one shown")                                  # a wrong shown count
    refused(lo, hi, keys, shown + [b"x"], match="one shown")
    refused(lo, hi, keys, None, match="one shown")
    refused(lo, hi, keys, [b"xx"] + shown[1:])
    refused(lo, hi, keys[:1])
    refused(lo, hi, [keys[0], keys[1][:3]] + keys[2:])
    refused(lo[:3], hi, keys)
    with pytest.raises(C.CircuitError, match="no shown"):
        W.MerkleLink(K, 9, 3, 0).chain(root, lo, hi, keys, shown)
    # n = 0, the absence of a whole interval: p < lo <= hi < s
    a, b = inc(members[2]), dec(members[3])
    assert len(st.chain(root, a, b, [members[2], members[3]], [b"p"])) == 1
    refused(members[2], b, [members[2], members[3]], [b"p"], match="p < lo")
    refused(a, members[3], [members[2], members[3]], [b"p"], match="hi < s")
    # a claimed result that omits k_2 is consistent on its face: chain accepts it, and its merged link is no record of the table
    short = [keys[0], keys[1], keys[3], keys[4]]
    merged = st.chain(root, lo, hi, short, [shown[0], shown[1], shown[3]])
    honest = st.chain(root, lo, hi, keys, shown)
    assert len(merged) == 3 and merged[0] == honest[0] and merged[2] == honest[3] and merged[1] not in honest
    assert all(bytes(r)[: 2 * K] != keys[1] + keys[3] for r in table)


# ------------------------------------------------------------------ 7. chain_cut
@pytest.mark.parametrize("cuts", [(1,), (2,), (1, 2)])
def test_chain_cut_with_the_climbs(tables, cuts):
    table, members, _ = tables[1]
    K, reveal = 4, 1
    lo, hi = M.probes(members, K)[0], members[2]
    rows, nodes, index, keys, status, model = M.range_segments(table, K, lo, hi, cuts)
    assert status == 0 and len(index) == 4 and nodes.shape == (4, len(cuts) + 1, 32)
    low = W.MerkleLink(K, 9, cuts[0], reveal)
    claim, shown = _claim(table, K, reveal, index)
    assert claim == [keys[0, 0].tobytes()] + [k.tobytes() for k in keys[:, 1]]
    stmts = low.chain_cut(nodes[:, 0], lo, hi, claim, shown)
    assert stmts == M.statements(nodes[:, 0], table, index, K, reveal)
    climbs = {levels: W.MerkleClimb(levels) for levels in {b - a for a, b in W.segment_levels(3, cuts)[1:]}}
    for i in range(4):
        bits = np.unpackbits(rows[0][i], bitorder="little")[: low.nin]
        row = _assign(low, bits)
        assert bytes(row[: low.lu // 8]) == stmts[i] and low.root_of(row) == nodes[i, 0].tobytes() == model.node(int(index[i]), cuts[0])
        upper = W.MerkleClimb.chain(nodes[i])
        assert nodes[i, -1].tobytes() == model.root()
        for g, (a, b) in enumerate(W.segment_levels(3, cuts)[1:], start=1):
            st = climbs[b - a]
            cb = np.unpackbits(rows[g][i], bitorder="little")[: st.nin]
            assert bytes(_assign(st, cb)[:64]) == upper[g - 1]
    with pytest.raises(C.CircuitError, match="one level-c_0 node per link"):
        low.chain_cut(nodes[:3, 0], lo, hi, claim, shown)


# ------------------------------------------------------------------ 8. indexed_range
@pytest.mark.parametrize("K,length,depth,nmembers", [(1, 2, 4, 9), (4, 8, 3, 5), (5, 13, 4, 11), (8, 55, 5, 20), (32, 64, 4, 13)])
def test_indexed_range_against_brute_force(K, length, depth, nmembers):
    rng = np.random.default_rng(11400 + K)
    table, members = M.make_table(rng, K, length, depth, nmembers, garbage=(1 << depth) - nmembers - 1)
    probes = M.probes(members, K)
    seen = set()
    pairs = [(probes[i], probes[j]) for i in range(0, len(probes), 2) for j in range(i, len(probes), 3)] + [(probes[0], probes[-1])]
    for lo, hi in pairs:
        got = W.indexed_range(table, K, lo, hi)
        assert got == M.links(table, K, lo, hi) and all(isinstance(s, int) for s in got)
        assert M.status(table, K, lo, hi, got) == 0 and len(got) == 1 + sum(lo <= m <= hi for m in members)
        seen.add(len(got))
    assert max(seen) == nmembers + 1 and len(seen) > 3
    # a malformed table: a duplicated lo breaks the tie by slot
    dup = table.copy()
    live = [s for s in range(len(dup)) if bytes(dup[s, :K]) < bytes(dup[s, K: 2 * K])]
    inert = [s for s in range(len(dup)) if s not in live]
    dup[inert[0]] = dup[live[2]]
    lo, hi = probes[0], probes[-1]
    got = W.indexed_range(dup, K, lo, hi)
    assert got == M.links(dup, K, lo, hi) and len(got) == nmembers + 2
    at = got.index(min(inert[0], live[2]))
    assert got[at + 1] == max(inert[0], live[2])


# ------------------------------------------------------------------ 9. refusals
def test_argument_refusals():
    for args in [(0, 8, 1), (33, 80, 1), (4, 7, 1), (4, 8, 0), (4, 8, 1, -1), (4, 8, 1, 1), (4, 9, 1, 2), (4.0, 8, 1), (4, 8, None), (4, 8, 1, "1")]:
        with pytest.raises(C.CircuitError):
            W.MerkleLink(*args)
    st = W.MerkleLink(4, 9, 1, 1)
    assert (st.key_bytes, st.length, st.depth, st.reveal, st.shown_bytes) == (4, 9, 1, 1, 9)
    record, sib = bytes(4) + b"\0\0\0\1" + b"p", bytes(32)
    for r, s, index in [(record[:8], [sib], 0), (record + b"x", [sib], 0), (record, [], 0), (record, [sib, sib], 0), (record, [sib[:31]], 0), (record, [sib], 2),
                        (record, [sib], -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(r, s, index)
    assert st.bits(record, [sib], 1).shape == (256 + 72 + 257,)
    table = np.zeros((8, 8), dtype=np.uint8)
    for t, K, lo, hi in [(table, 4, bytes(4), b"\0\0\0\2"), (table, 4, b"\0\0\0\1", b"\xff" * 4), (table, 4, b"\0\0\0\2", b"\0\0\0\1"), (table, 4, b"\1", b"\2"),
                         (table, 5, b"\0\0\0\0\1", b"\0\0\0\0\2"), (table, 0, b"", b""), (table.astype(np.uint32), 4, b"\0\0\0\1", b"\0\0\0\2"),
                         (table[0], 4, b"\0\0\0\1", b"\0\0\0\2")]:
        with pytest.raises(C.CircuitError):
            W.indexed_range(t, K, lo, hi)
    assert W.indexed_range(table, 4, b"\0\0\0\1", b"\0\0\0\2") == []
