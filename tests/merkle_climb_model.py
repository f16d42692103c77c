"""A pure-Python model of cut READ rows and nodes (words.MerkleClimb, MerkleTree.path_segments / record_segments / absent_segments) for
tests/test_merkle_climb_cpu.py and tests/test_gpu_merkle_climb.py, over tests/sha256_ref.py alone: the tree by merkle_parent, every row put together byte
by byte from the layout of csrc/merkle_rows.hpp -- no statement's bits() enters it, so the CPU test can hold bits() against it."""
import hashlib

import numpy as np

import sha256_ref as ref

NONE = 0xFFFFFFFF


def swap(digests: bytes) -> bytes:
    """digest bytes as the rows hold them: every big-endian word as a native little-endian uint32"""
    return b"".join(digests[i: i + 4][::-1] for i in range(0, len(digests), 4))


def ranges(depth, cuts):
    edges = [0] + [int(c) for c in cuts] + [depth]
    assert all(a < b for a, b in zip(edges, edges[1:]))
    return list(zip(edges, edges[1:]))


def tail(siblings, index, levels) -> bytes:
    """`levels` siblings as words, then ceil(levels / 8) bytes of the index inside the segment's subtree"""
    assert len(siblings) == levels and 0 <= index < 1 << levels
    return swap(b"".join(siblings)) + index.to_bytes((levels + 7) // 8, "little")


def climb_row_bytes(levels):
    return 64 + 32 * levels + (levels + 7) // 8


def climb_row(node, siblings, index) -> bytes:
    """words.MerkleClimb(levels): the node as words | 32 zero bytes | the tail"""
    return swap(node) + bytes(32) + tail(siblings, index, len(siblings))


def path_row(leaf, siblings, index) -> bytes:
    """words.MerklePath(depth): 32 zero bytes | the leaf as words | the tail"""
    return bytes(32) + swap(leaf) + tail(siblings, index, len(siblings))


def record_row(record, siblings, index) -> bytes:
    """words.MerkleRecord(length, depth): 32 zero bytes | the record | the tail"""
    return bytes(32) + bytes(record) + tail(siblings, index, len(siblings))


def absent_row(key, record, siblings, index) -> bytes:
    """words.MerkleAbsent(key_bytes, length, depth): 32 zero bytes | the key | the record | the tail"""
    return bytes(32) + bytes(key) + bytes(record) + tail(siblings, index, len(siblings))


class ClimbModel:
    """the tree over 2^depth leaves of 32 bytes, level by level"""

    def __init__(self, leaves):
        self.levels = [[bytes(x) for x in leaves]]
        while len(self.levels[-1]) > 1:
            cur = self.levels[-1]
            self.levels.append([ref.merkle_parent(cur[j], cur[j + 1]) for j in range(0, len(cur), 2)])
        self.depth = len(self.levels) - 1
        assert len(self.levels[0]) == 1 << self.depth

    def root(self):
        return self.levels[-1][0]

    def siblings(self, i, lo=0, hi=None):
        return [self.levels[l][(i >> l) ^ 1] for l in range(lo, self.depth if hi is None else hi)]

    def node(self, i, level):
        return self.levels[level][i >> level]

    def upper(self, i, cuts):
        """(the packed rows of segments 1 .. G, the published nodes X_0 .. X_G) of a read of leaf i"""
        rows = [climb_row(self.node(i, lo), self.siblings(i, lo, hi), (i >> lo) & ((1 << (hi - lo)) - 1)) for lo, hi in ranges(self.depth, cuts)[1:]]
        return rows, [self.node(i, c) for c in list(cuts) + [self.depth]]

    def low(self, i, cuts):
        """(the siblings, the index) of segment 0 of a read of leaf i"""
        c0 = int(cuts[0])
        return self.siblings(i, 0, c0), i & ((1 << c0) - 1)


def _arrays(rows, nodes):
    rows = [np.frombuffer(b"".join(seg), dtype=np.uint8).reshape(len(seg), -1).copy() for seg in rows]
    return rows, np.frombuffer(b"".join(x for n in nodes for x in n), dtype=np.uint8).reshape(len(nodes), -1, 32).copy()


def path_segments(model, indices, cuts):
    """(rows: one array [n, bytes] per segment, nodes [n, G + 1, 32]): segment 0 a MerklePath(c_0) row"""
    rows, nodes = [[] for _ in range(len(cuts) + 1)], []
    for i in indices:
        i = int(i)
        up, pub = model.upper(i, cuts)
        rows[0].append(path_row(model.levels[0][i], *model.low(i, cuts)))
        for g, r in enumerate(up):
            rows[g + 1].append(r)
        nodes.append(pub)
    return _arrays(rows, nodes)


def record_segments(table, indices, cuts):
    """path_segments over a table of records, leaf i = SHA-256(record i): segment 0 a MerkleRecord(length, c_0) row"""
    table = [bytes(r) for r in table]
    model = ClimbModel([hashlib.sha256(r).digest() for r in table])
    rows, nodes = path_segments(model, indices, cuts)
    rows[0] = np.frombuffer(b"".join(record_row(table[int(i)], *model.low(int(i), cuts)) for i in indices), dtype=np.uint8).reshape(len(indices), -1).copy()
    return rows, nodes, model


def locate(table, K, q):
    """(index, status) of mfh_merkle_absent_rows: the lowest live record whose own key q is (1), else the lowest whose range holds it (0), else none (2)"""
    live = [(i, r[:K], r[K: 2 * K]) for i, r in enumerate(table) if r[:K] < r[K: 2 * K]]
    for i, lo, hi in live:
        if lo == q:
            return i, 1
    for i, lo, hi in live:
        if lo < q < hi:
            return i, 0
    return NONE, 2


def absent_segments(table, K, keys, cuts):
    """(rows, nodes, index [nq], status [nq], the tree's model): segment 0 a MerkleAbsent(K, length, c_0) row.  A status 2 query has 32 zero bytes and the
    key in segment 0, zeros behind them, all-zero upper rows and all-zero nodes below the root"""
    table = [bytes(r) for r in table]
    model = ClimbModel([hashlib.sha256(r).digest() for r in table])
    depth, length, c0 = model.depth, len(table[0]), int(cuts[0])
    segs = ranges(depth, cuts)
    rows = [np.zeros((len(keys), 32 + K + length + 32 * c0 + (c0 + 7) // 8), dtype=np.uint8)]
    rows += [np.zeros((len(keys), climb_row_bytes(hi - lo)), dtype=np.uint8) for lo, hi in segs[1:]]
    nodes = np.zeros((len(keys), len(segs), 32), dtype=np.uint8)
    index, status = [], []
    for k, q in enumerate(keys):
        q = bytes(q)
        i, s = locate(table, K, q)
        index.append(i)
        status.append(s)
        nodes[k, -1] = list(model.root())
        if s == 2:
            rows[0][k, 32: 32 + K] = list(q)
            continue
        rows[0][k] = np.frombuffer(absent_row(q, table[i], *model.low(i, cuts)), dtype=np.uint8)
        up, pub = model.upper(i, cuts)
        for g, r in enumerate(up):
            rows[g + 1][k] = np.frombuffer(r, dtype=np.uint8)
        nodes[k] = [list(x) for x in pub]
    return rows, nodes, np.array(index, dtype=np.uint32), np.array(status, dtype=np.uint8), model
