"""A sequential host model of cut updates (words.MerkleSegment, MerkleTree.update_segments / update_record_segments / insert_key_segments) for
tests/test_merkle_segment_cpu.py and tests/test_gpu_merkle_segments.py: the tree of tests/test_gpu_merkle.py's ref_tree, one update at a time -- the nodes
on the leaf's path before and after, the siblings before, and every segment's packed row made by the statements' own bits()."""
import hashlib

import numpy as np

from c_lwe_snarks_amd import words as W
from test_gpu_merkle import _parent, ref_tree


def stand_in(cls, **sizes):
    """a statement without its circuit: bits() reads the sizes alone"""
    st = object.__new__(cls)
    for name, value in sizes.items():
        setattr(st, name, value)
    return st


def segment_row_bytes(levels):
    return 128 + 32 * levels + (levels + 7) // 8


def pack(bits):
    return np.packbits(bits, bitorder="little")


class TreeModel:
    def __init__(self, leaves):
        self.levels = ref_tree([bytes(x) for x in leaves])
        self.depth = len(self.levels) - 1

    def root(self):
        return self.levels[-1][0]

    def siblings(self, i):
        return [self.levels[l][(i >> l) ^ 1] for l in range(self.depth)]

    def path(self, i):
        return [self.levels[l][i >> l] for l in range(self.depth + 1)]

    def set(self, i, leaf):
        self.levels[0][i] = bytes(leaf)
        for l in range(self.depth):
            j = (i >> (l + 1)) << 1
            self.levels[l + 1][j >> 1] = _parent(self.levels[l][j], self.levels[l][j + 1])

    def update(self, i, leaf, cuts):
        """one update, applied: (the old path, the new path, the siblings before, the upper segments' packed rows, the published pairs [G + 1, 2, 32])"""
        old, sibs = self.path(i), self.siblings(i)
        self.set(i, leaf)
        new = self.path(i)
        rows = []
        for lo, hi in W.segment_levels(self.depth, cuts)[1:]:
            st = stand_in(W.MerkleSegment, levels=hi - lo, depth=hi - lo)
            rows.append(pack(st.bits(old[lo], new[lo], sibs[lo:hi], (i >> lo) & ((1 << (hi - lo)) - 1))))
        nodes = np.array([[list(old[c]), list(new[c])] for c in list(cuts) + [self.depth]], dtype=np.uint8)
        return old, new, sibs, rows, nodes


def leaf_batch(leaves, indices, new_leaves, cuts):
    """(rows: one array [n, bytes] per segment, nodes [n, G + 1, 2, 32], roots [n + 1, 32], the model afterwards): sequential leaf updates, segment 0 a
    MerkleUpdate(c_0) row"""
    m = TreeModel(leaves)
    c0 = cuts[0]
    st0 = stand_in(W.MerkleUpdate, depth=c0)
    rows = [[] for _ in range(len(cuts) + 1)]
    nodes, roots = [], [m.root()]
    for i, leaf in zip(indices, new_leaves):
        i = int(i)
        old, new, sibs, upper, pub = m.update(i, bytes(leaf), cuts)
        rows[0].append(pack(st0.bits(old[0], new[0], sibs[:c0], i & ((1 << c0) - 1))))
        for g, r in enumerate(upper):
            rows[g + 1].append(r)
        nodes.append(pub)
        roots.append(m.root())
    return [np.array(r, dtype=np.uint8) for r in rows], np.array(nodes, dtype=np.uint8), np.array([list(r) for r in roots], dtype=np.uint8), m


def record_batch(table, indices, new_records, cuts):
    """leaf_batch over a table of records: leaf i = SHA-256(record i), segment 0 a MerkleRecordUpdate(length, c_0) row; also the table afterwards"""
    table = [bytes(r) for r in table]
    m = TreeModel([hashlib.sha256(r).digest() for r in table])
    c0, length = cuts[0], len(table[0])
    st0 = stand_in(W.MerkleRecordUpdate, depth=c0, length=length)
    rows = [[] for _ in range(len(cuts) + 1)]
    nodes, roots = [], [m.root()]
    for i, rec in zip(indices, new_records):
        i, rec = int(i), bytes(rec)
        old_rec = table[i]
        table[i] = rec
        _, _, sibs, upper, pub = m.update(i, hashlib.sha256(rec).digest(), cuts)
        rows[0].append(pack(st0.bits(old_rec, rec, sibs[:c0], i & ((1 << c0) - 1))))
        for g, r in enumerate(upper):
            rows[g + 1].append(r)
        nodes.append(pub)
        roots.append(m.root())
    return [np.array(r, dtype=np.uint8) for r in rows], np.array(nodes, dtype=np.uint8), np.array([list(r) for r in roots], dtype=np.uint8), m, table


def insert_row_bytes(K, length, c0):
    return 128 + K + 3 * length + 64 * c0 + (2 * c0 + 7) // 8


def insert_batch(records, K, keys, payloads, cuts):
    """sequential key inserts (tests/merkle_insert_model.py's InsertModel finds p and s) with the path cut: (rows: segment 0 one MerkleInsert(K, length, c_0,
    joined=False) row an insert, the upper segments one MerkleSegment row an UPDATE; nodes_p, nodes_s [nk, G + 1, 2, 32]; index [nk, 2]; the 2 nk + 1 roots;
    the InsertModel afterwards)"""
    from merkle_insert_model import InsertModel

    m = InsertModel(records, K)
    depth, length, c0 = m.depth, m.length, cuts[0]
    low = (1 << c0) - 1
    st0 = stand_in(W.MerkleInsert, key_bytes=K, length=length, depth=c0, joined=False)
    ranges = W.segment_levels(depth, cuts)
    rows = [[] for _ in ranges]
    nodes, index, roots = [[], []], [], [m.root()]

    def step(i, record):
        """one record update, applied: (the siblings before, its upper rows appended, its published pairs)"""
        old, sibs = [m.levels[l][i >> l] for l in range(depth + 1)], m.siblings(i)
        m.set(i, record)
        new = [m.levels[l][i >> l] for l in range(depth + 1)]
        for g, (lo, hi) in enumerate(ranges[1:], start=1):
            st = stand_in(W.MerkleSegment, levels=hi - lo, depth=hi - lo)
            rows[g].append(pack(st.bits(old[lo], new[lo], sibs[lo:hi], (i >> lo) & ((1 << (hi - lo)) - 1))))
        roots.append(m.root())
        return sibs, np.array([[list(old[c]), list(new[c])] for c in list(cuts) + [depth]], dtype=np.uint8)

    for j, key in enumerate(keys):
        key = bytes(key)
        p = m.locate(key)
        s = next(i for i in range(len(m.records)) if not m.live(i))
        old_p = m.records[p]
        sibs_p, pub_p = step(p, old_p[:K] + key + old_p[2 * K:])
        old_s = m.records[s]
        new_s = (key + old_p[K: 2 * K] + bytes(b"" if payloads is None else payloads[j])).ljust(length, b"\0")
        sibs_s, pub_s = step(s, new_s)
        rows[0].append(pack(st0.bits(key, old_p, old_s, new_s, sibs_p[:c0], p & low, sibs_s[:c0], s & low)))
        nodes[0].append(pub_p)
        nodes[1].append(pub_s)
        index.append((p, s))
    rows = [np.array(r, dtype=np.uint8) for r in rows]
    return (rows, np.array(nodes[0], dtype=np.uint8), np.array(nodes[1], dtype=np.uint8), np.array(index, dtype=np.uint32).reshape(len(keys), 2),
            np.array([list(r) for r in roots], dtype=np.uint8), m)
