"""A brute-force model of sequential key inserts into an indexed table (words.MerkleInsert, MerkleTree.insert_keys) for tests/test_merkle_insert_cpu.py and
tests/test_gpu_merkle_insert.py: the table as a list of records, the tree of tests/test_gpu_merkle.py's ref_tree over their hashlib digests, one key at a
time -- the lowest live record whose range holds the key, the lowest inert slot of the table as it then stands, p's update, then s's."""
import hashlib

import numpy as np

from test_gpu_merkle import _parent, ref_tree


def stand_in(K, length, depth):
    """a MerkleInsert without its circuit: bits() reads key_bytes, length and depth alone"""
    from c_lwe_snarks_amd import words

    st = object.__new__(words.MerkleInsert)
    st.key_bytes, st.length, st.depth = K, length, depth
    return st


def row_bytes(K, length, depth):
    return 64 + K + 3 * length + 64 * depth + (2 * depth + 7) // 8


class InsertModel:
    def __init__(self, records, K):
        self.records = [bytes(r) for r in records]
        self.K, self.length = K, len(self.records[0])
        self.depth = len(self.records).bit_length() - 1
        assert len(self.records) == 1 << self.depth
        self.levels = ref_tree([hashlib.sha256(r).digest() for r in self.records])
        self.st = stand_in(K, self.length, self.depth)

    def root(self):
        return self.levels[-1][0]

    def live(self, i):
        return self.records[i][: self.K] < self.records[i][self.K: 2 * self.K]

    def siblings(self, i):
        return [self.levels[l][(i >> l) ^ 1] for l in range(self.depth)]

    def set(self, i, record):
        self.records[i] = bytes(record)
        self.levels[0][i] = hashlib.sha256(self.records[i]).digest()
        for l in range(self.depth):
            j = (i >> (l + 1)) << 1
            self.levels[l + 1][j >> 1] = _parent(self.levels[l][j], self.levels[l][j + 1])

    def locate(self, key):
        K = self.K
        return next(i for i, r in enumerate(self.records) if r[:K] < key < r[K: 2 * K])

    def insert(self, key, payload=b""):
        """(p, s, the arguments of MerkleInsert.bits): one insert, applied"""
        K, key = self.K, bytes(key)
        p = self.locate(key)
        s = next(i for i in range(len(self.records)) if not self.live(i))
        old_p, sibs_p = self.records[p], self.siblings(p)
        self.set(p, old_p[:K] + key + old_p[2 * K:])
        old_s, sibs_s = self.records[s], self.siblings(s)
        new_s = (key + old_p[K: 2 * K] + bytes(payload)).ljust(self.length, b"\0")
        self.set(s, new_s)
        return p, s, (key, old_p, old_s, new_s, sibs_p, p, sibs_s, s)

    def batch(self, keys, payloads=None):
        """(index [nk, 2], packed rows [nk, row bytes], the nk + 1 roots): the inserts in order, applied"""
        index, roots = [], [self.root()]
        rows = np.zeros((len(keys), row_bytes(self.K, self.length, self.depth)), dtype=np.uint8)
        for j, key in enumerate(keys):
            p, s, args = self.insert(key, b"" if payloads is None else payloads[j])
            index.append((p, s))
            rows[j] = np.packbits(self.st.bits(*args), bitorder="little")
            roots.append(self.root())
        return np.array(index, dtype=np.uint32).reshape(len(keys), 2), rows, roots
