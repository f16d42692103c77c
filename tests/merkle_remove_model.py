"""A brute-force model of sequential key removes from an indexed table (words.MerkleRemove, MerkleTree.remove_keys) for tests/test_merkle_remove_cpu.py and
tests/test_gpu_merkle_remove.py, beside tests/merkle_insert_model.py: the table as a list of records, the tree of tests/test_gpu_merkle.py's ref_tree over
their hashlib digests, one key at a time -- the lowest live record whose lo is the key (s), the lowest live record whose hi is the key (p), p's update
(hi <- s's hi), then s's (the all-zero record)."""
import numpy as np

from merkle_insert_model import InsertModel


def stand_in(K, length, depth, joined=True):
    """a MerkleRemove without its circuit: bits() reads key_bytes, length, depth and joined alone"""
    from c_lwe_snarks_amd import words

    st = object.__new__(words.MerkleRemove)
    st.key_bytes, st.length, st.depth, st.joined = K, length, depth, joined
    return st


def row_bytes(K, length, depth, zeros=64):
    return zeros + K + 2 * length + 64 * depth + (2 * depth + 7) // 8


def remove_cut_batch(records, K, keys, cuts):
    """sequential key removes with the path cut, beside tests/merkle_segments_model.py's insert_batch: (rows: segment 0 one MerkleRemove(K, length, c_0,
    joined=False) row a remove, the upper segments one MerkleSegment row an UPDATE; nodes_p, nodes_s [nk, G + 1, 2, 32]; index [nk, 2]; the 2 nk + 1 roots;
    the RemoveModel afterwards)"""
    from c_lwe_snarks_amd import words as W
    from merkle_segments_model import pack
    from merkle_segments_model import stand_in as any_stand_in

    m = RemoveModel(records, K)
    depth, length, c0 = m.depth, m.length, cuts[0]
    low = (1 << c0) - 1
    st0 = stand_in(K, length, c0, joined=False)
    ranges = W.segment_levels(depth, cuts)
    rows = [[] for _ in ranges]
    nodes, index, roots = [[], []], [], [m.root()]

    def step(i, record):
        """one record update, applied: (the siblings before, its upper rows appended, its published pairs)"""
        old, sibs = [m.levels[l][i >> l] for l in range(depth + 1)], m.siblings(i)
        m.set(i, record)
        new = [m.levels[l][i >> l] for l in range(depth + 1)]
        for g, (lo, hi) in enumerate(ranges[1:], start=1):
            st = any_stand_in(W.MerkleSegment, levels=hi - lo, depth=hi - lo)
            rows[g].append(pack(st.bits(old[lo], new[lo], sibs[lo:hi], (i >> lo) & ((1 << (hi - lo)) - 1))))
        roots.append(m.root())
        return sibs, np.array([[list(old[c]), list(new[c])] for c in list(cuts) + [depth]], dtype=np.uint8)

    for key in keys:
        key = bytes(key)
        s, p = m.own(key), m.prev(key)
        old_p = m.records[p]
        sibs_p, pub_p = step(p, old_p[:K] + m.records[s][K: 2 * K] + old_p[2 * K:])
        old_s = m.records[s]
        sibs_s, pub_s = step(s, bytes(length))
        rows[0].append(pack(st0.bits(key, old_p, old_s, sibs_p[:c0], p & low, sibs_s[:c0], s & low)))
        nodes[0].append(pub_p)
        nodes[1].append(pub_s)
        index.append((p, s))
    rows = [np.array(r, dtype=np.uint8) for r in rows]
    return (rows, np.array(nodes[0], dtype=np.uint8), np.array(nodes[1], dtype=np.uint8), np.array(index, dtype=np.uint32).reshape(len(keys), 2),
            np.array([list(r) for r in roots], dtype=np.uint8), m)


class RemoveModel(InsertModel):
    """InsertModel (records, levels, set, siblings, insert) with removes; self.rm is the MerkleRemove stand-in"""

    def __init__(self, records, K):
        super().__init__(records, K)
        self.rm = stand_in(K, self.length, self.depth)

    def own(self, key):
        """the lowest live record whose own key is `key`, or None"""
        return next((i for i, r in enumerate(self.records) if self.live(i) and r[: self.K] == key), None)

    def prev(self, key):
        """the lowest live record whose hi is `key`, or None"""
        return next((i for i, r in enumerate(self.records) if self.live(i) and r[self.K: 2 * self.K] == key), None)

    def remove(self, key):
        """(p, s, the arguments of MerkleRemove.bits): one remove, applied"""
        K, key = self.K, bytes(key)
        s, p = self.own(key), self.prev(key)
        assert s is not None and p is not None and p != s, (key.hex(), p, s)
        old_p, sibs_p, hi_s = self.records[p], self.siblings(p), self.records[s][K: 2 * K]
        self.set(p, old_p[:K] + hi_s + old_p[2 * K:])
        old_s, sibs_s = self.records[s], self.siblings(s)
        self.set(s, bytes(self.length))
        return p, s, (key, old_p, old_s, sibs_p, p, sibs_s, s)

    def remove_batch(self, keys):
        """(index [nk, 2], packed rows [nk, row bytes], the nk + 1 roots): the removes in order, applied"""
        index, roots = [], [self.root()]
        rows = np.zeros((len(keys), row_bytes(self.K, self.length, self.depth)), dtype=np.uint8)
        for j, key in enumerate(keys):
            p, s, args = self.remove(key)
            index.append((p, s))
            rows[j] = np.packbits(self.rm.bits(*args), bitorder="little")
            roots.append(self.root())
        return np.array(index, dtype=np.uint32).reshape(len(keys), 2), rows, roots
