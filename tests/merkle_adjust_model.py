"""A brute-force model of sequential deposits and withdrawals on the accounts of an indexed table (words.MerkleAdjust, MerkleTree.adjust_keys) and of the
table's supply (MerkleTree.total_balance) for tests/test_merkle_adjust_cpu.py and tests/test_gpu_merkle_adjust.py, beside tests/merkle_transfer_model.py: the
table as a list of records, the tree of tests/test_gpu_merkle.py's ref_tree over their hashlib digests, one step at a time on the table as it then stands --
the lowest live record whose lo is the key, its balance read as a big-endian integer out of bytes [2K, 2K + A), the record's update.  A packed row is put
together here byte by byte, not by the statement's bits()."""
import numpy as np

from merkle_insert_model import InsertModel
from merkle_transfer_model import ledger  # noqa: F401  (the tests' well-formed tables)


def row_bytes(K, length, depth, A=8):
    return 64 + K + A + 1 + length + 32 * depth + (depth + 7) // 8


def packed_row(key, amount, side, old_record, siblings, index, A):
    """64 zero bytes | k | v as A big-endian bytes | side | the old record | the siblings as words (each word's 4 bytes reversed) | the index bytes, LSB first"""
    depth = len(siblings)
    tail = b"".join(s[i: i + 4][::-1] for s in siblings for i in range(0, 32, 4)) + int(index).to_bytes((depth + 7) // 8, "little")
    return np.frombuffer(bytes(64) + bytes(key) + int(amount).to_bytes(A, "big") + bytes([side]) + bytes(old_record) + tail, dtype=np.uint8)


def supply(records, K, A=8):
    """(the sum of the live records' balances as a Python int, the number of live records)"""
    live = [r for r in records if bytes(r[:K]) < bytes(r[K: 2 * K])]
    return sum(int.from_bytes(bytes(r[2 * K: 2 * K + A]), "big") for r in live), len(live)


class AdjustModel(InsertModel):
    """InsertModel (records, levels, set, siblings) with adjusts"""

    def __init__(self, records, K, A=8):
        super().__init__(records, K)
        self.A = A

    def own(self, key):
        """the lowest live record whose own key is `key`, or None"""
        return next((i for i, r in enumerate(self.records) if self.live(i) and r[: self.K] == key), None)

    def balance(self, i):
        return int.from_bytes(self.records[i][2 * self.K: 2 * self.K + self.A], "big")

    def with_balance(self, i, value):
        r = self.records[i]
        return r[: 2 * self.K] + value.to_bytes(self.A, "big") + r[2 * self.K + self.A:]

    def supply(self):
        return supply(self.records, self.K, self.A)

    def status(self, key, v, side):
        """0 fine, 1 the key is no member, 3 an overdraft, 4 an overflow: the first that applies, on the table as it stands"""
        i = self.own(bytes(key))
        if i is None:
            return 1
        if side and v > self.balance(i):
            return 3
        return 4 if not side and self.balance(i) + v >= 1 << (8 * self.A) else 0

    def adjust(self, key, v, side):
        """(the slot, the arguments of MerkleAdjust.bits): one step, applied"""
        key, v, side = bytes(key), int(v), int(side)
        assert self.status(key, v, side) == 0, (key.hex(), v, side)
        i = self.own(key)
        old, sibs = self.records[i], self.siblings(i)
        self.set(i, self.with_balance(i, self.balance(i) - v if side else self.balance(i) + v))
        return i, (key, v, side, old, sibs, i)

    def adjust_batch(self, steps):
        """(index [nk], packed rows [nk, row bytes], the nk + 1 roots): the steps (key, v, side) in order, applied"""
        index, roots = [], [self.root()]
        rows = np.zeros((len(steps), row_bytes(self.K, self.length, self.depth, self.A)), dtype=np.uint8)
        for j, step in enumerate(steps):
            i, (key, v, side, old, sibs, _) = self.adjust(*step)
            index.append(i)
            rows[j] = packed_row(key, v, side, old, sibs, i, self.A)
            roots.append(self.root())
        return np.array(index, dtype=np.uint32), rows, roots

    def statuses(self, steps):
        """(index [nk] with 0xFFFFFFFF for no record, status [nk]) of a batch in which a step with a status is left out, on a COPY: nothing is applied here"""
        m = AdjustModel(self.records, self.K, self.A)
        index, status = [], []
        for key, v, side in steps:
            i = m.own(bytes(key))
            index.append(0xFFFFFFFF if i is None else i)
            status.append(m.status(key, int(v), int(side)))
            if not status[-1]:
                m.records[i] = m.with_balance(i, m.balance(i) - int(v) if side else m.balance(i) + int(v))  # (the tree is not needed here)
        return np.array(index, dtype=np.uint32), np.array(status, dtype=np.uint8)


def adjust_cut_batch(records, K, A, steps, cuts):
    """sequential adjusts with the path cut, through tests/merkle_segments_model.py's TreeModel.update: (rows: segment 0 one MerkleAdjust(K, length, c_0, A) row a
    step, every upper segment one MerkleSegment row a step; nodes [nk, G + 1, 2, 32]; index [nk]; the nk + 1 roots; the AdjustModel afterwards)"""
    import hashlib

    from merkle_segments_model import TreeModel

    m = AdjustModel(records, K, A)
    tree = TreeModel([hashlib.sha256(r).digest() for r in m.records])
    c0 = cuts[0]
    rows = [[] for _ in range(len(cuts) + 1)]
    nodes, index, roots = [], [], [tree.root()]
    for key, v, side in steps:
        i, (key, v, side, old, _, _) = m.adjust(key, v, side)
        _, _, sibs, upper, pub = tree.update(i, hashlib.sha256(m.records[i]).digest(), cuts)
        rows[0].append(packed_row(key, v, side, old, sibs[:c0], i & ((1 << c0) - 1), A))
        for g, r in enumerate(upper):
            rows[g + 1].append(r)
        nodes.append(pub)
        index.append(i)
        roots.append(tree.root())
        assert tree.root() == m.root()
    return ([np.array(r, dtype=np.uint8) for r in rows], np.array(nodes, dtype=np.uint8), np.array(index, dtype=np.uint32),
            np.array([list(r) for r in roots], dtype=np.uint8), m)
