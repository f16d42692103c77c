"""A brute-force model of sequential transfers between the accounts of an indexed table (words.MerkleTransfer, MerkleTree.transfer_keys) for
tests/test_merkle_transfer_cpu.py and tests/test_gpu_merkle_transfer.py, beside tests/merkle_remove_model.py: the table as a list of records, the tree of
tests/test_gpu_merkle.py's ref_tree over their hashlib digests, one transfer at a time on the table as it then stands -- the lowest live record whose lo is
the sender's key (p), the lowest live record whose lo is the receiver's (s), the balances read as big-endian integers out of the records' bytes [2K, 2K + A),
p's update (balance - v), then s's (balance + v)."""
import numpy as np

from merkle_insert_model import InsertModel


def stand_in(K, length, depth, A=8, joined=True):
    """a MerkleTransfer without its circuit: bits() reads key_bytes, amount_bytes, length, depth and joined alone"""
    from c_lwe_snarks_amd import words

    st = object.__new__(words.MerkleTransfer)
    st.key_bytes, st.amount_bytes, st.length, st.depth, st.joined = K, A, length, depth, joined
    return st


def row_bytes(K, length, depth, A=8, zeros=64):
    return zeros + 2 * K + A + 2 * length + 64 * depth + (2 * depth + 7) // 8


def ledger(W, accounts, K, depth, length, A, rng=None, shuffle=False):
    """the records of a well-formed indexed table whose members are the keys of `accounts` (a dict key -> balance), the balance in bytes [2K, 2K + A) and random
    bytes behind it; the sentinel record and the inert slots carry random bytes there too (a transfer must leave them alone)"""
    keys = sorted(accounts)
    filler = (lambda n: rng.bytes(n)) if rng is not None else (lambda n: bytes(n))
    table = W.indexed_records(keys, depth, length=length, payloads=[accounts[k].to_bytes(A, "big") + filler(length - 2 * K - A) for k in keys])
    records = [r.tobytes() for r in table]
    records = [r if r[:K] < r[K: 2 * K] else r[: 2 * K] + filler(length - 2 * K) for r in records]  # inert slots: lo == hi == 0, any payload
    records[0] = records[0][: 2 * K] + filler(length - 2 * K)
    if shuffle:
        records = [records[int(i)] for i in rng.permutation(len(records))]
    return records


class TransferModel(InsertModel):
    """InsertModel (records, levels, set, siblings) with transfers; self.tr is the MerkleTransfer stand-in"""

    def __init__(self, records, K, A=8):
        super().__init__(records, K)
        self.A = A
        self.tr = stand_in(K, self.length, self.depth, A)

    def own(self, key):
        """the lowest live record whose own key is `key`, or None"""
        return next((i for i, r in enumerate(self.records) if self.live(i) and r[: self.K] == key), None)

    def balance(self, i):
        return int.from_bytes(self.records[i][2 * self.K: 2 * self.K + self.A], "big")

    def with_balance(self, i, value):
        r = self.records[i]
        return r[: 2 * self.K] + value.to_bytes(self.A, "big") + r[2 * self.K + self.A:]

    def status(self, k_from, k_to, v):
        """0 fine, 1 the sender is no member, 2 the receiver is none, 3 an overdraft, 4 an overflow: the first that applies, on the table as it stands"""
        p, s = self.own(bytes(k_from)), self.own(bytes(k_to))
        if p is None:
            return 1
        if s is None:
            return 2
        if v > self.balance(p):
            return 3
        return 4 if self.balance(s) + v >= 1 << (8 * self.A) else 0

    def transfer(self, k_from, k_to, v):
        """(p, s, the arguments of MerkleTransfer.bits): one transfer, applied"""
        k_from, k_to, v = bytes(k_from), bytes(k_to), int(v)
        assert self.status(k_from, k_to, v) == 0 and k_from != k_to, (k_from.hex(), k_to.hex(), v)
        p, s = self.own(k_from), self.own(k_to)
        old_p, sibs_p = self.records[p], self.siblings(p)
        self.set(p, self.with_balance(p, self.balance(p) - v))
        old_s, sibs_s = self.records[s], self.siblings(s)
        self.set(s, self.with_balance(s, self.balance(s) + v))
        return p, s, (k_from, k_to, v, old_p, old_s, sibs_p, p, sibs_s, s)

    def transfer_batch(self, steps):
        """(index [nk, 2], packed rows [nk, row bytes], the nk + 1 roots): the transfers (k_from, k_to, v) in order, applied"""
        index, roots = [], [self.root()]
        rows = np.zeros((len(steps), row_bytes(self.K, self.length, self.depth, self.A)), dtype=np.uint8)
        for j, step in enumerate(steps):
            p, s, args = self.transfer(*step)
            index.append((p, s))
            rows[j] = np.packbits(self.tr.bits(*args), bitorder="little")
            roots.append(self.root())
        return np.array(index, dtype=np.uint32).reshape(len(steps), 2), rows, roots

    def statuses(self, steps):
        """(index [nk, 2] with 0xFFFFFFFF for no record, status [nk]) of a batch in which a step with a status is left out, on a COPY: nothing is applied here"""
        m = TransferModel(self.records, self.K, self.A)
        index, status = [], []
        for k_from, k_to, v in steps:
            p, s = m.own(bytes(k_from)), m.own(bytes(k_to))
            index.append((0xFFFFFFFF if p is None else p, 0xFFFFFFFF if s is None else s))
            status.append(m.status(k_from, k_to, v))
            if not status[-1]:
                m.records[p] = m.with_balance(p, m.balance(p) - int(v))  # (the tree is not needed here)
                m.records[s] = m.with_balance(s, m.balance(s) + int(v))
        return np.array(index, dtype=np.uint32).reshape(len(steps), 2), np.array(status, dtype=np.uint8)


def transfer_cut_batch(records, K, A, steps, cuts):
    """sequential transfers with the path cut, beside tests/merkle_remove_model.py's remove_cut_batch: (rows: segment 0 one MerkleTransfer(K, length, c_0, A,
    joined=False) row a transfer, the upper segments one MerkleSegment row an UPDATE; nodes_p, nodes_s [nk, G + 1, 2, 32]; index [nk, 2]; the 2 nk + 1 roots;
    the TransferModel afterwards)"""
    from c_lwe_snarks_amd import words as W
    from merkle_segments_model import pack
    from merkle_segments_model import stand_in as any_stand_in

    m = TransferModel(records, K, A)
    depth, length, c0 = m.depth, m.length, cuts[0]
    low = (1 << c0) - 1
    st0 = stand_in(K, length, c0, A, joined=False)
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

    for k_from, k_to, v in steps:
        k_from, k_to, v = bytes(k_from), bytes(k_to), int(v)
        assert m.status(k_from, k_to, v) == 0
        p, s = m.own(k_from), m.own(k_to)
        old_p = m.records[p]
        sibs_p, pub_p = step(p, m.with_balance(p, m.balance(p) - v))
        old_s = m.records[s]
        sibs_s, pub_s = step(s, m.with_balance(s, m.balance(s) + v))
        rows[0].append(pack(st0.bits(k_from, k_to, v, old_p, old_s, sibs_p[:c0], p & low, sibs_s[:c0], s & low)))
        nodes[0].append(pub_p)
        nodes[1].append(pub_s)
        index.append((p, s))
    rows = [np.array(r, dtype=np.uint8) for r in rows]
    return (rows, np.array(nodes[0], dtype=np.uint8), np.array(nodes[1], dtype=np.uint8), np.array(index, dtype=np.uint32).reshape(len(steps), 2),
            np.array([list(r) for r in roots], dtype=np.uint8), m)
