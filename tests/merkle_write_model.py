"""A brute-force model of sequential writes by key, plain and compare-and-set, on the records of an indexed table (words.MerkleWrite, MerkleTree.write_keys) for
tests/test_merkle_write_cpu.py and tests/test_gpu_merkle_write.py, beside tests/merkle_adjust_model.py: the table as a list of records, the tree of
tests/test_gpu_merkle.py's ref_tree over their hashlib digests, one step at a time on the table as it then stands -- the lowest live record whose lo is the
key, its bytes [lo, hi) compared with the expectation and replaced by the value, the record's update.  A packed row is put together here byte by byte, not by
the statement's bits().  A step is (key, value) or (key, value, expect); expect None is a plain write."""
import numpy as np

from merkle_insert_model import InsertModel


def row_bytes(K, length, depth, F, expect=False):
    return 64 + K + (2 * F if expect else F) + length + 32 * depth + (depth + 7) // 8


def packed_row(key, expect, value, old_record, siblings, index):
    """64 zero bytes | k | [e |] v | the old record | the siblings as words (each word's 4 bytes reversed) | the index bytes, LSB first"""
    depth = len(siblings)
    tail = b"".join(s[i: i + 4][::-1] for s in siblings for i in range(0, 32, 4)) + int(index).to_bytes((depth + 7) // 8, "little")
    return np.frombuffer(bytes(64) + bytes(key) + (b"" if expect is None else bytes(expect)) + bytes(value) + bytes(old_record) + tail, dtype=np.uint8)


def table_of(W, payloads, K, depth, length, rng=None, shuffle=False):
    """the records of a well-formed indexed table whose members are the keys of `payloads` (a dict key -> the length - 2K payload bytes); the sentinel record and
    the inert slots carry random bytes behind their keys (a write must leave them alone)"""
    keys = sorted(payloads)
    filler = (lambda n: rng.bytes(n)) if rng is not None else (lambda n: bytes(n))
    table = W.indexed_records(keys, depth, length=length, payloads=[bytes(payloads[k]) for k in keys])
    records = [r.tobytes() for r in table]
    records = [r if r[:K] < r[K: 2 * K] else r[: 2 * K] + filler(length - 2 * K) for r in records]
    records[0] = records[0][: 2 * K] + filler(length - 2 * K)
    if shuffle:
        records = [records[int(i)] for i in rng.permutation(len(records))]
    return records


def _step(step):
    key, value, expect = (tuple(step) + (None,))[:3]
    return bytes(key), bytes(value), None if expect is None else bytes(expect)


class WriteModel(InsertModel):
    """InsertModel (records, levels, set, siblings) with writes to the field [lo, hi)"""

    def __init__(self, records, K, field):
        super().__init__(records, K)
        self.lo, self.hi = field
        self.F = self.hi - self.lo
        assert 2 * K <= self.lo < self.hi <= self.length

    def own(self, key):
        """the lowest live record whose own key is `key`, or None"""
        return next((i for i, r in enumerate(self.records) if self.live(i) and r[: self.K] == key), None)

    def field(self, i):
        return self.records[i][self.lo: self.hi]

    def status(self, key, expect=None):
        """0 fine, 1 the key is no member, 5 the field is not what is expected: the first that applies, on the table as it stands"""
        i = self.own(bytes(key))
        if i is None:
            return 1
        return 5 if expect is not None and self.field(i) != bytes(expect) else 0

    def write(self, key, value, expect=None):
        """(the slot, the arguments of MerkleWrite.bits): one step, applied"""
        key, value, expect = _step((key, value, expect))
        assert len(value) == self.F and self.status(key, expect) == 0, (key.hex(), value.hex(), expect)
        i = self.own(key)
        old, sibs = self.records[i], self.siblings(i)
        self.set(i, old[: self.lo] + value + old[self.hi:])
        return i, (key,) + (() if expect is None else (expect,)) + (value, old, sibs, i)

    def write_batch(self, steps):
        """(index [nk], packed rows [nk, row bytes], the nk + 1 roots): the steps in order, applied; all with an expectation or none"""
        steps = [_step(s) for s in steps]
        conditional = bool(steps) and steps[0][2] is not None
        assert all((s[2] is not None) == conditional for s in steps)
        index, roots = [], [self.root()]
        rows = np.zeros((len(steps), row_bytes(self.K, self.length, self.depth, self.F, conditional)), dtype=np.uint8)
        for j, (key, value, expect) in enumerate(steps):
            i, args = self.write(key, value, expect)
            index.append(i)
            rows[j] = packed_row(key, expect, value, args[-3], args[-2], i)
            roots.append(self.root())
        return np.array(index, dtype=np.uint32), rows, roots

    def statuses(self, steps):
        """(index [nk] with 0xFFFFFFFF for no record, status [nk]) of a batch in which a step with a status is left out, on a COPY: nothing is applied here"""
        m = WriteModel(self.records, self.K, (self.lo, self.hi))
        index, status = [], []
        for key, value, expect in (_step(s) for s in steps):
            i = m.own(key)
            index.append(0xFFFFFFFF if i is None else i)
            status.append(m.status(key, expect))
            if not status[-1]:
                m.records[i] = m.records[i][: m.lo] + value + m.records[i][m.hi:]  # (the tree is not needed here)
        return np.array(index, dtype=np.uint32), np.array(status, dtype=np.uint8)


def write_cut_batch(records, K, field, steps, cuts):
    """sequential writes with the path cut, through tests/merkle_segments_model.py's TreeModel.update: (rows: segment 0 one MerkleWrite(K, length, c_0, field,
    expect) row a step, every upper segment one MerkleSegment row a step; nodes [nk, G + 1, 2, 32]; index [nk]; the nk + 1 roots; the WriteModel afterwards)"""
    import hashlib

    from merkle_segments_model import TreeModel

    m = WriteModel(records, K, field)
    tree = TreeModel([hashlib.sha256(r).digest() for r in m.records])
    c0 = cuts[0]
    rows = [[] for _ in range(len(cuts) + 1)]
    nodes, index, roots = [], [], [tree.root()]
    for key, value, expect in (_step(s) for s in steps):
        i, args = m.write(key, value, expect)
        _, _, sibs, upper, pub = tree.update(i, hashlib.sha256(m.records[i]).digest(), cuts)
        rows[0].append(packed_row(key, expect, value, args[-3], sibs[:c0], i & ((1 << c0) - 1)))
        for g, r in enumerate(upper):
            rows[g + 1].append(r)
        nodes.append(pub)
        index.append(i)
        roots.append(tree.root())
        assert tree.root() == m.root()
    return ([np.array(r, dtype=np.uint8) for r in rows], np.array(nodes, dtype=np.uint8), np.array(index, dtype=np.uint32),
            np.array([list(r) for r in roots], dtype=np.uint8), m)
