"""GPU: non-membership in an indexed table on the device (mfh_merkle_absent_rows, MerkleTree.locate_keys / absent_rows / absent_bits) against a brute-force
model in this file: a list of records, the lowest live record whose range holds a key or whose own key it is, leaves from hashlib.sha256 and the tree of
tests/test_gpu_merkle.py's ref_tree.

Every check compares index, status and the rows byte for byte against MerkleAbsent(key_bytes, length, depth).bits on the model, and the whole allocation
the table lives in afterwards: the table sits inside a larger uint8 tensor filled with 0xA5 (tests/test_gpu_merkle_record_update.py's Placed), and nothing
of it may change.

1. hand-made sets at depth 1, 2, 3 x key_bytes 1, 4: queries lo + 1, hi - 1, == lo and == hi (status 1, full rows) of every live record, an empty range
   hi = lo + 1 among them; the empty set, whose sentinel record holds every query.
2. key widths 1, 3, 4, 5, 8, 20, 32 at depth 3: members that differ in the first byte only, in the last byte only, and the pair ..00 FF / ..01 00.
3. alignment at depth 3, key_bytes 4 and 5: lengths 2K, 2K + 1, 55, 64, 65; the table 0 .. 3 bytes into its tensor; strides length and length + 5.
4. shapes: depth 8 and 9 (one workgroup, two) with 257 queries and duplicates; all 257 queries in one range (the wave's cooperative fill); 65 in one range
   and the rest spread; a random set at depth 12 with 300 queries, half of them members.
5. records in shuffled positions at depth 6; indexed_insert through update_records, then the same answers from the grown set, and the tree is the model's.
6. malformed tables: two live records with overlapping ranges report the lower index; a gap gives status 2, index 0xFFFFFFFF, a row of zeros and q with
   the rest untouched.
7. h_inputs = NULL gives the same index and status with no "merkle_paths" launch; the timing counts; a wider in_stride keeps its tail; scrubbed staging
   gives the same rows; a table produced late on the stream, on the null stream and on a caller's.
8. two chunks: depth 1, key_bytes 4, length 65 521 (a row is 65 590 bytes, a chunk 1 023 queries), 1 030 queries: both records on both sides of the seam.
9. every MFH_EINVAL case leaves tree, table and timing counts as they were; nq = 0 does nothing.
10. end to end at d = 2^17 with MerkleAbsent(4, 8, 1): four absent queries hold with the tree's root, violate no row, their proofs verify under
    statement(root, q_k) and under neither another absent key's statement, a member's, nor another root; a member's status 1 row does not hold and
    violates a row.

MerkleAbsent.bits reads key_bytes, length and depth alone; it is called on an instance made without its circuit (building one takes seconds for nothing)
-- the depth-1 case of test 1 checks that this stand-in and the statement give the same bits."""
import ctypes
import hashlib

import numpy as np
import pytest

from test_gpu_merkle import _assert_tree, _flip, ref_tree
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

SEED = bytes((41 * i + 7) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_locate", "merkle_absent_rows", "merkle_paths", "merkle_level", "sha256_records")


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def W():
    from c_lwe_snarks_amd import words

    return words


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()  # (the tree does not depend on the parameters)


# ---------------------------------------------------------------------------------------------------------------- the reference side
def _row_bytes(K, length, depth):
    return 32 + K + length + 32 * depth + (depth + 7) // 8


def _stand_in(K, length, depth):
    from c_lwe_snarks_amd import words

    st = object.__new__(words.MerkleAbsent)
    st.key_bytes, st.length, st.depth = K, length, depth
    return st


def _key(x, K):
    return int(x).to_bytes(K, "big")


class IndexedModel:
    """a table of records (lo | hi | payload) in given positions and the tree over their SHA-256 digests"""

    def __init__(self, records, K):
        self.records = [bytes(r) for r in records]
        self.K, self.length = K, len(self.records[0])
        self.depth = len(self.records).bit_length() - 1
        assert len(self.records) == 1 << self.depth
        self.levels = ref_tree([hashlib.sha256(r).digest() for r in self.records])
        self.st = _stand_in(K, self.length, self.depth)
        self.live = [(i, r[:K], r[K: 2 * K]) for i, r in enumerate(self.records) if r[:K] < r[K: 2 * K]]

    def root(self):
        return self.levels[-1][0]

    def locate(self, q):
        """(index, status): the lowest live record whose own key q is, else the lowest whose range holds it, else none"""
        for i, lo, hi in self.live:
            if lo == q:
                return i, 1
        for i, lo, hi in self.live:
            if lo < q < hi:
                return i, 0
        return NONE, 2

    def answers(self, keys):
        """(index [nq], status [nq], packed rows [nq, row bytes]); a status 2 row is 32 zero bytes and q, zeros behind them"""
        rowb = _row_bytes(self.K, self.length, self.depth)
        index, status, rows = [], [], np.zeros((len(keys), rowb), dtype=np.uint8)
        for k, q in enumerate(keys):
            q = bytes(q)
            i, s = self.locate(q)
            index.append(i)
            status.append(s)
            if s == 2:
                rows[k, 32: 32 + self.K] = np.frombuffer(q, dtype=np.uint8)
            else:
                sibs = [self.levels[l][(i >> l) ^ 1] for l in range(self.depth)]
                rows[k] = np.packbits(self.st.bits(q, self.records[i], sibs, i), bitorder="little")
        return np.array(index, dtype=np.uint32), np.array(status, dtype=np.uint8), rows


def _table(W, members, K, depth, length, rng):
    """the records of indexed_records with random payloads, as a list of bytes"""
    pay = [rng.bytes(length - 2 * K) for _ in members]
    keys = np.frombuffer(b"".join(members), dtype=np.uint8).reshape(len(members), K) if members else np.zeros((0, K), dtype=np.uint8)
    return [r.tobytes() for r in W.indexed_records(keys, depth, length=length, payloads=pay)]


def _edge_queries(records, K):
    """of every live record: lo + 1 and hi - 1 where they are inside, lo and hi themselves where they are no sentinels"""
    out = []
    for r in records:
        lo, hi = int.from_bytes(r[:K], "big"), int.from_bytes(r[K: 2 * K], "big")
        if lo < hi:
            out += [_key(x, K) for x in (lo + 1, hi - 1) if lo < x < hi]
            out += [_key(x, K) for x in (lo, hi) if 0 < x < (1 << 8 * K) - 1]
    return out


def _keys(queries, K):
    return np.frombuffer(b"".join(queries), dtype=np.uint8).reshape(len(queries), K).copy()


def _check(tree, model, table, queries, what, tree_too=False):
    """one absent_rows and one locate_keys call against the model; the table's whole allocation afterwards"""
    keys = _keys(queries, model.K)
    want_i, want_s, want_rows = model.answers(queries)
    rows, index, status = tree.absent_rows(table.view, keys)
    assert index.dtype == np.uint32 and status.dtype == np.uint8 and rows.dtype == np.uint8 and rows.shape == want_rows.shape, what
    assert np.array_equal(index, want_i) and np.array_equal(status, want_s), (what, index, want_i, status, want_s)
    assert np.array_equal(rows, want_rows), what
    index2, status2 = tree.locate_keys(table.view, keys)
    assert np.array_equal(index2, want_i) and np.array_equal(status2, want_s), what
    table.holds(model.records, what)
    if tree_too:
        _assert_tree(tree, model.levels, what)
    return want_s


def _setup(ctx, tree, records, **placing):
    table = Placed(ctx, records, **placing)
    tree.set_records(0, table.view)
    return table


# ---------------------------------------------------------------------------------------------------------------- 1. hand-made sets
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_hand_made_sets(ctx, W, depth, K):
    rng = np.random.default_rng(12000 + 10 * depth + K)
    length = 2 * K + 3
    top = 0x10 << (8 * (K - 1))
    members = [_key(x, K) for x in (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))][: (1 << depth) - 1]  # top, top + 1: an empty range
    tree = ctx.merkle_tree(depth)
    try:
        records = _table(W, members, K, depth, length, rng)
        model = IndexedModel(records, K)
        queries = _edge_queries(records, K)
        if depth == 1:  # the stand-in gives what the statement gives
            args = (queries[0], records[0], [rng.bytes(32)], 1)
            assert np.array_equal(model.st.bits(*args), W.MerkleAbsent(K, length, 1).bits(*args))
        table = _setup(ctx, tree, records, stride=length + 3, off=1)
        status = _check(tree, model, table, queries, (depth, K), tree_too=True)
        assert set(status) == {0, 1}
        if depth > 1:
            assert model.locate(members[0])[0] == 1 and model.locate(members[1]) == (2, 1)  # == hi of record 1: present at the next record
        # one query alone, and the whole list twice over
        _check(tree, model, table, queries[:1], (depth, K, "one"))
        _check(tree, model, table, queries + queries[::-1], (depth, K, "twice"))
        # the empty set: the sentinel record alone holds every query
        records = _table(W, [], K, depth, length, rng)
        model = IndexedModel(records, K)
        table = _setup(ctx, tree, records)
        some = [_key(x, K) for x in (1, top, (1 << 8 * K) - 2)]
        assert not _check(tree, model, table, some, (depth, K, "empty set"), tree_too=True).any()
        assert [model.locate(q)[0] for q in some] == [0, 0, 0]
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. key widths
@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 20, 32])
def test_key_widths(ctx, W, K):
    depth = 3
    rng = np.random.default_rng(12100 + K)
    length = 2 * K + 1
    if K == 1:
        members = [bytes([x]) for x in (0x10, 0x20, 0x30, 0x50, 0x51, 0x60, 0xFE)]
    else:
        rest, mid = rng.bytes(K - 1), rng.bytes(K - 2)
        members = [bytes([x]) + rest for x in (0x10, 0x20, 0x30)]  # the first byte alone differs
        members += [bytes([0x50]) + mid + bytes([x]) for x in (0x10, 0x20)]  # the last byte alone differs
        members += [bytes([0x60]) + bytes(K - 3) + tail for tail in (b"\x00\xff", b"\x01\x00")] if K >= 3 else []  # ordered as integers, not byte by byte from the end
    tree = ctx.merkle_tree(depth)
    try:
        records = _table(W, members, K, depth, length, rng)
        model = IndexedModel(records, K)
        table = _setup(ctx, tree, records, stride=length + 2, off=3)
        queries = _edge_queries(records, K)
        if K >= 3:  # between the pair, and on either side of it
            queries += [bytes([0x60]) + bytes(K - 3) + tail for tail in (b"\x00\xfe", b"\x01\x01")]
        status = _check(tree, model, table, queries, K)
        assert (status == 1).sum() >= 2 * len(members) - 1 and (status == 0).sum() >= len(members)
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. alignment
@pytest.mark.parametrize("K", [4, 5])
def test_alignment_sweep(ctx, W, K):
    depth = 3
    tree = ctx.merkle_tree(depth)
    try:
        for length in (2 * K, 2 * K + 1, 55, 64, 65):
            rng = np.random.default_rng(12200 + 100 * K + length)
            members = sorted({rng.bytes(K) for _ in range(7)})
            records = _table(W, members, K, depth, length, rng)
            perm = rng.permutation(8)
            records = [records[i] for i in perm]  # the last record of the allocation is then a live one in most cases
            model = IndexedModel(records, K)
            queries = _edge_queries(records, K)
            want = model.answers(queries)  # once: the alignment does not enter it
            keys = _keys(queries, K)
            for stride in (length, length + 5):
                for off in range(4):
                    table = _setup(ctx, tree, records, stride=stride, off=off)
                    assert table.view.data_ptr() % 4 == off
                    rows, index, status = tree.absent_rows(table.view, keys)
                    what = (K, length, stride, off)
                    assert np.array_equal(index, want[0]) and np.array_equal(status, want[1]) and np.array_equal(rows, want[2]), what
                    table.holds(records, what)
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. shapes
def _gapped_set(rng, n, K):
    """n random members outside [0x40.., 0xC0..): one record's range holds every key whose first byte is in [0x40, 0xC0)"""
    out = set()
    while len(out) < n:
        k = rng.bytes(K)
        if not 0x40 <= k[0] < 0xC0 and k not in (bytes(K), b"\xff" * K):
            out.add(k)
    return sorted(out)


@pytest.mark.parametrize("depth", [8, 9])
def test_workgroup_boundary_and_cooperative_fill(ctx, W, depth):
    K, length, nq = 8, 21, 257
    rng = np.random.default_rng(12300 + depth)
    members = _gapped_set(rng, (1 << depth) - 1, K)
    records = _table(W, members, K, depth, length, rng)
    model = IndexedModel(records, K)
    in_gap = lambda: bytes([int(rng.integers(0x40, 0xC0))]) + rng.bytes(K - 1)  # noqa: E731
    tree = ctx.merkle_tree(depth)
    try:
        table = _setup(ctx, tree, records, stride=length + 1, off=2)
        # duplicates: 257 draws from 40 keys, members among them
        pool = [members[int(i)] for i in rng.integers(0, len(members), size=15)] + [rng.bytes(K) for _ in range(20)] + [in_gap() for _ in range(5)]
        queries = [pool[int(i)] for i in rng.integers(0, len(pool), size=nq)]
        status = _check(tree, model, table, queries, (depth, "duplicates"), tree_too=True)
        assert (status == 1).any() and (status == 0).any() and len(set(queries)) < 41
        # every query in ONE range
        queries = [in_gap() for _ in range(nq)]
        want_i, _, _ = model.answers(queries)
        assert len(set(queries)) == nq and len(set(want_i.tolist())) == 1
        _check(tree, model, table, queries, (depth, "one range"))
        # 65 in that range (more than one stride of the wave), the rest spread over the others
        queries = [in_gap() for _ in range(65)] + [rng.bytes(K) for _ in range(nq - 65)]
        queries = [queries[int(i)] for i in rng.permutation(nq)]
        want_i, _, _ = model.answers(queries)
        assert np.bincount(want_i).max() >= 65 and len(set(want_i.tolist())) > 32
        _check(tree, model, table, queries, (depth, "65 in one range"))
    finally:
        tree.close()


def test_random_set_depth_12(ctx, W):
    depth, K, length, nq = 12, 8, 24, 300
    rng = np.random.default_rng(12400)
    members = sorted({rng.bytes(K) for _ in range(3000)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    model = IndexedModel(records, K)
    queries = [members[int(i)] for i in rng.integers(0, len(members), size=nq // 2)] + [rng.bytes(K) for _ in range(nq - nq // 2)]
    queries = [queries[int(i)] for i in rng.permutation(nq)]
    tree = ctx.merkle_tree(depth)
    try:
        table = _setup(ctx, tree, records, stride=length + 9, off=3)
        status = _check(tree, model, table, queries, "depth 12")
        assert (status == 1).sum() == nq // 2 and (status == 0).sum() == nq - nq // 2
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. unsorted layout, inserts
def test_shuffled_positions_and_inserts(ctx, W):
    depth, K, length = 6, 5, 17
    rng = np.random.default_rng(12500)
    members = sorted({rng.bytes(K) for _ in range(40)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    model = IndexedModel(records, K)
    tree = ctx.merkle_tree(depth)
    try:
        table = _setup(ctx, tree, records, stride=length + 2, off=1)
        fresh = [rng.bytes(K) for _ in range(12)]
        queries = _edge_queries(records, K) + fresh
        _check(tree, model, table, queries, "shuffled", tree_too=True)
        # insert the twelve fresh keys, one at a time: each is located on the device, the two updates go through update_records
        for n, key in enumerate(fresh):
            index, status = tree.locate_keys(table.view, _keys([key], K))
            assert status[0] == 0
            p = int(index[0])
            free = next(i for i, r in enumerate(records) if not r[:K] < r[K: 2 * K])
            idx, new = W.indexed_insert(records[p], p, key, free, payload=rng.bytes(length - 2 * K))
            assert idx == [p, free]
            tree.update_records(table.view, idx, new)
            for i, r in zip(idx, new):
                records[i] = r.tobytes()
            if n % 4 == 3 or n == len(fresh) - 1:
                model = IndexedModel(records, K)
                status = _check(tree, model, table, queries, ("after insert", n), tree_too=True)
                assert (status[-len(fresh):][: n + 1] == 1).all() and (status[-len(fresh):][n + 1:] == 0).all()
        assert sum(r[:K] < r[K: 2 * K] for r in records) == 1 + 40 + 12
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. malformed tables
def _raw(ctx, tree, table, K, keys, rows, index, status, stride=None):
    vp = ctypes.c_void_p
    return ctx.lib.mfh_merkle_absent_rows(ctx._h, tree._h, vp(table.view.data_ptr()), table.stride, table.length, K, len(keys), vp(keys.ctypes.data), keys.shape[1],
                                          vp(rows.ctypes.data) if rows is not None else None, (rows.shape[1] if stride is None else stride) if rows is not None else 0,
                                          vp(index.ctypes.data), vp(status.ctypes.data))


def test_malformed_tables(ctx):
    depth, K, length = 3, 2, 6
    rng = np.random.default_rng(12600)
    rec = lambda lo, hi: _key(lo, K) + _key(hi, K) + rng.bytes(length - 2 * K)  # noqa: E731
    # records 2 and 5 overlap in (0x3000, 0x4000); nothing covers [0x6000, 0x7000]; records 1 and 7 both carry the key 0x1000
    records = [bytes(length), rec(0x1000, 0x2000), rec(0x2000, 0x4000), rec(0x9000, 0x8000), rec(0, 0x1000), rec(0x3000, 0x6000), rec(0x7000, 0xFFFF), rec(0x1000, 0x1800)]
    model = IndexedModel(records, K)
    queries = [_key(x, K) for x in (0x3800, 0x3000, 0x6000, 0x6800, 0x7000, 0x1400, 0x1000, 0x8800, 0x2800, 0x5000)]
    want_i, want_s, want_rows = model.answers(queries)
    assert want_i.tolist() == [2, 5, NONE, NONE, 6, 1, 1, 6, 2, 5] and want_s.tolist() == [0, 1, 2, 2, 1, 0, 1, 0, 0, 0]
    tree = ctx.merkle_tree(depth)
    try:
        table = _setup(ctx, tree, records, stride=length + 1, off=1)
        _check(tree, model, table, queries, "malformed", tree_too=True)
        # a status 2 row: the 32 zero bytes and q are written, nothing else of the row
        keys = _keys(queries, K)
        rowb = _row_bytes(K, length, depth)
        rows = np.full((len(queries), rowb + 7), 0xAB, dtype=np.uint8)
        index, status = np.zeros(len(queries), dtype=np.uint32), np.zeros(len(queries), dtype=np.uint8)
        assert _raw(ctx, tree, table, K, keys, rows, index, status) == 0
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s)
        for k, s in enumerate(want_s):
            wrote = 32 + K if s == 2 else rowb
            assert np.array_equal(rows[k, :wrote], want_rows[k, :wrote]) and (rows[k, wrote:] == 0xAB).all(), k
        table.holds(records, "malformed, raw")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. miscellaneous
def test_locate_only_launch_counts_stride_and_scrub(ctx, W):
    depth, K, length, nq = 9, 8, 55, 300
    rng = np.random.default_rng(12700)
    members = sorted({rng.bytes(K) for _ in range(400)})
    records = _table(W, members, K, depth, length, rng)
    model = IndexedModel(records, K)
    queries = [members[int(i)] for i in rng.integers(0, 400, size=30)] + [rng.bytes(K) for _ in range(nq - 30)]
    keys = _keys(queries, K)
    want_i, want_s, want_rows = model.answers(queries)
    rowb = _row_bytes(K, length, depth)
    assert rowb == 385
    tree = ctx.merkle_tree(depth)
    try:
        table = _setup(ctx, tree, records, stride=length + 1)
        ctx.sync()
        ctx.set_timing(True)
        for kind in KINDS:
            ctx.timing_drain(kind)
        index, status = np.full(nq, 7, dtype=np.uint32), np.full(nq, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, keys, None, index, status) == 0  # locate only
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s)
        launches, ms, rows = ctx.timing_drain("merkle_locate")
        assert (launches, rows) == (1, 1 << depth)
        assert ctx.timing_drain("merkle_paths")[0] == 0 and ctx.timing_drain("merkle_absent_rows")[0] == 0
        buf = np.full((nq, rowb + 13), 0xAB, dtype=np.uint8)
        index[:], status[:] = 7, 7
        assert _raw(ctx, tree, table, K, keys, buf, index, status) == 0
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s)
        assert np.array_equal(buf[:, :rowb], want_rows) and (buf[:, rowb:] == 0xAB).all()
        l_launches, l_ms, l_rows = ctx.timing_drain("merkle_locate")
        g_launches, g_ms, g_rows = ctx.timing_drain("merkle_absent_rows")
        p_launches, p_ms, p_rows = ctx.timing_drain("merkle_paths")
        assert (l_launches, l_rows) == (1, 1 << depth) and (g_launches, g_rows) == (1, nq) and (p_launches, p_rows) == (1, nq)
        print(f"depth {depth}: {nq} queries: locate {l_ms:.3f} ms, gather {g_ms:.3f} ms, paths {p_ms:.3f} ms")
        assert ctx.timing_drain("merkle_level")[0] == 0 and ctx.timing_drain("sha256_records")[0] == 0
        ctx.set_timing(False)
        # the pinned staging zeroed between two calls: the same rows
        assert ctx.scrub_staging() == 0
        rows2, index2, status2 = tree.absent_rows(table.view, keys)
        assert np.array_equal(rows2, want_rows) and np.array_equal(index2, want_i) and np.array_equal(status2, want_s)
        bits, _, _ = tree.absent_bits(table.view, keys[:3])
        assert bits.shape == (3, 256 + 8 * K + 8 * length + 257 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows[:3])
        table.holds(records, "misc")
        _assert_tree(tree, model.levels, "misc")
    finally:
        ctx.set_timing(False)
        tree.close()


def _late_table(ctx, W):
    depth, K, length = 9, 4, 16
    rng = np.random.default_rng(12800)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = _table(W, members, K, depth, length, rng)
    model = IndexedModel(records, K)
    queries = [members[int(i)] for i in rng.integers(0, 300, size=10)] + [rng.bytes(K) for _ in range(54)]
    want = model.answers(queries)  # (first: nothing of the host's stands between the late table and the calls)
    keys = _keys(queries, K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        rows, index, status = tree.absent_rows(table.view, keys)
        assert np.array_equal(index, want[0]) and np.array_equal(status, want[1]) and np.array_equal(rows, want[2])
        table.holds(records, "late table")
        _assert_tree(tree, model.levels, "late table")
    finally:
        tree.close()


def test_ordering_null_stream(ctx, W):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_table(ctx, W)


def test_ordering_callers_stream(gpu_ctx_factory, mf, W):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_table(c, W)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 8. two chunks
def test_two_chunks(ctx, W):
    depth, K, length, nq = 1, 4, 65521, 1030
    rowb = _row_bytes(K, length, depth)
    per_chunk = (64 << 20) // rowb
    assert rowb == 65590 and per_chunk == 1023
    rng = np.random.default_rng(12900)
    member = _key(0x80000000, K)
    records = _table(W, [member], K, depth, length, rng)
    model = IndexedModel(records, K)
    queries = [rng.bytes(K) for _ in range(nq)]
    queries[per_chunk - 2: per_chunk + 2] = [_key(x, K) for x in (0x10, 0x90000000, 0x20, 0xA0000000)]  # both records on both sides of the seam
    queries[-1] = member
    want_i, want_s, want_rows = model.answers(queries)
    assert set(want_i[:per_chunk].tolist()) == set(want_i[per_chunk:].tolist()) == {0, 1} and want_s[-1] == 1
    tree = ctx.merkle_tree(depth)
    try:
        table = _setup(ctx, tree, records, stride=length + 2, off=1)
        ctx.sync()
        ctx.set_timing(True)
        for kind in KINDS:
            ctx.timing_drain(kind)
        rows, index, status = tree.absent_rows(table.view, _keys(queries, K))
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s) and np.array_equal(rows, want_rows)
        assert ctx.timing_drain("merkle_locate")[::2] == (1, 2)
        assert ctx.timing_drain("merkle_absent_rows")[::2] == (2, nq)
        assert ctx.timing_drain("merkle_paths")[::2] == (2, nq)
        table.holds(records, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. MFH_EINVAL
def test_einval(ctx, mf, W):
    import torch

    lib, h = ctx.lib, ctx._h
    depth, K, length = 3, 4, 17
    rng = np.random.default_rng(13000)
    members = sorted({rng.bytes(K) for _ in range(5)})
    records = _table(W, members, K, depth, length, rng)
    model = IndexedModel(records, K)
    rowb = _row_bytes(K, length, depth)
    tree = ctx.merkle_tree(depth)
    texts = []

    def refused(rc, handle=h):
        assert rc == EINVAL
        text = lib.mfh_last_error(handle).decode()
        assert text.startswith("mfh_merkle_absent_rows: "), text
        texts.append(text)

    try:
        table = _setup(ctx, tree, records, stride=length + 3, off=1)
        ctx.sync()
        ctx.set_timing(True)
        for kind in KINDS:
            ctx.timing_drain(kind)
        vp = ctypes.c_void_p
        keys = _keys([rng.bytes(K) for _ in range(3)], K)
        zero, ones = keys.copy(), keys.copy()
        zero[1], ones[2] = 0, 0xFF
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        index, status = np.full(3, 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        kp, zp, op, bp, ip, sp = (vp(a.ctypes.data) for a in (keys, zero, ones, buf, index, status))
        tp, ts, stride = vp(table.view.data_ptr()), table.stride, buf.shape[1]
        f = lib.mfh_merkle_absent_rows
        refused(f(h, None, tp, ts, length, K, 3, kp, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, ts, length, 0, 3, kp, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, ts, 66, 33, 3, kp, 33, bp, 1 << 12, ip, sp))
        texts.pop()  # (key_bytes 0 and 33: one text)
        refused(f(h, tree._h, tp, ts, 2 * K - 1, K, 3, kp, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, (1 << 20) + 1, (1 << 20) + 1, K, 3, kp, K, bp, 1 << 22, ip, sp))
        refused(f(h, tree._h, tp, length - 1, length, K, 3, kp, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K - 1, bp, stride, ip, sp))
        refused(f(h, tree._h, None, ts, length, K, 3, kp, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, None, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, bp, stride, None, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, bp, stride, ip, None))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, bp, rowb - 1, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, zp, K, bp, stride, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, op, K, bp, stride, ip, sp))
        texts.pop()  # (the two sentinels: one text)
        refused(f(h, tree._h, tp, ts, length, K, 3, zp, K, None, 0, ip, sp))  # locate only refuses a sentinel too
        texts.pop()
        assert f(None, tree._h, tp, ts, length, K, 3, kp, K, bp, stride, ip, sp) == EINVAL
        assert len(set(texts)) == len(texts) == 12, sorted(texts)
        if torch.cuda.device_count() > 1:
            other = mf.Context(mf.DEBUG, 1)
            try:
                assert f(other._h, tree._h, tp, ts, length, K, 3, kp, K, bp, stride, ip, sp) == EINVAL
                assert lib.mfh_last_error(other._h).decode() == "mfh_merkle_absent_rows: the tree belongs to another device"
            finally:
                other.close()
                torch.cuda.set_device(ctx.device)
        # nq = 0 does nothing, whatever the pointers; in_stride is not looked at without h_inputs
        assert f(h, tree._h, None, ts, length, K, 0, None, K, None, 0, None, None) == 0
        assert f(h, tree._h, tp, ts, length, K, 0, kp, K, bp, stride, ip, sp) == 0
        none = np.zeros((0, K), dtype=np.uint8)
        rows0, index0, status0 = tree.absent_rows(table.view, none)
        assert rows0.shape == (0, rowb) and index0.shape == (0,) and status0.shape == (0,)
        assert tree.absent_bits(table.view, none)[0].shape == (0, 256 + 8 * K + 8 * length + 257 * depth)
        assert [a.shape for a in tree.locate_keys(table.view, none)] == [(0,), (0,)]
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (index == 0xCDCDCDCD).all() and (status == 0xCD).all()
        for kind in KINDS:
            assert ctx.timing_drain(kind)[0] == 0, kind
        ctx.set_timing(False)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
        for bad_table, bad_keys in [(table.view, keys[0]), (table.view, keys.astype(np.int8)), (table.view, zero), (table.view, np.zeros((1, 9), dtype=np.uint8) + 1),
                                    (table.view, np.zeros((1, 0), dtype=np.uint8)), (table.view[:4], keys), (table.view.cpu().numpy(), keys),
                                    (table.view.to(torch.int8), keys), (table.view.t(), keys)]:
            for call in (tree.locate_keys, tree.absent_rows, tree.absent_bits):
                with pytest.raises(mf.MfhError):
                    call(bad_table, bad_keys)
        _assert_tree(tree, model.levels, "after the refused Python calls")
        table.holds(records, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 10. end to end
def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth = 4, 8, 1
    st = W.MerkleAbsent(K, length, depth)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == st.lu == 288 and (cc.nwires, cc.nrows) == W.MERKLE_ABSENT_SIZES[(K, length, depth)]
    rng = np.random.default_rng(13100)
    member = _key(0x6789ABCD, K)
    records = _table(W, [member], K, depth, length, rng)
    model = IndexedModel(records, K)
    absent = [_key(x, K) for x in (1, 0x6789ABCC, 0x6789ABCE, 0xFFFFFFFE)]
    tree = ctx.merkle_tree(depth)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        table = _setup(ctx, tree, records, stride=length + 1, off=3)
        root = tree.root()
        assert root == model.root()
        want_i, want_s, want_rows = model.answers(absent + [member])
        bits, index, status = tree.absent_bits(table.view, _keys(absent + [member], K))
        assert bits.shape == (5, 256 + 8 * K + 8 * length + 257 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows)
        assert index.tolist() == want_i.tolist() == [0, 0, 1, 1, 1] and status.tolist() == want_s.tolist() == [0, 0, 0, 0, 1]
        witness, holds = ctx.circuit_assign(prog, bits)
        assert holds.tolist() == [True] * 4 + [False]
        for k in range(5):
            assert st.root_of(witness[k]) == root, k
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count[:4].any() and (first[:4] == 0xFFFFFFFF).all()
        assert count[4] > 0 and first[4] != 0xFFFFFFFF  # the member's row: lo < q is violated

        ctx.ssp_prepare(None)
        alpha, beta, s = (int(x) for x in rng.integers(1, C.P, size=3, dtype=np.uint64))
        d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
        d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
        d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()
        vk = ctx.derive_vk(None, s, lu)
        deltas = [int(x) for x in rng.integers(0, C.P, size=4, dtype=np.uint64)]
        mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(4)]
        signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(4)]
        proofs = ctx.prove_batch_public(d_crs, None, lu, [witness[k].tobytes() for k in range(4)], deltas, mags, signs).clone()

        def verify(statements):
            return [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, statements), np.uint8)]

        own = [st.statement(root, q) for q in absent]
        assert all(len(x) == lu // 8 for x in own) and own == [witness[k][: lu // 8].tobytes() for k in range(4)]
        assert verify(own) == [True] * 4
        assert verify(own[1:] + own[:1]) == [False] * 4  # each under another absent key
        assert verify([st.statement(root, member)] * 4) == [False] * 4
        assert verify([st.statement(_flip(root, 77), q) for q in absent]) == [False] * 4
        table.holds(records, "end to end")
    finally:
        prog.close()
        tree.close()
