"""GPU: range reads of an indexed table (mfh_merkle_range_rows, mfh_merkle_range_rows_cut; k_range_flags, k_range_keys, k_range_order; MerkleTree.count_range /
range_rows / range_segments) against tests/merkle_range_model.py, a pure-Python model over tests/sha256_ref.py: count, index, keys, rows and nodes byte for byte.

1. depth 3, (4, 8) records, 5 members in shuffled slots and 2 garbage inert slots: EVERY pair lo <= hi of the probe set (members, members +- 1, 1, max - 1),
   uncut and under the cuts [1], [2], [1, 2] -- count, index, keys, rows, nodes, status 0, the root.
2. key widths 1, 5, 8 and 32 at depth 4 (a partial last word; KW = 1, 2 and 8), (8, 55) in a misaligned strided table.
3. tile, wave and workgroup edges of the order kernel: depth 10, random members in random slots, ranges of exactly 1, 63, 64, 65, 255, 256, 257 and 600 links
   (600: three LDS tiles, three workgroups).
4. the whole table: depth 12, 4 095 members, [00..01, FF..FE] -- 4 096 links: index and keys against the model, rows against record_rows, and a 50-link slice.
5. overflow: max_links = n - 1 is status 1 with the right count and untouched outputs, max_links = n status 0; count_range alone.
6. malformed tables give status 2 with the model's order and no rows: a duplicated lo (the tie breaks by slot), a gap, an overlap, no record below lo, no
   link at all.
7. two chunks: depth 11, (4, 65 521) records (a 134 MB table), 1 030 links -- 1 018 + 12 rows by update_chunk at this depth's row of 65 907 bytes.
8. launch counts by timing kind, wider strides, scrubbed staging.
9. every refusal leaves tree and table byte-identical and launches nothing.
10. a table produced late on the stream, on the null stream and on a caller's.
11. end to end at d = 2^17: MerkleLink(4, 9, 1, reveal=1) + MerkleClimb(1) on a depth-2 table with two members, a range holding both (three links), proved by
    prove_batch_public and verified against statements built from the nodes, the bounds, the returned keys and the shown bytes ALONE; rejected in another
    order and under a flipped root; no proof verifies the merged link of a claim that omits k_1."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

import merkle_climb_model as CM
import merkle_range_model as R
from test_gpu_merkle import _assert_tree, _flip
from test_gpu_merkle_record_update import Placed
from test_gpu_merkle_segments import _prover, _witnesses

pytestmark = pytest.mark.gpu

SEED = bytes((59 * i + 13) & 0xFF for i in range(40))
EINVAL = -1
KINDS = ("merkle_range", "merkle_range_order", "merkle_absent_rows", "merkle_paths", "merkle_climb_rows", "merkle_locate", "merkle_inert", "merkle_updates",
         "merkle_level", "sha256_records")
CUTS3 = [[1], [2], [1, 2]]


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


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), (what, g)


def _counts(ctx):
    return {kind: ctx.timing_drain(kind)[0] for kind in KINDS}


def _model(records):
    return CM.ClimbModel([hashlib.sha256(bytes(r)).digest() for r in records])


def _check_uncut(tree, view, records, K, lo, hi, model, what, max_links=None):
    want_rows, want_i, want_k, want_s, count = R.range_rows(records, K, lo, hi, model=model)
    assert tree.count_range(view, lo, hi) == count, what
    rows, index, keys, status = tree.range_rows(view, lo, hi, max_links)
    assert index.dtype == np.uint32 and keys.dtype == np.uint8 and rows.dtype == np.uint8 and status == want_s, (what, status, want_s)
    assert np.array_equal(index, want_i), (what, index, want_i)
    assert keys.shape == want_k.shape and np.array_equal(keys, want_k), what
    assert rows.shape == want_rows.shape and np.array_equal(rows, want_rows), what
    return rows, index, keys, status


def _check_cut(tree, view, records, K, lo, hi, cuts, model, what, max_links=None):
    want_rows, want_nodes, want_i, want_k, want_s, _ = R.range_segments(records, K, lo, hi, cuts, model=model)
    rows, nodes, index, keys, status = tree.range_segments(view, lo, hi, cuts, max_links)
    assert status == want_s and np.array_equal(index, want_i) and keys.shape == want_k.shape and np.array_equal(keys, want_k), what
    _same(rows, want_rows, what)
    assert nodes.shape == want_nodes.shape and np.array_equal(nodes, want_nodes), what
    assert all(nodes[i, -1].tobytes() == tree.root() == model.root() for i in range(len(nodes))), what
    return rows, nodes, index, keys, status


class Table:
    """a model table on the device with its tree: records (bytes), members, the Placed table, the tree and the tree's model"""

    def __init__(self, ctx, rng, K, length, depth, nmembers, garbage=2, stride=None, off=0, late=False):
        table, self.members = R.make_table(rng, K, length, depth, nmembers, garbage)
        self.K, self.length, self.depth = K, length, depth
        self.records = [r.tobytes() for r in table]
        self.model = _model(self.records)
        self.tree = ctx.merkle_tree(depth)
        self.placed = Placed(ctx, self.records, stride=stride, off=off, late=late)
        self.view = self.placed.view
        self.tree.set_records(0, self.view)

    def unchanged(self, what):
        self.placed.holds(self.records, what)
        _assert_tree(self.tree, self.model.levels, what)

    def close(self):
        self.tree.close()


# ---------------------------------------------------------------------------------------------------------------- 1. depth 3, every probe pair
@pytest.fixture(scope="module")
def table3(ctx):
    t = Table(ctx, np.random.default_rng(19000), 4, 8, 3, 5, stride=11, off=1)
    yield t
    t.close()


def test_depth_3_every_probe_pair_uncut(table3):
    t = table3
    probes = R.probes(t.members, t.K)
    assert len(probes) >= 12 and t.view.data_ptr() % 4 == 1
    sizes = set()
    for i, lo in enumerate(probes):
        for hi in probes[i:]:
            rows, index, keys, status = _check_uncut(t.tree, t.view, t.records, t.K, lo, hi, t.model, (lo, hi))
            assert status == 0 and [k.tobytes() for k in keys[1:, 0]] == [m for m in t.members if lo <= m <= hi]
            sizes.add(len(index))
    assert sizes == {1, 2, 3, 4, 5, 6}
    lo, hi = probes[0], probes[-1]
    bits, index, keys, status = t.tree.range_bits(t.view, lo, hi)
    assert bits.shape == (6, 256 + 64 + 257 * 3) and status == 0
    assert np.array_equal(np.packbits(bits, axis=1, bitorder="little"), R.range_rows(t.records, t.K, lo, hi, model=t.model)[0])
    t.unchanged("depth 3, uncut")


@pytest.mark.parametrize("cuts", CUTS3)
def test_depth_3_every_probe_pair_cut(table3, cuts):
    t = table3
    probes = R.probes(t.members, t.K)
    for i, lo in enumerate(probes):
        for hi in probes[i:]:
            status = _check_cut(t.tree, t.view, t.records, t.K, lo, hi, cuts, t.model, (cuts, lo, hi))[4]
            assert status == 0
    lo, hi = probes[0], probes[-1]
    bits, nodes, index, keys, status = t.tree.range_segment_bits(t.view, lo, hi, cuts)
    lv = [b - a for a, b in CM.ranges(3, cuts)]
    assert [b.shape for b in bits] == [(6, 256 + 64 + 257 * lv[0])] + [(6, 512 + 257 * x) for x in lv[1:]]
    _same([np.packbits(b, axis=1, bitorder="little") for b in bits], R.range_segments(t.records, t.K, lo, hi, cuts, model=t.model)[0], "bits")
    t.unchanged(("depth 3", cuts))


# ---------------------------------------------------------------------------------------------------------------- 2. key widths
@pytest.mark.parametrize("K,length,stride,off", [(1, 2, 3, 1), (5, 13, 14, 3), (8, 55, 58, 1), (32, 64, 67, 2)])
def test_key_widths(ctx, K, length, stride, off):
    t = Table(ctx, np.random.default_rng(19100 + K), K, length, 4, 11, garbage=3, stride=stride, off=off)
    try:
        assert t.view.data_ptr() % 4 == off and t.placed.stride % 4 != 0
        probes = R.probes(t.members, K)
        pairs = [(probes[i], probes[j]) for i in range(0, len(probes), 3) for j in range(i, len(probes), 5)] + [(probes[0], probes[-1]), (t.members[4], t.members[4])]
        seen = set()
        for lo, hi in pairs:
            rows, index, keys, status = _check_uncut(t.tree, t.view, t.records, K, lo, hi, t.model, (K, lo, hi))
            assert status == 0
            seen.add(len(index))
        assert max(seen) == 12 and len(seen) > 3
        for lo, hi in pairs[::4]:
            assert _check_cut(t.tree, t.view, t.records, K, lo, hi, [1, 3], t.model, (K, "cut", lo, hi))[4] == 0
        # a present-key lookup is the range [k, k]: link 1 is (k, successor) and carries k's payload
        k = t.members[4]
        rows, index, keys, status = t.tree.range_rows(t.view, k, k)
        assert status == 0 and keys[:, 0].tobytes() == t.members[3] + k and keys[:, 1].tobytes() == k + t.members[5]
        assert rows[1, 32: 32 + length].tobytes() == t.records[int(index[1])] and t.records[int(index[1])][:K] == k
        t.unchanged(("key width", K))
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the order kernel's edges
@pytest.fixture(scope="module")
def table10(ctx):
    t = Table(ctx, np.random.default_rng(19200), 4, 12, 10, 700, garbage=40, stride=13, off=2)
    yield t
    t.close()


def _range_of(t, n, start):
    """bounds of a range of exactly n links: n - 1 members from members[start] on; n = 1: a non-member between two members"""
    if n == 1:
        v = int.from_bytes(t.members[start], "big") + 1
        assert v.to_bytes(t.K, "big") not in t.members
        return v.to_bytes(t.K, "big"), v.to_bytes(t.K, "big")
    return t.members[start], t.members[start + n - 2]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_order_kernel_edges(table10, n):
    t = table10
    lo, hi = _range_of(t, n, 37)
    rows, index, keys, status = _check_uncut(t.tree, t.view, t.records, t.K, lo, hi, t.model, n)
    assert status == 0 and len(index) == n
    assert n < 3 or index.tolist() != sorted(index.tolist())  # table order is not key order
    _check_uncut(t.tree, t.view, t.records, t.K, lo, hi, t.model, (n, "given"), max_links=n)
    _check_uncut(t.tree, t.view, t.records, t.K, lo, hi, t.model, (n, "room"), max_links=n + 300)
    if n in (1, 65, 600):
        _check_cut(t.tree, t.view, t.records, t.K, lo, hi, [3, 8], t.model, (n, "cut"))
    t.unchanged(("edges", n))


# ---------------------------------------------------------------------------------------------------------------- 4. the whole table
def test_whole_table(ctx):
    K, length, depth = 4, 8, 12
    t = Table(ctx, np.random.default_rng(19300), K, length, depth, 4095, garbage=0)
    try:
        lo, hi = b"\0\0\0\1", b"\xff\xff\xff\xfe"
        order = R.links(t.records, K, lo, hi)
        assert len(order) == 4096 and R.status(t.records, K, lo, hi, order) == 0
        assert t.tree.count_range(t.view, lo, hi) == 4096
        rows, index, keys, status = t.tree.range_rows(t.view, lo, hi)
        assert status == 0 and np.array_equal(index, np.array(order, dtype=np.uint32)) and np.array_equal(keys, R.keys_of(t.records, K, order))
        assert sorted(index.tolist()) == list(range(4096))
        given = np.frombuffer(b"".join(t.records[s] for s in order), dtype=np.uint8).reshape(4096, length)
        assert np.array_equal(rows, t.tree.record_rows(given, order))
        # a 50-link slice of it
        a, b = t.members[2000], t.members[2048]
        rows50, index50, keys50, status50 = t.tree.range_rows(t.view, a, b)
        assert status50 == 0 and index50.tolist() == order[2000: 2050] and np.array_equal(keys50, keys[2000: 2050])
        assert np.array_equal(rows50, t.tree.record_rows(given[2000: 2050], order[2000: 2050])) and np.array_equal(rows50, rows[2000: 2050])
        _assert_tree(t.tree, t.model.levels, "whole table")
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------------- 5. overflow
def _raw(ctx, t, lo, hi, max_links, extra=0, cuts=None, fill=0xAB):
    """the C call with outputs of 0xAB: (rc, count, status, index, keys, rows or the list of row arrays)"""
    vp = ctypes.c_void_p
    a, b = np.frombuffer(lo, dtype=np.uint8), np.frombuffer(hi, dtype=np.uint8)
    count = ctypes.c_uint32(0xCDCDCDCD)
    status = np.full(1, 0xCD, dtype=np.uint8)
    index = np.full(max_links, 0xABABABAB, dtype=np.uint32)
    keys = np.full((max_links, 2, t.K), fill, dtype=np.uint8)
    head = (ctx._h, t.tree._h, vp(t.view.data_ptr()), t.placed.stride, t.length, t.K, vp(a.ctypes.data), vp(b.ctypes.data), max_links, ctypes.byref(count),
            vp(index.ctypes.data), vp(keys.ctypes.data))
    if cuts is None:
        rows = np.full((max_links, 32 + t.length + 32 * t.depth + (t.depth + 7) // 8 + extra), fill, dtype=np.uint8)
        rc = ctx.lib.mfh_merkle_range_rows(*head, vp(rows.ctypes.data), rows.shape[1], vp(status.ctypes.data))
    else:
        segs = CM.ranges(t.depth, cuts)
        widths = [32 + t.length + 32 * cuts[0] + (cuts[0] + 7) // 8] + [CM.climb_row_bytes(y - x) for x, y in segs[1:]]
        rows = [np.full((max_links, w + extra), fill, dtype=np.uint8) for w in widths]
        ptrs = (vp * len(rows))(*[r.ctypes.data for r in rows])
        strides = (ctypes.c_size_t * len(rows))(*[r.shape[1] for r in rows])
        cu = np.array(cuts, dtype=np.uint32)
        rc = ctx.lib.mfh_merkle_range_rows_cut(*head, len(cuts), vp(cu.ctypes.data), ptrs, strides, vp(status.ctypes.data))
    return rc, int(count.value), int(status[0]), index, keys, rows


def test_overflow(ctx, mf, table10):
    t = table10
    n = 65
    lo, hi = _range_of(t, n, 200)
    assert t.tree.count_range(t.view, lo, hi) == n
    for cuts in (None, [4]):
        rc, count, status, index, keys, rows = _raw(ctx, t, lo, hi, n - 1, cuts=cuts)
        assert (rc, count, status) == (0, n, 1)
        assert (index == 0xABABABAB).all() and (keys == 0xAB).all() and all((r == 0xAB).all() for r in (rows if cuts else [rows]))
        rc, count, status, index, keys, rows = _raw(ctx, t, lo, hi, n, cuts=cuts)
        assert (rc, count, status) == (0, n, 0) and np.array_equal(index, np.array(R.links(t.records, t.K, lo, hi), dtype=np.uint32))
    rows, index, keys, status = t.tree.range_rows(t.view, lo, hi, max_links=n - 1)
    assert status == 1 and rows.shape == (0, 32 + 12 + 320 + 2) and index.shape == (0,) and keys.shape == (0, 2, 4)
    rows, nodes, index, keys, status = t.tree.range_segments(t.view, lo, hi, [4], max_links=1)
    assert status == 1 and [r.shape[0] for r in rows] == [0, 0] and nodes.shape == (0, 2, 32) and index.shape == (0,)
    # the count query writes the count and the status alone: status 1 when there is a link (count > max_links = 0)
    rc, count, status, _, _, _ = _raw(ctx, t, lo, hi, 0)
    assert (rc, count, status) == (0, n, 1)
    for bad in (-1, 1.5, "3"):
        with pytest.raises(mf.MfhError):
            t.tree.range_rows(t.view, lo, hi, max_links=bad)
    t.unchanged("overflow")


# ---------------------------------------------------------------------------------------------------------------- 6. malformed tables
MALFORMED = {
    # name: (records as (lo, hi), lo, hi, the slots in the model's order)
    "a duplicated lo": ([(0x2000, 0xFFFF), (0x1000, 0x2000), (0, 0), (0, 0x1000), (0x1000, 0x2000), (5, 5), (9, 3), (0, 0)], 0x0800, 0x2800, [3, 1, 4, 0]),
    "a gap": ([(0x3000, 0xFFFF), (0, 0), (0x1000, 0x2000), (0, 0x1000), (0, 0), (0, 0), (0, 0), (0, 0)], 0x0800, 0x3800, [3, 2, 0]),
    "an overlap": ([(0x1000, 0x3000), (0x2000, 0xFFFF), (0, 0x1000), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)], 0x0800, 0x3800, [2, 0, 1]),
    "no record below lo": ([(0x2000, 0xFFFF), (0x1000, 0x2000), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)], 0x0800, 0x1800, [1]),
    "no link at all": ([(0x2000, 0xFFFF), (0x1000, 0x2000), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)], 0x0100, 0x0200, []),
    "the last hi not above hi": ([(0, 0x1000), (0x1000, 0x2000), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)], 0x0800, 0x2000, [0, 1]),
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_tables(ctx, name):
    recs, lo, hi, want_order = MALFORMED[name]
    K, length, depth = 2, 6, 3
    rng = np.random.default_rng(19400)
    key = lambda x: int(x).to_bytes(K, "big")  # noqa: E731
    records = [key(a) + key(b) + rng.bytes(length - 2 * K) for a, b in recs]
    lo, hi = key(lo), key(hi)
    assert R.links(records, K, lo, hi) == want_order and R.status(records, K, lo, hi, want_order) == 2

    class T:
        pass

    t = T()
    t.K, t.length, t.depth, t.records, t.model = K, length, depth, records, _model(records)
    t.tree = ctx.merkle_tree(depth)
    try:
        t.placed = Placed(ctx, records, stride=length + 1, off=3)
        t.view = t.placed.view
        t.tree.set_records(0, t.view)
        rows, index, keys, status = _check_uncut(t.tree, t.view, records, K, lo, hi, t.model, name)
        assert status == 2 and index.tolist() == want_order and rows.shape == (0, 32 + length + 96 + 1)
        for cuts in CUTS3:
            assert _check_cut(t.tree, t.view, records, K, lo, hi, cuts, t.model, (name, cuts))[4] == 2
        # raw: index and keys are written, no row is
        for cuts in (None, [1, 2]):
            rc, count, status, index, keys, rows = _raw(ctx, t, lo, hi, 6, cuts=cuts)
            n = len(want_order)
            assert (rc, count, status) == (0, n, 2) and index[:n].tolist() == want_order and (index[n:] == 0xABABABAB).all()
            assert np.array_equal(keys[:n], R.keys_of(records, K, want_order)) and (keys[n:] == 0xAB).all()
            assert all((r == 0xAB).all() for r in (rows if cuts else [rows]))
        t.placed.holds(records, name)
        _assert_tree(t.tree, t.model.levels, name)
    finally:
        t.tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. two chunks
@pytest.fixture(scope="module")
def table11(ctx):
    """depth 11, (4, 65 521) records: a 134 MB table, built once"""
    t = Table(ctx, np.random.default_rng(19500), 4, 65521, 11, 1500, garbage=20)
    yield t
    t.close()


def test_two_chunks(ctx, table11):
    t = table11
    n = 1030
    rowb = 32 + t.length + 32 * 11 + 2
    per_chunk = (64 << 20) // rowb
    assert rowb == 65907 and per_chunk == 1018 and per_chunk < n < 2 * per_chunk
    lo, hi = _range_of(t, n, 100)
    try:
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        rows, index, keys, status = _check_uncut(t.tree, t.view, t.records, t.K, lo, hi, t.model, "two chunks", max_links=n)
        assert status == 0 and len(index) == n
        assert ctx.timing_drain("merkle_paths")[::2] == (2, n)
        assert ctx.timing_drain("merkle_absent_rows")[::2] == (2, n)
        assert ctx.timing_drain("merkle_range")[::2] == (5, 2 << 11)           # the count query of the check, then the call
        assert ctx.timing_drain("merkle_range_order")[::2] == (2, 2 * n)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        # both sides of the seam hold their own records
        for i in (per_chunk - 1, per_chunk):
            assert rows[i, 32: 32 + 8].tobytes() == keys[i].tobytes() == t.records[int(index[i])][:8]
    finally:
        ctx.set_timing(False)


# ---------------------------------------------------------------------------------------------------------------- 8. launches, strides, scrub
def test_launch_counts_wider_strides_and_scrub(ctx, table10):
    t = table10
    n = 300
    lo, hi = _range_of(t, n, 50)
    want = R.range_rows(t.records, t.K, lo, hi, model=t.model)
    cuts = [3, 8]
    want_cut = R.range_segments(t.records, t.K, lo, hi, cuts, model=t.model)
    try:
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        assert t.tree.count_range(t.view, lo, hi) == n
        assert ctx.timing_drain("merkle_range")[::2] == (2, 1 << 10)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)
        rc, count, status, index, keys, rows = _raw(ctx, t, lo, hi, n + 7, extra=13)
        assert (rc, count, status) == (0, n, 0)
        launches, ms, total = ctx.timing_drain("merkle_range")
        print(f"depth 10, {n} links: flags + scan + select {ms:.3f} ms")
        assert (launches, total) == (3, 1 << 10)
        launches, ms, total = ctx.timing_drain("merkle_range_order")
        print(f"depth 10, {n} links: keys + order {ms:.3f} ms")
        assert (launches, total) == (2, 2 * (n + 7))
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_absent_rows": 1, "merkle_paths": 1}
        w = want[0].shape[1]
        assert np.array_equal(rows[:n, :w], want[0]) and (rows[:n, w:] == 0xAB).all() and (rows[n:] == 0xAB).all()
        assert np.array_equal(index[:n], want[1]) and (index[n:] == 0xABABABAB).all() and np.array_equal(keys[:n], want[2]) and (keys[n:] == 0xAB).all()
        # the cut call: the climb kernel in place of k_merkle_paths
        rc, count, status, index, keys, rows = _raw(ctx, t, lo, hi, n, extra=5, cuts=cuts)
        assert (rc, count, status) == (0, n, 0)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_range": 3, "merkle_range_order": 2, "merkle_absent_rows": 1, "merkle_climb_rows": 1}
        for g, r in enumerate(rows):
            w = want_cut[0][g].shape[1]
            assert np.array_equal(r[:, :w], want_cut[0][g]) and (r[:, w:] == 0xAB).all(), g
        # max_links = None asks for the count first: 2 + 3 launches
        t.tree.range_rows(t.view, lo, hi)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_range": 5, "merkle_range_order": 2, "merkle_absent_rows": 1, "merkle_paths": 1}
        # the pinned staging zeroed in between: the same rows
        assert ctx.scrub_staging() == 0
        _check_uncut(t.tree, t.view, t.records, t.K, lo, hi, t.model, "after the scrub", max_links=n)
        assert ctx.scrub_staging() == 0
        _check_cut(t.tree, t.view, t.records, t.K, lo, hi, cuts, t.model, "after the scrub, cut", max_links=n)
        _counts(ctx)
        ctx.set_timing(False)
        t.unchanged("launch counts")
    finally:
        ctx.set_timing(False)


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_einval(ctx, mf, table3):
    t = table3
    lib, h = ctx.lib, ctx._h
    K, length, depth = t.K, t.length, t.depth
    vp = ctypes.c_void_p
    texts = []

    def refused(rc, who):
        assert rc == EINVAL
        text = lib.mfh_last_error(h).decode()
        assert text.startswith(who + ": "), text
        texts.append(text)

    lo, hi = R.probes(t.members, K)[0], R.probes(t.members, K)[-1]
    a, b = (np.frombuffer(x, dtype=np.uint8) for x in (lo, hi))
    zero, ones = np.zeros(K, dtype=np.uint8), np.full(K, 0xFF, dtype=np.uint8)
    count = ctypes.c_uint32(0xCDCDCDCD)
    status = np.full(1, 0xCD, dtype=np.uint8)
    m = 6
    index, keys = np.full(m, 0xABABABAB, dtype=np.uint32), np.full((m, 2, K), 0xAB, dtype=np.uint8)
    rowb = 32 + length + 32 * depth + 1
    rows = np.full((m, rowb + 4), 0xAB, dtype=np.uint8)
    ap, bp, zp, op, ip, kp, rp, sp = (vp(x.ctypes.data) for x in (a, b, zero, ones, index, keys, rows, status))
    cp = ctypes.byref(count)
    tp, ts = vp(t.view.data_ptr()), t.placed.stride
    cuts = np.array([1, 2], dtype=np.uint32)
    widths = [32 + length + 32 + 1, 97, 97]
    seg = [np.full((m, w + 4), 0xAB, dtype=np.uint8) for w in widths]

    def outs(short=None, null=None):
        ptrs = (vp * 3)(*[None if g == null else s.ctypes.data for g, s in enumerate(seg)])
        strides = (ctypes.c_size_t * 3)(*[w - 1 if g == short else w + 4 for g, w in enumerate(widths)])
        return ptrs, strides

    try:
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        f, who = lib.mfh_merkle_range_rows, "mfh_merkle_range_rows"

        def call(tree=t.tree._h, table=tp, stride=ts, ln=length, kb=K, lo_=ap, hi_=bp, ml=m, cnt=cp, idx=ip, ks=kp, rws=rp, rstride=rowb + 4, st=sp):
            return f(h, tree, table, stride, ln, kb, lo_, hi_, ml, cnt, idx, ks, rws, rstride, st)

        assert call() == 0 and int(status[0]) == 0 and int(count.value) == 6  # the arguments are fine as they stand
        count.value, status[0] = 0xCDCDCDCD, 0xCD
        index[:], keys[:], rows[:] = 0xABABABAB, 0xAB, 0xAB
        _counts(ctx)
        refused(call(tree=None), who)
        refused(call(kb=0), who)
        refused(call(kb=33), who)
        texts.pop()
        refused(call(ln=2 * K - 1), who)
        refused(call(stride=(1 << 20) + 1, ln=(1 << 20) + 1), who)
        refused(call(stride=length - 1), who)
        refused(call(ml=(1 << 16) + 1), who)
        refused(call(rstride=rowb - 1), who)
        refused(call(table=None), who)
        refused(call(lo_=None), who)
        refused(call(hi_=None), who)
        refused(call(cnt=None), who)
        refused(call(st=None), who)
        refused(call(idx=None), who)
        refused(call(lo_=zp), who)
        refused(call(hi_=op), who)
        texts.pop()
        refused(call(lo_=op), who)
        texts.pop()
        refused(call(lo_=bp, hi_=ap), who)
        assert f(None, t.tree._h, tp, ts, length, K, ap, bp, m, cp, ip, kp, rp, rowb + 4, sp) == EINVAL
        assert len(set(texts)) == len(texts) == 15, sorted(texts)

        texts.clear()
        fc, who = lib.mfh_merkle_range_rows_cut, "mfh_merkle_range_rows_cut"
        ptrs, strides = outs()

        def cut(tree=t.tree._h, table=tp, stride=ts, ln=length, kb=K, lo_=ap, hi_=bp, ml=m, cnt=cp, idx=ip, ks=kp, nc=2, cu=vp(cuts.ctypes.data), p=ptrs, s=strides, st=sp):
            return fc(h, tree, table, stride, ln, kb, lo_, hi_, ml, cnt, idx, ks, nc, cu, p, s, st)

        refused(cut(tree=None), who)
        refused(cut(kb=0), who)
        refused(cut(ln=2 * K - 1), who)
        refused(cut(stride=length - 1), who)
        refused(cut(ml=(1 << 16) + 1), who)
        refused(cut(nc=0), who)
        refused(cut(cu=None), who)
        texts.pop()
        for bad in ([0, 2], [1, 3], [2, 2], [2, 1]):
            bc = np.array(bad, dtype=np.uint32)
            refused(cut(cu=vp(bc.ctypes.data)), who)
            if bad != [0, 2]:
                texts.pop()
        refused(cut(p=None), who)
        refused(cut(s=None), who)
        texts.pop()
        for g in range(3):
            p2, s2 = outs(null=g)
            refused(cut(p=p2, s=s2), who)
            p3, s3 = outs(short=g)
            refused(cut(p=p3, s=s3), who)
            if g:
                texts.pop()
                texts.pop()
        refused(cut(table=None), who)
        refused(cut(lo_=None), who)
        refused(cut(cnt=None), who)
        refused(cut(st=None), who)
        refused(cut(idx=None), who)
        refused(cut(hi_=zp), who)
        refused(cut(lo_=bp, hi_=ap), who)
        assert len(set(texts)) == len(texts) == 17, sorted(texts)

        # nothing was written, launched or changed
        assert (index == 0xABABABAB).all() and (keys == 0xAB).all() and (rows == 0xAB).all() and all((s == 0xAB).all() for s in seg)
        assert int(count.value) == 0xCDCDCDCD and int(status[0]) == 0xCD
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        t.unchanged("after the refused calls")
        for bad_lo, bad_hi in [(lo[:3], hi), (lo, hi + b"x"), (b"", b""), (bytes(K), hi), (lo, b"\xff" * K), (hi, lo), (bytes(33), bytes(33))]:
            for fn in (t.tree.count_range, t.tree.range_rows, t.tree.range_bits):
                with pytest.raises(mf.MfhError):
                    fn(t.view, bad_lo, bad_hi)
            with pytest.raises(mf.MfhError):
                t.tree.range_segments(t.view, bad_lo, bad_hi, [1])
        for bad in ([], [0], [3], [2, 2], [2, 1], [1, 3], None, 7):
            with pytest.raises(mf.MfhError):
                t.tree.range_segments(t.view, lo, hi, bad)
        for bad_table in (t.view[:4], t.view.cpu().numpy()):
            with pytest.raises(mf.MfhError):
                t.tree.range_rows(bad_table, lo, hi)
        with pytest.raises(mf.MfhError):
            t.tree.range_rows(t.view, lo, hi, max_links=(1 << 16) + 1)
        t.unchanged("after the refused Python calls")
    finally:
        ctx.set_timing(False)


# ---------------------------------------------------------------------------------------------------------------- 10. two streams
def _late_table(ctx):
    rng = np.random.default_rng(19600)
    K, length, depth, cuts = 4, 16, 9, [3, 7]
    table, members = R.make_table(rng, K, length, depth, 300, garbage=10)
    records = [r.tobytes() for r in table]
    model = _model(records)
    lo, hi = members[20], members[150]
    want = R.range_rows(records, K, lo, hi, model=model)  # (first: nothing of the host's stands between the late table and the calls)
    want_cut = R.range_segments(records, K, lo, hi, cuts, model=model)
    tree = ctx.merkle_tree(depth)
    try:
        placed = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, placed.view)  # no wait before it, nor before the next
        rows, index, keys, status = tree.range_rows(placed.view, lo, hi, max_links=200)
        assert status == 0 and np.array_equal(index, want[1]) and np.array_equal(keys, want[2]) and np.array_equal(rows, want[0]) and len(index) == 132
        rows, nodes, index, keys, status = tree.range_segments(placed.view, lo, hi, cuts)
        assert status == 0 and np.array_equal(index, want_cut[2]) and np.array_equal(nodes, want_cut[1])
        _same(rows, want_cut[0], "late table, cut")
        placed.holds(records, "late table")
        _assert_tree(tree, model.levels, "late table")
    finally:
        tree.close()


def test_ordering_null_stream(ctx):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_table(ctx)


def test_ordering_callers_stream(gpu_ctx_factory, mf):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_table(c)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 11. end to end
def test_end_to_end_range(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth, cuts, reveal = 4, 9, 2, [1], 1
    low, climb = W.MerkleLink(K, length, 1, reveal), W.MerkleClimb(1)
    cc_low, cc_climb = low.circuit.compile(p), climb.circuit.compile(p)
    assert (cc_low.lu, cc_climb.lu) == (256 + 72, 512) and (cc_low.nwires, cc_low.nrows) == W.MERKLE_LINK_SIZES[K, length, 1, reveal]
    rng = np.random.default_rng(19700)
    members = [int(x).to_bytes(K, "big") for x in (0x23456789, 0x6789ABCD)]
    edges = [bytes(K)] + members + [b"\xff" * K]
    live = [a + b + rng.bytes(1) for a, b in zip(edges, edges[1:])]
    records = [live[2], live[0], bytes(length), live[1]]  # key order is not table order; the links lie in both depth-1 subtrees
    lo, hi = (0x23456000).to_bytes(K, "big"), (0x70000000).to_bytes(K, "big")
    want_rows, want_nodes, want_i, want_k, want_s, model = R.range_segments(records, K, lo, hi, cuts)
    assert want_s == 0 and want_i.tolist() == [1, 3, 0]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=3)
        tree.set_records(0, table.view)
        bits, nodes, index, keys, status = tree.range_segment_bits(table.view, lo, hi, cuts)
        root = tree.root()
        table.holds(records, "end to end")
    finally:
        tree.close()
    assert status == 0 and np.array_equal(index, want_i) and np.array_equal(keys, want_k) and np.array_equal(nodes, want_nodes) and root == model.root()
    rows = [np.packbits(b, axis=1, bitorder="little") for b in bits]
    _same(rows, want_rows, "end to end")

    # the witnesses, and what the prover publishes next to the proofs: the nodes, the keys, the shown bytes
    w_low = _witnesses(ctx, cc_low, bits[0])
    shown = [low.shown_of(w_low[i])[2 * K:] for i in range(3)]
    assert shown == [records[int(s)][2 * K: 2 * K + reveal] for s in index]
    # the verifier's side: statements from the published nodes, the bounds, the returned keys and the shown bytes ALONE
    claim = [keys[0, 0].tobytes()] + [keys[i, 1].tobytes() for i in range(3)]
    assert claim == edges
    own_low = low.chain_cut(nodes[:, 0], lo, hi, claim, shown)
    own_climb = [W.MerkleClimb.chain(nodes[i])[0] for i in range(3)]
    assert all(nodes[i, 1].tobytes() == root for i in range(3))
    assert own_low == [w_low[i][: 32 + 2 * K + reveal].tobytes() for i in range(3)] == R.statements(nodes[:, 0], records, index, K, reveal)

    prove, verify = _prover(ctx, p, cc_low, rng, 3)
    proofs = prove(w_low)
    assert verify(proofs, own_low) == [True, True, True]
    assert verify(proofs, [own_low[1], own_low[2], own_low[0]]) == [False, False, False]                        # another order
    assert verify(proofs, low.chain_cut([_flip(nodes[i, 0].tobytes(), 77) for i in range(3)], lo, hi, claim, shown)) == [False, False, False]  # a flipped node
    assert verify(proofs, low.chain_cut(nodes[:, 0], lo, hi, claim, [_flip(v, 0) for v in shown])) == [False, False, False]                    # another balance
    # a claimed result that omits k_1: chain accepts the shorter list, which is consistent on its face, but no proof verifies its merged link (p, k_2)
    short = [claim[0], claim[2], claim[3]]
    for node in nodes[:, 0]:
        merged = low.chain_cut([node, nodes[2, 0]], lo, hi, short, [shown[0], shown[2]])
        assert len(merged) == 2 and merged[1] == own_low[2] and merged[0] not in own_low
        assert verify(proofs, [merged[0]] * 3) == [False, False, False]
        merged = low.chain_cut([node, nodes[2, 0]], lo, hi, short, [shown[1], shown[2]])
        assert verify(proofs, [merged[0]] * 3) == [False, False, False]

    # segment 1: every X_0 lies one level below the root
    w_climb = _witnesses(ctx, cc_climb, bits[1])
    assert [climb.top_of(w_climb[i]) for i in range(3)] == [root] * 3
    prove, verify = _prover(ctx, p, cc_climb, rng, 3)
    proofs = prove(w_climb)
    assert own_climb == [w_climb[i][:64].tobytes() for i in range(3)]
    assert verify(proofs, own_climb) == [True, True, True]
    assert own_climb[0] != own_climb[1] and own_climb[0] == own_climb[2]  # links 0 and 2 share a subtree
    assert verify(proofs, [own_climb[1], own_climb[0], own_climb[1]]) == [False, False, False]
    other_root = _flip(root, 77)
    assert verify(proofs, [W.MerkleClimb.chain([nodes[i, 0].tobytes(), other_root])[0] for i in range(3)]) == [False, False, False]
    print(f"test_end_to_end_range (MerkleLink(4, 9, 1, reveal=1) + MerkleClimb(1), d = 2^17): {time.time() - t0:.1f} s")
