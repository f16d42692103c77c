"""GPU: Merkle READS with the path cut into level ranges (mfh_merkle_paths_cut, mfh_merkle_absent_rows_cut, k_merkle_climb_rows; MerkleTree.path_segments /
record_segments / absent_segments) against tests/merkle_climb_model.py, a pure-Python model over tests/sha256_ref.py: rows and nodes byte for byte.

1. depth 3, cuts [1], [2], [1, 2], every leaf: rows and nodes are the model's, the *_bits forms pack to the rows, and the uncut path_rows row is the
   concatenation the segments imply (the leaf, every segment's siblings in order, the index bits split at the cuts).
2. depth 12, cuts [2] and [3, 11] (a 10-level and an 8-level segment: two index bytes and one; segments of 1, 2 and 3 levels), 300 indices repeated and
   unsorted, more than one workgroup a segment.
3. absent_segments at depth 3 and 9 with (4, 8) and (8, 55) records in a misaligned, strided table: index and status are locate_keys', statuses 0 and 1
   both occur, segment 0 is the model's depth-c_0 reading and agrees with absent_rows' row; a hand-made malformed table gives status 2 -- the key alone in
   segment 0 with the rest of the row untouched, zero upper rows, zero nodes below the root.
4. two chunks, by the existing recipe: depth 2, cut [1], length 65 521, 1 030 queries, both located records on both sides of the seam at 1 021.
5. record_segments against the model.
6. launch counts by timing kind: the cut calls launch "merkle_climb_rows" once a chunk and no "merkle_paths"; path_rows, absent_rows and update_segments
   launch exactly what they did; wider strides keep their tails; scrubbed staging gives the same rows.
7. every refusal leaves tree and table byte-identical and launches nothing.
8. a table produced late on the stream, on the null stream and on a caller's.
9. end to end at d = 2^17 on a depth-2 table of (4, 8) records with cut [1]: two absent keys proved as MerkleAbsent(4, 8, 1) plus MerkleClimb(1), one setup
   each; both verify against MerkleAbsent.statement(nodes[0], key) and MerkleClimb.chain(nodes); the climb proofs are rejected against a chain built with
   another root; a PRESENT key's segment-0 row is refused by ssp_rows_violations before it is paid for."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

import merkle_climb_model as M
from test_gpu_merkle import _assert_tree, _flip
from test_gpu_merkle_record_update import Placed
from test_gpu_merkle_segments import _prover, _witnesses

pytestmark = pytest.mark.gpu

SEED = bytes((53 * i + 11) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_climb_rows", "merkle_paths", "merkle_locate", "merkle_absent_rows", "merkle_segments", "merkle_updates", "merkle_level", "sha256_records")
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


def _keys(queries, K):
    return np.frombuffer(b"".join(queries), dtype=np.uint8).reshape(len(queries), K).copy()


def _table(W, members, K, depth, length, rng):
    pay = [rng.bytes(length - 2 * K) for _ in members]
    return [r.tobytes() for r in W.indexed_records(_keys(members, K), depth, length=length, payloads=pay)]


# ---------------------------------------------------------------------------------------------------------------- 1. depth 3, every leaf
@pytest.fixture(scope="module")
def tree3(ctx):
    rng = np.random.default_rng(17000)
    model = M.ClimbModel([rng.bytes(32) for _ in range(8)])
    tree = ctx.merkle_tree(3)
    tree.set_leaves(0, b"".join(model.levels[0]))
    yield tree, model
    tree.close()


@pytest.mark.parametrize("cuts", CUTS3)
def test_depth_3_every_leaf(tree3, cuts):
    tree, model = tree3
    indices = list(range(8))
    want_rows, want_nodes = M.path_segments(model, indices, cuts)
    rows, nodes = tree.path_segments(indices, cuts)
    _same(rows, want_rows, cuts)
    assert nodes.dtype == np.uint8 and nodes.shape == (8, len(cuts) + 1, 32) and np.array_equal(nodes, want_nodes)
    assert all(nodes[k, -1].tobytes() == tree.root() == model.root() for k in range(8))
    bits, nodes2 = tree.path_segment_bits(indices, cuts)
    segs = M.ranges(3, cuts)
    assert [b.shape for b in bits] == [(8, 512 + 257 * (hi - lo)) for lo, hi in segs] and np.array_equal(nodes2, nodes)
    _same([np.packbits(b, axis=1, bitorder="little") for b in bits], want_rows, (cuts, "bits"))
    # the uncut row is what the segments imply: the leaf, the siblings in order, the index bits split at the cuts
    uncut = tree.path_rows(indices)
    for k in indices:
        assert uncut[k, :64].tobytes() == rows[0][k, :64].tobytes()
        assert uncut[k, 64: 64 + 96].tobytes() == b"".join(r[k, 64: 64 + 32 * (hi - lo)].tobytes() for r, (lo, hi) in zip(rows, segs))
        assert int(uncut[k, 160]) == sum(int(r[k, 64 + 32 * (hi - lo)]) << lo for r, (lo, hi) in zip(rows, segs)) == k
    _assert_tree(tree, model.levels, cuts)
    # no statement at all
    rows0, nodes0 = tree.path_segments([], cuts)
    assert [r.shape for r in rows0] == [(0, r.shape[1]) for r in want_rows] and nodes0.shape == (0, len(cuts) + 1, 32)


# ---------------------------------------------------------------------------------------------------------------- 2. depth 12
@pytest.fixture(scope="module")
def tree12(ctx):
    rng = np.random.default_rng(17100)
    model = M.ClimbModel([rng.bytes(32) for _ in range(1 << 12)])
    tree = ctx.merkle_tree(12)
    tree.set_leaves(0, b"".join(model.levels[0]))
    yield tree, model
    tree.close()


@pytest.mark.parametrize("cuts", [[2], [3, 11], [1, 3, 6]])
def test_depth_12_repeated_unsorted(tree12, cuts):
    tree, model = tree12
    rng = np.random.default_rng(17200)
    pool = [0, 4095, 1024, 1023, 2048] + [int(x) for x in rng.integers(0, 1 << 12, size=60)]
    indices = [pool[int(i)] for i in rng.integers(0, len(pool), size=300)]
    assert len(set(indices)) < 70 and indices != sorted(indices)
    want_rows, want_nodes = M.path_segments(model, indices, cuts)
    assert [r.shape[1] for r in want_rows] == [64 + 32 * (hi - lo) + (hi - lo + 7) // 8 for lo, hi in M.ranges(12, cuts)]
    rows, nodes = tree.path_segments(np.array(indices, dtype=np.int64), cuts)
    _same(rows, want_rows, cuts)
    assert np.array_equal(nodes, want_nodes)
    if cuts == [2]:  # the 10-level segment's two index bytes hold index >> 2
        assert all(int.from_bytes(rows[1][k, -2:].tobytes(), "little") == i >> 2 for k, i in enumerate(indices)) and rows[1].shape[1] == 64 + 320 + 2
    _assert_tree(tree, model.levels, cuts)


# ---------------------------------------------------------------------------------------------------------------- 3. absent queries
def _check_absent(tree, table, records, K, queries, cuts, what):
    want_rows, want_nodes, want_i, want_s, model = M.absent_segments(records, K, queries, cuts)
    keys = _keys(queries, K)
    rows, nodes, index, status = tree.absent_segments(table.view, keys, cuts)
    assert index.dtype == np.uint32 and status.dtype == np.uint8
    index2, status2 = tree.locate_keys(table.view, keys)
    assert np.array_equal(index, index2) and np.array_equal(status, status2), what
    assert np.array_equal(index, want_i) and np.array_equal(status, want_s), (what, index, want_i, status, want_s)
    _same(rows, want_rows, what)
    assert np.array_equal(nodes, want_nodes), what
    # against the uncut call: the same head, the segments' siblings in order
    uncut, _, _ = tree.absent_rows(table.view, keys)
    head, segs = 32 + K + len(records[0]), M.ranges(model.depth, cuts)
    for k in np.flatnonzero(status != 2):
        assert uncut[k, :head].tobytes() == rows[0][k, :head].tobytes(), (what, k)
        tails = [rows[0][k, head: head + 32 * segs[0][1]].tobytes()] + [r[k, 64: 64 + 32 * (hi - lo)].tobytes() for r, (lo, hi) in zip(rows[1:], segs[1:])]
        assert uncut[k, head: head + 32 * model.depth].tobytes() == b"".join(tails), (what, k)
    table.holds(records, what)
    _assert_tree(tree, model.levels, what)
    return status, model


@pytest.mark.parametrize("K,length", [(4, 8), (8, 55)])
@pytest.mark.parametrize("depth,cutlists", [(3, CUTS3), (9, [[4], [1, 8]])])
def test_absent_segments(ctx, W, depth, cutlists, K, length):
    rng = np.random.default_rng(17300 + 100 * depth + K)
    members = sorted({rng.bytes(K) for _ in range((1 << depth) - 3)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    nq = 12 if depth == 3 else 70
    queries = [members[int(i)] for i in rng.integers(0, len(members), size=nq // 3)] + [rng.bytes(K) for _ in range(nq - nq // 3)]
    queries = [queries[int(i)] for i in rng.permutation(nq)] + queries[:2]  # (repeats)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 3, off=1)  # misaligned base, a stride that is no multiple of 4
        assert table.view.data_ptr() % 4 == 1
        tree.set_records(0, table.view)
        for cuts in cutlists:
            status, _ = _check_absent(tree, table, records, K, queries, cuts, (depth, K, cuts))
            assert set(status.tolist()) == {0, 1}
        bits, nodes, index, status = tree.absent_segment_bits(table.view, _keys(queries[:3], K), cutlists[0])
        lv = [hi - lo for lo, hi in M.ranges(depth, cutlists[0])]
        assert [b.shape for b in bits] == [(3, 256 + 8 * (K + length) + 257 * lv[0])] + [(3, 512 + 257 * x) for x in lv[1:]]
        want_rows = M.absent_segments(records, K, queries[:3], cutlists[0])[0]
        _same([np.packbits(b, axis=1, bitorder="little") for b in bits], want_rows, "bits")
    finally:
        tree.close()


def test_malformed_table_status_2(ctx):
    depth, K, length = 3, 2, 6
    rng = np.random.default_rng(17400)
    key = lambda x: int(x).to_bytes(K, "big")  # noqa: E731
    rec = lambda lo, hi: key(lo) + key(hi) + rng.bytes(length - 2 * K)  # noqa: E731
    # nothing covers [0x6000, 0x7000]; records 2 and 5 overlap in (0x3000, 0x4000)
    records = [bytes(length), rec(0x1000, 0x2000), rec(0x2000, 0x4000), rec(0x9000, 0x8000), rec(0, 0x1000), rec(0x3000, 0x6000), rec(0x7000, 0xFFFF), rec(0x1000, 0x1800)]
    queries = [key(x) for x in (0x3800, 0x3000, 0x6000, 0x6800, 0x7000, 0x1400, 0x1000, 0x8800)]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        for cuts in CUTS3:
            status, model = _check_absent(tree, table, records, K, queries, cuts, ("malformed", cuts))
            assert status.tolist() == [0, 1, 2, 2, 1, 0, 1, 0]
        # raw, into wider rows of 0xAB: a status 2 query writes the 32 zero bytes and its key in segment 0, all of its upper rows as zeros, nothing else
        cuts = [1, 2]
        want_rows, _, want_i, want_s, _ = M.absent_segments(records, K, queries, cuts)
        widths = [r.shape[1] for r in want_rows]
        bufs = [np.full((len(queries), w + e), 0xAB, dtype=np.uint8) for w, e in zip(widths, (5, 0, 9))]
        index, status = np.zeros(len(queries), dtype=np.uint32), np.zeros(len(queries), dtype=np.uint8)
        keys, cu = _keys(queries, K), np.array(cuts, dtype=np.uint32)
        vp = ctypes.c_void_p
        ptrs = (vp * 3)(*[b.ctypes.data for b in bufs])
        strides = (ctypes.c_size_t * 3)(*[b.shape[1] for b in bufs])
        rc = ctx.lib.mfh_merkle_absent_rows_cut(ctx._h, tree._h, vp(table.view.data_ptr()), table.stride, length, K, len(queries), vp(keys.ctypes.data), K, 2,
                                                vp(cu.ctypes.data), ptrs, strides, vp(index.ctypes.data), vp(status.ctypes.data))
        assert rc == 0, ctx.lib.mfh_last_error(ctx._h).decode()
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s)
        for k, s in enumerate(want_s):
            wrote = 32 + K if s == 2 else widths[0]
            assert np.array_equal(bufs[0][k, :wrote], want_rows[0][k, :wrote]) and (bufs[0][k, wrote:] == 0xAB).all(), k
            for g in (1, 2):
                assert np.array_equal(bufs[g][k, : widths[g]], want_rows[g][k]) and (bufs[g][k, widths[g]:] == 0xAB).all(), (k, g)
                assert bufs[g][k, : widths[g]].any() == (s != 2)
        table.holds(records, "malformed, raw")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. two chunks
def test_two_chunks(ctx, W):
    depth, K, length, nq, cuts = 2, 4, 65521, 1030, [1]
    per_chunk = (64 << 20) // (32 + K + length + 32 + 1 + 97)
    assert per_chunk == 1021
    rng = np.random.default_rng(17500)
    member = (0x80000000).to_bytes(K, "big")
    records = _table(W, [member], K, depth, length, rng)
    records = [records[i] for i in (2, 1, 3, 0)]  # the sentinel record at leaf 3 and the member's at leaf 1: one in each depth-1 subtree
    queries = [rng.bytes(K) for _ in range(nq)]
    queries[per_chunk - 2: per_chunk + 2] = [int(x).to_bytes(K, "big") for x in (0x10, 0x90000000, 0x20, 0xA0000000)]  # both records on both sides of the seam
    queries[-1] = member
    want_rows, want_nodes, want_i, want_s, model = M.absent_segments(records, K, queries, cuts)
    assert set(want_i[:per_chunk].tolist()) == set(want_i[per_chunk:].tolist()) == {1, 3} and want_s[-1] == 1
    assert want_i[per_chunk - 2: per_chunk + 2].tolist() == [3, 1, 3, 1]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        rows, nodes, index, status = tree.absent_segments(table.view, _keys(queries, K), cuts)
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s) and np.array_equal(nodes, want_nodes)
        _same(rows, want_rows, "two chunks")
        assert ctx.timing_drain("merkle_climb_rows")[::2] == (2, 2 * nq)
        assert ctx.timing_drain("merkle_absent_rows")[::2] == (2, nq)
        assert ctx.timing_drain("merkle_locate")[::2] == (1, 4)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        table.holds(records, "two chunks")
        _assert_tree(tree, model.levels, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. records
@pytest.mark.parametrize("length", [8, 55, 56])
def test_record_segments(ctx, mf, length):
    depth = 5
    rng = np.random.default_rng(17600 + length)
    records = [rng.bytes(length) for _ in range(1 << depth)]
    indices = [31, 0, 17, 17, 6, 30, 1]
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_records(0, np.frombuffer(b"".join(records), dtype=np.uint8).reshape(1 << depth, length))
        for cuts in ([2], [1, 4]):
            want_rows, want_nodes, model = M.record_segments(records, indices, cuts)
            given = np.frombuffer(b"".join(records[i] for i in indices), dtype=np.uint8).reshape(len(indices), length)
            for recs in (given, [records[i] for i in indices]):
                rows, nodes = tree.record_segments(recs, indices, cuts)
                _same(rows, want_rows, (length, cuts))
                assert np.array_equal(nodes, want_nodes)
            bits, _ = tree.record_segment_bits(given, indices, cuts)
            lv = [hi - lo for lo, hi in M.ranges(depth, cuts)]
            assert [b.shape for b in bits] == [(7, 256 + 8 * length + 257 * lv[0])] + [(7, 512 + 257 * x) for x in lv[1:]]
            _same([np.packbits(b, axis=1, bitorder="little") for b in bits], want_rows, "bits")
            # segment 0 is record_rows' head over the first c_0 siblings
            uncut = tree.record_rows(given, indices)
            assert np.array_equal(uncut[:, : 32 + length + 32 * cuts[0]], rows[0][:, : 32 + length + 32 * cuts[0]])
        _assert_tree(tree, model.levels, length)
        for bad in (given[:3], given.astype(np.int8), [b"ab", b"abc"] + [b"ab"] * 5):
            with pytest.raises(mf.MfhError):
                tree.record_segments(bad, indices, [2])
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. launches and strides
def test_launch_counts_and_wider_strides(ctx, W, tree12):
    tree, model = tree12
    depth, cuts, n = 12, [3, 11], 300
    rng = np.random.default_rng(17700)
    indices = [int(x) for x in rng.integers(0, 1 << depth, size=n)]
    want_rows, want_nodes = M.path_segments(model, indices, cuts)
    widths = [r.shape[1] for r in want_rows]
    assert widths == [64 + 96 + 1, 64 + 256 + 1, 64 + 32 + 1]
    bufs = [np.full((n, w + e), 0xAB, dtype=np.uint8) for w, e in zip(widths, (13, 0, 5))]
    iu, cu = np.array(indices, dtype=np.uint32), np.array(cuts, dtype=np.uint32)
    vp = ctypes.c_void_p
    ptrs = (vp * 3)(*[b.ctypes.data for b in bufs])
    strides = (ctypes.c_size_t * 3)(*[b.shape[1] for b in bufs])
    try:
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        rc = ctx.lib.mfh_merkle_paths_cut(ctx._h, tree._h, n, vp(iu.ctypes.data), 2, vp(cu.ctypes.data), ptrs, strides)
        assert rc == 0, ctx.lib.mfh_last_error(ctx._h).decode()
        launches, ms, total = ctx.timing_drain("merkle_climb_rows")
        print(f"depth {depth}, cuts {cuts}: k_merkle_climb_rows for {n} statements: {ms:.3f} ms")
        assert (launches, total) == (1, 3 * n)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)  # no k_merkle_paths, nothing else
        for g in range(3):
            assert np.array_equal(bufs[g][:, : widths[g]], want_rows[g]) and (bufs[g][:, widths[g]:] == 0xAB).all(), g
        # the pinned staging zeroed in between: the same rows
        assert ctx.scrub_staging() == 0
        rows, nodes = tree.path_segments(indices, cuts)
        _same(rows, want_rows, "after the scrub")
        assert np.array_equal(nodes, want_nodes)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_climb_rows": 1}
        # the uncut calls launch exactly what they did
        tree.path_rows(indices)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_paths": 1}
        K, length, d9 = 8, 55, 9
        members = sorted({rng.bytes(K) for _ in range(300)})
        records = _table(W, members, K, d9, length, rng)
        small = ctx.merkle_tree(d9)
        try:
            table = Placed(ctx, records, stride=length + 1)
            small.set_records(0, table.view)
            ctx.sync()
            _counts(ctx)
            keys = _keys([rng.bytes(K) for _ in range(40)], K)
            small.absent_rows(table.view, keys)
            assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_absent_rows": 1, "merkle_paths": 1}
            small.absent_segments(table.view, keys, [4])
            assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_absent_rows": 1, "merkle_climb_rows": 1}
            small.update_segments([5, 6, 5], rng.bytes(96), [2, 5])
            assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_updates": d9 + 1, "merkle_segments": 1}
        finally:
            small.close()
        ctx.set_timing(False)
        _assert_tree(tree, model.levels, "launch counts")
    finally:
        ctx.set_timing(False)


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_einval(ctx, mf, W):
    lib, h = ctx.lib, ctx._h
    depth, K, length, cuts = 3, 4, 17, [1, 2]
    rng = np.random.default_rng(17800)
    members = sorted({rng.bytes(K) for _ in range(5)})
    records = _table(W, members, K, depth, length, rng)
    model = M.ClimbModel([hashlib.sha256(r).digest() for r in records])
    tree = ctx.merkle_tree(depth)
    texts = []

    def refused(rc, who):
        assert rc == EINVAL
        text = lib.mfh_last_error(h).decode()
        assert text.startswith(who + ": "), text
        texts.append(text)

    try:
        table = Placed(ctx, records, stride=length + 3, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        vp = ctypes.c_void_p
        keys = _keys([rng.bytes(K) for _ in range(3)], K)
        zero = keys.copy()
        zero[1] = 0
        widths_p = [64 + 32 + 1] * 3
        widths_a = [32 + K + length + 32 + 1, 97, 97]
        index, status = np.full(3, 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        iu, bad_iu = np.array([1, 7, 1], dtype=np.uint32), np.array([1, 8, 1], dtype=np.uint32)
        cu = np.array(cuts, dtype=np.uint32)
        kp, zp, ip, sp, up, bup, cp = (vp(a.ctypes.data) for a in (keys, zero, index, status, iu, bad_iu, cu))
        tp, ts = vp(table.view.data_ptr()), table.stride

        def outs(widths, short=None, null=None):
            bufs = [np.full((3, w + 4), 0xAB, dtype=np.uint8) for w in widths]
            ptrs = (vp * 3)(*[None if g == null else b.ctypes.data for g, b in enumerate(bufs)])
            strides = (ctypes.c_size_t * 3)(*[w - 1 if g == short else w + 4 for g, w in enumerate(widths)])
            return bufs, ptrs, strides

        kept = []
        fp, who = lib.mfh_merkle_paths_cut, "mfh_merkle_paths_cut"
        bufs, ptrs, strides = outs(widths_p)
        kept.append(bufs)
        refused(fp(h, None, 3, up, 2, cp, ptrs, strides), who)
        refused(fp(h, tree._h, 3, up, 0, cp, ptrs, strides), who)
        refused(fp(h, tree._h, 3, up, 2, None, ptrs, strides), who)
        texts.pop()  # (ncuts = 0 and h_cuts null: one text)
        for bad in ([0, 2], [1, 3], [2, 2], [2, 1]):
            b = np.array(bad, dtype=np.uint32)
            refused(fp(h, tree._h, 3, up, 2, vp(b.ctypes.data), ptrs, strides), who)
            if bad != [0, 2]:
                texts.pop()  # (one text for every bad cut list)
        refused(fp(h, tree._h, 3, up, 2, cp, None, strides), who)
        refused(fp(h, tree._h, 3, up, 2, cp, ptrs, None), who)
        texts.pop()
        for g in range(3):
            _, p2, s2 = outs(widths_p, null=g)
            refused(fp(h, tree._h, 3, up, 2, cp, p2, s2), who)
            _, p3, s3 = outs(widths_p, short=g)
            refused(fp(h, tree._h, 3, up, 2, cp, p3, s3), who)
            if g:
                texts.pop()
                texts.pop()
        refused(fp(h, tree._h, 3, None, 2, cp, ptrs, strides), who)
        refused(fp(h, tree._h, 3, bup, 2, cp, ptrs, strides), who)
        assert fp(None, tree._h, 3, up, 2, cp, ptrs, strides) == EINVAL
        assert fp(h, tree._h, 0, None, 2, cp, ptrs, strides) == 0  # no statement: nothing to do
        assert len(set(texts)) == len(texts) == 8, sorted(texts)

        texts.clear()
        fa, who = lib.mfh_merkle_absent_rows_cut, "mfh_merkle_absent_rows_cut"
        bufs, ptrs, strides = outs(widths_a)
        kept.append(bufs)
        refused(fa(h, None, tp, ts, length, K, 3, kp, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, length, 0, 3, kp, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, 2 * K - 1, K, 3, kp, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, (1 << 20) + 1, (1 << 20) + 1, K, 3, kp, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, length - 1, length, K, 3, kp, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K - 1, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 0, cp, ptrs, strides, ip, sp), who)
        b = np.array([1, 3], dtype=np.uint32)
        refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 2, vp(b.ctypes.data), ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 2, cp, None, strides, ip, sp), who)
        for g in range(3):
            _, p2, s2 = outs(widths_a, null=g)
            refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 2, cp, p2, s2, ip, sp), who)
            _, p3, s3 = outs(widths_a, short=g)
            refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 2, cp, p3, s3, ip, sp), who)
            if g:
                texts.pop()
                texts.pop()
        refused(fa(h, tree._h, None, ts, length, K, 3, kp, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, None, K, 2, cp, ptrs, strides, ip, sp), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 2, cp, ptrs, strides, None, sp), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, kp, K, 2, cp, ptrs, strides, ip, None), who)
        refused(fa(h, tree._h, tp, ts, length, K, 3, zp, K, 2, cp, ptrs, strides, ip, sp), who)
        assert fa(None, tree._h, tp, ts, length, K, 3, kp, K, 2, cp, ptrs, strides, ip, sp) == EINVAL
        assert fa(h, tree._h, None, ts, length, K, 0, None, K, 2, cp, ptrs, strides, None, None) == 0
        assert len(set(texts)) == len(texts) == 16, sorted(texts)

        # nothing was written, launched or changed
        assert all((b == 0xAB).all() for bufs in kept for b in bufs) and (index == 0xCDCDCDCD).all() and (status == 0xCD).all()
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
        for bad in ([], [0], [3], [2, 2], [2, 1], [1, 3], None, 7):
            with pytest.raises(mf.MfhError):
                tree.path_segments([1, 2], bad)
            with pytest.raises(mf.MfhError):
                tree.absent_segments(table.view, keys, bad)
            with pytest.raises(mf.MfhError):
                tree.record_segments([records[1], records[2]], [1, 2], bad)
        for call in (tree.path_segments, tree.path_segment_bits):
            with pytest.raises(mf.MfhError):
                call([1, 8], [1])
            with pytest.raises(mf.MfhError):
                call([-1], [1])
        for bad_table, bad_keys in [(table.view, keys[0]), (table.view, zero), (table.view[:4], keys), (table.view.cpu().numpy(), keys)]:
            for call in (tree.absent_segments, tree.absent_segment_bits):
                with pytest.raises(mf.MfhError):
                    call(bad_table, bad_keys, [1])
        _assert_tree(tree, model.levels, "after the refused Python calls")
        table.holds(records, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. two streams
def _late_table(ctx, W):
    depth, K, length, cuts = 9, 4, 16, [3, 7]
    rng = np.random.default_rng(17900)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = _table(W, members, K, depth, length, rng)
    queries = [members[int(i)] for i in rng.integers(0, 300, size=10)] + [rng.bytes(K) for _ in range(54)]
    want = M.absent_segments(records, K, queries, cuts)  # (first: nothing of the host's stands between the late table and the calls)
    indices = [int(x) for x in rng.integers(0, 1 << depth, size=40)]
    want_paths = M.path_segments(want[4], indices, cuts)
    keys = _keys(queries, K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        rows, nodes, index, status = tree.absent_segments(table.view, keys, cuts)
        assert np.array_equal(index, want[2]) and np.array_equal(status, want[3]) and np.array_equal(nodes, want[1])
        _same(rows, want[0], "late table")
        rows, nodes = tree.path_segments(indices, cuts)
        _same(rows, want_paths[0], "late table, paths")
        assert np.array_equal(nodes, want_paths[1])
        table.holds(records, "late table")
        _assert_tree(tree, want[4].levels, "late table")
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


# ---------------------------------------------------------------------------------------------------------------- 9. end to end
def test_end_to_end_absent_key(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth, cuts = 4, 8, 2, [1]
    low, climb = W.MerkleAbsent(K, length, 1), W.MerkleClimb(1)
    cc_low, cc_climb = low.circuit.compile(p), climb.circuit.compile(p)
    assert (cc_low.lu, cc_climb.lu) == (288, 512) and (cc_climb.nwires, cc_climb.nrows) == W.MERKLE_CLIMB_SIZES[1]
    rng = np.random.default_rng(18000)
    members = [int(x).to_bytes(K, "big") for x in (0x23456789, 0x6789ABCD)]
    records = _table(W, members, K, depth, length, rng)
    records = [records[i] for i in (3, 0, 2, 1)]
    absent = [int(x).to_bytes(K, "big") for x in (0x6789ABCC, 0x12345678)]
    queries = absent + [members[1]]
    want_rows, want_nodes, want_i, want_s, model = M.absent_segments(records, K, queries, cuts)
    assert want_s.tolist() == [0, 0, 1] and want_i[0] >> 1 != want_i[1] >> 1  # the two absent keys' records lie in different depth-1 subtrees
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        bits, nodes, index, status = tree.absent_segment_bits(table.view, _keys(queries, K), cuts)
        root = tree.root()
        table.holds(records, "end to end")
    finally:
        tree.close()
    assert np.array_equal(index, want_i) and np.array_equal(status, want_s) and np.array_equal(nodes, want_nodes) and root == model.root()
    _same([np.packbits(b, axis=1, bitorder="little") for b in bits], want_rows, "end to end")
    # the verifier's side: statements from the published nodes and the keys alone
    pub = [[nodes[k, g].tobytes() for g in range(2)] for k in range(3)]
    assert all(x[1] == root for x in pub) and pub[0][0] != pub[1][0]
    own_low = [low.statement(pub[k][0], queries[k]) for k in range(2)]
    own_climb = [W.MerkleClimb.chain(pub[k])[0] for k in range(2)]

    # segment 0.  The present key's row is refused before it is paid for: its witness violates a row
    prog = ctx.circuit_load(cc_low, state="auto")
    try:
        witness, holds = ctx.circuit_assign(prog, bits[0])
    finally:
        prog.close()
    assert holds.tolist() == [True, True, False]
    assert [low.root_of(witness[k]) for k in range(3)] == [pub[k][0] for k in range(3)]
    ctx.ssp_set_rows(cc_low.rows, lu_max=cc_low.lu)
    count, first = ctx.ssp_rows_violations(witness)
    assert not count[:2].any() and (first[:2] == NONE).all() and count[2] > 0 and first[2] != NONE
    prove, verify = _prover(ctx, p, cc_low, rng, 2)
    proofs = prove(witness[:2])
    assert own_low == [witness[k][:36].tobytes() for k in range(2)]
    assert verify(proofs, own_low) == [True, True]
    assert verify(proofs, own_low[::-1]) == [False, False]
    assert verify(proofs, [low.statement(root, q) for q in absent]) == [False, False]  # X_0 is not the root

    # segment 1: X_0 lies one level below the root
    w_climb = _witnesses(ctx, cc_climb, bits[1][:2])
    assert [climb.top_of(w_climb[k]) for k in range(2)] == [root, root]
    prove, verify = _prover(ctx, p, cc_climb, rng, 2)
    proofs = prove(w_climb)
    assert own_climb == [w_climb[k][:64].tobytes() for k in range(2)]
    assert verify(proofs, own_climb) == [True, True]
    assert verify(proofs, own_climb[::-1]) == [False, False]
    other_root = _flip(root, 77)
    assert verify(proofs, [W.MerkleClimb.chain([pub[k][0], other_root])[0] for k in range(2)]) == [False, False]
    print(f"test_end_to_end_absent_key (MerkleAbsent(4, 8, 1) + MerkleClimb(1), d = 2^17): {time.time() - t0:.1f} s")
