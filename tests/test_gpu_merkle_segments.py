"""GPU: the update calls with the path cut into level ranges (mfh_merkle_update_rows_cut / _update_records_cut / _insert_keys_cut, MerkleTree.update_segments /
update_record_segments / insert_key_segments) against the sequential host model of tests/merkle_segments_model.py, and against the existing uncut calls on a
second tree.

1. leaf updates: every segment's rows byte for byte (segment 0 = MerkleUpdate(c_0).bits, segment g = MerkleSegment(c_g - c_g-1).bits), the published nodes,
   all roots and every node of the tree; and, from update_rows on a second tree, the uncut rows' leaves, siblings and indices, sliced.  Depth 3 with
   hand-made batches under cuts [1], [2], [1, 2] (a cut node touched earlier in the batch and one not, a sibling touched earlier, the same leaf twice) and
   with 257 random updates; depth 9 with 300 under [4]; depth 12 with 64 under [3, 7, 10] and under [2] (ten levels: two index bytes).
2. two chunks at depth 2 under [1]: both leaves under one level-1 node change on both sides of the seam, so the old node behind the seam is the stored
   one; segment 0 by leaf tracking in numpy, segment 1 by its chain (old node k = new node k - 1), zeros, sibling and index everywhere, and 64 sampled
   nodes and roots by merkle_parent.
3. launch counts ("merkle_segments" 1 a chunk with rows = k G, "merkle_updates" still depth + 1, the uncut calls none) and wider strides whose tails stay.
4. records of 8, 55 and 56 bytes at a misaligned offset and stride; inserts at depth 3 under [1] and [1, 2] (p and s in one subtree and in two, a key that
   falls into a range split earlier in the batch) against the model and against the per-key route through update_record_segments on a second tree.
5. every new MFH_EINVAL leaves buffers, tree and launch counts as they were; a late table on a caller's stream.
6. end to end: five leaf updates of a depth-2 tree under [1] -- MerkleUpdate(1) and MerkleSegment(1) each set up at d = 2^17, all ten proofs verify against
   statements built from `nodes` alone, none under its neighbour's statement, no segment proof with one published node swapped for another update's; and
   one insert at depth 2 -- MerkleInsert(4, 8, 1, joined=False) at d = 2^19 and its two MerkleSegment(1) proofs, the root between the two updates shared."""
import ctypes
import time

import numpy as np
import pytest

from merkle_segments_model import insert_batch, insert_row_bytes, leaf_batch, record_batch, segment_row_bytes
from test_gpu_merkle import _assert_tree, _leaves, _parent, ref_tree
from test_gpu_merkle_absent import _key, _keys, _table
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

SEED = bytes((47 * i + 9) & 0xFF for i in range(40))
EINVAL = -1
KINDS = ("merkle_segments", "merkle_updates", "merkle_level", "merkle_record_rows", "sha256_records")


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


def _edges(depth, cuts):
    e = [0] + list(cuts) + [depth]
    return list(zip(e, e[1:]))


def _index_bytes(values, nbits):
    v = np.asarray(values, dtype=np.uint64)
    return np.stack([(v >> (8 * b)).astype(np.uint8) for b in range((nbits + 7) // 8)], axis=1)


def _assert_slices_of_uncut(rows, uncut, indices, depth, cuts, head):
    """the cut rows against the uncut call's rows of `head` bytes before the siblings: segment 0 is the head, the first c_0 siblings and the index mod 2^c_0;
    segment g >= 1 has the siblings of its levels and (index >> c_g-1) mod 2^levels"""
    idx = np.asarray(indices, dtype=np.uint64)
    for g, (lo, hi) in enumerate(_edges(depth, cuts)):
        at = 128 if g else head
        assert np.array_equal(rows[g][:, at: at + 32 * (hi - lo)], uncut[:, head + 32 * lo: head + 32 * hi]), g
        assert np.array_equal(rows[g][:, at + 32 * (hi - lo):], _index_bytes((idx >> lo) & ((1 << (hi - lo)) - 1), hi - lo)), g
        if g:
            assert not rows[g][:, 64:128].any()
    assert np.array_equal(rows[0][:, :head], uncut[:, :head])


def _check_leaves(ctx, leaves, indices, new, cuts, what):
    depth = len(leaves).bit_length() - 1
    want_rows, want_nodes, want_roots, model = leaf_batch(leaves, indices, new, cuts)
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        a.set_leaves(0, b"".join(leaves))
        b.set_leaves(0, b"".join(leaves))
        rows, nodes, roots = a.update_segments(indices, b"".join(new), cuts, roots=True)
        assert len(rows) == len(cuts) + 1 and [r.shape for r in rows] == [r.shape for r in want_rows], what
        for g, (got, want) in enumerate(zip(rows, want_rows)):
            assert np.array_equal(got, want), (what, g)
        assert np.array_equal(nodes, want_nodes) and np.array_equal(roots, want_roots), what
        _assert_tree(a, model.levels, what)
        uncut, uroots = b.update_rows(indices, b"".join(new), roots=True)
        assert np.array_equal(uroots, roots), what
        _assert_slices_of_uncut(rows, uncut, indices, depth, cuts, 128)
        _assert_tree(b, model.levels, what)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 1. leaf updates
HAND_MADE = [("a cut node touched earlier, then one not", [0, 1, 6]), ("a sibling touched earlier", [2, 3, 2, 0]), ("the same leaf twice", [5, 5]),
             ("cousins and back", [0, 2, 4, 1, 7, 0, 3])]


@pytest.mark.parametrize("cuts", [[1], [2], [1, 2]])
def test_hand_made_batches(ctx, cuts):
    rng = np.random.default_rng(16000 + 10 * len(cuts) + cuts[0])
    leaves = _leaves(rng, 8)
    for what, indices in HAND_MADE:
        _check_leaves(ctx, leaves, indices, _leaves(rng, len(indices)), cuts, (cuts, what))


@pytest.mark.parametrize("depth,nupd,cuts", [(3, 257, [1, 2]), (3, 257, [2]), (9, 300, [4]), (12, 64, [3, 7, 10]), (12, 64, [2])])
def test_random_batches(ctx, depth, nupd, cuts):
    rng = np.random.default_rng(16100 + depth + len(cuts))
    leaves = _leaves(np.random.default_rng(1200), 1 << 12) if depth == 12 else _leaves(rng, 1 << depth)  # (depth 12: test_gpu_merkle.py's leaves, cached parents)
    hot = [0, 1, 6, 7] + [int(x) for x in rng.integers(0, 1 << depth, size=4)]
    indices = [hot[int(rng.integers(0, 8))] if rng.integers(0, 2) else int(rng.integers(0, 1 << depth)) for _ in range(nupd)]
    assert len(set(indices)) < nupd
    if cuts == [2]:
        assert segment_row_bytes(depth - 2) == 128 + 32 * (depth - 2) + (2 if depth == 12 else 1)
    _check_leaves(ctx, leaves, indices, _leaves(rng, nupd), cuts, (depth, nupd, cuts))


# ---------------------------------------------------------------------------------------------------------------- 2. two chunks
def _swap_words(a):
    return a.reshape(len(a), 8, 4)[:, :, ::-1].reshape(len(a), 32)


def test_two_chunks(ctx):
    depth, cuts = 2, [1]
    rowb = segment_row_bytes(1)
    assert rowb == 161
    per_chunk = (64 << 20) // (2 * rowb)  # both segments' rows together
    nupd = per_chunk + 3
    assert per_chunk == 208412
    rng = np.random.default_rng(16200)
    start = rng.integers(0, 256, size=(4, 32), dtype=np.uint8)
    new = rng.integers(0, 256, size=(nupd, 32), dtype=np.uint8)
    idx = rng.integers(0, 2, size=nupd).astype(np.uint32)  # leaves 0 and 1: level-1 node 0 in every update, node 1 never
    idx[per_chunk - 2: per_chunk + 2] = [0, 1, 1, 0]  # both leaves change on both sides of the seam
    k = np.arange(nupd)
    before = []
    for s in (0, 1):
        last = np.maximum.accumulate(np.where(idx == s, k, -1))
        prev = np.concatenate([[-1], last[:-1]])
        before.append(np.where(prev[:, None] >= 0, new[np.maximum(prev, 0)], start[s]))
    mine = (idx == 1)[:, None]
    old, sib = np.where(mine, before[1], before[0]), np.where(mine, before[0], before[1])
    want0 = np.concatenate([np.zeros((nupd, 64), dtype=np.uint8), _swap_words(old), _swap_words(new), _swap_words(sib), idx[:, None].astype(np.uint8)], axis=1)
    other = _parent(start[2].tobytes(), start[3].tobytes())  # level-1 node 1, the sibling of every upper row
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, start)
        ctx.sync()
        ctx.set_timing(True)
        for kind in KINDS:
            ctx.timing_drain(kind)
        t0 = time.time()
        rows, nodes, roots = tree.update_segments(idx, new, cuts, roots=True)
        print(f"depth 2, cuts [1]: {nupd} updates in two chunks: {time.time() - t0:.2f} s")
        launches, _, total = ctx.timing_drain("merkle_segments")
        assert (launches, total) == (2, nupd)
        launches, _, total = ctx.timing_drain("merkle_updates")
        assert (launches, total) == (2 * (depth + 1), nupd * depth)
        ctx.set_timing(False)
        assert rows[0].shape == want0.shape == (nupd, rowb) and np.array_equal(rows[0], want0)
        up = rows[1]
        assert up.shape == (nupd, rowb) and not up[:, 64:128].any() and not up[:, 160].any()
        assert (up[:, 128:160] == _swap_words(np.frombuffer(other, dtype=np.uint8)[None, :])).all()
        # one node carries every update: the old node of update k is the new node of update k - 1, across the seam too, where it is the STORED node
        assert np.array_equal(up[1:, :32], up[:-1, 32:64])
        assert np.array_equal(nodes[:, 0].reshape(nupd, 64), _swap_words(up[:, :64].reshape(2 * nupd, 32)).reshape(nupd, 64))
        assert np.array_equal(nodes[:, 1, 0], roots[:-1]) and np.array_equal(nodes[:, 1, 1], roots[1:])
        after = [np.concatenate([before[s][1:], before[s][-1:]]) for s in (0, 1)]
        after[int(idx[-1])][-1] = new[-1]
        assert nodes[0, 0, 0].tobytes() == _parent(start[0].tobytes(), start[1].tobytes())
        picks = [0, per_chunk - 2, per_chunk - 1, per_chunk, per_chunk + 1, nupd - 1] + [int(x) for x in rng.integers(0, nupd, size=58)]
        for t in picks:
            node = _parent(after[0][t].tobytes(), after[1][t].tobytes())
            assert nodes[t, 0, 1].tobytes() == node and roots[t + 1].tobytes() == _parent(node, other), t
        final = [after[0][-1].tobytes(), after[1][-1].tobytes(), start[2].tobytes(), start[3].tobytes()]
        _assert_tree(tree, ref_tree(final), "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. launches and strides
def _counts(ctx):
    return {kind: ctx.timing_drain(kind)[0] for kind in KINDS}


def test_launch_counts_and_wider_strides(ctx):
    depth, nupd, cuts = 9, 300, [2, 5]
    rng = np.random.default_rng(16300)
    leaves = _leaves(rng, 1 << depth)
    indices = [int(x) for x in rng.integers(0, 24, size=nupd)]
    new = _leaves(rng, nupd)
    want_rows, want_nodes, want_roots, model = leaf_batch(leaves, indices, new, cuts)
    widths = [r.shape[1] for r in want_rows]
    assert widths == [128 + 64 + 1, 128 + 96 + 1, 128 + 128 + 1]
    extra = [13, 0, 5]
    bufs = [np.full((nupd, w + e), 0xAB, dtype=np.uint8) for w, e in zip(widths, extra)]
    roots = np.full((nupd + 1, 32), 0xCD, dtype=np.uint8)
    iu, cu = np.array(indices, dtype=np.uint32), np.array(cuts, dtype=np.uint32)
    ptrs = (ctypes.c_void_p * 3)(*[b.ctypes.data for b in bufs])
    strides = (ctypes.c_size_t * 3)(*[b.shape[1] for b in bufs])
    d_new = ctx.to_device(np.frombuffer(b"".join(new), dtype=np.uint8))
    vp = ctypes.c_void_p
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, b"".join(leaves))
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        rc = ctx.lib.mfh_merkle_update_rows_cut(ctx._h, tree._h, nupd, vp(iu.ctypes.data), vp(d_new.data_ptr()), 2, vp(cu.ctypes.data), ptrs, strides, vp(roots.ctypes.data))
        assert rc == 0, ctx.lib.mfh_last_error(ctx._h).decode()
        launches, ms, total = ctx.timing_drain("merkle_segments")
        print(f"depth {depth}, cuts {cuts}: k_merkle_cut_rows for {nupd} updates: {ms:.3f} ms")
        assert (launches, total) == (1, nupd * 2)
        launches, _, total = ctx.timing_drain("merkle_updates")
        assert (launches, total) == (depth + 1, nupd * depth)
        assert _counts(ctx) == dict.fromkeys(KINDS, 0)
        for g in range(3):
            assert np.array_equal(bufs[g][:, : widths[g]], want_rows[g]), g
            assert (bufs[g][:, widths[g]:] == 0xAB).all(), g
        assert np.array_equal(roots, want_roots)
        _assert_tree(tree, model.levels, "wider strides")
        # h_roots = NULL, the pinned staging zeroed in between: the same rows from the same starting tree
        tree.set_leaves(0, b"".join(leaves))
        assert ctx.scrub_staging() == 0
        for b in bufs:
            b[:] = 0
        assert ctx.lib.mfh_merkle_update_rows_cut(ctx._h, tree._h, nupd, vp(iu.ctypes.data), vp(d_new.data_ptr()), 2, vp(cu.ctypes.data), ptrs, strides, None) == 0
        for g in range(3):
            assert np.array_equal(bufs[g][:, : widths[g]], want_rows[g]), g
        _counts(ctx)
        # the uncut calls launch no cut kernel, and their counts are what they were
        tree.set_leaves(0, b"".join(leaves))
        ctx.sync()
        _counts(ctx)
        tree.update_rows(indices, b"".join(new))
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_updates": depth + 1}
        table = Placed(ctx, [rng.bytes(8) for _ in range(1 << depth)])
        tree.set_records(0, table.view)
        ctx.sync()
        _counts(ctx)
        tree.update_records(table.view, indices[:7], np.frombuffer(rng.bytes(56), dtype=np.uint8).reshape(7, 8))
        assert _counts(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_updates": depth + 1, "merkle_record_rows": 2, "sha256_records": 1}
        ctx.set_timing(False)
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. records and inserts
@pytest.mark.parametrize("length", [8, 55, 56])
def test_record_updates(ctx, length):
    depth, cuts = 3, [1, 2]
    rng = np.random.default_rng(16400 + length)
    records = [rng.bytes(length) for _ in range(8)]
    indices = [5, 4, 5, 1, 6, 5]
    new = [rng.bytes(length) for _ in indices]
    want_rows, want_nodes, want_roots, model, final = record_batch(records, indices, new, cuts)
    new_arr = np.stack([np.frombuffer(r, dtype=np.uint8) for r in new])
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        ta, tb = Placed(ctx, records, stride=length + 3, off=1), Placed(ctx, records, stride=length + 3, off=1)
        a.set_records(0, ta.view)
        b.set_records(0, tb.view)
        rows, nodes, roots = a.update_record_segments(ta.view, indices, new_arr, cuts, roots=True)
        for g, (got, want) in enumerate(zip(rows, want_rows)):
            assert got.shape == want.shape and np.array_equal(got, want), (length, g)
        assert np.array_equal(nodes, want_nodes) and np.array_equal(roots, want_roots)
        ta.holds(final, "cut")
        _assert_tree(a, model.levels, "cut")
        uncut, uroots = b.update_records(tb.view, indices, new_arr, roots=True)
        assert np.array_equal(uroots, roots)
        _assert_slices_of_uncut(rows, uncut, indices, depth, cuts, 64 + 2 * length)
        tb.holds(final, "uncut")
        bits = a.update_record_segment_bits(ta.view, indices[:1], new_arr[:1], cuts)[0]
        assert [x.shape for x in bits] == [(1, 512 + 16 * length + 257), (1, 1024 + 257), (1, 1024 + 257)]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("cuts", [[1], [1, 2]])
def test_inserts(ctx, W, cuts):
    depth, K, length = 3, 4, 11
    rng = np.random.default_rng(16500 + len(cuts))
    top = 0x10 << 24
    records = _table(W, [_key(x, K) for x in (top, top + 1, 3 * top)], K, depth, length, rng)  # slots 0 .. 3 live, 4 .. 7 inert
    # 4 top + 2 goes into record 3 and slot 4: two depth-1 subtrees; 4 top + 3 falls into the range that insert made, slot 4's, with slot 5: ONE subtree;
    # 4 top + 1 falls into what is left of record 3's range, with slot 6 (slot 7 stays inert for the last call below)
    keys = [_key(4 * top + 2, K), _key(4 * top + 3, K), _key(4 * top + 1, K)]
    payloads = [rng.bytes(length - 2 * K) for _ in keys]
    want_rows, want_p, want_s, want_index, want_roots, model = insert_batch(records, K, keys, payloads, cuts)
    assert want_index.tolist() == [[3, 4], [4, 5], [3, 6]]
    pay = np.frombuffer(b"".join(payloads), dtype=np.uint8).reshape(len(keys), length - 2 * K).copy()
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        ta, tb = Placed(ctx, records, stride=length + 2, off=3), Placed(ctx, records, stride=length + 2, off=3)
        a.set_records(0, ta.view)
        b.set_records(0, tb.view)
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        rows, nodes_p, nodes_s, index = a.insert_key_segments(ta.view, _keys(keys, K), cuts, pay)
        counts = _counts(ctx)
        ctx.set_timing(False)
        assert counts == {"merkle_segments": 1, "merkle_updates": depth + 1, "merkle_level": 0, "merkle_record_rows": 2, "sha256_records": 1}
        assert rows[0].shape == (len(keys), insert_row_bytes(K, length, cuts[0])) and all(r.shape[0] == 2 * len(keys) for r in rows[1:])
        for g, (got, want) in enumerate(zip(rows, want_rows)):
            assert got.shape == want.shape and np.array_equal(got, want), (cuts, g)
        assert np.array_equal(index, want_index) and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s)
        assert np.array_equal(nodes_p[:, -1, 0], want_roots[0:-1:2]) and np.array_equal(nodes_p[:, -1, 1], want_roots[1::2])
        assert np.array_equal(nodes_s[:, -1, 0], want_roots[1::2]) and np.array_equal(nodes_s[:, -1, 1], want_roots[2::2])
        ta.holds(model.records, "cut inserts")
        _assert_tree(a, model.levels, "cut inserts")
        # the per-key route: locate, the lowest inert slot, indexed_insert, two cut record updates
        c0, head = cuts[0], 64 + 2 * length
        cur = list(records)
        for j, key in enumerate(keys):
            at, st = b.locate_keys(tb.view, _keys([key], K))
            p = int(at[0])
            free = next(i for i, r in enumerate(cur) if not r[:K] < r[K: 2 * K])
            assert st[0] == 0 and [p, free] == index[j].tolist()
            idx, new = W.indexed_insert(cur[p], p, key, free, payload=payloads[j])
            two, pub = b.update_record_segments(tb.view, idx, new, cuts)
            for i, rec in zip(idx, new):
                cur[i] = rec.tobytes()
            low = (p & ((1 << c0) - 1)) | (free & ((1 << c0) - 1)) << c0
            want0 = np.concatenate([np.zeros(128, dtype=np.uint8), np.frombuffer(key, dtype=np.uint8), two[0][0, 64: 64 + length], two[0][1, 64: head],
                                    two[0][0, head: head + 32 * c0], two[0][1, head: head + 32 * c0],
                                    np.frombuffer(low.to_bytes((2 * c0 + 7) // 8, "little"), dtype=np.uint8)])
            assert np.array_equal(rows[0][j], want0), j
            for g in range(1, len(cuts) + 1):
                assert np.array_equal(rows[g][2 * j: 2 * j + 2], two[g]), (j, g)
            assert np.array_equal(nodes_p[j], pub[0]) and np.array_equal(nodes_s[j], pub[1]), j
        assert np.array_equal(ta.whole.cpu().numpy(), tb.whole.cpu().numpy())
        _assert_tree(b, model.levels, "per key")
        bits = a.insert_key_segment_bits(ta.view, _keys([_key(7, K)], K), cuts)[0]
        assert [x.shape for x in bits] == [(1, 1024 + 8 * K + 24 * length + 514 * c0)] + [(2, 1024 + 257 * (hi - lo)) for lo, hi in _edges(depth, cuts)[1:]]
    finally:
        ctx.set_timing(False)
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. MFH_EINVAL, ordering
def test_einval(ctx, W):
    lib, h = ctx.lib, ctx._h
    depth, K, length = 3, 4, 8
    rng = np.random.default_rng(16600)
    records = _table(W, [_key(0x10 << 24, K)], K, depth, length, rng)
    from merkle_insert_model import InsertModel

    levels = InsertModel(records, K).levels
    vp = ctypes.c_void_p
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _counts(ctx)
        idx = np.array([5, 0, 7], dtype=np.uint32)
        d_new = ctx.to_device(np.full(3 * 32, 0xEE, dtype=np.uint8))
        d_rec = ctx.to_device(np.full((3, length), 0xEE, dtype=np.uint8))
        keys = _keys([_key(5, K), _key(6, K), _key(9, K)], K)
        roots = np.full((7, 32), 0xCD, dtype=np.uint8)
        index, status = np.full((3, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        good = np.array([1, 2], dtype=np.uint32)
        row0 = {"rows": 128 + 32 + 1, "records": 64 + 2 * length + 32 + 1, "keys": 128 + K + 3 * length + 64 + 1}
        calls = {
            "rows": lambda n, c, r, s: lib.mfh_merkle_update_rows_cut(h, tree._h, 3, vp(idx.ctypes.data), vp(d_new.data_ptr()), n, c, r, s, vp(roots.ctypes.data)),
            "records": lambda n, c, r, s: lib.mfh_merkle_update_records_cut(h, tree._h, 3, vp(idx.ctypes.data), vp(table.view.data_ptr()), table.stride, length,
                                                                            vp(d_rec.data_ptr()), length, n, c, r, s, vp(roots.ctypes.data)),
            "keys": lambda n, c, r, s: lib.mfh_merkle_insert_keys_cut(h, tree._h, vp(table.view.data_ptr()), table.stride, length, K, 3, vp(keys.ctypes.data), K, None, 0,
                                                                      n, c, r, s, vp(roots.ctypes.data), vp(index.ctypes.data), vp(status.ctypes.data)),
        }
        for name, call in calls.items():
            who = {"rows": "mfh_merkle_update_rows_cut", "records": "mfh_merkle_update_records_cut", "keys": "mfh_merkle_insert_keys_cut"}[name]
            nupper = 6 if name == "keys" else 3
            bufs = [np.full((3, row0[name] + 2), 0xAB, dtype=np.uint8), np.full((nupper, 161 + 2), 0xAB, dtype=np.uint8), np.full((nupper, 161), 0xAB, dtype=np.uint8)]
            ptrs = (ctypes.c_void_p * 3)(*[b.ctypes.data for b in bufs])
            strides = (ctypes.c_size_t * 3)(*[b.shape[1] for b in bufs])
            texts = []

            def refused(rc):
                assert rc == EINVAL, (name, rc)
                text = lib.mfh_last_error(h).decode()
                assert text.startswith(who + ": "), text
                texts.append(text)

            cp = vp(good.ctypes.data)
            refused(call(0, cp, ptrs, strides))  # no cuts
            refused(call(2, None, ptrs, strides))
            for bad in ([0, 2], [1, 3], [2, 2], [2, 1], [1, 8]):  # below 1, not below the depth, not ascending
                arr = np.array(bad, dtype=np.uint32)
                refused(call(2, vp(arr.ctypes.data), ptrs, strides))
            refused(call(2, cp, None, strides))  # a null pointer array
            refused(call(2, cp, ptrs, None))
            for g in range(3):  # a null segment pointer, a short stride
                holed = (ctypes.c_void_p * 3)(*[None if j == g else b.ctypes.data for j, b in enumerate(bufs)])
                refused(call(2, cp, holed, strides))
                short = (ctypes.c_size_t * 3)(*[(row0[name] if j == 0 else 161) - 1 if j == g else b.shape[1] for j, b in enumerate(bufs)])
                refused(call(2, cp, ptrs, short))
            assert len(set(texts)) == 5, sorted(set(texts))  # no cuts (ncuts 0 or h_cuts null) | bad cuts | a null array | a null segment | a short stride
            assert all((b == 0xAB).all() for b in bufs) and (roots == 0xCD).all() and (status == 0xCD).all(), name
            assert _counts(ctx) == dict.fromkeys(KINDS, 0), name
            _assert_tree(tree, levels, name)
            table.holds(records, name)
        ctx.set_timing(False)
        for bad in ([], [0], [3], [2, 1], None):
            with pytest.raises(ctx_error()):
                tree.update_segments([1], bytes(32), bad)
        _assert_tree(tree, levels, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


def ctx_error():
    import c_lwe_snarks_amd as m

    return m.MfhError


def test_late_table_on_a_callers_stream(gpu_ctx_factory, mf, W):
    import torch

    depth, K, length, nk, cuts = 9, 4, 16, 32, [4]
    rng = np.random.default_rng(16700)
    members = sorted({rng.bytes(K) for _ in range(200)})
    records = _table(W, members, K, depth, length, rng)
    keys = [rng.bytes(K) for _ in range(nk)]
    payloads = [rng.bytes(length - 2 * K) for _ in keys]
    want_rows, want_p, want_s, want_index, _, model = insert_batch(records, K, keys, payloads, cuts)  # (first: nothing of the host's between the late table and the calls)
    pay = np.frombuffer(b"".join(payloads), dtype=np.uint8).reshape(nk, length - 2 * K).copy()
    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        tree = c.merkle_tree(depth)
        try:
            table = Placed(c, records, stride=length + 1, off=1, late=True)
            tree.set_records(0, table.view)  # no wait before it, nor before the next
            rows, nodes_p, nodes_s, index = tree.insert_key_segments(table.view, _keys(keys, K), cuts, pay)
            assert np.array_equal(index, want_index) and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s)
            assert all(np.array_equal(a, b) for a, b in zip(rows, want_rows))
            table.holds(model.records, "late table")
            _assert_tree(tree, model.levels, "late table")
        finally:
            tree.close()
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def _prover(ctx, p, cc, rng, n):
    """setup for the compiled statement on ctx, whose rows _witnesses has registered: (prove(witness rows) -> proofs, verify(proofs, statements) -> [bool])"""
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    lu = cc.lu
    ctx.ssp_prepare(None)
    alpha, beta, s = (int(x) for x in rng.integers(1, C.P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()
    vk = ctx.derive_vk(None, s, lu)

    def prove(witness):
        deltas = [int(x) for x in rng.integers(0, C.P, size=n, dtype=np.uint64)]
        mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(n)]
        signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(n)]
        return ctx.prove_batch_public(d_crs, None, lu, [witness[k].tobytes() for k in range(n)], deltas, mags, signs).clone()

    def verify(proofs, statements):
        return [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, statements), np.uint8)]

    return prove, verify


def _witnesses(ctx, cc, bits):
    prog = ctx.circuit_load(cc, state="auto")
    try:
        witness, holds = ctx.circuit_assign(prog, bits)
        assert holds.all()
        ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count.any() and (first == 0xFFFFFFFF).all()
        return witness
    finally:
        prog.close()


def test_end_to_end_leaf_updates(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    low, seg = W.MerkleUpdate(1), W.MerkleSegment(1)
    cc_low, cc_seg = low.circuit.compile(p), seg.circuit.compile(p)
    assert (cc_low.lu, cc_seg.lu) == (512, 1024) and (cc_seg.nwires, cc_seg.nrows) == W.MERKLE_SEGMENT_SIZES[1]
    rng = np.random.default_rng(16800)
    leaves = _leaves(rng, 4)
    indices = [0, 1, 3, 0, 2]
    new = _leaves(rng, 5)
    tree = ctx.merkle_tree(2)
    try:
        tree.set_leaves(0, b"".join(leaves))
        bits, nodes, roots = tree.update_segment_bits(indices, b"".join(new), [1], roots=True)
    finally:
        tree.close()
    want_rows, want_nodes, want_roots, _ = leaf_batch(leaves, indices, new, [1])
    assert [b.shape for b in bits] == [(5, 1024 + 257), (5, 1024 + 257)] and np.array_equal(nodes, want_nodes) and np.array_equal(roots, want_roots)
    assert all(np.array_equal(np.packbits(b, axis=1, bitorder="little"), w) for b, w in zip(bits, want_rows))
    # the verifier's side: statements from the published list alone
    pub = [[(nodes[k, g, 0].tobytes(), nodes[k, g, 1].tobytes()) for g in range(2)] for k in range(5)]
    own_low = [W.MerkleUpdate.statement(*pub[k][0]) for k in range(5)]
    own_seg = [W.MerkleSegment.chain(pub[k])[0] for k in range(5)]
    assert len(set(own_low)) == 5 and len(set(own_seg)) == 5 and all(len(x) == 128 for x in own_seg)
    assert all(pub[k][1] == (roots[k].tobytes(), roots[k + 1].tobytes()) for k in range(5))

    w_low = _witnesses(ctx, cc_low, bits[0])
    assert [low.roots_of(w_low[k]) for k in range(5)] == [pub[k][0] for k in range(5)]
    prove, verify = _prover(ctx, p, cc_low, rng, 5)
    proofs = prove(w_low)
    assert own_low == [w_low[k][:64].tobytes() for k in range(5)]
    assert verify(proofs, own_low) == [True] * 5
    assert verify(proofs, own_low[1:] + own_low[:1]) == [False] * 5

    w_seg = _witnesses(ctx, cc_seg, bits[1])
    assert [seg.tops_of(w_seg[k]) for k in range(5)] == [pub[k][1] for k in range(5)]
    prove, verify = _prover(ctx, p, cc_seg, rng, 5)
    proofs = prove(w_seg)
    assert own_seg == [w_seg[k][:128].tobytes() for k in range(5)]
    assert verify(proofs, own_seg) == [True] * 5
    assert verify(proofs, own_seg[1:] + own_seg[:1]) == [False] * 5
    # one published node swapped for the other update's: the lower old node, the lower new node, the old root, the new root
    for part in range(4):
        swapped = []
        for k in range(5):
            args = [pub[k][0][0], pub[k][0][1], pub[k][1][0], pub[k][1][1]]
            j = (k + 1) % 5
            args[part] = [pub[j][0][0], pub[j][0][1], pub[j][1][0], pub[j][1][1]][part]
            swapped.append(W.MerkleSegment.statement(*args))
        assert all(a != b for a, b in zip(swapped, own_seg))
        assert verify(proofs, swapped) == [False] * 5, part
    print(f"test_end_to_end_leaf_updates (MerkleUpdate(1) + MerkleSegment(1), d = 2^17): {time.time() - t0:.1f} s")


def test_end_to_end_insert(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p19, p17 = mf.Params(d=1 << 19, m=349525), mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p19)
    ctx.set_seed(SEED)
    K, length, depth, cuts = 4, 8, 2, [1]
    st, seg = W.MerkleInsert(K, length, 1, joined=False), W.MerkleSegment(1)
    cc = st.circuit.compile(p19)
    assert cc.lu == st.lu == 1056 and (cc.nwires, cc.nrows) == W.MERKLE_INSERT_SPLIT_SIZES[(K, length, 1)]
    rng = np.random.default_rng(16900)
    member = _key(0x6789ABCD, K)
    records = [r.tobytes() for r in W.indexed_records(_keys([_key(0x10, K), _key(0x7000_0000, K)], K), depth)]  # slots 0 .. 2 live, 3 inert
    want_rows, want_p, want_s, want_index, want_roots, model = insert_batch(records, K, [member], None, cuts)
    assert want_index.tolist() == [[1, 3]]  # p and s in two depth-1 subtrees
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        bits, nodes_p, nodes_s, index = tree.insert_key_segment_bits(table.view, _keys([member], K), cuts)
        table.holds(model.records, "end to end")
    finally:
        tree.close()
    assert index.tolist() == [[1, 3]] and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s)
    assert all(np.array_equal(np.packbits(b, axis=1, bitorder="little"), w) for b, w in zip(bits, want_rows))
    pub_p = [(nodes_p[0, g, 0].tobytes(), nodes_p[0, g, 1].tobytes()) for g in range(2)]
    pub_s = [(nodes_s[0, g, 0].tobytes(), nodes_s[0, g, 1].tobytes()) for g in range(2)]
    r0, r_mid, r1 = (r.tobytes() for r in want_roots)
    assert pub_p[1] == (r0, r_mid) and pub_s[1] == (r_mid, r1) and len({r0, r_mid, r1}) == 3  # R_mid is shared by the two chains
    own = st.statement(*pub_p[0], *pub_s[0], member)

    witness = _witnesses(ctx, cc, bits[0])
    assert st.tops_of(witness[0]) == pub_p[0] + pub_s[0] and own == witness[0][: st.lu // 8].tobytes()
    prove, verify = _prover(ctx, p19, cc, rng, 1)
    proofs = prove(witness)
    assert verify(proofs, [own]) == [True]
    assert verify(proofs, [st.statement(*pub_p[0], *pub_s[0], _key(0x6789ABCE, K))]) == [False]
    assert verify(proofs, [st.statement(*pub_p[0], pub_s[0][1], pub_s[0][0], member)]) == [False]
    assert verify(proofs, [st.statement(pub_s[0][0], pub_p[0][1], pub_p[0][0], pub_s[0][1], member)]) == [False]

    c17 = gpu_ctx_factory(p17)
    c17.set_seed(SEED)
    cs = seg.circuit.compile(p17)
    w_seg = _witnesses(c17, cs, bits[1])
    assert [seg.tops_of(w_seg[k]) for k in range(2)] == [pub_p[1], pub_s[1]]
    prove, verify = _prover(c17, p17, cs, rng, 2)
    proofs = prove(w_seg)
    own_seg = [W.MerkleSegment.chain(pub_p)[0], W.MerkleSegment.chain(pub_s)[0]]
    assert verify(proofs, own_seg) == [True, True]
    assert verify(proofs, own_seg[::-1]) == [False, False]
    broken = [W.MerkleSegment.statement(*pub_p[0], r0, r1), W.MerkleSegment.statement(*pub_s[0], r0, r1)]  # chains that skip R_mid
    assert verify(proofs, broken) == [False, False]
    print(f"test_end_to_end_insert (MerkleInsert(4, 8, 1, joined=False) at d = 2^19, two MerkleSegment(1) at d = 2^17): {time.time() - t0:.1f} s")
