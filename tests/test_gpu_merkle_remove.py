"""GPU: a batch of sequential key removes from an indexed table on the device in ONE call (mfh_merkle_remove_keys, MerkleTree.remove_keys / remove_bits) and
with the path cut (mfh_merkle_remove_keys_cut, MerkleTree.remove_key_segments).

Every case compares h_index, h_status, the rows, the roots, the table's whole allocation (tests/test_gpu_merkle_record_update.py's Placed, with its 0xA5
surroundings) and the tree's nodes against
  the per-key route through the EXISTING calls on a second tree and table: per key locate_keys for the key's own record, a search of a host copy of the table
  for the lowest live record whose hi is the key, words.indexed_remove, update_records -- the remove's row put together out of the two MerkleRecordUpdate
  rows; and
  the brute-force model of tests/merkle_remove_model.py, its rows MerkleRemove.bits on a stand-in made without its circuit (test 1's first case checks that the
  stand-in and the real statement give the same bits).

1. hand-made sets at depth 2 and 3, key_bytes 1 and 4: one remove; the smallest member (P is the sentinel record); the largest (the inherited hi is FF..FF);
   three adjacent members in ascending, descending and middle-first order; every member, down to the empty set.
2. key widths 1, 3, 4, 5, 8, 20, 32 at depth 3.
3. alignment at key_bytes 4 and 5: lengths 2K, 2K + 1, 2K + 15, 2K + 16, 55, 64, 65; the table 0 .. 3 bytes into its tensor; strides length and length + 5;
   an adjacent pair (the inherited hi is a key of the batch) and a single member (it is a hi of the table).
4. a key's own record and its predecessor on both sides of a wave's and a workgroup's boundary (indices 63 / 64 and 255 / 256, depth 8 and 9); a shuffled
   table at depth 12 with 300 removes; a malformed table with two live records sharing one hi, and two sharing one lo: the lowest index.
5. refusals after the search (a non-member, a member without a predecessor): MFH_EINVAL, h_status filled, nothing written, no record or tree kernel; every
   up-front MFH_EINVAL case leaves the timing counts as they were; nk = 0 does nothing.
6. h_inputs = NULL; the launch counts of one chunk; a wider in_stride keeps its tail; scrubbed staging; a table produced late on the null stream and on a
   caller's.
7. two chunks: key_bytes 4, length 2^19 (a row is 1 049 094 bytes, a chunk 63 removes), 64 removes -- at depth 7: a depth-6 table holds 63 members at most.
8. after a batch, locate_keys / absent_rows on the shrunk table answer as the model does; insert_keys followed by remove_keys of the same keys restores the
   table's bytes and the root.
9. the cut call at depth 3 under [1], [2], [1, 2] and at depth 9 under [4]: rows, nodes and roots against the model and against the uncut rows sliced.
10. end to end with MerkleRemove(4, 8, 1) at Params(d=1 << 19, m=349525), and one cut removal at depth 3 under [1] with its MerkleSegment(2) proofs."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

from merkle_remove_model import RemoveModel, remove_cut_batch, row_bytes, stand_in
from test_gpu_merkle import _assert_tree, _flip
from test_gpu_merkle_absent import IndexedModel, _key, _keys, _table
from test_gpu_merkle_record_update import Placed
from test_gpu_merkle_segments import _prover, _witnesses

pytestmark = pytest.mark.gpu

SEED = bytes((47 * i + 3) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_owners", "merkle_remove_records", "merkle_locate", "merkle_inert", "merkle_insert_records", "sha256_records", "merkle_record_rows", "merkle_updates",
         "merkle_level", "merkle_paths", "merkle_absent_rows", "merkle_segments")


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


# ---------------------------------------------------------------------------------------------------------------- the two references
def _raw(ctx, tree, table, K, keys, rows, roots, index, status, nk=None, in_stride=None, key_stride=None):
    vp = ctypes.c_void_p
    ptr = lambda a: vp(a.ctypes.data) if a is not None else None  # noqa: E731
    return ctx.lib.mfh_merkle_remove_keys(ctx._h, tree._h if tree is not None else None, vp(table.view.data_ptr()) if table is not None else None, table.stride if table else 0,
                                          table.length if table else 0, K, len(keys) if nk is None else nk, ptr(keys), keys.shape[1] if key_stride is None else key_stride,
                                          ptr(rows), (rows.shape[1] if rows is not None else 0) if in_stride is None else in_stride, ptr(roots), ptr(index), ptr(status))


def _live(r, K):
    return r[:K] < r[K: 2 * K]


def _sequential(ctx, W, records, K, keys, **placing):
    """the route a user has without the call, one key at a time on a tree and table of its own: (index, rows, roots, the table's image, the tree's levels)"""
    records = list(records)
    length, depth = len(records[0]), len(records).bit_length() - 1
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        index, roots = [], [tree.root()]
        rows = np.zeros((len(keys), row_bytes(K, length, depth)), dtype=np.uint8)
        for j, key in enumerate(keys):
            at, st = tree.locate_keys(table.view, _keys([key], K))
            assert st[0] == 1
            s = int(at[0])
            p = next(i for i, r in enumerate(records) if _live(r, K) and r[K: 2 * K] == key)
            idx, new = W.indexed_remove(records[p], p, records[s], s, key_bytes=K)
            two, r = tree.update_records(table.view, idx, new, roots=True)
            for i, rec in zip(idx, new):
                records[i] = rec.tobytes()
            index.append(idx)
            roots.append(r[2].tobytes())
            head = 64 + 2 * length
            bits = sum(((p >> l) & 1) << l | ((s >> l) & 1) << (depth + l) for l in range(depth))
            rows[j] = np.concatenate([np.zeros(64, dtype=np.uint8), np.frombuffer(key, dtype=np.uint8), two[0, 64: 64 + length], two[1, 64: 64 + length],
                                      two[0, head: head + 32 * depth], two[1, head: head + 32 * depth],
                                      np.frombuffer(bits.to_bytes((2 * depth + 7) // 8, "little"), dtype=np.uint8)])
        levels = [tree.nodes(l).cpu().numpy().tobytes() for l in range(depth + 1)]
        return np.array(index, dtype=np.uint32).reshape(len(keys), 2), rows, roots, table.whole.cpu().numpy(), levels
    finally:
        tree.close()


def _remove(ctx, tree, table, K, keys):
    """one raw call: (rc, rows, roots, index, status)"""
    nk, depth = len(keys), tree.depth
    rows = np.zeros((nk, row_bytes(K, table.length, depth)), dtype=np.uint8)
    roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.full((nk, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(nk, 0xCD, dtype=np.uint8)
    rc = _raw(ctx, tree, table, K, _keys(keys, K), rows, roots, index, status)
    return rc, rows, roots, index, status


def _check(ctx, W, records, K, keys, what, seq=None, model=None, **placing):
    """one batch on a fresh tree and table against the per-key route (seq: its results, when another placing has them already) and the model"""
    depth = len(records).bit_length() - 1
    if model is None:
        model = RemoveModel(records, K)
        model.want = model.remove_batch(keys)
    want_index, want_rows, want_roots = model.want
    own = seq is None  # (another placing's sequential result is compared in everything but the allocation's image)
    if own:
        seq = _sequential(ctx, W, records, K, keys, **placing)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        rc, rows, roots, index, status = _remove(ctx, tree, table, K, keys)
        assert rc == 0, (what, ctx.lib.mfh_last_error(ctx._h).decode())
        assert np.array_equal(index, want_index) and (status == 1).all(), (what, index, want_index, status)
        assert [r.tobytes() for r in roots] == want_roots, what
        assert np.array_equal(rows, want_rows), what
        table.holds(model.records, what)
        _assert_tree(tree, model.levels, what)
        s_index, s_rows, s_roots, s_image, s_levels = seq
        assert np.array_equal(index, s_index) and np.array_equal(rows, s_rows), what
        assert [r.tobytes() for r in roots] == s_roots, what
        if own:
            assert np.array_equal(table.whole.cpu().numpy(), s_image), what
        assert [tree.nodes(l).cpu().numpy().tobytes() for l in range(depth + 1)] == s_levels, what
    finally:
        tree.close()
    return model, seq


def _members(K, count):
    top = 0x10 << (8 * (K - 1))
    xs = (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))
    return [_key(x, K) for x in xs][:count]


# ---------------------------------------------------------------------------------------------------------------- 1. hand-made sets
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("depth", [2, 3])
def test_hand_made_sets(ctx, W, depth, K):
    rng = np.random.default_rng(17000 + 10 * depth + K)
    length = 2 * K + 3
    members = _members(K, (1 << depth) - 1)  # a full table: record 0 the sentinel's, record r member r - 1's
    records = _table(W, members, K, depth, length, rng)
    placing = dict(stride=length + 3, off=1)
    if depth == 2 and K == 4:  # the stand-in gives what the statement gives
        args = RemoveModel(records, K).remove(members[1])[2]
        assert np.array_equal(stand_in(K, length, depth).bits(*args), W.MerkleRemove(K, length, depth).bits(*args))
    model, _ = _check(ctx, W, records, K, [members[1]], (depth, K, "one"), **placing)
    assert model.want[0].tolist() == [[1, 2]]
    model, _ = _check(ctx, W, records, K, [members[0]], (depth, K, "the smallest"), **placing)
    assert model.want[0].tolist() == [[0, 1]] and model.records[0][:2 * K] == bytes(K) + members[1]
    model, _ = _check(ctx, W, records, K, [members[-1]], (depth, K, "the largest"), **placing)
    last = len(members)
    assert model.want[0].tolist() == [[last - 1, last]] and model.records[last - 1][K: 2 * K] == b"\xff" * K
    if depth == 3:
        a, b, c = members[2], members[3], members[4]  # records 3, 4, 5; record 2's hi is a
        for order, want_p in (((a, b, c), [2, 2, 2]), ((c, b, a), [4, 3, 2]), ((b, a, c), [3, 2, 2]), ((b, c, a), [3, 3, 2])):
            model, _ = _check(ctx, W, records, K, list(order), (K, "three adjacent", order), **placing)
            assert model.want[0][:, 0].tolist() == want_p and sorted(model.want[0][:, 1].tolist()) == [3, 4, 5]
            assert model.records[2][: 2 * K] == members[1] + members[5]
    # every member, down to the empty set: shuffled, and in descending order (every P is the record just below)
    for order in ([members[int(i)] for i in rng.permutation(len(members))], members[::-1]):
        model, _ = _check(ctx, W, records, K, order, (depth, K, "every member"), stride=length, off=3)
        assert model.records == [bytes(K) + b"\xff" * K + records[0][2 * K:]] + [bytes(length)] * ((1 << depth) - 1)


# ---------------------------------------------------------------------------------------------------------------- 2. key widths
@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 20, 32])
def test_key_widths(ctx, W, K):
    depth = 3
    rng = np.random.default_rng(17100 + K)
    length = 2 * K + 1
    if K == 1:
        members = [bytes([x]) for x in (0x10, 0x50, 0x51, 0x60, 0xFE)]
    else:
        rest, mid = rng.bytes(K - 1), rng.bytes(K - 2)
        # neighbours that differ in the last byte alone, in the first byte alone, and ..00 FF against ..01 00: ordered as integers
        members = [bytes([0x10]) + rest, bytes([0x20]) + rest, bytes([0x50]) + mid + bytes([0x10]), bytes([0x50]) + mid + bytes([0x11]), bytes([0x60]) + bytes(K - 2) + b"\xff",
                   bytes([0x60]) + bytes(K - 3) + b"\x01\x00"]
    assert members == sorted(members)
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    keys = [members[int(i)] for i in rng.permutation(len(members))][:-1]
    _check(ctx, W, records, K, keys, K, stride=length + 2, off=3)


# ---------------------------------------------------------------------------------------------------------------- 3. alignment
@pytest.mark.parametrize("K", [4, 5])
def test_alignment_sweep(ctx, W, K):
    depth = 3
    for length in (2 * K, 2 * K + 1, 2 * K + 15, 2 * K + 16, 55, 64, 65):
        rng = np.random.default_rng(17200 + 100 * K + length)
        members = sorted({rng.bytes(K) for _ in range(6)})
        records = _table(W, members, K, depth, length, rng)
        records = [records[i] for i in rng.permutation(8)]
        keys = [members[2], members[1], members[4]]  # 2 first: 1 then inherits a hi that is no hi of the table before the batch; 4: a hi of the table
        model = seq = None
        for stride in (length, length + 5):
            for off in range(4):
                what = (K, length, stride, off)
                model, got = _check(ctx, W, records, K, keys, what, seq=seq, model=model, stride=stride, off=off)
                seq = got
        keys = [members[1], members[2], members[5]]  # 1 first: its new hi is the KEY members[2], still there; the largest member
        model = seq = None
        for stride, off in ((length, 1), (length + 5, 2)):
            model, seq = _check(ctx, W, records, K, keys, (K, length, stride, off, "a key as hi"), seq=seq, model=model, stride=stride, off=off)


# ---------------------------------------------------------------------------------------------------------------- 4. the search
@pytest.mark.parametrize("depth", [8, 9])
def test_own_and_prev_at_the_boundaries(ctx, W, depth):
    K, length = 8, 21
    n = 1 << depth
    rng = np.random.default_rng(17400 + depth)
    members = sorted({rng.bytes(K) for _ in range(n - 9)})
    assert len(members) == n - 9
    packed = _table(W, members, K, depth, length, rng)  # record r: rank r in key order, record 0 the sentinel's
    # (the rank of the key's own record, its slot, its predecessor's slot): both sides of a wave's and a workgroup's boundary, either way round, and the ends
    want = [(10, 63, 64), (20, 128, 127), (30, n - 1, 0), (40, 1, n - 2)] + ([(50, 256, 255), (60, 319, 320)] if depth == 9 else [])
    slot_of = {}
    for rank, s, p in want:
        slot_of[rank], slot_of[rank - 1] = s, p
    rest = iter(int(i) for i in rng.permutation(n) if int(i) not in set(slot_of.values()))
    records = [None] * n
    for r, rec in enumerate(packed):
        records[slot_of[r] if r in slot_of else next(rest)] = rec
    keys = [packed[rank][:K] for rank, _, _ in want]
    model, _ = _check(ctx, W, records, K, keys, (depth, "boundaries"), stride=length + 1, off=2)
    assert model.want[0].tolist() == [[p, s] for _, s, p in want]


def test_shuffled_table_depth_12(ctx, W):
    depth, K, length, nk = 12, 8, 24, 300
    rng = np.random.default_rng(17500)
    members = sorted({rng.bytes(K) for _ in range(3000)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    run = members[700:740]  # forty adjacent members, shuffled among the others
    others = [members[int(i)] for i in rng.permutation(3000) if not 700 <= int(i) < 740][: nk - 40]
    keys = run + others
    keys = [keys[int(i)] for i in rng.permutation(nk)]
    model, _ = _check(ctx, W, records, K, keys, "depth 12", stride=length + 9, off=3)
    assert len(set(model.want[0][:, 1].tolist())) == nk and sum(model.live(i) for i in range(1 << depth)) == 1 + 3000 - nk


def test_malformed_table_lowest_index(ctx, W):
    depth, K, length = 3, 2, 7
    rng = np.random.default_rng(17600)
    rec = lambda lo, hi: _key(lo, K) + _key(hi, K) + rng.bytes(length - 2 * K)  # noqa: E731
    # 0x5000 is the hi of records 5 and 2 and the lo of records 6 and 3; 0x9000's own record is 7, and its predecessors are 6 and 3
    records = [rec(0, 0x1000), rec(0x1000, 0x3000), rec(0x3000, 0x5000), rec(0x5000, 0x9000), bytes(length), rec(0x2000, 0x5000), rec(0x5000, 0x9000), rec(0x9000, 0xFFFF)]
    model, _ = _check(ctx, W, records, K, [_key(0x5000, K)], "two share a hi, two a lo", stride=length + 1, off=1)
    assert model.want[0].tolist() == [[2, 3]]
    model, _ = _check(ctx, W, records, K, [_key(0x9000, K)], "two predecessors", stride=length + 1, off=1)
    assert model.want[0].tolist() == [[3, 7]]


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def _drain(ctx):
    return {kind: ctx.timing_drain(kind)[0] for kind in KINDS}


def test_refusals_after_the_search(ctx, W):
    depth, K, length = 3, 2, 6
    rng = np.random.default_rng(17700)
    rec = lambda lo, hi: _key(lo, K) + _key(hi, K) + rng.bytes(length - 2 * K)  # noqa: E731
    # no live record has 0x7000 as its hi: a member without a predecessor; 0x6000 is the lo of an inert record alone
    records = [bytes(length), rec(0x1000, 0x2000), rec(0x2000, 0x6800), rec(0x9000, 0x8000), rec(0, 0x1000), rec(0x7000, 0xFFFF), rec(0x6000, 0x6000), bytes(length)]
    model = RemoveModel(records, K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        cases = [("a non-member", [0x1000, 0x1800, 0x2000], [[4, 1], [NONE, NONE], [1, 2]], [1, 0, 1]),
                 ("the lo of an inert record", [0x6000, 0x2000], [[NONE, NONE], [1, 2]], [0, 1]),
                 ("a hi that is no lo", [0x6800], [[2, NONE]], [0]),
                 ("a member without a predecessor", [0x2000, 0x7000], [[1, 2], [NONE, 5]], [1, 2])]
        texts = set()
        for what, xs, want_i, want_s in cases:
            rc, rows, roots, index, status = _remove(ctx, tree, table, K, [_key(x, K) for x in xs])
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_remove_keys: "), (what, rc, text)
            texts.add(text)
            assert status.tolist() == want_s and index.tolist() == want_i, (what, status, index)
            assert not rows.any() and not roots.any(), what
            counts = _drain(ctx)
            assert counts == dict.fromkeys(KINDS, 0) | {"merkle_owners": 1}, (what, counts)
            table.holds(records, what)
            _assert_tree(tree, model.levels, what)
        assert len(texts) == 2  # not a member | no predecessor
        ctx.set_timing(False)
        rc, rows, roots, index, status = _remove(ctx, tree, table, K, [_key(x, K) for x in (0x2000, 0x1000)])
        assert rc == 0 and index.tolist() == [[1, 2], [4, 1]] and status.tolist() == [1, 1]
    finally:
        ctx.set_timing(False)
        tree.close()


def test_einval_up_front(ctx, mf, W):
    import torch

    lib, h = ctx.lib, ctx._h
    depth, K, length = 3, 4, 17
    rng = np.random.default_rng(17800)
    members = sorted({rng.bytes(K) for _ in range(5)})
    records = _table(W, members, K, depth, length, rng)
    model = RemoveModel(records, K)
    rowb = row_bytes(K, length, depth)
    tree = ctx.merkle_tree(depth)
    vp = ctypes.c_void_p

    try:
        table = Placed(ctx, records, stride=length + 3, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        keys = _keys(members[1:4], K)
        zero, ones, twice = keys.copy(), keys.copy(), keys.copy()
        zero[1], ones[2], twice[2] = 0, 0xFF, twice[0]
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((7, 32), 0xAB, dtype=np.uint8)
        index, status = np.full((3, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        kp, zp, op, wp, bp, rp, ip, sp = (vp(a.ctypes.data) for a in (keys, zero, ones, twice, buf, roots, index, status))
        tp, ts, stride = vp(table.view.data_ptr()), table.stride, buf.shape[1]
        # the cut call's own arguments: cuts [1], segment 0's rows and the upper segment's
        cut = np.array([1], dtype=np.uint32)
        seg0, seg1 = np.full((3, row_bytes(K, length, 1, zeros=128) + 2), 0xAB, dtype=np.uint8), np.full((6, 128 + 64 + 1), 0xAB, dtype=np.uint8)
        ptrs = (ctypes.c_void_p * 2)(seg0.ctypes.data, seg1.ctypes.data)
        strides = (ctypes.c_size_t * 2)(seg0.shape[1], seg1.shape[1])
        cp = vp(cut.ctypes.data)

        def plain(t, table_p, table_s, length_, K_, nk, keys_p, key_s, rows_p, in_s, index_p, status_p, handle=h):
            return lib.mfh_merkle_remove_keys(handle, t, table_p, table_s, length_, K_, nk, keys_p, key_s, rows_p, in_s, rp, index_p, status_p)

        def cut_call(t, table_p, table_s, length_, K_, nk, keys_p, key_s, rows_p, in_s, index_p, status_p, handle=h):
            return lib.mfh_merkle_remove_keys_cut(handle, t, table_p, table_s, length_, K_, nk, keys_p, key_s, 1, cp, ptrs, strides, rp, index_p, status_p)

        for who, f in (("mfh_merkle_remove_keys", plain), ("mfh_merkle_remove_keys_cut", cut_call)):
            texts = []

            def refused(rc, handle=h):
                assert rc == EINVAL, who
                text = lib.mfh_last_error(handle).decode()
                assert text.startswith(who + ": "), text
                texts.append(text)

            refused(f(None, tp, ts, length, K, 3, kp, K, bp, stride, ip, sp))  # a null tree
            refused(f(tree._h, tp, ts, length, 0, 3, kp, K, bp, stride, ip, sp))
            refused(f(tree._h, tp, ts, 66, 33, 3, kp, 33, bp, 1 << 12, ip, sp))
            texts.pop()  # (key_bytes 0 and 33: one text)
            refused(f(tree._h, tp, ts, 2 * K - 1, K, 3, kp, K, bp, stride, ip, sp))
            refused(f(tree._h, tp, (1 << 20) + 1, (1 << 20) + 1, K, 3, kp, K, bp, 1 << 23, ip, sp))
            refused(f(tree._h, tp, length - 1, length, K, 3, kp, K, bp, stride, ip, sp))
            refused(f(tree._h, tp, ts, length, K, 3, kp, K - 1, bp, stride, ip, sp))
            refused(f(tree._h, None, ts, length, K, 3, kp, K, bp, stride, ip, sp))
            refused(f(tree._h, tp, ts, length, K, 3, None, K, bp, stride, ip, sp))
            refused(f(tree._h, tp, ts, length, K, 3, kp, K, bp, stride, None, sp))
            refused(f(tree._h, tp, ts, length, K, 3, kp, K, bp, stride, ip, None))
            refused(f(tree._h, tp, ts, length, K, 9, kp, K, bp, stride, ip, sp))  # more keys than slots (read before any key is)
            refused(f(tree._h, tp, ts, length, K, 3, zp, K, bp, stride, ip, sp))
            refused(f(tree._h, tp, ts, length, K, 3, op, K, bp, stride, ip, sp))
            texts.pop()  # (the two sentinels: one text)
            refused(f(tree._h, tp, ts, length, K, 3, wp, K, bp, stride, ip, sp))
            if f is plain:
                refused(f(tree._h, tp, ts, length, K, 3, kp, K, bp, rowb - 1, ip, sp))  # a short in_stride with h_inputs given
                refused(f(tree._h, tp, ts, length, K, 3, zp, K, None, 0, ip, sp))  # no rows: a sentinel is refused too
                texts.pop()
            assert f(tree._h, tp, ts, length, K, 3, kp, K, bp, stride, ip, sp, handle=None) == EINVAL
            assert len(set(texts)) == len(texts) == (14 if f is plain else 13), sorted(texts)
            if torch.cuda.device_count() > 1:
                other = mf.Context(mf.DEBUG, 1)
                try:
                    assert f(tree._h, tp, ts, length, K, 3, kp, K, bp, stride, ip, sp, handle=other._h) == EINVAL
                    assert lib.mfh_last_error(other._h).decode() == who + ": the tree belongs to another device"
                finally:
                    other.close()
                    torch.cuda.set_device(ctx.device)
        # the cut call's own cases, as cuts_refused lists them
        g = lib.mfh_merkle_remove_keys_cut
        texts = []
        cut0, cut3 = np.array([0], dtype=np.uint32), np.array([3], dtype=np.uint32)
        for ncuts, cuts_p, rows_p, strides_p in [(0, cp, ptrs, strides), (1, None, ptrs, strides), (1, vp(cut0.ctypes.data), ptrs, strides),
                                                 (1, vp(cut3.ctypes.data), ptrs, strides), (1, cp, None, strides), (1, cp, ptrs, None),
                                                 (1, cp, (ctypes.c_void_p * 2)(None, seg1.ctypes.data), strides), (1, cp, (ctypes.c_void_p * 2)(seg0.ctypes.data, None), strides),
                                                 (1, cp, ptrs, (ctypes.c_size_t * 2)(seg0.shape[1] - 3, seg1.shape[1])), (1, cp, ptrs, (ctypes.c_size_t * 2)(seg0.shape[1], 192))]:
            assert g(h, tree._h, tp, ts, length, K, 3, kp, K, ncuts, cuts_p, rows_p, strides_p, rp, ip, sp) == EINVAL
            text = lib.mfh_last_error(h).decode()
            assert text.startswith("mfh_merkle_remove_keys_cut: "), text
            texts.append(text)
        assert len(set(texts)) == 5, sorted(set(texts))  # no cuts | bad cuts | a null array | a null segment | a short stride
        # nk = 0 does nothing, whatever the pointers
        assert plain(tree._h, None, ts, length, K, 0, None, K, None, 0, None, None) == 0
        assert plain(tree._h, tp, ts, length, K, 0, kp, K, bp, stride, ip, sp) == 0
        assert cut_call(tree._h, tp, ts, length, K, 0, kp, K, bp, stride, ip, sp) == 0
        none = np.zeros((0, K), dtype=np.uint8)
        rows0, index0, roots0 = tree.remove_keys(table.view, none, roots=True)
        assert rows0.shape == (0, rowb) and index0.shape == (0, 2) and index0.dtype == np.uint32 and roots0.tobytes() == model.root()
        assert tree.remove_bits(table.view, none)[0].shape == (0, 512 + 8 * K + 16 * length + 514 * depth)
        rows0, nodes_p0, nodes_s0, index0 = tree.remove_key_segments(table.view, none, [1])
        assert [r.shape[0] for r in rows0] == [0, 0] and nodes_p0.shape == nodes_s0.shape == (0, 2, 2, 32) and index0.shape == (0, 2)
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xAB).all() and (index == 0xCDCDCDCD).all() and (status == 0xCD).all() and (seg0 == 0xAB).all() and (seg1 == 0xAB).all()
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
        absent = _keys([bytes(a ^ 1 if i == K - 1 else a for i, a in enumerate(members[0]))], K)
        for bad_table, bad_keys in [(table.view, keys[0]), (table.view, keys.astype(np.int8)), (table.view, zero), (table.view, twice), (table.view, np.zeros((1, 9), dtype=np.uint8) + 1),
                                    (table.view[:4], keys), (table.view.cpu().numpy(), keys), (table.view, absent)]:
            for call in (tree.remove_keys, tree.remove_bits, lambda t, k: tree.remove_key_segments(t, k, [1]), lambda t, k: tree.remove_key_segment_bits(t, k, [2])):
                with pytest.raises(mf.MfhError):
                    call(bad_table, bad_keys)
        for bad_cuts in ([], [0], [3], [2, 1], None):
            with pytest.raises(mf.MfhError):
                tree.remove_key_segments(table.view, keys, bad_cuts)
        with pytest.raises(mf.MfhError) as e:
            tree.remove_keys(table.view, absent)
        assert "mfh_merkle_remove_keys: a key is not a member" in str(e.value)
        with pytest.raises(mf.MfhError) as e:
            tree.remove_key_segments(table.view, absent, [1])
        assert "mfh_merkle_remove_keys_cut: a key is not a member" in str(e.value)
        _assert_tree(tree, model.levels, "after the refused Python calls")
        table.holds(records, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. rows and streams
def test_no_rows_launch_counts_stride_and_scrub(ctx, W):
    depth, K, length, nk = 9, 8, 55, 100
    rng = np.random.default_rng(17900)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = _table(W, members, K, depth, length, rng)
    keys = [members[int(i)] for i in rng.permutation(300)[:nk]]
    model = RemoveModel(records, K)
    want_index, want_rows, want_roots = model.remove_batch(keys)
    rowb = row_bytes(K, length, depth)
    assert rowb == 64 + 8 + 110 + 576 + 3
    karr = _keys(keys, K)
    tree = ctx.merkle_tree(depth)
    try:
        # no rows: the same table, tree and roots
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.zeros((nk, 2), dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, karr, None, roots, index, status) == 0
        assert np.array_equal(index, want_index) and (status == 1).all() and [r.tobytes() for r in roots] == want_roots
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: v[0] for k, v in timed.items()} == dict.fromkeys(KINDS, 0) | {"merkle_owners": 1, "merkle_remove_records": 1, "sha256_records": 1, "merkle_record_rows": 1,
                                                                                  "merkle_updates": depth + 1}
        table.holds(model.records, "no rows")
        _assert_tree(tree, model.levels, "no rows")
        # rows, a wider in_stride, no roots: one chunk's launches
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        _drain(ctx)
        buf = np.full((nk, rowb + 13), 0xAB, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, karr, buf, None, index, status) == 0
        assert np.array_equal(buf[:, :rowb], want_rows) and (buf[:, rowb:] == 0xAB).all()
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | {
            "merkle_owners": (1, 1 << depth), "merkle_remove_records": (1, 2 * nk), "sha256_records": (1, 2 * nk), "merkle_record_rows": (2, 2 * nk),
            "merkle_updates": (depth + 1, 2 * nk * depth)}
        print(f"depth {depth}: {nk} removes: " + ", ".join(f"{k} {v[1]:.3f} ms" for k, v in timed.items() if v[0]))
        ctx.set_timing(False)
        table.holds(model.records, "rows")
        # the pinned staging zeroed between two calls; the Python calls
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        assert ctx.scrub_staging() == 0
        rows2, index2, roots2 = tree.remove_keys(table.view, karr, roots=True)
        assert np.array_equal(rows2, want_rows) and np.array_equal(index2, want_index) and [r.tobytes() for r in roots2] == want_roots
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        bits, index3 = tree.remove_bits(table.view, karr[:3])
        assert bits.shape == (3, 512 + 8 * K + 16 * length + 514 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows[:3])
        assert np.array_equal(index3, want_index[:3])
    finally:
        ctx.set_timing(False)
        tree.close()


def _late_table(ctx, W):
    depth, K, length, nk = 9, 4, 16, 64
    rng = np.random.default_rng(18000)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = _table(W, members, K, depth, length, rng)
    keys = [members[int(i)] for i in rng.permutation(len(members))[:nk]]
    model = RemoveModel(records, K)
    want_index, want_rows, want_roots = model.remove_batch(keys)  # (first: nothing of the host's stands between the late table and the calls)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        rows, index, roots = tree.remove_keys(table.view, _keys(keys, K), roots=True)
        assert np.array_equal(index, want_index) and np.array_equal(rows, want_rows) and [r.tobytes() for r in roots] == want_roots
        table.holds(model.records, "late table")
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


# ---------------------------------------------------------------------------------------------------------------- 7. two chunks
def test_two_chunks(ctx, W):
    depth, K, length = 7, 4, 1 << 19  # (depth 6 holds 63 members: one fewer than a chunk and a remove)
    rowb = row_bytes(K, length, depth)
    per_chunk = (64 << 20) // rowb
    nk = per_chunk + 1
    assert rowb == 64 + K + 2 * length + 64 * depth + 2 == 1049094 and per_chunk == 63 and nk == 64
    rng = np.random.default_rng(18100)
    members = sorted({rng.bytes(K) for _ in range(90)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    # adjacent members on both sides of the seam between removes 62 and 63: 63's P and inherited hi depend on chunk 0's removes
    picked = [members[int(i)] for i in rng.permutation(90) if not 40 <= int(i) < 45][: nk - 5]
    keys = picked + [members[i] for i in (42, 41, 44, 43, 40)]  # remove 63, chunk 1's only one: P is member 39's record, the hi member 44's, four removes away
    assert len(keys) == nk == len(set(keys))
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rc, rows, roots, index, status = _remove(ctx, tree, table, K, keys)
        counts = {kind: ctx.timing_drain(kind)[::2] for kind in KINDS}
        ctx.set_timing(False)
        assert rc == 0 and (status == 1).all()
        assert counts == dict.fromkeys(KINDS, (0, 0)) | {"merkle_owners": (1, 1 << depth), "merkle_remove_records": (1, 2 * nk), "sha256_records": (2, 2 * nk),
                                                         "merkle_record_rows": (4, 2 * nk), "merkle_updates": (2 * (depth + 1), 2 * nk * depth)}
        model = RemoveModel(records, K)
        want_index, want_rows, want_roots = model.remove_batch(keys)
        assert np.array_equal(index, want_index) and [r.tobytes() for r in roots] == want_roots and np.array_equal(rows, want_rows)
        table.holds(model.records, "two chunks")
        _assert_tree(tree, model.levels, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()
    # ... and the per-key route, on the records' first 40 bytes: the same indices (the rows and roots above are the model's)
    short = [r[:40] for r in records]
    _check(ctx, W, short, K, keys, "two chunks' batch, short records", stride=41, off=1)


# ---------------------------------------------------------------------------------------------------------------- 8. after a batch
def test_queries_after_a_batch_and_the_round_trip(ctx, W):
    depth, K, length, nk = 6, 5, 17, 12
    rng = np.random.default_rng(18200)
    members = sorted({rng.bytes(K) for _ in range(40)})
    records = W.indexed_records(_keys(members, K), depth, length=length, payloads=[rng.bytes(length - 2 * K) for _ in members])
    records = [r.tobytes() for r in records]  # in rank order, the unused slots all zero: the lowest inert slot is where an insert goes and a remove leaves
    gone = [members[int(i)] for i in rng.permutation(40)[:nk]]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        root0 = tree.root()
        model = RemoveModel(records, K)
        want = model.remove_batch(gone)
        rows, index = tree.remove_keys(table.view, _keys(gone, K))
        assert np.array_equal(index, want[0]) and np.array_equal(rows, want[1])
        shrunk = IndexedModel(model.records, K)
        queries = gone + [m for m in members if m not in gone][:10]
        want_i, want_s, want_rows = shrunk.answers(queries)
        rows, index, status = tree.absent_rows(table.view, _keys(queries, K))
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s) and np.array_equal(rows, want_rows)
        assert not status[:nk].any() and status[nk:].tolist() == [1] * 10  # the removed keys are absent now, each inside one live range
        index2, status2 = tree.locate_keys(table.view, _keys(queries, K))
        assert np.array_equal(index2, want_i) and np.array_equal(status2, want_s)
        table.holds(model.records, "shrunk")
        _assert_tree(tree, shrunk.levels, "shrunk")
        # the round trip from here: new keys in, with payloads, and out again in another order
        base, base_root = list(model.records), tree.root()
        fresh = [rng.bytes(K) for _ in range(9)]
        lo = int.from_bytes(fresh[0], "big")
        fresh += [_key(lo + x, K) for x in (3, 1, 2)]  # neighbours of one range
        pay = np.frombuffer(rng.bytes(len(fresh) * (length - 2 * K)), dtype=np.uint8).reshape(len(fresh), length - 2 * K).copy()
        tree.insert_keys(table.view, _keys(fresh, K), pay)
        assert tree.root() != base_root
        back = [fresh[int(i)] for i in rng.permutation(len(fresh))]
        rows, index, roots = tree.remove_keys(table.view, _keys(back, K), roots=True)
        table.holds(base, "the round trip")
        assert tree.root() == base_root == roots[-1].tobytes() and base_root != root0
        _assert_tree(tree, shrunk.levels, "the round trip")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. the cut call
def _cut_check(ctx, W, records, K, keys, cuts, what, **placing):
    depth, length = len(records).bit_length() - 1, len(records[0])
    want_rows, want_p, want_s, want_index, want_roots, model = remove_cut_batch(records, K, keys, cuts)
    nk, G, c0 = len(keys), len(cuts), cuts[0]
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        ta, tb = Placed(ctx, records, **placing), Placed(ctx, records, **placing)
        a.set_records(0, ta.view)
        b.set_records(0, tb.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rows, nodes_p, nodes_s, index = a.remove_key_segments(ta.view, _keys(keys, K), cuts)
        counts = _drain(ctx)
        ctx.set_timing(False)
        assert counts == dict.fromkeys(KINDS, 0) | {"merkle_owners": 1, "merkle_remove_records": 1, "merkle_segments": 1, "merkle_updates": depth + 1, "merkle_record_rows": 2,
                                                    "sha256_records": 1}, what
        assert rows[0].shape == (nk, row_bytes(K, length, c0, zeros=128)) and all(r.shape[0] == 2 * nk for r in rows[1:]), what
        for g, (got, want) in enumerate(zip(rows, want_rows)):
            assert got.shape == want.shape and np.array_equal(got, want), (what, g)
        assert np.array_equal(index, want_index) and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s), what
        assert np.array_equal(nodes_p[:, G, 1], nodes_s[:, G, 0]), what  # the root between the two updates
        assert np.array_equal(nodes_p[:, -1, 0], want_roots[0:-1:2]) and np.array_equal(nodes_s[:, -1, 1], want_roots[2::2]), what
        ta.holds(model.records, what)
        _assert_tree(a, model.levels, what)
        # the uncut call on the second tree: the same index, table and tree; its rows sliced are every segment's
        urows, uindex, uroots = b.remove_keys(tb.view, _keys(keys, K), roots=True)
        assert np.array_equal(uindex, index) and np.array_equal(uroots, want_roots[0::2]), what
        assert np.array_equal(ta.whole.cpu().numpy(), tb.whole.cpu().numpy()), what
        _assert_tree(b, model.levels, what)
        head = 64 + K + 2 * length
        low = (1 << c0) - 1
        edges = [0] + list(cuts) + [depth]
        for j in range(nk):
            u = urows[j]
            sibs = (u[head: head + 32 * depth], u[head + 32 * depth: head + 64 * depth])
            bits = (int(index[j, 0]) & low) | (int(index[j, 1]) & low) << c0
            want0 = np.concatenate([np.zeros(128, dtype=np.uint8), u[64: head], sibs[0][: 32 * c0], sibs[1][: 32 * c0],
                                    np.frombuffer(bits.to_bytes((2 * c0 + 7) // 8, "little"), dtype=np.uint8)])
            assert np.array_equal(rows[0][j], want0), (what, j)
            for g in range(1, G + 1):
                lo, hi = edges[g], edges[g + 1]
                for side in (0, 1):
                    r = rows[g][2 * j + side]
                    assert np.array_equal(r[128: 128 + 32 * (hi - lo)], sibs[side][32 * lo: 32 * hi]), (what, j, g, side)
                    at = (int(index[j, side]) >> lo) & ((1 << (hi - lo)) - 1)
                    assert r[128 + 32 * (hi - lo):].tobytes() == at.to_bytes((hi - lo + 7) // 8, "little") and not r[64: 128].any(), (what, j, g, side)
    finally:
        ctx.set_timing(False)
        a.close()
        b.close()


@pytest.mark.parametrize("cuts", [[1], [2], [1, 2]])
def test_cut_removes_depth_3(ctx, W, cuts):
    depth, K, length = 3, 4, 11
    rng = np.random.default_rng(18300 + 10 * len(cuts) + cuts[0])
    members = _members(K, 7)
    records = _table(W, members, K, depth, length, rng)
    # member r - 1 is record r: (P, s) = (2, 3) and (4, 5), each in one height-1 subtree; then member 3, whose neighbours on both sides are gone: (2, 4), two
    # height-1 subtrees of one height-2 subtree; the smallest member last: (0, 1)
    keys = [members[2], members[4], members[3], members[0]]
    assert remove_cut_batch(records, K, keys, cuts)[3].tolist() == [[2, 3], [4, 5], [2, 4], [0, 1]]
    _cut_check(ctx, W, records, K, keys, cuts, ("depth 3", cuts), stride=length + 2, off=3)
    bits = None
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        bits = tree.remove_key_segment_bits(table.view, _keys([members[5]], K), cuts)[0]
    finally:
        tree.close()
    edges = [0] + cuts + [depth]
    assert [x.shape for x in bits] == [(1, 1024 + 8 * K + 16 * length + 514 * cuts[0])] + [(2, 1024 + 257 * (hi - lo)) for lo, hi in zip(edges[1:], edges[2:])]


def test_cut_removes_depth_9(ctx, W):
    depth, K, length, nk = 9, 8, 24, 40
    rng = np.random.default_rng(18400)
    members = sorted({rng.bytes(K) for _ in range(400)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    keys = members[100:108] + [members[int(i)] for i in rng.permutation(400) if not 100 <= int(i) < 108][: nk - 8]
    keys = [keys[int(i)] for i in rng.permutation(nk)]
    _cut_check(ctx, W, records, K, keys, [4], "depth 9 under [4]", stride=length + 1, off=2)


# ---------------------------------------------------------------------------------------------------------------- 10. end to end
def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 19, m=349525)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth = 4, 8, 1
    st = W.MerkleRemove(K, length, depth)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == st.lu == 544 and (cc.nwires, cc.nrows) == W.MERKLE_REMOVE_SIZES[(K, length, depth)]
    rng = np.random.default_rng(18500)
    members = [_key(x, K) for x in (0x6789ABCD, 0x01020304, 0xFEDCBA98)]  # a depth-1 table holds one member: three removes with an insert between them
    records = [r.tobytes() for r in W.indexed_records(_keys(members[:1], K), depth)]
    model = RemoveModel(records, K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        bits, pairs = [], []
        for j, member in enumerate(members):
            if j:
                tree.insert_keys(table.view, _keys([member], K))
                model.insert(member)
            b, index, roots = tree.remove_bits(table.view, _keys([member], K), roots=True)
            want_index, want_rows, want_roots = model.remove_batch([member])
            assert b.shape == (1, st.nin) and np.array_equal(np.packbits(b, axis=1, bitorder="little"), want_rows) and index.tolist() == want_index.tolist() == [[0, 1]]
            assert [r.tobytes() for r in roots] == want_roots and want_roots[0] != want_roots[1]
            bits.append(b[0])
            pairs.append(tuple(want_roots))
        table.holds(model.records, "end to end")
        assert len(set(pairs)) == 3 and len({r1 for _, r1 in pairs}) == 1  # three members out of one and the same empty set
        # a fourth row with s = p: slot 0 opened twice, the second time in the tree after its update
        old_p, old_s = records
        leaf_s = hashlib.sha256(old_s).digest()
        twice = st.bits(members[0], old_p, old_p[:K] + old_s[K:], [leaf_s], 0, [leaf_s], 0)
        assert model.levels[0][1] == hashlib.sha256(bytes(length)).digest()
        prog = ctx.circuit_load(cc, state="auto")
        try:
            witness, holds = ctx.circuit_assign(prog, np.stack(bits + [twice]))
        finally:
            prog.close()
        assert holds.tolist() == [True] * 3 + [False]
        for k in range(3):
            assert st.roots_of(witness[k]) == pairs[k], k
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count[:3].any() and (first[:3] == 0xFFFFFFFF).all() and count[3] > 0 and first[3] != 0xFFFFFFFF
        prove, verify = _prover(ctx, p, cc, rng, 3)
        proofs = prove(witness)
        own = [st.statement(*pairs[k], members[k]) for k in range(3)]
        assert all(len(x) == lu // 8 for x in own) and own == [witness[k][: lu // 8].tobytes() for k in range(3)]
        assert verify(proofs, own) == [True] * 3
        assert verify(proofs, [st.statement(*pairs[k], members[(k + 1) % 3]) for k in range(3)]) == [False] * 3  # another key
        assert verify(proofs, [st.statement(pairs[k][1], pairs[k][0], members[k]) for k in range(3)]) == [False] * 3  # the roots swapped
        assert verify(proofs, [st.statement(_flip(pairs[0][0], 77), pairs[0][1], members[0]), st.statement(pairs[1][0], _flip(pairs[1][1], 200), members[1]), own[2]]) == [False, False, True]
    finally:
        tree.close()
    print(f"test_end_to_end_proofs (MerkleRemove(4, 8, 1), d = 2^19): {time.time() - t0:.1f} s")


def test_end_to_end_cut_removal(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p19, p18 = mf.Params(d=1 << 19, m=349525), mf.Params(d=1 << 18, m=174762)
    ctx = gpu_ctx_factory(p19)
    ctx.set_seed(SEED)
    K, length, depth, cuts = 4, 8, 3, [1]
    st, seg = W.MerkleRemove(K, length, 1, joined=False), W.MerkleSegment(2)
    cc = st.circuit.compile(p19)
    assert cc.lu == st.lu == 1056 and (cc.nwires, cc.nrows) == W.MERKLE_REMOVE_SPLIT_SIZES[(K, length, 1)]
    rng = np.random.default_rng(18600)
    members = [_key(x, K) for x in (0x10, 0x6789ABCD, 0x7000_0000, 0x7100_0000)]
    records = [r.tobytes() for r in W.indexed_records(_keys(members, K), depth)]  # record r = member r - 1
    member = members[2]  # P = record 2, s = record 3: one height-1 subtree, so X_p' == X_s; the upper chains still differ
    want_rows, want_p, want_s, want_index, want_roots, model = remove_cut_batch(records, K, [member], cuts)
    assert want_index.tolist() == [[2, 3]]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        bits, nodes_p, nodes_s, index = tree.remove_key_segment_bits(table.view, _keys([member], K), cuts)
        table.holds(model.records, "end to end")
    finally:
        tree.close()
    assert index.tolist() == [[2, 3]] and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s)
    assert all(np.array_equal(np.packbits(b, axis=1, bitorder="little"), w) for b, w in zip(bits, want_rows))
    # the verifier's side: statements from the returned nodes alone
    pub_p = [(nodes_p[0, g, 0].tobytes(), nodes_p[0, g, 1].tobytes()) for g in range(2)]
    pub_s = [(nodes_s[0, g, 0].tobytes(), nodes_s[0, g, 1].tobytes()) for g in range(2)]
    r0, r_mid, r1 = (r.tobytes() for r in want_roots)
    assert pub_p[1] == (r0, r_mid) and pub_s[1] == (r_mid, r1) and len({r0, r_mid, r1}) == 3 and pub_p[0][1] == pub_s[0][0]
    own = st.statement(*pub_p[0], *pub_s[0], member)

    witness = _witnesses(ctx, cc, bits[0])
    assert st.tops_of(witness[0]) == pub_p[0] + pub_s[0] and own == witness[0][: st.lu // 8].tobytes()
    prove, verify = _prover(ctx, p19, cc, rng, 1)
    proofs = prove(witness)
    assert verify(proofs, [own]) == [True]
    assert verify(proofs, [st.statement(*pub_p[0], *pub_s[0], members[1])]) == [False]
    assert verify(proofs, [st.statement(pub_p[0][1], pub_p[0][0], *pub_s[0], member)]) == [False]
    assert verify(proofs, [st.statement(*pub_p[0], pub_s[0][1], pub_s[0][0], member)]) == [False]

    c18 = gpu_ctx_factory(p18)
    c18.set_seed(SEED)
    cs = seg.circuit.compile(p18)
    assert (cs.nwires, cs.nrows) == W.MERKLE_SEGMENT_SIZES[2]
    w_seg = _witnesses(c18, cs, bits[1])
    assert [seg.tops_of(w_seg[k]) for k in range(2)] == [pub_p[1], pub_s[1]]
    prove, verify = _prover(c18, p18, cs, rng, 2)
    proofs = prove(w_seg)
    own_seg = [W.MerkleSegment.chain(pub_p)[0], W.MerkleSegment.chain(pub_s)[0]]
    assert verify(proofs, own_seg) == [True, True]
    assert verify(proofs, own_seg[::-1]) == [False, False]
    broken = [W.MerkleSegment.statement(*pub_p[0], r0, r1), W.MerkleSegment.statement(*pub_s[0], r0, r1)]  # chains that skip R_mid
    assert verify(proofs, broken) == [False, False]
    print(f"test_end_to_end_cut_removal (MerkleRemove(4, 8, 1, joined=False) at d = 2^19, two MerkleSegment(2) at d = 2^18): {time.time() - t0:.1f} s")
