"""GPU: a batch of sequential key inserts into an indexed table on the device in ONE call (mfh_merkle_insert_keys, MerkleTree.insert_keys / insert_bits).

Every case compares h_index, h_status, the rows, the roots, the table's whole allocation (tests/test_gpu_merkle_record_update.py's Placed, with its 0xA5
surroundings) and the tree's nodes against
  the sequential route through the EXISTING calls on a second tree and table: per key locate_keys, words.indexed_insert into the lowest inert slot of a host
  copy of the table, update_records -- the insert's row put together out of the two MerkleRecordUpdate rows; and
  the brute-force model of tests/merkle_insert_model.py, its rows MerkleInsert.bits on a stand-in made without its circuit (test 1's first case checks that the
  stand-in and the real statement give the same bits).

1. hand-made sets at depth 2 and 3, key_bytes 1 and 4: one insert; two into two ranges; three into ONE range in ascending, descending and middle-first order
   (pred and succ); the empty set; a full table minus one slot.
2. key widths 1, 3, 4, 5, 8, 20, 32 at depth 3: keys that differ from a member in the first byte only and in the last byte only.
3. alignment at key_bytes 4 and 5: lengths 2K, 2K + 1, 2K + 15, 2K + 16, 55, 64, 65; the table 0 .. 3 bytes into its tensor; strides length and length + 5;
   random payloads, with keys whose record is an earlier key's (pred >= 0) and whose hi is an earlier key (succ >= 0).
4. the inert search: slots that are all zero, lo == hi != 0, lo > hi; inert slots at index 0, at the last index and on both sides of a wave's and a
   workgroup's boundary (depth 8 and 9), with exactly nk of them and with more; a shuffled table at depth 12 with 300 inserts.
5. refusals after the search (a member, a gap, one key more than inert slots): MFH_EINVAL, h_status filled, nothing written, no record or tree kernel; every
   up-front MFH_EINVAL case leaves the timing counts as they were; nk = 0 does nothing.
6. h_inputs = NULL; the launch counts of one chunk; a wider in_stride keeps its tail; scrubbed staging; a table produced late on the null stream and on a
   caller's.
7. two chunks: depth 6, key_bytes 4, length 2^19 (a row is 1 573 318 bytes, a chunk 42 inserts), 44 inserts; a split by MerkleRecordUpdate's rows would be
   63 updates, between the two updates of insert 31.
8. after a batch, absent_rows on the grown table answers as the model does.
9. end to end with MerkleInsert(4, 8, 1) at Params(d=1 << 19, m=349525)."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

from merkle_insert_model import InsertModel, row_bytes, stand_in
from test_gpu_merkle import _assert_tree, _flip
from test_gpu_merkle_absent import IndexedModel, _key, _keys, _table
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

SEED = bytes((43 * i + 5) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_locate", "merkle_inert", "merkle_insert_records", "sha256_records", "merkle_record_rows", "merkle_updates", "merkle_level", "merkle_paths",
         "merkle_absent_rows")


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
def _raw(ctx, tree, table, K, keys, pay, rows, roots, index, status, nk=None, in_stride=None, key_stride=None, pay_stride=None):
    vp = ctypes.c_void_p
    ptr = lambda a: vp(a.ctypes.data) if a is not None else None  # noqa: E731
    return ctx.lib.mfh_merkle_insert_keys(ctx._h, tree._h if tree is not None else None, vp(table.view.data_ptr()) if table is not None else None, table.stride if table else 0,
                                          table.length if table else 0, K, len(keys) if nk is None else nk, ptr(keys), keys.shape[1] if key_stride is None else key_stride,
                                          ptr(pay), (pay.shape[1] if pay is not None else 0) if pay_stride is None else pay_stride, ptr(rows),
                                          (rows.shape[1] if rows is not None else 0) if in_stride is None else in_stride, ptr(roots), ptr(index), ptr(status))


def _sequential(ctx, W, records, K, keys, payloads, **placing):
    """the existing route, one key at a time on a tree and table of its own: (index, status, rows, roots, the table's image, the tree's levels as bytes)"""
    records = list(records)
    length, depth = len(records[0]), len(records).bit_length() - 1
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        _, status = tree.locate_keys(table.view, _keys(keys, K)) if keys else (None, np.zeros(0, dtype=np.uint8))
        index, roots = [], [tree.root()]
        rows = np.zeros((len(keys), row_bytes(K, length, depth)), dtype=np.uint8)
        for j, key in enumerate(keys):
            at, st = tree.locate_keys(table.view, _keys([key], K))
            assert st[0] == 0
            p = int(at[0])
            free = next(i for i, r in enumerate(records) if not r[:K] < r[K: 2 * K])
            idx, new = W.indexed_insert(records[p], p, key, free, payload=payloads[j] if payloads is not None else b"")
            two, r = tree.update_records(table.view, idx, new, roots=True)
            for i, rec in zip(idx, new):
                records[i] = rec.tobytes()
            index.append(idx)
            roots.append(r[2].tobytes())
            head = 64 + 2 * length
            bits = sum(((p >> l) & 1) << l | ((free >> l) & 1) << (depth + l) for l in range(depth))
            rows[j] = np.concatenate([np.zeros(64, dtype=np.uint8), np.frombuffer(key, dtype=np.uint8), two[0, 64: 64 + length], two[1, 64: head],
                                      two[0, head: head + 32 * depth], two[1, head: head + 32 * depth],
                                      np.frombuffer(bits.to_bytes((2 * depth + 7) // 8, "little"), dtype=np.uint8)])
        levels = [tree.nodes(l).cpu().numpy().tobytes() for l in range(depth + 1)]
        return np.array(index, dtype=np.uint32).reshape(len(keys), 2), status, rows, roots, table.whole.cpu().numpy(), levels
    finally:
        tree.close()


def _pay_array(payloads, n, width):
    if payloads is None:
        return None
    return np.frombuffer(b"".join(payloads), dtype=np.uint8).reshape(n, width).copy()


def _insert(ctx, tree, table, K, keys, payloads):
    """one raw call: (rc, rows, roots, index, status)"""
    nk, depth = len(keys), tree.depth
    rows = np.zeros((nk, row_bytes(K, table.length, depth)), dtype=np.uint8)
    roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.full((nk, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(nk, 0xCD, dtype=np.uint8)
    rc = _raw(ctx, tree, table, K, _keys(keys, K), _pay_array(payloads, nk, table.length - 2 * K), rows, roots, index, status)
    return rc, rows, roots, index, status


def _check(ctx, W, records, K, keys, payloads, what, seq=None, model=None, **placing):
    """one batch on a fresh tree and table against the sequential route (seq: its results, when another placing has them already) and the model"""
    depth = len(records).bit_length() - 1
    if model is None:
        model = InsertModel(records, K)
        model.want = model.batch(keys, payloads)
    want_index, want_rows, want_roots = model.want
    own = seq is None  # (another placing's sequential result is compared in everything but the allocation's image)
    if own:
        seq = _sequential(ctx, W, records, K, keys, payloads, **placing)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        rc, rows, roots, index, status = _insert(ctx, tree, table, K, keys, payloads)
        assert rc == 0, (what, ctx.lib.mfh_last_error(ctx._h).decode())
        assert np.array_equal(index, want_index) and not status.any(), (what, index, want_index, status)
        assert [r.tobytes() for r in roots] == want_roots, what
        assert np.array_equal(rows, want_rows), what
        table.holds(model.records, what)
        _assert_tree(tree, model.levels, what)
        s_index, s_status, s_rows, s_roots, s_image, s_levels = seq
        assert np.array_equal(index, s_index) and np.array_equal(status, s_status) and np.array_equal(rows, s_rows), what
        assert [r.tobytes() for r in roots] == s_roots, what
        if own:
            assert np.array_equal(table.whole.cpu().numpy(), s_image), what
        assert [tree.nodes(l).cpu().numpy().tobytes() for l in range(depth + 1)] == s_levels, what
    finally:
        tree.close()
    return model, seq


def _members(K, depth, count=None):
    top = 0x10 << (8 * (K - 1))
    xs = (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))
    return [_key(x, K) for x in xs][: (1 << depth) - 1 if count is None else count]


# ---------------------------------------------------------------------------------------------------------------- 1. hand-made sets
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("depth", [2, 3])
def test_hand_made_sets(ctx, W, depth, K):
    rng = np.random.default_rng(14000 + 10 * depth + K)
    length = 2 * K + 3
    top = 0x10 << (8 * (K - 1))
    nmem = 1 if depth == 2 else 3  # depth 2: 2 live, 2 inert; depth 3: 4 live, 4 inert
    members = _members(K, depth, nmem)  # top (, top + 1, 3 top)
    records = _table(W, members, K, depth, length, rng)
    pay = lambda n: [rng.bytes(length - 2 * K) for _ in range(n)]  # noqa: E731
    if depth == 2 and K == 4:  # the stand-in gives what the statement gives
        args = InsertModel(records, K).insert(_key(top + 5, K), b"abc")[2]
        assert np.array_equal(stand_in(K, length, depth).bits(*args), W.MerkleInsert(K, length, depth).bits(*args))
    _check(ctx, W, records, K, [_key(top + 5, K)], pay(1), (depth, K, "one"), stride=length + 3, off=1)
    _check(ctx, W, records, K, [_key(top + 5, K)], None, (depth, K, "one, zero payload"), stride=length + 3, off=1)
    _check(ctx, W, records, K, [_key(top + 9, K), _key(5, K)], pay(2), (depth, K, "two ranges"), stride=length + 3, off=1)
    if depth == 3:
        a, b, c = (_key(4 * top + x, K) for x in (1, 2, 3))  # all inside (3 top, FF..)
        for order in ((a, b, c), (c, b, a), (b, a, c), (b, c, a)):
            model, _ = _check(ctx, W, records, K, list(order), pay(3), (K, "one range", order), stride=length + 3, off=1)
            want = model.want[0].tolist()  # record 3 = (3 top, FF..) holds all three at first; the inert slots are 4, 5, 6
            assert [s for _, s in want] == [4, 5, 6]
            assert [p for p, _ in want] == {(a, b, c): [3, 4, 5], (c, b, a): [3, 3, 3], (b, a, c): [3, 3, 4], (b, c, a): [3, 4, 3]}[order]
        # the empty set: every key falls into the sentinel record's range first
        empty = _table(W, [], K, depth, length, rng)
        _check(ctx, W, empty, K, [_key(x, K) for x in (top, 3, 2 * top, 0xFE << (8 * (K - 1)))], pay(4), (K, "the empty set"))
    # a full table minus one slot
    full = _table(W, _members(K, depth, (1 << depth) - 2), K, depth, length, rng)
    full = [full[i] for i in rng.permutation(1 << depth)]
    model, _ = _check(ctx, W, full, K, [_key(2 * top, K)], pay(1), (depth, K, "one free slot"), stride=length, off=3)
    assert all(model.live(i) for i in range(1 << depth))


# ---------------------------------------------------------------------------------------------------------------- 2. key widths
@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 20, 32])
def test_key_widths(ctx, W, K):
    depth = 3
    rng = np.random.default_rng(14100 + K)
    length = 2 * K + 1
    if K == 1:
        members, keys = [bytes([x]) for x in (0x10, 0x50, 0x60)], [bytes([x]) for x in (0x11, 0x4F, 0x51, 0xFE)]
    else:
        rest, mid = rng.bytes(K - 1), rng.bytes(K - 2)
        members = [bytes([0x10]) + rest, bytes([0x50]) + mid + bytes([0x10]), bytes([0x60]) + bytes(K - 2) + b"\xff"]
        # the first byte alone differs from a member; the last byte alone; ..01 00 against ..00 FF: ordered as integers, not byte by byte from the end
        keys = [bytes([0x20]) + rest, bytes([0x50]) + mid + bytes([0x20]), bytes([0x50]) + mid + bytes([0x0F])]
        keys += [bytes([0x60]) + bytes(K - 3) + b"\x01\x00"]
    records = _table(W, members, K, depth, length, rng)
    _check(ctx, W, records, K, keys, [rng.bytes(1) for _ in keys], K, stride=length + 2, off=3)


# ---------------------------------------------------------------------------------------------------------------- 3. alignment
@pytest.mark.parametrize("K", [4, 5])
def test_alignment_sweep(ctx, W, K):
    depth = 3
    for length in (2 * K, 2 * K + 1, 2 * K + 15, 2 * K + 16, 55, 64, 65):
        rng = np.random.default_rng(14200 + 100 * K + length)
        members = sorted({rng.bytes(K) for _ in range(3)})
        records = _table(W, members, K, depth, length, rng)
        records = [records[i] for i in rng.permutation(8)]
        lo = int.from_bytes(members[0], "big")
        gap = (int.from_bytes(members[1], "big") - lo) // 8
        keys = [_key(lo + x * gap, K) for x in (4, 2, 6)] + [rng.bytes(K)]  # one range: pred -1 / succ 0, then pred 0 / succ -1; a random one
        payloads = [rng.bytes(length - 2 * K) for _ in keys]
        model = seq = None
        for stride in (length, length + 5):
            for off in range(4):
                what = (K, length, stride, off)
                model, got = _check(ctx, W, records, K, keys, payloads, what, seq=seq, model=model, stride=stride, off=off)
                seq = got


# ---------------------------------------------------------------------------------------------------------------- 4. the inert search
def test_inert_kinds(ctx, W):
    depth, K, length = 3, 2, 7
    rng = np.random.default_rng(14300)
    rec = lambda lo, hi: _key(lo, K) + _key(hi, K) + rng.bytes(length - 2 * K)  # noqa: E731
    # inert: 0 (lo == hi != 0), 2 (all zero), 3 (lo > hi), 6 (lo == hi == FFFF)
    records = [rec(0x7777, 0x7777), rec(0, 0x1000), bytes(length), rec(0x9000, 0x8000), rec(0x1000, 0x5000), rec(0x5000, 0xFFFF), rec(0xFFFF, 0xFFFF), rec(0x9000, 0x8FFF)]
    keys = [_key(x, K) for x in (0x2000, 0x0800, 0x3000, 0x6000)]
    model, _ = _check(ctx, W, records, K, keys, [rng.bytes(3) for _ in keys], "inert kinds", stride=length + 1, off=1)
    assert model.want[0][:, 1].tolist() == [0, 2, 3, 6]


@pytest.mark.parametrize("depth", [8, 9])
def test_inert_slots_at_the_boundaries(ctx, W, depth):
    K, length = 8, 21
    n = 1 << depth
    rng = np.random.default_rng(14400 + depth)
    free = sorted({0, 63, 64, 127, 128, 255, n - 1} | ({256, 319, 320} if depth == 9 else set()))
    members = sorted({rng.bytes(K) for _ in range(n - 1 - len(free))})
    assert len(members) == n - 1 - len(free)
    packed = _table(W, members, K, depth, length, rng)
    live = [packed[int(i)] for i in rng.permutation(n - len(free))]
    records, it = [], iter(live)
    for i in range(n):
        records.append(bytes(length) if i in free else next(it))
    keys = [rng.bytes(K) for _ in free]
    payloads = [rng.bytes(length - 2 * K) for _ in free]
    model, _ = _check(ctx, W, records, K, keys, payloads, (depth, "exactly nk inert slots"), stride=length + 1, off=2)
    assert model.want[0][:, 1].tolist() == free and all(model.live(i) for i in range(n))
    model, _ = _check(ctx, W, records, K, keys[:3], payloads[:3], (depth, "more inert slots than keys"), stride=length + 1, off=2)
    assert model.want[0][:, 1].tolist() == free[:3]


def test_shuffled_table_depth_12(ctx, W):
    depth, K, length, nk = 12, 8, 24, 300
    rng = np.random.default_rng(14500)
    members = sorted({rng.bytes(K) for _ in range(3000)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    keys = [rng.bytes(K) for _ in range(nk - 40)]
    keys += [(int.from_bytes(members[7], "big") + 1 + int(x)).to_bytes(K, "big") for x in rng.permutation(40)]  # forty neighbours in one range, shuffled
    keys = [keys[int(i)] for i in rng.permutation(nk)]
    model, _ = _check(ctx, W, records, K, keys, [rng.bytes(length - 2 * K) for _ in keys], "depth 12", stride=length + 9, off=3)
    assert len(set(model.want[0][:, 1].tolist())) == nk and sum(model.live(i) for i in range(1 << depth)) == 1 + 3000 + nk


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def _drain(ctx):
    return {kind: ctx.timing_drain(kind)[0] for kind in KINDS}


def test_refusals_after_the_search(ctx, W):
    depth, K, length = 3, 2, 6
    rng = np.random.default_rng(14600)
    rec = lambda lo, hi: _key(lo, K) + _key(hi, K) + rng.bytes(length - 2 * K)  # noqa: E731
    # nothing covers [0x6000, 0x7000]; four inert slots: 0, 3, 6, 7
    records = [bytes(length), rec(0x1000, 0x2000), rec(0x2000, 0x6000), rec(0x9000, 0x8000), rec(0, 0x1000), rec(0x7000, 0xFFFF), rec(0x6000, 0x6000), bytes(length)]
    model = InsertModel(records, K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        cases = [("a member", [0x1800, 0x2000, 0x7800], [1, 2, 5], [0, 1, 0], 0),
                 ("a gap", [0x1800, 0x6800, 0x7800], [1, NONE, 5], [0, 2, 0], 0),
                 ("one key too many", [0x1800, 0x2800, 0x7800, 0x0800, 0x7900], [1, 2, 5, 4, 5], [0, 0, 0, 0, 0], 3)]
        texts = set()
        for what, xs, want_i, want_s, inert_launches in cases:
            rc, rows, roots, index, status = _insert(ctx, tree, table, K, [_key(x, K) for x in xs], None)
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_insert_keys: "), (what, rc, text)
            texts.add(text)
            assert status.tolist() == want_s and index[:, 0].tolist() == want_i, (what, status, index)
            assert not rows.any() and not roots.any(), what
            counts = _drain(ctx)
            assert counts == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_inert": inert_launches}, (what, counts)
            table.holds(records, what)
            _assert_tree(tree, model.levels, what)
        assert len(texts) == 3
        # the same table takes exactly its four inert slots' worth
        ctx.set_timing(False)
        rc, rows, roots, index, status = _insert(ctx, tree, table, K, [_key(x, K) for x in (0x1800, 0x2800, 0x7800, 0x0800)], None)
        assert rc == 0 and index[:, 1].tolist() == [0, 3, 6, 7]
    finally:
        ctx.set_timing(False)
        tree.close()


def test_einval_up_front(ctx, mf, W):
    import torch

    lib, h = ctx.lib, ctx._h
    depth, K, length = 3, 4, 17
    rng = np.random.default_rng(14700)
    members = sorted({rng.bytes(K) for _ in range(4)})
    records = _table(W, members, K, depth, length, rng)
    model = InsertModel(records, K)
    rowb = row_bytes(K, length, depth)
    tree = ctx.merkle_tree(depth)
    texts = []

    def refused(rc, handle=h):
        assert rc == EINVAL
        text = lib.mfh_last_error(handle).decode()
        assert text.startswith("mfh_merkle_insert_keys: "), text
        texts.append(text)

    try:
        table = Placed(ctx, records, stride=length + 3, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        vp = ctypes.c_void_p
        keys = _keys([rng.bytes(K) for _ in range(3)], K)
        zero, ones, twice = keys.copy(), keys.copy(), keys.copy()
        zero[1], ones[2], twice[2] = 0, 0xFF, twice[0]
        pay = np.zeros((3, length - 2 * K), dtype=np.uint8)
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((4, 32), 0xAB, dtype=np.uint8)
        index, status = np.full((3, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        kp, zp, op, wp, pp, bp, rp, ip, sp = (vp(a.ctypes.data) for a in (keys, zero, ones, twice, pay, buf, roots, index, status))
        tp, ts, stride, ps = vp(table.view.data_ptr()), table.stride, buf.shape[1], pay.shape[1]
        f = lib.mfh_merkle_insert_keys
        refused(f(h, None, tp, ts, length, K, 3, kp, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, 0, 3, kp, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, 66, 33, 3, kp, 33, pp, ps, bp, 1 << 12, rp, ip, sp))
        texts.pop()  # (key_bytes 0 and 33: one text)
        refused(f(h, tree._h, tp, ts, 2 * K - 1, K, 3, kp, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, (1 << 20) + 1, (1 << 20) + 1, K, 3, kp, K, None, 0, bp, 1 << 23, rp, ip, sp))
        refused(f(h, tree._h, tp, length - 1, length, K, 3, kp, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K - 1, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, pp, ps - 1, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, None, ts, length, K, 3, kp, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, None, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, pp, ps, bp, stride, rp, None, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, pp, ps, bp, stride, rp, ip, None))
        refused(f(h, tree._h, tp, ts, length, K, 3, kp, K, pp, ps, bp, rowb - 1, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 9, kp, K, pp, ps, bp, stride, rp, ip, sp))  # more keys than slots (read before any key is)
        refused(f(h, tree._h, tp, ts, length, K, 3, zp, K, pp, ps, bp, stride, rp, ip, sp))
        refused(f(h, tree._h, tp, ts, length, K, 3, op, K, pp, ps, bp, stride, rp, ip, sp))
        texts.pop()  # (the two sentinels: one text)
        refused(f(h, tree._h, tp, ts, length, K, 3, zp, K, None, 0, None, 0, None, ip, sp))  # no rows, no payloads: a sentinel is refused too
        texts.pop()
        refused(f(h, tree._h, tp, ts, length, K, 3, wp, K, pp, ps, bp, stride, rp, ip, sp))
        assert f(None, tree._h, tp, ts, length, K, 3, kp, K, pp, ps, bp, stride, rp, ip, sp) == EINVAL
        assert len(set(texts)) == len(texts) == 15, sorted(texts)
        if torch.cuda.device_count() > 1:
            other = mf.Context(mf.DEBUG, 1)
            try:
                assert f(other._h, tree._h, tp, ts, length, K, 3, kp, K, pp, ps, bp, stride, rp, ip, sp) == EINVAL
                assert lib.mfh_last_error(other._h).decode() == "mfh_merkle_insert_keys: the tree belongs to another device"
            finally:
                other.close()
                torch.cuda.set_device(ctx.device)
        # nk = 0 does nothing, whatever the pointers
        assert f(h, tree._h, None, ts, length, K, 0, None, K, None, 0, None, 0, None, None, None) == 0
        assert f(h, tree._h, tp, ts, length, K, 0, kp, K, pp, ps, bp, stride, rp, ip, sp) == 0
        none = np.zeros((0, K), dtype=np.uint8)
        rows0, index0, roots0 = tree.insert_keys(table.view, none, roots=True)
        assert rows0.shape == (0, rowb) and index0.shape == (0, 2) and index0.dtype == np.uint32 and roots0.tobytes() == model.root()
        assert tree.insert_bits(table.view, none)[0].shape == (0, 512 + 8 * K + 24 * length + 514 * depth)
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xAB).all() and (index == 0xCDCDCDCD).all() and (status == 0xCD).all()
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
        bad_pay = np.zeros((3, length - 2 * K + 1), dtype=np.uint8)
        for bad_table, bad_keys, bad_p in [(table.view, keys[0], None), (table.view, keys.astype(np.int8), None), (table.view, zero, None), (table.view, twice, None),
                                           (table.view, np.zeros((1, 9), dtype=np.uint8) + 1, None), (table.view[:4], keys, None), (table.view.cpu().numpy(), keys, None),
                                           (table.view, keys, bad_pay), (table.view, keys, pay.astype(np.int8)), (table.view, _keys([members[0]], K), None)]:
            for call in (tree.insert_keys, tree.insert_bits):
                with pytest.raises(mf.MfhError):
                    call(bad_table, bad_keys, bad_p)
        with pytest.raises(mf.MfhError) as e:
            tree.insert_keys(table.view, _keys([members[0]], K))
        assert "mfh_merkle_insert_keys: a key is already a member" in str(e.value)
        _assert_tree(tree, model.levels, "after the refused Python calls")
        table.holds(records, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. rows and streams
def test_no_rows_launch_counts_stride_and_scrub(ctx, W):
    depth, K, length, nk = 9, 8, 55, 100
    rng = np.random.default_rng(14800)
    members = sorted({rng.bytes(K) for _ in range(200)})
    records = _table(W, members, K, depth, length, rng)
    keys = [rng.bytes(K) for _ in range(nk)]
    payloads = [rng.bytes(length - 2 * K) for _ in keys]
    model = InsertModel(records, K)
    want_index, want_rows, want_roots = model.batch(keys, payloads)
    rowb = row_bytes(K, length, depth)
    assert rowb == 64 + 8 + 165 + 576 + 3
    karr, parr = _keys(keys, K), _pay_array(payloads, nk, length - 2 * K)
    tree = ctx.merkle_tree(depth)
    try:
        # no rows: the same table, tree and roots
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.zeros((nk, 2), dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, karr, parr, None, roots, index, status) == 0
        assert np.array_equal(index, want_index) and not status.any() and [r.tobytes() for r in roots] == want_roots
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: v[0] for k, v in timed.items()} == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_inert": 3, "merkle_insert_records": 1, "sha256_records": 1,
                                                                                  "merkle_record_rows": 1, "merkle_updates": depth + 1}
        table.holds(model.records, "no rows")
        _assert_tree(tree, model.levels, "no rows")
        # rows, a wider in_stride, no roots: one chunk's launches
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        _drain(ctx)
        buf = np.full((nk, rowb + 13), 0xAB, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, karr, parr, buf, None, index, status) == 0
        assert np.array_equal(buf[:, :rowb], want_rows) and (buf[:, rowb:] == 0xAB).all()
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | {
            "merkle_locate": (1, 1 << depth), "merkle_inert": (3, 1 << depth), "merkle_insert_records": (1, 2 * nk), "sha256_records": (1, 2 * nk),
            "merkle_record_rows": (2, 2 * nk), "merkle_updates": (depth + 1, 2 * nk * depth)}
        print(f"depth {depth}: {nk} inserts: " + ", ".join(f"{k} {v[1]:.3f} ms" for k, v in timed.items() if v[0]))
        ctx.set_timing(False)
        table.holds(model.records, "rows")
        # the pinned staging zeroed between two calls; the Python calls
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        assert ctx.scrub_staging() == 0
        rows2, index2, roots2 = tree.insert_keys(table.view, karr, parr, roots=True)
        assert np.array_equal(rows2, want_rows) and np.array_equal(index2, want_index) and [r.tobytes() for r in roots2] == want_roots
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        bits, index3 = tree.insert_bits(table.view, karr[:3], parr[:3])
        assert bits.shape == (3, 512 + 8 * K + 24 * length + 514 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows[:3])
        assert np.array_equal(index3, want_index[:3])
    finally:
        ctx.set_timing(False)
        tree.close()


def _late_table(ctx, W):
    depth, K, length, nk = 9, 4, 16, 64
    rng = np.random.default_rng(14900)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = _table(W, members, K, depth, length, rng)
    keys = [rng.bytes(K) for _ in range(nk)]
    payloads = [rng.bytes(length - 2 * K) for _ in keys]
    model = InsertModel(records, K)
    want_index, want_rows, want_roots = model.batch(keys, payloads)  # (first: nothing of the host's stands between the late table and the calls)
    karr, parr = _keys(keys, K), _pay_array(payloads, nk, length - 2 * K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        rows, index, roots = tree.insert_keys(table.view, karr, parr, roots=True)
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
    depth, K, length, nk = 6, 4, 1 << 19, 44
    rowb = row_bytes(K, length, depth)
    per_chunk = (64 << 20) // rowb
    update_rowb = 64 + 2 * length + 32 * depth + (depth + 7) // 8
    assert rowb == 1573318 and per_chunk == 42 < nk and (64 << 20) // update_rowb == 63  # an unpaired split: between updates 62 and 63, insert 31's two
    rng = np.random.default_rng(15000)
    members = sorted({rng.bytes(K) for _ in range((1 << depth) - 1 - nk)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    lo = int.from_bytes(members[3], "big")
    keys = [rng.bytes(K) for _ in range(nk)]
    keys[30], keys[31], keys[41], keys[42], keys[43] = (_key(lo + x, K) for x in (50, 40, 60, 45, 55))  # one range on both sides of both seams
    payloads = [rng.bytes(length - 2 * K) for _ in keys]
    model, _ = _check(ctx, W, records, K, keys, payloads, "two chunks", stride=length + 2, off=1)
    assert all(model.live(i) for i in range(1 << depth))


def test_two_chunks_launch_counts(ctx, W):
    depth, K, length, nk = 6, 4, 1 << 19, 44
    rng = np.random.default_rng(15001)
    records = _table(W, sorted({rng.bytes(K) for _ in range(5)}), K, depth, length, rng)
    keys = _keys([rng.bytes(K) for _ in range(nk)], K)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rows, index = tree.insert_keys(table.view, keys)
        assert index[:, 1].tolist() == list(range(6, 6 + nk))
        counts = {kind: ctx.timing_drain(kind)[::2] for kind in KINDS}
        assert counts == dict.fromkeys(KINDS, (0, 0)) | {"merkle_locate": (1, 1 << depth), "merkle_inert": (3, 1 << depth), "merkle_insert_records": (1, 2 * nk),
                                                         "sha256_records": (2, 2 * nk), "merkle_record_rows": (4, 2 * nk), "merkle_updates": (2 * (depth + 1), 2 * nk * depth)}
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. absence after a batch
def test_absent_rows_after_a_batch(ctx, W):
    depth, K, length, nk = 6, 5, 17, 12
    rng = np.random.default_rng(15100)
    members = sorted({rng.bytes(K) for _ in range(40)})
    records = _table(W, members, K, depth, length, rng)
    records = [records[int(i)] for i in rng.permutation(1 << depth)]
    keys = sorted(rng.bytes(K) for _ in range(nk))
    between = [((int.from_bytes(a, "big") + int.from_bytes(b, "big")) // 2).to_bytes(K, "big") for a, b in zip(keys, keys[1:])]
    shuffled = [keys[int(i)] for i in rng.permutation(nk)]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        queries = shuffled + [q for q in between if q not in members]
        before = IndexedModel(records, K)
        rows, index, status = tree.absent_rows(table.view, _keys(queries, K))
        assert not status.any() and np.array_equal(rows, before.answers(queries)[2])
        model = InsertModel(records, K)
        want = model.batch(shuffled, None)
        rows, index = tree.insert_keys(table.view, _keys(shuffled, K))
        assert np.array_equal(index, want[0]) and np.array_equal(rows, want[1])
        grown = IndexedModel(model.records, K)
        want_i, want_s, want_rows = grown.answers(queries)
        rows, index, status = tree.absent_rows(table.view, _keys(queries, K))
        assert np.array_equal(index, want_i) and np.array_equal(status, want_s) and np.array_equal(rows, want_rows)
        assert status[:nk].tolist() == [1] * nk and not status[nk:].any()
        table.holds(model.records, "grown")
        _assert_tree(tree, grown.levels, "grown")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. end to end
def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    t0 = time.time()
    p = mf.Params(d=1 << 19, m=349525)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth = 4, 8, 1
    st = W.MerkleInsert(K, length, depth)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == st.lu == 544 and (cc.nwires, cc.nrows) == W.MERKLE_INSERT_SIZES[(K, length, depth)]
    rng = np.random.default_rng(15200)
    member = _key(0x6789ABCD, K)
    records = [r.tobytes() for r in W.indexed_records(np.zeros((0, K), dtype=np.uint8), depth)]  # the empty set; a depth-1 table has one inert slot: ONE insert
    leaf1 = hashlib.sha256(records[1]).digest()
    model = InsertModel(records, K)
    tree = ctx.merkle_tree(depth)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        bits, index, roots = tree.insert_bits(table.view, _keys([member], K), roots=True)
        want_index, want_rows, want_roots = model.batch([member])
        assert bits.shape == (1, st.nin) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows) and index.tolist() == want_index.tolist() == [[0, 1]]
        r0, r1 = (r.tobytes() for r in roots)
        assert [r0, r1] == want_roots and r0 != r1
        # a fifth row whose old_s is the live record: s = p, opened in the tree after p's update
        new_p, new_s = model.records
        live = st.bits(member, records[0], new_p, new_s, [leaf1], 0, [leaf1], 0)  # (slot 1 is still inert when slot 0 is opened the second time)
        batch = np.concatenate([np.repeat(bits, 4, axis=0), live[None, :]])
        witness, holds = ctx.circuit_assign(prog, batch)
        assert holds.tolist() == [True] * 4 + [False]
        for k in range(4):
            assert st.roots_of(witness[k]) == (r0, r1), k
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count[:4].any() and (first[:4] == 0xFFFFFFFF).all()
        assert count[4] > 0 and first[4] != 0xFFFFFFFF

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

        own = st.statement(r0, r1, member)
        assert len(own) == lu // 8 and own == witness[0][: lu // 8].tobytes()
        assert verify([own] * 4) == [True] * 4
        assert verify([st.statement(r0, r1, _key(0x6789ABCE, K))] * 4) == [False] * 4  # another key
        assert verify([st.statement(r1, r0, member)] * 4) == [False] * 4  # swapped roots
        assert verify([st.statement(_flip(r0, 77), r1, member), st.statement(r0, _flip(r1, 200), member)] * 2) == [False] * 4
        # MerkleRecordUpdate-style statement bytes are too short: the statement refuses to make them, and padded with a zero key they verify nothing
        with pytest.raises(C.CircuitError):
            st.statement(r0, r1, b"")
        assert len(W.MerkleRecordUpdate.statement(r0, r1)) == 64 != lu // 8 and verify([W.MerkleRecordUpdate.statement(r0, r1)] * 4) == [False] * 4
        table.holds(model.records, "end to end")
    finally:
        prog.close()
        tree.close()
    print(f"test_end_to_end_proofs (MerkleInsert(4, 8, 1), d = 2^19): {time.time() - t0:.1f} s")
