"""GPU: growing a tree and its indexed table in place of a rebuild (mfh_merkle_grow, mfh_merkle_grow_leaves; k_grow_nodes, k_grow_spine, k_grow_table;
MerkleTree.grow) against words.indexed_grow, words.grown_root, hashlib and a tree computed here over the WHOLE grown table (test_gpu_merkle_load's
vectorised levels over tests/sha256_ref.py's constants) -- every level of the new tree, not the root alone.

1. depth 1 -> 2, 3 -> 4, 3 -> 7, 9 -> 10: K in 1, 5, 8, 32, length 2K and 2K + 7, a table after load_keys; old and new tables misaligned and strided, the new
   one prefilled with random bytes: the new table, its gaps and surroundings, every level, the returned roots, the old pair unchanged.
2. depth 12 -> 13 and 12 -> 15: k_grow_nodes and k_grow_table span many workgroups and every level crosses a copy / constant boundary inside one.
   In 1. and 2. every shape also runs with BOTH tables packed (stride = length, still misaligned), where k_grow_table takes the whole table as one row.
3. leaf mode 3 -> 6, and a record tree grown without tables.
4. life after growth, 4 -> 5: a full table refuses a batch of inserts, the grown one takes it; check_table, absent_rows, range_segments on the grown pair.
5. every MFH_EINVAL: nothing written, nothing launched, *out untouched -- the 2^32-unit bound of a strided table at depth 24 among them, with pointers that
   only place the tables; "a tree of another device" needs a second GPU and is not reached here.
6. queue-only: a table produced late on the stream, on the null stream and on a caller's; roots=False, more work queued behind it, one sync at the end.
7. launch counts by timing kind."""
import ctypes

import numpy as np
import pytest

import sha256_ref
from test_gpu_merkle import _assert_tree
from test_gpu_merkle_load import _garbage_table, _keys, _levels, _parents
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

EINVAL = -1
KINDS = ("merkle_grow", "sha256_records", "merkle_level")


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


def _as_words(node):
    """a node's 32 bytes as a row holds a sibling: eight native words holding the big-endian words' values"""
    return np.frombuffer(node, dtype=">u4").astype("<u4").tobytes()


def _rows(table):
    return [r.tobytes() for r in table]


def _loaded(ctx, W, rng, depth, K, length, n, stride=None, off=0, late=False, keys=None):
    """(tree, placed table, host table, levels): an indexed table of n members in a tree of `depth`, made by load_keys"""
    keys = _keys(rng, K, n) if keys is None else keys
    pay = [rng.bytes(length - 2 * K) for _ in range(n)]
    host = W.indexed_records(keys, depth, length, pay)
    tree = ctx.merkle_tree(depth)
    if late:
        placed = Placed(ctx, _rows(host), stride=stride, off=off, late=True)
        tree.set_records(0, placed.view)  # no wait before it
    else:
        placed, _ = _garbage_table(ctx, rng, depth, length, stride=stride, off=off)
        assert tree.load_keys(placed.view, keys, pay if length > 2 * K else None) == (0, None)
    return tree, placed, host, _levels(host)


def _grow_and_compare(ctx, W, rng, tree, placed, host, levels, D, what, stride=None, off=0):
    """tree.grow into a prefilled, misplaced new table: the table and its surroundings, every level, the roots, the old pair"""
    d, length = tree.depth, host.shape[1]
    new, _ = _garbage_table(ctx, rng, D, length, stride=stride, off=off)
    grown, view, (r0, r1) = tree.grow(D, placed.view, out=new.view, roots=True)
    try:
        assert grown.depth == D and view.data_ptr() == new.view.data_ptr() and tuple(view.shape) == (1 << D, length), what
        want = W.indexed_grow(host, D)
        new.holds(_rows(want), what)  # byte for byte, the gaps of a wider stride and the bytes around the table included
        want_levels = _levels(want)
        _assert_tree(grown, want_levels, what)
        assert (r0, r1) == (levels[-1][0], W.grown_root(levels[-1][0], d, D, length)) and r1 == want_levels[-1][0], what
        placed.holds(_rows(host), what)  # the old pair: only read
        _assert_tree(tree, levels, what)
    except BaseException:
        grown.close()
        raise
    return grown, new, want, want_levels


# ---------------------------------------------------------------------------------------------------------------- 1. small depths
@pytest.mark.parametrize("d,D", [(1, 2), (3, 4), (3, 7), (9, 10)])
def test_small_depths(ctx, W, d, D):
    rng = np.random.default_rng(32000 + 100 * d + D)
    for i, K in enumerate((1, 5, 8, 32)):
        for j, length in enumerate((2 * K, 2 * K + 7)):
            n = min((1 << d) - 1, 200 if K == 1 else 300)
            for packed in (False, True):  # (both tables packed: k_grow_table takes the whole table as one row)
                tree, placed, host, levels = _loaded(ctx, W, rng, d, K, length, n, stride=None if packed else length + 1 + j, off=1 + i % 3)
                try:
                    assert placed.view.data_ptr() % 4 == (1 + i % 3) % 4
                    grown, new, _, _ = _grow_and_compare(ctx, W, rng, tree, placed, host, levels, D, (d, D, K, length, packed),
                                                         stride=None if packed else length + 3 - j, off=(i + j + 2) % 4)
                    assert new.view.data_ptr() % 4 == (i + j + 2) % 4
                    assert grown.check_table(new.view, K) == (0, n + 1, None)
                    grown.close()
                finally:
                    tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. many workgroups
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("D", [13, 15])
def test_many_workgroups(ctx, W, D, packed):
    rng = np.random.default_rng(32500 + D)
    d, K, length = 12, 8, 23
    tree, placed, host, levels = _loaded(ctx, W, rng, d, K, length, 3000, stride=None if packed else length + 2, off=3)
    try:
        grown, new, _, _ = _grow_and_compare(ctx, W, rng, tree, placed, host, levels, D, (d, D, packed), stride=length, off=1)
        assert grown.check_table(new.view, K) == (0, 3001, None)
        # a contiguous table the call allocates itself, no roots
        again, view = tree.grow(D, placed.view)
        assert view.is_contiguous() and tuple(view.shape) == (1 << D, length)
        assert np.array_equal(view.cpu().numpy(), W.indexed_grow(host, D))
        assert again.root() == grown.root()
        again.close()
        grown.close()
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. leaves, and a tree alone
def _leaf_levels(leaves):
    cur = np.frombuffer(b"".join(leaves), dtype=np.uint8).reshape(-1, 32)
    levels = [cur]
    while len(cur) > 1:
        cur = _parents(cur)
        levels.append(cur)
    return [[bytes(x) for x in level] for level in levels]


def test_leaves_and_tree_alone(ctx, W):
    rng = np.random.default_rng(33000)
    tree = ctx.merkle_tree(3)
    try:
        assert tree.root() == W.inert_roots(3)[-1]  # a fresh tree of leaves
        leaves = [rng.bytes(32) for _ in range(8)]
        tree.set_leaves(0, b"".join(leaves))
        grown, (r0, r1) = tree.grow(6, roots=True)
        want = _leaf_levels(leaves + [bytes(32)] * 56)
        _assert_tree(grown, want, "leaves")
        _assert_tree(tree, _leaf_levels(leaves), "leaves: the old tree")
        assert (r0, r1) == (_leaf_levels(leaves)[-1][0], W.grown_root(r0, 3, 6)) and r1 == want[-1][0]
        fresh = ctx.merkle_tree(6)
        assert fresh.root() == W.inert_roots(6)[-1] != r1
        fresh.close()
        twice = grown.grow(8)  # no roots, no table: the tree itself
        _assert_tree(twice, _leaf_levels(leaves + [bytes(32)] * 248), "leaves, grown twice")
        assert twice.root() == W.grown_root(r0, 3, 8)
        twice.close()
        grown.close()
    finally:
        tree.close()
    K, length, d, D = 5, 17, 3, 5
    tree, placed, host, levels = _loaded(ctx, W, rng, d, K, length, 6)
    try:
        grown = tree.grow(D, length=length)
        assert isinstance(grown, type(tree))
        _assert_tree(grown, _levels(W.indexed_grow(host, D)), "a record tree alone")
        assert sha256_ref.merkle_parent(grown.nodes(D - 1).cpu().numpy()[0].tobytes(), W.inert_roots(D - 1, length)[-1]) == grown.root()
        placed.holds(_rows(host), "a record tree alone")
        grown.close()
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. life after growth
def _host_insert(W, table, K, key):
    """words.indexed_insert of one key on a host table: the record whose range holds it, the lowest inert slot"""
    lo = [r[:K].tobytes() for r in table]
    hi = [r[K: 2 * K].tobytes() for r in table]
    p = next(s for s in range(len(table)) if lo[s] < key < hi[s])
    free = next(s for s in range(len(table)) if lo[s] >= hi[s])
    idx, new = W.indexed_insert(table[p].tobytes(), p, key, free)
    table[idx] = new


def test_life_after_growth(ctx, mf, W):
    rng = np.random.default_rng(34000)
    K, length, d, D = 4, 13, 4, 5
    keys = _keys(rng, K, 19)
    members, more = keys[:15], keys[15:]
    tree, placed, host, levels = _loaded(ctx, W, rng, d, K, length, 15, stride=length + 1, off=1, keys=members)
    try:
        with pytest.raises(mf.MfhError, match="mfh_merkle_insert_keys: the table has fewer inert slots than keys to insert"):
            tree.insert_keys(placed.view, more)
        placed.holds(_rows(host), "a refused batch")
        probe = np.stack([more[0], members[3]])
        rows0, index0, status0 = tree.absent_rows(placed.view, probe)
        grown, new, want, _ = _grow_and_compare(ctx, W, rng, tree, placed, host, levels, D, "life", stride=length + 2, off=2)
        try:
            rows1, index1, status1 = grown.absent_rows(new.view, probe)
            assert np.array_equal(index0, index1) and np.array_equal(status0, status1) and list(status0) == [0, 1]
            head = 32 + K + length + 32 * d  # the key, the record and the siblings inside the old tree; above them the constants E_d .. E_D-1
            assert np.array_equal(rows0[:, :head], rows1[:, :head])
            assert [rows1[k, head: head + 32].tobytes() for k in range(2)] == [_as_words(W.inert_roots(d, length)[d])] * 2
            grown.insert_keys(new.view, more)
            for key in more:
                _host_insert(W, want, K, key.tobytes())
            new.holds(_rows(want), "the batch, after the growth")
            _assert_tree(grown, _levels(want), "the batch, after the growth")
            assert grown.check_table(new.view, K) == (0, 20, None) == W.indexed_check(want, K)
            lo, hi = min(m.tobytes() for m in keys), max(m.tobytes() for m in keys)
            rows, nodes, index, rkeys, status = grown.range_segments(new.view, lo, hi, [4])
            assert status == 0 and [int(s) for s in index] == W.indexed_range(want, K, lo, hi) and len(index) == 20
            assert all(nodes[i][-1].tobytes() == grown.root() for i in range(len(index)))
        finally:
            grown.close()
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. MFH_EINVAL
def test_einval(ctx, mf, W):
    rng = np.random.default_rng(35000)
    K, length, d, D = 4, 11, 3, 5
    tree, placed, host, levels = _loaded(ctx, W, rng, d, K, length, 5, stride=13, off=1)
    new, new_records = _garbage_table(ctx, rng, D, length, stride=14, off=2)
    lib, h = ctx.lib, ctx._h
    vp = ctypes.c_void_p
    try:
        tp, np_ = placed.view.data_ptr(), new.view.data_ptr()
        out, roots = vp(0x77), (ctypes.c_uint8 * 64)(*([7] * 64))
        ctx.sync()
        ctx.set_timing(True)
        texts = []

        def refused(rc, who):
            assert rc == EINVAL
            text = lib.mfh_last_error(h).decode()
            assert text.startswith(who + ": "), text
            texts.append(text)
            assert out.value == 0x77 and list(roots) == [7] * 64

        grow = lambda **kw: lib.mfh_merkle_grow(h, kw.get("t", tree._h), kw.get("D", D), vp(kw.get("table", tp)), kw.get("stride", 13), kw.get("length", length),
                                                vp(kw.get("new", np_)), kw.get("nstride", 14), kw.get("out", ctypes.byref(out)), kw.get("roots", roots))
        span = 7 * 13 + length  # the old table's
        for kw in (dict(t=None), dict(out=None), dict(D=d), dict(D=d - 1), dict(D=0), dict(D=25), dict(length=(1 << 20) + 1, stride=1 << 21, nstride=1 << 21),
                   dict(stride=10), dict(nstride=10), dict(table=None), dict(new=None), dict(new=tp), dict(new=tp + span - 1), dict(new=tp - (31 * 14 + length) + 1),
                   dict(new=tp - 100), dict(table=None, new=None, length=(1 << 20) + 1), dict(table=None, new=None, D=3),
                   # 2^24 records of ceil((4078 + 3) / 16) = 256 units are 2^32 items of k_grow_table (strided tables: a row is a record)
                   dict(D=24, length=4078, stride=4079, nstride=4079, new=tp + (1 << 20)), dict(D=24, length=1 << 20, stride=1 << 20, nstride=(1 << 20) + 1, new=tp + (1 << 24))):
            refused(grow(**kw), "mfh_merkle_grow")
        for kw in (dict(t=None), dict(out=None), dict(D=d), dict(D=25)):
            refused(lib.mfh_merkle_grow_leaves(h, kw.get("t", tree._h), kw.get("D", D), kw.get("out", ctypes.byref(out)), roots), "mfh_merkle_grow_leaves")
        assert len(set(texts)) >= 10 and any("2^32 units" in t for t in texts)
        assert {kind: ctx.timing_drain(kind)[0] for kind in KINDS} == dict.fromkeys(KINDS, 0)
        placed.holds(_rows(host), "refusals")
        new.holds(new_records, "refusals")
        _assert_tree(tree, levels, "refusals")
        # the legal neighbours: a new table that ends where the old one begins, and one that begins where it ends
        new_span = 31 * 14 + length
        whole = ctx.zeros(new_span + span + new_span)  # (an old table of zero records in the middle: the placement alone is looked at)
        base = whole.data_ptr() + new_span
        for at in (base - new_span, base + span):
            assert lib.mfh_merkle_grow(h, tree._h, D, vp(base), 13, length, vp(at), 14, ctypes.byref(out), None) == 0
            assert out.value != 0x77
            lib.mfh_merkle_destroy(out)
            out = vp(0x77)
        ctx.sync()
        assert ctx.timing_drain("merkle_grow")[0] == 6
        # the Python method: the parser's refusals
        for bad in (dict(new_depth=d), dict(new_depth=25), dict(new_depth=2.5), dict(new_depth=D, out=new.view), dict(new_depth=D, length=-1),
                    dict(new_depth=D, table=placed.view, length=length + 1), dict(new_depth=D, table=placed.view, out=new.view[:16]),
                    dict(new_depth=D, table=placed.view, out=new.view[:, :5]), dict(new_depth=D, table=placed.view[:4]), dict(new_depth=D, table=host)):
            with pytest.raises(mf.MfhError):
                tree.grow(**bad)
        assert ctx.timing_drain("merkle_grow")[0] == 0
    finally:
        for kind in KINDS:
            ctx.timing_drain(kind)
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. queue-only
def _late_growth(ctx, W):
    rng = np.random.default_rng(36000)
    K, length, d, D = 8, 20, 9, 11
    keys = _keys(rng, K, 300)
    host = W.indexed_records(keys, d, length, [rng.bytes(4) for _ in range(300)])
    want = W.indexed_grow(host, D)  # (first: nothing of the host's stands between the late table and the calls)
    levels, want_levels = _levels(host), _levels(want)
    tree = ctx.merkle_tree(d)
    try:
        new = Placed(ctx, [bytes(length)] * (1 << D), stride=length + 3, off=3)
        placed = Placed(ctx, _rows(host), stride=length + 1, off=1, late=True)
        tree.set_records(0, placed.view)  # no wait before it, nor before the next
        grown, view = tree.grow(D, placed.view, out=new.view)  # queue-only: no roots
        top = grown.nodes(D).clone()  # more work behind it on the same stream, still no wait
        tall = grown.grow(D + 1, length=length)
        ctx.sync()  # the one wait
        assert top.cpu().numpy().tobytes() == want_levels[-1][0]
        new.holds(_rows(want), "late table")
        _assert_tree(grown, want_levels, "late table")
        assert tall.root() == W.grown_root(levels[-1][0], d, D + 1, length)
        _assert_tree(tree, levels, "late table: the old tree")
        placed.holds(_rows(host), "late table: the old table")
        assert ctx.scrub_staging() == 0
        again, view, (r0, r1) = tree.grow(D, placed.view, roots=True)
        assert (r0, r1) == (levels[-1][0], want_levels[-1][0]) and np.array_equal(view.cpu().numpy(), want)
        for t in (again, tall, grown):
            t.close()
    finally:
        tree.close()


def test_ordering_null_stream(ctx, W):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_growth(ctx, W)


def test_ordering_callers_stream(gpu_ctx_factory, mf, W):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_growth(c, W)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 7. launch counts
def test_launch_counts(ctx, W):
    rng = np.random.default_rng(37000)
    K, length, d, D = 8, 16, 6, 9
    tree, placed, host, levels = _loaded(ctx, W, rng, d, K, length, 40)
    counts = lambda: {kind: ctx.timing_drain(kind) for kind in KINDS}
    made = []
    try:
        ctx.sync()
        ctx.set_timing(True)
        counts()
        made.append(tree.grow(D, placed.view, roots=True)[0])
        got = counts()
        assert (got["merkle_grow"][0], got["merkle_grow"][2]) == (3, (2 << D) + (D - d) + (1 << D))
        assert got["sha256_records"][0] == 0 and got["merkle_level"][0] == 0
        print(f"depth {d} -> {D}, {1 << D} records of {length} bytes: {got['merkle_grow'][1]:.3f} ms in 3 launches")
        made.append(tree.grow(D, length=length))
        made.append(tree.grow(D + 1))
        ctx.sync()
        got = counts()
        assert (got["merkle_grow"][0], got["merkle_grow"][2]) == (4, (2 << D) + (D - d) + (4 << D) + (D + 1 - d))
        assert got["sha256_records"][0] == 0 and got["merkle_level"][0] == 0
        assert made[0].root() == made[1].root() == W.grown_root(levels[-1][0], d, D, length)
    finally:
        ctx.set_timing(False)
        for t in made:
            t.close()
        tree.close()
