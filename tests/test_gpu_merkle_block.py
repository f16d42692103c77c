"""GPU: MerkleTree.apply_block / apply_block_segments (mfh_merkle_block_keys, mfh_merkle_block_keys_cut) -- a block of transfers, adjusts and writes in any
order, applied in order in ONE device call -- against the existing per-kind calls run once per maximal run of one kind on a second copy of table and tree (the
reference: transfer_keys, adjust_keys, write_keys and their *_segments forms) and against tests/merkle_block_model.py.  Everything is compared: every step's
row, index, status, all roots, the table's whole allocation (the bytes between the records too: Placed) and every node of the tree.

 1. 24 interleaved steps of all three kinds over 5 live keys at depth 3: keys repeat, a write covers the balance before a transfer that needs it, a
    compare-and-set expects what an adjust of the block left.
 2. single-kind blocks equal transfer_keys / adjust_keys / write_keys (plain, conditional) byte for byte.
 3. the cut forms [1], [2], [1, 2] at depth 3, node pairs and first_update included.
 4. geometry: K = 1, 5, 7, 8, 32; length 23 at stride 29, 3 bytes into the tensor; A = 1, 5, 8; write fields of 1, 16 and 17 bytes that straddle a unit;
    a key whose window is two units beside keys whose window is one; a field that ends at `length`; K = 5 and 7 once more with records of 41 and 45
    bytes, where the 16- and 17-byte fields fit.
 5. nk = 1, 63, 64, 65, 255, 256, 257 at depth 10, a third of the steps transfers: nupd crosses workgroup boundaries off a step boundary.
 6. two chunks (records of 2^19 bytes, depth 2) with one transfer's two updates on both sides of the seam.
 7. the policies: a block with every status; fail-fast leaves everything as it was with no launch behind the search, skip equals the block without its
    failed steps.
 8. every refusal up front through the raw C calls, nothing queued.
 9. launch counts and work rows from the timing kinds; the per-kind calls' counts are what they were.
10. the null stream, a caller's stream, mfh_scrub_staging.
11. neighbours: total_balance, check_table, a block on a grown pair.
12. witnesses: one block of three steps, one of each kind, through circuit_assign of each step's own statement's program."""
import ctypes

import numpy as np
import pytest

from merkle_block_model import NONE, BlockModel, row_bytes
from merkle_transfer_model import ledger
from test_gpu_merkle import _assert_tree
from test_gpu_merkle_absent import _key, _keys
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

EINVAL = -1
NO_EXPECT = 0xFFFFFFFFFFFFFFFF
KINDS = ("merkle_locate", "merkle_block_windows", "merkle_block_records", "merkle_fields", "merkle_write_records", "merkle_balances", "merkle_adjust_records",
         "merkle_transfer_records", "merkle_balance_sum", "merkle_owners", "merkle_remove_records", "merkle_inert", "merkle_insert_records", "sha256_records",
         "merkle_record_rows", "merkle_updates", "merkle_level", "merkle_paths", "merkle_absent_rows", "merkle_segments")


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


def _drain(ctx):
    return {kind: ctx.timing_drain(kind)[0] for kind in KINDS}


def _nodes(ctx, tree):
    return [ctx.to_host(tree.nodes(l)).tobytes() for l in range(tree.depth + 1)]


def _block_of(W, K, A, steps):
    b = W.Block(K, A)
    b.steps = list(steps)
    return b


def _runs(W, block):
    """the maximal runs of steps one existing call can take: one kind and, for writes, one field and all with or all without an expectation"""
    runs = []
    for j, s in enumerate(block.steps):
        sig = (s[0],) if s[0] != W.Block.WRITE else (s[0], s[2], s[4] is not None)
        if runs and runs[-1][0] == sig:
            runs[-1][1].append(j)
        else:
            runs.append((sig, [j]))
    return runs


def _reference(ctx, W, tree, table, K, A, block, cuts=None):
    """the block through the EXISTING calls, one call a maximal run, on this tree and table: rows (per step), index [nk, 2], roots [nk + 1] and, cut, the
    upper segments' rows and the node pairs per update"""
    B = W.Block
    rows, index, roots = [None] * len(block), np.full((len(block), 2), NONE, dtype=np.uint32), [tree.root()]
    segments, nodes = None, []
    for sig, js in _runs(W, block):
        steps = [block.steps[j] for j in js]
        keys = _keys([s[1] for s in steps], K)
        if sig[0] == B.TRANSFER:
            args = (table.view, keys, _keys([s[2] for s in steps], K), [s[3] for s in steps])
            out = tree.transfer_key_segments(*args, cuts, amount_bytes=A) if cuts else tree.transfer_keys(*args, amount_bytes=A, roots=True)
        elif sig[0] == B.ADJUST:
            args = (table.view, keys, [s[2] for s in steps])
            out = tree.adjust_key_segments(*args, cuts, sides=[s[3] for s in steps], amount_bytes=A) if cuts else tree.adjust_keys(*args, [s[3] for s in steps], A, roots=True)
        else:
            args = (table.view, keys, [s[3] for s in steps], sig[1])
            expect = [s[4] for s in steps] if sig[2] else None
            out = tree.write_key_segments(*args, cuts, expect=expect) if cuts else tree.write_keys(*args, expect=expect, roots=True)
        if not cuts:
            r, idx, rts = out
            roots += [x.tobytes() for x in rts[1:]]
        elif sig[0] == B.TRANSFER:
            r_all, nodes_p, nodes_s, idx = out
            r, upper = r_all[0], r_all[1:]
            pairs = np.stack([nodes_p, nodes_s], axis=1).reshape(2 * len(js), *nodes_p.shape[1:])
            roots += [x[-1, 1].tobytes() for x in nodes_s]
        else:
            r_all, pairs, idx = out
            r, upper = r_all[0], r_all[1:]
            roots += [x[-1, 1].tobytes() for x in pairs]
        if cuts:
            segments = [[] for _ in upper] if segments is None else segments
            for g, u in enumerate(upper):
                segments[g] += list(u)
            nodes += list(pairs)
        for n, j in enumerate(js):
            rows[j] = r[n]
            index[j, : np.atleast_1d(idx[n]).size] = idx[n]
    out = {"rows": rows, "index": index, "roots": roots}
    if cuts:
        out.update(segments=[np.array(s, dtype=np.uint8) for s in segments], nodes=np.array(nodes, dtype=np.uint8))
    return out


def _same(res, want, what, cut=False):
    """a BlockResult against the model's dict (or the reference's, which has no status)"""
    assert res.index.dtype == np.uint32 and np.array_equal(res.index, want["index"]), (what, res.index, want["index"])
    if "status" in want:
        assert np.array_equal(res.status, want["status"]), (what, res.status, want["status"])
    assert [r.tobytes() for r in res.roots] == [bytes(r) for r in want["roots"]], what
    assert len(res.rows) == len(want["rows"])
    for j, (got, row) in enumerate(zip(res.rows, want["rows"])):
        assert (got is None) == (row is None) and (row is None or np.array_equal(got, row)), (what, j)
    if "first_update" in want:
        assert np.array_equal(res.first_update, want["first_update"]), what
        assert np.array_equal(res.update_roots, want["update_roots"]), what
    if cut:
        assert len(res.segments) == len(want["segments"]) and all(np.array_equal(a, b) for a, b in zip(res.segments, want["segments"])), what
        assert np.array_equal(res.nodes, want["nodes"]), what


def _check(ctx, W, records, K, A, block, what, cuts=None, skip_failed=False, reference=True, **placing):
    """one block on a fresh tree and table against the model and, on a second copy, against the existing calls; returns (the result, the model)"""
    depth = len(records).bit_length() - 1
    model = BlockModel(W, records, K, A)
    want = model.apply(block, skip_failed=skip_failed, cuts=cuts)
    tree, tree2 = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        res = tree.apply_block_segments(table.view, block, cuts, skip_failed=skip_failed) if cuts else tree.apply_block(table.view, block, skip_failed=skip_failed)
        _same(res, want, what, cut=bool(cuts))
        table.holds(model.records, what)
        _assert_tree(tree, model.levels, what)
        if reference:
            table2 = Placed(ctx, records, **placing)
            tree2.set_records(0, table2.view)
            applied = _block_of(W, K, A, [s for s, st in zip(block.steps, want["status"]) if not st])
            ref = _reference(ctx, W, tree2, table2, K, A, applied, cuts)
            ok = [j for j, st in enumerate(want["status"]) if not st]
            for n, j in enumerate(ok):
                assert np.array_equal(res.rows[j], ref["rows"][n]), (what, j)
                assert np.array_equal(res.index[j], ref["index"][n]), (what, j)
                assert res.roots[j].tobytes() == ref["roots"][n] and res.roots[j + 1].tobytes() == ref["roots"][n + 1], (what, j)
            if cuts:
                assert all(np.array_equal(a, b) for a, b in zip(res.segments, ref["segments"])) and np.array_equal(res.nodes, ref["nodes"]), what
            assert np.array_equal(table.whole.cpu().numpy(), table2.whole.cpu().numpy()), what
            assert _nodes(ctx, tree) == _nodes(ctx, tree2), what
    finally:
        tree.close()
        tree2.close()
    return res, model


def _five(W, rng, K=4, A=8, length=19, depth=3):
    top = 0x10 << (8 * (K - 1))
    keys = [_key(x, K) for x in (top, top + 1, 3 * top, 5 * top + 7, 9 * top)]
    records = ledger(W, {k: 1000 * (i + 1) for i, k in enumerate(keys)}, K, depth, length, A, rng)
    return keys, records


def _interleaved(W, keys, K=4, A=8, length=19):
    """24 steps, the kinds interleaved over 5 live keys: a write over the balance before a transfer that needs it, a compare-and-set on the balance that only
    an adjust of the block satisfies, memo and flag writes with fields of their own"""
    a, b, c, d, e = keys
    bal, memo, flag = (2 * K, 2 * K + A), (2 * K + A, length), (length - 1, length)
    blk = W.Block(K, A)
    blk.adjust(a, 500).transfer(a, b, 1500).write(c, memo, b"m-1").transfer(b, c, 3499).adjust(b, 1, 1).write(b, flag, b"\x01", expect=None)
    blk.write(d, bal, (77).to_bytes(A, "big")).transfer(d, e, 77).adjust(d, 9).write(d, bal, (10).to_bytes(A, "big"), expect=(9).to_bytes(A, "big"))
    blk.transfer(e, a, 5077).write(c, memo, b"m-2", expect=b"m-1").adjust(a, 5077, 1).transfer(c, d, 6499).write(a, (2 * K + 1, length - 1), bytes(range(A + 1)))
    blk.adjust(e, 1).transfer(d, e, 6509).write(e, flag, b"\xfe").write(e, flag, b"\xfd", expect=b"\xfe").adjust(c, 12345).transfer(c, b, 12345).adjust(b, 12345, 1)
    blk.write(b, memo, b"end").transfer(e, d, 6510)
    return blk


# ---------------------------------------------------------------------------------------------------------------- 1. against the existing calls
def test_interleaved_block_against_the_existing_calls(ctx, W):
    keys, records = _five(W, np.random.default_rng(52000))
    block = _interleaved(W, keys)
    assert len(block) == 24 and len(_runs(W, block)) == 24  # every run has length 1: the existing route is 24 calls
    res, model = _check(ctx, W, records, 4, 8, block, "interleaved", stride=20, off=1)
    assert not res.status.any() and int(res.first_update[-1]) == 24 + sum(s[0] == 0 for s in block.steps)
    assert res.rows_of(W.Block.TRANSFER)[0] == [j for j, s in enumerate(block.steps) if s[0] == 0]
    steps, rows = res.rows_of(W.Block.WRITE, (18, 19), expect=True)
    assert steps == [18] and rows.shape == (1, row_bytes(W, block.steps[18], 4, 8, 19, 3))


# ---------------------------------------------------------------------------------------------------------------- 2. single-kind blocks
@pytest.mark.parametrize("kind", ["transfers", "adjusts", "writes", "conditional"])
def test_single_kind_blocks(ctx, W, kind):
    K, A, length = 4, 8, 19
    rng = np.random.default_rng(52100)
    keys, records = _five(W, rng)
    blk = W.Block(K, A)
    shadow = BlockModel(W, records, K, A)  # (for the expectations each step meets)
    for j in range(12):
        x, y = keys[int(rng.integers(0, 5))], keys[int(rng.integers(0, 5))]
        if kind == "transfers":
            blk.transfer(x, y if y != x else keys[(keys.index(x) + 1) % 5], int(rng.integers(0, 50)))
        elif kind == "adjusts":
            blk.adjust(x, int(rng.integers(0, 100)), j % 2)
        else:
            value = rng.bytes(9)
            blk.write(x, (10, 19), value, expect=shadow.records[shadow.own(x)][10:19] if kind == "conditional" else None)
            shadow.records[shadow.own(x)] = shadow.records[shadow.own(x)][:10] + value
    assert len(_runs(W, blk)) == 1
    res, _ = _check(ctx, W, records, K, A, blk, kind, stride=21, off=2)
    assert not res.status.any()


# ---------------------------------------------------------------------------------------------------------------- 3. cut forms
@pytest.mark.parametrize("cuts", [[1], [2], [1, 2]])
def test_cut_forms(ctx, W, cuts):
    keys, records = _five(W, np.random.default_rng(52200))
    block = _interleaved(W, keys)
    res, _ = _check(ctx, W, records, 4, 8, block, cuts, cuts=cuts, stride=19, off=0)
    nupd = int(res.first_update[-1])
    assert nupd == 24 + sum(s[0] == 0 for s in block.steps) == 32 and res.nodes.shape == (nupd, len(cuts) + 1, 2, 32) and [s.shape[0] for s in res.segments] == [nupd] * len(cuts)
    assert np.array_equal(np.diff(res.first_update.astype(np.int64)), [2 if s[0] == 0 else 1 for s in block.steps])
    assert np.array_equal(res.nodes[:, -1, 0], res.update_roots[:-1]) and np.array_equal(res.nodes[:, -1, 1], res.update_roots[1:])


# ---------------------------------------------------------------------------------------------------------------- 4. geometry
@pytest.mark.parametrize("K,A,longer", [(1, 1, 0), (5, 5, 0), (7, 8, 0), (8, 8, 0), (32, 5, 0), (5, 5, 41), (7, 8, 45)])
def test_geometry_sweep(ctx, W, K, A, longer):
    depth = 3
    # (K = 8 with A = 8 and K = 32 do not fit 23 bytes; at K = 5 and 7 a record of 23 bytes has no room for the 16- and 17-byte fields: `longer` gives it)
    length = longer or (23 if 2 * K + A <= 23 else 2 * K + A + 35)
    rng = np.random.default_rng(52300 + K)
    top = 0x10 << (8 * (K - 1))
    keys = [_key(x, K) for x in (top, top + 1, 3 * top, 5 * top + 7)]
    cap = (1 << (8 * A)) - 1
    records = ledger(W, {k: min(cap // 2, 100 + i) for i, k in enumerate(keys)}, K, depth, length, A, rng)
    a, b, c, d = keys
    lo0 = 2 * K
    blk = W.Block(K, A)
    blk.adjust(a, 3).transfer(a, b, 2).adjust(c, 1, 1)  # a, b, c: one unit of window each (so far)
    for F in (1, 16, 17):
        if lo0 + F > length:
            continue
        # a field that straddles a 16-byte unit of the record where the length allows it, and one that ends at `length`
        lo = min(max(lo0, 16 - F // 2 if 16 - F // 2 >= lo0 else lo0 + 1), length - F)
        blk.write(d, (lo, lo + F), rng.bytes(F))
        blk.write(b, (length - F, length), rng.bytes(F), expect=None)
    blk.transfer(b, a, 1).adjust(a, 1, 1)
    if length - lo0 >= 17:  # d's window: two units and more, beside a and c whose window stays one
        blk.write(d, (lo0, lo0 + 17), bytes([0] * A) + rng.bytes(17 - A) if A < 17 else rng.bytes(17))
        blk.adjust(d, 1)
    if longer or K in (1, 8, 32):  # every field shape and the two-unit window took part
        assert sorted({s[2][1] - s[2][0] for s in blk.steps if s[0] == W.Block.WRITE}) == [1, 16, 17] and blk.steps[-1][0] == W.Block.ADJUST
    res, _ = _check(ctx, W, records, K, A, blk, (K, A, length), stride=length + 6, off=3)
    assert not res.status.any(), res.status


# ---------------------------------------------------------------------------------------------------------------- 5. sizes
@pytest.fixture(scope="module")
def depth_10(W):
    depth, K, A, length = 10, 8, 8, 55
    rng = np.random.default_rng(52400)
    members = sorted({rng.bytes(K) for _ in range(500)})
    return members, ledger(W, {k: 1 << 40 for k in members}, K, depth, length, A, rng, shuffle=True)


def _third_transfers(W, rng, members, nk, K=8, A=8):
    some = [members[int(i)] for i in rng.permutation(len(members))[:40]]
    blk = W.Block(K, A)
    for j in range(nk):
        x, y = (some[int(i)] for i in rng.permutation(40)[:2])
        if j % 3 == 1:
            blk.transfer(x, y, int(rng.integers(0, 1 << 30)))
        elif j % 3 == 0:
            blk.adjust(x, int(rng.integers(0, 1 << 30)), int(rng.integers(0, 2)))
        else:
            blk.write(x, (24, 32), rng.bytes(8))
    return blk


@pytest.mark.parametrize("nk", [1, 63, 64, 65, 255, 256, 257])
def test_block_sizes_depth_10(ctx, W, depth_10, nk):
    members, records = depth_10
    blk = _third_transfers(W, np.random.default_rng(52400 + nk), members, nk)
    res, _ = _check(ctx, W, records, 8, 8, blk, nk, reference=False, stride=56, off=2)
    assert not res.status.any() and int(res.first_update[-1]) == nk + nk // 3 + (nk % 3 == 2)


# ---------------------------------------------------------------------------------------------------------------- 6. two chunks, a transfer across the seam
def test_two_chunks_with_a_transfer_across_the_seam(ctx, W):
    depth, K, A, length = 2, 4, 8, 1 << 19
    field = (length - 8, length)
    rng = np.random.default_rng(52500)
    keys = [_key(x, K) for x in (0x10000000, 0x10000001, 0x30000000)]
    records = ledger(W, {k: 1 << 40 for k in keys}, K, depth, length, A, rng, shuffle=True)
    blk = W.Block(K, A)
    last = {}
    for j in range(126):  # 126 one-update steps: updates 0 .. 125
        k = keys[j % 3]
        if j % 2:
            blk.adjust(k, j, j % 4 == 1)
        else:
            v = rng.bytes(8)
            blk.write(k, field, v, expect=last.get(k))
            last[k] = v
    blk.transfer(keys[0], keys[2], 12345)  # updates 126 and 127
    blk.write(keys[2], field, rng.bytes(8), expect=last[keys[2]])  # update 128
    per_chunk = (64 << 20) // max((row_bytes(W, s, K, A, length, depth) + (s[0] == 0)) // (2 if s[0] == 0 else 1) for s in blk.steps)
    assert per_chunk == 127 and len(blk) == 128
    model = BlockModel(W, records, K, A)
    want = model.apply(blk)
    assert list(want["first_update"][126:]) == [126, 128, 129] and not want["status"].any()
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        res = tree.apply_block(table.view, blk)
        counts = {kind: ctx.timing_drain(kind)[::2] for kind in KINDS}
        ctx.set_timing(False)
        nupd = 129
        assert counts == dict.fromkeys(KINDS, (0, 0)) | {"merkle_locate": (1, 1 << depth), "merkle_block_windows": (1, 3), "merkle_block_records": (1, nupd),
                                                         "sha256_records": (2, nupd), "merkle_record_rows": (4, nupd), "merkle_updates": (2 * (depth + 1), nupd * depth)}
        _same(res, want, "two chunks")
        table.holds(model.records, "two chunks")
        _assert_tree(tree, model.levels, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. policies
def _every_status(W, keys, ghost, K=4, A=8, length=19):
    a, b, c, d, e = keys  # balances 1000 .. 5000
    memo = (2 * K + A, length)
    blk = W.Block(K, A)
    blk.adjust(a, 10).transfer(ghost, a, 1).transfer(a, ghost, 1).transfer(a, b, 1011).transfer(a, b, 1010).adjust(a, 1, 1).adjust(a, 5)
    blk.adjust(c, (1 << 64) - 3000).write(c, memo, b"one").write(c, memo, b"two", expect=b"xxx").write(c, memo, b"two", expect=b"one").write(ghost, memo, b"abc")
    blk.adjust(ghost, 1).transfer(d, e, 4000).adjust(b, 1).adjust(e, 2, 1).write(d, memo, b"zzz")
    return blk, [0, 1, 2, 3, 0, 3, 0, 4, 0, 5, 0, 1, 1, 0, 0, 0, 0]


def test_policies(ctx, W, mf):
    K, A, length, depth = 4, 8, 19, 3
    keys, records = _five(W, np.random.default_rng(52600))
    ghost = _key(0x60000000, K)
    records[6] = ghost + ghost + records[6][2 * K:]  # the lo of an inert record alone: no member
    blk, statuses = _every_status(W, keys, ghost)
    model = BlockModel(W, records, K, A)
    want = model.apply(blk, skip_failed=True)
    # both conditions on the model, before the GPU runs: every status occurs, and at least half the steps apply
    assert list(want["status"]) == statuses and set(statuses) == {0, 1, 2, 3, 4, 5} and 2 * statuses.count(0) >= len(statuses)
    before = BlockModel(W, records, K, A)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        with pytest.raises(mf.MfhError) as e:  # fail-fast
            tree.apply_block(table.view, blk)
        assert "mfh_merkle_block_keys: " in str(e.value) and "h_status 1" in str(e.value)  # the first failed step's
        assert list(e.value.status) == statuses and np.array_equal(e.value.index, want["index"])
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_block_windows": 1}  # no launch behind the search
        table.holds(records, "fail-fast")
        _assert_tree(tree, before.levels, "fail-fast")
        assert tree.root() == before.root()
        with pytest.raises(mf.MfhError) as e:
            tree.apply_block_segments(table.view, blk, [1])
        assert "mfh_merkle_block_keys_cut: " in str(e.value)
        table.holds(records, "fail-fast, cut")
        _drain(ctx)
        res = tree.apply_block(table.view, blk, skip_failed=True)  # skip
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_block_windows": 1, "merkle_block_records": 1, "sha256_records": 1, "merkle_record_rows": 2,
                                                         "merkle_updates": depth + 1}
        ctx.set_timing(False)
        _same(res, want, "skip")
        for j, st in enumerate(statuses):
            assert (res.rows[j] is None) == bool(st) and (not st or res.roots[j].tobytes() == res.roots[j + 1].tobytes())
        table.holds(model.records, "skip")
        _assert_tree(tree, model.levels, "skip")
        # a step behind a skipped overdraft sees the balance without it: 1010 was still there for the second transfer, and the deposit of 5 lands on 0
        assert model.balance(model.own(keys[0])) == 5
        # the raw call leaves the row slot of a skipped step as it was
        table3 = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table3.view)
        raw = _raw_args(ctx, tree, table3, blk)
        assert _raw_call(ctx, tree, raw, skip=1) == 0 and list(raw["status"]) == statuses and np.array_equal(raw["first_update"], want["first_update"])
        for j, st in enumerate(statuses):
            slot = raw["rows"][int(raw["row_at"][j]): int(raw["row_at"][j + 1])]
            assert (slot == 0xAB).all() if st else np.array_equal(slot, want["rows"][j]), j
        table3.holds(model.records, "skip, raw")
    finally:
        ctx.set_timing(False)
        tree.close()
    # the block without its failed steps, fail-fast, on a fresh pair: the same rows, roots, table and tree
    clean = _block_of(W, K, A, [s for s, st in zip(blk.steps, statuses) if not st])
    res2, model2 = _check(ctx, W, records, K, A, clean, "the block without its failed steps", stride=length + 1, off=1)
    assert model2.records == model.records and np.array_equal(res2.update_roots, res.update_roots)
    assert all(np.array_equal(x, y) for x, y in zip(res2.rows, [r for r in res.rows if r is not None]))
    res3, _ = _check(ctx, W, records, K, A, blk, "skip, against the existing calls", skip_failed=True, stride=length + 1, off=1)
    assert np.array_equal(res3.status, statuses)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def _raw_args(ctx, tree, table, block, cut=None):
    """the arguments of the raw call as a dict of named values, arrays kept alive in it"""
    B, K, A, nk = type(block), block.key_bytes, block.amount_bytes, len(block)
    d0 = cut[0] if cut else tree.depth
    a = {"table": table.view.data_ptr(), "stride": table.stride, "length": table.length, "K": K, "A": A, "nk": nk}
    a["kinds"] = np.array([s[0] for s in block.steps], dtype=np.uint8)
    a["keys"] = _keys([s[1] for s in block.steps], K)
    a["keys_to"] = _keys([s[2] if s[0] == B.TRANSFER else s[1] for s in block.steps], K)
    a["key_stride"] = K
    a["amounts"] = np.array([s[3] if s[0] == B.TRANSFER else s[2] if s[0] == B.ADJUST else 0 for s in block.steps], dtype=np.uint64)
    a["sides"] = np.array([s[3] if s[0] == B.ADJUST else 0 for s in block.steps], dtype=np.uint8)
    a["fields"] = np.array([s[2] if s[0] == B.WRITE else (0, 0) for s in block.steps], dtype=np.uint32).reshape(nk, 2)
    values, expect, value_at, expect_at = b"", b"", [], []
    for s in block.steps:
        value_at.append(len(values))
        expect_at.append(NO_EXPECT)
        if s[0] == B.WRITE:
            values += s[3]
            if s[4] is not None:
                expect_at[-1] = len(expect)
                expect += s[4]
    a["value_at"], a["expect_at"] = np.array(value_at, dtype=np.uint64), np.array(expect_at, dtype=np.uint64)
    a["values"], a["expect"] = np.frombuffer(values + b"\0", dtype=np.uint8).copy(), np.frombuffer(expect + b"\0", dtype=np.uint8).copy()
    a["values_bytes"], a["expect_bytes"], a["skip"] = len(values), len(expect), 0
    rowb = [int(ctx.lib.mfh_merkle_block_row_bytes(int(s[0]), K, A, table.length, d0, int(f[0]), int(f[1]), int(s[0] == B.WRITE and s[4] is not None), int(bool(cut))))
            for s, f in zip(block.steps, a["fields"])]
    a["row_at"] = np.concatenate([[0], np.cumsum(rowb)]).astype(np.uint64)
    a["rows"] = np.full(int(a["row_at"][-1]) + 8, 0xAB, dtype=np.uint8)
    a["roots"], a["index"] = np.zeros((2 * nk + 1, 32), dtype=np.uint8), np.full((nk, 2), 0xCDCDCDCD, dtype=np.uint32)
    a["status"], a["first_update"] = np.full(nk, 0xCD, dtype=np.uint8), np.full(nk + 1, 0xCDCDCDCD, dtype=np.uint32)
    if cut:
        nmax = sum(2 if s[0] == B.TRANSFER else 1 for s in block.steps)
        edges = list(cut) + [tree.depth]
        a["upper"] = [np.zeros((nmax, 128 + 32 * (hi - lo) + (hi - lo + 7) // 8), dtype=np.uint8) for lo, hi in zip(edges, edges[1:])]
        a["cuts"] = np.array(cut, dtype=np.uint32)
        a["ncuts"] = len(cut)
    return a


def _raw_call(ctx, tree, a, **over):
    a = {**a, **over}
    vp = ctypes.c_void_p
    ptr = lambda x: None if x is None else vp(x.ctypes.data)  # noqa: E731
    front = (ctx._h, tree._h, vp(a["table"]) if a["table"] else None, a["stride"], a["length"], a["K"], a["A"], a["nk"], ptr(a["kinds"]), ptr(a["keys"]), ptr(a["keys_to"]),
             a["key_stride"], ptr(a["amounts"]), ptr(a["sides"]), ptr(a["fields"]), ptr(a["value_at"]), ptr(a["values"]), a["values_bytes"], ptr(a["expect_at"]),
             ptr(a["expect"]), a["expect_bytes"], a["skip"])
    back = (ptr(a["row_at"]), ptr(a["roots"]), ptr(a["index"]), ptr(a["status"]), ptr(a["first_update"]))
    if "cuts" not in a:
        return ctx.lib.mfh_merkle_block_keys(*front, ptr(a["rows"]), *back)
    arrays = [a["rows"]] + list(a["upper"])
    ptrs = (vp * len(arrays))(*[None if x is None else x.ctypes.data for x in arrays])
    strides = (ctypes.c_size_t * len(arrays))(*([0] + [x.shape[1] for x in a["upper"]])) if a.get("strides") is None else a["strides"]
    return ctx.lib.mfh_merkle_block_keys_cut(*front, a["ncuts"], ptr(a["cuts"]), ptrs if a.get("h_rows", True) else None, strides, *back)


def test_einval_up_front(ctx, W):
    K, A, length, depth = 4, 8, 19, 3
    keys, records = _five(W, np.random.default_rng(52700))
    a_key, b_key, c_key = keys[:3]
    blk = W.Block(K, A).transfer(a_key, b_key, 5).adjust(c_key, 7, 1).write(a_key, (16, 19), b"abc").write(b_key, (9, 12), b"xyz", expect=b"\0\0\0")
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        base = _raw_args(ctx, tree, table, blk)
        cut = _raw_args(ctx, tree, table, blk, cut=[1])
        ctx.set_timing(True)
        _drain(ctx)

        def arr(name, j, value, args=base):
            x = args[name].copy()
            x.reshape(-1)[j] = value
            return {name: x}

        def key_at(name, j, key):
            x = base[name].copy()
            x[j] = np.frombuffer(key, dtype=np.uint8)
            return {name: x}

        short = base["row_at"].copy()
        short[2:] -= 1  # row 1's slot one byte short
        short_cut = cut["row_at"].copy()
        short_cut[2:] -= 1
        cases = [
            ({"K": 0}, "key_bytes must be in [1, 32]"), ({"K": 33}, "key_bytes must be in [1, 32]"), ({"length": 7}, "length shorter than the two keys"),
            ({"length": (1 << 20) + 1, "stride": 1 << 21}, "length above 2^20 bytes"), ({"stride": length - 1}, "table_stride shorter than length"),
            ({"key_stride": K - 1}, "key_stride shorter than key_bytes"), ({"A": 0}, "amount_bytes must be in [1, 8]"), ({"A": 9}, "amount_bytes must be in [1, 8]"),
            ({"length": 2 * K + A - 1}, "length shorter than the two keys and the balance"), ({"table": 0}, "steps without d_table"), ({"keys": None}, "steps without h_keys"),
            ({"index": None}, "steps without h_index"), ({"status": None}, "steps without h_status"), (key_at("keys", 1, bytes(K)), "the all-zero or the all-0xFF key"),
            (key_at("keys", 0, b"\xff" * K), "the all-zero or the all-0xFF key"), ({"kinds": None}, "steps without h_kinds"), ({"first_update": None}, "steps without h_first_update"),
            ({"row_at": None}, "rows without h_row_at"), (arr("kinds", 1, 3), "a kind is none of"), ({"keys_to": None}, "transfers without h_keys_to"),
            (key_at("keys_to", 0, b"\xff" * K), "the all-zero or the all-0xFF key"), (key_at("keys_to", 0, a_key), "a transfer from an account to itself"),
            ({"amounts": None}, "without h_amounts"), ({**arr("amounts", 0, 1 << 16), "A": 2}, "an amount does not fit amount_bytes bytes"),
            ({**arr("amounts", 1, 1 << 24), "A": 3}, "an amount does not fit amount_bytes bytes"), (arr("sides", 1, 2), "a side is neither 0"),
            ({"fields": None}, "writes without h_fields"), ({"value_at": None}, "writes without h_value_at"), ({"values": None}, "writes without h_values"),
            (arr("fields", 4, 2 * K - 1), "the keys are not writable"), (arr("fields", 5, 16), "a field's hi must be above its lo"), (arr("fields", 5, length + 1), "a field's hi above length"),
            (arr("value_at", 3, 4), "a value's bytes lie outside h_values"), ({"values_bytes": 5}, "a value's bytes lie outside h_values"),
            (arr("expect_at", 3, 1), "an expectation's bytes lie outside h_expect"), ({"expect": None}, "an expectation's bytes lie outside h_expect"),
            ({"row_at": short}, "a row's slot in h_rows is shorter than the step's row"),
        ]
        for over, word in cases:
            rc = _raw_call(ctx, tree, base, **over)
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_block_keys: ") and word in text, (over.keys(), rc, text)
        cut_cases = [({"ncuts": 0}, "no cuts"), ({"cuts": None}, "no cuts"), ({"cuts": np.array([3], dtype=np.uint32)}, "the cuts are not"), ({"cuts": np.array([0], dtype=np.uint32)}, "the cuts are not"),
                     ({"h_rows": False}, "h_rows or h_strides is null"), ({"rows": None}, "a segment without its rows"), ({"upper": [None]}, "a segment without its rows"),
                     ({"strides": (ctypes.c_size_t * 2)(0, 100)}, "a segment's stride shorter than its row's bytes"), (arr("kinds", 0, 9, cut), "a kind is none of"),
                     ({"row_at": short_cut}, "a row's slot in h_rows is shorter than the step's row")]
        for over, word in cut_cases:
            if over.get("upper") == [None]:
                over = {**over, "strides": (ctypes.c_size_t * 2)(0, 200)}
            rc = _raw_call(ctx, tree, cut, **over)
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_block_keys_cut: ") and word in text, (over.keys(), rc, text)
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)  # nothing was queued
        table.holds(records, "refusals")
        assert (base["rows"] == 0xAB).all() and (base["status"] == 0xCD).all()
        assert ctx.lib.mfh_merkle_block_row_bytes(3, K, A, length, depth, 0, 0, 0, 0) == 0
        # nk = 0 does nothing; the same arguments are fine
        assert _raw_call(ctx, tree, base, nk=0) == 0 and _drain(ctx) == dict.fromkeys(KINDS, 0)
        assert _raw_call(ctx, tree, base) == 0 and (base["status"] == 0).all() and (base["rows"][-8:] == 0xAB).all() and list(base["first_update"]) == [0, 2, 3, 4, 5]
    finally:
        ctx.set_timing(False)
        tree.close()


def test_wrapper_argument_errors(ctx, W, mf):
    K, A, length, depth = 4, 8, 19, 3
    keys, records = _five(W, np.random.default_rng(52800))
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        blk = W.Block(K, A).adjust(keys[0], 1)
        for call, word in [(lambda: tree.apply_block(table.view.cpu().numpy(), blk), "apply_block: the table"), (lambda: tree.apply_block(table.view, [(1, keys[0], 1, 0)]), "a words.Block"),
                           (lambda: tree.apply_block(table.view, W.Block(K, A).write(keys[0], (8, 20), bytes(12))), "a write's field"),
                           (lambda: tree.apply_block(table.view[:, :15], W.Block(K, A)), "2 key_bytes + amount_bytes <= length"),
                           (lambda: tree.apply_block_segments(table.view, blk, [3]), "apply_block_segments: cuts"), (lambda: tree.apply_block_segments(table.view, blk, []), "cuts")]:
            with pytest.raises(mf.MfhError) as e:
                call()
            assert word in str(e.value), (word, str(e.value))
        table.holds(records, "argument errors")
        res = tree.apply_block(table.view, W.Block(K, A))  # an empty block
        assert res.rows == [] and res.roots.shape == (1, 32) and res.roots[0].tobytes() == tree.root() and res.rows_of(W.Block.ADJUST) [0] == []
        with pytest.raises(mf.MfhError):
            res.rows_of(W.Block.WRITE)
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. launch counts
def test_launch_counts_and_work_rows(ctx, W, depth_10):
    depth, K, A, length, nk = 10, 8, 8, 55, 100
    members, records = depth_10
    blk = _third_transfers(W, np.random.default_rng(52900), members, nk)
    nu = len({k for s in blk.steps for k in ((s[1], s[2]) if s[0] == 0 else (s[1],))})
    nupd = nk + sum(s[0] == 0 for s in blk.steps)
    model = BlockModel(W, records, K, A)
    want = model.apply(blk)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        res = tree.apply_block(table.view, blk)
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        # one search, one gather, one build launch; per chunk as adjust_keys on nupd updates
        want_counts = {"merkle_locate": (1, 1 << depth), "merkle_block_windows": (1, nu), "merkle_block_records": (1, nupd), "sha256_records": (1, nupd), "merkle_record_rows": (2, nupd),
                       "merkle_updates": (depth + 1, nupd * depth)}
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | want_counts
        print(f"depth {depth}: a block of {nk} steps, {nupd} updates: " + ", ".join(f"{k} {v[1]:.3f} ms" for k, v in timed.items() if v[0]))
        _same(res, want, "counts")
        # the cut call: one more launch a chunk
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        _drain(ctx)
        tree.apply_block_segments(table.view, blk, [4, 7])
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | want_counts | {"merkle_segments": (1, 2 * nupd)}
        # the per-kind calls queue what they always have
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        _drain(ctx)
        k8 = _keys(members[:7], K)
        tree.adjust_keys(table.view, k8, [1] * 7)
        assert {k: v for k, v in _drain(ctx).items() if v} == {"merkle_locate": 1, "merkle_balances": 1, "merkle_adjust_records": 1, "sha256_records": 1, "merkle_record_rows": 2,
                                                               "merkle_updates": depth + 1}
        tree.transfer_keys(table.view, k8[:3], k8[3:6], [1, 2, 3])
        assert {k: v for k, v in _drain(ctx).items() if v} == {"merkle_locate": 1, "merkle_balances": 1, "merkle_transfer_records": 1, "sha256_records": 1, "merkle_record_rows": 2,
                                                               "merkle_updates": depth + 1}
        tree.write_keys(table.view, k8, [bytes(8)] * 7, (24, 32))
        assert {k: v for k, v in _drain(ctx).items() if v} == {"merkle_locate": 1, "merkle_write_records": 1, "sha256_records": 1, "merkle_record_rows": 2, "merkle_updates": depth + 1}
        tree.write_keys(table.view, k8[:1], [bytes(8)], (24, 32), expect=[bytes(8)])
        assert {k: v for k, v in _drain(ctx).items() if v} == {"merkle_locate": 1, "merkle_fields": 1, "merkle_write_records": 1, "sha256_records": 1, "merkle_record_rows": 2,
                                                               "merkle_updates": depth + 1}
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 10. streams, staging
def _late_block(ctx, W):
    from test_gpu_merkle_record_update import Placed as P

    depth, K, A, length = 9, 4, 8, 24
    rng = np.random.default_rng(53000)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = ledger(W, {k: 1 << 40 for k in members}, K, depth, length, A, rng, shuffle=True)
    blk = W.Block(K, A)
    for j in range(64):
        x, y = (members[int(i)] for i in rng.permutation(20)[:2])
        (blk.transfer(x, y, j) if j % 3 == 0 else blk.adjust(x, j, j % 2) if j % 3 == 1 else blk.write(x, (17, 24), rng.bytes(7)))
    model = BlockModel(W, records, K, A)
    want = model.apply(blk)  # (first: nothing of the host's stands between the late table and the calls)
    tree = ctx.merkle_tree(depth)
    try:
        table = P(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        res = tree.apply_block(table.view, blk)
        _same(res, want, "late table")
        table.holds(model.records, "late table")
        _assert_tree(tree, model.levels, "late table")
    finally:
        tree.close()


def test_ordering_null_stream(ctx, W):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_block(ctx, W)


def test_ordering_callers_stream(gpu_ctx_factory, mf, W):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_block(c, W)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()


def test_the_same_after_scrub_staging(ctx, W):
    keys, records = _five(W, np.random.default_rng(53100))
    blk = _interleaved(W, keys)
    model = BlockModel(W, records, 4, 8)
    want = model.apply(blk)
    tree = ctx.merkle_tree(3)
    try:
        for scrub in (False, True):  # the pinned staging zeroed between two identical calls: the same rows from the same starting table
            table = Placed(ctx, records, stride=20)
            tree.set_records(0, table.view)
            if scrub:
                assert ctx.scrub_staging() == 0
            _same(tree.apply_block(table.view, blk), want, scrub)
            table.holds(model.records, scrub)
        assert ctx.scrub_staging() == 0
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 11. neighbours
def test_neighbours(ctx, W):
    depth, K, A, length = 6, 8, 8, 55
    rng = np.random.default_rng(53200)
    members = sorted({rng.bytes(K) for _ in range(40)})
    records = ledger(W, {k: 1 << 40 for k in members}, K, depth, length, A, rng, shuffle=True)
    blk = _third_transfers(W, rng, members, 60)
    blk.adjust(members[0], 1 << 41, 1)  # an overdraft: skipped
    model = BlockModel(W, records, K, A)
    want = model.apply(blk, skip_failed=True)
    moved = sum((-s[2] if s[3] else s[2]) for s, st in zip(blk.steps, want["status"]) if s[0] == 1 and not st)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        supply, live = tree.total_balance(table.view, K, A)
        assert live == 41 and tree.check_table(table.view, K) == (0, 41, None)  # (the 40 accounts and the sentinel record)
        res = tree.apply_block(table.view, blk, skip_failed=True)
        _same(res, want, "neighbours")
        assert list(res.status[-1:]) == [3] and not res.status[:-1].any()
        assert tree.total_balance(table.view, K, A) == (supply + moved, 41) == model.supply()  # (the writes of this block lie behind the balance)
        assert tree.check_table(table.view, K) == (0, 41, None)
        grown, wide = tree.grow(depth + 2, table.view)  # a block on a pair that grow made
        try:
            big = BlockModel(W, [bytes(r) for r in W.indexed_grow(np.stack([np.frombuffer(r, dtype=np.uint8) for r in model.records]), depth + 2)], K, A)
            more = _third_transfers(W, rng, members, 20)
            g_want = big.apply(more)
            _same(grown.apply_block(wide, more), g_want, "grown")
            assert [bytes(r) for r in wide.cpu().numpy()] == big.records
            _assert_tree(grown, big.levels, "grown")
            assert grown.check_table(wide, K) == (0, 41, None)
        finally:
            grown.close()
        table.holds(model.records, "the old pair is only read")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 12. witnesses
def test_witnesses_of_one_step_of_each_kind(gpu_ctx_factory, mf, W):
    p = mf.Params(d=1 << 19, m=349525)
    ctx = gpu_ctx_factory(p)
    K, A, length, depth = 4, 8, 16, 1
    a_key, b_key = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585")
    # a depth-1 table has no room for the sentinel record beside two accounts: the two records close the ring by hand
    records = [a_key + b_key + (1000).to_bytes(8, "big"), b_key + b"\xff" * K + (5).to_bytes(8, "big")]
    blk = W.Block(K, A).adjust(a_key, 24).transfer(a_key, b_key, 1024).write(b_key, (8, 16), (3).to_bytes(8, "big"), expect=(1029).to_bytes(8, "big"))
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        res = tree.apply_block(table.view, blk)
        model = BlockModel(W, records, K, A)
        _same(res, model.apply(blk), "witnesses")
        stmts = blk.statements(length, depth, res.roots, res.status)
        for j, (kind, field, expect) in enumerate([(W.Block.ADJUST, None, False), (W.Block.TRANSFER, None, False), (W.Block.WRITE, (8, 16), True)]):
            key, statement = stmts[j]
            st = getattr(W, key[0])(*key[1:])
            cc = st.circuit.compile(p)
            steps, bits = res.bits_of(kind, field, expect)
            assert steps == [j] and bits.shape == (1, st.nin)
            flipped = bits.copy()
            # one value bit: the top bit of the side byte (asserted 0), bit 7 of the amount (1152 overdraws 1024), the first bit of the expectation
            flipped[0, 512 + 8 * K if kind == W.Block.WRITE else cc.lu - 1] ^= 1
            prog = ctx.circuit_load(cc, state="auto")
            try:
                witness, holds = ctx.circuit_assign(prog, np.concatenate([bits, flipped]))
            finally:
                prog.close()
            assert witness[0][: cc.lu // 8].tobytes() == statement and len(statement) == cc.lu // 8, key
            assert st.roots_of(witness[0]) == (res.roots[j].tobytes(), res.roots[j + 1].tobytes())
            assert holds.tolist() == [True, False], key  # with one value bit flipped the step no longer holds
    finally:
        tree.close()
