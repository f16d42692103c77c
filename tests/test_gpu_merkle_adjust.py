"""GPU: a batch of sequential deposits and withdrawals on the accounts of an indexed table in ONE call (mfh_merkle_adjust_keys, MerkleTree.adjust_keys /
adjust_bits), with the path cut (mfh_merkle_adjust_keys_cut, MerkleTree.adjust_key_segments), and the table's supply (mfh_merkle_balance_sum,
MerkleTree.total_balance).

Every case compares h_index, h_status, the rows, the roots, the table's whole allocation (tests/test_gpu_merkle_record_update.py's Placed, with its 0xA5
surroundings) and the tree's nodes byte for byte against the brute-force model of tests/merkle_adjust_model.py, whose rows are put together byte by byte; test 1
also against the per-step route through the EXISTING calls (locate_keys, words.indexed_adjust, update_records).

1. a depth-3 table, every account, both sides, uncut and under [1], [2], [1, 2]; a key five times with a withdrawal that only the batch's earlier deposit
   covers; nk = 0; h_inputs = NULL through the C call; sides = NULL.
2. alignment: key widths 1, 5, 7, 8 and 32 with amount_bytes 1, 3 and 8 ((7, 8): the balance at bytes [14, 22) straddles a 16-byte unit), lengths 16, 55 and
   56 where the record has room (else 2K + A and 2K + A + 7), the table 1 .. 3 bytes into its tensor at strides length and length + 5.
3. 1, 63, 64, 65, 255, 256 and 257 steps at depth 10.
4. two chunks: length 2^19 (a chunk is 127 steps), 128 steps at depth 2, an account on both sides of the seam.
5. a missing key, an overdraft and an overflow at a later step, each alone: status 1 / 3 / 4 at that step, the library's text, table and root unchanged,
   no record or tree kernel.
6. every up-front refusal; the launch counts of a call by timing kind.
7. late tables on the null stream and on a caller's; the same rows after mfh_scrub_staging.
8. total_balance at depths 1, 6, 8, 9 and 12, garbage in inert slots, amount_bytes 1 .. 8, 1 024 live records at 2^64 - 1, strided misaligned tables at key
   widths 1, 5, 8 and 32; unchanged by transfer_keys, changed by the deposits less the withdrawals by adjust_keys.
9. end to end: three steps on a depth-2 table proved as MerkleAdjust(4, 16, 2, 8) and, under [1], as MerkleAdjust(4, 16, 1, 8) plus MerkleSegment(1) rows
   verified from the published nodes alone; every proof rejected under a flipped amount bit, a flipped side, another key and the two roots swapped."""
import ctypes
import time

import numpy as np
import pytest

from merkle_adjust_model import AdjustModel, adjust_cut_batch, ledger, row_bytes, supply
from test_gpu_merkle import _assert_tree
from test_gpu_merkle_absent import _key, _keys
from test_gpu_merkle_record_update import Placed
from test_gpu_merkle_segments import _prover, _witnesses

pytestmark = pytest.mark.gpu

SEED = bytes((59 * i + 13) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_locate", "merkle_balances", "merkle_adjust_records", "merkle_balance_sum", "merkle_transfer_records", "merkle_owners", "merkle_remove_records",
         "merkle_inert", "merkle_insert_records", "sha256_records", "merkle_record_rows", "merkle_updates", "merkle_level", "merkle_paths", "merkle_absent_rows",
         "merkle_segments")


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


def _split(steps, K):
    return _keys([s[0] for s in steps], K), np.array([s[1] for s in steps], dtype=np.uint64), np.array([s[2] for s in steps], dtype=np.uint8)


def _raw(ctx, tree, table, K, A, steps, rows, roots, index, status, in_stride=None, sides=True):
    vp = ctypes.c_void_p
    ptr = lambda a: vp(a.ctypes.data) if a is not None else None  # noqa: E731
    k, v, s = _split(steps, K)
    return ctx.lib.mfh_merkle_adjust_keys(ctx._h, tree._h, vp(table.view.data_ptr()), table.stride, table.length, K, A, len(steps), ptr(k), K, ptr(v), ptr(s) if sides else None,
                                          ptr(rows), (rows.shape[1] if rows is not None else 0) if in_stride is None else in_stride, ptr(roots), ptr(index), ptr(status))


def _adjust(ctx, tree, table, K, A, steps, sides=True):
    """one raw call: (rc, rows, roots, index, status)"""
    nk, depth = len(steps), tree.depth
    rows = np.zeros((nk, row_bytes(K, table.length, depth, A)), dtype=np.uint8)
    roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.full(nk, 0xCDCDCDCD, dtype=np.uint32), np.full(nk, 0xCD, dtype=np.uint8)
    rc = _raw(ctx, tree, table, K, A, steps, rows, roots, index, status, sides=sides)
    return rc, rows, roots, index, status


def _check(ctx, records, K, A, steps, what, model=None, sides=True, **placing):
    """one batch on a fresh tree and table against the model (given with its `want`, when another placing has run it already)"""
    depth = len(records).bit_length() - 1
    if model is None:
        model = AdjustModel(records, K, A)
        model.want = model.adjust_batch(steps)
    want_index, want_rows, want_roots = model.want
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        rc, rows, roots, index, status = _adjust(ctx, tree, table, K, A, steps, sides)
        assert rc == 0, (what, ctx.lib.mfh_last_error(ctx._h).decode())
        assert np.array_equal(index, want_index) and (status == 0).all(), (what, index, want_index, status)
        assert [r.tobytes() for r in roots] == want_roots, what
        assert np.array_equal(rows, want_rows), what
        table.holds(model.records, what)
        _assert_tree(tree, model.levels, what)
    finally:
        tree.close()
    return model


def _sequential(ctx, W, records, K, A, steps):
    """the route a user has without the call, one step at a time on a tree and table of its own: (index, rows, roots, the table's records)"""
    records = list(records)
    length, depth = len(records[0]), len(records).bit_length() - 1
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        index, roots = [], [tree.root()]
        rows = np.zeros((len(steps), row_bytes(K, length, depth, A)), dtype=np.uint8)
        for j, (key, v, side) in enumerate(steps):
            at, st = tree.locate_keys(table.view, _keys([key], K))
            assert st.tolist() == [1]
            i = int(at[0])
            new = W.indexed_adjust(records[i], int(v), int(side), K, amount_bytes=A)
            one, r = tree.update_records(table.view, [i], new.reshape(1, length), roots=True)
            records[i] = new.tobytes()
            index.append(i)
            roots.append(r[1].tobytes())
            rows[j] = np.concatenate([np.zeros(64, dtype=np.uint8), np.frombuffer(key + int(v).to_bytes(A, "big") + bytes([side]), dtype=np.uint8), one[0, 64: 64 + length],
                                      one[0, 64 + 2 * length:]])
        table.holds(records, "the per-step route")
        return np.array(index, dtype=np.uint32), rows, roots, records
    finally:
        tree.close()


def _accounts(K, count):
    top = 0x10 << (8 * (K - 1))
    xs = (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))
    return [_key(x, K) for x in xs][:count]


# ---------------------------------------------------------------------------------------------------------------- 1. every account, both sides
def _every_account(W, K=4, A=8, length=19, depth=3, seed=21000):
    rng = np.random.default_rng(seed)
    keys = _accounts(K, (1 << depth) - 1)  # a full table: record 0 the sentinel's, record r account r - 1's
    records = ledger(W, {k: 1000 + 100 * i for i, k in enumerate(keys)}, K, depth, length, A, rng)
    steps = [(k, 10 + i, 0) for i, k in enumerate(keys)] + [(k, 1000 + 100 * i, 1) for i, k in enumerate(keys)] + [(keys[2], 0, 1), (keys[6], 0, 0), (keys[0], 10, 1)]
    return keys, records, steps


def test_every_account_both_sides(ctx, W):
    K, A = 4, 8
    keys, records, steps = _every_account(W)
    model = _check(ctx, records, K, A, steps, "every account", stride=22, off=1)
    assert model.want[0].tolist() == list(range(1, 8)) * 2 + [3, 7, 1] and [model.balance(r) for r in range(1, 8)] == [0] + [10 + i for i in range(1, 7)]
    s_index, s_rows, s_roots, s_records = _sequential(ctx, W, records, K, A, steps)
    assert np.array_equal(s_index, model.want[0]) and np.array_equal(s_rows, model.want[1]) and s_roots == model.want[2] and s_records == model.records
    deposits = [s for s in steps if s[2] == 0]
    _check(ctx, records, K, A, deposits, "sides = NULL: all deposits", sides=False, stride=19, off=3)


@pytest.mark.parametrize("cuts", [[1], [2], [1, 2]])
def test_every_account_both_sides_cut(ctx, W, cuts):
    K, A, depth, length = 4, 8, 3, 19
    keys, records, steps = _every_account(W)
    want_rows, want_nodes, want_index, want_roots, model = adjust_cut_batch(records, K, A, steps, cuts)
    k, v, s = _split(steps, K)
    nk, c0 = len(steps), cuts[0]
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        ta, tb = Placed(ctx, records, stride=length + 2, off=3), Placed(ctx, records, stride=length + 2, off=3)
        a.set_records(0, ta.view)
        b.set_records(0, tb.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rows, nodes, index = a.adjust_key_segments(ta.view, k, v, cuts, sides=s, amount_bytes=A)
        counts = _drain(ctx)
        ctx.set_timing(False)
        assert counts == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_balances": 1, "merkle_adjust_records": 1, "merkle_segments": 1, "merkle_updates": depth + 1,
                                                    "merkle_record_rows": 2, "sha256_records": 1}, cuts
        assert rows[0].shape == (nk, row_bytes(K, length, c0, A)) and all(r.shape[0] == nk for r in rows[1:])
        for g, (got, want) in enumerate(zip(rows, want_rows)):
            assert got.shape == want.shape and np.array_equal(got, want), (cuts, g)
        assert np.array_equal(index, want_index) and np.array_equal(nodes, want_nodes)
        assert np.array_equal(nodes[:, -1, 0], want_roots[:-1]) and np.array_equal(nodes[:, -1, 1], want_roots[1:])
        ta.holds(model.records, cuts)
        _assert_tree(a, model.levels, cuts)
        # as update_record_segments gives them for nk updates: the same table route on the second tree
        new = np.stack([np.frombuffer(r, dtype=np.uint8) for r in _replay(records, K, A, steps)])
        u_rows, u_nodes = b.update_record_segments(tb.view, want_index, new, cuts)
        assert np.array_equal(u_nodes, nodes) and all(np.array_equal(x, y) for x, y in zip(u_rows[1:], rows[1:]))
        assert np.array_equal(ta.whole.cpu().numpy(), tb.whole.cpu().numpy())
        # the uncut call's rows sliced are segment 0's
        tb2 = Placed(ctx, records)
        b.set_records(0, tb2.view)
        urows, uindex, uroots = b.adjust_keys(tb2.view, k, v, sides=s, amount_bytes=A, roots=True)
        assert np.array_equal(uindex, index) and np.array_equal(uroots, want_roots)
        head = 64 + K + A + 1 + length
        for j in range(nk):
            low = int(index[j]) & ((1 << c0) - 1)
            want0 = np.concatenate([urows[j, : head + 32 * c0], np.frombuffer(low.to_bytes((c0 + 7) // 8, "little"), dtype=np.uint8)])
            assert np.array_equal(rows[0][j], want0), (cuts, j)
        bits = b.adjust_key_segment_bits(tb2.view, k[:2], [1, 2], cuts, sides=[0, 1], amount_bytes=A)[0]
        edges = [0] + cuts + [depth]
        assert [x.shape for x in bits] == [(2, 512 + 8 * (K + A + 1) + 8 * length + 257 * c0)] + [(2, 1024 + 257 * (hi - lo)) for lo, hi in zip(edges[1:], edges[2:])]
    finally:
        ctx.set_timing(False)
        a.close()
        b.close()


def _replay(records, K, A, steps):
    """the new record of every step, in order"""
    m = AdjustModel(records, K, A)
    out = []
    for step in steps:
        i, _ = m.adjust(*step)
        out.append(m.records[i])
    return out


def test_a_key_five_times_and_a_withdrawal_the_batch_covers(ctx, W):
    K, A, depth, length = 4, 2, 2, 11
    rng = np.random.default_rng(21100)
    a, b, c = _accounts(K, 3)
    records = ledger(W, {a: 5, b: 0xFFF0, c: 0}, K, depth, length, A, rng)
    steps = [(a, 100, 0), (b, 15, 0), (a, 105, 1), (a, 0xFFFF, 0), (c, 0, 1), (a, 0xFFFF, 1), (a, 7, 0)]  # 105 > 5: only the deposit of 100 covers it; up to the limit and back
    model = _check(ctx, records, K, A, steps, "five times", stride=length + 1, off=2)
    assert model.want[0].tolist() == [1, 2, 1, 1, 3, 1, 1] and (model.balance(1), model.balance(2), model.balance(3)) == (7, 0xFFFF, 0)
    assert AdjustModel(records, K, A).statuses(steps[2:3])[1].tolist() == [3]  # ... alone it overdraws
    many = [(a, 1 + j if j % 2 else 100 + j, j % 2) if j % 3 else (b, 0, 1) for j in range(2, 2 + (1 << depth) + 5)]  # more steps than the table has slots
    _check(ctx, records, K, A, many, "more steps than slots", stride=length, off=1)


def test_nk_zero_and_no_rows(ctx, W):
    K, A, depth, length = 4, 8, 3, 19
    keys, records, steps = _every_account(W)
    model = AdjustModel(records, K, A)
    before = model.root()
    want_index, want_rows, want_roots = model.adjust_batch(steps)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        assert ctx.lib.mfh_merkle_adjust_keys(ctx._h, tree._h, None, table.stride, length, K, A, 0, None, K, None, None, None, 0, None, None, None) == 0
        none = np.zeros((0, K), dtype=np.uint8)
        rows0, index0, roots0 = tree.adjust_keys(table.view, none, [], amount_bytes=A, roots=True)
        assert rows0.shape == (0, row_bytes(K, length, depth, A)) and index0.shape == (0,) and roots0.tobytes() == before
        assert tree.adjust_bits(table.view, none, [])[0].shape == (0, 512 + 8 * (K + A + 1) + 8 * length + 257 * depth)
        rows0, nodes0, index0 = tree.adjust_key_segments(table.view, none, [], [1])
        assert [r.shape[0] for r in rows0] == [0, 0] and nodes0.shape == (0, 2, 2, 32)
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        table.holds(records, "nk = 0")
        # h_inputs = NULL: the adjusts, no rows
        nk = len(steps)
        roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.zeros(nk, dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, A, steps, None, roots, index, status) == 0
        assert np.array_equal(index, want_index) and (status == 0).all() and [r.tobytes() for r in roots] == want_roots
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_balances": 1, "merkle_adjust_records": 1, "sha256_records": 1, "merkle_record_rows": 1,
                                                         "merkle_updates": depth + 1}
        table.holds(model.records, "no rows")
        _assert_tree(tree, model.levels, "no rows")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. alignment
@pytest.mark.parametrize("K", [1, 5, 7, 8, 32])
def test_alignment_sweep(ctx, W, K):
    depth = 3
    for A in (1, 3, 8):
        lengths = [n for n in (16, 55, 56) if n >= 2 * K + A] or [2 * K + A, 2 * K + A + 7]
        top = (1 << (8 * A)) - 1
        for length in lengths:
            rng = np.random.default_rng(21200 + 1000 * K + 100 * A + length)
            if K == 1:
                keys = [bytes([x]) for x in (0x10, 0x50, 0x51, 0x60, 0xFE)]
            else:
                keys = sorted({rng.bytes(K) for _ in range(6)})
            records = ledger(W, {k: int(rng.integers(top // 4, top // 2 + 1)) for k in keys}, K, depth, length, A, rng, shuffle=True)
            # every byte of the balance changes; an account twice; whichever record is the table's last (its unit ends at the span's end) is somebody's or is gathered around
            steps = [(keys[0], top // 5, 1), (keys[1], top // 3, 0), (keys[2], top // 7, 1), (keys[0], top // 9, 0), (keys[3], 1, 1), (keys[4], top // 2 - 1, 0), (keys[-1], 0, 0)]
            model = None
            for stride, off in ((length, 3), (length + 5, 1), (length + 5, 2)):
                model = _check(ctx, records, K, A, steps, (K, A, length, stride, off), model=model, stride=stride, off=off)


# ---------------------------------------------------------------------------------------------------------------- 3. batch sizes
@pytest.fixture(scope="module")
def depth_10(W):
    depth, K, A, length = 10, 8, 8, 55
    rng = np.random.default_rng(21300)
    members = sorted({rng.bytes(K) for _ in range(500)})
    records = ledger(W, {k: int(rng.integers(0, 1 << 40)) for k in members}, K, depth, length, A, rng, shuffle=True)
    return members, records


@pytest.mark.parametrize("nk", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_depth_10(ctx, depth_10, nk):
    K, A, length = 8, 8, 55
    members, records = depth_10
    rng = np.random.default_rng(21300 + nk)
    accounts = [members[int(i)] for i in rng.permutation(len(members))[:40]]
    run = AdjustModel(records, K, A)
    balance = {k: run.balance(run.own(k)) for k in accounts}
    steps = []
    for j in range(nk):  # withdrawals around the running balances: many spend what the batch delivered
        k = accounts[int(rng.integers(0, 40))]
        side = int(rng.integers(0, 2))
        v = int(rng.integers(0, balance[k] + 1)) if side else int(rng.integers(0, 1 << 41))
        balance[k] += -v if side else v
        steps.append((k, v, side))
    _check(ctx, records, K, A, steps, nk, stride=length + 1, off=2)


# ---------------------------------------------------------------------------------------------------------------- 4. two chunks
def test_two_chunks(ctx, W):
    depth, K, A, length = 2, 4, 8, 1 << 19
    rowb = row_bytes(K, length, depth, A)
    per_chunk = (64 << 20) // rowb
    nk = per_chunk + 1
    assert per_chunk == 127 and nk == 128
    rng = np.random.default_rng(21400)
    keys = _accounts(K, 3)
    records = ledger(W, {k: 10000 for k in keys}, K, depth, length, A, rng, shuffle=True)
    steps = [(keys[j % 3], 1 + j, j % 2) for j in range(nk - 2)]
    steps += [(keys[0], 20000, 0), (keys[0], 25000, 1)]  # steps 126 and 127, on both sides of the seam: 127 spends what 126 delivered
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rc, rows, roots, index, status = _adjust(ctx, tree, table, K, A, steps)
        counts = {kind: ctx.timing_drain(kind)[::2] for kind in KINDS}
        ctx.set_timing(False)
        assert rc == 0 and (status == 0).all(), ctx.lib.mfh_last_error(ctx._h).decode()
        assert counts == dict.fromkeys(KINDS, (0, 0)) | {"merkle_locate": (1, 1 << depth), "merkle_balances": (1, 3), "merkle_adjust_records": (1, nk), "sha256_records": (2, nk),
                                                         "merkle_record_rows": (4, nk), "merkle_updates": (2 * (depth + 1), nk * depth)}
        model = AdjustModel(records, K, A)
        want_index, want_rows, want_roots = model.adjust_batch(steps)
        assert np.array_equal(index, want_index) and [r.tobytes() for r in roots] == want_roots and np.array_equal(rows, want_rows)
        table.holds(model.records, "two chunks")
        _assert_tree(tree, model.levels, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. failures
def test_statuses_leave_everything_as_it_was(ctx, W, mf):
    depth, K, A, length = 3, 2, 2, 9
    rng = np.random.default_rng(21500)
    a, b, c, ghost = (_key(x, K) for x in (0x1000, 0x2000, 0x7000, 0x6000))
    records = ledger(W, {a: 100, b: 0xFFF0, c: 5}, K, depth, length, A, rng)  # slots 1, 2, 3
    records[5] = ghost + ghost + records[5][2 * K:]  # the lo of an inert record alone: no member
    model = AdjustModel(records, K, A)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        cases = [("a key that is no member", [(a, 1, 0), (ghost, 0, 0), (c, 1, 1)], [1, NONE, 3], [0, 1, 0], "not a member"),
                 ("an overdraft at the third step", [(a, 60, 1), (a, 5, 0), (a, 46, 1), (a, 45, 1)], [1, 1, 1, 1], [0, 0, 3, 0], "overdraws"),
                 ("an overflow at the second step", [(b, 15, 0), (b, 1, 0), (b, 16, 1), (c, 0, 0)], [2, 2, 2, 3], [0, 4, 0, 0], "past 2^(8 amount_bytes) - 1")]
        texts = set()
        for what, steps, want_i, want_s, word in cases:
            m_index, m_status = model.statuses(steps)
            assert m_status.tolist() == want_s and m_index.tolist() == want_i, what
            rc, rows, roots, index, status = _adjust(ctx, tree, table, K, A, steps)
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_adjust_keys: ") and word in text and f"h_status {max(want_s)}" in text, (what, rc, text)
            texts.add(text)
            assert status.tolist() == want_s and index.tolist() == want_i, (what, status, index)
            assert not rows.any() and not roots.any(), what
            assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_balances": 1}, what
            table.holds(records, what)
            _assert_tree(tree, model.levels, what)
            assert tree.root() == model.root()
        assert len(texts) == 3  # one text a status
        ctx.set_timing(False)
        with pytest.raises(mf.MfhError) as e:
            tree.adjust_keys(table.view, _keys([a], K), [101], sides=[1], amount_bytes=A)
        assert "mfh_merkle_adjust_keys: a withdrawal overdraws" in str(e.value)
        with pytest.raises(mf.MfhError) as e:
            tree.adjust_key_segments(table.view, _keys([b], K), [16], [1], amount_bytes=A)
        assert "mfh_merkle_adjust_keys_cut: a deposit takes" in str(e.value)
        table.holds(records, "after the refused calls")
        rc, rows, roots, index, status = _adjust(ctx, tree, table, K, A, [(b, 15, 0), (c, 5, 1)])
        assert rc == 0 and index.tolist() == [2, 3] and status.tolist() == [0, 0]
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals, launch counts
def test_einval_up_front(ctx, mf, W):
    lib, h = ctx.lib, ctx._h
    depth, K, A, length = 3, 4, 3, 17
    rng = np.random.default_rng(21600)
    keys = sorted({rng.bytes(K) for _ in range(5)})
    records = ledger(W, {k: 1000 for k in keys}, K, depth, length, A, rng)
    model = AdjustModel(records, K, A)
    rowb = row_bytes(K, length, depth, A)
    tree = ctx.merkle_tree(depth)
    vp = ctypes.c_void_p
    try:
        table = Placed(ctx, records, stride=length + 3, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        k = _keys(keys[0:3], K)
        zero, ones = k.copy(), k.copy()
        zero[1], ones[2] = 0, 0xFF
        v, big = np.array([1, 2, 3], dtype=np.uint64), np.array([1, 1 << 24, 3], dtype=np.uint64)
        s, two = np.array([0, 1, 0], dtype=np.uint8), np.array([0, 1, 2], dtype=np.uint8)
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((4, 32), 0xAB, dtype=np.uint8)
        index, status = np.full(3, 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        kp, zp, op, vp_, gp, sp_, wp, bp, rp, ip, sp = (vp(x.ctypes.data) for x in (k, zero, ones, v, big, s, two, buf, roots, index, status))
        tp, ts, stride = vp(table.view.data_ptr()), table.stride, buf.shape[1]
        cut = np.array([1], dtype=np.uint32)
        seg0, seg1 = np.full((3, row_bytes(K, length, 1, A) + 2), 0xAB, dtype=np.uint8), np.full((3, 128 + 64 + 1), 0xAB, dtype=np.uint8)
        ptrs = (ctypes.c_void_p * 2)(seg0.ctypes.data, seg1.ctypes.data)
        strides = (ctypes.c_size_t * 2)(seg0.shape[1], seg1.shape[1])
        short = (ctypes.c_size_t * 2)(seg0.shape[1] - 3, seg1.shape[1])
        cp = vp(cut.ctypes.data)

        def plain(t_, table_p, table_s, length_, K_, A_, nk, keys_p, key_s, amounts_p, sides_p, rows_p, in_s, index_p, status_p, handle=h):
            return lib.mfh_merkle_adjust_keys(handle, t_, table_p, table_s, length_, K_, A_, nk, keys_p, key_s, amounts_p, sides_p, rows_p, in_s, rp, index_p, status_p)

        def cut_call(t_, table_p, table_s, length_, K_, A_, nk, keys_p, key_s, amounts_p, sides_p, rows_p, in_s, index_p, status_p, handle=h, cuts=cp, st=strides):
            return lib.mfh_merkle_adjust_keys_cut(handle, t_, table_p, table_s, length_, K_, A_, nk, keys_p, key_s, amounts_p, sides_p, 1, cuts, ptrs, st, rp, index_p, status_p)

        for who, g in (("mfh_merkle_adjust_keys", plain), ("mfh_merkle_adjust_keys_cut", cut_call)):
            texts = []

            def refused(rc, handle=h):
                assert rc == EINVAL, who
                text = lib.mfh_last_error(handle).decode()
                assert text.startswith(who + ": "), text
                texts.append(text)

            ok = (tree._h, tp, ts, length, K, A, 3, kp, K, vp_, sp_, bp, stride, ip, sp)

            def but(**changes):
                names = ("tree", "table", "ts", "length", "K", "A", "nk", "k", "ks", "v", "s", "rows", "in_s", "index", "status")
                return tuple(changes.get(n, x) for n, x in zip(names, ok))

            refused(g(*but(tree=None)))
            refused(g(*but(K=0)))
            refused(g(*but(K=33, length=80, ks=33, in_s=1 << 12)))
            texts.pop()  # (key_bytes 0 and 33: one text)
            refused(g(*but(A=0)))
            refused(g(*but(A=9)))
            texts.pop()  # (amount_bytes 0 and 9: one text)
            refused(g(*but(length=2 * K - 1)))
            refused(g(*but(length=2 * K + A - 1)))  # room for the keys, not for the balance
            refused(g(*but(ts=length - 1)))
            refused(g(*but(ks=K - 1)))
            for name in ("table", "k", "v", "index", "status"):
                refused(g(*but(**{name: None})))
            refused(g(*but(k=zp)))
            refused(g(*but(k=op)))
            texts.pop()  # (the two sentinels: one text)
            refused(g(*but(s=wp)))  # a side of 2
            refused(g(*but(v=gp)))  # 2^24 does not fit three bytes
            if g is plain:
                refused(g(*but(in_s=rowb - 1)))
                assert "64 + key_bytes + amount_bytes + 1 + length + 32 depth + ceil(depth / 8)" in texts[-1]
                refused(g(*but(rows=None, in_s=0, k=zp)))  # no rows: a sentinel is refused too
                texts.pop()
            else:
                refused(g(*ok, st=short))
                refused(g(*ok, cuts=None))
            assert g(*ok, handle=None) == EINVAL
            assert len(set(texts)) == len(texts) == (16 if g is plain else 17), sorted(texts)
        assert cut_call(*but(nk=0)) == 0
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xAB).all() and (index == 0xCDCDCDCD).all() and (status == 0xCD).all() and (seg0 == 0xAB).all() and (seg1 == 0xAB).all()
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        # mfh_merkle_balance_sum's
        total, live = (ctypes.c_uint64 * 2)(7, 7), ctypes.c_uint32(7)
        texts = []
        for args in [(None, tp, ts, length, K, A, total), (tree._h, tp, ts, length, 0, A, total), (tree._h, tp, ts, 80, 33, A, total), (tree._h, tp, ts, length, K, 0, total),
                     (tree._h, tp, ts, length, K, 9, total), (tree._h, tp, ts, 2 * K + A - 1, K, A, total), (tree._h, tp, length - 1, length, K, A, total),
                     (tree._h, None, ts, length, K, A, total), (tree._h, tp, ts, length, K, A, None)]:
            assert lib.mfh_merkle_balance_sum(h, *args, ctypes.byref(live)) == EINVAL
            text = lib.mfh_last_error(h).decode()
            assert text.startswith("mfh_merkle_balance_sum: "), text
            texts.append(text)
        assert len(set(texts)) == 7 and (total[0], total[1], live.value) == (7, 7, 7)
        assert lib.mfh_merkle_balance_sum(None, tree._h, tp, ts, length, K, A, total, None) == EINVAL
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        assert lib.mfh_merkle_balance_sum(h, tree._h, tp, ts, length, K, A, total, None) == 0 and (total[0], total[1]) == (supply(records, K, A)[0], 0)  # h_live may be NULL
        assert {kind: ctx.timing_drain(kind)[::2] for kind in KINDS} == dict.fromkeys(KINDS, (0, 0)) | {"merkle_balance_sum": (2, 1 << depth)}
        ctx.set_timing(False)
        for bad in [(k[0], [1, 2, 3], None), (k, [1, 2], None), (k, [1, -2, 3], None), (k, [1, 2.5, "x"], None), (zero, [1, 2, 3], None), (k, [1, 1 << 24, 3], None),
                    (k, [1, 2, 3], [0, 1]), (k, [1, 2, 3], [0, 1, 2]), (k, [1, 2, 1003], [0, 0, 1])]:
            for call in (lambda *x: tree.adjust_keys(table.view, x[0], x[1], sides=x[2], amount_bytes=A), lambda *x: tree.adjust_key_segments(table.view, x[0], x[1], [1], sides=x[2], amount_bytes=A)):
                with pytest.raises(mf.MfhError):
                    call(*bad)
        for ab in (0, 9, 10, 2.0):  # (10: the record has no room)
            with pytest.raises(mf.MfhError):
                tree.adjust_keys(table.view, k, [1, 2, 3], amount_bytes=ab)
            with pytest.raises(mf.MfhError):
                tree.total_balance(table.view, K, amount_bytes=ab)
        for cuts in ([], [0], [3], [2, 1]):
            with pytest.raises(mf.MfhError):
                tree.adjust_key_segments(table.view, k, [1, 2, 3], cuts, amount_bytes=A)
        with pytest.raises(mf.MfhError):
            tree.total_balance(table.view, 0, amount_bytes=A)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
    finally:
        ctx.set_timing(False)
        tree.close()


def test_launch_counts_and_stride(ctx, depth_10):
    depth, K, A, length, nk = 10, 8, 8, 55, 100
    members, records = depth_10
    rng = np.random.default_rng(21700)
    steps = [(members[int(rng.integers(0, 30))], int(rng.integers(0, 1 << 30)), 0) for _ in range(nk)]
    nu = len({s[0] for s in steps})
    model = AdjustModel(records, K, A)
    want_index, want_rows, want_roots = model.adjust_batch(steps)
    rowb = row_bytes(K, length, depth, A)
    assert rowb == 64 + 8 + 8 + 1 + 55 + 320 + 2
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        buf = np.full((nk, rowb + 13), 0xAB, dtype=np.uint8)
        index, status = np.zeros(nk, dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, A, steps, buf, None, index, status) == 0  # a wider in_stride, no roots
        assert np.array_equal(buf[:, :rowb], want_rows) and (buf[:, rowb:] == 0xAB).all() and np.array_equal(index, want_index)
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | {
            "merkle_locate": (1, 1 << depth), "merkle_balances": (1, nu), "merkle_adjust_records": (1, nk), "sha256_records": (1, nk), "merkle_record_rows": (2, nk),
            "merkle_updates": (depth + 1, nk * depth)}  # one search, one gather, one build launch; depth + 1 tree launches a chunk, as update_records
        print(f"depth {depth}: {nk} adjusts: " + ", ".join(f"{k} {v[1]:.3f} ms" for k, v in timed.items() if v[0]))
        table.holds(model.records, "rows")
        ctx.set_timing(False)
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        k, v, s = _split(steps, K)
        bits, index3 = tree.adjust_bits(table.view, k[:3], [int(x) for x in v[:3]])  # sides=None
        assert bits.shape == (3, 512 + 8 * (K + A + 1) + 8 * length + 257 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows[:3])
        assert np.array_equal(index3, want_index[:3])
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. streams, staging
def _late_table(ctx, W):
    depth, K, A, length, nk = 9, 4, 8, 24, 64
    rng = np.random.default_rng(21800)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = ledger(W, {k: 1 << 33 for k in members}, K, depth, length, A, rng, shuffle=True)
    steps = [(members[int(rng.integers(0, 20))], int(rng.integers(0, 1 << 28)), int(rng.integers(0, 2))) for _ in range(nk)]
    model = AdjustModel(records, K, A)
    before = model.supply()
    want_index, want_rows, want_roots = model.adjust_batch(steps)  # (first: nothing of the host's stands between the late table and the calls)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        assert tree.total_balance(table.view, K, A) == before
        rows, index, roots = tree.adjust_keys(table.view, *_split(steps, K)[:2], sides=_split(steps, K)[2], roots=True)
        assert np.array_equal(index, want_index) and np.array_equal(rows, want_rows) and [r.tobytes() for r in roots] == want_roots
        assert tree.total_balance(table.view, K, A) == model.supply()
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


def test_the_same_after_scrub_staging(ctx, W):
    K, A, depth, length = 4, 8, 3, 19
    keys, records, steps = _every_account(W)
    model = AdjustModel(records, K, A)
    before = model.supply()
    want_index, want_rows, want_roots = model.adjust_batch(steps)
    tree = ctx.merkle_tree(depth)
    try:
        for scrub in (False, True):  # the pinned staging zeroed between two identical calls: the same rows from the same starting table
            table = Placed(ctx, records, stride=length + 1)
            tree.set_records(0, table.view)
            if scrub:
                assert ctx.scrub_staging() == 0
            assert tree.total_balance(table.view, K, A) == before
            if scrub:
                assert ctx.scrub_staging() == 0
            rc, rows, roots, index, status = _adjust(ctx, tree, table, K, A, steps)
            assert rc == 0 and np.array_equal(rows, want_rows) and np.array_equal(index, want_index) and [r.tobytes() for r in roots] == want_roots
            table.holds(model.records, scrub)
        assert ctx.scrub_staging() == 0
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. the supply
def _garbage(records, K, rng):
    """every inert slot gets lo >= hi -- equal, or above -- and random balance bytes: none of it counts"""
    out = []
    for r in records:
        if r[:K] < r[K: 2 * K]:
            out.append(r)
            continue
        lo = rng.bytes(K)
        hi = lo if rng.integers(0, 2) else bytes(K)
        out.append(lo + hi + bytes(b | 0x80 for b in rng.bytes(len(r) - 2 * K)))
    return out


@pytest.mark.parametrize("depth", [1, 6, 8, 9, 12])
def test_total_balance_depths(ctx, W, depth):
    K, length = 4, 21
    rng = np.random.default_rng(21900 + depth)
    nmem = 1 if depth == 1 else (1 << depth) * 2 // 3
    members = sorted({rng.bytes(K) for _ in range(nmem)} - {bytes(K), b"\xff" * K})
    tree = ctx.merkle_tree(depth)
    try:
        for A in range(1, 9):
            top = (1 << (8 * A)) - 1
            records = ledger(W, {k: int(rng.integers(0, top, endpoint=True, dtype=np.uint64)) for k in members}, K, depth, length, A, rng, shuffle=True)
            records = _garbage(records, K, rng)
            want = supply(records, K, A)
            assert want[1] == len(members) + 1 and sum(1 for r in records if not r[:K] < r[K: 2 * K]) == (1 << depth) - want[1]
            table = Placed(ctx, records, stride=length + (A % 3), off=A % 4)
            assert tree.total_balance(table.view, K, amount_bytes=A) == want, (depth, A)
            table.holds(records, "only read")
    finally:
        tree.close()


def test_total_balance_high_word(ctx, W):
    depth, K, A, length = 11, 8, 8, 24
    rng = np.random.default_rng(22000)
    members = sorted({rng.bytes(K) for _ in range(1023)})
    records = ledger(W, dict.fromkeys(members, (1 << 64) - 1), K, depth, length, A, rng, shuffle=True)
    records = [r[: 2 * K] + b"\xff" * A + r[2 * K + A:] if r[:K] < r[K: 2 * K] else r for r in records]  # the sentinel's record too: 1 024 live records
    records = _garbage(records, K, rng)
    want = supply(records, K, A)
    assert want == (1024 * ((1 << 64) - 1), 1024) and want[0] >> 64 == 1023
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        assert tree.total_balance(table.view, K) == want
        total, live = (ctypes.c_uint64 * 2)(), ctypes.c_uint32()
        assert ctx.lib.mfh_merkle_balance_sum(ctx._h, tree._h, ctypes.c_void_p(table.view.data_ptr()), table.stride, length, K, A, total, ctypes.byref(live)) == 0
        assert (total[0], total[1], live.value) == ((1 << 64) - 1024, 1023, 1024)
    finally:
        tree.close()


@pytest.mark.parametrize("K", [1, 5, 8, 32])
def test_total_balance_key_widths(ctx, W, K):
    depth = 9  # two workgroups
    tree = ctx.merkle_tree(depth)
    try:
        for A, length in ((8, 2 * K + 8), (3, 2 * K + 3 + 6), (5, max(55, 2 * K + 5))):
            rng = np.random.default_rng(22100 + 10 * K + A)
            members = sorted({rng.bytes(K) for _ in range(200)} - {bytes(K), b"\xff" * K})
            top = (1 << (8 * A)) - 1
            records = _garbage(ledger(W, {k: int(rng.integers(0, top, endpoint=True, dtype=np.uint64)) for k in members}, K, depth, length, A, rng, shuffle=True), K, rng)
            want = supply(records, K, A)
            for stride, off in ((length, 1), (length + 5, 2), (length + 3, 3)):
                table = Placed(ctx, records, stride=stride, off=off)
                assert tree.total_balance(table.view, K, amount_bytes=A) == want, (K, A, stride, off)
    finally:
        tree.close()


def test_conservation(ctx, W):
    depth, K, A, length = 8, 8, 8, 55
    rng = np.random.default_rng(22200)
    members = sorted({rng.bytes(K) for _ in range(100)})
    records = _garbage(ledger(W, {k: int(rng.integers(1 << 30, 1 << 62)) for k in members}, K, depth, length, A, rng, shuffle=True), K, rng)
    before = supply(records, K, A)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        assert tree.total_balance(table.view, K) == before
        pairs = [tuple(members[int(i)] for i in rng.permutation(100)[:2]) for _ in range(50)]
        tree.transfer_keys(table.view, _keys([p[0] for p in pairs], K), _keys([p[1] for p in pairs], K), [int(rng.integers(0, 1 << 20)) for _ in pairs])
        assert tree.total_balance(table.view, K) == before  # a transfer conserves the supply
        steps = [(members[int(rng.integers(0, 100))], int(rng.integers(0, 1 << 19)), int(rng.integers(0, 2))) for _ in range(60)]
        k, v, s = _split(steps, K)
        tree.adjust_keys(table.view, k, v, sides=s)
        change = sum(int(x) for x, side in zip(v, s) if not side) - sum(int(x) for x, side in zip(v, s) if side)
        assert tree.total_balance(table.view, K) == (before[0] + change, before[1])
        got = [bytes(r) for r in table.view.cpu().numpy()]
        assert supply(got, K, A) == (before[0] + change, before[1])
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. end to end
A_KEY, B_KEY, C_KEY = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("c1aa557f")
STEPS = [(A_KEY, 0x100000000, 0), (A_KEY, 0xFFFFFFFF, 1), (C_KEY, 5, 0)]  # a deposit, a withdrawal of part of it (a long borrow), a deposit to another key


def _rejected(st, pair, step):
    """the statements a proof of (pair, step) must NOT verify against: a flipped amount bit, a flipped side, another key, the two roots swapped"""
    key, v, side = step
    return [st.statement(*pair, key, v ^ (1 << 9), side), st.statement(*pair, key, v, side ^ 1), st.statement(*pair, B_KEY, v, side), st.statement(pair[1], pair[0], key, v, side)]


def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 19, m=349525)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth, A = 4, 16, 2, 8
    st = W.MerkleAdjust(K, length, depth, A)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == st.lu == 616 and (cc.nwires, cc.nrows) == W.MERKLE_ADJUST_SIZES[(K, length, depth, A)]
    rng = np.random.default_rng(22300)
    records = ledger(W, {A_KEY: 7, B_KEY: 1000, C_KEY: 77}, K, depth, length, A, rng)
    model = AdjustModel(records, K, A)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        k, v, s = _split(STEPS, K)
        bits, index, roots = tree.adjust_bits(table.view, k, v, sides=s, roots=True)
        want_index, want_rows, want_roots = model.adjust_batch(STEPS)
        assert bits.shape == (3, st.nin) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows) and index.tolist() == want_index.tolist() == [1, 1, 3]
        assert [r.tobytes() for r in roots] == want_roots and len(set(want_roots)) == 4
        table.holds(model.records, "end to end")
        assert (model.balance(1), model.balance(3)) == (8, 82)
    finally:
        tree.close()
    pairs = list(zip(want_roots, want_roots[1:]))
    over = st.bits(A_KEY, 8, 1, records[1], AdjustModel(records, K, A).siblings(1), 1)  # a fourth row that overdraws the table as it first stood by one
    prog = ctx.circuit_load(cc, state="auto")
    try:
        witness, holds = ctx.circuit_assign(prog, np.stack(list(bits) + [over]))
    finally:
        prog.close()
    assert holds.tolist() == [True] * 3 + [False]
    for j in range(3):
        assert st.roots_of(witness[j]) == pairs[j], j
    ctx.ssp_set_rows(cc.rows, lu_max=lu)
    count, first = ctx.ssp_rows_violations(witness)
    assert not count[:3].any() and (first[:3] == 0xFFFFFFFF).all() and count[3] > 0 and first[3] != 0xFFFFFFFF
    prove, verify = _prover(ctx, p, cc, rng, 3)
    proofs = prove(witness)
    own = [st.statement(*pairs[j], *STEPS[j]) for j in range(3)]
    assert all(len(x) == lu // 8 for x in own) and own == [witness[j][: lu // 8].tobytes() for j in range(3)]
    assert verify(proofs, own) == [True] * 3
    for which in range(4):
        assert verify(proofs, [_rejected(st, pairs[j], STEPS[j])[which] for j in range(3)]) == [False] * 3, which
    print(f"test_end_to_end_proofs (MerkleAdjust(4, 16, 2, 8), d = 2^19): {time.time() - t0:.1f} s")


def test_end_to_end_cut_adjusts(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p18, p17 = mf.Params(d=1 << 18, m=174762), mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p18)
    ctx.set_seed(SEED)
    K, length, depth, A, cuts = 4, 16, 2, 8, [1]
    st, seg = W.MerkleAdjust(K, length, 1, A), W.MerkleSegment(1)
    cc = st.circuit.compile(p18)
    assert cc.lu == st.lu == 616 and (cc.nwires, cc.nrows) == W.MERKLE_ADJUST_SIZES[(K, length, 1, A)]
    rng = np.random.default_rng(22400)
    records = ledger(W, {A_KEY: 7, B_KEY: 1000, C_KEY: 77}, K, depth, length, A, rng)
    want_rows, want_nodes, want_index, want_roots, model = adjust_cut_batch(records, K, A, STEPS, cuts)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        k, v, s = _split(STEPS, K)
        bits, nodes, index = tree.adjust_key_segment_bits(table.view, k, v, cuts, sides=s)
        table.holds(model.records, "end to end")
    finally:
        tree.close()
    assert index.tolist() == [1, 1, 3] and np.array_equal(nodes, want_nodes)
    assert all(np.array_equal(np.packbits(b, axis=1, bitorder="little"), w) for b, w in zip(bits, want_rows))
    # the verifier's side: statements from the returned nodes alone
    pub = [[(nodes[j, g, 0].tobytes(), nodes[j, g, 1].tobytes()) for g in range(2)] for j in range(3)]
    assert [x[1] for x in pub] == [(want_roots[j].tobytes(), want_roots[j + 1].tobytes()) for j in range(3)]
    own = [st.statement(*pub[j][0], *STEPS[j]) for j in range(3)]
    witness = _witnesses(ctx, cc, bits[0])
    assert [st.roots_of(witness[j]) for j in range(3)] == [x[0] for x in pub] and own == [witness[j][: st.lu // 8].tobytes() for j in range(3)]
    prove, verify = _prover(ctx, p18, cc, rng, 3)
    proofs = prove(witness)
    assert verify(proofs, own) == [True] * 3
    for which in range(4):
        assert verify(proofs, [_rejected(st, pub[j][0], STEPS[j])[which] for j in range(3)]) == [False] * 3, which

    c17 = gpu_ctx_factory(p17)
    c17.set_seed(SEED)
    cs = seg.circuit.compile(p17)
    assert (cs.nwires, cs.nrows) == W.MERKLE_SEGMENT_SIZES[1]
    w_seg = _witnesses(c17, cs, bits[1])
    assert [seg.tops_of(w_seg[j]) for j in range(3)] == [x[1] for x in pub]
    prove, verify = _prover(c17, p17, cs, rng, 3)
    proofs = prove(w_seg)
    own_seg = [W.MerkleSegment.chain(pub[j])[0] for j in range(3)]
    assert verify(proofs, own_seg) == [True] * 3
    assert verify(proofs, own_seg[1:] + own_seg[:1]) == [False] * 3
    assert verify(proofs, [W.MerkleSegment.statement(x[0][1], x[0][0], x[1][1], x[1][0]) for x in pub]) == [False] * 3  # both pairs swapped
    print(f"test_end_to_end_cut_adjusts (MerkleAdjust(4, 16, 1, 8) at d = 2^18, three MerkleSegment(1) at d = 2^17): {time.time() - t0:.1f} s")
