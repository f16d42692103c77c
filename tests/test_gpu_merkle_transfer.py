"""GPU: a batch of sequential transfers between the accounts of an indexed table on the device in ONE call (mfh_merkle_transfer_keys, MerkleTree.transfer_keys /
transfer_bits) and with the path cut (mfh_merkle_transfer_keys_cut, MerkleTree.transfer_key_segments).

Every case compares h_index, h_status, the rows, the roots, the table's whole allocation (tests/test_gpu_merkle_record_update.py's Placed, with its 0xA5
surroundings) and the tree's nodes against
  the per-step route through the EXISTING calls on a second tree and table: per transfer locate_keys for the two keys, words.indexed_transfer on a host copy
  of the two records, update_records -- the transfer's row put together out of the two MerkleRecordUpdate rows; and
  the brute-force model of tests/merkle_transfer_model.py, its rows MerkleTransfer.bits on a stand-in made without its circuit (test 1's first case checks that
  the stand-in and the real statement give the same bits).

1. hand-made ledgers at depth 2 and 3, key_bytes 1 and 4, amount_bytes 8 and 2: one transfer; v = 0 and v = the whole balance; an account sending three times;
   a chain a -> b -> c in which b spends what it has just received; more transfers than the table has slots.
2. key widths 1, 3, 4, 5, 8, 20, 32 at depth 3.
3. alignment: key_bytes 7 with amount_bytes 8 (the balance, bytes [14, 22), straddles a 16-byte unit) and key_bytes 4 with amount_bytes 3; lengths 2K + A,
   2K + A + 1, 55, 64, 65; the table 0 .. 3 bytes into its tensor; strides length and length + 5.
4. 300 transfers among 40 accounts in a shuffled table at depth 12.
5. two chunks: key_bytes 4, length 2^19 (a chunk is 63 transfers), 64 transfers among five accounts at depth 3, an account on both sides of the seam.
6. each status (a sender and a receiver that are no members, an overdraft, an overflow, at a later step of the batch): MFH_EINVAL, h_status and h_index
   filled, nothing written, no record or tree kernel; every up-front MFH_EINVAL case leaves the timing counts as they were; nk = 0 does nothing.
7. h_inputs = NULL; the launch counts of one chunk by timing kind; a wider in_stride keeps its tail; insert_keys and remove_keys launch what they did.
8. a table produced late on the null stream and on a caller's.
9. the cut call at depth 3 under [1], [2], [1, 2] and at depth 9 under [4]: rows, nodes and roots against the model and against the uncut rows sliced.
10. end to end with MerkleTransfer(4, 16, 1, 8) at Params(d=1 << 19, m=349525): three transfers proved and verified, a statement with v + 1 rejected; one cut
    transfer at depth 3 under [1] with its MerkleSegment(2) proofs verified from the published nodes alone."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

from merkle_transfer_model import TransferModel, ledger, row_bytes, stand_in, transfer_cut_batch
from test_gpu_merkle import _assert_tree, _flip
from test_gpu_merkle_absent import _key, _keys, _table
from test_gpu_merkle_record_update import Placed
from test_gpu_merkle_segments import _prover, _witnesses

pytestmark = pytest.mark.gpu

SEED = bytes((53 * i + 11) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_locate", "merkle_balances", "merkle_transfer_records", "merkle_owners", "merkle_remove_records", "merkle_inert", "merkle_insert_records", "sha256_records",
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


def _split(steps, K):
    return _keys([s[0] for s in steps], K), _keys([s[1] for s in steps], K), np.array([s[2] for s in steps], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the two references
def _raw(ctx, tree, table, K, A, steps, rows, roots, index, status, in_stride=None):
    vp = ctypes.c_void_p
    ptr = lambda a: vp(a.ctypes.data) if a is not None else None  # noqa: E731
    f, t, v = _split(steps, K)
    return ctx.lib.mfh_merkle_transfer_keys(ctx._h, tree._h, vp(table.view.data_ptr()), table.stride, table.length, K, A, len(steps), ptr(f), ptr(t), K, ptr(v), ptr(rows),
                                            (rows.shape[1] if rows is not None else 0) if in_stride is None else in_stride, ptr(roots), ptr(index), ptr(status))


def _sequential(ctx, W, records, K, A, steps, **placing):
    """the route a user has without the call, one transfer at a time on a tree and table of its own: (index, rows, roots, the table's image, the tree's levels)"""
    records = list(records)
    length, depth = len(records[0]), len(records).bit_length() - 1
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        index, roots = [], [tree.root()]
        rows = np.zeros((len(steps), row_bytes(K, length, depth, A)), dtype=np.uint8)
        for j, (k_from, k_to, v) in enumerate(steps):
            at, st = tree.locate_keys(table.view, _keys([k_from, k_to], K))
            assert st.tolist() == [1, 1]
            p, s = int(at[0]), int(at[1])
            idx, new = W.indexed_transfer(records[p], p, records[s], s, int(v), K, amount_bytes=A)
            two, r = tree.update_records(table.view, idx, new, roots=True)
            for i, rec in zip(idx, new):
                records[i] = rec.tobytes()
            index.append(idx)
            roots.append(r[2].tobytes())
            head = 64 + 2 * length
            bits = sum(((p >> l) & 1) << l | ((s >> l) & 1) << (depth + l) for l in range(depth))
            rows[j] = np.concatenate([np.zeros(64, dtype=np.uint8), np.frombuffer(k_from + k_to + int(v).to_bytes(A, "big"), dtype=np.uint8), two[0, 64: 64 + length],
                                      two[1, 64: 64 + length], two[0, head: head + 32 * depth], two[1, head: head + 32 * depth],
                                      np.frombuffer(bits.to_bytes((2 * depth + 7) // 8, "little"), dtype=np.uint8)])
        levels = [tree.nodes(l).cpu().numpy().tobytes() for l in range(depth + 1)]
        return np.array(index, dtype=np.uint32).reshape(len(steps), 2), rows, roots, table.whole.cpu().numpy(), levels
    finally:
        tree.close()


def _transfer(ctx, tree, table, K, A, steps):
    """one raw call: (rc, rows, roots, index, status)"""
    nk, depth = len(steps), tree.depth
    rows = np.zeros((nk, row_bytes(K, table.length, depth, A)), dtype=np.uint8)
    roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.full((nk, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(nk, 0xCD, dtype=np.uint8)
    rc = _raw(ctx, tree, table, K, A, steps, rows, roots, index, status)
    return rc, rows, roots, index, status


def _check(ctx, W, records, K, A, steps, what, seq=None, model=None, **placing):
    """one batch on a fresh tree and table against the per-step route (seq: its results, when another placing has them already) and the model"""
    depth = len(records).bit_length() - 1
    if model is None:
        model = TransferModel(records, K, A)
        model.want = model.transfer_batch(steps)
    want_index, want_rows, want_roots = model.want
    own = seq is None  # (another placing's sequential result is compared in everything but the allocation's image)
    if own:
        seq = _sequential(ctx, W, records, K, A, steps, **placing)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        rc, rows, roots, index, status = _transfer(ctx, tree, table, K, A, steps)
        assert rc == 0, (what, ctx.lib.mfh_last_error(ctx._h).decode())
        assert np.array_equal(index, want_index) and (status == 0).all(), (what, index, want_index, status)
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


def _accounts(K, count):
    top = 0x10 << (8 * (K - 1))
    xs = (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))
    return [_key(x, K) for x in xs][:count]


# ---------------------------------------------------------------------------------------------------------------- 1. hand-made ledgers
@pytest.mark.parametrize("K,A", [(1, 8), (4, 8), (4, 2)])
@pytest.mark.parametrize("depth", [2, 3])
def test_hand_made_ledgers(ctx, W, depth, K, A):
    rng = np.random.default_rng(19000 + 100 * depth + 10 * K + A)
    length = 2 * K + A + 3
    keys = _accounts(K, (1 << depth) - 1)  # a full table: record 0 the sentinel's, record r account r - 1's
    top = (1 << (8 * A)) - 1
    a, b, c = keys[0], keys[1], keys[2]
    records = ledger(W, {**{k: 1000 + i for i, k in enumerate(keys)}, a: 50000, b: 0, c: top - 7}, K, depth, length, A, rng)
    placing = dict(stride=length + 3, off=1)
    if depth == 2 and K == 4 and A == 8:  # the stand-in gives what the statement gives
        args = TransferModel(records, K, A).transfer(a, b, 5)[2]
        assert np.array_equal(stand_in(K, length, depth, A).bits(*args), W.MerkleTransfer(K, length, depth, A).bits(*args))
    model, _ = _check(ctx, W, records, K, A, [(a, b, 300)], (depth, K, A, "one"), **placing)
    assert model.want[0].tolist() == [[1, 2]] and (model.balance(1), model.balance(2)) == (49700, 300)
    _check(ctx, W, records, K, A, [(a, b, 0)], (depth, K, A, "nothing"), **placing)
    model, _ = _check(ctx, W, records, K, A, [(a, b, 50000), (b, c, 7)], (depth, K, A, "the whole balance, and up to the limit"), **placing)
    assert (model.balance(1), model.balance(2), model.balance(3)) == (0, 49993, top)
    model, _ = _check(ctx, W, records, K, A, [(a, b, 10), (a, c, 1), (a, b, 49989)], (depth, K, A, "three times"), **placing)
    assert (model.balance(1), model.balance(2)) == (0, 49999)
    model, _ = _check(ctx, W, records, K, A, [(a, b, 7), (b, c, 7), (c, b, top)], (depth, K, A, "a chain"), stride=length, off=3)  # b had nothing; c reaches the limit and hands it on
    assert model.want[0].tolist() == [[1, 2], [2, 3], [3, 2]] and (model.balance(1), model.balance(2), model.balance(3)) == (49993, top, 0)
    back_and_forth = [(a, b, 10 + j) if j % 2 == 0 else (b, a, 1 + j) for j in range((1 << depth) + 3)]  # more transfers than the table has slots
    _check(ctx, W, records, K, A, back_and_forth, (depth, K, A, "back and forth"), **placing)


# ---------------------------------------------------------------------------------------------------------------- 2. key widths
@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 20, 32])
def test_key_widths(ctx, W, K):
    depth, A = 3, 8
    rng = np.random.default_rng(19100 + K)
    length = 2 * K + A + 1
    if K == 1:
        keys = [bytes([x]) for x in (0x10, 0x50, 0x51, 0x60, 0xFE)]
    else:
        rest, mid = rng.bytes(K - 1), rng.bytes(K - 2)
        keys = [bytes([0x10]) + rest, bytes([0x20]) + rest, bytes([0x50]) + mid + bytes([0x10]), bytes([0x50]) + mid + bytes([0x11]), bytes([0x60]) + bytes(K - 2) + b"\xff",
                bytes([0x60]) + bytes(K - 3) + b"\x01\x00"]
    assert keys == sorted(keys)
    records = ledger(W, {k: int(rng.integers(1 << 40, 1 << 62)) for k in keys}, K, depth, length, A, rng, shuffle=True)
    order = [int(i) for i in rng.permutation(len(keys))]
    steps = [(keys[i], keys[j], int(rng.integers(0, 1 << 40))) for i, j in zip(order, order[1:] + order[:1])] + [(keys[2], keys[3], 1), (keys[3], keys[2], 1 << 39)]
    _check(ctx, W, records, K, A, steps, K, stride=length + 2, off=3)


# ---------------------------------------------------------------------------------------------------------------- 3. alignment
@pytest.mark.parametrize("K,A", [(7, 8), (4, 3)])
def test_alignment_sweep(ctx, W, K, A):
    depth = 3
    for length in (2 * K + A, 2 * K + A + 1, 55, 64, 65):
        rng = np.random.default_rng(19200 + 100 * K + length)
        keys = sorted({rng.bytes(K) for _ in range(6)})
        top = (1 << (8 * A)) - 1
        records = ledger(W, {k: int(rng.integers(top // 4, top // 2)) for k in keys}, K, depth, length, A, rng, shuffle=True)
        # every byte of the balance changes on both sides; an account twice; the last record of the table (its unit ends at the span's end) is somebody's
        steps = [(keys[0], keys[1], top // 5), (keys[1], keys[2], top // 4), (keys[3], keys[0], top // 7), (keys[4], keys[5], 1), (keys[5], keys[4], top // 9)]
        model = seq = None
        for stride in (length, length + 5):
            for off in range(4):
                model, got = _check(ctx, W, records, K, A, steps, (K, A, length, stride, off), seq=seq, model=model, stride=stride, off=off)
                seq = got


# ---------------------------------------------------------------------------------------------------------------- 4. many steps among few accounts
def test_300_transfers_among_40_accounts_depth_12(ctx, W):
    depth, K, A, length, nk = 12, 8, 8, 55, 300
    rng = np.random.default_rng(19300)
    members = sorted({rng.bytes(K) for _ in range(700)})
    accounts = [members[int(i)] for i in rng.permutation(len(members))[:40]]
    balances = {k: (int(rng.integers(0, 1000)) if k in accounts else 5) for k in members}
    records = ledger(W, balances, K, depth, length, A, rng, shuffle=True)
    run = {k: balances[k] for k in accounts}
    steps = []
    while len(steps) < nk:  # amounts around the running balances: many steps spend what the batch delivered
        f, t = (accounts[int(i)] for i in rng.permutation(40)[:2])
        v = int(rng.integers(0, run[f] + 1))
        run[f], run[t] = run[f] - v, run[t] + v
        steps.append((f, t, v))
    model, _ = _check(ctx, W, records, K, A, steps, "300 among 40", stride=length + 1, off=2)
    assert len({int(i) for i in model.want[0].ravel()}) <= 40 and sum(run.values()) == sum(balances[k] for k in accounts)


# ---------------------------------------------------------------------------------------------------------------- 5. two chunks
def test_two_chunks(ctx, W):
    depth, K, A, length = 3, 4, 8, 1 << 19
    rowb = row_bytes(K, length, depth, A)
    per_chunk = (64 << 20) // rowb
    nk = per_chunk + 1
    assert per_chunk == 63 and nk == 64
    rng = np.random.default_rng(19400)
    keys = _accounts(K, 5)
    records = ledger(W, {k: 10000 for k in keys}, K, depth, length, A, rng, shuffle=True)
    steps = [(keys[j % 5], keys[(j + 1 + j % 3) % 5], 1 + j) for j in range(nk - 2)]
    steps += [(keys[0], keys[1], 3), (keys[1], keys[2], 5000)]  # transfers 62 and 63, on both sides of the seam: 63's old record of p is what 62 left
    assert len(steps) == nk and all(s[0] != s[1] for s in steps)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rc, rows, roots, index, status = _transfer(ctx, tree, table, K, A, steps)
        counts = {kind: ctx.timing_drain(kind)[::2] for kind in KINDS}
        ctx.set_timing(False)
        assert rc == 0 and (status == 0).all(), ctx.lib.mfh_last_error(ctx._h).decode()
        assert counts == dict.fromkeys(KINDS, (0, 0)) | {"merkle_locate": (1, 1 << depth), "merkle_balances": (1, 5), "merkle_transfer_records": (1, 2 * nk),
                                                         "sha256_records": (2, 2 * nk), "merkle_record_rows": (4, 2 * nk), "merkle_updates": (2 * (depth + 1), 2 * nk * depth)}
        model = TransferModel(records, K, A)
        want_index, want_rows, want_roots = model.transfer_batch(steps)
        assert np.array_equal(index, want_index) and [r.tobytes() for r in roots] == want_roots and np.array_equal(rows, want_rows)
        table.holds(model.records, "two chunks")
        _assert_tree(tree, model.levels, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()
    # ... and the per-step route, on the records' first 40 bytes
    _check(ctx, W, [r[:40] for r in records], K, A, steps, "two chunks' batch, short records", stride=41, off=1)


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_statuses_leave_everything_as_it_was(ctx, W):
    depth, K, A, length = 3, 2, 2, 9
    rng = np.random.default_rng(19500)
    a, b, c, ghost = (_key(x, K) for x in (0x1000, 0x2000, 0x7000, 0x6000))
    records = ledger(W, {a: 100, b: 0xFFF0, c: 5}, K, depth, length, A, rng)  # slots 1, 2, 3
    records[5] = ghost + ghost + records[5][2 * K:]  # the lo of an inert record alone: no member
    model = TransferModel(records, K, A)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        cases = [("a sender that is no member", [(a, c, 1), (ghost, a, 0), (c, a, 1)], [[1, 3], [NONE, 1], [3, 1]], [0, 1, 0]),
                 ("a receiver that is no member", [(a, ghost, 1)], [[1, NONE]], [2]),
                 ("neither", [(ghost, _key(0x6001, K), 1)], [[NONE, NONE]], [1]),
                 ("an overdraft at the third step", [(a, c, 60), (c, a, 65), (a, c, 106), (a, c, 105)], [[1, 3], [3, 1], [1, 3], [1, 3]], [0, 0, 3, 0]),
                 ("what the batch delivered is spendable, one more is not", [(a, c, 100), (c, a, 106)], [[1, 3], [3, 1]], [0, 3]),
                 ("an overflow at the second step", [(a, b, 15), (a, b, 1), (c, b, 0)], [[1, 2]] * 2 + [[3, 2]], [0, 4, 0]),
                 ("overdraft before overflow", [(c, b, 16)], [[3, 2]], [3])]
        texts = set()
        for what, steps, want_i, want_s in cases:
            m_index, m_status = model.statuses(steps)
            assert m_status.tolist() == want_s and m_index.tolist() == want_i, what
            rc, rows, roots, index, status = _transfer(ctx, tree, table, K, A, steps)
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_transfer_keys: "), (what, rc, text)
            texts.add(text)
            assert status.tolist() == want_s and index.tolist() == want_i, (what, status, index)
            assert not rows.any() and not roots.any(), what
            assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_balances": 1}, what
            table.holds(records, what)
            _assert_tree(tree, model.levels, what)
        assert len(texts) == 4  # one text a status
        ctx.set_timing(False)
        rc, rows, roots, index, status = _transfer(ctx, tree, table, K, A, [(a, b, 15), (c, a, 5)])
        assert rc == 0 and index.tolist() == [[1, 2], [3, 1]] and status.tolist() == [0, 0]
    finally:
        ctx.set_timing(False)
        tree.close()


def test_einval_up_front(ctx, mf, W):
    lib, h = ctx.lib, ctx._h
    depth, K, A, length = 3, 4, 3, 17
    rng = np.random.default_rng(19600)
    keys = sorted({rng.bytes(K) for _ in range(5)})
    records = ledger(W, {k: 1000 for k in keys}, K, depth, length, A, rng)
    model = TransferModel(records, K, A)
    rowb = row_bytes(K, length, depth, A)
    tree = ctx.merkle_tree(depth)
    vp = ctypes.c_void_p
    try:
        table = Placed(ctx, records, stride=length + 3, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        f, t = _keys(keys[0:3], K), _keys(keys[1:4], K)
        zero, ones, same = t.copy(), f.copy(), t.copy()
        zero[1], ones[2], same[2] = 0, 0xFF, f[2]
        v, big = np.array([1, 2, 3], dtype=np.uint64), np.array([1, 1 << 24, 3], dtype=np.uint64)
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((7, 32), 0xAB, dtype=np.uint8)
        index, status = np.full((3, 2), 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        fp, tp_, zp, op, sp_, vp_, gp, bp, rp, ip, sp = (vp(x.ctypes.data) for x in (f, t, zero, ones, same, v, big, buf, roots, index, status))
        tp, ts, stride = vp(table.view.data_ptr()), table.stride, buf.shape[1]
        cut = np.array([1], dtype=np.uint32)
        seg0, seg1 = np.full((3, row_bytes(K, length, 1, A, zeros=128) + 2), 0xAB, dtype=np.uint8), np.full((6, 128 + 64 + 1), 0xAB, dtype=np.uint8)
        ptrs = (ctypes.c_void_p * 2)(seg0.ctypes.data, seg1.ctypes.data)
        strides = (ctypes.c_size_t * 2)(seg0.shape[1], seg1.shape[1])
        cp = vp(cut.ctypes.data)

        def plain(t_, table_p, table_s, length_, K_, A_, nk, from_p, to_p, key_s, amounts_p, rows_p, in_s, index_p, status_p, handle=h):
            return lib.mfh_merkle_transfer_keys(handle, t_, table_p, table_s, length_, K_, A_, nk, from_p, to_p, key_s, amounts_p, rows_p, in_s, rp, index_p, status_p)

        def cut_call(t_, table_p, table_s, length_, K_, A_, nk, from_p, to_p, key_s, amounts_p, rows_p, in_s, index_p, status_p, handle=h):
            return lib.mfh_merkle_transfer_keys_cut(handle, t_, table_p, table_s, length_, K_, A_, nk, from_p, to_p, key_s, amounts_p, 1, cp, ptrs, strides, rp, index_p, status_p)

        for who, g in (("mfh_merkle_transfer_keys", plain), ("mfh_merkle_transfer_keys_cut", cut_call)):
            texts = []

            def refused(rc, handle=h):
                assert rc == EINVAL, who
                text = lib.mfh_last_error(handle).decode()
                assert text.startswith(who + ": "), text
                texts.append(text)

            ok = (tree._h, tp, ts, length, K, A, 3, fp, tp_, K, vp_, bp, stride, ip, sp)

            def but(**changes):
                names = ("tree", "table", "ts", "length", "K", "A", "nk", "f", "t", "ks", "v", "rows", "in_s", "index", "status")
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
            for name in ("table", "f", "t", "v", "index", "status"):
                refused(g(*but(**{name: None})))
            refused(g(*but(t=zp)))
            refused(g(*but(f=op)))
            texts.pop()  # (the two sentinels, a receiver and a sender: one text)
            refused(g(*but(t=sp_)))  # from == to in step 2
            refused(g(*but(v=gp)))  # 2^24 does not fit three bytes
            if g is plain:
                refused(g(*but(in_s=rowb - 1)))
                refused(g(*but(rows=None, in_s=0, t=zp)))  # no rows: a sentinel is refused too
                texts.pop()
            assert g(*ok, handle=None) == EINVAL
            assert len(set(texts)) == len(texts) == (17 if g is plain else 16), sorted(texts)
        # nk = 0 does nothing, whatever the pointers
        assert plain(tree._h, None, ts, length, K, A, 0, None, None, K, None, None, 0, None, None) == 0
        assert cut_call(*but(nk=0)) == 0
        none = np.zeros((0, K), dtype=np.uint8)
        rows0, index0, roots0 = tree.transfer_keys(table.view, none, none, [], amount_bytes=A, roots=True)
        assert rows0.shape == (0, rowb) and index0.shape == (0, 2) and roots0.tobytes() == model.root()
        assert tree.transfer_bits(table.view, none, none, [], amount_bytes=A)[0].shape == (0, 512 + 16 * K + 8 * A + 16 * length + 514 * depth)
        rows0, nodes_p0, nodes_s0, index0 = tree.transfer_key_segments(table.view, none, none, [], [1], amount_bytes=A)
        assert [r.shape[0] for r in rows0] == [0, 0] and nodes_p0.shape == nodes_s0.shape == (0, 2, 2, 32)
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xAB).all() and (index == 0xCDCDCDCD).all() and (status == 0xCD).all() and (seg0 == 0xAB).all() and (seg1 == 0xAB).all()
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        for bad in [(f[0], t, [1, 2, 3]), (f, t[:2], [1, 2, 3]), (f, t, [1, 2]), (f, t, [1, -2, 3]), (f, t, [1, 2.5, "x"]), (f, same, [1, 2, 3]), (f, zero, [1, 2, 3]), (f, t, [1, 1 << 24, 3]),
                    (f, t, [1, 2, 1003])]:
            for call in (lambda *x: tree.transfer_keys(table.view, *x, amount_bytes=A), lambda *x: tree.transfer_key_segments(table.view, *x, [1], amount_bytes=A)):
                with pytest.raises(mf.MfhError):
                    call(*bad)
        for ab in (0, 9, 10, 2.0):  # (10: the record has no room)
            with pytest.raises(mf.MfhError):
                tree.transfer_keys(table.view, f, t, [1, 2, 3], amount_bytes=ab)
        with pytest.raises(mf.MfhError) as e:
            tree.transfer_keys(table.view, f, t, [1, 2, 1003], amount_bytes=A)
        assert "mfh_merkle_transfer_keys: a transfer overdraws" in str(e.value)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. rows, launch counts
def test_no_rows_launch_counts_and_stride(ctx, W):
    depth, K, A, length, nk = 9, 8, 8, 55, 100
    rng = np.random.default_rng(19700)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = ledger(W, {k: 1 << 40 for k in members}, K, depth, length, A, rng, shuffle=True)
    accounts = members[:30]
    steps = []
    for j in range(nk):
        x, y = (int(i) for i in rng.permutation(30)[:2])
        steps.append((accounts[x], accounts[y], int(rng.integers(0, 1 << 30))))
    nu = len({k for s in steps for k in s[:2]})
    model = TransferModel(records, K, A)
    want_index, want_rows, want_roots = model.transfer_batch(steps)
    rowb = row_bytes(K, length, depth, A)
    assert rowb == 64 + 16 + 8 + 110 + 576 + 3
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.zeros((nk, 2), dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, A, steps, None, roots, index, status) == 0
        assert np.array_equal(index, want_index) and (status == 0).all() and [r.tobytes() for r in roots] == want_roots
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_balances": 1, "merkle_transfer_records": 1, "sha256_records": 1, "merkle_record_rows": 1,
                                                         "merkle_updates": depth + 1}
        table.holds(model.records, "no rows")
        _assert_tree(tree, model.levels, "no rows")
        # rows, a wider in_stride, no roots: one chunk's launches
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        _drain(ctx)
        buf = np.full((nk, rowb + 13), 0xAB, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, A, steps, buf, None, index, status) == 0
        assert np.array_equal(buf[:, :rowb], want_rows) and (buf[:, rowb:] == 0xAB).all()
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | {
            "merkle_locate": (1, 1 << depth), "merkle_balances": (1, nu), "merkle_transfer_records": (1, 2 * nk), "sha256_records": (1, 2 * nk),
            "merkle_record_rows": (2, 2 * nk), "merkle_updates": (depth + 1, 2 * nk * depth)}
        print(f"depth {depth}: {nk} transfers: " + ", ".join(f"{k} {v[1]:.3f} ms" for k, v in timed.items() if v[0]))
        table.holds(model.records, "rows")
        # the Python calls
        ctx.set_timing(False)
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        f, t, v = _split(steps, K)
        rows2, index2, roots2 = tree.transfer_keys(table.view, f, t, v, roots=True)
        assert np.array_equal(rows2, want_rows) and np.array_equal(index2, want_index) and [r.tobytes() for r in roots2] == want_roots
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        bits, index3 = tree.transfer_bits(table.view, f[:3], t[:3], [int(x) for x in v[:3]])
        assert bits.shape == (3, 512 + 16 * K + 8 * A + 16 * length + 514 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows[:3])
        assert np.array_equal(index3, want_index[:3])
    finally:
        ctx.set_timing(False)
        tree.close()


def test_inserts_and_removes_launch_what_they_did(ctx, W):
    depth, K, length, nk = 6, 4, 12, 5
    rng = np.random.default_rng(19800)
    members = sorted({rng.bytes(K) for _ in range(20)})
    records = _table(W, members[:15], K, depth, length, rng)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        tree.insert_keys(table.view, _keys(members[15:], K))
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_inert": 3, "merkle_insert_records": 1, "sha256_records": 1, "merkle_record_rows": 2,
                                                         "merkle_updates": depth + 1}
        tree.remove_keys(table.view, _keys(members[15:], K))
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_owners": 1, "merkle_remove_records": 1, "sha256_records": 1, "merkle_record_rows": 2, "merkle_updates": depth + 1}
        tree.locate_keys(table.view, _keys(members[:3], K))
        assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1}
        table.holds(records, "the round trip")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. streams
def _late_table(ctx, W):
    depth, K, A, length, nk = 9, 4, 8, 24, 64
    rng = np.random.default_rng(19900)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = ledger(W, {k: 1 << 33 for k in members}, K, depth, length, A, rng, shuffle=True)
    steps = []
    for j in range(nk):
        x, y = (int(i) for i in rng.permutation(20)[:2])
        steps.append((members[x], members[y], int(rng.integers(0, 1 << 28))))
    model = TransferModel(records, K, A)
    want_index, want_rows, want_roots = model.transfer_batch(steps)  # (first: nothing of the host's stands between the late table and the calls)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        rows, index, roots = tree.transfer_keys(table.view, *_split(steps, K), roots=True)
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


# ---------------------------------------------------------------------------------------------------------------- 9. the cut call
def _cut_check(ctx, W, records, K, A, steps, cuts, what, **placing):
    depth, length = len(records).bit_length() - 1, len(records[0])
    want_rows, want_p, want_s, want_index, want_roots, model = transfer_cut_batch(records, K, A, steps, cuts)
    nk, G, c0 = len(steps), len(cuts), cuts[0]
    f, t, v = _split(steps, K)
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        ta, tb = Placed(ctx, records, **placing), Placed(ctx, records, **placing)
        a.set_records(0, ta.view)
        b.set_records(0, tb.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rows, nodes_p, nodes_s, index = a.transfer_key_segments(ta.view, f, t, v, cuts, amount_bytes=A)
        counts = _drain(ctx)
        ctx.set_timing(False)
        assert counts == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_balances": 1, "merkle_transfer_records": 1, "merkle_segments": 1, "merkle_updates": depth + 1,
                                                    "merkle_record_rows": 2, "sha256_records": 1}, what
        assert rows[0].shape == (nk, row_bytes(K, length, c0, A, zeros=128)) and all(r.shape[0] == 2 * nk for r in rows[1:]), what
        for g, (got, want) in enumerate(zip(rows, want_rows)):
            assert got.shape == want.shape and np.array_equal(got, want), (what, g)
        assert np.array_equal(index, want_index) and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s), what
        assert np.array_equal(nodes_p[:, G, 1], nodes_s[:, G, 0]), what  # the root between the two updates
        assert np.array_equal(nodes_p[:, -1, 0], want_roots[0:-1:2]) and np.array_equal(nodes_s[:, -1, 1], want_roots[2::2]), what
        ta.holds(model.records, what)
        _assert_tree(a, model.levels, what)
        # the uncut call on the second tree: the same index, table and tree; its rows sliced are every segment's
        urows, uindex, uroots = b.transfer_keys(tb.view, f, t, v, amount_bytes=A, roots=True)
        assert np.array_equal(uindex, index) and np.array_equal(uroots, want_roots[0::2]), what
        assert np.array_equal(ta.whole.cpu().numpy(), tb.whole.cpu().numpy()), what
        _assert_tree(b, model.levels, what)
        head = 64 + 2 * K + A + 2 * length
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
def test_cut_transfers_depth_3(ctx, W, cuts):
    depth, K, A, length = 3, 4, 8, 19
    rng = np.random.default_rng(20000 + 10 * len(cuts) + cuts[0])
    keys = _accounts(K, 7)
    records = ledger(W, {k: 500 for k in keys}, K, depth, length, A, rng)
    # account r - 1 is record r: (2, 3) in one height-1 subtree; (3, 4) in two height-1 subtrees of one height-2 subtree; (1, 6) in two height-2 subtrees;
    # (3, 2) once more, spending what it received
    steps = [(keys[1], keys[2], 500), (keys[2], keys[3], 1), (keys[0], keys[5], 77), (keys[2], keys[1], 999)]
    assert transfer_cut_batch(records, K, A, steps, cuts)[3].tolist() == [[2, 3], [3, 4], [1, 6], [3, 2]]
    _cut_check(ctx, W, records, K, A, steps, cuts, ("depth 3", cuts), stride=length + 2, off=3)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        bits = tree.transfer_key_segment_bits(table.view, _keys([keys[4]], K), _keys([keys[6]], K), [3], cuts)[0]
    finally:
        tree.close()
    edges = [0] + cuts + [depth]
    assert [x.shape for x in bits] == [(1, 1024 + 16 * K + 8 * A + 16 * length + 514 * cuts[0])] + [(2, 1024 + 257 * (hi - lo)) for lo, hi in zip(edges[1:], edges[2:])]


def test_cut_transfers_depth_9(ctx, W):
    depth, K, A, length, nk = 9, 8, 5, 24, 40
    rng = np.random.default_rng(20100)
    members = sorted({rng.bytes(K) for _ in range(400)})
    records = ledger(W, {k: 1 << 30 for k in members}, K, depth, length, A, rng, shuffle=True)
    steps = []
    for j in range(nk):
        x, y = (int(i) for i in rng.permutation(12)[:2])
        steps.append((members[30 * x], members[30 * y], int(rng.integers(0, 1 << 25))))
    _cut_check(ctx, W, records, K, A, steps, [4], "depth 9 under [4]", stride=length + 1, off=2)


# ---------------------------------------------------------------------------------------------------------------- 10. end to end
A_KEY, B_KEY = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585")


def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 19, m=349525)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth, A = 4, 16, 1, 8
    st = W.MerkleTransfer(K, length, depth, A)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == st.lu == 640 and (cc.nwires, cc.nrows) == W.MERKLE_TRANSFER_SIZES[(K, length, depth, A)]
    rng = np.random.default_rng(20200)
    # a depth-1 table has no room for the sentinel record beside two accounts: the two records close the ring by hand
    records = [A_KEY + B_KEY + (0x0100000000000000).to_bytes(8, "big"), B_KEY + b"\xff" * K + (0x00000000FFFFFFFF).to_bytes(8, "big")]
    steps = [(A_KEY, B_KEY, 1), (B_KEY, A_KEY, 0x100000000), (A_KEY, B_KEY, 0x0100000000000000)]  # a long borrow and a long carry; the whole balance, just received; the top byte
    model = TransferModel(records, K, A)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        f, t, v = _split(steps, K)
        bits, index, roots = tree.transfer_bits(table.view, f, t, v, roots=True)  # three transfers in a table of two slots
        want_index, want_rows, want_roots = model.transfer_batch(steps)
        assert bits.shape == (3, st.nin) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows) and index.tolist() == want_index.tolist() == [[0, 1], [1, 0], [0, 1]]
        assert [r.tobytes() for r in roots] == want_roots and len(set(want_roots)) == 4
        table.holds(model.records, "end to end")
        assert (model.balance(0), model.balance(1)) == (0xFFFFFFFF, 0x0100000000000000)
        pairs = list(zip(want_roots, want_roots[1:]))
        # a fourth row that overdraws the table as it first stood by one: the subtractor's wires wrap to FF..FF, and s is opened beside that record
        wrapped = records[0][: 2 * K] + b"\xff" * 8
        over = st.bits(A_KEY, B_KEY, 0x0100000000000001, records[0], records[1], [hashlib.sha256(records[1]).digest()], 0, [hashlib.sha256(wrapped).digest()], 1)
        prog = ctx.circuit_load(cc, state="auto")
        try:
            witness, holds = ctx.circuit_assign(prog, np.stack(list(bits) + [over]))
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
        own = [st.statement(*pairs[k], *steps[k]) for k in range(3)]
        assert all(len(x) == lu // 8 for x in own) and own == [witness[k][: lu // 8].tobytes() for k in range(3)]
        assert verify(proofs, own) == [True] * 3
        assert verify(proofs, [st.statement(*pairs[k], steps[k][0], steps[k][1], steps[k][2] + 1) for k in range(3)]) == [False] * 3  # v + 1
        assert verify(proofs, [st.statement(*pairs[k], steps[k][1], steps[k][0], steps[k][2]) for k in range(3)]) == [False] * 3  # the other way round
        assert verify(proofs, [st.statement(pairs[k][1], pairs[k][0], *steps[k]) for k in range(3)]) == [False] * 3  # the roots swapped
        assert verify(proofs, [st.statement(_flip(pairs[0][0], 77), pairs[0][1], *steps[0]), st.statement(pairs[1][0], _flip(pairs[1][1], 200), *steps[1]), own[2]]) == [False, False, True]
    finally:
        tree.close()
    print(f"test_end_to_end_proofs (MerkleTransfer(4, 16, 1, 8), d = 2^19): {time.time() - t0:.1f} s")


def test_end_to_end_cut_transfer(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p19, p18 = mf.Params(d=1 << 19, m=349525), mf.Params(d=1 << 18, m=174762)
    ctx = gpu_ctx_factory(p19)
    ctx.set_seed(SEED)
    K, length, depth, A, cuts = 4, 16, 3, 8, [1]
    st, seg = W.MerkleTransfer(K, length, 1, A, joined=False), W.MerkleSegment(2)
    cc = st.circuit.compile(p19)
    assert cc.lu == st.lu == 1152 and (cc.nwires, cc.nrows) == W.MERKLE_TRANSFER_SPLIT_SIZES[(K, length, 1, A)]
    rng = np.random.default_rng(20300)
    keys = [_key(x, K) for x in (0x10, 0x6789ABCD, 0x7000_0000, 0x7100_0000)]
    records = ledger(W, {k: 1000 for k in keys}, K, depth, length, A, rng)  # record r = account r - 1
    step = (keys[1], keys[3], 250)  # p = record 2, s = record 4: two height-1 subtrees
    want_rows, want_p, want_s, want_index, want_roots, model = transfer_cut_batch(records, K, A, [step], cuts)
    assert want_index.tolist() == [[2, 4]]
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        bits, nodes_p, nodes_s, index = tree.transfer_key_segment_bits(table.view, *_split([step], K), cuts)
        table.holds(model.records, "end to end")
    finally:
        tree.close()
    assert index.tolist() == [[2, 4]] and np.array_equal(nodes_p, want_p) and np.array_equal(nodes_s, want_s)
    assert all(np.array_equal(np.packbits(b, axis=1, bitorder="little"), w) for b, w in zip(bits, want_rows))
    # the verifier's side: statements from the returned nodes alone
    pub_p = [(nodes_p[0, g, 0].tobytes(), nodes_p[0, g, 1].tobytes()) for g in range(2)]
    pub_s = [(nodes_s[0, g, 0].tobytes(), nodes_s[0, g, 1].tobytes()) for g in range(2)]
    r0, r_mid, r1 = (r.tobytes() for r in want_roots)
    assert pub_p[1] == (r0, r_mid) and pub_s[1] == (r_mid, r1) and len({r0, r_mid, r1}) == 3 and pub_p[0][1] != pub_s[0][0]
    own = st.statement(*pub_p[0], *pub_s[0], *step)

    witness = _witnesses(ctx, cc, bits[0])
    assert st.tops_of(witness[0]) == pub_p[0] + pub_s[0] and own == witness[0][: st.lu // 8].tobytes()
    prove, verify = _prover(ctx, p19, cc, rng, 1)
    proofs = prove(witness)
    assert verify(proofs, [own]) == [True]
    assert verify(proofs, [st.statement(*pub_p[0], *pub_s[0], step[0], step[1], 251)]) == [False]
    assert verify(proofs, [st.statement(*pub_p[0], *pub_s[0], step[0], keys[2], 250)]) == [False]
    assert verify(proofs, [st.statement(pub_p[0][1], pub_p[0][0], *pub_s[0], *step)]) == [False]

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
    print(f"test_end_to_end_cut_transfer (MerkleTransfer(4, 16, 1, 8, joined=False) at d = 2^19, two MerkleSegment(2) at d = 2^18): {time.time() - t0:.1f} s")
