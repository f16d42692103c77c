"""GPU: a batch of sequential writes by key on an indexed table in ONE call, plain and compare-and-set (mfh_merkle_write_keys, MerkleTree.write_keys /
write_bits), and with the path cut (mfh_merkle_write_keys_cut, MerkleTree.write_key_segments).

Every case compares h_index, h_status, the rows, the roots, the table's whole allocation (tests/test_gpu_merkle_record_update.py's Placed, with its 0xA5
surroundings) and the tree's nodes byte for byte against the brute-force model of tests/merkle_write_model.py, whose rows are put together byte by byte; test 1
also against the per-step route through the EXISTING calls (locate_keys, words.indexed_write, update_records).

1. a depth-3 table, K = 4, length 19, fields (8, 16) and (9, 14): every live key once, plain and with expectations, uncut and under [1], [2], [1, 2].
2. one key five times with e_j = v_j-1, which only the batch satisfies; a no-op write; nk = 0; h_inputs = NULL through the C call.
3. alignment: key widths 1, 5, 7, 8 and 32; the first payload byte alone, the last byte alone (hi = length), the whole payload, a field straddling a 16-byte
   unit of the record, F = 17 and 33 where the record has room; lengths 2K + F, 55 and 56; the table 1 .. 3 bytes into its tensor at strides length and
   length + 5.
4. 1, 63, 64, 65, 255, 256 and 257 steps at depth 10.
5. two chunks: length 2^19 (a chunk is 127 steps), 128 steps at depth 2, the field the record's last 8 bytes, a key on both sides of the seam.
6. a missing key, a failed expectation, and an expectation that the table met before the batch but an earlier step has since overwritten (status 5), each
   alone at a later step: status, text, table and root unchanged, no record or tree kernel.
7. every up-front refusal; the launch counts of a call by timing kind: plain merkle_locate 1, merkle_fields 0, merkle_write_records 1; with expectations
   merkle_fields 1; per chunk as adjust_keys.
8. late tables on the null stream and on a caller's; the same rows after mfh_scrub_staging.
9. neighbours: total_balance unchanged by writes outside the balance; check_table status 0 afterwards; a write on a pair that grow made.
10. end to end: three steps (A, A again expecting the first value, C) proved as MerkleWrite(4, 16, 2, (8, 16), expect=True) at d = 2^19, a fourth row with a
    wrong expectation does not hold; under [1] as MerkleWrite(4, 16, 1, ..) at d = 2^18 plus MerkleSegment(1) at d = 2^17 from the published nodes alone;
    every proof rejected under a flipped value bit, a flipped expected bit, another key and the two roots swapped."""
import ctypes
import time

import numpy as np
import pytest

from merkle_write_model import WriteModel, row_bytes, table_of, write_cut_batch
from test_gpu_merkle import _assert_tree
from test_gpu_merkle_absent import _key, _keys
from test_gpu_merkle_record_update import Placed
from test_gpu_merkle_segments import _prover, _witnesses

pytestmark = pytest.mark.gpu

SEED = bytes((61 * i + 17) & 0xFF for i in range(40))
EINVAL = -1
NONE = 0xFFFFFFFF
KINDS = ("merkle_locate", "merkle_fields", "merkle_write_records", "merkle_balances", "merkle_adjust_records", "merkle_balance_sum", "merkle_transfer_records",
         "merkle_owners", "merkle_remove_records", "merkle_inert", "merkle_insert_records", "sha256_records", "merkle_record_rows", "merkle_updates", "merkle_level",
         "merkle_paths", "merkle_absent_rows", "merkle_segments")


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


def _conditional(steps):
    return bool(steps) and len(steps[0]) == 3 and steps[0][2] is not None


def _split(steps, K, F):
    """(keys [nk, K], values [nk, F], expectations [nk, F] or None)"""
    arr = lambda xs: np.frombuffer(b"".join(bytes(x) for x in xs), dtype=np.uint8).reshape(len(xs), F).copy()  # noqa: E731
    return _keys([s[0] for s in steps], K), arr([s[1] for s in steps]), arr([s[2] for s in steps]) if _conditional(steps) else None


def _raw(ctx, tree, table, K, field, steps, rows, roots, index, status, in_stride=None):
    vp = ctypes.c_void_p
    ptr = lambda a: vp(a.ctypes.data) if a is not None else None  # noqa: E731
    F = field[1] - field[0]
    k, v, e = _split(steps, K, F)
    return ctx.lib.mfh_merkle_write_keys(ctx._h, tree._h, vp(table.view.data_ptr()), table.stride, table.length, K, field[0], field[1], len(steps), ptr(k), K, ptr(v), F, ptr(e), F,
                                         ptr(rows), (rows.shape[1] if rows is not None else 0) if in_stride is None else in_stride, ptr(roots), ptr(index), ptr(status))


def _write(ctx, tree, table, K, field, steps):
    """one raw call: (rc, rows, roots, index, status)"""
    nk, depth = len(steps), tree.depth
    rows = np.zeros((nk, row_bytes(K, table.length, depth, field[1] - field[0], _conditional(steps))), dtype=np.uint8)
    roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.full(nk, 0xCDCDCDCD, dtype=np.uint32), np.full(nk, 0xCD, dtype=np.uint8)
    rc = _raw(ctx, tree, table, K, field, steps, rows, roots, index, status)
    return rc, rows, roots, index, status


def _check(ctx, records, K, field, steps, what, model=None, **placing):
    """one batch on a fresh tree and table against the model (given with its `want`, when another placing has run it already)"""
    depth = len(records).bit_length() - 1
    if model is None:
        model = WriteModel(records, K, field)
        model.want = model.write_batch(steps)
    want_index, want_rows, want_roots = model.want
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, **placing)
        tree.set_records(0, table.view)
        rc, rows, roots, index, status = _write(ctx, tree, table, K, field, steps)
        assert rc == 0, (what, ctx.lib.mfh_last_error(ctx._h).decode())
        assert np.array_equal(index, want_index) and (status == 0).all(), (what, index, want_index, status)
        assert [r.tobytes() for r in roots] == want_roots, what
        assert np.array_equal(rows, want_rows), what
        table.holds(model.records, what)
        _assert_tree(tree, model.levels, what)
    finally:
        tree.close()
    return model


def _expecting(records, K, field, steps):
    """the plain steps (key, value) with the expectation each meets when they run in order"""
    m = WriteModel(records, K, field)
    out = []
    for key, value in steps:
        out.append((key, value, m.field(m.own(key))))
        m.write(key, value)
    return out


def _sequential(ctx, W, records, K, field, steps):
    """the route a user has without the call, one step at a time on a tree and table of its own: (index, rows, roots, the table's records)"""
    records = list(records)
    length, depth = len(records[0]), len(records).bit_length() - 1
    cond = _conditional(steps)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        index, roots = [], [tree.root()]
        rows = np.zeros((len(steps), row_bytes(K, length, depth, field[1] - field[0], cond)), dtype=np.uint8)
        for j, step in enumerate(steps):
            key, value, expect = (tuple(step) + (None,))[:3]
            at, st = tree.locate_keys(table.view, _keys([key], K))
            assert st.tolist() == [1]
            i = int(at[0])
            new = W.indexed_write(records[i], field, value, K, expect=expect)
            one, r = tree.update_records(table.view, [i], new.reshape(1, length), roots=True)
            records[i] = new.tobytes()
            index.append(i)
            roots.append(r[1].tobytes())
            rows[j] = np.concatenate([np.zeros(64, dtype=np.uint8), np.frombuffer(key + (expect or b"") + value, dtype=np.uint8), one[0, 64: 64 + length], one[0, 64 + 2 * length:]])
        table.holds(records, "the per-step route")
        return np.array(index, dtype=np.uint32), rows, roots, records
    finally:
        tree.close()


def _members(K, count):
    top = 0x10 << (8 * (K - 1))
    xs = (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))
    return [_key(x, K) for x in xs][:count]


def _random_table(W, rng, keys, K, depth, length, shuffle=False):
    return table_of(W, {k: rng.bytes(length - 2 * K) for k in keys}, K, depth, length, rng, shuffle=shuffle)


# ---------------------------------------------------------------------------------------------------------------- 1. every live key once
def _every_key(W, field, K=4, length=19, depth=3, seed=41000):
    rng = np.random.default_rng(seed)
    keys = _members(K, (1 << depth) - 1)  # a full table: record 0 the sentinel's, record r key r - 1's
    records = _random_table(W, rng, keys, K, depth, length)
    steps = [(k, rng.bytes(field[1] - field[0])) for k in keys]
    return keys, records, steps


@pytest.mark.parametrize("field", [(8, 16), (9, 14)])
def test_every_live_key_once(ctx, W, field):
    K = 4
    keys, records, steps = _every_key(W, field)
    for batch, placing in ((steps, dict(stride=22, off=1)), (_expecting(records, K, field, steps), dict(stride=19, off=3))):
        model = _check(ctx, records, K, field, batch, ("every key", field, _conditional(batch)), **placing)
        assert model.want[0].tolist() == list(range(1, 8))
        assert [r[: field[0]] + r[field[1]:] for r in model.records] == [r[: field[0]] + r[field[1]:] for r in records]  # nothing but the field
        s_index, s_rows, s_roots, s_records = _sequential(ctx, W, records, K, field, batch)
        assert np.array_equal(s_index, model.want[0]) and np.array_equal(s_rows, model.want[1]) and s_roots == model.want[2] and s_records == model.records


@pytest.mark.parametrize("cuts", [[1], [2], [1, 2]])
@pytest.mark.parametrize("field", [(8, 16), (9, 14)])
def test_every_live_key_once_cut(ctx, W, field, cuts):
    K, depth, length = 4, 3, 19
    F = field[1] - field[0]
    keys, records, plain = _every_key(W, field)
    for steps in (plain, _expecting(records, K, field, plain)):
        cond = _conditional(steps)
        want_rows, want_nodes, want_index, want_roots, model = write_cut_batch(records, K, field, steps, cuts)
        k, v, e = _split(steps, K, F)
        nk, c0 = len(steps), cuts[0]
        a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
        try:
            ta, tb = Placed(ctx, records, stride=length + 2, off=3), Placed(ctx, records)
            a.set_records(0, ta.view)
            b.set_records(0, tb.view)
            ctx.sync()
            ctx.set_timing(True)
            _drain(ctx)
            rows, nodes, index = a.write_key_segments(ta.view, k, v, field, cuts, expect=e)
            counts = _drain(ctx)
            ctx.set_timing(False)
            assert counts == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_fields": int(cond), "merkle_write_records": 1, "merkle_segments": 1,
                                                        "merkle_updates": depth + 1, "merkle_record_rows": 2, "sha256_records": 1}, cuts
            assert rows[0].shape == (nk, row_bytes(K, length, c0, F, cond)) and all(r.shape[0] == nk for r in rows[1:])
            for g, (got, want) in enumerate(zip(rows, want_rows)):
                assert got.shape == want.shape and np.array_equal(got, want), (cuts, g)
            assert np.array_equal(index, want_index) and np.array_equal(nodes, want_nodes)
            assert np.array_equal(nodes[:, -1, 0], want_roots[:-1]) and np.array_equal(nodes[:, -1, 1], want_roots[1:])
            ta.holds(model.records, cuts)
            _assert_tree(a, model.levels, cuts)
            # the uncut call's rows sliced are segment 0's
            urows, uindex, uroots = b.write_keys(tb.view, k, v, field, expect=e, roots=True)
            assert np.array_equal(uindex, index) and np.array_equal(uroots, want_roots)
            head = 64 + K + (2 * F if cond else F) + length
            for j in range(nk):
                low = int(index[j]) & ((1 << c0) - 1)
                want0 = np.concatenate([urows[j, : head + 32 * c0], np.frombuffer(low.to_bytes((c0 + 7) // 8, "little"), dtype=np.uint8)])
                assert np.array_equal(rows[0][j], want0), (cuts, j)
            tb2 = Placed(ctx, records)
            b.set_records(0, tb2.view)
            bits = b.write_key_segment_bits(tb2.view, k[:2], v[:2], field, cuts, expect=None if e is None else e[:2])[0]
            edges = [0] + cuts + [depth]
            assert [x.shape for x in bits] == [(2, 8 * head + 257 * c0)] + [(2, 1024 + 257 * (hi - lo)) for lo, hi in zip(edges[1:], edges[2:])]
            assert np.array_equal(np.packbits(bits[0], axis=1, bitorder="little"), want_rows[0][:2])
        finally:
            ctx.set_timing(False)
            a.close()
            b.close()


# ---------------------------------------------------------------------------------------------------------------- 2. a chain, a no-op, nk = 0, no rows
def test_a_key_five_times_expecting_what_the_batch_wrote(ctx, W):
    K, depth, length, field = 4, 2, 15, (9, 13)
    rng = np.random.default_rng(41100)
    a, b, c = _members(K, 3)
    records = _random_table(W, rng, [a, b, c], K, depth, length)
    m = WriteModel(records, K, field)
    vs = [rng.bytes(4) for _ in range(5)]
    chain = [(a, vs[0], m.field(m.own(a)))] + [(a, vs[j], vs[j - 1]) for j in range(1, 5)]
    steps = chain[:2] + [(b, m.field(m.own(b)), m.field(m.own(b)))] + chain[2:]  # in between: a no-op write on another key
    model = _check(ctx, records, K, field, steps, "five times", stride=length + 1, off=2)
    assert model.want[0].tolist() == [1, 1, 2, 1, 1, 1] and model.field(1) == vs[4] and model.records[2] == records[2]
    assert model.want[2][2] == model.want[2][3] and len(set(model.want[2])) == 6  # the no-op: R' = R
    for j in range(1, 5):
        assert m.status(a, chain[j][2]) == 5  # ... alone, against the table before the batch, every later link fails
    many = [(a, bytes([j] * 4)) if j % 3 else (b, bytes([j ^ 0xFF] * 4)) for j in range((1 << depth) + 5)]  # more steps than the table has slots
    _check(ctx, records, K, field, many, "more steps than slots", stride=length, off=1)


def test_nk_zero_and_no_rows(ctx, W):
    K, depth, length, field = 4, 3, 19, (9, 14)
    F = 5
    keys, records, plain = _every_key(W, field)
    for steps in (plain, _expecting(records, K, field, plain)):
        cond = _conditional(steps)
        model = WriteModel(records, K, field)
        before = model.root()
        want_index, want_rows, want_roots = model.write_batch(steps)
        tree = ctx.merkle_tree(depth)
        try:
            table = Placed(ctx, records, stride=length + 1, off=1)
            tree.set_records(0, table.view)
            ctx.sync()
            ctx.set_timing(True)
            _drain(ctx)
            assert ctx.lib.mfh_merkle_write_keys(ctx._h, tree._h, None, table.stride, length, K, 9, 14, 0, None, K, None, F, None, F, None, 0, None, None, None) == 0
            none, empty = np.zeros((0, K), dtype=np.uint8), np.zeros((0, F), dtype=np.uint8)
            rows0, index0, roots0 = tree.write_keys(table.view, none, empty, field, expect=empty if cond else None, roots=True)
            assert rows0.shape == (0, row_bytes(K, length, depth, F, cond)) and index0.shape == (0,) and roots0.tobytes() == before
            assert tree.write_bits(table.view, none, [], field)[0].shape == (0, 512 + 8 * (K + F) + 8 * length + 257 * depth)
            rows0, nodes0, index0 = tree.write_key_segments(table.view, none, empty, field, [1])
            assert [r.shape[0] for r in rows0] == [0, 0] and nodes0.shape == (0, 2, 2, 32)
            assert _drain(ctx) == dict.fromkeys(KINDS, 0)
            table.holds(records, "nk = 0")
            # h_inputs = NULL: the writes, no rows
            nk = len(steps)
            roots, index, status = np.zeros((nk + 1, 32), dtype=np.uint8), np.zeros(nk, dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
            assert _raw(ctx, tree, table, K, field, steps, None, roots, index, status) == 0
            assert np.array_equal(index, want_index) and (status == 0).all() and [r.tobytes() for r in roots] == want_roots
            assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_fields": int(cond), "merkle_write_records": 1, "sha256_records": 1,
                                                             "merkle_record_rows": 1, "merkle_updates": depth + 1}
            table.holds(model.records, "no rows")
            _assert_tree(tree, model.levels, "no rows")
        finally:
            ctx.set_timing(False)
            tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. alignment
def _field_shapes(K, length):
    """(field, what) of the sweep for records of `length` bytes"""
    lo = 2 * K
    shapes = {(lo, lo + 1): "the first payload byte", (length - 1, length): "the last byte", (lo, length): "the whole payload"}
    edge = 16 * (lo // 16 + 1)  # the first unit boundary behind the keys
    if lo < edge - 1 and edge + 2 <= length:
        shapes[(edge - 2, edge + 2)] = "across a 16-byte unit of the record"
    for F in (17, 33):  # one byte into the payload where the record has room, else (length = 2K + F) the whole payload
        at = lo + 1 if lo + 1 + F <= length else lo
        if at + F <= length:
            shapes[(at, at + F)] = f"F = {F}"
    return list(shapes.items())


@pytest.mark.parametrize("K", [1, 5, 7, 8, 32])
def test_alignment_sweep(ctx, W, K):
    depth = 3
    seen = set()
    for length in sorted({2 * K + 1, 2 * K + 17, 2 * K + 33, max(55, 2 * K + 3), max(56, 2 * K + 4)}):  # 2K + F for F = 1, 17 and 33 (the whole payload), 55 and 56
        rng = np.random.default_rng(41200 + 1000 * K + length)
        keys = [bytes([x]) for x in (0x10, 0x50, 0x51, 0x60, 0xFE)] if K == 1 else sorted({rng.bytes(K) for _ in range(6)})
        records = _random_table(W, rng, keys, K, depth, length, shuffle=True)
        for field, what in _field_shapes(K, length):
            F = field[1] - field[0]
            seen.add(what)
            # a key twice; whichever record is the table's last (its unit ends at the span's end) is somebody's or is gathered around
            plain = [(keys[0], rng.bytes(F)), (keys[1], rng.bytes(F)), (keys[2], bytes(F)), (keys[0], b"\xff" * F), (keys[3], rng.bytes(F)), (keys[4], rng.bytes(F)),
                     (keys[-1], rng.bytes(F))]
            _check(ctx, records, K, field, plain, (K, length, field, what, "plain"), stride=length + 5, off=1)
            steps, model = _expecting(records, K, field, plain), None
            for stride, off in ((length, 3), (length + 5, 1), (length + 5, 2)):  # with expectations both kernels run: the gather and the build
                model = _check(ctx, records, K, field, steps, (K, length, field, what, stride, off), model=model, stride=stride, off=off)
    assert seen == {"the first payload byte", "the last byte", "the whole payload", "across a 16-byte unit of the record", "F = 17", "F = 33"}


# ---------------------------------------------------------------------------------------------------------------- 4. batch sizes
@pytest.fixture(scope="module")
def depth_10(W):
    depth, K, length = 10, 8, 55
    rng = np.random.default_rng(41300)
    members = sorted({rng.bytes(K) for _ in range(500)})
    return members, _random_table(W, rng, members, K, depth, length, shuffle=True)


@pytest.mark.parametrize("nk", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_depth_10(ctx, depth_10, nk):
    K, length, field = 8, 55, (16, 24)
    members, records = depth_10
    rng = np.random.default_rng(41300 + nk)
    some = [members[int(i)] for i in rng.permutation(len(members))[:40]]
    plain = [(some[int(rng.integers(0, 40))], rng.bytes(8)) for _ in range(nk)]
    steps = plain if nk % 2 else _expecting(records, K, field, plain)  # expectations that mostly only the batch satisfies
    _check(ctx, records, K, field, steps, nk, stride=length + 1, off=2)


# ---------------------------------------------------------------------------------------------------------------- 5. two chunks
def test_two_chunks(ctx, W):
    depth, K, length = 2, 4, 1 << 19
    field = (length - 8, length)
    rowb = row_bytes(K, length, depth, 8, True)
    per_chunk = (64 << 20) // rowb
    nk = per_chunk + 1
    assert per_chunk == 127 and nk == 128
    rng = np.random.default_rng(41400)
    keys = _members(K, 3)
    records = _random_table(W, rng, keys, K, depth, length, shuffle=True)
    plain = [(keys[j % 3], rng.bytes(8)) for j in range(nk - 2)] + [(keys[0], rng.bytes(8)), (keys[0], rng.bytes(8))]  # steps 126 and 127, on both sides of the seam
    steps = _expecting(records, K, field, plain)  # 127 expects what 126 wrote
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        rc, rows, roots, index, status = _write(ctx, tree, table, K, field, steps)
        counts = {kind: ctx.timing_drain(kind)[::2] for kind in KINDS}
        ctx.set_timing(False)
        assert rc == 0 and (status == 0).all(), ctx.lib.mfh_last_error(ctx._h).decode()
        assert counts == dict.fromkeys(KINDS, (0, 0)) | {"merkle_locate": (1, 1 << depth), "merkle_fields": (1, 3), "merkle_write_records": (1, nk), "sha256_records": (2, nk),
                                                         "merkle_record_rows": (4, nk), "merkle_updates": (2 * (depth + 1), nk * depth)}
        model = WriteModel(records, K, field)
        want_index, want_rows, want_roots = model.write_batch(steps)
        assert np.array_equal(index, want_index) and [r.tobytes() for r in roots] == want_roots and np.array_equal(rows, want_rows)
        table.holds(model.records, "two chunks")
        _assert_tree(tree, model.levels, "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. failures
def test_statuses_leave_everything_as_it_was(ctx, W, mf):
    depth, K, length, field = 3, 2, 9, (5, 8)
    rng = np.random.default_rng(41500)
    a, b, c, ghost = (_key(x, K) for x in (0x1000, 0x2000, 0x7000, 0x6000))
    records = _random_table(W, rng, [a, b, c], K, depth, length)  # slots 1, 2, 3
    records[5] = ghost + ghost + records[5][2 * K:]  # the lo of an inert record alone: no member
    model = WriteModel(records, K, field)
    fa, fb, fc = (model.field(i) for i in (1, 2, 3))
    x, y = b"\x01\x02\x03", b"\xf1\xf2\xf3"
    assert len({fa, fb, fc, x, y}) == 5
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        cases = [("a key that is no member", [(a, x, fa), (ghost, x, x), (c, y, fc)], [1, NONE, 3], [0, 1, 0], "not a member", 1),
                 ("a key that is no member, plain", [(a, x), (b, y), (ghost, x), (a, y)], [1, 2, NONE, 1], [0, 0, 1, 0], "not a member", 0),
                 ("a failed expectation at the third step", [(a, x, fa), (b, y, fb), (c, x, y), (c, x, fc)], [1, 2, 3, 3], [0, 0, 5, 0], "not what was expected", 1),
                 ("an expectation an earlier step has overwritten", [(a, x, fa), (b, y, fb), (a, y, fa), (a, y, x)], [1, 2, 1, 1], [0, 0, 5, 0], "not what was expected", 1)]
        texts = set()
        for what, steps, want_i, want_s, word, fields in cases:
            m_index, m_status = model.statuses(steps)
            assert m_status.tolist() == want_s and m_index.tolist() == want_i, what
            rc, rows, roots, index, status = _write(ctx, tree, table, K, field, steps)
            text = ctx.lib.mfh_last_error(ctx._h).decode()
            assert rc == EINVAL and text.startswith("mfh_merkle_write_keys: ") and word in text and f"h_status {max(want_s)}" in text, (what, rc, text)
            texts.add(text)
            assert status.tolist() == want_s and index.tolist() == want_i, (what, status, index)
            assert not rows.any() and not roots.any(), what
            assert _drain(ctx) == dict.fromkeys(KINDS, 0) | {"merkle_locate": 1, "merkle_fields": fields}, what
            table.holds(records, what)
            _assert_tree(tree, model.levels, what)
            assert tree.root() == model.root()
        assert len(texts) == 2  # one text a status
        assert model.status(a, fa) == 0  # (the stale expectation is one the table met before the batch)
        ctx.set_timing(False)
        with pytest.raises(mf.MfhError) as e:
            tree.write_keys(table.view, _keys([a], K), [x], field, expect=[y])
        assert "mfh_merkle_write_keys: a field is not what was expected" in str(e.value)
        with pytest.raises(mf.MfhError) as e:
            tree.write_key_segments(table.view, _keys([ghost], K), [x], field, [1])
        assert "mfh_merkle_write_keys_cut: a key is not a member" in str(e.value)
        table.holds(records, "after the refused calls")
        rc, rows, roots, index, status = _write(ctx, tree, table, K, field, [(b, x, fb), (b, y, x)])
        assert rc == 0 and index.tolist() == [2, 2] and status.tolist() == [0, 0]
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals, launch counts
def test_einval_up_front(ctx, mf, W):
    lib, h = ctx.lib, ctx._h
    depth, K, length, field = 3, 4, 17, (10, 13)
    F = 3
    rng = np.random.default_rng(41600)
    keys = sorted({rng.bytes(K) for _ in range(5)})
    records = _random_table(W, rng, keys, K, depth, length)
    model = WriteModel(records, K, field)
    rowb = row_bytes(K, length, depth, F, True)
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
        v, e = np.full((3, F), 7, dtype=np.uint8), np.stack([np.frombuffer(model.field(model.own(x)), dtype=np.uint8) for x in keys[0:3]])
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((4, 32), 0xAB, dtype=np.uint8)
        index, status = np.full(3, 0xCDCDCDCD, dtype=np.uint32), np.full(3, 0xCD, dtype=np.uint8)
        kp, zp, op, vp_, ep, bp, rp, ip, sp = (vp(x.ctypes.data) for x in (k, zero, ones, v, e, buf, roots, index, status))
        tp, ts, stride = vp(table.view.data_ptr()), table.stride, buf.shape[1]
        cut = np.array([1], dtype=np.uint32)
        seg0, seg1 = np.full((3, row_bytes(K, length, 1, F, True) + 2), 0xAB, dtype=np.uint8), np.full((3, 128 + 64 + 1), 0xAB, dtype=np.uint8)
        ptrs = (ctypes.c_void_p * 2)(seg0.ctypes.data, seg1.ctypes.data)
        strides = (ctypes.c_size_t * 2)(seg0.shape[1], seg1.shape[1])
        short = (ctypes.c_size_t * 2)(seg0.shape[1] - 3, seg1.shape[1])
        cp = vp(cut.ctypes.data)

        def plain(t_, table_p, table_s, length_, K_, lo, hi, nk, keys_p, key_s, values_p, value_s, expect_p, expect_s, rows_p, in_s, index_p, status_p, handle=h):
            return lib.mfh_merkle_write_keys(handle, t_, table_p, table_s, length_, K_, lo, hi, nk, keys_p, key_s, values_p, value_s, expect_p, expect_s, rows_p, in_s, rp, index_p, status_p)

        def cut_call(t_, table_p, table_s, length_, K_, lo, hi, nk, keys_p, key_s, values_p, value_s, expect_p, expect_s, rows_p, in_s, index_p, status_p, handle=h, cuts=cp, st=strides):
            return lib.mfh_merkle_write_keys_cut(handle, t_, table_p, table_s, length_, K_, lo, hi, nk, keys_p, key_s, values_p, value_s, expect_p, expect_s, 1, cuts, ptrs, st, rp, index_p,
                                                 status_p)

        for who, g in (("mfh_merkle_write_keys", plain), ("mfh_merkle_write_keys_cut", cut_call)):
            texts = []

            def refused(rc, handle=h):
                assert rc == EINVAL, who
                text = lib.mfh_last_error(handle).decode()
                assert text.startswith(who + ": "), text
                texts.append(text)

            ok = (tree._h, tp, ts, length, K, field[0], field[1], 3, kp, K, vp_, F, ep, F, bp, stride, ip, sp)

            def but(**changes):
                names = ("tree", "table", "ts", "length", "K", "lo", "hi", "nk", "k", "ks", "v", "vs", "e", "es", "rows", "in_s", "index", "status")
                return tuple(changes.get(n, x) for n, x in zip(names, ok))

            refused(g(*but(tree=None)))
            refused(g(*but(K=0)))
            refused(g(*but(K=33, length=80, ks=33, lo=70, hi=73, in_s=1 << 12)))
            texts.pop()  # (key_bytes 0 and 33: one text)
            refused(g(*but(length=2 * K - 1)))
            refused(g(*but(ts=length - 1)))
            refused(g(*but(ks=K - 1)))
            refused(g(*but(lo=2 * K - 1)))  # the keys are not writable
            refused(g(*but(lo=0, hi=F)))
            texts.pop()  # (one text)
            refused(g(*but(hi=field[0])))  # an empty field
            refused(g(*but(lo=field[1], hi=field[0])))
            texts.pop()  # (one text)
            refused(g(*but(lo=length - 2, hi=length + 1)))
            refused(g(*but(vs=F - 1)))
            refused(g(*but(es=F - 1)))
            for name in ("table", "k", "v", "index", "status"):
                refused(g(*but(**{name: None})))
            refused(g(*but(k=zp)))
            refused(g(*but(k=op)))
            texts.pop()  # (the two sentinels: one text)
            if g is plain:
                refused(g(*but(in_s=rowb - 1)))
                assert "64 + key_bytes" in texts[-1]
                refused(g(*but(e=None, es=0, in_s=rowb - F - 1)))  # plain rows are F bytes shorter (expect_stride is then ignored)
                texts.pop()
                refused(g(*but(rows=None, in_s=0, k=zp)))  # no rows: a sentinel is refused too
                texts.pop()
            else:
                refused(g(*ok, st=short))
                refused(g(*ok, cuts=None))
            assert g(*ok, handle=None) == EINVAL
            assert len(set(texts)) == len(texts) == (17 if g is plain else 18), sorted(texts)
        assert cut_call(*but(nk=0)) == 0
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xAB).all() and (index == 0xCDCDCDCD).all() and (status == 0xCD).all() and (seg0 == 0xAB).all() and (seg1 == 0xAB).all()
        assert _drain(ctx) == dict.fromkeys(KINDS, 0)
        ctx.set_timing(False)
        vals = [b"abc"] * 3
        for bad in [(k[0], vals, field, None), (k, vals[:2], field, None), (k, [b"ab"] * 3, field, None), (k, [b"abc", b"ab", b"abcd"], field, None), (zero, vals, field, None),
                    (k, vals, field, vals[:2]), (k, vals, field, [b"abcd"] * 3), (k, vals, (7, 10), None), (k, vals, (10, 10), None), (k, vals, (15, 18), None), (k, vals, (10.0, 13), None),
                    (k, vals, 10, None), (k, np.zeros((3, F), dtype=np.uint16), field, None)]:
            for call in (lambda *x: tree.write_keys(table.view, x[0], x[1], x[2], expect=x[3]), lambda *x: tree.write_key_segments(table.view, x[0], x[1], x[2], [1], expect=x[3])):
                with pytest.raises(mf.MfhError):
                    call(*bad)
        for cuts in ([], [0], [3], [2, 1]):
            with pytest.raises(mf.MfhError):
                tree.write_key_segments(table.view, k, vals, field, cuts)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
    finally:
        ctx.set_timing(False)
        tree.close()


@pytest.mark.parametrize("conditional", [False, True])
def test_launch_counts_and_stride(ctx, depth_10, conditional):
    depth, K, length, nk, field = 10, 8, 55, 100, (16, 24)
    members, records = depth_10
    rng = np.random.default_rng(41700)
    plain = [(members[int(rng.integers(0, 30))], rng.bytes(8)) for _ in range(nk)]
    steps = _expecting(records, K, field, plain) if conditional else plain
    nu = len({s[0] for s in steps})
    model = WriteModel(records, K, field)
    want_index, want_rows, want_roots = model.write_batch(steps)
    rowb = row_bytes(K, length, depth, 8, conditional)
    assert rowb == 64 + 8 + (16 if conditional else 8) + 55 + 320 + 2
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        _drain(ctx)
        buf = np.full((nk, rowb + 13), 0xAB, dtype=np.uint8)
        index, status = np.zeros(nk, dtype=np.uint32), np.full(nk, 7, dtype=np.uint8)
        assert _raw(ctx, tree, table, K, field, steps, buf, None, index, status, in_stride=buf.shape[1]) == 0  # a wider in_stride, no roots
        assert np.array_equal(buf[:, :rowb], want_rows) and (buf[:, rowb:] == 0xAB).all() and np.array_equal(index, want_index)
        timed = {kind: ctx.timing_drain(kind) for kind in KINDS}
        want = {"merkle_locate": (1, 1 << depth), "merkle_write_records": (1, nk), "sha256_records": (1, nk), "merkle_record_rows": (2, nk), "merkle_updates": (depth + 1, nk * depth)}
        if conditional:
            want["merkle_fields"] = (1, nu)
        assert {k: (v[0], v[2]) for k, v in timed.items()} == dict.fromkeys(KINDS, (0, 0)) | want  # one search, at most one gather, one build launch; per chunk as adjust_keys
        print(f"depth {depth}: {nk} writes: " + ", ".join(f"{k} {v[1]:.3f} ms" for k, v in timed.items() if v[0]))
        table.holds(model.records, "rows")
        ctx.set_timing(False)
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        k, v, e = _split(steps, K, 8)
        bits, index3 = tree.write_bits(table.view, k[:3], [bytes(x) for x in v[:3]], field, expect=None if e is None else [bytes(x) for x in e[:3]])  # bytes-likes
        assert bits.shape == (3, 8 * (rowb - 322) + 257 * depth) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows[:3])
        assert np.array_equal(index3, want_index[:3])
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. streams, staging
def _late_table(ctx, W):
    depth, K, length, nk, field = 9, 4, 24, 64, (11, 20)
    rng = np.random.default_rng(41800)
    members = sorted({rng.bytes(K) for _ in range(300)})
    records = _random_table(W, rng, members, K, depth, length, shuffle=True)
    steps = _expecting(records, K, field, [(members[int(rng.integers(0, 20))], rng.bytes(9)) for _ in range(nk)])
    model = WriteModel(records, K, field)
    want_index, want_rows, want_roots = model.write_batch(steps)  # (first: nothing of the host's stands between the late table and the calls)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        k, v, e = _split(steps, K, 9)
        rows, index, roots = tree.write_keys(table.view, k, v, field, expect=e, roots=True)
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


def test_the_same_after_scrub_staging(ctx, W):
    K, depth, length, field = 4, 3, 19, (9, 14)
    keys, records, plain = _every_key(W, field)
    steps = _expecting(records, K, field, plain + plain[::-1])
    model = WriteModel(records, K, field)
    want_index, want_rows, want_roots = model.write_batch(steps)
    tree = ctx.merkle_tree(depth)
    try:
        for scrub in (False, True):  # the pinned staging zeroed between two identical calls: the same rows from the same starting table
            table = Placed(ctx, records, stride=length + 1)
            tree.set_records(0, table.view)
            if scrub:
                assert ctx.scrub_staging() == 0
            rc, rows, roots, index, status = _write(ctx, tree, table, K, field, steps)
            assert rc == 0 and np.array_equal(rows, want_rows) and np.array_equal(index, want_index) and [r.tobytes() for r in roots] == want_roots
            table.holds(model.records, scrub)
        assert ctx.scrub_staging() == 0
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. neighbours
def test_neighbours(ctx, W):
    depth, K, A, length, field = 6, 8, 8, 55, (24, 40)  # the balance is bytes [16, 24): the field lies behind it
    rng = np.random.default_rng(41900)
    members = sorted({rng.bytes(K) for _ in range(40)})
    records = _random_table(W, rng, members, K, depth, length, shuffle=True)
    model = WriteModel(records, K, field)
    plain = [(members[int(rng.integers(0, 40))], rng.bytes(16)) for _ in range(50)]
    steps = _expecting(records, K, field, plain)
    want_index, want_rows, want_roots = model.write_batch(steps)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1)
        tree.set_records(0, table.view)
        supply = tree.total_balance(table.view, K, A)
        assert tree.check_table(table.view, K) == (0, 41, None)
        k, v, e = _split(steps, K, 16)
        rows, index = tree.write_keys(table.view, k, v, field, expect=e)
        assert np.array_equal(rows, want_rows) and np.array_equal(index, want_index)
        assert tree.total_balance(table.view, K, A) == supply  # the writes lie outside the balance
        assert tree.check_table(table.view, K) == (0, 41, None) == W.indexed_check(np.stack([np.frombuffer(r, dtype=np.uint8) for r in model.records]), K)
        table.holds(model.records, "neighbours")
        # a write on a pair that grow made
        grown, wide = tree.grow(depth + 2, table.view)
        try:
            big = WriteModel([bytes(r) for r in W.indexed_grow(np.stack([np.frombuffer(r, dtype=np.uint8) for r in model.records]), depth + 2)], K, field)
            more = _expecting(big.records, K, field, [(members[int(rng.integers(0, 40))], rng.bytes(16)) for _ in range(20)])
            g_index, g_rows, g_roots = big.write_batch(more)
            k, v, e = _split(more, K, 16)
            rows, index, roots = grown.write_keys(wide, k, v, field, expect=e, roots=True)
            assert np.array_equal(rows, g_rows) and np.array_equal(index, g_index) and [r.tobytes() for r in roots] == g_roots
            assert [bytes(r) for r in wide.cpu().numpy()] == big.records
            _assert_tree(grown, big.levels, "grown")
            assert grown.check_table(wide, K) == (0, 41, None)
        finally:
            grown.close()
        table.holds(model.records, "the old pair is only read")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 10. end to end
A_KEY, B_KEY, C_KEY = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("c1aa557f")
FIELD = (8, 16)
V1, V2, V3 = bytes.fromhex("0102030405060708"), bytes.fromhex("f0e0d0c0b0a09080"), bytes.fromhex("00000000ffffffff")


def _e2e_steps(records):
    m = WriteModel(records, 4, FIELD)
    return [(A_KEY, V1, m.field(m.own(A_KEY))), (A_KEY, V2, V1), (C_KEY, V3, m.field(m.own(C_KEY)))]  # A, A again expecting the first value, C


def _rejected(st, pair, step):
    """the statements a proof of (pair, step) must NOT verify against: a flipped value bit, a flipped expected bit, another key, the two roots swapped"""
    key, v, e = step
    flip = lambda x, bit: bytes(b ^ (1 << (bit % 8)) if j == bit // 8 else b for j, b in enumerate(x))  # noqa: E731
    return [st.statement(*pair, key, e, flip(v, 9)), st.statement(*pair, key, flip(e, 62), v), st.statement(*pair, B_KEY, e, v), st.statement(pair[1], pair[0], key, e, v)]


def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p = mf.Params(d=1 << 19, m=349525)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    K, length, depth = 4, 16, 2
    st = W.MerkleWrite(K, length, depth, FIELD, expect=True)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == st.lu == 672 and (cc.nwires, cc.nrows) == W.MERKLE_WRITE_SIZES[(K, length, depth, FIELD, True)]
    rng = np.random.default_rng(42300)
    records = _random_table(W, rng, [A_KEY, B_KEY, C_KEY], K, depth, length)
    steps = _e2e_steps(records)
    model = WriteModel(records, K, FIELD)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        k, v, e = _split(steps, K, 8)
        bits, index, roots = tree.write_bits(table.view, k, v, FIELD, expect=e, roots=True)
        want_index, want_rows, want_roots = model.write_batch(steps)
        assert bits.shape == (3, st.nin) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows) and index.tolist() == want_index.tolist() == [1, 1, 3]
        assert [r.tobytes() for r in roots] == want_roots and len(set(want_roots)) == 4
        table.holds(model.records, "end to end")
        assert (model.field(1), model.field(3)) == (V2, V3)
    finally:
        tree.close()
    pairs = list(zip(want_roots, want_roots[1:]))
    wrong = st.bits(A_KEY, V1, V3, records[1], WriteModel(records, K, FIELD).siblings(1), 1)  # a fourth row whose expectation the table as it first stood does not meet
    prog = ctx.circuit_load(cc, state="auto")
    try:
        witness, holds = ctx.circuit_assign(prog, np.stack(list(bits) + [wrong]))
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
    own = [st.statement(*pairs[j], steps[j][0], steps[j][2], steps[j][1]) for j in range(3)]
    assert all(len(x) == lu // 8 for x in own) and own == [witness[j][: lu // 8].tobytes() for j in range(3)]
    assert verify(proofs, own) == [True] * 3
    for which in range(4):
        assert verify(proofs, [_rejected(st, pairs[j], steps[j])[which] for j in range(3)]) == [False] * 3, which
    print(f"test_end_to_end_proofs (MerkleWrite(4, 16, 2, (8, 16), expect=True), d = 2^19): {time.time() - t0:.1f} s")


def test_end_to_end_cut_writes(gpu_ctx_factory, mf, W):
    t0 = time.time()
    p18, p17 = mf.Params(d=1 << 18, m=174762), mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p18)
    ctx.set_seed(SEED)
    K, length, depth, cuts = 4, 16, 2, [1]
    st, seg = W.MerkleWrite(K, length, 1, FIELD, expect=True), W.MerkleSegment(1)
    cc = st.circuit.compile(p18)
    assert cc.lu == st.lu == 672 and (cc.nwires, cc.nrows) == W.MERKLE_WRITE_SIZES[(K, length, 1, FIELD, True)]
    rng = np.random.default_rng(42400)
    records = _random_table(W, rng, [A_KEY, B_KEY, C_KEY], K, depth, length)
    steps = _e2e_steps(records)
    want_rows, want_nodes, want_index, want_roots, model = write_cut_batch(records, K, FIELD, steps, cuts)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=3)
        tree.set_records(0, table.view)
        k, v, e = _split(steps, K, 8)
        bits, nodes, index = tree.write_key_segment_bits(table.view, k, v, FIELD, cuts, expect=e)
        table.holds(model.records, "end to end")
    finally:
        tree.close()
    assert index.tolist() == [1, 1, 3] and np.array_equal(nodes, want_nodes)
    assert all(np.array_equal(np.packbits(b, axis=1, bitorder="little"), w) for b, w in zip(bits, want_rows))
    # the verifier's side: statements from the returned nodes alone
    pub = [[(nodes[j, g, 0].tobytes(), nodes[j, g, 1].tobytes()) for g in range(2)] for j in range(3)]
    assert [x[1] for x in pub] == [(want_roots[j].tobytes(), want_roots[j + 1].tobytes()) for j in range(3)]
    own = [st.statement(*pub[j][0], steps[j][0], steps[j][2], steps[j][1]) for j in range(3)]
    witness = _witnesses(ctx, cc, bits[0])
    assert [st.roots_of(witness[j]) for j in range(3)] == [x[0] for x in pub] and own == [witness[j][: st.lu // 8].tobytes() for j in range(3)]
    prove, verify = _prover(ctx, p18, cc, rng, 3)
    proofs = prove(witness)
    assert verify(proofs, own) == [True] * 3
    for which in range(4):
        assert verify(proofs, [_rejected(st, pub[j][0], steps[j])[which] for j in range(3)]) == [False] * 3, which

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
    print(f"test_end_to_end_cut_writes (MerkleWrite(4, 16, 1, (8, 16), True) at d = 2^18, three MerkleSegment(1) at d = 2^17): {time.time() - t0:.1f} s")
