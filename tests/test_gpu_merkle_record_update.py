"""GPU: batches of sequential record updates of a device table and its tree (mfh_merkle_update_records, MerkleTree.update_records / update_record_bits)
against a sequential model in this file: a list of records, leaves from hashlib.sha256, and tests/test_gpu_merkle_update.py's Model walking
tests/sha256_ref.py's merkle_parent (memoised in tests/test_gpu_merkle.py).

Every check of a batch compares the rows byte for byte against MerkleRecordUpdate(length, depth).bits, all n + 1 roots, every node of the tree, and the
whole allocation the table lives in afterwards: the table sits inside a larger uint8 tensor filled with 0xA5, so the bytes before it, in the gaps of a
wider stride and behind its last record are compared too.

1. hand-made collisions at depth 1, 2, 3 x lengths 1, 55: test_gpu_merkle_update.py's batches (single, one index three times, 2j then 2j + 1 and the
   reverse, cousins), each on a fresh table and all in a row.
2. alignment sweep at depth 3 with 257 updates (8 records: every collision, a second workgroup), lengths 1, 3, 16, 17, 55, 56, 64, 65, 119: table and new
   records each start 0, 1, 2, 3 bytes into a larger tensor (all 16 pairs: source and destination shifts of the table store are independent), at strides
   length and length + 5.  The model runs once per length; alignment does not enter it.
3. random batches: depth 9 with 300 updates, depth 12 with 64, length 55.
4. a wider in_stride keeps its tail bytes; "merkle_updates" counts depth + 1, "sha256_records" 1 with rows = updates, "merkle_record_rows" 2 with rows =
   updates, "merkle_level" 0; h_roots = NULL and scrubbed staging give the same rows.
5. two chunks: depth 1, length 65 521, 520 updates: a row is 131 139 bytes, a chunk 511 updates; both leaves are hit on both sides of the seam.
6. after a batch, a second tree built by set_records(0, table) has the same nodes.
7. end to end at d = 2^18 with MerkleRecordUpdate(55, 1, frozen=(0, 8)): five sequential updates that keep bytes [0, 8) hold with roots_of = (R_k, R_k+1),
   violate no row, and their proofs verify under statement(R_k, R_k+1) and under neither the neighbour's statement nor the roots swapped; a sixth row
   whose new record changes byte 0 does not hold and violates a row; a table overwritten behind the tree's back gives an old root that is not R_k.
8. every MFH_EINVAL case leaves the nodes, the table's bytes and the timing counts as they were; nupd = 0 does nothing.
9. new records as numpy and as a device tensor, the table as a column slice of a wider tensor; table and new records produced late on the stream, on the
   null stream and on a caller's stream.

MerkleRecordUpdate.bits reads the length and the depth alone; it is called on a stand-in holding the two (building the statement's circuit takes seconds
for nothing) -- the depth-1 case of test 1 checks that the stand-in and the statement give the same bits."""
import ctypes
import hashlib
import types

import numpy as np
import pytest

from test_gpu_merkle import _assert_tree, _late, _parent
from test_gpu_merkle_update import Model, _hand_made

pytestmark = pytest.mark.gpu

SEED = bytes((37 * i + 11) & 0xFF for i in range(40))
EINVAL = -1
FILL = 0xA5


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


# ---------------------------------------------------------------------------------------------------------------- the reference side
def _row_bytes(length, depth):
    return 64 + 2 * length + 32 * depth + (depth + 7) // 8


def _bits(length, depth, old, new, sibs, index):
    from c_lwe_snarks_amd import words

    return words.MerkleRecordUpdate.bits(types.SimpleNamespace(length=length, depth=depth), old, new, sibs, index)


def _records(rng, n, length):
    return [rng.bytes(length) for _ in range(n)]


class RecordModel(Model):
    """a list of records and the tree over their SHA-256 digests, updated one record at a time"""

    def __init__(self, records):
        self.records = [bytes(r) for r in records]
        self.length = len(self.records[0])
        super().__init__([hashlib.sha256(r).digest() for r in self.records])

    def update(self, i, new):
        """(the MerkleRecordUpdate input row before the update, packed; the root after it)"""
        sibs = [self.levels[l][(i >> l) ^ 1] for l in range(self.depth)]
        row = np.packbits(_bits(self.length, self.depth, self.records[i], new, sibs, i), bitorder="little")
        self.records[i] = bytes(new)
        cur = self.levels[0][i] = hashlib.sha256(new).digest()
        for l in range(self.depth):
            j = i >> l
            cur = _parent(sibs[l], cur) if j & 1 else _parent(cur, sibs[l])
            self.levels[l + 1][j >> 1] = cur
        return row, cur

    def batch(self, indices, new_records):
        """(packed rows [n, row bytes], roots [n + 1] as bytes)"""
        roots, rows = [self.root()], []
        for i, new in zip(indices, new_records):
            row, root = self.update(int(i), new)
            rows.append(row)
            roots.append(root)
        rows = np.stack(rows) if rows else np.zeros((0, _row_bytes(self.length, self.depth)), dtype=np.uint8)
        assert rows.shape[1] == _row_bytes(self.length, self.depth)
        return rows, roots


class Placed:
    """n records of one length inside a larger uint8 device tensor filled with 0xA5: `view` is the [n, length] tensor at `stride`, starting 32 + off bytes
    into `whole`, with 32 more bytes behind the last record; image(records) is what the allocation must hold when the records are `records`"""

    def __init__(self, ctx, records, stride=None, off=0, late=False):
        self.n, self.length = len(records), len(records[0])
        self.stride = self.length if stride is None else stride
        self.start = 32 + off
        img = self.image(records)
        self.whole = _late(ctx, img.tobytes()) if late else ctx.to_device(img)
        assert self.whole.data_ptr() % 16 == 0
        self.view = self.whole.as_strided((self.n, self.length), (self.stride, 1), self.start)

    def image(self, records):
        img = np.full(self.start + (self.n - 1) * self.stride + self.length + 32, FILL, dtype=np.uint8)
        for i, r in enumerate(records):
            at = self.start + i * self.stride
            img[at: at + self.length] = np.frombuffer(bytes(r), dtype=np.uint8)
        return img

    def holds(self, records, what=""):
        assert np.array_equal(self.whole.cpu().numpy(), self.image(records)), what


def _check_against(tree, table, new_data, indices, want_rows, want_roots, levels, records, what):
    """one update_records call against a model's results: rows, roots, every node, the table's whole allocation"""
    rows, roots = tree.update_records(table.view, indices, new_data, roots=True)
    assert rows.dtype == np.uint8 and rows.shape == want_rows.shape, what
    assert np.array_equal(rows, want_rows), what
    assert roots.shape == (len(indices) + 1, 32) and [r.tobytes() for r in roots] == want_roots, what
    _assert_tree(tree, levels, what)
    table.holds(records, what)


def _check_batch(tree, model, table, indices, new_records, what, new_data=None):
    want_rows, want_roots = model.batch(indices, new_records)
    if new_data is None:
        new_data = np.stack([np.frombuffer(r, dtype=np.uint8) for r in new_records])
    _check_against(tree, table, new_data, indices, want_rows, want_roots, model.levels, model.records, what)


# ---------------------------------------------------------------------------------------------------------------- 1. hand-made collisions
@pytest.mark.parametrize("length", [1, 55])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_hand_made_batches(ctx, W, depth, length):
    rng = np.random.default_rng(9900 + 100 * depth + length)
    records = _records(rng, 1 << depth, length)
    if depth == 1:  # the stand-in gives what the statement gives
        args = (records[0], records[1], [rng.bytes(32)], 1)
        assert np.array_equal(_bits(length, 1, *args), W.MerkleRecordUpdate(length, 1).bits(*args))
    tree = ctx.merkle_tree(depth)
    try:
        # each batch on a fresh table and tree, then all of them one after the other on one table
        for what, indices in _hand_made(depth):
            table = Placed(ctx, records, stride=length + 3, off=1)
            tree.set_records(0, table.view)
            _check_batch(tree, RecordModel(records), table, indices, _records(rng, len(indices), length), (depth, length, what))
        table = Placed(ctx, records)
        tree.set_records(0, table.view)
        model = RecordModel(records)
        for what, indices in _hand_made(depth):
            _check_batch(tree, model, table, indices, _records(rng, len(indices), length), (depth, length, "in a row", what))
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. alignment sweep
@pytest.mark.parametrize("length", [1, 3, 16, 17, 55, 56, 64, 65, 119])
def test_alignment_sweep(ctx, length):
    depth, nupd = 3, 257
    rng = np.random.default_rng(10000 + length)
    records = _records(rng, 8, length)
    indices = [int(x) for x in rng.integers(0, 8, size=nupd)]
    assert set(indices) == set(range(8))
    new = _records(rng, nupd, length)
    model = RecordModel(records)
    want_rows, want_roots = model.batch(indices, new)  # once: the alignment does not enter it
    tree = ctx.merkle_tree(depth)
    try:
        for stride in (length, length + 5):
            for t_off in range(4):
                for n_off in range(4):
                    table = Placed(ctx, records, stride=stride, off=t_off)
                    fresh = Placed(ctx, new, stride=stride, off=n_off)
                    assert table.view.data_ptr() % 4 == t_off and fresh.view.data_ptr() % 4 == n_off
                    tree.set_records(0, table.view)
                    what = (length, stride, t_off, n_off)
                    _check_against(tree, table, fresh.view, indices, want_rows, want_roots, model.levels, model.records, what)
                    fresh.holds(new, what)  # the new records are only read
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. random batches
@pytest.mark.parametrize("depth,nupd", [(9, 300), (12, 64)])
def test_random_batches(ctx, depth, nupd):
    length = 55
    rng = np.random.default_rng(10100 + depth)
    records = _records(rng, 1 << depth, length)
    # heavy repeats: half of the draws come from 8 records that include two sibling pairs
    hot = [0, 1, 6, 7] + [int(x) for x in rng.integers(0, 1 << depth, size=4)]
    indices = [hot[int(rng.integers(0, 8))] if rng.integers(0, 2) else int(rng.integers(0, 1 << depth)) for _ in range(nupd)]
    assert len(set(indices)) < nupd
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 9, off=3)
        tree.set_records(0, table.view)
        _check_batch(tree, RecordModel(records), table, indices, _records(rng, nupd, length), (depth, nupd))
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. stride and launches
def test_wider_stride_and_launch_counts(ctx):
    depth, nupd, length = 9, 300, 55
    rng = np.random.default_rng(10200)
    records = _records(rng, 1 << depth, length)
    indices = [int(x) for x in rng.integers(0, 24, size=nupd)]
    new = _records(rng, nupd, length)
    model = RecordModel(records)
    want_rows, want_roots = model.batch(indices, new)
    rowb = _row_bytes(length, depth)
    assert rowb == 464
    stride = rowb + 13
    buf = np.full((nupd, stride), 0xAB, dtype=np.uint8)
    roots = np.full((nupd + 1, 32), 0xCD, dtype=np.uint8)
    iu = np.array(indices, dtype=np.uint32)
    fresh = Placed(ctx, new)
    tree = ctx.merkle_tree(depth)
    vp = ctypes.c_void_p

    def call(table, out, out_stride, h_roots):
        return ctx.lib.mfh_merkle_update_records(ctx._h, tree._h, nupd, vp(iu.ctypes.data), vp(table.view.data_ptr()), table.stride, length,
                                                 vp(fresh.view.data_ptr()), fresh.stride, vp(out.ctypes.data), out_stride, h_roots)

    try:
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        for kind in ("merkle_level", "sha256_records", "merkle_updates", "merkle_record_rows"):
            ctx.timing_drain(kind)
        assert call(table, buf, stride, vp(roots.ctypes.data)) == 0
        launches, ms, rows = ctx.timing_drain("merkle_updates")
        assert (launches, rows) == (depth + 1, nupd * depth)
        h_launches, h_ms, h_rows = ctx.timing_drain("sha256_records")
        assert (h_launches, h_rows) == (1, nupd)
        c_launches, c_ms, c_rows = ctx.timing_drain("merkle_record_rows")
        assert (c_launches, c_rows) == (2, nupd)
        print(f"depth {depth}: {nupd} record updates: tree {ms:.3f} ms, hash {h_ms:.3f} ms, gather + table store {c_ms:.3f} ms")
        assert ctx.timing_drain("merkle_level")[0] == 0
        ctx.set_timing(False)
        assert np.array_equal(buf[:, :rowb], want_rows)
        assert (buf[:, rowb:] == 0xAB).all()
        assert [r.tobytes() for r in roots] == want_roots
        _assert_tree(tree, model.levels, "wider stride")
        table.holds(model.records, "wider stride")
        # h_roots = NULL, and the pinned staging zeroed between two calls: the same rows from the same starting table
        table = Placed(ctx, records, stride=length + 1)
        tree.set_records(0, table.view)
        assert ctx.scrub_staging() == 0
        buf2 = np.zeros((nupd, rowb), dtype=np.uint8)
        assert call(table, buf2, rowb, None) == 0
        assert np.array_equal(buf2, want_rows)
        _assert_tree(tree, model.levels, "no roots")
        table.holds(model.records, "no roots")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. two chunks
def test_two_chunks(ctx):
    depth, length, nupd = 1, 65521, 520
    rowb = _row_bytes(length, depth)
    per_chunk = (64 << 20) // rowb
    assert rowb == 131139 and per_chunk == 511
    rng = np.random.default_rng(10300)
    records = _records(rng, 2, length)
    new = rng.integers(0, 256, size=(nupd, length), dtype=np.uint8)
    idx = rng.integers(0, 2, size=nupd)
    idx[per_chunk - 2: per_chunk + 2] = [0, 1, 1, 0]  # both records change on both sides of the seam ...
    idx[-4:] = [1, 0, 0, 1]  # ... and the second chunk reads what it wrote itself, too
    assert set(idx[:per_chunk]) == set(idx[per_chunk:]) == {0, 1}
    model = RecordModel(records)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 2, off=1)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        for kind in ("merkle_level", "sha256_records", "merkle_updates", "merkle_record_rows"):
            ctx.timing_drain(kind)
        _check_batch(tree, model, table, [int(i) for i in idx], [r.tobytes() for r in new], "two chunks", new_data=new)
        assert ctx.timing_drain("merkle_updates")[::2] == (2 * (depth + 1), nupd * depth)
        assert ctx.timing_drain("sha256_records")[::2] == (2, nupd)
        assert ctx.timing_drain("merkle_record_rows")[::2] == (4, nupd)
        assert ctx.timing_drain("merkle_level")[0] == 0
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. against set_records
def test_same_tree_as_set_records(ctx):
    depth, nupd, length = 9, 300, 55
    rng = np.random.default_rng(10400)
    records = rng.integers(0, 256, size=(1 << depth, length), dtype=np.uint8)
    idx = rng.integers(0, 40, size=nupd)
    new = rng.integers(0, 256, size=(nupd, length), dtype=np.uint8)
    final = records.copy()
    for i, r in zip(idx, new):
        final[i] = r
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        table = ctx.to_device(records).reshape(1 << depth, length)
        a.set_records(0, table)
        a.update_records(table, idx, new)
        assert np.array_equal(table.cpu().numpy(), final)
        b.set_records(0, table)
        ctx.sync()
        for l in range(depth + 1):
            assert a.nodes(l).cpu().numpy().tobytes() == b.nodes(l).cpu().numpy().tobytes(), l
        assert a.root() == b.root()
        assert a.nodes(0).cpu().numpy().tobytes() == b"".join(hashlib.sha256(r.tobytes()).digest() for r in final)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    p = mf.Params(d=1 << 18, m=174762)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    length = 55
    st = W.MerkleRecordUpdate(length, 1, frozen=(0, 8))
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == 512
    nin = 512 + 16 * length + 257
    rng = np.random.default_rng(10500)
    records = _records(rng, 2, length)
    indices = [0, 1, 1, 0, 1]
    new = [records[i][:8] + rng.bytes(length - 8) for i in indices]  # bytes [0, 8), the key, stay
    tree = ctx.merkle_tree(1)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        table = Placed(ctx, records, stride=length + 1, off=2)
        tree.set_records(0, table.view)
        model = RecordModel(records)
        want_rows, want_roots = model.batch(indices, new)
        bits, roots = tree.update_record_bits(table.view, indices, np.stack([np.frombuffer(r, dtype=np.uint8) for r in new]), roots=True)
        assert bits.shape == (5, nin) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows)
        roots = [r.tobytes() for r in roots]
        assert roots == want_roots and len(set(roots)) == 6
        table.holds(model.records, "end to end")
        witness, holds = ctx.circuit_assign(prog, bits)
        assert holds.all()
        for k in range(5):
            assert st.roots_of(witness[k]) == (roots[k], roots[k + 1]), k
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count.any() and (first == 0xFFFFFFFF).all()

        ctx.ssp_prepare(None)
        alpha, beta, s = (int(x) for x in rng.integers(1, C.P, size=3, dtype=np.uint64))
        d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
        d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
        d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()
        vk = ctx.derive_vk(None, s, lu)
        deltas = [int(x) for x in rng.integers(0, C.P, size=5, dtype=np.uint64)]
        mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(5)]
        signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(5)]
        proofs = ctx.prove_batch_public(d_crs, None, lu, [witness[k].tobytes() for k in range(5)], deltas, mags, signs).clone()

        def verify(statements):
            return [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, statements), np.uint8)]

        own = [st.statement(roots[k], roots[k + 1]) for k in range(5)]
        assert all(len(x) == 64 for x in own) and own == [witness[k][:64].tobytes() for k in range(5)]
        assert verify(own) == [True] * 5
        assert verify(own[1:] + own[:1]) == [False] * 5  # each against its neighbour's transition
        assert verify([st.statement(roots[k + 1], roots[k]) for k in range(5)]) == [False] * 5  # the transition backwards

        # a sixth update whose new record changes byte 0 of the frozen key: both roots are computed, the statement does not hold
        moved = bytes([model.records[0][0] ^ 1]) + rng.bytes(length - 1)
        want_row, want_root = model.batch([0], [moved])
        bits6, roots6 = tree.update_record_bits(table.view, [0], np.frombuffer(moved, dtype=np.uint8).reshape(1, length), roots=True)
        assert np.array_equal(np.packbits(bits6, axis=1, bitorder="little"), want_row)
        assert [r.tobytes() for r in roots6] == want_root == [roots[5], model.root()]
        witness6, holds6 = ctx.circuit_assign(prog, bits6)
        assert not holds6.any() and st.roots_of(witness6[0]) == (roots[5], model.root())
        count6, first6 = ctx.ssp_rows_violations(witness6)
        assert count6[0] > 0 and first6[0] != 0xFFFFFFFF
        table.holds(model.records, "the sixth update")

        # the documented precondition, pinned: record 0 overwritten behind the tree's back -- the row's computed old root is not the tree's root
        r_before = tree.root()
        forged = model.records[0][:8] + rng.bytes(length - 8)
        table.view[0] = ctx.to_device(np.frombuffer(forged, dtype=np.uint8))
        nxt = forged[:8] + rng.bytes(length - 8)
        bits7, roots7 = tree.update_record_bits(table.view, [0], np.frombuffer(nxt, dtype=np.uint8).reshape(1, length), roots=True)
        assert roots7[0].tobytes() == r_before
        witness7, holds7 = ctx.circuit_assign(prog, bits7)
        assert holds7.all()  # (the circuit's own relation holds: the key stayed)
        old7, new7 = st.roots_of(witness7[0])
        sib = model.levels[0][1]
        assert old7 != r_before and old7 == _parent(hashlib.sha256(forged).digest(), sib)
        assert new7 == roots7[1].tobytes() == _parent(hashlib.sha256(nxt).digest(), sib)
    finally:
        prog.close()
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. MFH_EINVAL
def test_einval(ctx, mf):
    import torch

    lib, h = ctx.lib, ctx._h
    depth, length = 3, 17
    rng = np.random.default_rng(10600)
    records = _records(rng, 8, length)
    model = RecordModel(records)
    rowb = _row_bytes(length, depth)
    tree = ctx.merkle_tree(depth)
    texts = []

    def refused(rc, handle=h):
        assert rc == EINVAL
        text = lib.mfh_last_error(handle).decode()
        assert text.startswith("mfh_merkle_update_records: "), text
        texts.append(text)

    try:
        table = Placed(ctx, records, stride=length + 3, off=1)
        fresh = Placed(ctx, _records(rng, 3, length), stride=length + 2, off=3)
        tree.set_records(0, table.view)
        ctx.sync()
        ctx.set_timing(True)
        for kind in ("merkle_level", "sha256_records", "merkle_updates", "merkle_record_rows"):
            ctx.timing_drain(kind)
        vp = ctypes.c_void_p
        idx = np.array([5, 0, 7], dtype=np.uint32)
        bad = np.array([5, 0, 8], dtype=np.uint32)
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((4, 32), 0xCD, dtype=np.uint8)
        ip, xp, bp, rp = vp(idx.ctypes.data), vp(bad.ctypes.data), vp(buf.ctypes.data), vp(roots.ctypes.data)
        tp, ts, fp, fs = vp(table.view.data_ptr()), table.stride, vp(fresh.view.data_ptr()), fresh.stride
        stride = buf.shape[1]
        f = lib.mfh_merkle_update_records
        refused(f(h, None, 3, ip, tp, ts, length, fp, fs, bp, stride, rp))
        refused(f(h, tree._h, 3, None, tp, ts, length, fp, fs, bp, stride, rp))
        refused(f(h, tree._h, 3, ip, tp, ts, length, fp, fs, None, stride, rp))
        refused(f(h, tree._h, 3, ip, None, ts, length, fp, fs, bp, stride, rp))
        refused(f(h, tree._h, 3, ip, tp, ts, length, None, fs, bp, stride, rp))
        refused(f(h, tree._h, 3, xp, tp, ts, length, fp, fs, bp, stride, rp))
        refused(f(h, tree._h, 3, ip, tp, length - 1, length, fp, fs, bp, stride, rp))
        refused(f(h, tree._h, 3, ip, tp, ts, length, fp, length - 1, bp, stride, rp))
        refused(f(h, tree._h, 3, ip, tp, (1 << 20) + 1, (1 << 20) + 1, fp, (1 << 20) + 1, bp, 1 << 22, rp))
        refused(f(h, tree._h, 3, ip, tp, ts, length, fp, fs, bp, rowb - 1, rp))
        assert f(None, tree._h, 3, ip, tp, ts, length, fp, fs, bp, stride, rp) == EINVAL
        assert len(set(texts)) == 10, sorted(set(texts))
        if torch.cuda.device_count() > 1:
            other = mf.Context(mf.DEBUG, 1)
            try:
                assert f(other._h, tree._h, 3, ip, tp, ts, length, fp, fs, bp, stride, rp) == EINVAL
                assert lib.mfh_last_error(other._h).decode() == "mfh_merkle_update_records: the tree belongs to another device"
            finally:
                other.close()
                torch.cuda.set_device(ctx.device)
        # nupd = 0 does nothing, whatever the pointers
        assert f(h, tree._h, 0, None, None, ts, length, None, fs, None, rowb, None) == 0
        assert f(h, tree._h, 0, ip, tp, ts, length, fp, fs, bp, stride, rp) == 0
        none = np.zeros((0, length), dtype=np.uint8)
        rows0, roots0 = tree.update_records(table.view, [], none, roots=True)
        assert rows0.shape == (0, rowb) and roots0.shape == (1, 32) and roots0[0].tobytes() == model.root()
        assert tree.update_record_bits(table.view, [], none).shape == (0, 512 + 16 * length + 257 * depth)
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xCD).all()
        for kind in ("merkle_updates", "merkle_level", "sha256_records", "merkle_record_rows"):
            assert ctx.timing_drain(kind)[0] == 0, kind
        ctx.set_timing(False)
        _assert_tree(tree, model.levels, "after the refused calls")
        table.holds(records, "after the refused calls")
        one = np.zeros((1, length), dtype=np.uint8)
        for bad_table, bad_idx, bad_new in [(table.view, [1, 2], one), (table.view, [1], one[:, :-1]), (table.view, [-1], one), (table.view, [1 << 32], one),
                                            (table.view[:4], [1], one), (table.view.cpu().numpy(), [1], one), (table.view.to(torch.int8), [1], one),
                                            (table.view, [1], one.astype(np.int8)), (table.view.t(), [1], one)]:
            with pytest.raises(mf.MfhError):
                tree.update_records(bad_table, bad_idx, bad_new)
        _assert_tree(tree, model.levels, "after the refused Python calls")
        table.holds(records, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 9. inputs and ordering
def test_new_records_as_numpy_and_tensor_table_as_column_slice(ctx):
    depth, length, width = 3, 21, 40
    rng = np.random.default_rng(10700)
    wide = rng.integers(0, 256, size=(8, width), dtype=np.uint8)
    records = [wide[i, 7: 7 + length].tobytes() for i in range(8)]
    indices = [3, 2, 3, 6, 2]
    new = _records(rng, 5, length)
    arr = np.stack([np.frombuffer(r, dtype=np.uint8) for r in new])
    wide_new = rng.integers(0, 256, size=(5, width), dtype=np.uint8)
    wide_new[:, 2: 2 + length] = arr
    d_wide_new = ctx.to_device(wide_new).reshape(5, width)
    inputs = [("numpy", arr), ("tensor", ctx.to_device(arr).reshape(5, length)), ("a column slice", d_wide_new[:, 2: 2 + length])]
    tree = ctx.merkle_tree(depth)
    try:
        for what, data in inputs:
            d_wide = ctx.to_device(wide).reshape(8, width)
            table = d_wide[:, 7: 7 + length]
            assert table.stride(0) == width and not table.is_contiguous()
            tree.set_records(0, table)
            model = RecordModel(records)
            want_rows, want_roots = model.batch(indices, new)
            rows, roots = tree.update_records(table, indices, data, roots=True)
            assert np.array_equal(rows, want_rows) and [r.tobytes() for r in roots] == want_roots, what
            _assert_tree(tree, model.levels, what)
            after = wide.copy()
            for i, r in enumerate(model.records):
                after[i, 7: 7 + length] = np.frombuffer(r, dtype=np.uint8)
            assert np.array_equal(d_wide.cpu().numpy(), after), what  # the other columns stay
        assert np.array_equal(d_wide_new.cpu().numpy(), wide_new)
    finally:
        tree.close()


def _late_updates(ctx):
    depth, nupd, length = 9, 64, 55
    rng = np.random.default_rng(10800)
    records = _records(rng, 1 << depth, length)
    indices = [int(x) for x in rng.integers(0, 16, size=nupd)]
    new = _records(rng, nupd, length)
    model = RecordModel(records)
    want_rows, want_roots = model.batch(indices, new)  # (first: nothing of the host's stands between the late inputs and the calls)
    tree = ctx.merkle_tree(depth)
    try:
        table = Placed(ctx, records, stride=length + 1, off=1, late=True)
        fresh = Placed(ctx, new, off=2, late=True)
        tree.set_records(0, table.view)  # no wait before it, nor before the next
        _check_against(tree, table, fresh.view, indices, want_rows, want_roots, model.levels, model.records, "late table and new records")
    finally:
        tree.close()


def test_ordering_null_stream(ctx):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_updates(ctx)


def test_ordering_callers_stream(gpu_ctx_factory, mf):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_updates(c)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()
