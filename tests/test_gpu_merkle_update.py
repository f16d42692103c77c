"""GPU: batches of sequential one-leaf updates (mfh_merkle_update_rows, MerkleTree.update_rows / update_bits) against a sequential model in this file over
tests/sha256_ref.py's merkle_parent, memoised as in tests/test_gpu_merkle.py (whose cache, tree builder and helpers are used here, so the depth-12 tree
of that file's `ref12` leaves is computed once a session).

1. exactness: the rows byte for byte against MerkleUpdate(depth).bits, all nupd + 1 roots and every node of the tree afterwards -- depth 1, 2, 3 with a
   single update, the same index three times, leaf 2j then 2j + 1 and the reverse, two leaves of different subtrees then their common ancestor's other
   side; depth 3 with 257 random updates (8 leaves: every kind of collision, and a second workgroup); depth 9 with 300; depth 12 with 64.
2. a wider in_stride keeps its tail bytes; "merkle_updates" counts depth + 1 launches and nupd x depth compressions a chunk, "merkle_level" none.
3. two chunks: depth 1 with (64 << 20) // 161 + 3 updates, the model being leaf tracking in numpy (at depth 1 a row's old leaf and sibling are leaf
   values): every row, 64 sampled roots by merkle_parent, the final tree.
4. after a batch, a second tree given the final leaves by set_leaves has the same nodes.
5. end to end at d = 2^17 with MerkleUpdate(1): update_bits of 5 sequential updates (one index repeated) hold in circuit_assign with
   roots_of = (R_k, R_k+1), violate no row, and their proofs verify under statement(R_k, R_k+1) and under neither the neighbour's statement nor the
   statement with the roots swapped.
6. every MFH_EINVAL case leaves the nodes and the timing counts as they were; nupd = 0 does nothing.
7. new leaves as bytes, numpy, an aligned and a misaligned device tensor, and the digests of Context.sha256_records; new leaves produced late on the
   stream, on the null stream and on a caller's stream.

MerkleUpdate(depth).bits reads the depth alone.  At depth 1, 2 and 3 it is called on the statement; at depth 9 and 12, where building the statement's
circuit (up to 680 000 gates) would take seconds for nothing, the same method is called on a stand-in that holds the depth -- depth 3 checks that
both give the same bits."""
import ctypes
import functools
import hashlib
import types

import numpy as np
import pytest

from test_gpu_merkle import _assert_tree, _late, _leaves, _parent, ref_tree

pytestmark = pytest.mark.gpu

SEED = bytes((31 * i + 5) & 0xFF for i in range(40))
EINVAL = -1


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
@functools.lru_cache(maxsize=None)
def _statement(depth):
    from c_lwe_snarks_amd import words

    return words.MerkleUpdate(depth) if depth <= 3 else types.SimpleNamespace(depth=depth)


def _bits(depth, old, new, sibs, index):
    from c_lwe_snarks_amd import words

    return words.MerkleUpdate.bits(_statement(depth), old, new, sibs, index)


def _row_bytes(depth):
    return 128 + 32 * depth + (depth + 7) // 8


class Model:
    """the tree as lists of nodes per level, updated one leaf at a time"""

    def __init__(self, leaves):
        self.levels = [list(level) for level in ref_tree(leaves)]
        self.depth = len(self.levels) - 1

    def root(self):
        return self.levels[-1][0]

    def update(self, i, new):
        """(the MerkleUpdate input bits before the update, the root after it)"""
        sibs = [self.levels[l][(i >> l) ^ 1] for l in range(self.depth)]
        bits = _bits(self.depth, self.levels[0][i], new, sibs, i)
        cur = self.levels[0][i] = new
        for l in range(self.depth):
            j = i >> l
            cur = _parent(sibs[l], cur) if j & 1 else _parent(cur, sibs[l])
            self.levels[l + 1][j >> 1] = cur
        return bits, cur

    def batch(self, indices, new_leaves):
        """(packed rows [n, row bytes], roots [n + 1] as bytes)"""
        roots, rows = [self.root()], []
        for i, new in zip(indices, new_leaves):
            bits, root = self.update(int(i), new)
            rows.append(bits)
            roots.append(root)
        width = 1024 + 257 * self.depth
        rows = np.packbits(np.stack(rows), axis=1, bitorder="little") if rows else np.zeros((0, (width + 7) // 8), dtype=np.uint8)
        assert rows.shape[1] == _row_bytes(self.depth)
        return rows, roots


def _check_batch(tree, model, indices, new_leaves, what, data=None):
    """one update_rows call against the model: rows, roots, every node"""
    want_rows, want_roots = model.batch(indices, new_leaves)
    rows, roots = tree.update_rows(indices, b"".join(new_leaves) if data is None else data, roots=True)
    assert rows.dtype == np.uint8 and rows.shape == want_rows.shape, what
    assert np.array_equal(rows, want_rows), what
    assert roots.shape == (len(indices) + 1, 32) and [r.tobytes() for r in roots] == want_roots, what
    _assert_tree(tree, model.levels, what)


@pytest.fixture(scope="module")
def ref12():
    """tests/test_gpu_merkle.py's depth-12 leaves (the same generator): their tree comes out of the shared cache"""
    return _leaves(np.random.default_rng(1200), 1 << 12)


# ---------------------------------------------------------------------------------------------------------------- 1. exactness
def _hand_made(depth):
    n = 1 << depth
    j = n // 2 - 1
    cousins = [0, 1 << (depth - 2), 1 << (depth - 1), 0] if depth >= 2 else [0, 1, 0]
    return [("single", [n - 1]), ("same index three times", [1, 1, 1]), ("2j then 2j + 1", [2 * j, 2 * j + 1]), ("2j + 1 then 2j", [2 * j + 1, 2 * j]),
            ("two subtrees, then the other side", cousins)]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_hand_made_batches(ctx, W, depth):
    rng = np.random.default_rng(9000 + depth)
    leaves = _leaves(rng, 1 << depth)
    if depth == 3:  # the stand-in of the deep cases gives what the statement gives
        args = (leaves[0], leaves[1], leaves[2:5], 5)
        assert np.array_equal(W.MerkleUpdate.bits(types.SimpleNamespace(depth=3), *args), _statement(3).bits(*args))
    tree = ctx.merkle_tree(depth)
    try:
        # each batch on a fresh copy of the starting tree, then all of them one after the other on one tree
        for what, indices in _hand_made(depth):
            tree.set_leaves(0, b"".join(leaves))
            _check_batch(tree, Model(leaves), indices, _leaves(rng, len(indices)), (depth, what))
        tree.set_leaves(0, b"".join(leaves))
        model = Model(leaves)
        for what, indices in _hand_made(depth):
            _check_batch(tree, model, indices, _leaves(rng, len(indices)), (depth, "in a row", what))
    finally:
        tree.close()


@pytest.mark.parametrize("depth,nupd", [(3, 257), (9, 300), (12, 64)])
def test_random_batches(ctx, ref12, depth, nupd):
    rng = np.random.default_rng(9100 + depth)
    leaves = ref12 if depth == 12 else _leaves(rng, 1 << depth)
    # heavy repeats at every depth: half of the draws come from 8 leaves that include two sibling pairs
    hot = [0, 1, 6 % (1 << depth), 7 % (1 << depth)] + [int(x) for x in rng.integers(0, 1 << depth, size=4)]
    indices = [hot[int(rng.integers(0, 8))] if rng.integers(0, 2) else int(rng.integers(0, 1 << depth)) for _ in range(nupd)]
    assert len(set(indices)) < nupd
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, b"".join(leaves))
        _check_batch(tree, Model(leaves), indices, _leaves(rng, nupd), (depth, nupd))
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. stride and launches
def test_wider_stride_and_launch_counts(ctx):
    depth, nupd = 9, 300
    rng = np.random.default_rng(9200)
    leaves = _leaves(rng, 1 << depth)
    indices = [int(x) for x in rng.integers(0, 24, size=nupd)]
    new = _leaves(rng, nupd)
    model = Model(leaves)
    want_rows, want_roots = model.batch(indices, new)
    rowb = _row_bytes(depth)
    assert rowb == 418
    stride = rowb + 13
    buf = np.full((nupd, stride), 0xAB, dtype=np.uint8)
    roots = np.full((nupd + 1, 32), 0xCD, dtype=np.uint8)
    iu = np.array(indices, dtype=np.uint32)
    d_new = ctx.to_device(np.frombuffer(b"".join(new), dtype=np.uint8))
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, b"".join(leaves))
        ctx.sync()
        ctx.set_timing(True)
        ctx.timing_drain("merkle_level")
        vp = ctypes.c_void_p
        rc = ctx.lib.mfh_merkle_update_rows(ctx._h, tree._h, nupd, vp(iu.ctypes.data), vp(d_new.data_ptr()), vp(buf.ctypes.data), stride, vp(roots.ctypes.data))
        assert rc == 0
        launches, ms, rows = ctx.timing_drain("merkle_updates")
        print(f"depth {depth}: {nupd} updates in {launches} launches over {rows} compressions: {ms:.3f} ms")
        assert (launches, rows) == (depth + 1, nupd * depth)
        assert ctx.timing_drain("merkle_level")[0] == 0
        ctx.set_timing(False)
        assert np.array_equal(buf[:, :rowb], want_rows)
        assert (buf[:, rowb:] == 0xAB).all()
        assert [r.tobytes() for r in roots] == want_roots
        _assert_tree(tree, model.levels, "wider stride")
        # h_roots = NULL, and the pinned staging zeroed between two calls: the same rows from the same starting tree
        tree.set_leaves(0, b"".join(leaves))
        assert ctx.scrub_staging() == 0
        buf2 = np.zeros((nupd, rowb), dtype=np.uint8)
        assert ctx.lib.mfh_merkle_update_rows(ctx._h, tree._h, nupd, vp(iu.ctypes.data), vp(d_new.data_ptr()), vp(buf2.ctypes.data), rowb, None) == 0
        assert np.array_equal(buf2, want_rows)
        _assert_tree(tree, model.levels, "no roots")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. two chunks
def _swap_words(a):
    """[n, 32] digest bytes -> the bytes of their eight words as little-endian uint32"""
    return a.reshape(len(a), 8, 4)[:, :, ::-1].reshape(len(a), 32)


def test_two_chunks(ctx):
    depth = 1
    rowb = _row_bytes(depth)
    assert rowb == 161
    per_chunk = (64 << 20) // rowb
    nupd = per_chunk + 3
    assert per_chunk == 416825 and nupd == 416828
    rng = np.random.default_rng(9300)
    start = rng.integers(0, 256, size=(2, 32), dtype=np.uint8)
    new = rng.integers(0, 256, size=(nupd, 32), dtype=np.uint8)
    idx = rng.integers(0, 2, size=nupd).astype(np.uint32)
    idx[per_chunk - 2: per_chunk + 2] = [0, 1, 1, 0]  # both leaves change on both sides of the seam
    # leaf tracking: before update k, leaf s holds new[j] for the last j < k with idx[j] == s, else start[s]
    k = np.arange(nupd)
    before = []
    for s in (0, 1):
        last = np.maximum.accumulate(np.where(idx == s, k, -1))
        prev = np.concatenate([[-1], last[:-1]])
        before.append(np.where(prev[:, None] >= 0, new[np.maximum(prev, 0)], start[s]))
    mine = (idx == 1)[:, None]
    old, sib = np.where(mine, before[1], before[0]), np.where(mine, before[0], before[1])
    want = np.concatenate([np.zeros((nupd, 64), dtype=np.uint8), _swap_words(old), _swap_words(new), _swap_words(sib), idx[:, None].astype(np.uint8)], axis=1)
    assert want.shape == (nupd, rowb)
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, start)
        ctx.sync()
        ctx.set_timing(True)
        rows, roots = tree.update_rows(idx, new, roots=True)
        launches, ms, total = ctx.timing_drain("merkle_updates")
        ctx.set_timing(False)
        print(f"depth 1: {nupd} updates in {launches} launches: {ms:.3f} ms")
        assert (launches, total) == (2 * (depth + 1), nupd * depth)
        assert rows.shape == want.shape and np.array_equal(rows, want)
        # root t + 1 is the parent of the two leaves after update t
        after = [np.concatenate([before[s][1:], before[s][-1:]]) for s in (0, 1)]
        after[int(idx[-1])][-1] = new[-1]
        assert roots.shape == (nupd + 1, 32)
        assert roots[0].tobytes() == _parent(start[0].tobytes(), start[1].tobytes())
        picks = [0, per_chunk - 2, per_chunk - 1, per_chunk, per_chunk + 1, nupd - 1] + [int(x) for x in rng.integers(0, nupd, size=58)]
        assert len(picks) == 64
        for t in picks:
            assert roots[t + 1].tobytes() == _parent(after[0][t].tobytes(), after[1][t].tobytes()), t
        final = [after[0][-1].tobytes(), after[1][-1].tobytes()]
        _assert_tree(tree, ref_tree(final), "two chunks")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. against set_leaves
def test_same_tree_as_set_leaves(ctx):
    depth, nupd = 9, 300
    rng = np.random.default_rng(9400)
    leaves = rng.integers(0, 256, size=(1 << depth, 32), dtype=np.uint8)
    idx = rng.integers(0, 40, size=nupd)
    new = rng.integers(0, 256, size=(nupd, 32), dtype=np.uint8)
    final = leaves.copy()
    for i, leaf in zip(idx, new):
        final[i] = leaf
    a, b = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
    try:
        a.set_leaves(0, leaves)
        a.update_rows(idx, new)
        b.set_leaves(0, final)
        ctx.sync()
        for l in range(depth + 1):
            assert a.nodes(l).cpu().numpy().tobytes() == b.nodes(l).cpu().numpy().tobytes(), l
        assert a.root() == b.root()
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def test_end_to_end_proofs(gpu_ctx_factory, mf, W):
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    st = _statement(1)
    cc = st.circuit.compile(p)
    lu = cc.lu
    assert lu == 512
    rng = np.random.default_rng(9500)
    leaves = _leaves(rng, 2)
    indices = [0, 1, 1, 0, 1]
    new = _leaves(rng, 5)
    tree = ctx.merkle_tree(1)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        tree.set_leaves(0, b"".join(leaves))
        model = Model(leaves)
        want_rows, want_roots = model.batch(indices, new)
        bits, roots = tree.update_bits(indices, b"".join(new), roots=True)
        assert bits.shape == (5, 1024 + 257) and np.array_equal(np.packbits(bits, axis=1, bitorder="little"), want_rows)
        roots = [r.tobytes() for r in roots]
        assert roots == want_roots and len(set(roots)) == 6
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
    finally:
        prog.close()
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. MFH_EINVAL
def test_einval(ctx):
    import torch

    lib, h = ctx.lib, ctx._h
    depth = 3
    leaves = _leaves(np.random.default_rng(9600), 8)
    levels = ref_tree(leaves)
    rowb = _row_bytes(depth)
    tree = ctx.merkle_tree(depth)
    texts = []

    def refused(rc, handle=h):
        assert rc == EINVAL
        text = lib.mfh_last_error(handle).decode()
        assert text.startswith("mfh_merkle_update_rows: "), text
        texts.append(text)

    try:
        tree.set_leaves(0, b"".join(leaves))
        ctx.sync()
        ctx.set_timing(True)
        ctx.timing_drain("merkle_level")
        vp = ctypes.c_void_p
        d_new = torch.full((3 * 32 + 16,), 0xEE, dtype=torch.uint8, device=ctx.device)
        assert d_new.data_ptr() % 16 == 0
        idx = np.array([5, 0, 7], dtype=np.uint32)
        bad = np.array([5, 0, 8], dtype=np.uint32)
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        roots = np.full((4, 32), 0xCD, dtype=np.uint8)
        ip, xp, np_, bp, rp = vp(idx.ctypes.data), vp(bad.ctypes.data), vp(d_new.data_ptr()), vp(buf.ctypes.data), vp(roots.ctypes.data)
        stride = buf.shape[1]
        refused(lib.mfh_merkle_update_rows(h, None, 3, ip, np_, bp, stride, rp))
        refused(lib.mfh_merkle_update_rows(h, tree._h, 3, None, np_, bp, stride, rp))
        refused(lib.mfh_merkle_update_rows(h, tree._h, 3, ip, None, bp, stride, rp))
        refused(lib.mfh_merkle_update_rows(h, tree._h, 3, ip, np_, None, stride, rp))
        refused(lib.mfh_merkle_update_rows(h, tree._h, 3, xp, np_, bp, stride, rp))
        refused(lib.mfh_merkle_update_rows(h, tree._h, 3, ip, np_, bp, rowb - 1, rp))
        for off in (1, 4, 8):
            refused(lib.mfh_merkle_update_rows(h, tree._h, 3, ip, vp(d_new.data_ptr() + off), bp, stride, rp))
        assert lib.mfh_merkle_update_rows(None, tree._h, 3, ip, np_, bp, stride, rp) == EINVAL
        assert len(set(texts)) == 7, sorted(set(texts))  # (the three misalignments share one)
        if torch.cuda.device_count() > 1:
            import c_lwe_snarks_amd as m

            other = m.Context(m.DEBUG, 1)
            try:
                assert lib.mfh_merkle_update_rows(other._h, tree._h, 3, ip, np_, bp, stride, rp) == EINVAL
                assert lib.mfh_last_error(other._h).decode() == "mfh_merkle_update_rows: the tree belongs to another device"
            finally:
                other.close()
                torch.cuda.set_device(ctx.device)
        # nupd = 0 does nothing, whatever the pointers
        assert lib.mfh_merkle_update_rows(h, tree._h, 0, None, None, None, rowb, None) == 0
        assert lib.mfh_merkle_update_rows(h, tree._h, 0, ip, np_, bp, stride, rp) == 0
        rows0, roots0 = tree.update_rows([], b"", roots=True)
        assert rows0.shape == (0, rowb) and roots0.shape == (1, 32) and roots0[0].tobytes() == levels[-1][0]
        assert tree.update_bits([], b"").shape == (0, 1024 + 257 * depth)
        # nothing was written, launched or changed
        assert (buf == 0xAB).all() and (roots == 0xCD).all()
        assert ctx.timing_drain("merkle_updates")[0] == 0 and ctx.timing_drain("merkle_level")[0] == 0
        ctx.set_timing(False)
        _assert_tree(tree, levels, "after the refused calls")
        for bad_idx, bad_leaves in [([1, 2], bytes(32)), ([1], bytes(31)), ([-1], bytes(32)), ([1 << 32], bytes(32))]:
            with pytest.raises(ctx_error()):
                tree.update_rows(bad_idx, bad_leaves)
        _assert_tree(tree, levels, "after the refused Python calls")
    finally:
        ctx.set_timing(False)
        tree.close()


def ctx_error():
    import c_lwe_snarks_amd as m

    return m.MfhError


# ---------------------------------------------------------------------------------------------------------------- 7. inputs and ordering
def test_new_leaves_as_bytes_numpy_tensors_and_digests(ctx):
    import torch

    depth = 3
    rng = np.random.default_rng(9700)
    leaves = _leaves(rng, 8)
    indices = [3, 2, 3, 6, 2]
    records = rng.integers(0, 256, size=(5, 55), dtype=np.uint8)
    new = [hashlib.sha256(r.tobytes()).digest() for r in records]
    raw = b"".join(new)
    arr = np.frombuffer(raw, dtype=np.uint8).reshape(5, 32)
    wide = torch.zeros(8 + 5 * 32, dtype=torch.uint8, device=ctx.device)
    wide[8:] = ctx.to_device(arr)
    off = wide[8:]
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    inputs = [("bytes", raw), ("bytearray", bytearray(raw)), ("numpy", arr), ("tensor", ctx.to_device(arr).reshape(5, 32)), ("misaligned tensor", off),
              ("sha256_records", ctx.sha256_records(records))]
    tree = ctx.merkle_tree(depth)
    try:
        for what, data in inputs:
            tree.set_leaves(0, b"".join(leaves))
            _check_batch(tree, Model(leaves), indices, new, what, data=data)
    finally:
        tree.close()


def _late_updates(ctx, ref12):
    depth, nupd = 12, 64
    rng = np.random.default_rng(9800)
    indices = [int(x) for x in rng.integers(0, 16, size=nupd)]
    new = _leaves(rng, nupd)
    tree = ctx.merkle_tree(depth)
    try:
        d_all, d_new = _late(ctx, b"".join(ref12)), _late(ctx, b"".join(new))
        tree.set_leaves(0, d_all)
        _check_batch(tree, Model(ref12), indices, new, "late new leaves", data=d_new)  # no wait before it
    finally:
        tree.close()


def test_ordering_null_stream(ctx, ref12):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_updates(ctx, ref12)


def test_ordering_callers_stream(gpu_ctx_factory, mf, ref12):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_updates(c, ref12)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()
