"""GPU: the Merkle tree in device memory (mfh_merkle, Context.merkle_tree) against the pure-Python compression of tests/sha256_ref.py.

1. full builds at depths 1, 2, 3, 9 and 12 (levels of many workgroups, one workgroup, part of one): every node of every level, read through nodes(level),
   and root() equal the reference tree; a fresh handle is the tree of zero leaves; a build is `depth` launches over 2^depth - 1 parents.  These comparisons
   are also what pins the device pass of sha256_dev.hpp (its v_bitop3 truth tables and v_alignbit rotations): the CPU test sees the host pass alone.
2. updates of a built depth-12 tree: after each range every node equals the reference rebuilt from the leaves, and the launches recompute exactly the
   ranges' parents; leaves as bytes, numpy and a device tensor give the same tree.
3. paths at depths 1, 2, 7, 8, 9 and 12 (direction bits in less than one, one and more than one byte): path_bits equals MerklePath(depth).bits of the
   reference tree's leaf and siblings; a wider in_stride leaves the rest of the row alone; 116 108 statements at depth 16 go through two chunks.
4. every MFH_EINVAL case through the raw C calls: the code, a text of its own, nothing written or launched.
5. one root, many proofs: 33 statements of one depth-2 tree hold with the tree's root; four proofs verify under the ONE statement
   MerklePath.statement(root), fail under a root with a bit flipped, and fail under the new root after a leaf changed, while fresh proofs pass.
6. two overlapping set_leaves and root() with no wait in between, on the null stream and on a caller's stream behind late inputs.

The reference's node function is memoised (a pure function of 64 bytes): "the reference tree rebuilt from scratch" recomputes what changed."""
import ctypes
import functools

import numpy as np
import pytest

import sha256_ref as ref

pytestmark = pytest.mark.gpu

SEED = bytes((29 * i + 3) & 0xFF for i in range(40))
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
_parent = functools.lru_cache(maxsize=None)(ref.merkle_parent)


def ref_tree(leaves):
    """levels[l][j] = node j of level l (0 = the leaves) of the tree over `leaves`"""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([_parent(cur[j], cur[j + 1]) for j in range(0, len(cur), 2)])
    return levels


def _leaves(rng, n):
    return [rng.bytes(32) for _ in range(n)]


@pytest.fixture(scope="module")
def ref12():
    """random leaves of depth 12 and their tree, shared and never changed"""
    leaves = _leaves(np.random.default_rng(1200), 1 << 12)
    return leaves, ref_tree(leaves)


@functools.lru_cache(maxsize=None)
def _statement(depth):
    from c_lwe_snarks_amd import words

    return words.MerklePath(depth)


def _assert_tree(tree, levels, what=""):
    assert len(levels) == tree.depth + 1
    for l, want in enumerate(levels):
        got = tree.nodes(l)
        assert tuple(got.shape) == (1 << (tree.depth - l), 32)
        assert got.cpu().numpy().tobytes() == b"".join(want), (what, l)
    assert tree.root() == levels[-1][0], what


def _expected_rows(depth, first, count):
    return [((first + count - 1) >> l) - (first >> l) + 1 for l in range(1, depth + 1)]


# ---------------------------------------------------------------------------------------------------------------- 1. full builds
@pytest.mark.parametrize("depth", [1, 2, 3, 9, 12])
def test_full_build(ctx, ref12, depth):
    n = 1 << depth
    leaves, levels = ref12 if depth == 12 else (None, None)
    if leaves is None:
        leaves = _leaves(np.random.default_rng(100 + depth), n)
        levels = ref_tree(leaves)
    tree = ctx.merkle_tree(depth)
    try:
        _assert_tree(tree, ref_tree([bytes(32)] * n), "fresh handle")
        ctx.set_timing(True)
        tree.set_leaves(0, b"".join(leaves))
        launches, ms, rows = ctx.timing_drain("merkle_level")
        ctx.set_timing(False)
        print(f"depth {depth}: full build, {launches} launches of k_merkle_level over {rows} parents: {ms:.3f} ms")
        assert (launches, rows) == (depth, n - 1)
        _assert_tree(tree, levels, "full build")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. updates
# (first, count, parents at level 1)
UPDATES = [(0, 1, 1), (4095, 1, 1), (1, 1, 1), (1023, 3, 2), (511, 514, 258), (512, 512, 256), (510, 512, 256), (3, 510, 256), (2, 510, 255)]


def test_updates(ctx, ref12):
    depth = 12
    leaves = list(ref12[0])
    tree = ctx.merkle_tree(depth)
    rng = np.random.default_rng(1201)
    try:
        tree.set_leaves(0, b"".join(leaves))
        ctx.set_timing(True)
        for k, (first, count, level1) in enumerate(UPDATES):
            new = _leaves(rng, count)
            leaves[first: first + count] = new
            data = b"".join(new)
            if k % 3 == 1:
                data = np.frombuffer(data, dtype=np.uint8).reshape(count, 32)
            elif k % 3 == 2:
                data = ctx.to_device(np.frombuffer(data, dtype=np.uint8)).reshape(count, 32)
            tree.set_leaves(first, data)
            launches, ms, rows = ctx.timing_drain("merkle_level")
            want = _expected_rows(depth, first, count)
            assert want[0] == level1 and want[-1] == 1
            assert (launches, rows) == (depth, sum(want)), (first, count)
            _assert_tree(tree, ref_tree(leaves), (first, count))
        tree.set_leaves(7, b"")  # count = 0: nothing
        assert ctx.timing_drain("merkle_level")[0] == 0
        ctx.set_timing(False)
        _assert_tree(tree, ref_tree(leaves), "count 0")
    finally:
        ctx.set_timing(False)
        tree.close()


def test_leaves_as_bytes_numpy_and_device_tensor(ctx):
    depth = 3
    leaves = _leaves(np.random.default_rng(1202), 8)
    levels = ref_tree(leaves)
    raw = b"".join(leaves)
    arr = np.frombuffer(raw, dtype=np.uint8).reshape(8, 32)
    for what, data in [("bytes", raw), ("bytearray", bytearray(raw)), ("numpy", arr), ("tensor", ctx.to_device(arr).reshape(8, 32))]:
        tree = ctx.merkle_tree(depth)
        try:
            tree.set_leaves(0, data)
            _assert_tree(tree, levels, what)
        finally:
            tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. paths
def _siblings(levels, i):
    return [levels[l][(i >> l) ^ 1] for l in range(len(levels) - 1)]


@pytest.mark.parametrize("depth", [1, 2, 7, 8, 9, 12])
def test_paths(ctx, ref12, depth):
    n = 1 << depth
    if depth == 12:
        leaves, levels = ref12
    else:
        leaves = _leaves(np.random.default_rng(300 + depth), n)
        levels = ref_tree(leaves)
    rng = np.random.default_rng(400 + depth)
    idx = [0, 1, n - 1] + [int(x) for x in rng.integers(0, n, size=29)]
    idx.append(idx[5])  # a repeat at every depth
    assert len(idx) == 33
    st = _statement(depth)
    nin = 256 + 256 * (depth + 1) + depth
    rowb = 32 + 32 * (depth + 1) + (depth + 7) // 8
    assert rowb == (nin + 7) // 8
    want = np.stack([st.bits(leaves[i], _siblings(levels, i), i) for i in idx])
    assert want.shape == (33, nin)
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, b"".join(leaves))
        assert tree.nin == nin
        got = tree.path_bits(idx)
        assert got.dtype == np.uint8 and got.shape == (33, nin)
        assert np.array_equal(got, want)
        rows = tree.path_rows(idx)
        assert rows.shape == (33, rowb)
        assert np.array_equal(rows, np.packbits(want, axis=1, bitorder="little"))  # (the last byte's bits past nin are zero)
        # a wider row through the C call: the bytes past ceil(nin / 8) are left alone
        stride = rowb + 13
        buf = np.full((33, stride), 0xAB, dtype=np.uint8)
        iu = np.array(idx, dtype=np.uint32)
        rc = ctx.lib.mfh_merkle_paths(ctx._h, tree._h, 33, ctypes.c_void_p(iu.ctypes.data), ctypes.c_void_p(buf.ctypes.data), stride)
        assert rc == 0
        assert np.array_equal(buf[:, :rowb], rows)
        assert (buf[:, rowb:] == 0xAB).all()
        # the pinned staging zeroed between two calls changes nothing
        assert ctx.scrub_staging() == 0
        assert np.array_equal(tree.path_rows(idx), rows)
    finally:
        tree.close()


def _unpack_row(row, depth):
    """(leaf, siblings, index) of a packed row"""
    def node(k):
        b = bytes(row[32 + 32 * k: 64 + 32 * k])
        return b"".join(b[i: i + 4][::-1] for i in range(0, 32, 4))

    return node(0), [node(1 + l) for l in range(depth)], int.from_bytes(bytes(row[32 + 32 * (depth + 1):]), "little")


def test_paths_two_chunks(ctx):
    import torch

    depth, nb = 16, 116108
    rowb = 32 + 32 * (depth + 1) + 2
    assert rowb == 578 and (64 << 20) // rowb == 116105  # statements per chunk: the call below runs 116 105 + 3
    g = torch.Generator(device="cpu")
    g.manual_seed(1600)
    leaves = torch.randint(0, 256, (1 << depth, 32), dtype=torch.uint8, generator=g).to(ctx.device)
    rng = np.random.default_rng(1601)
    idx = rng.integers(0, 1 << depth, size=nb).astype(np.uint32)
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, leaves)
        ctx.set_timing(True)
        rows = tree.path_rows(idx)
        launches, ms, total = ctx.timing_drain("merkle_paths")
        ctx.set_timing(False)
        print(f"depth 16: {nb} paths in {launches} launches of k_merkle_paths: {ms:.3f} ms")
        assert (launches, total) == (2, nb)
        assert rows.shape == (nb, rowb) and not rows[:, :32].any()
        root = tree.root()
        host = leaves.cpu().numpy()
        picks = [0, 116104, 116105, 116106, nb - 1] + [int(x) for x in rng.integers(0, nb, size=32)]
        for b in picks:
            leaf, sibs, index = _unpack_row(rows[b], depth)
            assert index == int(idx[b]) and leaf == host[index].tobytes(), b
            assert ref.merkle_root(leaf, sibs, index) == root, b
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. MFH_EINVAL
def test_einval(ctx, ref12):
    import torch

    lib, h = ctx.lib, ctx._h
    depth = 12
    leaves, levels = ref12
    tree = ctx.merkle_tree(depth)
    texts = []

    def refused(rc, who):
        assert rc == EINVAL, who
        text = lib.mfh_last_error(h).decode()
        assert text.startswith(who + ": "), text
        texts.append(text)

    try:
        tree.set_leaves(0, b"".join(leaves))
        ctx.sync()
        ctx.set_timing(True)
        vp = ctypes.c_void_p
        # create
        for d in (0, 25, 0xFFFFFFFF):
            out = vp(0x1234)
            refused(lib.mfh_merkle_create(h, d, ctypes.byref(out)), "mfh_merkle_create")
            assert out.value == 0x1234
        refused(lib.mfh_merkle_create(h, 3, None), "mfh_merkle_create")
        assert lib.mfh_merkle_create(None, 3, ctypes.byref(vp())) == EINVAL
        # set_leaves
        d_new = torch.full((64,), 0xEE, dtype=torch.uint8, device=ctx.device)
        refused(lib.mfh_merkle_set_leaves(h, None, 0, 1, vp(d_new.data_ptr())), "mfh_merkle_set_leaves")
        refused(lib.mfh_merkle_set_leaves(h, tree._h, 0, 1, None), "mfh_merkle_set_leaves")
        for first, count in [(1 << depth, 1), ((1 << depth) - 1, 2), (0, (1 << depth) + 1), (0xFFFFFFFF, 2), (1 << depth, 0xFFFFFFFF)]:
            refused(lib.mfh_merkle_set_leaves(h, tree._h, first, count, vp(d_new.data_ptr())), "mfh_merkle_set_leaves")
        assert lib.mfh_merkle_set_leaves(None, tree._h, 0, 1, vp(d_new.data_ptr())) == EINVAL
        # root
        root = (ctypes.c_uint8 * 32)(*([0xAB] * 32))
        refused(lib.mfh_merkle_root(h, None, root), "mfh_merkle_root")
        refused(lib.mfh_merkle_root(h, tree._h, None), "mfh_merkle_root")
        assert lib.mfh_merkle_root(None, tree._h, root) == EINVAL
        assert bytes(root) == b"\xab" * 32
        # nodes
        p = vp(0x1234)
        assert lib.mfh_merkle_nodes(None, 0, ctypes.byref(p)) == EINVAL
        refused(lib.mfh_merkle_nodes(tree._h, 0, None), "mfh_merkle_nodes")
        refused(lib.mfh_merkle_nodes(tree._h, depth + 1, ctypes.byref(p)), "mfh_merkle_nodes")
        assert p.value == 0x1234
        # paths
        rowb = 32 + 32 * (depth + 1) + 2
        idx = np.array([5, 0, 4095], dtype=np.uint32)
        bad = np.array([5, 0, 4096], dtype=np.uint32)
        buf = np.full((3, rowb + 4), 0xAB, dtype=np.uint8)
        ip, bp, xp = vp(idx.ctypes.data), vp(buf.ctypes.data), vp(bad.ctypes.data)
        refused(lib.mfh_merkle_paths(h, None, 3, ip, bp, buf.shape[1]), "mfh_merkle_paths")
        refused(lib.mfh_merkle_paths(h, tree._h, 3, None, bp, buf.shape[1]), "mfh_merkle_paths")
        refused(lib.mfh_merkle_paths(h, tree._h, 3, ip, None, buf.shape[1]), "mfh_merkle_paths")
        refused(lib.mfh_merkle_paths(h, tree._h, 3, xp, bp, buf.shape[1]), "mfh_merkle_paths")
        refused(lib.mfh_merkle_paths(h, tree._h, 3, ip, bp, rowb - 1), "mfh_merkle_paths")
        assert lib.mfh_merkle_paths(None, tree._h, 3, ip, bp, buf.shape[1]) == EINVAL
        assert (buf == 0xAB).all()
        # a tree of another device, where there is one
        if torch.cuda.device_count() > 1:
            import c_lwe_snarks_amd as m

            other = m.Context(m.DEBUG, 1)
            try:
                oh = other._h
                for rc, who in [(lib.mfh_merkle_set_leaves(oh, tree._h, 0, 1, vp(d_new.data_ptr())), "mfh_merkle_set_leaves"),
                                (lib.mfh_merkle_root(oh, tree._h, root), "mfh_merkle_root"),
                                (lib.mfh_merkle_paths(oh, tree._h, 3, ip, bp, buf.shape[1]), "mfh_merkle_paths")]:
                    assert rc == EINVAL
                    assert lib.mfh_last_error(oh).decode() == who + ": the tree belongs to another device"
                assert bytes(root) == b"\xab" * 32 and (buf == 0xAB).all()
            finally:
                other.close()
                torch.cuda.set_device(ctx.device)  # (the other context's calls made its device HIP's current one)
        # each case has a text of its own (the depths of create share theirs, and so do the ranges of set_leaves)
        assert len(set(texts)) == 2 + 3 + 2 + 2 + 5, sorted(set(texts))
        # nothing was launched, nothing changed
        assert ctx.timing_drain("merkle_level")[0] == 0 and ctx.timing_drain("merkle_paths")[0] == 0
        ctx.set_timing(False)
        _assert_tree(tree, levels, "after the refused calls")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. one root, many proofs
def _flip(bits: bytes, bit: int) -> bytes:
    b = bytearray(bits)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def test_one_root_many_proofs(gpu_ctx_factory, mf, W):
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    st = W.MerklePath(2)
    cc = st.circuit.compile(p)
    lu = cc.lu
    rng = np.random.default_rng(1700)
    leaves = _leaves(rng, 4)
    tree = ctx.merkle_tree(2)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        tree.set_leaves(0, b"".join(leaves))
        idx = [0, 1, 2, 3] + [int(x) for x in rng.integers(0, 4, size=29)]
        witness, holds = ctx.circuit_assign(prog, tree.path_bits(idx))
        root = tree.root()
        assert root == ref_tree(leaves)[-1][0]
        assert holds.all()
        for b in range(len(idx)):
            assert st.root_of(witness[b]) == root, b
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count.any() and (first == 0xFFFFFFFF).all()

        ctx.ssp_prepare(None)
        alpha, beta, s = (int(x) for x in rng.integers(1, C.P, size=3, dtype=np.uint64))
        d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
        d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
        d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, d_err).clone()
        vk = ctx.derive_vk(None, s, lu)

        def prove(rows):
            k = len(rows)
            deltas = [int(x) for x in rng.integers(0, C.P, size=k, dtype=np.uint64)]
            mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(k)]
            signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(k)]
            return ctx.prove_batch_public(d_crs, None, lu, [r.tobytes() for r in rows], deltas, mags, signs).clone()

        def verify(proofs, statement, k):
            return [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, [statement] * k), np.uint8)]

        proofs = prove([witness[b] for b in range(4)])  # one per leaf
        stmt = st.statement(root)
        assert stmt == witness[0][:32].tobytes()
        assert verify(proofs, stmt, 4) == [True] * 4  # the SAME statement for all four
        assert verify(proofs, st.statement(_flip(root, 77)), 4) == [False] * 4

        new_leaf = rng.bytes(32)
        tree.set_leaves(2, new_leaf)
        leaves[2] = new_leaf
        root2 = tree.root()
        assert root2 == ref_tree(leaves)[-1][0] and root2 != root
        stmt2 = st.statement(root2)
        assert verify(proofs, stmt2, 4) == [False] * 4
        witness2, holds2 = ctx.circuit_assign(prog, tree.path_bits([2, 0]))
        assert holds2.all() and st.root_of(witness2[0]) == root2 and st.root_of(witness2[1]) == root2
        fresh = prove([witness2[0], witness2[1]])  # index 2: a new leaf; index 0: the same leaf, a new path
        assert verify(fresh, stmt2, 2) == [True, True]
        assert verify(fresh, stmt, 2) == [False, False]
    finally:
        prog.close()
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. ordering
def _late(ctx, raw):
    """raw on the device as the OUTPUT of a few milliseconds of unrelated work on torch's current stream (24 passes over 128 MB, then a write that depends
    on them): whatever reads it out of the stream's order reads the 0x5A filler"""
    import torch

    t = ctx.to_device(np.frombuffer(raw, dtype=np.uint8))
    out = torch.full_like(t, 0x5A)
    x = torch.zeros(1 << 25, dtype=torch.float32, device=ctx.device)
    for _ in range(24):
        x.mul_(0.5).add_(1.0)
    gate = (x[:1] < 0).to(torch.uint8)  # 0, known when the passes are done
    torch.bitwise_xor(t, gate, out=out)
    return out


def _overlapping_updates(ctx, ref12):
    leaves = list(ref12[0])
    rng = np.random.default_rng(1800)
    a, b = _leaves(rng, 300), _leaves(rng, 400)
    tree = ctx.merkle_tree(12)
    try:
        d_all, d_a, d_b = _late(ctx, b"".join(leaves)), _late(ctx, b"".join(a)), _late(ctx, b"".join(b))
        tree.set_leaves(0, d_all)
        tree.set_leaves(100, d_a)
        tree.set_leaves(250, d_b)  # overlaps [250, 400) of the one before
        root = tree.root()  # no wait before it
        leaves[100:400] = a
        leaves[250:650] = b
        levels = ref_tree(leaves)
        assert root == levels[-1][0]
        _assert_tree(tree, levels, "overlapping updates")
    finally:
        tree.close()


def test_ordering_null_stream(ctx, ref12):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _overlapping_updates(ctx, ref12)


def test_ordering_callers_stream(gpu_ctx_factory, mf, ref12):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _overlapping_updates(c, ref12)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()
