"""GPU: SHA-256 of whole records on the device (mfh_sha256_records, mfh_merkle_set_records: k_sha256_records), the record rows of words.MerkleRecord,
and Sha256Message.statement, against hashlib and the pure-Python tree of tests/sha256_ref.py.

1. sha256_records against hashlib, every record compared: lengths {0, 1, 3, 55, 56, 63, 64, 65, 119, 120, 128, 200} x counts {1, 63, 64, 65, 255, 256, 257,
   513} packed at a base offset of one byte; then strides {length, length + 1, length + 7, the next multiple of 64} x base offsets {0, 1, 2, 3} at counts
   257 and 513.  The records lie in one tensor with 16 + offset bytes before the span and 64 after it (valid memory: the bound on reads is pinned by
   tests/test_sha256_records_host_cpu.py and the kernel's clipped loads, not probed here); gaps and surroundings are 0xFF, and one case is repeated with
   them zero: the digests are the same, so no byte outside a record enters a digest.  A numpy array and a column slice of a wider table (no copy) too.
2. set_records at (first, count) in {(0, all), (1, 1), (255, 2), (256, 256), (last, 1)} -- those that fit -- in trees of depth 1, 2, 9 and 12: the leaves
   equal hashlib, every node of every level equals the reference, untouched leaves are unchanged; "merkle_level" shows `depth` launches with the parent
   counts set_leaves would give, "sha256_records" one launch of `count` rows.
3. record_bits equals MerkleRecord(length, depth).bits(record, siblings, index) built from nodes(), repeated indices among them.
4. end to end at MerkleRecord(5, 1), d = 2^17: 33 statements of one tree hold with the tree's root, no row is violated, four proofs verify under the one
   statement of that root and fail under the root after another record was set; a row with a record that is not in the tree assigns to another root.
5. two Sha256Message(56) proofs verify against Sha256Message.statement(d) for d from sha256_records and fail against each other's digest.
6. every MFH_EINVAL case through the raw C calls: the code, a text naming the function, nothing launched or written.
7. ordering: set_records from a device tensor written on the context's stream just before the call, on the null stream and on a caller's stream."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import sha256_ref as ref

pytestmark = pytest.mark.gpu

SEED = bytes((31 * i + 5) & 0xFF for i in range(40))
EINVAL = -1
LENGTHS = [0, 1, 3, 55, 56, 63, 64, 65, 119, 120, 128, 200]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]


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
    return gpu_ctx_factory()  # (hashing does not depend on the parameters)


# ---------------------------------------------------------------------------------------------------------------- the reference side
_parent = functools.lru_cache(maxsize=None)(ref.merkle_parent)


def ref_tree(leaves):
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([_parent(cur[j], cur[j + 1]) for j in range(0, len(cur), 2)])
    return levels


def _digests(records):
    return np.frombuffer(b"".join(hashlib.sha256(bytes(r)).digest() for r in records), dtype=np.uint8).reshape(len(records), 32)


@functools.lru_cache(maxsize=None)
def _random_records(length, count):
    """count random records of `length` bytes, shared by the cases of one shape and never changed"""
    a = np.random.default_rng(5000 + 7 * length + count).integers(0, 256, size=(count, length), dtype=np.uint8)
    a.setflags(write=False)
    return a, _digests(a)


def _placed(ctx, records, stride, offset, fill=0xFF):
    """the records as a [n, length] view of one device tensor: 16 + offset bytes of `fill`, the records at `stride` (gaps of `fill`), 64 bytes of `fill`"""
    import torch

    n, length = records.shape
    base = 16 + offset
    span = (n - 1) * stride + length
    host = np.full(base + span + 64, fill, dtype=np.uint8)
    for r in range(n):
        host[base + r * stride: base + r * stride + length] = records[r]
    buf = ctx.to_device(host)
    view = torch.as_strided(buf, (n, length), (stride, 1), base)
    assert not length or view.data_ptr() == buf.data_ptr() + base
    return view


def _strides(length):
    return [length, length + 1, length + 7, (length // 64 + 1) * 64]


# ---------------------------------------------------------------------------------------------------------------- 1. sha256_records
@pytest.mark.parametrize("length", LENGTHS)
def test_digests_equal_hashlib_lengths_by_counts(ctx, length):
    for count in COUNTS:
        records, want = _random_records(length, count)
        got = ctx.sha256_records(_placed(ctx, records, length, 1))
        assert tuple(got.shape) == (count, 32) and got.device == ctx.device
        assert np.array_equal(got.cpu().numpy(), want), (length, count)


@pytest.mark.parametrize("length", LENGTHS)
def test_digests_equal_hashlib_strides_by_offsets(ctx, length):
    for count in (257, 513):
        records, want = _random_records(length, count)
        for stride in _strides(length):
            for offset in range(4):
                got = ctx.sha256_records(_placed(ctx, records, stride, offset))
                assert np.array_equal(got.cpu().numpy(), want), (length, count, stride, offset)


@pytest.mark.parametrize("length,stride,offset", [(55, 62, 3), (119, 120, 1), (3, 10, 2)])
def test_bytes_outside_a_record_enter_no_digest(ctx, length, stride, offset):
    records, want = _random_records(length, 257)
    ff = ctx.sha256_records(_placed(ctx, records, stride, offset, fill=0xFF)).cpu().numpy()
    zero = ctx.sha256_records(_placed(ctx, records, stride, offset, fill=0x00)).cpu().numpy()
    assert np.array_equal(ff, zero) and np.array_equal(ff, want)


def test_known_digests(ctx):
    got = ctx.sha256_records(np.frombuffer(b"abc", dtype=np.uint8).reshape(1, 3)).cpu().numpy()
    assert got.tobytes().hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"  # FIPS 180-4's example
    empty = ctx.sha256_records(np.zeros((2, 0), dtype=np.uint8)).cpu().numpy()
    assert empty[0].tobytes() == empty[1].tobytes() == hashlib.sha256(b"").digest()
    assert tuple(ctx.sha256_records(np.zeros((0, 7), dtype=np.uint8)).shape) == (0, 32)


def test_numpy_and_a_column_slice_without_a_copy(ctx, mf):
    import torch

    records, want = _random_records(55, 257)
    assert np.array_equal(ctx.sha256_records(np.array(records)).cpu().numpy(), want)
    table = torch.full((257, 96), 0xFF, dtype=torch.uint8, device=ctx.device)
    table[:, 9: 64] = ctx.to_device(records).reshape(257, 55)
    cols = table[:, 9: 64]
    assert cols.data_ptr() == table.data_ptr() + 9 and cols.stride() == (96, 1) and not cols.is_contiguous()
    assert np.array_equal(ctx.sha256_records(cols).cpu().numpy(), want)
    for bad in (table[:, 9: 64].to(torch.int8), table[:, 9: 64: 2], table.t(), table[0], table.cpu()):
        with pytest.raises(mf.MfhError):
            ctx.sha256_records(bad)
    with pytest.raises(mf.MfhError):
        ctx.sha256_records(np.zeros((3, 5), dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------- 2. set_records
def _assert_tree(tree, levels, what=""):
    assert len(levels) == tree.depth + 1
    for l, want in enumerate(levels):
        got = tree.nodes(l)
        assert tuple(got.shape) == (1 << (tree.depth - l), 32)
        assert got.cpu().numpy().tobytes() == b"".join(want), (what, l)
    assert tree.root() == levels[-1][0], what


def _expected_rows(depth, first, count):
    return [((first + count - 1) >> l) - (first >> l) + 1 for l in range(1, depth + 1)]


@pytest.mark.parametrize("depth", [1, 2, 9, 12])
def test_set_records(ctx, depth):
    n = 1 << depth
    rng = np.random.default_rng(900 + depth)
    leaves = [rng.bytes(32) for _ in range(n)]
    cases = [(f, c) for f, c in [(0, n), (1, 1), (255, 2), (256, 256), (n - 1, 1)] if f + c <= n]
    assert len(cases) == (5 if depth >= 9 else 3)
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_leaves(0, b"".join(leaves))
        ctx.set_timing(True)
        for k, (first, count) in enumerate(cases):
            length = (55, 70, 3, 120, 64)[k]
            records = rng.integers(0, 256, size=(count, length), dtype=np.uint8)
            before = tree.nodes(0).cpu().numpy().copy()
            if k % 2:
                tree.set_records(first, records)  # a host array, uploaded and kept until a call that waits
            else:
                tree.set_records(first, _placed(ctx, records, length + k + 1, k & 3))
            launches, _, rows = ctx.timing_drain("merkle_level")
            assert (launches, rows) == (depth, sum(_expected_rows(depth, first, count))), (first, count)
            assert ctx.timing_drain("sha256_records")[::2] == (1, count), (first, count)
            want = _digests(records)
            after = tree.nodes(0).cpu().numpy()
            assert np.array_equal(after[first: first + count], want), (first, count)
            assert np.array_equal(after[:first], before[:first]) and np.array_equal(after[first + count:], before[first + count:])
            leaves[first: first + count] = [want[i].tobytes() for i in range(count)]
            _assert_tree(tree, ref_tree(leaves), (first, count))
        tree.set_records(n - 1, np.zeros((0, 9), dtype=np.uint8))  # count = 0: nothing
        assert ctx.timing_drain("merkle_level")[0] == 0 and ctx.timing_drain("sha256_records")[0] == 0
        ctx.set_timing(False)
        _assert_tree(tree, ref_tree(leaves), "count 0")
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 3. record rows
@pytest.mark.parametrize("length,depth", [(3, 2), (55, 3), (56, 2), (64, 9)])
def test_record_bits(ctx, W, length, depth):
    n = 1 << depth
    records, digests = _random_records(length, n)
    rng = np.random.default_rng(300 + depth)
    idx = [0, 1, n - 1] + [int(x) for x in rng.integers(0, n, size=9)]
    idx += [idx[4], 0]  # repeats
    st = W.MerkleRecord(length, depth)
    nin = 256 + 8 * length + 257 * depth
    tree = ctx.merkle_tree(depth)
    try:
        tree.set_records(0, np.array(records))
        levels = [tree.nodes(l).cpu().numpy() for l in range(depth + 1)]
        assert np.array_equal(levels[0], digests)
        want = np.stack([st.bits(records[i].tobytes(), [levels[l][(i >> l) ^ 1].tobytes() for l in range(depth)], i) for i in idx])
        assert want.shape == (len(idx), nin)
        got = tree.record_bits(records[idx], idx)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
        rows = tree.record_rows([records[i].tobytes() for i in idx], idx)  # bytes-likes as well
        assert rows.shape == (len(idx), (nin + 7) // 8)
        assert np.array_equal(rows, np.packbits(want, axis=1, bitorder="little"))
        assert np.array_equal(rows[:, 32 + length:], tree.path_rows(idx)[:, 64:]) and not rows[:, :32].any()
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. end to end
def _flip(bits: bytes, bit: int) -> bytes:
    b = bytearray(bits)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def _prover(ctx, p, rng, lu):
    """(prove, verify) of a context whose SSP rows are set: a fresh key and CRS"""
    import oracle_lib as ol

    from c_lwe_snarks_amd import circuit as C

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

    def verify(proofs, statements):
        return [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, proofs, list(statements)), np.uint8)]

    return prove, verify


def test_record_membership_end_to_end(gpu_ctx_factory, mf, W):
    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    st = W.MerkleRecord(5, 1)
    cc = st.circuit.compile(p)
    lu = cc.lu
    rng = np.random.default_rng(1900)
    records = rng.integers(0, 256, size=(2, 5), dtype=np.uint8)
    tree = ctx.merkle_tree(1)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        tree.set_records(0, records)
        idx = [0, 1] + [int(x) for x in rng.integers(0, 2, size=31)]
        witness, holds = ctx.circuit_assign(prog, tree.record_bits(records[idx], idx))
        root = tree.root()
        leaves = [hashlib.sha256(records[i].tobytes()).digest() for i in range(2)]
        assert root == ref.merkle_parent(*leaves)
        assert holds.all()
        for b in range(len(idx)):
            assert st.root_of(witness[b]) == root, b
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        count, first = ctx.ssp_rows_violations(witness)
        assert not count.any() and (first == 0xFFFFFFFF).all()

        prove, verify = _prover(ctx, p, rng, lu)
        proofs = prove([witness[b] for b in range(4)])
        stmt = st.statement(root)
        assert stmt == witness[0][:32].tobytes()
        assert verify(proofs, [stmt] * 4) == [True] * 4  # the SAME statement for all four
        assert verify(proofs, [st.statement(_flip(root, 77))] * 4) == [False] * 4

        # a record that is not in the tree, with the path of leaf 1: another root
        stranger = rng.integers(0, 256, size=(1, 5), dtype=np.uint8)
        w2, h2 = ctx.circuit_assign(prog, tree.record_bits(stranger, [1]))
        assert h2.all() and st.root_of(w2[0]) == ref.merkle_parent(leaves[0], hashlib.sha256(stranger[0].tobytes()).digest()) != root
        assert verify(prove([w2[0], witness[1]]), [stmt, stmt]) == [False, True]

        # the tree after that record was set: the old proofs fail under the new root
        tree.set_records(1, stranger)
        root2 = tree.root()
        assert root2 == st.root_of(w2[0])
        assert verify(proofs, [st.statement(root2)] * 4) == [False] * 4
    finally:
        prog.close()
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. Sha256Message.statement
def test_message_proofs_verify_against_device_digests(gpu_ctx_factory, mf, W):
    p = mf.Params(d=1 << 17, m=87381)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    st = W.Sha256Message(56)
    cc = st.circuit.compile(p)
    lu = cc.lu
    rng = np.random.default_rng(1950)
    messages = rng.integers(0, 256, size=(2, 56), dtype=np.uint8)
    prog = ctx.circuit_load(cc, state="auto")
    try:
        digests = ctx.sha256_records(messages).cpu().numpy()
        assert np.array_equal(digests, _digests(messages)) and digests[0].tobytes() != digests[1].tobytes()
        witness, holds = ctx.circuit_assign(prog, np.stack([st.bits(m.tobytes()) for m in messages]))
        assert holds.all()
        ctx.ssp_set_rows(cc.rows, lu_max=lu)
        prove, verify = _prover(ctx, p, rng, lu)
        proofs = prove([witness[0], witness[1]])
        stmts = [W.Sha256Message.statement(d.tobytes()) for d in digests]  # from the device digests alone: no witness row
        assert stmts[0] == witness[0][:32].tobytes()
        assert verify(proofs, stmts) == [True, True]
        assert verify(proofs, stmts[::-1]) == [False, False]
    finally:
        prog.close()


# ---------------------------------------------------------------------------------------------------------------- 6. MFH_EINVAL
def test_einval(ctx):
    import torch

    lib, h = ctx.lib, ctx._h
    vp = ctypes.c_void_p
    depth = 9
    rng = np.random.default_rng(1960)
    leaves = [rng.bytes(32) for _ in range(1 << depth)]
    tree = ctx.merkle_tree(depth)
    texts = {"mfh_sha256_records": set(), "mfh_merkle_set_records": set()}

    def refused(rc, who):
        assert rc == EINVAL, who
        text = lib.mfh_last_error(h).decode()
        assert text.startswith(who + ": "), text
        texts[who].add(text)

    try:
        tree.set_leaves(0, b"".join(leaves))
        d_rec = torch.full((4 * 64,), 0x11, dtype=torch.uint8, device=ctx.device)
        d_dig = torch.full((4 * 32 + 16,), 0xAB, dtype=torch.uint8, device=ctx.device)
        rec, dig = d_rec.data_ptr(), d_dig.data_ptr()
        assert dig % 16 == 0
        ctx.sync()
        ctx.set_timing(True)
        big = (1 << 20) + 1
        who = "mfh_sha256_records"
        refused(lib.mfh_sha256_records(h, None, 64, 55, 4, vp(dig)), who)       # records without d_records
        refused(lib.mfh_sha256_records(h, vp(rec), 64, 55, 4, None), who)       # ... without d_digests
        refused(lib.mfh_sha256_records(h, vp(rec), 54, 55, 4, vp(dig)), who)    # stride < length
        refused(lib.mfh_sha256_records(h, vp(rec), big, big, 1, vp(dig)), who)  # length above the limit
        for mis in (1, 4, 8):
            refused(lib.mfh_sha256_records(h, vp(rec), 64, 55, 4, vp(dig + mis)), who)  # d_digests not 16-byte aligned
        assert lib.mfh_sha256_records(None, vp(rec), 64, 55, 4, vp(dig)) == EINVAL
        assert len(texts[who]) == 5, sorted(texts[who])
        who = "mfh_merkle_set_records"
        refused(lib.mfh_merkle_set_records(h, None, 0, 4, vp(rec), 64, 55), who)       # a null tree
        refused(lib.mfh_merkle_set_records(h, tree._h, 0, 4, None, 64, 55), who)       # records without d_records
        refused(lib.mfh_merkle_set_records(h, tree._h, 0, 4, vp(rec), 54, 55), who)    # stride < length
        refused(lib.mfh_merkle_set_records(h, tree._h, 0, 1, vp(rec), big, big), who)  # length above the limit
        for first, count in [(1 << depth, 1), ((1 << depth) - 1, 2), (0, (1 << depth) + 1), (0xFFFFFFFF, 2), (1 << depth, 0xFFFFFFFF)]:
            refused(lib.mfh_merkle_set_records(h, tree._h, first, count, vp(rec), 64, 55), who)  # first + count > 2^depth
        assert lib.mfh_merkle_set_records(None, tree._h, 0, 4, vp(rec), 64, 55) == EINVAL
        assert len(texts[who]) == 5, sorted(texts[who])
        # a tree of another device, where there is one
        if torch.cuda.device_count() > 1:
            import c_lwe_snarks_amd as m

            other = m.Context(m.DEBUG, 1)
            try:
                assert lib.mfh_merkle_set_records(other._h, tree._h, 0, 4, vp(rec), 64, 55) == EINVAL
                assert lib.mfh_last_error(other._h).decode() == "mfh_merkle_set_records: the tree belongs to another device"
            finally:
                other.close()
                torch.cuda.set_device(ctx.device)
        # nothing was launched, nothing was written
        assert ctx.timing_drain("sha256_records")[0] == 0 and ctx.timing_drain("merkle_level")[0] == 0
        ctx.set_timing(False)
        assert (d_dig.cpu().numpy() == 0xAB).all() and (d_rec.cpu().numpy() == 0x11).all()
        _assert_tree(tree, ref_tree(leaves), "after the refused calls")
        # the limit itself is accepted: one record of 2^20 bytes (16 385 blocks)
        one = torch.zeros(1 << 20, dtype=torch.uint8, device=ctx.device)
        got = ctx.sha256_records(one.reshape(1, -1)).cpu().numpy()
        assert got.tobytes() == hashlib.sha256(bytes(1 << 20)).digest()
    finally:
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. ordering
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


def _records_behind_late_inputs(ctx):
    depth, length = 9, 61
    n = 1 << depth
    records, digests = _random_records(length, n)
    newer, newer_digests = _random_records(length, 300)
    tree = ctx.merkle_tree(depth)
    try:
        d_all = _late(ctx, records.tobytes()).reshape(n, length)
        d_new = _late(ctx, newer.tobytes()).reshape(300, length)
        tree.set_records(0, d_all)
        tree.set_records(100, d_new)  # overlaps the one before
        level0 = tree.nodes(0).clone()  # behind the same stream: no wait before it
        root = tree.root()
        leaves = [digests[i].tobytes() for i in range(n)]
        leaves[100:400] = [newer_digests[i].tobytes() for i in range(300)]
        levels = ref_tree(leaves)
        assert level0.cpu().numpy().tobytes() == b"".join(leaves)
        assert root == levels[-1][0]
        _assert_tree(tree, levels, "records behind late inputs")
    finally:
        tree.close()


def test_ordering_null_stream(ctx):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _records_behind_late_inputs(ctx)


def test_ordering_callers_stream(gpu_ctx_factory, mf):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _records_behind_late_inputs(c)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()
