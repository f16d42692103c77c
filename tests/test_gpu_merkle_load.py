"""GPU: the bulk load and the invariant check of an indexed table (mfh_merkle_load_keys, mfh_merkle_check_table; key_sort = k_sort_tiles + k_sort_merge,
k_load_entries, k_load_dups, k_load_records, k_check_entries, k_chain_check, k_leaf_check, k_node_check; MerkleTree.load_keys / check_table) against
words.indexed_records, words.indexed_check, hashlib and a tree computed here (numpy over tests/sha256_ref.py's constants; the pure-Python model at depth 3).

1. depth 3: K in 1, 4, 5, 8, 17, 32, length 2K and 2K + 7, 0, 1, 2, 5, 7 members in shuffled order, in a misaligned strided table: table, gaps, every level.
2. tile, wave and pass edges: depth 13, K = 8 and 32, nk from 63 to 8 191, keys random / ascending / descending / sharing their first K - 1 bytes (nk <= 254:
   a last byte has no more values), payloads of 0, 1 and 23 bytes.
3. refusals by status: duplicates (neighbours in the input; in different tiles), two duplicated keys, sentinel keys, both: the exact `where`, nothing written.
4. MFH_EINVAL: nothing written, nothing launched.
5. check_table on good tables: after load_keys (the live counts of case 2 among them) and after insert / remove / transfer / adjust batches at depth 9.
6. check_table on broken tables at depth 10: the chain defects of tests/test_merkle_check_cpu.py against words.indexed_check; payload, leaf and node flips.
7. round trip: load_keys, then remove_keys of all of it in two batches.
8. keys produced late on the stream, on the null stream and on a caller's; scrubbed staging.
9. launch counts by timing kind."""
import ctypes
import hashlib

import numpy as np
import pytest

import merkle_climb_model as CM
import sha256_ref
from test_gpu_merkle import _assert_tree, _late
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

EINVAL = -1
NEW_KINDS = ("merkle_sort", "merkle_load", "merkle_check")
KINDS = NEW_KINDS + ("merkle_level", "sha256_records", "merkle_range", "merkle_range_order", "merkle_inert", "merkle_locate")
EDGES = [63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5123, 8191]
TILE = 1024  # mf::kSortTile (csrc/merkle_sort.hpp; tests/test_merkle_sort_host_cpu.py reads it from the header)


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


# ---- the tree, vectorised: parent = compress(IV, left || right) over a whole level at once
def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _parents(nodes):
    """uint8 [2n, 32] -> uint8 [n, 32]"""
    w = list(nodes.reshape(-1, 64).view(">u4").astype(np.uint32).T)
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> np.uint32(3))
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> np.uint32(10))
        w.append(w[t - 16] + s0 + w[t - 7] + s1)
    iv = [np.full(len(w[0]), v, dtype=np.uint32) for v in sha256_ref.IV]
    a, b, c, d, e, f, g, h = iv
    for t in range(64):
        t1 = h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g)) + np.uint32(sha256_ref.K[t]) + w[t]
        t2 = (_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))
        a, b, c, d, e, f, g, h = t1 + t2, a, b, c, d + t1, e, f, g
    out = np.stack([x + y for x, y in zip(iv, (a, b, c, d, e, f, g, h))], axis=1)
    return out.astype(">u4").view(np.uint8).reshape(-1, 32)


def _levels(table):
    """the levels of the tree over a host table, each a list of node bytes, leaves first"""
    cur = np.frombuffer(b"".join(hashlib.sha256(r.tobytes()).digest() for r in table), dtype=np.uint8).reshape(-1, 32)
    levels = [cur]
    while len(cur) > 1:
        cur = _parents(cur)
        levels.append(cur)
    return [[bytes(n) for n in level] for level in levels]


def _keys(rng, K, n, kind="random"):
    """n distinct keys of K bytes, none a sentinel, as uint8 [n, K]"""
    if kind == "prefix":  # one prefix of K - 1 bytes, the last byte differs
        assert n <= 254
        last = rng.choice(np.arange(1, 255), size=n, replace=False).astype(np.uint8)
        return np.concatenate([np.broadcast_to(rng.integers(1, 255, size=K - 1, dtype=np.uint8), (n, K - 1)), last[:, None]], axis=1)
    if K == 1:
        return rng.choice(np.arange(1, 255), size=n, replace=False).astype(np.uint8).reshape(n, 1)
    keys = np.zeros((0, K), dtype=np.uint8)
    while len(keys) < n:
        more = rng.integers(0, 256, size=(2 * n + 8, K), dtype=np.uint8)
        more = more[~((more == 0).all(axis=1) | (more == 0xFF).all(axis=1))]
        keys = np.unique(np.concatenate([keys, more]), axis=0)  # (sorted)
    keys = keys[rng.choice(len(keys), size=n, replace=False)]
    order = np.lexsort(tuple(keys[:, j] for j in range(K - 1, -1, -1)))
    return keys[order] if kind == "ascending" else keys[order[::-1]] if kind == "descending" else keys


def _garbage_table(ctx, rng, depth, length, stride=None, off=0):
    records = [rng.bytes(length) for _ in range(1 << depth)]
    return Placed(ctx, records, stride=stride, off=off), records


def _load_and_compare(ctx, W, tree, placed, keys, payloads, length, what, levels=True):
    want = W.indexed_records(keys, tree.depth, length, None if payloads is None else [bytes(p) for p in payloads])
    assert tree.load_keys(placed.view, keys, payloads) == (0, None), what
    placed.holds([r.tobytes() for r in want], what)  # byte for byte, the gaps of a wider stride and the bytes around the table included
    assert not want[len(keys) + 1:].any()
    if levels:
        _assert_tree(tree, _levels(want), what)
    return want


# ---------------------------------------------------------------------------------------------------------------- 1. depth 3
@pytest.mark.parametrize("K", [1, 4, 5, 8, 17, 32])
def test_depth_3(ctx, W, K):
    rng = np.random.default_rng(21000 + K)
    tree = ctx.merkle_tree(3)
    try:
        for length in (2 * K, 2 * K + 7):
            for n in (0, 1, 2, 5, 7):
                placed, _ = _garbage_table(ctx, rng, 3, length, stride=length + 3, off=1 + n % 3)
                assert placed.view.data_ptr() % 4 == (1 + n % 3) % 4
                keys = _keys(rng, K, n)
                pay = rng.integers(0, 256, size=(n, 7), dtype=np.uint8) if length > 2 * K else None
                want = _load_and_compare(ctx, W, tree, placed, keys, pay, length, (K, length, n))
                model = CM.ClimbModel([hashlib.sha256(r.tobytes()).digest() for r in want])  # the pure-Python model, every level
                _assert_tree(tree, model.levels, (K, length, n))
                assert tree.check_table(placed.view, K) == (0, n + 1, None)
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 2. tile, wave and pass edges
@pytest.fixture(scope="module")
def tree13(ctx):
    tree = ctx.merkle_tree(13)
    yield tree
    tree.close()


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("nk", EDGES)
def test_edges(ctx, W, tree13, K, nk):
    rng = np.random.default_rng(22000 + 10 * nk + K)
    at = EDGES.index(nk)
    for i, kind in enumerate(("random", "ascending", "descending", "prefix")):
        if kind == "prefix" and nk > 254:
            continue
        P = (0, 1, 23)[(i + at) % 3]
        length = 2 * K + P + (at % 2)  # (every other case: a zero byte behind the payload)
        placed, _ = _garbage_table(ctx, rng, 13, length, stride=length + (i % 2), off=i)
        keys = _keys(rng, K, nk, kind)
        pay = rng.integers(0, 256, size=(nk, P), dtype=np.uint8) if P else None
        _load_and_compare(ctx, W, tree13, placed, keys, pay, length, (K, nk, kind, P))
        assert tree13.check_table(placed.view, K) == (0, nk + 1, None), (K, nk, kind)  # (5.: the live counts at every edge)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals by status
def test_refusals_by_status(ctx, W, tree13):
    rng = np.random.default_rng(23000)
    K, length = 8, 19
    placed, records = _garbage_table(ctx, rng, 13, length, stride=length + 2, off=3)
    tree13.set_records(0, placed.view)
    levels = _levels(np.frombuffer(b"".join(records), dtype=np.uint8).reshape(-1, length))
    pay = rng.integers(0, 256, size=(3000, 3), dtype=np.uint8)

    def refused(keys, want, what, payloads=None):
        assert tree13.load_keys(placed.view, keys, payloads) == want, what
        placed.holds(records, what)
        _assert_tree(tree13, levels, what)

    base = _keys(rng, K, 3000)
    order = np.lexsort(tuple(base[:, j] for j in range(K - 1, -1, -1)))  # order[r]: the input index of sorted key r
    keys = base.copy()
    keys[11] = keys[10]
    refused(keys, (1, (10, 11)), "a duplicate, neighbours in the input")
    keys = base.copy()
    keys[2500] = keys[100]  # the copies stand in the first and the third tile of the input
    refused(keys, (1, (100, 2500)), "a duplicate across tiles", pay)
    keys = base.copy()
    keys[int(order[2000])] = keys[int(order[1999])]  # the larger duplicated key ...
    keys[int(order[7])] = keys[int(order[6])]        # ... and the smaller: this one is reported
    refused(keys, (1, tuple(sorted((int(order[6]), int(order[7]))))), "two duplicated keys")
    keys[5] = keys[700] = keys[2999] = keys[int(order[6])]  # three more copies of the smallest duplicated key: the two lowest indices
    refused(keys, (1, tuple(sorted({5, 700, 2999, int(order[6]), int(order[7])})[:2])), "five copies")
    for sentinel in (0x00, 0xFF):
        keys = base.copy()
        keys[1234] = sentinel
        refused(keys, (2, 1234), f"the all-{sentinel:02x} key")
    keys = base.copy()
    keys[2500], keys[77], keys[78] = 0xFF, 0x00, keys[79]
    refused(keys, (2, 77), "both sentinels and a duplicate")
    refused(np.zeros((1, K), dtype=np.uint8), (2, 0), "one key, a sentinel")
    refused(np.stack([base[0], base[0]]), (1, (0, 1)), "two keys, equal")
    # a partial last word: the all-FF key of 5 bytes, and keys that differ from it in the last byte alone
    tree = ctx.merkle_tree(3)
    try:
        placed5, _ = _garbage_table(ctx, rng, 3, 10)
        keys = np.full((3, 5), 0xFF, dtype=np.uint8)
        keys[0, 4], keys[2, 4] = 0xFE, 0xFD
        assert tree.load_keys(placed5.view, keys) == (2, 1)
        keys[1, 4] = 0xFE
        assert tree.load_keys(placed5.view, keys) == (1, (0, 1))
        keys[1, 4] = 0xFC
        assert tree.load_keys(placed5.view, keys) == (0, None)
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 4. MFH_EINVAL
def test_einval(ctx, mf, W):
    rng = np.random.default_rng(24000)
    K, length, depth = 4, 11, 3
    placed, records = _garbage_table(ctx, rng, depth, length, stride=13, off=1)
    tree, other = ctx.merkle_tree(depth), None
    lib, h = ctx.lib, ctx._h
    vp = ctypes.c_void_p
    try:
        tree.set_records(0, placed.view)
        levels = _levels(np.frombuffer(b"".join(records), dtype=np.uint8).reshape(-1, length))
        keys = ctx.to_device(_keys(rng, K, 8)).reshape(8, K)
        pay = ctx.to_device(rng.integers(0, 256, size=(8, 3), dtype=np.uint8))
        status, out = (ctypes.c_uint32 * 3)(7, 7, 7), (ctypes.c_uint32 * 4)(7, 7, 7, 7)
        tp, kp, pp = vp(placed.view.data_ptr()), vp(keys.data_ptr()), vp(pay.data_ptr())
        ctx.sync()
        ctx.set_timing(True)
        texts = []

        def refused(rc, who):
            assert rc == EINVAL
            text = lib.mfh_last_error(h).decode()
            assert text.startswith(who + ": "), text
            texts.append(text)
            assert list(status) == [7, 7, 7] and list(out) == [7, 7, 7, 7]

        load = lambda **kw: lib.mfh_merkle_load_keys(h, kw.get("t", tree._h), kw.get("table", tp), kw.get("stride", 13), kw.get("length", length), kw.get("K", K),
                                                     kw.get("nk", 7), kw.get("keys", kp), kw.get("pay", pp), kw.get("P", 3), kw.get("status", status))
        check = lambda **kw: lib.mfh_merkle_check_table(h, kw.get("t", tree._h), kw.get("table", tp), kw.get("stride", 13), kw.get("length", length), kw.get("K", K),
                                                        kw.get("out", out))
        for kw in (dict(nk=8), dict(K=0), dict(K=33), dict(length=10), dict(P=4), dict(stride=10), dict(table=None), dict(keys=None), dict(P=0), dict(status=None),
                   dict(t=None), dict(length=(1 << 20) + 1, stride=1 << 21)):
            refused(load(**kw), "mfh_merkle_load_keys")
        for kw in (dict(K=0), dict(K=33), dict(length=7), dict(stride=10), dict(table=None), dict(out=None), dict(t=None), dict(length=(1 << 20) + 1, stride=1 << 21)):
            refused(check(**kw), "mfh_merkle_check_table")
        assert len(set(texts)) >= 12
        assert {kind: ctx.timing_drain(kind)[0] for kind in KINDS} == dict.fromkeys(KINDS, 0)
        placed.holds(records, "refusals")
        _assert_tree(tree, levels, "refusals")
        # the legal neighbours of the refusals: nk = 2^depth - 1, NULL payloads with payload_bytes > 0, NULL keys with nk = 0
        assert load(nk=7) == 0 and list(status) == [0, 0xFFFFFFFF, 0xFFFFFFFF]
        assert load(nk=7, pay=None) == 0 and load(nk=0, keys=None, pay=None) == 0
        assert {kind: ctx.timing_drain(kind)[0] > 0 for kind in NEW_KINDS} == {"merkle_sort": True, "merkle_load": True, "merkle_check": False}
        assert check() == 0 and list(out) == [0, 1, 0xFFFFFFFF, 0xFFFFFFFF]
        assert (ctx.timing_drain("merkle_check")[0], ctx.timing_drain("merkle_sort")[0]) == (4 + 3 + depth, 1)
        # the Python methods: the library's text, or the parser's
        view = placed.view
        with pytest.raises(mf.MfhError, match="mfh_merkle_load_keys: more keys"):
            tree.load_keys(view, _keys(rng, K, 8))
        with pytest.raises(mf.MfhError, match="mfh_merkle_load_keys: length shorter"):
            tree.load_keys(view, _keys(rng, K, 2), [b"12345678"] * 2)
        with pytest.raises(W.CircuitError):
            tree.load_keys(view, [b"ab", b"abc"])
        with pytest.raises(W.CircuitError):
            tree.load_keys(view, np.zeros((2, 33), dtype=np.uint8))
        with pytest.raises(mf.MfhError, match="one payload per key"):
            tree.load_keys(view, _keys(rng, K, 2), [b"1"] * 3)
        with pytest.raises(mf.MfhError):
            tree.load_keys(view, keys[:, :3])  # (a device tensor that is not contiguous)
        with pytest.raises(mf.MfhError):
            tree.load_keys(view[:4], _keys(rng, K, 2))
        for bad in (0, 33, 6, 1.5):
            with pytest.raises(mf.MfhError):
                tree.check_table(view, bad)
        assert {kind: ctx.timing_drain(kind)[0] for kind in NEW_KINDS} == dict.fromkeys(NEW_KINDS, 0)
    finally:
        for kind in KINDS:
            ctx.timing_drain(kind)
        ctx.set_timing(False)
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 5. check_table on good tables
def test_check_after_batches(ctx, W):
    rng = np.random.default_rng(25000)
    K, A, length, depth = 8, 8, 27, 9
    tree = ctx.merkle_tree(depth)
    try:
        placed, _ = _garbage_table(ctx, rng, depth, length, stride=length + 1, off=2)
        view = placed.view
        keys = _keys(rng, K, 340)
        members, fresh = keys[:300], keys[300:]
        pay = np.zeros((300, length - 2 * K), dtype=np.uint8)
        pay[:, A - 2: A] = rng.integers(1, 256, size=(300, 2), dtype=np.uint8)  # balances of at most 2 bytes: no overflow
        assert tree.load_keys(view, ctx.to_device(members).reshape(300, K), ctx.to_device(pay).reshape(300, -1)) == (0, None)  # (device tensors, as they are)
        assert tree.check_table(view, K) == (0, 301, None)
        tree.remove_keys(view, members[:50])
        assert tree.check_table(view, K) == (0, 251, None)
        tree.insert_keys(view, fresh)  # into the slots the removes emptied: the slots are no longer in key order
        assert tree.check_table(view, K) == (0, 291, None)
        tree.transfer_keys(view, members[60:80], members[100:120], [1] * 20, A)
        tree.adjust_keys(view, members[200:230], [3] * 30, amount_bytes=A)
        status, live, where = tree.check_table(view, K)
        host = view.cpu().numpy()
        assert (status, live, where) == (0, 291, None) == W.indexed_check(host, K)
        los = [r[:K].tobytes() for r in host if r[:K].tobytes() < r[K: 2 * K].tobytes()]
        assert len(los) == 291 and los != sorted(los)  # the slots are no longer in key order
        assert tree.total_balance(view, K, A)[1] == 291
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 6. check_table on broken tables
def test_check_broken_tables(ctx, W):
    import torch

    rng = np.random.default_rng(26000)
    K, length, depth, n = 5, 13, 10, 600
    tree = ctx.merkle_tree(depth)
    try:
        good = W.indexed_records(_keys(rng, K, n), depth, length, [rng.bytes(3) for _ in range(n)])[rng.permutation(1 << depth)]
        assert W.indexed_check(good, K) == (0, n + 1, None)
        live = np.flatnonzero(good[:, K: 2 * K].any(axis=1))  # (a live record's hi is not zero)
        slot = [int(s) for s in live[np.lexsort(tuple(good[live, j] for j in range(K - 1, -1, -1)))]]  # slot[i]: where sorted live record i stands
        inert = [int(s) for s in np.flatnonzero(~good[:, K: 2 * K].any(axis=1))]
        assert len(slot) == n + 1 and not good[slot[0], :K].any()
        placed = Placed(ctx, [r.tobytes() for r in good], stride=length + 2, off=1)
        view = placed.view
        tree.set_records(0, view)
        assert tree.check_table(view, K) == (0, n + 1, None)

        def planted(edit, want=None, rehash=True):
            """the device table with `edit` applied by index assignments (and the tree built over it): check_table's answer against the model's"""
            host = good.copy()
            for s, col, value in edit(host):
                host[s, col] = value
                view[s, col] = torch.as_tensor(value, dtype=torch.uint8, device=view.device) if np.ndim(value) else int(value)
            if rehash:
                tree.set_records(0, view)
            back = view.cpu().numpy()
            assert np.array_equal(back, host)
            model = W.indexed_check(back, K)  # (of the host copy)
            got = tree.check_table(view, K)
            assert got == model and (want is None or got == want), (got, model, want)
            view.copy_(torch.as_tensor(good, device=view.device))  # (a strided copy: the gaps stay)
            tree.set_records(0, view)

        planted(lambda t: [(slot[0], K - 1, 1)], (1, n + 1, slot[0]))                       # a wrong first lo
        planted(lambda t: [(slot[300], K - 1, t[slot[300], K - 1] ^ 1)], (1, n + 1, slot[300]))      # a gap (or an overlap: the lowest bit of a lo)
        planted(lambda t: [(slot[299], 2 * K - 1, t[slot[299], 2 * K - 1] ^ 1)], (1, n + 1, slot[300]))  # the lowest bit of a hi
        for twin in (inert[0], inert[-1]):                                                      # a duplicated lo: the tie breaks by slot
            planted(lambda t: [(twin, slice(None), t[slot[2]])], (1, n + 2, max(twin, slot[2])))
        planted(lambda t: [(slot[n], 2 * K - 1, 0xFE)], (1, n + 1, slot[n]))                # the last hi
        planted(lambda t: [(slice(None), slice(0, 2 * K), 0)], (1, 0, 0xFFFFFFFF))              # no live record at all
        planted(lambda t: [(slot[17], K - 1, t[slot[17], K - 1] ^ 0x80), (slot[16], 2 * K - 1, t[slot[16], 2 * K - 1] ^ 0x80)], (0, n + 1, None))  # (both ends: still a chain)
        # the last byte of a partial word alone decides (K = 5: byte 4 is word 1's only byte)
        planted(lambda t: [(slot[450], 4, t[slot[450], 4] ^ 0x40)], (1, n + 1, slot[450]))
        # the remaining plants: leaves and nodes (the chain is good)
        view[slot[77], 2 * K + 1] ^= 4                                                          # one flipped payload byte
        assert tree.check_table(view, K) == (2, n + 1, slot[77])
        view[inert[5], length - 1] ^= 1                                                         # ... and an inert slot's byte, lower or higher: the lowest slot
        assert tree.check_table(view, K) == (2, n + 1, min(slot[77], inert[5]))
        view[slot[77], 2 * K + 1] ^= 4
        view[inert[5], length - 1] ^= 1
        assert tree.check_table(view, K) == (0, n + 1, None)
        tree.nodes(0)[333, 31] ^= 1                                                             # one flipped leaf
        assert tree.check_table(view, K) == (2, n + 1, 333)
        tree.nodes(1)[100, 0] ^= 0x80                                                           # ... hides a flipped node
        assert tree.check_table(view, K) == (2, n + 1, 333)
        tree.nodes(0)[333, 31] ^= 1
        assert tree.check_table(view, K) == (3, n + 1, (1, 100))                                # level 1: the node itself is wrong ...
        tree.nodes(1)[100, 0] ^= 0x80
        tree.nodes(3)[9, 7] ^= 2                                                                # level 3: wrong, and so is its parent's check at level 4
        tree.nodes(depth)[0, 0] ^= 1                                                            # ... and the root
        assert tree.check_table(view, K) == (3, n + 1, (3, 9))
        tree.nodes(3)[9, 7] ^= 2
        assert tree.check_table(view, K) == (3, n + 1, (depth, 0))                              # the root's level
        # precedence: chain > leaves > nodes
        view[slot[n], 2 * K - 1] = 0xFE
        tree.nodes(0)[1, 1] ^= 1
        assert tree.check_table(view, K) == (1, n + 1, slot[n])
        view[slot[n], 2 * K - 1] = 0xFF
        assert tree.check_table(view, K) == (2, n + 1, 1)
        tree.nodes(0)[1, 1] ^= 1
        assert tree.check_table(view, K) == (3, n + 1, (depth, 0))
        tree.nodes(depth)[0, 0] ^= 1
        assert tree.check_table(view, K) == (0, n + 1, None)
        placed.holds([r.tobytes() for r in good], "check_table only reads")
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 7. round trip
def test_round_trip(ctx, W):
    rng = np.random.default_rng(27000)
    K, length, depth = 8, 21, 8
    tree = ctx.merkle_tree(depth)
    try:
        placed, _ = _garbage_table(ctx, rng, depth, length, stride=length + 3, off=1)
        keys = _keys(rng, K, 200)
        _load_and_compare(ctx, W, tree, placed, keys, rng.integers(0, 256, size=(200, 5), dtype=np.uint8), length, "round trip")
        tree.remove_keys(placed.view, keys[:120])
        tree.remove_keys(placed.view, keys[120:])
        empty = W.indexed_records(np.zeros((0, K), dtype=np.uint8), depth, length)
        placed.holds([r.tobytes() for r in empty], "the empty set's table")
        _assert_tree(tree, _levels(empty), "the empty set's tree")
        assert tree.check_table(placed.view, K) == (0, 1, None)
    finally:
        tree.close()


# ---------------------------------------------------------------------------------------------------------------- 8. streams
def _late_keys(ctx, W):
    rng = np.random.default_rng(28000)
    K, P, length, depth, n = 8, 3, 20, 12, 3000
    keys, pay = _keys(rng, K, n), rng.integers(0, 256, size=(n, P), dtype=np.uint8)
    want = W.indexed_records(keys, depth, length, [bytes(p) for p in pay])  # (first: nothing of the host's stands between the late keys and the call)
    levels = _levels(want)
    tree = ctx.merkle_tree(depth)
    try:
        placed, _ = _garbage_table(ctx, rng, depth, length, stride=length + 1, off=1)
        d_pay = ctx.to_device(pay).reshape(n, P)
        d_keys = _late(ctx, keys.tobytes()).reshape(n, K)
        assert tree.load_keys(placed.view, d_keys, d_pay) == (0, None)  # no wait before it
        placed.holds([r.tobytes() for r in want], "late keys")
        _assert_tree(tree, levels, "late keys")
        assert ctx.scrub_staging() == 0
        assert tree.check_table(placed.view, K) == (0, n + 1, None)
        assert ctx.scrub_staging() == 0
        assert tree.load_keys(placed.view, keys[::-1], pay[::-1]) == (0, None)
        placed.holds([r.tobytes() for r in want], "after the scrub")
    finally:
        tree.close()


def test_ordering_null_stream(ctx, W):
    import torch

    assert torch.cuda.current_stream().cuda_stream == 0
    _late_keys(ctx, W)


def test_ordering_callers_stream(gpu_ctx_factory, mf, W):
    import torch

    s = torch.cuda.Stream()
    c = gpu_ctx_factory(mf.DEBUG)
    with torch.cuda.stream(s):
        assert s.cuda_stream != 0 and torch.cuda.current_stream() == s
        c.set_stream(s)
        _late_keys(c, W)
        c.sync()
    c.set_stream(None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 9. launch counts
def test_launch_counts(ctx, W, tree13):
    rng = np.random.default_rng(29000)
    K, length, depth = 8, 16, 13
    placed, _ = _garbage_table(ctx, rng, depth, length)
    counts = lambda: {kind: ctx.timing_drain(kind)[0] for kind in KINDS}
    try:
        ctx.sync()
        ctx.set_timing(True)
        counts()
        for nk in (5123, TILE, 700, 1, 0):
            tiles = -(-nk // TILE)
            passes = (tiles - 1).bit_length() if tiles > 1 else 0
            assert tree13.load_keys(placed.view, _keys(rng, K, nk)) == (0, None)
            launches, ms, rows = ctx.timing_drain("merkle_sort")
            assert (launches, rows) == ((1 + passes, (1 + passes) * nk) if nk else (0, 0)), nk
            print(f"depth 13, {nk} keys of {K} bytes: sort {ms:.3f} ms in {launches} launches")
            assert nk > TILE or launches <= 1  # no merge launch within one tile
            assert counts() == dict.fromkeys(KINDS, 0) | {"merkle_load": 4 if nk else 1, "sha256_records": 1, "merkle_level": depth}, nk
            assert tree13.check_table(placed.view, K) == (0, nk + 1, None)
            tiles = -(-(nk + 1) // TILE)
            passes = (tiles - 1).bit_length() if tiles > 1 else 0
            assert counts() == dict.fromkeys(KINDS, 0) | {"merkle_check": 4 + 3 + depth, "merkle_sort": 1 + passes, "sha256_records": 1}, nk
        # a refused load launches what stands in front of the wait and nothing behind it
        keys = _keys(rng, K, 2000)
        keys[5] = keys[1500]
        assert tree13.load_keys(placed.view, keys) == (1, (5, 1500))
        assert counts() == dict.fromkeys(KINDS, 0) | {"merkle_load": 3, "merkle_sort": 2}
    finally:
        ctx.set_timing(False)
