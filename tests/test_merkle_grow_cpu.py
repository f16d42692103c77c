"""CPU: the host model and the verifier's side of growing a tree and its table (words.merkle_node, inert_roots, grown_root, indexed_grow) against a tree
computed here with hashlib and tests/sha256_ref.py, the compression function written from the standard and independent of words.py.

1. merkle_node against sha256_ref.merkle_parent.
2. inert_roots and grown_root against the whole tree over indexed_grow(indexed_records(...), D): depths 1 -> 2, 2 -> 5, 3 -> 4, K = 1 and 8, length 2K and
   2K + 7, with and without members; every right-hand subtree of the grown tree has the root E_l, the spine ends in grown_root.
3. leaf mode against a tree of zero leaves with a few leaves set; a fresh tree's root is inert_roots(D)[-1].
4. grown_root composes: d -> m -> D is d -> D.
5. indexed_check gives the grown table the answer it gave the original, good tables and broken ones.
6. the refusals."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sha256_ref  # noqa: E402
from c_lwe_snarks_amd.words import CircuitError, grown_root, indexed_check, indexed_grow, indexed_records, inert_roots, merkle_node  # noqa: E402

SHAPES = [(1, 2), (2, 5), (3, 4)]


def _levels(leaves):
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        cur = levels[-1]
        levels.append([sha256_ref.merkle_parent(cur[i], cur[i + 1]) for i in range(0, len(cur), 2)])
    return levels


def _members(rng, K, n):
    keys = set()
    while len(keys) < n:
        k = rng.bytes(K)
        if k not in (bytes(K), b"\xff" * K):
            keys.add(k)
    return sorted(keys)


def test_merkle_node():
    rng = np.random.default_rng(31000)
    for left, right in [(bytes(32), bytes(32)), (b"\xff" * 32, b"\xff" * 32)] + [(rng.bytes(32), rng.bytes(32)) for _ in range(8)]:
        assert merkle_node(left, right) == sha256_ref.merkle_parent(left, right)
    assert merkle_node(np.zeros(32, dtype=np.uint8), bytearray(32)) == sha256_ref.merkle_parent(bytes(32), bytes(32))


@pytest.mark.parametrize("d,D", SHAPES)
@pytest.mark.parametrize("K", [1, 8])
def test_grown_tree_of_records(d, D, K):
    rng = np.random.default_rng(31100 + 100 * d + 10 * D + K)
    for length in (2 * K, 2 * K + 7):
        for n in (0, (1 << d) - 1):
            keys = _members(rng, K, n)
            pay = [rng.bytes(length - 2 * K) for _ in keys]
            table = indexed_records(keys, d, length, pay) if keys else indexed_records(np.zeros((0, K), dtype=np.uint8), d, length)
            grown = indexed_grow(table, D)
            assert grown.shape == (1 << D, length) and np.array_equal(grown[: 1 << d], table) and not grown[1 << d:].any()
            old = _levels([hashlib.sha256(r.tobytes()).digest() for r in table])
            new = _levels([hashlib.sha256(r.tobytes()).digest() for r in grown])
            e = inert_roots(D, length)
            assert len(e) == D + 1 and e[0] == hashlib.sha256(bytes(length)).digest()
            for l in range(D + 1):
                width = 1 << max(d - l, 0)  # the old tree's part of level l (the spine's node above the old root)
                assert new[l][width:] == [e[l]] * ((1 << (D - l)) - width), (l, "every node right of the old tree is E_l")
                if l <= d:
                    assert new[l][:width] == old[l]
            assert grown_root(old[-1][0], d, D, length) == new[-1][0]
            assert grown_root(np.frombuffer(old[-1][0], dtype=np.uint8), d, D, length) == new[-1][0]


@pytest.mark.parametrize("d,D", SHAPES + [(3, 6)])
def test_grown_tree_of_leaves(d, D):
    rng = np.random.default_rng(31200 + 10 * d + D)
    assert _levels([bytes(32)] * (1 << D))[-1][0] == inert_roots(D)[-1]  # a fresh tree's root
    leaves = [bytes(32)] * (1 << d)
    for i in rng.choice(1 << d, size=min(3, 1 << d), replace=False):
        leaves[int(i)] = rng.bytes(32)
    old = _levels(leaves)
    new = _levels(leaves + [bytes(32)] * ((1 << D) - (1 << d)))
    assert grown_root(old[-1][0], d, D) == new[-1][0]
    assert grown_root(old[-1][0], d, D) != grown_root(old[-1][0], d, D, 32)  # (32 zero BYTES as a record hash to another leaf)


def test_grown_root_composes():
    rng = np.random.default_rng(31300)
    for length in (None, 0, 16, 55, 71):
        root = rng.bytes(32)
        for d, m, D in ((1, 2, 3), (2, 4, 5), (3, 4, 9), (1, 12, 24), (19, 20, 21)):
            assert grown_root(grown_root(root, d, m, length), m, D, length) == grown_root(root, d, D, length)
    e = inert_roots(24, 55)
    assert [len(x) for x in e] == [32] * 25 and len(set(e)) == 25
    assert inert_roots(0) == [bytes(32)] and inert_roots(5, 55) == e[:6]


def test_indexed_check_of_the_grown_table():
    rng = np.random.default_rng(31400)
    K, length, d = 4, 11, 5
    keys = _members(rng, K, 20)
    good = indexed_records(keys, d, length)[rng.permutation(1 << d)]
    assert indexed_check(good, K) == (0, 21, None)
    slot = int(np.flatnonzero(good[:, K: 2 * K].any(axis=1))[7])
    broken = good.copy()
    broken[slot, 2 * K - 1] ^= 1
    empty = np.zeros_like(good)
    for table in (good, broken, empty):
        want = indexed_check(table, K)
        for D in (6, 9):
            assert indexed_check(indexed_grow(table, D), K) == want
    assert indexed_check(broken, K)[0] == 1 and indexed_check(empty, K) == (1, 0, 0xFFFFFFFF)


def test_refusals():
    root = bytes(32)
    for d, D in ((0, 1), (1, 1), (2, 1), (1, 25), (24, 25), (-1, 3), (1.0, 2), (1, 2.0), (None, 2)):
        with pytest.raises(CircuitError, match="grown_root"):
            grown_root(root, d, D)
    for bad in (bytes(31), bytes(33), b"", "0" * 32, None, 5):
        with pytest.raises(CircuitError, match="grown_root"):
            grown_root(bad, 1, 2)
    for depth, length in ((-1, None), (25, None), (1.5, None), (3, -1), (3, (1 << 20) + 1), (3, 1.5), (3, "55")):
        with pytest.raises(CircuitError, match="inert_roots"):
            inert_roots(depth, length)
    with pytest.raises(CircuitError, match="grown_root|inert_roots"):
        grown_root(root, 1, 2, -1)
    table = np.zeros((8, 6), dtype=np.uint8)
    for t, D in ((table, 3), (table, 2), (table, 25), (table, 4.0), (table[:6], 4), (table[:1], 4), (table.astype(np.uint16), 4), (table.reshape(8, 3, 2), 4), (table.tolist(), 4)):
        with pytest.raises(CircuitError, match="indexed_grow"):
            indexed_grow(t, D)
    assert indexed_grow(table, 4).shape == (16, 6) and indexed_grow(table, 24).shape == (1 << 24, 6)
    for bad in (bytes(31), bytes(33)):
        with pytest.raises(CircuitError, match="merkle_node"):
            merkle_node(bad, bytes(32))
