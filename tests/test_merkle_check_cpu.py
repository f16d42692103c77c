"""CPU: words.indexed_check, the host model of the CHAIN part of MerkleTree.check_table (mfh_merkle_check_table): do the live records of an indexed table,
sorted by (lo, slot), tile the key space from 00..00 to FF..FF?  The device check against this model: tests/test_gpu_merkle_load.py.

1. good tables: words.indexed_records for K in 1, 5, 8, 32 and 0, 1, 7 members, in place and with the records shuffled into random slots of a larger table.
2. defects, each with its expected (status, live, where): a wrong first lo, a gap, an overlap, a duplicated lo (the tie breaks by slot), a last hi that is
   not FF..FF, no live record at all, and a difference in the last byte of a partial word only.
3. 2^13 records (the model is vectorised) and malformed arguments."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c_lwe_snarks_amd import words  # noqa: E402
from c_lwe_snarks_amd.words import CircuitError, indexed_check, indexed_records  # noqa: E402

WIDTHS = [1, 5, 8, 32]


def _members(rng, K, n):
    top = (1 << (8 * K)) - 1
    if K == 1:
        values = [int(v) for v in rng.choice(np.arange(2, top - 1, 3), size=n, replace=False)]
    else:
        values = list({int.from_bytes(rng.bytes(K), "big") | 4 for _ in range(4 * n + 4)} - {top})[:n]
    assert len(values) == n
    return [v.to_bytes(K, "big") for v in values]


def _shuffled(rng, table, nslots):
    """the live records of `table` in random slots of a table of nslots records; (the new table, slot of sorted record i)"""
    live = [r for r in table if r.any()]
    out = np.zeros((nslots, table.shape[1]), dtype=np.uint8)
    slots = rng.choice(nslots, size=len(live), replace=False)
    for r, s in zip(live, slots):
        out[s] = r
    return out, [int(s) for s in slots]


@pytest.mark.parametrize("K", WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 7])
def test_good_tables(K, n):
    rng = np.random.default_rng(100 * K + n)
    for length in (2 * K, 2 * K + 7):
        table = indexed_records(np.frombuffer(b"".join(_members(rng, K, n)), dtype=np.uint8).reshape(n, K), 4, length)
        assert indexed_check(table, K) == (0, n + 1, None)
        moved, _ = _shuffled(rng, table, 32)
        assert indexed_check(moved, K) == (0, n + 1, None)


@pytest.mark.parametrize("K", WIDTHS)
def test_defects(K):
    rng = np.random.default_rng(7000 + K)
    n = 7
    table = indexed_records(_members(rng, K, n), 4)
    good, slot = _shuffled(rng, table, 32)  # slot[i]: where sorted record i stands
    assert indexed_check(good, K) == (0, n + 1, None)

    t = good.copy()  # a wrong first lo: the sentinel record starts above 00..00 (still below its hi: the members are >= 2)
    t[slot[0], K - 1] = 1
    assert indexed_check(t, K) == (1, n + 1, slot[0])

    t = good.copy()  # a gap in front of sorted record 4: its lowest bit flips (members differ by more than that)
    t[slot[4], K - 1] ^= 1
    assert indexed_check(t, K) == (1, n + 1, slot[4])

    t = good.copy()  # an overlap: the lowest bit of record 3's hi flips
    t[slot[3], 2 * K - 1] ^= 1
    assert indexed_check(t, K) == (1, n + 1, slot[4])

    t = good.copy()  # a duplicated lo: a copy of sorted record 2 in a free slot -- the two stand in slot order, and the chain breaks at the second
    free = [s for s in range(32) if s not in slot]
    for twin in (free[0], free[-1]):
        u = t.copy()
        u[twin] = u[slot[2]]
        first, second = sorted((twin, slot[2]))
        assert indexed_check(u, K) == (1, n + 2, second), (twin, first)

    t = good.copy()  # the last hi is not FF..FF
    t[slot[n], 2 * K - 1] = 0xFE
    assert indexed_check(t, K) == (1, n + 1, slot[n])

    t = np.zeros_like(good)  # no live record at all: every slot inert, and a record with lo == hi is inert too
    assert indexed_check(t, K) == (1, 0, 0xFFFFFFFF)
    t[5, :K] = 9
    t[5, K: 2 * K] = 9
    assert indexed_check(t, K) == (1, 0, 0xFFFFFFFF)

    if K % 4:  # a difference in the LAST byte of a partial word only: hi_0 and lo_1 agree in every byte but byte K - 1
        a = bytes([0x80] * (K - 1)) + b"\x10"
        two = indexed_records([a], 2)
        assert indexed_check(two, K) == (0, 2, None)
        two[1, K - 1] ^= 1
        assert indexed_check(two, K) == (1, 2, 1)


def test_large_and_payload_bytes_are_ignored():
    rng = np.random.default_rng(5)
    K, n = 8, (1 << 13) - 1
    keys = rng.integers(1, 255, size=(n, K), dtype=np.uint8)
    keys = np.unique(keys, axis=0)
    table = indexed_records(keys, 13, 2 * K + 3, payloads=[b"\xff\xff\xff"] * len(keys))
    perm = rng.permutation(1 << 13)
    moved = table[perm]
    assert indexed_check(moved, K) == (0, len(keys) + 1, None)
    at = int(np.flatnonzero(perm == 4000)[0])  # sorted record 4000 stands in slot `at`
    moved[at, 0] ^= 0x80  # its lo leaves its place: it is inert (lo > hi), live (a gap where it stood) or elsewhere in the order -- the model decides
    status, live, where = indexed_check(moved, K)
    assert status == 1 and live in (len(keys), len(keys) + 1) and 0 <= where < 1 << 13


def test_malformed_arguments():
    table = indexed_records([b"\x05"], 2)
    for bad in (lambda: indexed_check(table, 0), lambda: indexed_check(table, 33), lambda: indexed_check(table, 2), lambda: indexed_check(table, 1.0),
                lambda: indexed_check(table.astype(np.uint16), 1), lambda: indexed_check(table[0], 1), lambda: indexed_check(table.tolist(), 1)):
        with pytest.raises(CircuitError):
            bad()
    assert words.indexed_check(table, 1) == (0, 2, None)
