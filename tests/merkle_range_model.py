"""A pure-Python model of range reads (words.MerkleLink, MerkleTree.range_rows / range_segments) for tests/test_merkle_link_cpu.py and
tests/test_gpu_merkle_range.py, over tests/sha256_ref.py and tests/merkle_climb_model.py alone: select, order, status, the rows byte by byte from the layout
of csrc/merkle_rows.hpp, cut rows and nodes -- neither words.indexed_range nor a statement's bits() enters it, so the CPU test can hold both against it."""
import hashlib

import numpy as np

import merkle_climb_model as CM


def make_table(rng, K, length, depth, nmembers, garbage=2):
    """(np.uint8 [2^depth, length] table, the sorted members): a well-formed indexed table put together by hand -- the sentinel record and one record per
    member with random payloads, in SHUFFLED slots; `garbage` of the inert slots hold lo >= hi drawn from the members' span (so they lie inside ranges), the
    others are all zero"""
    assert nmembers + 1 + garbage <= 1 << depth
    members = set()
    while len(members) < nmembers:
        k = rng.bytes(K)
        if k != bytes(K) and k != b"\xff" * K:
            members.add(k)
    members = sorted(members)
    edges = [bytes(K)] + members + [b"\xff" * K]
    records = [a + b + rng.bytes(length - 2 * K) for a, b in zip(edges, edges[1:])]
    for g in range(garbage):
        x, y = sorted((members[int(rng.integers(nmembers))], members[int(rng.integers(nmembers))]))
        records.append((y + x if g % 2 else y + y) + rng.bytes(length - 2 * K))  # lo > hi (or equal), and lo == hi
    records += [bytes(length)] * ((1 << depth) - len(records))
    perm = rng.permutation(1 << depth)
    table = np.frombuffer(b"".join(records[int(i)] for i in perm), dtype=np.uint8).reshape(1 << depth, length).copy()
    return table, members


def probes(members, K):
    """the bounds a test walks: the members, members +- 1, 1 and max - 1, without the sentinels, ascending"""
    top = (1 << (8 * K)) - 1
    values = {1, top - 1}
    for m in members:
        v = int.from_bytes(m, "big")
        values |= {v - 1, v, v + 1}
    return [v.to_bytes(K, "big") for v in sorted(values) if 0 < v < top]


def links(table, K, lo, hi):
    """the slots of the links of [lo, hi], ordered by (record.lo, slot): the live records with record.hi >= lo and record.lo <= hi"""
    lo, hi = bytes(lo), bytes(hi)
    found = []
    for slot, r in enumerate(table):
        r = bytes(r)
        rlo, rhi = r[:K], r[K: 2 * K]
        if rlo < rhi and rhi >= lo and rlo <= hi:
            found.append((rlo, slot))
    return [slot for _, slot in sorted(found)]


def status(table, K, lo, hi, order):
    """0 when the ordered links chain across [lo, hi], else 2: at least one, the first's lo < lo, every hi the next one's lo, the last's hi > hi"""
    recs = [bytes(table[s]) for s in order]
    if not recs or not recs[0][:K] < bytes(lo) or not recs[-1][K: 2 * K] > bytes(hi):
        return 2
    return 0 if all(a[K: 2 * K] == b[:K] for a, b in zip(recs, recs[1:])) else 2


def keys_of(table, K, order):
    """np.uint8 [n, 2, K]: (lo, hi) of every link"""
    return np.frombuffer(b"".join(bytes(table[s])[: 2 * K] for s in order), dtype=np.uint8).reshape(len(order), 2, K).copy()


def range_rows(table, K, lo, hi, max_links=None, model=None):
    """(rows [n, 32 + length + 32 depth + ceil(depth / 8)], index, keys, status, count) as MerkleTree.range_rows gives them: nothing on status 1, index and
    keys alone on status 2.  model: the tree's merkle_climb_model.ClimbModel when the caller has one already"""
    table = [bytes(r) for r in table]
    order = links(table, K, lo, hi)
    count = len(order)
    model = model or CM.ClimbModel([hashlib.sha256(r).digest() for r in table])
    rowb = 32 + len(table[0]) + 32 * model.depth + (model.depth + 7) // 8
    none = np.zeros((0, rowb), dtype=np.uint8)
    if max_links is not None and count > max_links:
        return none, np.zeros(0, dtype=np.uint32), np.zeros((0, 2, K), dtype=np.uint8), 1, count
    st = status(table, K, lo, hi, order)
    index, keys = np.array(order, dtype=np.uint32), keys_of(table, K, order)
    if st:
        return none, index, keys, st, count
    rows = [CM.record_row(table[s], model.siblings(s), s) for s in order]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(count, rowb).copy(), index, keys, 0, count


def range_segments(table, K, lo, hi, cuts, model=None):
    """(rows: one array a segment, nodes [n, G + 1, 32], index, keys, status, the tree's model): segment 0 a MerkleLink(K, length, c_0) row -- MerkleRecord's --
    over the subtree that holds the link's record, MerkleClimb rows above it; no rows and no nodes unless the status is 0"""
    table = [bytes(r) for r in table]
    order = links(table, K, lo, hi)
    st = status(table, K, lo, hi, order)
    model = model or CM.ClimbModel([hashlib.sha256(r).digest() for r in table])
    c0, segs = int(cuts[0]), CM.ranges(model.depth, cuts)
    n = len(order) if st == 0 else 0
    rows = [np.zeros((n, 32 + len(table[0]) + 32 * c0 + (c0 + 7) // 8), dtype=np.uint8)] + [np.zeros((n, CM.climb_row_bytes(b - a)), dtype=np.uint8) for a, b in segs[1:]]
    nodes = np.zeros((n, len(segs), 32), dtype=np.uint8)
    for i, s in enumerate(order[:n]):
        rows[0][i] = np.frombuffer(CM.record_row(table[s], *model.low(s, cuts)), dtype=np.uint8)
        up, pub = model.upper(s, cuts)
        for g, r in enumerate(up):
            rows[g + 1][i] = np.frombuffer(r, dtype=np.uint8)
        nodes[i] = [list(x) for x in pub]
    return rows, nodes, np.array(order, dtype=np.uint32), keys_of(table, K, order), st, model


def statements(tops, table, index, K, reveal):
    """the statement bytes of the links `index`, put together here: link i's top (the root, or under a cut its level-c_0 node) as words, then lo | hi | the
    first `reveal` payload bytes of its record"""
    return [CM.swap(bytes(top)) + bytes(table[int(s)])[: 2 * K + reveal] for top, s in zip(tops, index)]
