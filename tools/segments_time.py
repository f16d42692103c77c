"""Same-box timing of the update calls with the path cut into level ranges (MerkleTree.update_segments and insert_key_segments: the parent call's kernels
and k_merkle_cut_rows of merkle.hip) at depth --log-leaves (default 20).  One process; before every call the tree (and the table) is restored (not timed);
every leg is called once to warm up, then --reps times (default 7), and the medians are reported.  One JSON line per case, also appended to --out
(default profiles/segments_time.jsonl).  The cases: 1 020 leaf updates under cuts [10]; 255 and 1 020 inserts of 8-byte keys into 55-byte records of a
half-full indexed table under cuts [4, 12].  Per case:
  * "call_ms": the cut call from the call to its return (it waits for the stream), kernel timing on, and by HIP events in the same calls
    "cut_kernel_ms" (kind "merkle_segments", one launch) and "other_kernels_ms" (every other kind of the call).
  * "uncut_call_ms": the parent call (update_rows / insert_keys with roots) in the same run, so "cut_minus_uncut_ms" is what cutting costs.
  * "host_nodes_ms": what a user could do before -- after the uncut call, every cut node recomputed on the host from the row's old and new leaf and its
    siblings (the compression function in numpy, vectorised over the batch, one pass per level below the highest cut, old and new side together; for
    inserts the leaves are hashlib digests of the records in the row) -- and "baseline_ms" = uncut_call_ms + host_nodes_ms, "baseline_over_call".
The host's nodes must equal the call's published nodes ("equal_baseline") before a time is reported; the exit status says so.  No ratio was fixed in
advance.  dev tool.  usage: python tools/segments_time.py [--log-leaves 20] [--reps 7] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import c_lwe_snarks_amd as mf  # noqa: E402

K = 8
KINDS = ["merkle_segments", "merkle_updates", "merkle_locate", "merkle_inert", "merkle_insert_records", "sha256_records", "merkle_record_rows"]


def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % q for q in out):
            out.append(k)
        k += 1
    return out


def _frac(prime, root):
    lo, hi, target = 0, 1 << 40, prime << (32 * root)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if mid ** root <= target else (lo, mid - 1)
    return lo & 0xFFFFFFFF


IV = np.array([_frac(p, 2) for p in _primes(8)], dtype=np.uint32)
KK = np.array([_frac(p, 3) for p in _primes(64)], dtype=np.uint32)


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def parents(left, right):
    """uint8 [n, 32] x 2 -> uint8 [n, 32]: compress(IV, left || right) of FIPS 180-4 for n pairs at once, no padding block (the tree's node function)"""
    w = list(np.ascontiguousarray(np.concatenate([left, right], axis=1)).view(">u4").astype(np.uint32).T)
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> np.uint32(3))
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> np.uint32(10))
        w.append(w[t - 16] + s0 + w[t - 7] + s1)
    a, b, c, d, e, f, g, h = (np.full(len(left), v, dtype=np.uint32) for v in IV)
    for t in range(64):
        t1 = h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g)) + KK[t] + w[t]
        t2 = (_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))
        a, b, c, d, e, f, g, h = t1 + t2, a, b, c, d + t1, e, f, g
    out = np.stack([x + v for x, v in zip((a, b, c, d, e, f, g, h), IV)], axis=1)
    return out.astype(">u4").view(np.uint8).reshape(len(left), 32)


def _words_to_bytes(a):
    return a.reshape(a.shape[0], -1, 4)[:, :, ::-1].reshape(a.shape[0], -1)


def host_nodes(old, new, siblings, index, cuts):
    """[n, len(cuts), 2, 32]: the old and the new node of every cut level on each update's path, from its old and new leaf, its siblings (uint8 [n, depth,
    32], digest byte order) and its index"""
    n, top = len(old), cuts[-1]
    cur = np.concatenate([old, new])
    out = np.zeros((n, len(cuts), 2, 32), dtype=np.uint8)
    for l in range(top):
        sib = np.concatenate([siblings[:, l], siblings[:, l]])
        right = np.concatenate([(index >> l) & 1, (index >> l) & 1]).astype(bool)[:, None]
        cur = parents(np.where(right, sib, cur), np.where(right, cur, sib))
        if l + 1 in cuts:
            g = cuts.index(l + 1)
            out[:, g, 0], out[:, g, 1] = cur[:n], cur[n:]
    return out


def _emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def _med(xs):
    return round(statistics.median(xs), 4)


def _table(rng, depth, length):
    """tools/insert_time.py's table: the sentinel record and 2^(depth-1) - 1 members in the lower half, the upper half all zero"""
    n, live = 1 << depth, 1 << (depth - 1)
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=live + 4096, dtype=np.uint64))[: live - 1]
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = np.zeros((n, length), dtype=np.uint8)
    table[:live] = rng.integers(0, 256, size=(live, length), dtype=np.uint8)
    table[:live, :K] = lo.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(live, K)
    return table


def _timed(ctx, reps, restore, call):
    """(walls, per-kind kernel ms lists, the last result) of reps calls after one warm-up"""
    walls, kerns, got = [], {k: [] for k in KINDS}, None
    for r in range(reps + 1):
        restore()
        t0 = time.perf_counter()
        got = call()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ks = {k: ctx.timing_drain(k)[1] for k in KINDS}
        if r:
            walls.append(wall)
            for k in KINDS:
                kerns[k].append(ks[k])
    return walls, kerns, got


def _report(base, a, walls, kerns, uncut_walls, host, good, **more):
    others = [sum(kerns[k][i] for k in KINDS[1:]) for i in range(len(walls))]
    call, uncut, nodes = _med(walls), _med(uncut_walls), _med(host)
    _emit({**base, **more, "call_ms": call, "call_ms_all": [round(x, 4) for x in walls], "cut_kernel_ms": _med(kerns["merkle_segments"]),
           "cut_kernel_ms_all": [round(x, 4) for x in kerns["merkle_segments"]], "other_kernels_ms": _med(others), "uncut_call_ms": uncut,
           "cut_minus_uncut_ms": round(call - uncut, 4), "host_nodes_ms": nodes, "baseline_ms": round(uncut + nodes, 4),
           "baseline_over_call": round((uncut + nodes) / call, 1), "equal_baseline": good}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-leaves", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_leaves, 1 << a.log_leaves
    base = {"tool": "segments_time", "depth": depth, "reps": a.reps}
    ok = True
    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    rng = np.random.default_rng(2040)

    def drain():
        ctx.sync()
        for kind in KINDS + ["merkle_level"]:
            ctx.timing_drain(kind)

    # ---- leaf updates
    cuts = [depth // 2]
    leaves = ctx.to_device(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    tree = ctx.merkle_tree(depth)

    def restore():
        tree.set_leaves(0, leaves)
        drain()

    for nupd in (1020,):
        idx = rng.integers(0, n, size=nupd)
        new = ctx.to_device(rng.integers(0, 256, size=(nupd, 32), dtype=np.uint8))
        walls, kerns, got = _timed(ctx, a.reps, restore, lambda: tree.update_segments(idx, new, cuts, roots=True))
        uwalls, _, ugot = _timed(ctx, a.reps, restore, lambda: tree.update_rows(idx, new, roots=True))
        host, mine = [], None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            rows = ugot[0]
            sib = _words_to_bytes(rows[:, 128: 128 + 32 * depth]).reshape(nupd, depth, 32)
            mine = host_nodes(_words_to_bytes(rows[:, 64:96]), _words_to_bytes(rows[:, 96:128]), sib, idx, cuts)
            if r:
                host.append((time.perf_counter() - t0) * 1e3)
        good = bool(np.array_equal(mine, got[1][:, :-1]) and np.array_equal(ugot[1], got[2]))
        ok = ok and good
        _report(base, a, walls, kerns, uwalls, host, good, case="leaf updates", updates=nupd, cuts=cuts)
    tree.close()
    del leaves

    # ---- inserts
    length = 55
    cuts = [depth // 5, 3 * depth // 5] if depth >= 5 else [1]
    pristine = ctx.to_device(_table(rng, depth, length)).reshape(n, length)
    table = pristine.clone()
    tree = ctx.merkle_tree(depth)

    def restore_table():
        table.copy_(pristine)
        tree.set_records(0, table)
        drain()

    for nk in (255, 1020):
        keys = rng.integers(1, 255, size=(nk, K), dtype=np.uint8)
        pay = rng.integers(0, 256, size=(nk, length - 2 * K), dtype=np.uint8)
        walls, kerns, got = _timed(ctx, a.reps, restore_table, lambda: tree.insert_key_segments(table, keys, cuts, pay))
        uwalls, _, ugot = _timed(ctx, a.reps, restore_table, lambda: tree.insert_keys(table, keys, pay, roots=True))
        host, mine = [], None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            rows, index = ugot[0], ugot[1].astype(np.int64)
            at = 64 + K
            old_p, old_s, new_s = rows[:, at: at + length], rows[:, at + length: at + 2 * length], rows[:, at + 2 * length: at + 3 * length]
            new_p = np.concatenate([old_p[:, :K], rows[:, 64: 64 + K], old_p[:, 2 * K:]], axis=1)
            dig = lambda recs: np.frombuffer(b"".join(hashlib.sha256(x.tobytes()).digest() for x in recs), dtype=np.uint8).reshape(len(recs), 32)  # noqa: E731
            tail = at + 3 * length
            sib_p = _words_to_bytes(rows[:, tail: tail + 32 * depth]).reshape(nk, depth, 32)
            sib_s = _words_to_bytes(rows[:, tail + 32 * depth: tail + 64 * depth]).reshape(nk, depth, 32)
            mine = host_nodes(np.concatenate([dig(old_p), dig(old_s)]), np.concatenate([dig(new_p), dig(new_s)]), np.concatenate([sib_p, sib_s]),
                              np.concatenate([index[:, 0], index[:, 1]]), cuts)
            if r:
                host.append((time.perf_counter() - t0) * 1e3)
        good = bool(np.array_equal(mine[:nk], got[1][:, :-1]) and np.array_equal(mine[nk:], got[2][:, :-1]) and np.array_equal(ugot[1], got[3])
                    and np.array_equal(ugot[2][:-1], got[1][:, -1, 0]) and np.array_equal(ugot[2][1:], got[2][:, -1, 1]))
        ok = ok and good
        _report(base, a, walls, kerns, uwalls, host, good, case="inserts", inserts=nk, length=length, key_bytes=K, cuts=cuts)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
