"""Same-box timing of RANGE reads of an indexed table (MerkleTree.count_range / range_rows / range_segments: k_range_flags, k_range_keys, k_range_order of
merkle.hip) on the table the other key calls are measured on: 2^depth records of 55 bytes with 8-byte keys, HALF full -- the sentinel record and 2^(depth - 1)
- 1 members in shuffled slots, the other slots all zero.  One process; every leg is called once to warm up, then --reps times (default 7), and the medians
are reported; kernel timing is ON in every leg.  One JSON line per case, also appended to --out (default profiles/range_time.jsonl).  A case is a tree
(depth 19 uncut, depth 20 cut at [10]) and a range holding 1, 255, 1 020 or 16 384 members (one link more); its legs, all in the same run:
  * "call_ms": range_rows / range_segments with max_links = the links, from the call to its return, and its kernels by kind ("merkle_range": flags, scan
    and select together; "merkle_range_order": keys and order together; "merkle_absent_rows"; "merkle_paths" or "merkle_climb_rows").
  * "count_call_ms" / "flags_scan_kernel_ms": count_range, whose two launches are k_range_flags and the one-workgroup scan.
  * per tree, the parent's kernels that stream the same table: "locate_kernel_ms", k_key_locate for one absent key (locate_keys), and
    "inert_kernel_ms", k_inert_flags + scan + select inside insert_keys of one key (removed again behind it, outside the timed part).
  * "host_ms": what a user has today -- the table to the host, words.indexed_range, MerkleTree.record_rows / record_segments of the slots found.  Its rows
    are compared with the call's ("equal_host").
No ratio or time was fixed in advance.  dev tool.  usage: python tools/range_time.py [--depths 19 20] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import c_lwe_snarks_amd as mf  # noqa: E402
from c_lwe_snarks_amd import words as W  # noqa: E402

K, LENGTH = 8, 55
KINDS = ["merkle_range", "merkle_range_order", "merkle_absent_rows", "merkle_paths", "merkle_climb_rows", "merkle_locate", "merkle_inert", "merkle_owners",
         "merkle_updates", "merkle_insert_records", "merkle_remove_records", "sha256_records", "merkle_level"]


def _emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def _med(xs):
    return round(statistics.median(xs), 4)


def _all(xs):
    return [round(x, 4) for x in xs]


def _reps(ctx, fn, kinds, reps, after=None):
    """(wall ms of each repetition, [kernel ms of each repetition] per kind, the last result): one warm-up call, then reps; `after` runs untimed behind each"""
    walls, kerns, out = [], [[] for _ in kinds], None
    for r in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ks = [ctx.timing_drain(k)[1] for k in kinds]
        if after:
            after()
            ctx.sync()
            for k in KINDS:
                ctx.timing_drain(k)
        if r:
            walls.append(wall)
            for acc, k in zip(kerns, ks):
                acc.append(k)
    return walls, kerns, out


def _table(rng, depth):
    """(np.uint8 [2^depth, LENGTH], the sorted members as uint64): a half-full indexed table in shuffled slots, random payloads on the live records"""
    n = 1 << depth
    live = n // 2
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=live + 4096, dtype=np.uint64))[: live - 1]
    assert len(keys) == live - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = np.zeros((n, LENGTH), dtype=np.uint8)
    slots = rng.permutation(n)[:live]
    table[slots] = rng.integers(0, 256, size=(live, LENGTH), dtype=np.uint8)
    table[slots, :K] = lo.astype(">u8").view(np.uint8).reshape(live, K)
    table[slots, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(live, K)
    return table, keys


def _key(v):
    return int(v).to_bytes(K, "big")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs="+", default=[19, 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_time.jsonl"))
    a = ap.parse_args()
    ok = True
    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    rng = np.random.default_rng(2032)
    for depth in a.depths:
        n = 1 << depth
        cuts = None if depth <= 19 else [10]
        base = {"tool": "range_time", "records": n, "members": n // 2 - 1, "length": LENGTH, "key_bytes": K, "depth": depth, "cuts": cuts, "reps": a.reps}
        host_table, members = _table(rng, depth)
        table = ctx.to_device(host_table).reshape(n, LENGTH)
        tree = ctx.merkle_tree(depth)
        tree.set_records(0, table)
        ctx.sync()
        for kind in KINDS:
            ctx.timing_drain(kind)
        # the parent's kernels over the same table, in the same run
        absent = np.frombuffer(_key(int(members[1000]) + 1), dtype=np.uint8).reshape(1, K).copy()
        assert int(members[1000]) + 1 != int(members[1001])
        _, (locate,), _ = _reps(ctx, lambda: tree.locate_keys(table, absent), ["merkle_locate"], a.reps)
        _, (inert,), _ = _reps(ctx, lambda: tree.insert_keys(table, absent), ["merkle_inert"], a.reps, after=lambda: tree.remove_keys(table, absent))
        ok = ok and bool(np.array_equal(table.cpu().numpy(), host_table))
        for inside in (1, 255, 1020, 16384):
            links = inside + 1
            first = int(rng.integers(1, len(members) - inside - 1))
            lo, hi = _key(members[first]), _key(members[first + inside - 1])
            cw, (ck,), count = _reps(ctx, lambda: tree.count_range(table, lo, hi), ["merkle_range"], a.reps)
            if cuts is None:
                kinds = ["merkle_range", "merkle_range_order", "merkle_absent_rows", "merkle_paths"]
                rw, kerns, (rows, index, keys, status) = _reps(ctx, lambda: tree.range_rows(table, lo, hi, max_links=links), kinds, a.reps)

                def host():
                    t = table.cpu().numpy()
                    slots = W.indexed_range(t, K, lo, hi)
                    return tree.record_rows(t[slots], slots), slots

                hw, _, (h_rows, h_slots) = _reps(ctx, host, ["merkle_paths"], a.reps)
                good = bool(np.array_equal(rows, h_rows))
            else:
                kinds = ["merkle_range", "merkle_range_order", "merkle_absent_rows", "merkle_climb_rows"]
                rw, kerns, (rows, nodes, index, keys, status) = _reps(ctx, lambda: tree.range_segments(table, lo, hi, cuts, max_links=links), kinds, a.reps)

                def host():
                    t = table.cpu().numpy()
                    slots = W.indexed_range(t, K, lo, hi)
                    return tree.record_segments(t[slots], slots, cuts), slots

                hw, _, ((h_rows, h_nodes), h_slots) = _reps(ctx, host, ["merkle_climb_rows"], a.reps)
                good = bool(all(np.array_equal(x, y) for x, y in zip(rows, h_rows)) and np.array_equal(nodes, h_nodes))
            good = good and status == 0 and count == links == len(index) and index.tolist() == h_slots
            good = good and keys[1:, 0].tobytes() == members[first: first + inside].astype(">u8").tobytes()
            ok = ok and good
            _emit({**base, "members_inside": inside, "links": links, "call_ms": _med(rw), "call_ms_all": _all(rw), "range_kernels_ms": _med(kerns[0]),
                   "range_kernels_ms_all": _all(kerns[0]), "order_kernels_ms": _med(kerns[1]), "order_kernels_ms_all": _all(kerns[1]),
                   "gather_kernel_ms": _med(kerns[2]), "paths_or_climb_kernel_ms": _med(kerns[3]), "count_call_ms": _med(cw), "count_call_ms_all": _all(cw),
                   "flags_scan_kernel_ms": _med(ck), "flags_scan_kernel_ms_all": _all(ck), "locate_kernel_ms": _med(locate), "locate_kernel_ms_all": _all(locate),
                   "inert_kernel_ms": _med(inert), "inert_kernel_ms_all": _all(inert), "host_ms": _med(hw), "host_ms_all": _all(hw),
                   "host_over_call": round(_med(hw) / _med(rw), 2), "equal_host": good}, a.out)
        tree.close()
        del table
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
