"""Same-box timing of non-membership lookups in an indexed table on the device (MerkleTree.locate_keys / absent_rows: k_key_locate, k_absent_gather and
k_merkle_paths of merkle.hip) for a table of 2^--log-records records (default 20) with 8-byte keys, every slot but one a member.  One process; every leg is
called once to warm up, then --reps times (default 7), and the medians are reported.  One JSON line per case, also appended to --out (default
profiles/absent_time.jsonl).  A case is a record length (16 bytes: the two keys alone, packed; 55 bytes: the longest one-block record) and a number of
queries (255, 1 020), all absent, drawn at random:
  * "locate_call_ms" / "locate_kernel_ms": locate_keys from the call to its return (it waits for the stream), and the HIP-event time of its one launch (kind
    "merkle_locate"); "key_gbytes_per_s" = the table's key bytes (2^D x 16) over the kernel time, "table_gbytes_per_s" = the table's span over it.
  * "rows_call_ms" and the kernel times by kind ("merkle_locate", "merkle_absent_rows", "merkle_paths") of absent_rows.
  * the baseline a user has today, in the same run: the table copied to the host ("host_copy_ms"), np.searchsorted of the queries on the records' own keys
    viewed as big-endian integers ("host_search_ms"; the table of this tool is sorted by position, which the device call does not need and the baseline
    does -- a table that took inserts would have to be sorted first), then MerkleTree.record_rows of the found records ("host_rows_ms").
    "baseline_over_rows_call" is their sum over rows_call_ms.  The baseline's indices and rows are compared with the device's ("equal_baseline").
No ratio was fixed in advance.  dev tool.  usage: python tools/absent_time.py [--log-records 20] [--reps 7] [--out FILE]"""
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

K = 8


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


def _reps(ctx, fn, kinds, reps):
    """(wall ms of each repetition, [kernel ms of each repetition] per kind, the last result): one warm-up call, then reps"""
    walls, kerns, out = [], [[] for _ in kinds], None
    for r in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ks = [ctx.timing_drain(k)[1] for k in kinds]
        if r:
            walls.append(wall)
            for acc, k in zip(kerns, ks):
                acc.append(k)
    return walls, kerns, out


def _table(rng, depth, length):
    """np.uint8 [2^depth, length]: the sentinel record and 2^depth - 1 members in ascending order (indexed_records' layout, built with numpy), random payloads"""
    n = 1 << depth
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=n + 4096, dtype=np.uint64))[: n - 1]
    assert len(keys) == n - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = rng.integers(0, 256, size=(n, length), dtype=np.uint8)
    table[:, :K] = lo.astype(">u8").view(np.uint8).reshape(n, K)
    table[:, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(n, K)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absent_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    base = {"tool": "absent_time", "records": n, "key_bytes": K, "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    rng = np.random.default_rng(2029)
    kinds = ["merkle_locate", "merkle_absent_rows", "merkle_paths"]
    for length in (16, 55):
        host_table = _table(rng, depth, length)
        table = ctx.to_device(host_table).reshape(n, length)
        tree = ctx.merkle_tree(depth)
        tree.set_records(0, table)
        ctx.sync()
        for kind in kinds + ["sha256_records", "merkle_level"]:
            ctx.timing_drain(kind)
        for nq in (255, 1020):
            keys = rng.integers(1, 255, size=(nq, K), dtype=np.uint8)  # (no byte 0x00 or 0xFF: no sentinel)
            lw, (lk,), (l_index, l_status) = _reps(ctx, lambda: tree.locate_keys(table, keys), kinds[:1], a.reps)
            rw, (rk_l, rk_g, rk_p), (rows, index, status) = _reps(ctx, lambda: tree.absent_rows(table, keys), kinds, a.reps)
            # the baseline: the table to the host, a search on the host, the rows of the found records
            cc, ss, bb, b_rows, b_idx = [], [], [], None, None
            for r in range(a.reps + 1):
                ctx.sync()
                t0 = time.perf_counter()
                host = table.cpu().numpy()
                t1 = time.perf_counter()
                los = np.ascontiguousarray(host[:, :K]).view(">u8").reshape(n)
                b_idx = np.searchsorted(los, keys.view(">u8").reshape(nq), side="right") - 1
                t2 = time.perf_counter()
                b_rows = tree.record_rows(host[b_idx], b_idx)
                t3 = time.perf_counter()
                ctx.timing_drain("merkle_paths")
                if r:
                    cc.append((t1 - t0) * 1e3), ss.append((t2 - t1) * 1e3), bb.append((t3 - t2) * 1e3)
            good = bool(np.array_equal(l_index, index) and np.array_equal(l_status, status) and not status.any() and np.array_equal(index, b_idx.astype(np.uint32))
                        and np.array_equal(rows[:, 32 + K:], b_rows[:, 32:]) and np.array_equal(rows[:, 32: 32 + K], keys) and not rows[:, :32].any())
            ok = ok and good
            span = (n - 1) * length + length
            _emit({**base, "length": length, "queries": nq, "locate_call_ms": _med(lw), "locate_call_ms_all": _all(lw), "locate_kernel_ms": _med(lk),
                   "locate_kernel_ms_all": _all(lk), "key_gbytes_per_s": round(n * 2 * K / (_med(lk) * 1e6), 1), "table_gbytes_per_s": round(span / (_med(lk) * 1e6), 1),
                   "rows_call_ms": _med(rw), "rows_call_ms_all": _all(rw), "rows_locate_kernel_ms": _med(rk_l), "rows_gather_kernel_ms": _med(rk_g),
                   "rows_paths_kernel_ms": _med(rk_p), "host_copy_ms": _med(cc), "host_search_ms": _med(ss), "host_rows_ms": _med(bb),
                   "baseline_ms": round(_med(cc) + _med(ss) + _med(bb), 4), "baseline_over_rows_call": round((_med(cc) + _med(ss) + _med(bb)) / _med(rw), 1),
                   "equal_baseline": good}, a.out)
        tree.close()
        del table
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
