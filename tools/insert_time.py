"""Same-box timing of batches of key inserts into an indexed table on the device (MerkleTree.insert_keys: k_key_locate, k_inert_flags / _scan / _select,
k_insert_records and the record-update chain of merkle.hip) for a table of 2^--log-records records (default 20) with 8-byte keys, half full: the sentinel
record and 2^(D-1) - 1 members in the lower half, the upper half inert.  One process; before every call the table is restored from a device copy and the
tree rebuilt (not timed); every leg is called once to warm up, then --reps times (default 7), and the medians are reported.  One JSON line per case, also
appended to --out (default profiles/insert_time.jsonl).  A case is a record length (16 bytes: the two keys alone; 55 bytes: the longest one-block record)
and a number of random absent keys per call (255, 1 020):
  * "call_ms": insert_keys(roots=True) from the call to its return (it waits for the stream), and by HIP events in the same calls "locate_kernel_ms"
    (kind "merkle_locate"), "inert_kernel_ms" ("merkle_inert", three launches), "build_kernel_ms" ("merkle_insert_records") and "update_chain_ms"
    ("sha256_records" + "merkle_record_rows" + "merkle_updates").
  * the baseline a user has today, in the same run, "baseline_ms": the table copied to the host and its inert slots listed with numpy ("host_copy_ms"),
    then per key locate_keys, words.indexed_insert into the next inert slot and update_records ("loop_ms").  "baseline_over_call" is their ratio.
Both ways must leave the same table, the same tree (every level) and the same roots ("equal_baseline") before a time is reported; the exit status says so.
No ratio was fixed in advance.  dev tool.  usage: python tools/insert_time.py [--log-records 20] [--reps 7] [--out FILE]"""
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

K = 8
KINDS = ["merkle_locate", "merkle_inert", "merkle_insert_records", "sha256_records", "merkle_record_rows", "merkle_updates"]


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


def _table(rng, depth, length):
    """np.uint8 [2^depth, length]: the sentinel record and 2^(depth-1) - 1 members in ascending order in the lower half, the upper half all zero"""
    n, live = 1 << depth, 1 << (depth - 1)
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=live + 4096, dtype=np.uint64))[: live - 1]
    assert len(keys) == live - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = np.zeros((n, length), dtype=np.uint8)
    table[:live] = rng.integers(0, 256, size=(live, length), dtype=np.uint8)
    table[:live, :K] = lo.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(live, K)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insert_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    base = {"tool": "insert_time", "records": n, "key_bytes": K, "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    rng = np.random.default_rng(2030)
    for length in (16, 55):
        pristine = ctx.to_device(_table(rng, depth, length)).reshape(n, length)
        table = pristine.clone()
        tree = ctx.merkle_tree(depth)

        def restore():
            table.copy_(pristine)
            tree.set_records(0, table)
            ctx.sync()
            for kind in KINDS + ["merkle_level"]:
                ctx.timing_drain(kind)

        for nk in (255, 1020):
            keys = rng.integers(1, 255, size=(nk, K), dtype=np.uint8)  # (no byte 0x00 or 0xFF: no sentinel; 8 random bytes: no member, no repeat)
            pay = rng.integers(0, 256, size=(nk, length - 2 * K), dtype=np.uint8)
            walls, kerns, got = [], {k: [] for k in KINDS}, None
            for r in range(a.reps + 1):
                restore()
                t0 = time.perf_counter()
                got = tree.insert_keys(table, keys, pay, roots=True)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                ks = {k: ctx.timing_drain(k)[1] for k in KINDS}
                if r:
                    walls.append(wall)
                    for k in KINDS:
                        kerns[k].append(ks[k])
            d_table, d_levels, d_roots, d_index = table.clone(), [tree.nodes(l).clone() for l in range(depth + 1)], got[2], got[1]
            # the baseline: the table to the host for its inert slots, then one key at a time through the existing calls
            cc, ll, b_roots, b_index = [], [], None, None
            for r in range(a.reps + 1):
                restore()
                t0 = time.perf_counter()
                host = table.cpu().numpy()
                free = np.flatnonzero(~(np.ascontiguousarray(host[:, :K]).view(">u8").reshape(n) < np.ascontiguousarray(host[:, K: 2 * K]).view(">u8").reshape(n)))
                t1 = time.perf_counter()
                b_roots, b_index = [tree.root()], []
                for j in range(nk):
                    at, status = tree.locate_keys(table, keys[j: j + 1])
                    p, s = int(at[0]), int(free[j])
                    idx, new = W.indexed_insert(host[p].tobytes(), p, keys[j].tobytes(), s, payload=pay[j].tobytes())
                    _, roots = tree.update_records(table, idx, new, roots=True)
                    host[idx] = new  # (the host copy follows the table, as the user's would)
                    b_roots.append(roots[2].tobytes())
                    b_index.append((p, s))
                ctx.sync()
                t2 = time.perf_counter()
                if r:
                    cc.append((t1 - t0) * 1e3), ll.append((t2 - t1) * 1e3)
            torch = ctx.torch
            good = bool(torch.equal(table, d_table) and all(torch.equal(tree.nodes(l), d_levels[l]) for l in range(depth + 1))
                        and [x.tobytes() for x in d_roots] == b_roots and d_index.tolist() == [list(x) for x in b_index])
            ok = ok and good
            chain = [x + y + z for x, y, z in zip(kerns["sha256_records"], kerns["merkle_record_rows"], kerns["merkle_updates"])]
            _emit({**base, "length": length, "inserts": nk, "call_ms": _med(walls), "call_ms_all": _all(walls), "locate_kernel_ms": _med(kerns["merkle_locate"]),
                   "inert_kernel_ms": _med(kerns["merkle_inert"]), "inert_kernel_ms_all": _all(kerns["merkle_inert"]), "build_kernel_ms": _med(kerns["merkle_insert_records"]),
                   "build_kernel_ms_all": _all(kerns["merkle_insert_records"]), "update_chain_ms": _med(chain), "host_copy_ms": _med(cc), "loop_ms": _med(ll),
                   "baseline_ms": round(_med(cc) + _med(ll), 4), "baseline_over_call": round((_med(cc) + _med(ll)) / _med(walls), 1), "equal_baseline": good}, a.out)
        tree.close()
        del table, pristine
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
