"""Same-box timing of batches of transfers between the accounts of an indexed table on the device (MerkleTree.transfer_keys / transfer_key_segments:
k_key_locate, k_balance_gather, k_transfer_records and the record-update chain of merkle.hip) for a table of 2^--log-records records (default 20) of 55 bytes
with 8-byte keys and 8-byte balances, half full: the sentinel record and 2^(D-1) - 1 members in the lower half, the upper half all zero.  One process; before
every call the table is restored from a device copy and the tree rebuilt (not timed); every leg is called once to warm up, then --reps times (default 7), and
the medians are reported; kernel timing is on in every leg.  One JSON line per case, also appended to --out (default profiles/transfer_time.jsonl).  A case is a
number of transfers per call (255, 1 020) between random members, each amount at most a quarter of what a member starts with:
  * "call_ms": transfer_keys(roots=True) from the call to its return (it waits for the stream), and by HIP events in the same calls "locate_kernel_ms" (kind
    "merkle_locate"), "balances_kernel_ms" ("merkle_balances"), "build_kernel_ms" ("merkle_transfer_records") and "update_chain_ms" ("sha256_records" +
    "merkle_record_rows" + "merkle_updates").
  * "cut_call_ms": transfer_key_segments under --cuts (default 4,12) likewise, with "segments_kernel_ms" ("merkle_segments").
  * the route a user has without the call, in the same run, "baseline_ms": the table copied to the host ("host_copy_ms"), then per transfer locate_keys for the
    two keys, words.indexed_transfer on the host copy's two records and update_records ("loop_ms").  "baseline_over_call" is their ratio.
Both ways must leave the same table, the same tree (every level), the same roots and the same (p, s) ("equal_baseline"), and the cut call the same table, tree
and every second root ("equal_cut"), before a time is reported; the exit status says so.  No ratio or time was fixed in advance.  dev tool.
usage: python tools/transfer_time.py [--log-records 20] [--reps 7] [--cuts 4,12] [--out FILE]"""
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

K, A, LENGTH = 8, 8, 55
START = 1 << 40  # every member's balance before a batch
KINDS = ["merkle_locate", "merkle_balances", "merkle_transfer_records", "merkle_segments", "sha256_records", "merkle_record_rows", "merkle_updates"]


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


def _table(rng, depth):
    """(np.uint8 [2^depth, LENGTH], the members as uint64): the sentinel record and 2^(depth-1) - 1 members in ascending order in the lower half, each with the
    balance START in bytes [2K, 2K + A), the upper half all zero"""
    n, live = 1 << depth, 1 << (depth - 1)
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=live + 4096, dtype=np.uint64))[: live - 1]
    assert len(keys) == live - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = np.zeros((n, LENGTH), dtype=np.uint8)
    table[:live] = rng.integers(0, 256, size=(live, LENGTH), dtype=np.uint8)
    table[:live, :K] = lo.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, 2 * K: 2 * K + A] = np.frombuffer(START.to_bytes(A, "big"), dtype=np.uint8)
    return table, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cuts", default="4,12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    cuts = [int(x) for x in a.cuts.split(",")]
    base = {"tool": "transfer_time", "records": n, "length": LENGTH, "key_bytes": K, "amount_bytes": A, "reps": a.reps, "cuts": cuts}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    torch = ctx.torch
    rng = np.random.default_rng(2032)
    image, members = _table(rng, depth)
    pristine = ctx.to_device(image).reshape(n, LENGTH)
    table = pristine.clone()
    tree = ctx.merkle_tree(depth)

    def restore():
        table.copy_(pristine)
        tree.set_records(0, table)
        ctx.sync()
        for kind in KINDS + ["merkle_level"]:
            ctx.timing_drain(kind)

    def as_keys(values):
        return values.astype(">u8").view(np.uint8).reshape(len(values), K).copy()

    for nk in (255, 1020):
        pairs = np.array([rng.choice(len(members), size=2, replace=False) for _ in range(nk)])  # (random members: an account seldom occurs twice, as in a user's batch)
        f, t = as_keys(members[pairs[:, 0]]), as_keys(members[pairs[:, 1]])
        amounts = [int(x) for x in rng.integers(0, START // 4, size=nk)]
        walls, kerns, got = [], {k: [] for k in KINDS}, None
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            got = tree.transfer_keys(table, f, t, amounts, amount_bytes=A, roots=True)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ks = {k: ctx.timing_drain(k)[1] for k in KINDS}
            if r:
                walls.append(wall)
                for k in KINDS:
                    kerns[k].append(ks[k])
        d_table, d_levels, d_roots, d_index = table.clone(), [tree.nodes(l).clone() for l in range(depth + 1)], got[2], got[1]
        # the cut call
        cut_walls, cut_segs, cut = [], [], None
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            cut = tree.transfer_key_segments(table, f, t, amounts, cuts, amount_bytes=A)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ks = {k: ctx.timing_drain(k)[1] for k in KINDS}
            if r:
                cut_walls.append(wall)
                cut_segs.append(ks["merkle_segments"])
        good_cut = bool(torch.equal(table, d_table) and all(torch.equal(tree.nodes(l), d_levels[l]) for l in range(depth + 1)) and np.array_equal(cut[3], d_index)
                        and np.array_equal(cut[1][:, -1, 0], d_roots[:-1]) and np.array_equal(cut[2][:, -1, 1], d_roots[1:]))
        # the baseline: the table to the host, then one transfer at a time through the existing calls
        cc, ll, b_roots, b_index = [], [], None, None
        both = np.stack([f, t], axis=1)  # [nk, 2, K]
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            host = table.cpu().numpy()
            t1 = time.perf_counter()
            b_roots, b_index = [tree.root()], []
            for j in range(nk):
                at, status = tree.locate_keys(table, both[j])
                p, s = int(at[0]), int(at[1])
                idx, new = W.indexed_transfer(host[p].tobytes(), p, host[s].tobytes(), s, amounts[j], K, amount_bytes=A)
                _, roots = tree.update_records(table, idx, new, roots=True)
                host[idx] = new  # (the host copy follows the table, as the user's would)
                b_roots.append(roots[2].tobytes())
                b_index.append((p, s))
            ctx.sync()
            t2 = time.perf_counter()
            if r:
                cc.append((t1 - t0) * 1e3), ll.append((t2 - t1) * 1e3)
        good = bool(torch.equal(table, d_table) and all(torch.equal(tree.nodes(l), d_levels[l]) for l in range(depth + 1))
                    and [x.tobytes() for x in d_roots] == b_roots and d_index.tolist() == [list(x) for x in b_index])
        ok = ok and good and good_cut
        chain = [x + y + z for x, y, z in zip(kerns["sha256_records"], kerns["merkle_record_rows"], kerns["merkle_updates"])]
        _emit({**base, "transfers": nk, "unique_keys": int(len(np.unique(pairs))), "call_ms": _med(walls), "call_ms_all": _all(walls),
               "locate_kernel_ms": _med(kerns["merkle_locate"]), "locate_kernel_ms_all": _all(kerns["merkle_locate"]), "balances_kernel_ms": _med(kerns["merkle_balances"]),
               "balances_kernel_ms_all": _all(kerns["merkle_balances"]), "build_kernel_ms": _med(kerns["merkle_transfer_records"]),
               "build_kernel_ms_all": _all(kerns["merkle_transfer_records"]), "update_chain_ms": _med(chain), "cut_call_ms": _med(cut_walls), "cut_call_ms_all": _all(cut_walls),
               "segments_kernel_ms": _med(cut_segs), "host_copy_ms": _med(cc), "loop_ms": _med(ll), "baseline_ms": round(_med(cc) + _med(ll), 4),
               "baseline_over_call": round((_med(cc) + _med(ll)) / _med(walls), 1), "equal_baseline": good, "equal_cut": good_cut}, a.out)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
