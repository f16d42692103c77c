"""Same-box timing of batches of deposits and withdrawals on the accounts of an indexed table on the device (MerkleTree.adjust_keys / adjust_key_segments:
k_key_locate, k_balance_gather, k_adjust_records and the record-update chain of merkle.hip) and of the table's supply (MerkleTree.total_balance: k_balance_sum,
k_balance_fold) for a table of 2^--log-records records (default 20) of 55 bytes with 8-byte keys and 8-byte balances, half full: the sentinel record and
2^(D-1) - 1 members in the lower half, the upper half all zero.  One process; before every call the table is restored from a device copy and the tree rebuilt
(not timed); every leg is called once to warm up, then --reps times (default 7), and the medians are reported; kernel timing is on in every leg.  One JSON
line per case, also appended to --out (default profiles/adjust_time.jsonl).

A case "adjusts" is a number of steps per call (255, 1 020) on random members, deposits and withdrawals mixed, each amount at most a quarter of what a member
starts with:
  * "call_ms": adjust_keys(roots=True) from the call to its return (it waits for the stream), and by HIP events in the same calls "locate_kernel_ms" (kind
    "merkle_locate"), "balances_kernel_ms" ("merkle_balances"), "build_kernel_ms" ("merkle_adjust_records") and "update_chain_ms" ("sha256_records" +
    "merkle_record_rows" + "merkle_updates").
  * "cut_call_ms": adjust_key_segments under --cuts (default 10) likewise, with "segments_kernel_ms" ("merkle_segments").
  * "transfer_call_ms", "transfer_update_chain_ms": transfer_keys(roots=True), the call this one stands beside, on the same table with the same keys as
    senders and as many other members as receivers: twice the record updates.
  * the route a user has without the call, in the same run, "baseline_ms": the table copied to the host ("host_copy_ms"), then per step locate_keys for the
    key, words.indexed_adjust on the host copy's record and update_records ("loop_ms").  "baseline_over_call" is their ratio.
Both ways must leave the same table, the same tree (every level), the same roots and the same index ("equal_baseline"), and the cut call the same table, tree
and roots ("equal_cut"), before a time is reported.
The case "supply": "call_ms" is total_balance from the call to its return, "sum_kernel_ms" the two launches of kind "merkle_balance_sum"; the yardstick
"locate_kernel_ms" is k_key_locate over 255 keys on the same table (locate_keys), which streams the same records; the host route "baseline_ms" is the table
copied to the host ("host_copy_ms") and summed with numpy ("host_sum_ms": lo < hi as big-endian uint64, the balances in two 32-bit halves).  "equal": both
give the same sum and live count.  The exit status says whether every comparison held.  No ratio or time was fixed in advance.  dev tool.
usage: python tools/adjust_time.py [--log-records 20] [--reps 7] [--cuts 10] [--out FILE]"""
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
KINDS = ["merkle_locate", "merkle_balances", "merkle_adjust_records", "merkle_transfer_records", "merkle_balance_sum", "merkle_segments", "sha256_records",
         "merkle_record_rows", "merkle_updates"]


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


def _host_supply(host):
    """(sum, live) of a host copy of the table with numpy: lo < hi as big-endian uint64, the balances summed in two 32-bit halves (no overflow below 2^32 records)"""
    lo = np.ascontiguousarray(host[:, :K]).view(">u8").reshape(-1)
    hi = np.ascontiguousarray(host[:, K: 2 * K]).view(">u8").reshape(-1)
    bal = np.ascontiguousarray(host[:, 2 * K: 2 * K + A]).view(">u8").reshape(-1).astype(np.uint64)
    live = lo < hi
    bal = bal[live]
    return (int((bal >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int((bal & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)), int(live.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cuts", default="10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjust_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    cuts = [int(x) for x in a.cuts.split(",")]
    base = {"tool": "adjust_time", "records": n, "length": LENGTH, "key_bytes": K, "amount_bytes": A, "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    torch = ctx.torch
    rng = np.random.default_rng(2033)
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
        picks = rng.choice(len(members), size=2 * nk, replace=False)  # (random members: an account seldom occurs twice, as in a user's batch)
        k, others = as_keys(members[picks[:nk]]), as_keys(members[picks[nk:]])
        amounts = [int(x) for x in rng.integers(0, START // 4, size=nk)]
        sides = rng.integers(0, 2, size=nk).astype(np.uint8)
        walls, kerns, got = [], {x: [] for x in KINDS}, None
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            got = tree.adjust_keys(table, k, amounts, sides=sides, amount_bytes=A, roots=True)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ks = {x: ctx.timing_drain(x)[1] for x in KINDS}
            if r:
                walls.append(wall)
                for x in KINDS:
                    kerns[x].append(ks[x])
        d_table, d_levels, d_roots, d_index = table.clone(), [tree.nodes(l).clone() for l in range(depth + 1)], got[2], got[1]
        # the cut call
        cut_walls, cut_segs, cut = [], [], None
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            cut = tree.adjust_key_segments(table, k, amounts, cuts, sides=sides, amount_bytes=A)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ks = {x: ctx.timing_drain(x)[1] for x in KINDS}
            if r:
                cut_walls.append(wall)
                cut_segs.append(ks["merkle_segments"])
        good_cut = bool(torch.equal(table, d_table) and all(torch.equal(tree.nodes(l), d_levels[l]) for l in range(depth + 1)) and np.array_equal(cut[2], d_index)
                        and np.array_equal(cut[1][:, -1, 0], d_roots[:-1]) and np.array_equal(cut[1][:, -1, 1], d_roots[1:]))
        # the call this one stands beside: transfers from the same keys, twice the record updates
        t_walls, t_chain = [], []
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            tree.transfer_keys(table, k, others, amounts, amount_bytes=A, roots=True)
            ctx.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ks = {x: ctx.timing_drain(x)[1] for x in KINDS}
            if r:
                t_walls.append(wall)
                t_chain.append(ks["sha256_records"] + ks["merkle_record_rows"] + ks["merkle_updates"])
        # the baseline: the table to the host, then one step at a time through the existing calls
        cc, ll, b_roots, b_index = [], [], None, None
        for r in range(a.reps + 1):
            restore()
            t0 = time.perf_counter()
            host = table.cpu().numpy()
            t1 = time.perf_counter()
            b_roots, b_index = [tree.root()], []
            for j in range(nk):
                at, status = tree.locate_keys(table, k[j: j + 1])
                i = int(at[0])
                new = W.indexed_adjust(host[i].tobytes(), amounts[j], int(sides[j]), K, amount_bytes=A)
                _, roots = tree.update_records(table, [i], new.reshape(1, LENGTH), roots=True)
                host[i] = new  # (the host copy follows the table, as the user's would)
                b_roots.append(roots[1].tobytes())
                b_index.append(i)
            ctx.sync()
            t2 = time.perf_counter()
            if r:
                cc.append((t1 - t0) * 1e3), ll.append((t2 - t1) * 1e3)
        good = bool(torch.equal(table, d_table) and all(torch.equal(tree.nodes(l), d_levels[l]) for l in range(depth + 1))
                    and [x.tobytes() for x in d_roots] == b_roots and d_index.tolist() == b_index)
        ok = ok and good and good_cut
        chain = [x + y + z for x, y, z in zip(kerns["sha256_records"], kerns["merkle_record_rows"], kerns["merkle_updates"])]
        _emit({**base, "case": "adjusts", "cuts": cuts, "steps": nk, "unique_keys": int(len(np.unique(picks[:nk]))), "call_ms": _med(walls), "call_ms_all": _all(walls),
               "locate_kernel_ms": _med(kerns["merkle_locate"]), "locate_kernel_ms_all": _all(kerns["merkle_locate"]), "balances_kernel_ms": _med(kerns["merkle_balances"]),
               "balances_kernel_ms_all": _all(kerns["merkle_balances"]), "build_kernel_ms": _med(kerns["merkle_adjust_records"]),
               "build_kernel_ms_all": _all(kerns["merkle_adjust_records"]), "update_chain_ms": _med(chain), "update_chain_ms_all": _all(chain), "cut_call_ms": _med(cut_walls),
               "cut_call_ms_all": _all(cut_walls), "segments_kernel_ms": _med(cut_segs), "transfer_call_ms": _med(t_walls), "transfer_call_ms_all": _all(t_walls),
               "transfer_update_chain_ms": _med(t_chain), "call_over_transfer_call": round(_med(walls) / _med(t_walls), 3), "host_copy_ms": _med(cc), "loop_ms": _med(ll),
               "baseline_ms": round(_med(cc) + _med(ll), 4), "baseline_over_call": round((_med(cc) + _med(ll)) / _med(walls), 1), "equal_baseline": good, "equal_cut": good_cut},
              a.out)

    # the supply
    restore()
    queries = as_keys(members[rng.choice(len(members), size=255, replace=False)])
    walls, sums, locs, got = [], [], [], None
    for r in range(a.reps + 1):
        for x in KINDS:
            ctx.timing_drain(x)
        t0 = time.perf_counter()
        got = tree.total_balance(table, K, amount_bytes=A)
        wall = (time.perf_counter() - t0) * 1e3
        launches, ms, rows = ctx.timing_drain("merkle_balance_sum")
        tree.locate_keys(table, queries)
        loc = ctx.timing_drain("merkle_locate")[1]
        if r:
            walls.append(wall), sums.append(ms), locs.append(loc)
            ok = ok and (launches, rows) == (2, n)
    cc, ss, host_got = [], [], None
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        host = table.cpu().numpy()
        t1 = time.perf_counter()
        host_got = _host_supply(host)
        t2 = time.perf_counter()
        if r:
            cc.append((t1 - t0) * 1e3), ss.append((t2 - t1) * 1e3)
    good = got == host_got == (START * (n // 2 - 1) + int.from_bytes(image[0, 2 * K: 2 * K + A].tobytes(), "big"), n // 2)
    ok = ok and good
    _emit({**base, "case": "supply", "call_ms": _med(walls), "call_ms_all": _all(walls), "sum_kernel_ms": _med(sums), "sum_kernel_ms_all": _all(sums),
           "table_gbytes_per_s": round(n * LENGTH / (_med(sums) * 1e6), 1), "locate_kernel_ms": _med(locs), "locate_kernel_ms_all": _all(locs),
           "sum_over_locate_kernel": round(_med(sums) / _med(locs), 2), "host_copy_ms": _med(cc), "host_sum_ms": _med(ss), "baseline_ms": round(_med(cc) + _med(ss), 4),
           "baseline_over_call": round((_med(cc) + _med(ss)) / _med(walls), 1), "live": got[1], "equal": good}, a.out)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
