"""Same-box timing of batches of writes by key, plain and compare-and-set, on an indexed table on the device (MerkleTree.write_keys / write_key_segments:
k_key_locate, k_field_gather, k_write_records and the record-update chain of merkle.hip) for a table of 2^--log-records records (default 20) of 55 bytes with
8-byte keys, half full: the sentinel record and 2^(D-1) - 1 members in the lower half, the upper half all zero.  The field is bytes [16, 24) -- where
adjust_keys has its balance, so both calls rewrite the same bytes of the same records.  One process; before every call the table is restored from a device
copy and the tree rebuilt (not timed); kernel timing is on in every leg.  One JSON line per case, also appended to --out (default profiles/write_time.jsonl).

A case is --steps writes per call (default 1 020) on random members, "plain" or "expect" (every step expects the bytes the table holds: START's):
  * --rounds rounds (default 3), and in every round, one after the other, the legs "adjust" (adjust_keys(roots=True) on the same keys and table, deposits and
    withdrawals mixed: the yardstick), "write" (write_keys(roots=True)) and "write_cut" (write_key_segments under --cuts, default 10); a leg is called once to
    warm up, then --reps times (default 7).  Per leg the median of every round ("*_call_ms_rounds") and of all repeats ("*_call_ms"), from the call to its
    return (it waits for the stream), and by HIP events in the same calls "locate_kernel_ms" (kind "merkle_locate"), "fields_kernel_ms" ("merkle_fields": the
    gather, 0 for plain writes), "build_kernel_ms" ("merkle_write_records"), "update_chain_ms" ("sha256_records" + "merkle_record_rows" + "merkle_updates") and,
    cut, "segments_kernel_ms".
  * "adjust_range_ms": the min and max of adjust_keys' round medians; "write_inside_or_below": write_keys' median of all repeats is not above that max;
    "write_over_adjust": the ratio of the two medians of all repeats.
  * the route a user has without the call, in the same run, "baseline_ms": the table copied to the host ("host_copy_ms"), then per step locate_keys for the
    key, words.indexed_write on the host copy's record and update_records ("loop_ms"), --baseline-reps times (default 3).  "baseline_over_call" is their ratio.
Both ways must leave the same table, the same tree (every level), the same roots and the same index ("equal_baseline"), and the cut call the same table, tree
and roots ("equal_cut"), before a time is reported.  The exit status says whether every comparison held.  No ratio or time was fixed in advance.  dev tool.
usage: python tools/write_time.py [--log-records 20] [--steps 1020] [--reps 7] [--rounds 3] [--cuts 10] [--out FILE]"""
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

K, A, LENGTH, FIELD = 8, 8, 55, (16, 24)
F = FIELD[1] - FIELD[0]
START = 1 << 40  # bytes [16, 24) of every member before a batch, as a big-endian integer: adjust_keys' balance
KINDS = ["merkle_locate", "merkle_fields", "merkle_write_records", "merkle_balances", "merkle_adjust_records", "merkle_segments", "sha256_records", "merkle_record_rows",
         "merkle_updates"]


def _emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def _med(xs):
    return round(statistics.median(xs), 4)


def _table(rng, depth):
    """(np.uint8 [2^depth, LENGTH], the members as uint64): the sentinel record and 2^(depth-1) - 1 members in ascending order in the lower half, each with START
    in bytes [16, 24), the upper half all zero"""
    n, live = 1 << depth, 1 << (depth - 1)
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=live + 4096, dtype=np.uint64))[: live - 1]
    assert len(keys) == live - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = np.zeros((n, LENGTH), dtype=np.uint8)
    table[:live] = rng.integers(0, 256, size=(live, LENGTH), dtype=np.uint8)
    table[:live, :K] = lo.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, FIELD[0]: FIELD[1]] = np.frombuffer(START.to_bytes(F, "big"), dtype=np.uint8)
    return table, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1020)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--cuts", default="10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_time.jsonl"))
    a = ap.parse_args()
    depth, n, nk = a.log_records, 1 << a.log_records, a.steps
    cuts = [int(x) for x in a.cuts.split(",")]
    base = {"tool": "write_time", "records": n, "length": LENGTH, "key_bytes": K, "field": list(FIELD), "steps": nk, "reps": a.reps, "rounds": a.rounds, "cuts": cuts}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    torch = ctx.torch
    rng = np.random.default_rng(2041)
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

    picks = rng.choice(len(members), size=nk, replace=False)  # (random members: a key seldom occurs twice, as in a user's batch)
    k = members[picks].astype(">u8").view(np.uint8).reshape(nk, K).copy()
    values = rng.integers(0, 256, size=(nk, F), dtype=np.uint8)
    before = np.tile(np.frombuffer(START.to_bytes(F, "big"), dtype=np.uint8), (nk, 1))
    amounts = [int(x) for x in rng.integers(0, START // 4, size=nk)]
    sides = rng.integers(0, 2, size=nk).astype(np.uint8)

    for case in ("plain", "expect"):
        expect = before if case == "expect" else None
        legs = {"adjust": lambda: tree.adjust_keys(table, k, amounts, sides=sides, amount_bytes=A, roots=True),
                "write": lambda: tree.write_keys(table, k, values, FIELD, expect=expect, roots=True),
                "write_cut": lambda: tree.write_key_segments(table, k, values, FIELD, cuts, expect=expect)}
        walls = {leg: [] for leg in legs}  # per round
        kerns = {leg: {x: [] for x in KINDS} for leg in legs}
        kept = {}
        for _ in range(a.rounds):
            for leg, call in legs.items():
                mine = []
                for r in range(a.reps + 1):
                    restore()
                    t0 = time.perf_counter()
                    got = call()
                    ctx.sync()
                    wall = (time.perf_counter() - t0) * 1e3
                    ks = {x: ctx.timing_drain(x)[1] for x in KINDS}
                    if r:
                        mine.append(wall)
                        for x in KINDS:
                            kerns[leg][x].append(ks[x])
                walls[leg].append(mine)
                if leg not in kept:
                    kept[leg] = (got, table.clone(), [tree.nodes(l).clone() for l in range(depth + 1)])
        (w_rows, w_index, w_roots), w_table, w_levels = kept["write"]
        (c_rows, c_nodes, c_index), c_table, c_levels = kept["write_cut"]
        good_cut = bool(torch.equal(c_table, w_table) and all(torch.equal(x, y) for x, y in zip(c_levels, w_levels)) and np.array_equal(c_index, w_index)
                        and np.array_equal(c_nodes[:, -1, 0], w_roots[:-1]) and np.array_equal(c_nodes[:, -1, 1], w_roots[1:]))
        # the baseline: the table to the host, then one step at a time through the existing calls
        cc, ll, b_roots, b_index = [], [], None, None
        for r in range(a.baseline_reps + 1):
            restore()
            t0 = time.perf_counter()
            host = table.cpu().numpy()
            t1 = time.perf_counter()
            b_roots, b_index = [tree.root()], []
            for j in range(nk):
                at, status = tree.locate_keys(table, k[j: j + 1])
                i = int(at[0])
                new = W.indexed_write(host[i].tobytes(), FIELD, values[j].tobytes(), K, expect=None if expect is None else expect[j].tobytes())
                _, roots = tree.update_records(table, [i], new.reshape(1, LENGTH), roots=True)
                host[i] = new  # (the host copy follows the table, as the user's would)
                b_roots.append(roots[1].tobytes())
                b_index.append(i)
            ctx.sync()
            t2 = time.perf_counter()
            if r:
                cc.append((t1 - t0) * 1e3), ll.append((t2 - t1) * 1e3)
        good = bool(torch.equal(table, w_table) and all(torch.equal(tree.nodes(l), w_levels[l]) for l in range(depth + 1))
                    and [x.tobytes() for x in w_roots] == b_roots and w_index.tolist() == b_index)
        ok = ok and good and good_cut
        flat = {leg: [x for mine in walls[leg] for x in mine] for leg in legs}
        rounds = {leg: [_med(mine) for mine in walls[leg]] for leg in legs}
        kern = lambda leg, x: _med(kerns[leg][x])  # noqa: E731
        chain = lambda leg: _med([x + y + z for x, y, z in zip(kerns[leg]["sha256_records"], kerns[leg]["merkle_record_rows"], kerns[leg]["merkle_updates"])])  # noqa: E731
        res = {**base, "case": case, "unique_keys": int(len(np.unique(picks)))}
        for leg in legs:
            res[f"{leg}_call_ms"] = _med(flat[leg])
            res[f"{leg}_call_ms_rounds"] = rounds[leg]
            res[f"{leg}_call_ms_min_max"] = [round(min(flat[leg]), 4), round(max(flat[leg]), 4)]
            res[f"{leg}_locate_kernel_ms"] = kern(leg, "merkle_locate")
            res[f"{leg}_update_chain_ms"] = chain(leg)
        res.update({"adjust_balances_kernel_ms": kern("adjust", "merkle_balances"), "adjust_build_kernel_ms": kern("adjust", "merkle_adjust_records"),
                    "write_fields_kernel_ms": kern("write", "merkle_fields"), "write_build_kernel_ms": kern("write", "merkle_write_records"),
                    "write_cut_fields_kernel_ms": kern("write_cut", "merkle_fields"), "write_cut_build_kernel_ms": kern("write_cut", "merkle_write_records"),
                    "write_cut_segments_kernel_ms": kern("write_cut", "merkle_segments"),
                    "adjust_range_ms": [min(rounds["adjust"]), max(rounds["adjust"])], "write_inside_or_below": bool(_med(flat["write"]) <= max(rounds["adjust"])),
                    "write_over_adjust": round(_med(flat["write"]) / _med(flat["adjust"]), 3), "host_copy_ms": _med(cc), "loop_ms": _med(ll),
                    "baseline_ms": round(_med(cc) + _med(ll), 4), "baseline_over_call": round((_med(cc) + _med(ll)) / _med(flat["write"]), 1), "equal_baseline": good,
                    "equal_cut": good_cut})
        _emit(res, a.out)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
