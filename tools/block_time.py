"""Same-box timing of BLOCKS -- transfers, adjusts and writes in one device call (MerkleTree.apply_block: k_key_locate, k_window_gather, k_window_records and the
record-update chain of merkle.hip) -- against the route a caller has without it: the block cut into maximal runs of one kind, one existing call a run
(transfer_keys, adjust_keys, write_keys with roots=True).  The table has 2^--log-records records (default 20) of 55 bytes with 8-byte keys, half full: the
sentinel record and 2^(D-1) - 1 members in the lower half, the upper half all zero; amount_bytes = 8, and the writes' field is bytes [16, 24), the balance
itself, compare-and-set against the bytes the table holds.  One process; before every timed call the table is restored from a device copy and the tree rebuilt
(not timed); kernel timing is on in every leg.  One JSON line per block shape, also appended to --out (default profiles/block_time.jsonl).

Two shapes of --steps steps (default 1 020) on distinct random members:
  * "runs3": three runs of steps / 3 -- transfers, then adjusts, then writes: the per-run route is 3 calls;
  * "alternating": the kinds alternating step by step: every run has length 1, the per-run route is `steps` calls.
Per shape --rounds rounds (default 3), and in every round, one after the other, the legs "runs" (the yardstick: the existing calls) and "block"
(apply_block); a leg is called once to warm up, then --reps times (default 7).  Per leg the median of every round ("*_ms_rounds") and of all repeats
("*_ms"), from the first call to the last one's return (each waits for the stream), and by HIP events in the same calls the kernels' own times, summed over
the calls of one application: "locate_kernel_ms", "gather_kernel_ms" (k_balance_gather + k_field_gather for the runs, k_window_gather for the block),
"build_kernel_ms" (k_refield_records under its three kinds, k_window_records) and "update_chain_ms" ("sha256_records" + "merkle_record_rows" +
"merkle_updates").  "runs_range_ms": the min and max of the yardstick's round medians; "block_inside_or_below": the block's median of all repeats is not above
that max; "runs_over_block": the ratio of the two medians of all repeats.
The arguments of both legs are made once a block, outside the timed calls: the existing calls' arrays here, the block's by Block.columns(), which keeps them
("block_columns_once_ms": that one pass over the steps, timed on a copy of the block).
Both legs must leave the same table, the same tree (every level), the same roots and the same index ("equal") before a time is reported.  The exit status is 0
when "equal" held for every shape AND "block_inside_or_below" held for "runs3", the shape whose two routes launch the same chain; the "alternating" shape's
times are recorded without a criterion.  No ratio or time was fixed in advance.  dev tool.
usage: python tools/block_time.py [--log-records 20] [--steps 1020] [--reps 7] [--rounds 3] [--out FILE]"""
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
START = 1 << 40  # the balance of every member before a block
GATHER = ["merkle_balances", "merkle_fields", "merkle_block_windows"]
BUILD = ["merkle_transfer_records", "merkle_adjust_records", "merkle_write_records", "merkle_block_records"]
CHAIN = ["sha256_records", "merkle_record_rows", "merkle_updates"]
KINDS = ["merkle_locate"] + GATHER + BUILD + CHAIN


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
    as its balance, the upper half all zero"""
    n, live = 1 << depth, 1 << (depth - 1)
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=live + 4096, dtype=np.uint64))[: live - 1]
    assert len(keys) == live - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = np.zeros((n, LENGTH), dtype=np.uint8)
    table[:live] = rng.integers(0, 256, size=(live, LENGTH), dtype=np.uint8)
    table[:live, :K] = lo.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(live, K)
    table[:live, FIELD[0]: FIELD[1]] = np.frombuffer(START.to_bytes(A, "big"), dtype=np.uint8)
    return table, keys


def _runs(block):
    """the maximal runs of one kind: (kind, the steps)"""
    runs = []
    for s in block.steps:
        if runs and runs[-1][0] == s[0]:
            runs[-1][1].append(s)
        else:
            runs.append((s[0], [s]))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1020)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_time.jsonl"))
    a = ap.parse_args()
    depth, n, nk = a.log_records, 1 << a.log_records, a.steps
    base = {"tool": "block_time", "records": n, "length": LENGTH, "key_bytes": K, "amount_bytes": A, "write_field": list(FIELD), "steps": nk, "reps": a.reps, "rounds": a.rounds}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    torch = ctx.torch
    rng = np.random.default_rng(2051)
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

    # distinct members throughout, so that every compare-and-set meets the bytes the table held before the block
    key = lambda: next(picks).tobytes()  # noqa: E731  (picks: drawn anew for every shape, below)
    before = START.to_bytes(A, "big")

    def step(blk, kind):
        if kind == 0:
            blk.transfer(key(), key(), int(rng.integers(0, START // 8)))
        elif kind == 1:
            blk.adjust(key(), int(rng.integers(0, START // 8)), int(rng.integers(0, 2)))
        else:
            blk.write(key(), FIELD, int(rng.integers(START, 2 * START)).to_bytes(A, "big"), expect=before)

    shapes = {"runs3": [j * 3 // nk for j in range(nk)], "alternating": [j % 3 for j in range(nk)]}
    for shape, kinds in shapes.items():
        picks = iter(members[rng.choice(len(members), size=2 * nk, replace=False)].astype(">u8").view(np.uint8).reshape(2 * nk, K))
        blk = W.Block(K, A)
        for kind in kinds:
            step(blk, kind)
        runs = []
        for kind, steps in _runs(blk):  # the existing calls' arguments, made once
            k = np.frombuffer(b"".join(s[1] for s in steps), dtype=np.uint8).reshape(len(steps), K)
            if kind == 0:
                to = np.frombuffer(b"".join(s[2] for s in steps), dtype=np.uint8).reshape(len(steps), K)
                runs.append((lambda k=k, to=to, v=[s[3] for s in steps]: tree.transfer_keys(table, k, to, v, amount_bytes=A, roots=True)))
            elif kind == 1:
                runs.append((lambda k=k, v=[s[2] for s in steps], sd=[s[3] for s in steps]: tree.adjust_keys(table, k, v, sides=sd, amount_bytes=A, roots=True)))
            else:
                val = np.frombuffer(b"".join(s[3] for s in steps), dtype=np.uint8).reshape(len(steps), A)
                exp = np.frombuffer(b"".join(s[4] for s in steps), dtype=np.uint8).reshape(len(steps), A)
                runs.append((lambda k=k, val=val, exp=exp: tree.write_keys(table, k, val, FIELD, expect=exp, roots=True)))

        def per_run():
            return [call() for call in runs]

        def block():
            return tree.apply_block(table, blk)

        def comparable(leg, got):  # (index, roots) in one form for both legs, made outside the timed calls
            if leg == "block":
                return [int(x) for x in got.index.reshape(-1) if x != 0xFFFFFFFF], [x.tobytes() for x in got.roots[1:]]
            return [int(x) for _, idx, _ in got for x in np.asarray(idx).reshape(-1)], [x.tobytes() for _, _, r in got for x in r[1:]]

        # the block's arrays are made once a block (Block.columns, cached), as the yardstick's are above: what that one pass costs, on a copy
        fresh = W.Block(K, A)
        fresh.steps = list(blk.steps)
        t0 = time.perf_counter()
        fresh.columns()
        columns_ms = round((time.perf_counter() - t0) * 1e3, 4)
        legs = {"runs": per_run, "block": block}
        walls = {leg: [] for leg in legs}
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
                    kept[leg] = (comparable(leg, got), table.clone(), [tree.nodes(l).clone() for l in range(depth + 1)])
        (r_got, r_table, r_levels), (b_got, b_table, b_levels) = kept["runs"], kept["block"]
        good = bool(torch.equal(r_table, b_table) and all(torch.equal(x, y) for x, y in zip(r_levels, b_levels)) and r_got == b_got)
        ok = ok and good
        flat = {leg: [x for mine in walls[leg] for x in mine] for leg in legs}
        rounds = {leg: [_med(mine) for mine in walls[leg]] for leg in legs}
        total = lambda leg, kinds: _med([sum(xs) for xs in zip(*[kerns[leg][x] for x in kinds])])  # noqa: E731
        res = {**base, "shape": shape, "calls_per_application": {"runs": len(runs), "block": 1}, "updates": nk + kinds.count(0), "block_columns_once_ms": columns_ms}
        for leg in legs:
            res[f"{leg}_ms"] = _med(flat[leg])
            res[f"{leg}_ms_rounds"] = rounds[leg]
            res[f"{leg}_ms_min_max"] = [round(min(flat[leg]), 4), round(max(flat[leg]), 4)]
            res[f"{leg}_locate_kernel_ms"] = total(leg, ["merkle_locate"])
            res[f"{leg}_gather_kernel_ms"] = total(leg, GATHER)
            res[f"{leg}_build_kernel_ms"] = total(leg, BUILD)
            res[f"{leg}_update_chain_ms"] = total(leg, CHAIN)
        res.update({"runs_field_gather_kernel_ms": total("runs", ["merkle_fields"]), "runs_write_records_kernel_ms": total("runs", ["merkle_write_records"]),
                    "runs_range_ms": [min(rounds["runs"]), max(rounds["runs"])], "block_inside_or_below": bool(_med(flat["block"]) <= max(rounds["runs"])),
                    "runs_over_block": round(_med(flat["runs"]) / _med(flat["block"]), 2), "equal": good})
        ok = ok and (shape != "runs3" or res["block_inside_or_below"])
        _emit(res, a.out)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
