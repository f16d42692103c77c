"""Same-box timing of batches of sequential record updates (MerkleTree.update_records: mfh_merkle_update_records -- k_sha256_records, k_record_gather, the
level and store kernels of mfh_merkle_update_rows, k_record_store of merkle.hip): 255 and 1 020 random updates of a table of 2^9 records of 55 bytes and
its tree of depth 9.  One process; every leg is called once to warm up, then --reps times (default 7), and the medians are reported.  One JSON line per
nupd, also appended to --out (default profiles/record_updates_time.jsonl).  The table and the new records are device tensors in every leg:
  "call_ms"     update_records(table, indices, new_records, roots=True) from the call to its return (it waits for the stream), kernel timing off;
  "kernel_ms"   the sum of the call's launches' HIP-event times in further calls with kernel timing on, by kind: "sha256_records", "merkle_record_rows"
                (gather + table store) and "merkle_updates", with their launch counts;
  "a_ms"        the yardstick (a), what gives the same rows, roots, tree and table without this call: Context.sha256_records(new), update_rows, the old
                records of the rows (the table's records at the indices, downloaded, or an earlier update's new record: "the last earlier update at my
                index", tracked in numpy) spliced with the new records (downloaded) and update_rows' siblings into the rows in numpy, then the table
                written back by index assignment from the last update at each index; then a sync.  "a_host_new_ms" is the same with the new records
                also at hand in host memory (no download of them): the cheaper of the two is what "call_over_a" compares against;
  "b_ms"        the yardstick (b): update_rows alone on the same indices with the digests already computed; "call_minus_b_ms" is the price of the hash,
                the gather, the table store and the wider rows.
All three ways are first run once on equal tables and trees: rows, roots, final tree root and table must agree ("equal").
No time was fixed in advance.  dev tool.  usage: python tools/record_updates_time.py [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import c_lwe_snarks_amd as mf  # noqa: E402

DEPTH, LENGTH = 9, 55


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


def _wall(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def _parents_way(ctx, tree, table, idx, d_new, h_new=None):
    """the same rows, roots, tree and table from what the library had before update_records"""
    n = len(idx)
    digests = ctx.sha256_records(d_new)
    rows_u, roots = tree.update_rows(idx, digests, roots=True)
    # the last earlier update at my index, and whether I am the last at it
    order = np.argsort(idx, kind="stable")
    same = idx[order][1:] == idx[order][:-1]
    prev = np.full(n, -1, dtype=np.int64)
    prev[order[1:][same]] = order[:-1][same]
    last = np.ones(n, dtype=bool)
    last[order[:-1][same]] = False
    d_idx = torch.from_numpy(idx).to(table.device)
    new = d_new.cpu().numpy() if h_new is None else h_new
    old = table[d_idx].cpu().numpy()
    old = np.where((prev >= 0)[:, None], new[np.maximum(prev, 0)], old)
    rows = np.concatenate([np.zeros((n, 64), dtype=np.uint8), old, new, rows_u[:, 128:]], axis=1)
    keep = torch.from_numpy(np.flatnonzero(last)).to(table.device)
    table[d_idx[keep]] = d_new[keep]
    return rows, roots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_updates_time.jsonl"))
    a = ap.parse_args()
    base = {"tool": "record_updates_time", "reps": a.reps, "depth": DEPTH, "length": LENGTH}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    g = torch.Generator(device="cpu")
    g.manual_seed(2031)
    start = torch.randint(0, 256, (1 << DEPTH, LENGTH), dtype=torch.uint8, generator=g)
    rng = np.random.default_rng(2032)
    kinds = ("sha256_records", "merkle_record_rows", "merkle_updates")
    for nupd in (255, 1020):
        idx = rng.integers(0, 1 << DEPTH, size=nupd).astype(np.int64)
        h_new = torch.randint(0, 256, (nupd, LENGTH), dtype=torch.uint8, generator=g)
        d_new = h_new.to(ctx.device)
        h_new = h_new.numpy()
        trees = [ctx.merkle_tree(DEPTH) for _ in range(3)]
        tables = [start.to(ctx.device) for _ in range(2)]
        ta, tb, tc = trees
        ta.set_records(0, tables[0])
        tb.set_records(0, tables[1])
        tc.set_records(0, tables[1])
        # once each on equal tables and trees: the same rows, roots, root and table (and the warm-up of all)
        rows, roots = ta.update_records(tables[0], idx, d_new, roots=True)
        rows_a, roots_a = _parents_way(ctx, tb, tables[1], idx, d_new)
        digests = ctx.sha256_records(d_new)
        tc.update_rows(idx, digests, roots=True)
        equal = bool(np.array_equal(rows, rows_a) and np.array_equal(roots, roots_a) and ta.root() == tb.root() == tc.root() == roots[-1].tobytes()
                     and torch.equal(tables[0], tables[1]))
        ok = ok and equal

        walls, was, wahs, wbs = [], [], [], []
        for _ in range(a.reps):  # the three ways alternate
            walls.append(_wall(ctx, lambda: ta.update_records(tables[0], idx, d_new, roots=True))[0])
            was.append(_wall(ctx, lambda: _parents_way(ctx, tb, tables[1], idx, d_new))[0])
            wahs.append(_wall(ctx, lambda: _parents_way(ctx, tb, tables[1], idx, d_new, h_new))[0])
            wbs.append(_wall(ctx, lambda: tc.update_rows(idx, digests, roots=True))[0])
        ctx.set_timing(True)
        for kind in kinds:
            ctx.timing_drain(kind)
        kerns, launches = {k: [] for k in kinds}, {}
        for _ in range(a.reps):
            ta.update_records(tables[0], idx, d_new, roots=True)
            for kind in kinds:
                n, ms, _ = ctx.timing_drain(kind)
                launches[kind] = n
                kerns[kind].append(ms)
        ctx.set_timing(False)
        ok = ok and launches == {"sha256_records": 1, "merkle_record_rows": 2, "merkle_updates": DEPTH + 1}
        a_best = min(_med(was), _med(wahs))
        _emit({**base, "nupd": nupd, "call_ms": _med(walls), "call_ms_all": _all(walls), "a_ms": _med(was), "a_ms_all": _all(was), "a_host_new_ms": _med(wahs),
               "a_host_new_ms_all": _all(wahs), "b_ms": _med(wbs), "b_ms_all": _all(wbs), "call_over_a": round(_med(walls) / a_best, 3),
               "call_minus_b_ms": round(_med(walls) - _med(wbs), 4), "us_per_update_call": round(_med(walls) * 1e3 / nupd, 3),
               "kernel_ms": {k: _med(v) for k, v in kerns.items()}, "kernel_ms_total": round(sum(_med(v) for v in kerns.values()), 4), "launches": launches,
               "equal": equal}, a.out)
        for t in trees:
            t.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
