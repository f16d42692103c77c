"""Same-box timing of batches of sequential one-leaf updates (MerkleTree.update_rows: mfh_merkle_update_rows, k_merkle_update_level / _store of
merkle.hip): 255 and 1 020 random updates of trees of depth 10 and 20.  One process; every leg is called once to warm up, then --reps times (default 7),
and the medians are reported.  One JSON line per leg, also appended to --out (default profiles/updates_time.jsonl):
  * level: the yardstick (b), measured first and in this process as tools/records_time.py does: builds of depth 20 and 19 from a device tensor, kernel sums
    of kind "merkle_level"; their difference is the time of 2^19 compressions by k_merkle_level at its widest level, "ns_per_compression".
  * updates: per (depth, nupd), indices uniform over the leaves and new leaves in a device tensor:
      "call_ms"    update_rows(indices, new_leaves, roots=True) from the call to its return (it waits for the stream), kernel timing off;
      "kernel_ms"  the sum of the call's launches' HIP-event times (kind "merkle_updates") in further calls with kernel timing on, and "launches";
      "loop_ms"    the yardstick (a), what a user did before this call existed: for every update path_rows([i]) then set_leaves(i, leaf), then a sync
                   (--loop-reps times, default 3; kernel timing off), and "loop_over_call";
      "yardstick_b_ms" = nupd x depth x ns_per_compression, and "kernel_over_b".
    Both ways are first run once on two trees with the same leaves: the roots must agree, and every row's old leaf, siblings and index must be what
    path_rows gave in the loop ("rows_equal_loop", "root_equals_loop").
No time was fixed in advance.  dev tool.  usage: python tools/updates_time.py [--reps 7] [--loop-reps 3] [--out FILE]"""
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


def _loop(tree, idx, d_new):
    """the user's way before update_rows: one path and one one-leaf update at a time; returns the MerklePath rows"""
    rows = []
    for k, i in enumerate(idx):
        rows.append(tree.path_rows([i])[0])
        tree.set_leaves(i, d_new[k])
    return np.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "updates_time.jsonl"))
    a = ap.parse_args()
    base = {"tool": "updates_time", "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    g = torch.Generator(device="cpu")
    g.manual_seed(2029)
    all_leaves = torch.randint(0, 256, (1 << 20, 32), dtype=torch.uint8, generator=g).to(ctx.device)

    # ---- yardstick (b): the tree's own compressions at its widest level
    ctx.set_timing(True)
    kern = {}
    for dd in (20, 19):
        tree = ctx.merkle_tree(dd)
        ks = []
        for r in range(a.reps + 1):
            tree.set_leaves(0, all_leaves[: 1 << dd])
            k = ctx.timing_drain("merkle_level")[1]
            if r:
                ks.append(k)
        kern[dd] = _med(ks)
        tree.close()
    ctx.set_timing(False)
    ns_comp = (kern[20] - kern[19]) * 1e6 / (1 << 19)
    _emit({**base, "leg": "level", "build_kernel_ms": kern[20], "shallower_kernel_ms": kern[19], "widest_level_us": round((kern[20] - kern[19]) * 1e3, 2),
           "ns_per_compression": round(ns_comp, 5)}, a.out)

    rng = np.random.default_rng(2030)
    for depth in (10, 20):
        leaves = all_leaves[: 1 << depth]
        for nupd in (255, 1020):
            idx = [int(x) for x in rng.integers(0, 1 << depth, size=nupd)]
            d_new = torch.randint(0, 256, (nupd, 32), dtype=torch.uint8, generator=g).to(ctx.device)
            ta, tb = ctx.merkle_tree(depth), ctx.merkle_tree(depth)
            ta.set_leaves(0, leaves)
            tb.set_leaves(0, leaves)
            # once each on equal trees: the same rows, the same final root (and the warm-up of both)
            rows, roots = ta.update_rows(idx, d_new, roots=True)
            paths = _loop(tb, idx, d_new)
            rows_equal = bool(np.array_equal(rows[:, 64:96], paths[:, 32:64]) and np.array_equal(rows[:, 128:], paths[:, 64:]) and not rows[:, :64].any())
            root_equal = ta.root() == tb.root() == roots[-1].tobytes()
            ok = ok and rows_equal and root_equal

            walls = [_wall(ctx, lambda: ta.update_rows(idx, d_new, roots=True))[0] for _ in range(a.reps)]
            loops = [_wall(ctx, lambda: _loop(tb, idx, d_new))[0] for _ in range(a.loop_reps)]
            ctx.set_timing(True)
            ctx.timing_drain("merkle_updates")
            kerns, launches = [], 0
            for _ in range(a.reps):
                ta.update_rows(idx, d_new, roots=True)
                launches, ms, comps = ctx.timing_drain("merkle_updates")
                ok = ok and comps == nupd * depth
                kerns.append(ms)
            ctx.set_timing(False)
            b_ms = nupd * depth * ns_comp / 1e6
            _emit({**base, "leg": "updates", "depth": depth, "nupd": nupd, "call_ms": _med(walls), "call_ms_all": _all(walls), "kernel_ms": _med(kerns),
                   "kernel_ms_all": _all(kerns), "launches": launches, "loop_reps": a.loop_reps, "loop_ms": _med(loops), "loop_ms_all": _all(loops),
                   "loop_over_call": round(_med(loops) / _med(walls), 1), "us_per_update_call": round(_med(walls) * 1e3 / nupd, 3),
                   "us_per_update_loop": round(_med(loops) * 1e3 / nupd, 1), "yardstick_b_ms": round(b_ms, 6), "kernel_over_b": round(_med(kerns) / b_ms, 1),
                   "rows_equal_loop": rows_equal, "root_equals_loop": bool(root_equal)}, a.out)
            ta.close()
            tb.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
