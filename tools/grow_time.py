"""Same-box timing of growing a tree and its indexed table on the device (MerkleTree.grow: k_grow_nodes, k_grow_spine, k_grow_table of merkle.hip) next to
the route a user had before it: a rebuild.  One process; every leg is called --warmups times (default 3), then --reps times (default 20), and the medians
are reported.  One JSON line per case, also appended to --out (default profiles/grow_time.jsonl).  A case is a growth (depth 19 -> 20, 20 -> 21) and a key
width and record length ((8, 55), (32, 71)); the old table is half full (load_keys of 2^(d-1) random keys):
  * "grow_ms": grow(D, table) from the call to the end of a sync behind it -- the allocation of the new nodes and of the new table inside --, and by HIP
    events in the same calls "kernels_ms" (kind "merkle_grow", "launches" of them) and "table_kernel_ms" (its last launch, k_grow_table); from grow(D,
    length=L) calls, which launch the first two alone, "nodes_kernel_ms" (k_grow_nodes) and "spine_kernel_ms" (k_grow_spine).  "nodes_gbps" and "table_gbps"
    are the two streaming launches' bytes a second: 32 (2^(d+1) - 1) bytes read and 32 (2^(D+1) - 1 - (D - d)) written; 2^d length read and 2^D length
    written.  "roots_ms": the same call with roots=True, which waits itself.
  * the REBUILD route, in the same run, "rebuild_ms": a fresh tree of the new depth (merkle_tree), a device copy of the table into a zeroed larger tensor,
    set_records(0, whole table), sync; "rebuild_kernels_ms" its "sha256_records" + "merkle_level" launches (the fresh tree's zero levels among them).
    "rebuild_over_grow" is the ratio.
Both routes must leave the same table, the same levels and the same root, which is words.grown_root of the old one ("equal_rebuild"), before a time is
reported; the exit status says so.  No ratio was fixed in advance.  dev tool.
usage: python tools/grow_time.py [--reps 20] [--warmups 3] [--out FILE]"""
import argparse
import ctypes
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

KINDS = ["merkle_grow", "sha256_records", "merkle_level", "merkle_sort", "merkle_load"]


def _emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def _med(xs):
    return round(statistics.median(xs), 4)


def _drain(ctx, kind):
    """(launches, total ms, last launch's ms) of a timing kind"""
    count, rows, total, last = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double(), ctypes.c_float()
    ctx._chk(ctx.lib.mfh_timing_drain(ctx._h, kind.encode(), ctypes.byref(count), ctypes.byref(total), ctypes.byref(rows), ctypes.byref(last)))
    return int(count.value), float(total.value), float(last.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_time.jsonl"))
    a = ap.parse_args()
    base = {"tool": "grow_time", "reps": a.reps, "warmups": a.warmups}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    torch = ctx.torch
    rng = np.random.default_rng(2041)
    for d, D in ((19, 20), (20, 21)):
        for K, length in ((8, 55), (32, 71)):
            n, N, nk = 1 << d, 1 << D, 1 << (d - 1)
            keys = np.unique(rng.integers(1, 255, size=(nk + nk // 8 + 64, K), dtype=np.uint8), axis=0)  # (no byte 0x00 or 0xFF: no sentinel)
            keys = keys[rng.permutation(len(keys))[:nk]]
            assert len(keys) == nk
            tree = ctx.merkle_tree(d)
            table = ctx.zeros(n * length).reshape(n, length)
            assert tree.load_keys(table, keys, rng.integers(0, 256, size=(nk, length - 2 * K), dtype=np.uint8)) == (0, None)
            old_root = tree.root()
            walls, kern, tab, launches = [], [], [], 0
            grown = new = None
            for r in range(a.warmups + a.reps):
                if grown is not None:
                    grown.close()
                    del new
                ctx.sync()
                for kind in KINDS:
                    _drain(ctx, kind)
                t0 = time.perf_counter()
                grown, new = tree.grow(D, table)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                launches, k_ms, t_ms = _drain(ctx, "merkle_grow")
                if r >= a.warmups:
                    walls.append(wall), kern.append(k_ms), tab.append(t_ms)
            nodes, spine, roots_ms = [], [], []
            for r in range(a.warmups + a.reps):
                alone = tree.grow(D, length=length)
                ctx.sync()
                _, k_ms, s_ms = _drain(ctx, "merkle_grow")
                alone.close()
                t0 = time.perf_counter()
                again, view, (r0, r1) = tree.grow(D, table, roots=True)
                wall = (time.perf_counter() - t0) * 1e3
                again.close()
                del view
                _drain(ctx, "merkle_grow")
                if r >= a.warmups:
                    nodes.append(k_ms - s_ms), spine.append(s_ms), roots_ms.append(wall)
            # the rebuild route
            rebuild, rkern = [], []
            fresh = whole = None
            for r in range(a.warmups + a.reps):
                if fresh is not None:
                    fresh.close()
                    del whole
                ctx.sync()
                for kind in KINDS:
                    _drain(ctx, kind)
                t0 = time.perf_counter()
                fresh = ctx.merkle_tree(D)
                whole = torch.zeros((N, length), dtype=torch.uint8, device=ctx.device)
                whole[:n].copy_(table)
                fresh.set_records(0, whole)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                k_ms = _drain(ctx, "sha256_records")[1] + _drain(ctx, "merkle_level")[1]
                if r >= a.warmups:
                    rebuild.append(wall), rkern.append(k_ms)
            good = bool(torch.equal(new, whole) and all(torch.equal(grown.nodes(l), fresh.nodes(l)) for l in range(D + 1))
                        and grown.root() == fresh.root() == W.grown_root(old_root, d, D, length) == r1 and r0 == old_root and tree.root() == old_root)
            ok = ok and good
            nodes_bytes = 32 * ((2 << d) - 1) + 32 * ((2 << D) - 1 - (D - d))
            table_bytes = (n + N) * length
            _emit({**base, "depth": d, "new_depth": D, "key_bytes": K, "length": length, "keys": nk, "grow_ms": _med(walls), "kernels_ms": _med(kern),
                   "launches": launches, "nodes_kernel_ms": _med(nodes), "spine_kernel_ms": _med(spine), "table_kernel_ms": _med(tab),
                   "nodes_gbps": round(nodes_bytes / (_med(nodes) * 1e6), 1), "table_gbps": round(table_bytes / (_med(tab) * 1e6), 1), "roots_ms": _med(roots_ms),
                   "rebuild_ms": _med(rebuild), "rebuild_kernels_ms": _med(rkern), "rebuild_over_grow": round(_med(rebuild) / _med(walls), 1),
                   "equal_rebuild": good}, a.out)
            for t in (grown, fresh, tree):
                t.close()
            del new, whole, table
            for kind in KINDS:
                _drain(ctx, kind)
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
