"""Same-box timing of the bulk load and the invariant check of an indexed table on the device (MerkleTree.load_keys / check_table: key_sort = k_sort_tiles +
k_sort_merge, k_load_entries, k_load_dups, k_load_records, k_chain_check, k_leaf_check, k_node_check of merkle.hip) for a table of 2^--log-records records
(default 20).  One process; every leg is called --warmups times (default 3), then --reps times (default 20), and the medians are reported.  One JSON line per
case, also appended to --out (default profiles/load_time.jsonl).  A case is a key width and record length ((8, 55), (32, 71)) and a number of random keys
(2^(D-1) and 2^D - 1), each with length - 2 key_bytes payload bytes:
  * "load_ms": load_keys of the HOST keys and payloads from the call to its return -- the upload of nk (key_bytes + payload_bytes) bytes included --, and by HIP
    events in the same calls "sort_kernel_ms" (kind "merkle_sort", "sort_launches" of them; "merge_gbps" = the bytes the merge passes read and write,
    2 passes nk (kw + 1) 4, over the passes' share of that time, the tile sort's taken as one launch's mean), "build_kernel_ms" (the last launch of
    "merkle_load": k_load_records), "load_kernels_ms" (all of "merkle_load") and "tree_ms" ("sha256_records" + "merkle_level").
  * the HOST route, in the same run, "host_ms": np.lexsort over the keys' big-endian 64-bit words, vectorised record assembly, to_device of the whole table,
    set_records, sync -- "host_sort_ms", "host_build_ms", "host_upload_ms" -- with --host-reps repeats (default: --reps).  Not the Python loop of
    words.indexed_records, which would flatter the device.  "host_over_load" is the ratio.
  * "check_ms": check_table on the result, with "check_kernels_ms" ("merkle_check" + "merkle_sort" + "sha256_records"); the host route "host_check_ms": the
    table copied to the host plus words.indexed_check (the chain alone: the host route has no check of leaves and nodes).
Both routes must leave the same table and the same root, and both checks must agree ("equal_host"), before a time is reported; the exit status says so.
No ratio was fixed in advance.  dev tool.  usage: python tools/load_time.py [--log-records 20] [--reps 20] [--warmups 3] [--host-reps N] [--out FILE]"""
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

TILE = 1024  # mf::kSortTile (csrc/merkle_sort.hpp)
KINDS = ["merkle_sort", "merkle_load", "merkle_check", "sha256_records", "merkle_level"]


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


def _host_table(keys, pay, depth, length):
    """(table, sort seconds, build seconds): the table of words.indexed_records(keys, depth, length, pay), vectorised"""
    n, K = keys.shape
    t0 = time.perf_counter()
    cols = np.ascontiguousarray(keys).view(">u8").astype(np.uint64)  # K = 8, 32: whole 64-bit words, big-endian
    order = np.lexsort(tuple(cols[:, j] for j in range(cols.shape[1] - 1, -1, -1)))
    t1 = time.perf_counter()
    table = np.zeros((1 << depth, length), dtype=np.uint8)
    sk = keys[order]
    table[1: n + 1, :K] = sk
    table[:n, K: 2 * K] = sk
    table[n, K: 2 * K] = 0xFF
    table[1: n + 1, 2 * K: 2 * K + pay.shape[1]] = pay[order]
    return table, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    host_reps = a.reps if a.host_reps is None else a.host_reps
    base = {"tool": "load_time", "records": n, "reps": a.reps, "warmups": a.warmups, "host_reps": host_reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    torch = ctx.torch
    rng = np.random.default_rng(2040)
    for K, length in ((8, 55), (32, 71)):
        kw, P = (K + 3) // 4, length - 2 * K
        tree = ctx.merkle_tree(depth)
        table = ctx.zeros(n * length).reshape(n, length)
        for nk in (n // 2, n - 1):
            keys = np.unique(rng.integers(1, 255, size=(nk + nk // 8 + 64, K), dtype=np.uint8), axis=0)  # (no byte 0x00 or 0xFF: no sentinel)
            keys = keys[rng.permutation(len(keys))[:nk]]
            assert len(keys) == nk
            pay = rng.integers(0, 256, size=(nk, P), dtype=np.uint8)
            passes = max(0, (-(-nk // TILE) - 1).bit_length())
            walls, sort, build, load, tre, launches = [], [], [], [], [], 0
            for r in range(a.warmups + a.reps):
                table.fill_(0xA5)
                ctx.sync()
                for kind in KINDS:
                    _drain(ctx, kind)
                t0 = time.perf_counter()
                got = tree.load_keys(table, keys, pay)
                ctx.sync()
                wall = (time.perf_counter() - t0) * 1e3
                assert got == (0, None)
                (launches, s_ms, _), (_, l_ms, b_ms) = _drain(ctx, "merkle_sort"), _drain(ctx, "merkle_load")
                t_ms = _drain(ctx, "sha256_records")[1] + _drain(ctx, "merkle_level")[1]
                if r >= a.warmups:
                    walls.append(wall), sort.append(s_ms), build.append(b_ms), load.append(l_ms), tre.append(t_ms)
            d_table, d_root = table.clone(), tree.root()
            checks, ckern = [], []
            for r in range(a.warmups + a.reps):
                t0 = time.perf_counter()
                d_check = tree.check_table(table, K)
                checks.append((time.perf_counter() - t0) * 1e3)
                ckern.append(sum(_drain(ctx, kind)[1] for kind in ("merkle_check", "merkle_sort", "sha256_records")))
            checks, ckern = checks[a.warmups:], ckern[a.warmups:]
            # the host route
            hs, hb, hu, hc, h_check = [], [], [], [], None
            for r in range(1 + host_reps):
                t0 = time.perf_counter()
                host, s_s, b_s = _host_table(keys, pay, depth, length)
                t1 = time.perf_counter()
                up = ctx.to_device(host).reshape(n, length)
                tree.set_records(0, up)
                ctx.sync()
                t2 = time.perf_counter()
                back = up.cpu().numpy()
                h_check = W.indexed_check(back, K)
                t3 = time.perf_counter()
                if r:
                    hs.append(s_s * 1e3), hb.append(b_s * 1e3), hu.append((t2 - t1) * 1e3), hc.append((t3 - t2) * 1e3)
            good = bool(torch.equal(up, d_table) and tree.root() == d_root and d_check == h_check == (0, nk + 1, None))
            ok = ok and good
            for kind in KINDS:
                _drain(ctx, kind)
            merge_ms = _med(sort) * passes / launches if launches else 0.0
            host_ms = _med(hs) + _med(hb) + _med(hu)
            _emit({**base, "key_bytes": K, "length": length, "keys": nk, "load_ms": _med(walls), "sort_kernel_ms": _med(sort), "sort_launches": launches,
                   "merge_gbps": round(2 * passes * nk * (kw + 1) * 4 / (merge_ms * 1e6), 1) if merge_ms else None, "build_kernel_ms": _med(build),
                   "load_kernels_ms": _med(load), "tree_ms": _med(tre), "host_sort_ms": _med(hs), "host_build_ms": _med(hb), "host_upload_ms": _med(hu),
                   "host_ms": round(host_ms, 4), "host_over_load": round(host_ms / _med(walls), 1), "check_ms": _med(checks), "check_kernels_ms": _med(ckern),
                   "host_check_ms": _med(hc), "host_check_over_check": round(_med(hc) / _med(checks), 1), "equal_host": good}, a.out)
            del up, d_table
        tree.close()
        del table
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
