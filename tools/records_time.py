"""Same-box timing of SHA-256 of whole records on the device (Context.sha256_records, MerkleTree.set_records: k_sha256_records of merkle.hip) for
2^--log-records records (default 20).  One process; every leg is called once to warm up, then --reps times (default 7), and the medians are reported.
One JSON line per leg, also appended to --out (default profiles/records_time.jsonl):
  * level: the yardstick (b), measured first and in this process: builds of depth D and D - 1 (D = --log-records) from a device tensor, kernel sums of kind
    "merkle_level"; a build one level shallower lacks exactly the widest level, so the difference is the time of 2^(D - 1) compressions by k_merkle_level,
    "ns_per_compression".  Also the build's call time, what set_records stands next to.
  * records: for lengths 55, 64 and 119 bytes, packed and at a stride of length + 1: sha256_records from a device tensor -- "call_ms" from the call to the
    end of a sync (the call itself only queues), "kernel_ms" the launch's HIP-event time (kind "sha256_records"); "yardstick_b_ms" = blocks x records x
    ns_per_compression, and "kernel_over_b" their ratio: what assembling blocks from unaligned bytes costs on top of the arithmetic both kernels share.
    64 digests of every leg are checked against hashlib.  With the packed legs, the yardstick (a), what a user did before: hashlib.sha256 over the same
    records on the host, then an upload and set_leaves ("host_hash_ms", "upload_set_leaves_ms"; --host-reps times, default 3: it takes about a second).
  * set_records: all 2^D records of 55 bytes, packed, hashed into the leaves of a depth-D tree and the tree rebuilt: call and kernel times (both kinds),
    next to the build's; the root is checked against the tree built from the host digests.
No time was fixed in advance.  dev tool.  usage: python tools/records_time.py [--log-records 20] [--reps 7] [--host-reps 3] [--out FILE]"""
import argparse
import hashlib
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


def _timed(ctx, fn, kinds):
    """(wall ms to the end of a sync, [kernel ms of each kind], result) of one call"""
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, [ctx.timing_drain(k)[1] for k in kinds], out


def _reps(ctx, fn, kinds, reps):
    walls, kerns, out = [], [[] for _ in kinds], None
    for r in range(reps + 1):
        wall, ks, out = _timed(ctx, fn, kinds)
        if r:
            walls.append(wall)
            for acc, k in zip(kerns, ks):
                acc.append(k)
    return walls, kerns, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    base = {"tool": "records_time", "records": n, "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    g = torch.Generator(device="cpu")
    g.manual_seed(2027)

    # ---- yardstick (b): the tree's own compressions at its widest level
    leaves = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(ctx.device)
    kern, call = {}, {}
    for dd in (depth, depth - 1):
        tree = ctx.merkle_tree(dd)
        w, (k,), _ = _reps(ctx, lambda: tree.set_leaves(0, leaves[: 1 << dd]), ["merkle_level"], a.reps)
        kern[dd], call[dd] = _med(k), _med(w)
        tree.close()
    ns_comp = (kern[depth] - kern[depth - 1]) * 1e6 / (1 << (depth - 1))
    _emit({**base, "leg": "level", "build_depth": depth, "build_call_ms": call[depth], "build_kernel_ms": kern[depth], "shallower_kernel_ms": kern[depth - 1],
           "widest_level_parents": 1 << (depth - 1), "widest_level_us": round((kern[depth] - kern[depth - 1]) * 1e3, 2),
           "ns_per_compression": round(ns_comp, 5)}, a.out)
    del leaves

    # ---- the records legs
    rng = np.random.default_rng(2028)
    packed55 = None
    for length in (55, 64, 119):
        blocks = (length + 9 + 63) // 64
        for stride in (length, length + 1):
            buf = torch.randint(0, 256, ((n - 1) * stride + length + 64,), dtype=torch.uint8, generator=g).to(ctx.device)
            view = torch.as_strided(buf, (n, length), (stride, 1), 0)
            w, (k,), digests = _reps(ctx, lambda: ctx.sha256_records(view), ["sha256_records"], a.reps)
            picks = [0, 1, 255, 256, n - 1] + [int(x) for x in rng.integers(0, n, size=59)]
            got = digests[picks].cpu().numpy()
            rows = view[picks].cpu().numpy()
            good = all(got[i].tobytes() == hashlib.sha256(rows[i].tobytes()).digest() for i in range(len(picks)))
            ok = ok and good
            b_ms = blocks * n * ns_comp / 1e6
            res = {**base, "leg": "records", "length": length, "stride": stride, "blocks": blocks, "call_ms": _med(w), "call_ms_all": _all(w),
                   "kernel_ms": _med(k), "kernel_ms_all": _all(k), "record_gbytes_per_s": round(n * length / (_med(k) * 1e6), 1),
                   "yardstick_b_ms": round(b_ms, 4), "kernel_over_b": round(_med(k) / b_ms, 3), "digests_equal_hashlib": bool(good)}
            if stride == length:  # yardstick (a): the host's way
                host = view.cpu().numpy()
                hh, uu = [], []
                tree = ctx.merkle_tree(depth)
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    hd = b"".join(hashlib.sha256(r).digest() for r in host)
                    t1 = time.perf_counter()
                    tree.set_leaves(0, np.frombuffer(hd, dtype=np.uint8))
                    ctx.sync()
                    t2 = time.perf_counter()
                    hh.append((t1 - t0) * 1e3), uu.append((t2 - t1) * 1e3)
                ctx.timing_drain("merkle_level")
                res.update({"host_reps": a.host_reps, "host_hash_ms": _med(hh), "upload_set_leaves_ms": _med(uu),
                            "host_way_over_call": round((_med(hh) + _med(uu)) / _med(w), 1)})
                if length == 55:
                    packed55 = (view, tree.root())
                tree.close()
            _emit(res, a.out)

    # ---- set_records of every leaf: hash and build in one call
    view, want_root = packed55
    tree = ctx.merkle_tree(depth)
    w, (kr, kl), _ = _reps(ctx, lambda: tree.set_records(0, view), ["sha256_records", "merkle_level"], a.reps)
    good = tree.root() == want_root
    ok = ok and good
    _emit({**base, "leg": "set_records", "length": 55, "depth": depth, "call_ms": _med(w), "call_ms_all": _all(w), "records_kernel_ms": _med(kr),
           "levels_kernel_ms": _med(kl), "build_call_ms": call[depth], "build_kernel_ms": kern[depth], "root_equals_host_built_tree": bool(good)}, a.out)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
