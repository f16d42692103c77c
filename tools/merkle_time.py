"""Same-box timing of the Merkle tree in device memory (Context.merkle_tree, merkle.hip) at --depth (default 20).
One process; every leg is called once to warm up, then --reps times (default 7), and the medians are reported.  One JSON line per leg, also appended to
--out (default profiles/merkle_time.jsonl):
  * build: set_leaves of all 2^depth leaves from a device tensor -- "call_ms" from the call to the end of a sync (the call itself only queues), and
    "kernel_ms" the sum of the depth launches of k_merkle_level (HIP events of mfh_set_timing, kind "merkle_level");
    ALTERNATED with the yardstick, the only way the library could compute these nodes on the GPU before: circuit_assign of
    words.Sha256Compress(chaining="iv", adds="sum") at D = 2^16, 1 020 statements a call (blocks = left || right of random nodes; the digests are checked
    against tests/sha256_ref.py).  Time per compression both ways and the ratio;
  * level: builds of depth - 1 and depth - 2 leaves: a build one level shallower lacks exactly the widest level, so the difference of the kernel sums
    is that one level's time ("level_kernel_us"), next to its VALU estimate;
  * update1 / update1024: one leaf, and 1 024 contiguous leaves from an odd index;
  * paths255 / paths1020: path_rows for random indices ("kernel_ms": kind "merkle_paths"); the rows' roots are checked against root() through
    tests/sha256_ref.py for 8 statements;
  * assign255 / assign1020 (skipped with --no-assign): circuit_assign of words.MerklePath(depth) on those rows at D = 2^20, M = 699 050, for scale;
    every computed root must equal root().
The estimate the measured kernel times stand next to is printed with the build leg: VALU issue alone, from the instruction counts
of the shipped k_merkle_level and the issue rates csrc/aes_dev.hpp records.
dev tool.  usage: python tools/merkle_time.py [--depth 20] [--reps 7] [--no-assign] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import c_lwe_snarks_amd as mf  # noqa: E402
import sha256_ref  # noqa: E402
from c_lwe_snarks_amd import words  # noqa: E402

# k_merkle_level as shipped (hipcc -O3, gfx950): v_alignbit_b32 + v_perm_b32 at ~4.3 SIMD-clocks a wave instruction, the other VALU at ~2.5
SLOW_VALU, FAST_VALU = 570 + 24, 352 + 235 + 126 + 96 + 16  # (16: the moves and the address arithmetic)
SIMDS, CLOCK_GHZ = 1024, 2.4


def valu_estimate_us(parents):
    """VALU issue alone: waves of 64 parents spread over the SIMDs"""
    waves_per_simd = -(-(-(-parents // 64)) // SIMDS)
    return waves_per_simd * (SLOW_VALU * 4.3 + FAST_VALU * 2.5) / (CLOCK_GHZ * 1e3)


def _emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _med(xs):
    return round(statistics.median(xs), 4)


def _all(xs):
    return [round(x, 4) for x in xs]


def _timed(ctx, fn, kind):
    """(wall ms to the end of a sync, kernel ms of `kind`, launches) of one call"""
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3
    n, ms, _ = ctx.timing_drain(kind)
    return wall, ms, n, out


def _unpack_row(row, depth):
    def node(k):
        b = bytes(row[32 + 32 * k: 64 + 32 * k])
        return b"".join(b[i: i + 4][::-1] for i in range(0, 32, 4))

    return node(0), [node(1 + l) for l in range(depth)], int.from_bytes(bytes(row[32 + 32 * (depth + 1):]), "little")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-assign", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.depth, 1 << a.depth
    base = {"tool": "merkle_time", "depth": depth, "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    g = torch.Generator(device="cpu")
    g.manual_seed(2020)
    leaves = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(ctx.device)
    t0 = time.perf_counter()
    tree = ctx.merkle_tree(depth)
    create_ms = (time.perf_counter() - t0) * 1e3

    # ---- build, alternated with the yardstick
    yp = mf.Params(d=1 << 16, m=43690)
    yst = words.Sha256Compress(chaining="iv", adds="sum")
    ycc = yst.circuit.compile(yp)
    yctx = mf.Context(yp, 0)
    yprog = yctx.circuit_load(ycc, state="auto")
    nb = 1020
    blocks = leaves[: 2 * nb].cpu().numpy().reshape(nb, 64)
    ybits = np.stack([yst.bits(blocks[b].tobytes()) for b in range(nb)])
    ctx.set_timing(True)
    yctx.set_timing(True)
    bw, bk, yw, yk = [], [], [], []
    for r in range(a.reps + 1):
        wall, kern, launches, _ = _timed(ctx, lambda: tree.set_leaves(0, leaves), "merkle_level")
        ywall, ykern, _, (ywit, yholds) = _timed(yctx, lambda: yctx.circuit_assign(yprog, ybits), "circuit_assign_sum")
        if r:
            bw.append(wall), bk.append(kern), yw.append(ywall), yk.append(ykern)
    yctx.set_timing(False)
    level1 = tree.nodes(1)[:nb].cpu().numpy()
    same = all(yst.digest_of(ywit[b]) == level1[b].tobytes() == sha256_ref.merkle_parent(blocks[b, :32].tobytes(), blocks[b, 32:].tobytes()) for b in range(nb))
    ok = ok and same and bool(yholds.all()) and launches == depth
    est = sum(valu_estimate_us((n >> l)) for l in range(1, depth + 1))
    _emit({**base, "leg": "build", "leaves": n, "compressions": n - 1, "create_ms": round(create_ms, 3), "launches": launches,
           "call_ms": _med(bw), "call_ms_all": _all(bw), "kernel_ms": _med(bk), "kernel_ms_all": _all(bk),
           "launch_and_gap_ms": round(_med(bw) - _med(bk), 4), "valu_estimate_ms": round(est / 1e3, 4),
           "valu_estimate_widest_level_us": round(valu_estimate_us(n >> 1), 2), "hbm_bytes": 96 * (n - 1),
           "ns_per_compression_call": round(_med(bw) * 1e6 / (n - 1), 3), "ns_per_compression_kernel": round(_med(bk) * 1e6 / (n - 1), 3),
           "yardstick": "circuit_assign of Sha256Compress(iv, sum), d = 2^16, 1020 statements", "yardstick_call_ms": _med(yw), "yardstick_call_ms_all": _all(yw),
           "yardstick_kernel_ms": _med(yk), "yardstick_ns_per_compression_call": round(_med(yw) * 1e6 / nb, 1),
           "yardstick_ns_per_compression_kernel": round(_med(yk) * 1e6 / nb, 1),
           "yardstick_over_tree_per_compression_call": round((_med(yw) / nb) / (_med(bw) / (n - 1)), 1),
           "yardstick_over_tree_per_compression_kernel": round((_med(yk) / nb) / (_med(bk) / (n - 1)), 1), "digests_equal": bool(same)}, a.out)
    yprog.close()
    yctx.close()

    # ---- single levels: a build one level shallower lacks exactly the widest level, so the difference of the kernel sums is that level's time
    prev = _med(bk)
    for dd in (depth - 1, depth - 2):
        if dd < 1:
            break
        small = ctx.merkle_tree(dd)
        k = []
        for r in range(a.reps + 1):
            _, kern, launches, _ = _timed(ctx, lambda: small.set_leaves(0, leaves[: 1 << dd]), "merkle_level")
            if r:
                k.append(kern)
        small.close()
        _emit({**base, "leg": "level", "build_depth": dd, "launches": launches, "kernel_ms": _med(k), "kernel_ms_all": _all(k),
               "level_parents": 1 << dd, "level_kernel_us": round((prev - _med(k)) * 1e3, 2), "level_valu_estimate_us": round(valu_estimate_us(1 << dd), 2),
               "level_hbm_bytes": 96 << dd}, a.out)
        prev = _med(k)

    # ---- updates: a one-leaf update is `depth` launches of one parent each, so its time is what the launches of the narrow top levels cost
    for name, first, count in (("update1", 12345, 1), ("update1024", 12345, 1024)):
        if first + count > n:
            first = 0
            count = min(count, n)
        new = torch.randint(0, 256, (count, 32), dtype=torch.uint8, generator=g).to(ctx.device)
        w, k = [], []
        for r in range(a.reps + 1):
            wall, kern, launches, _ = _timed(ctx, lambda: tree.set_leaves(first, new), "merkle_level")
            if r:
                w.append(wall), k.append(kern)
        leaves[first: first + count] = new
        parents = sum(((first + count - 1) >> l) - (first >> l) + 1 for l in range(1, depth + 1))
        _emit({**base, "leg": name, "first": first, "count": count, "parents": parents, "launches": launches, "call_ms": _med(w), "call_ms_all": _all(w),
               "kernel_ms": _med(k), "kernel_ms_all": _all(k), "kernel_us_per_launch": round(_med(k) * 1e3 / launches, 3),
               "call_us_per_launch": round(_med(w) * 1e3 / launches, 3)}, a.out)

    # ---- paths
    root = tree.root()
    rng = np.random.default_rng(2021)
    rows_of = {}
    for nb in (255, 1020):
        idx = rng.integers(0, n, size=nb)
        w, k = [], []
        for r in range(a.reps + 1):
            wall, kern, launches, rows = _timed(ctx, lambda: tree.path_rows(idx), "merkle_paths")
            if r:
                w.append(wall), k.append(kern)
        rows_of[nb] = rows
        good = True
        for b in range(8):
            leaf, sibs, index = _unpack_row(rows[b], depth)
            good = good and index == int(idx[b]) and sha256_ref.merkle_root(leaf, sibs, index) == root
        ok = ok and good
        _emit({**base, "leg": f"paths{nb}", "nb": nb, "row_bytes": int(rows.shape[1]), "launches": launches, "call_ms": _med(w), "call_ms_all": _all(w),
               "kernel_ms": _med(k), "kernel_ms_all": _all(k), "roots_equal": bool(good)}, a.out)
    ctx.set_timing(False)

    # ---- for scale: the witnesses of MerklePath(depth) on those rows
    if not a.no_assign:
        p = mf.Params(d=1 << 20, m=699050)
        st = words.MerklePath(depth)
        cc = st.circuit.compile(p)
        actx = mf.Context(p, 0)
        prog = actx.circuit_load(cc, state="auto")
        for nb, rows in rows_of.items():
            bits = np.unpackbits(rows, axis=1, bitorder="little")[:, : tree.nin]
            w = []
            for r in range(a.reps + 1):
                actx.sync()
                t0 = time.perf_counter()
                witness, holds = actx.circuit_assign(prog, bits)
                if r:
                    w.append((time.perf_counter() - t0) * 1e3)
            good = bool(holds.all()) and all(st.root_of(witness[b]) == root for b in range(nb))
            ok = ok and good
            _emit({**base, "leg": f"assign{nb}", "nb": nb, "d": p.d, "m": p.m, "state": prog.state, "nwires": cc.nwires, "call_ms": _med(w),
                   "call_ms_all": _all(w), "roots_equal_tree_root": bool(good)}, a.out)
        prog.close()
        actx.close()
    tree.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
