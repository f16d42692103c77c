"""Same-box timing of Merkle READS with the path cut into level ranges (MerkleTree.path_segments / absent_segments: k_merkle_climb_rows of merkle.hip) on
the table the write calls are measured on: 2^--log-records records (default 20) of 55 bytes with 8-byte keys under a tree of that depth, every slot but one
a member.  One process; every leg is called once to warm up, then --reps times (default 7), and the medians are reported; kernel timing is ON in every
leg.  One JSON line per case, also appended to --out (default profiles/climb_time.jsonl).  A case is a number of statements (255, 1 020) and a cut list
([depth / 2] and [1]); its legs, all in the same run:
  * "paths_cut_call_ms" and "climb_kernel_ms": path_segments of random leaves from the call to its return (it waits for the stream, and asks for the root
    behind it), and the HIP-event time of its one launch (kind "merkle_climb_rows").
  * "paths_call_ms" / "paths_kernel_ms": the parent's own route, path_rows uncut (kind "merkle_paths").
  * "absent_cut_call_ms" and its kernels by kind ("merkle_locate", "merkle_absent_rows", "merkle_climb_rows"): absent_segments of absent random keys.
  * "absent_call_ms" and its kernels ("merkle_locate", "merkle_absent_rows", "merkle_paths"): absent_rows uncut.
  * "host_ms": what a user could do before -- path_rows, then every cut level's nodes gathered through torch indexing of MerkleTree.nodes(level) and
    brought to the host, and the segments' rows spliced with numpy.  Its rows and nodes are compared with path_segments' ("equal_host").
  * "extra_row_bytes": what the cut rows of the case have over the uncut rows, all statements together -- the bytes the cut call moves more over PCIe.
No ratio or time was fixed in advance.  dev tool.  usage: python tools/climb_time.py [--log-records 20] [--reps 7] [--out FILE]"""
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

K, LENGTH = 8, 55


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


def _reps(ctx, fn, kinds, reps):
    """(wall ms of each repetition, [kernel ms of each repetition] per kind, the last result): one warm-up call, then reps"""
    walls, kerns, out = [], [[] for _ in kinds], None
    for r in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ks = [ctx.timing_drain(k)[1] for k in kinds]
        if r:
            walls.append(wall)
            for acc, k in zip(kerns, ks):
                acc.append(k)
    return walls, kerns, out


def _table(rng, depth, length):
    """np.uint8 [2^depth, length]: the sentinel record and 2^depth - 1 members in ascending order (indexed_records' layout, built with numpy), random payloads"""
    n = 1 << depth
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=n + 4096, dtype=np.uint64))[: n - 1]
    assert len(keys) == n - 1
    lo = np.concatenate([np.zeros(1, dtype=np.uint64), keys])
    hi = np.concatenate([keys, np.full(1, (1 << 64) - 1, dtype=np.uint64)])
    table = rng.integers(0, 256, size=(n, length), dtype=np.uint8)
    table[:, :K] = lo.astype(">u8").view(np.uint8).reshape(n, K)
    table[:, K: 2 * K] = hi.astype(">u8").view(np.uint8).reshape(n, K)
    return table


def _index_bytes(values, levels):
    return np.ascontiguousarray(values.astype("<u4")).view(np.uint8).reshape(len(values), 4)[:, : (levels + 7) // 8]


def _host_segments(ctx, tree, idx, cuts):
    """path_segments by the routes that existed before it: the uncut rows, the cut levels' nodes through torch indexing, numpy splicing"""
    depth, n = tree.depth, len(idx)
    rows = tree.path_rows(idx)
    edges = [0] + list(cuts) + [depth]
    out, nodes = [], np.zeros((n, len(cuts) + 1, 32), dtype=np.uint8)
    for g, (lo, hi) in enumerate(zip(edges, edges[1:])):
        lv = hi - lo
        sibs = rows[:, 64 + 32 * lo: 64 + 32 * hi]
        low = _index_bytes((idx >> lo) & ((1 << lv) - 1), lv)
        if g == 0:
            out.append(np.concatenate([rows[:, :64], sibs, low], axis=1))
            continue
        at = ctx.torch.as_tensor((idx >> lo).astype(np.int64), device=ctx.device)
        node = tree.nodes(lo)[at].cpu().numpy()
        nodes[:, g - 1] = node
        words = node.reshape(n, 8, 4)[..., ::-1].reshape(n, 32)
        out.append(np.concatenate([words, np.zeros((n, 32), dtype=np.uint8), sibs, low], axis=1))
    nodes[:, -1] = np.frombuffer(tree.root(), dtype=np.uint8)
    return out, nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "climb_time.jsonl"))
    a = ap.parse_args()
    depth, n = a.log_records, 1 << a.log_records
    base = {"tool": "climb_time", "records": n, "length": LENGTH, "key_bytes": K, "reps": a.reps}
    ok = True

    ctx = mf.Context(mf.DEBUG, 0)
    ctx.set_timing(True)
    rng = np.random.default_rng(2031)
    table = ctx.to_device(_table(rng, depth, LENGTH)).reshape(n, LENGTH)
    tree = ctx.merkle_tree(depth)
    tree.set_records(0, table)
    ctx.sync()
    every = ["merkle_climb_rows", "merkle_paths", "merkle_locate", "merkle_absent_rows", "sha256_records", "merkle_level"]
    for kind in every:
        ctx.timing_drain(kind)
    uncut_row = 64 + 32 * depth + (depth + 7) // 8
    for nq in (255, 1020):
        idx = rng.integers(0, n, size=nq, dtype=np.int64).astype(np.uint32)
        keys = rng.integers(1, 255, size=(nq, K), dtype=np.uint8)  # (no byte 0x00 or 0xFF: no sentinel)
        pw, (pk,), p_rows = _reps(ctx, lambda: tree.path_rows(idx), ["merkle_paths"], a.reps)
        aw, (ak_l, ak_g, ak_p), (a_rows, a_index, a_status) = _reps(ctx, lambda: tree.absent_rows(table, keys), ["merkle_locate", "merkle_absent_rows", "merkle_paths"], a.reps)
        for cuts in ([depth // 2], [1]):
            cw, (ck,), (c_rows, c_nodes) = _reps(ctx, lambda: tree.path_segments(idx, cuts), ["merkle_climb_rows"], a.reps)
            sw, (sk_l, sk_g, sk_c), (s_rows, s_nodes, s_index, s_status) = _reps(
                ctx, lambda: tree.absent_segments(table, keys, cuts), ["merkle_locate", "merkle_absent_rows", "merkle_climb_rows"], a.reps)
            hw, _, (h_rows, h_nodes) = _reps(ctx, lambda: _host_segments(ctx, tree, idx, cuts), ["merkle_paths"], a.reps)
            edges = [0] + cuts + [depth]
            good = bool(all(np.array_equal(x, y) for x, y in zip(c_rows, h_rows)) and np.array_equal(c_nodes, h_nodes)
                        and np.array_equal(s_index, a_index) and np.array_equal(s_status, a_status) and not s_status.any()
                        and np.array_equal(s_rows[0][:, : 32 + K + LENGTH + 32 * cuts[0]], a_rows[:, : 32 + K + LENGTH + 32 * cuts[0]])
                        and all(np.array_equal(r[:, 64: 64 + 32 * (hi - lo)], a_rows[:, 32 + K + LENGTH + 32 * lo: 32 + K + LENGTH + 32 * hi])
                                for r, (lo, hi) in list(zip(s_rows, zip(edges, edges[1:])))[1:])
                        and np.array_equal(p_rows[:, :64], c_rows[0][:, :64]))
            ok = ok and good
            extra = nq * (sum(r.shape[1] for r in c_rows) - uncut_row)
            _emit({**base, "statements": nq, "cuts": cuts, "climb_kernel_ms": _med(ck), "climb_kernel_ms_all": _all(ck), "paths_cut_call_ms": _med(cw),
                   "paths_cut_call_ms_all": _all(cw), "paths_call_ms": _med(pw), "paths_call_ms_all": _all(pw), "paths_kernel_ms": _med(pk),
                   "paths_cut_minus_uncut_ms": round(_med(cw) - _med(pw), 4), "absent_cut_call_ms": _med(sw), "absent_cut_call_ms_all": _all(sw),
                   "absent_cut_locate_kernel_ms": _med(sk_l), "absent_cut_gather_kernel_ms": _med(sk_g), "absent_cut_climb_kernel_ms": _med(sk_c),
                   "absent_call_ms": _med(aw), "absent_call_ms_all": _all(aw), "absent_locate_kernel_ms": _med(ak_l), "absent_gather_kernel_ms": _med(ak_g),
                   "absent_paths_kernel_ms": _med(ak_p), "absent_cut_minus_uncut_ms": round(_med(sw) - _med(aw), 4), "host_ms": _med(hw), "host_ms_all": _all(hw),
                   "host_over_paths_cut_call": round(_med(hw) / _med(cw), 2), "extra_row_bytes": extra, "equal_host": good}, a.out)
    tree.close()
    ctx.set_timing(False)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
