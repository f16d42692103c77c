"""Same-box A/B of the public-input batch prover: mfh_prove_batch_public (lu public wires) against mfh_prove_batch on the same statements, default instance.
Interleaved A B A B ... so that clock and power drift land on both sides; the median of each side and their ratio are printed, one JSON line per regime.
dev tool.
Statements: "same" = every proof the instance's satisfying input (all valid; every k_add_public block selects the same public rows), "mixed" = each its own random
statement bits over the instance's witness (the representative case for the V step: almost every block of 16 statements selects all lu rows; the inputs do not satisfy
the SSP, so both sides take the Euclidean polynomial step alike).
usage: python tools/public_input_time.py [--n 1020] [--lu 10] [--reps 7] [--regimes transient,resident] [--statements same,mixed] [--out FILE]"""
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
import bench  # noqa: E402
import c_lwe_snarks_amd as mf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1020)
    ap.add_argument("--lu", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--regimes", default="transient,resident")
    ap.add_argument("--statements", default="same,mixed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = mf.DEFAULT
    ctx = mf.Context(p, 0)
    ctx.set_seed(bytes((37 * i + 11) & 0xFF for i in range(40)))
    inst = bench.build_instance(mf, ctx, torch, p, 20260101)
    ctx.ssp_prepare(inst["d_ssp"])
    d_crs = ctx.setup_public(inst["d_ssp"], inst["alpha"], inst["beta"], inst["s"], a.lu, inst["sk"], inst["err"])
    rng = np.random.default_rng(5)
    nb = a.n
    ub = (a.lu + 7) // 8

    def statements(kind):
        out = []
        for b in range(nb):
            x = bytearray(inst["bits"])
            if kind == "mixed":
                u = int.from_bytes(rng.bytes(ub), "little") & ((1 << a.lu) - 1)
                for i in range(a.lu):
                    x[i >> 3] = (x[i >> 3] & ~(1 << (i & 7)) | (((u >> i) & 1) << (i & 7))) & 0xFF
            out.append(bytes(x))
        return out

    deltas = [int(x) for x in rng.integers(0, mf.P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(5)] * nb
    vk = ctx.derive_vk(inst["d_ssp"], inst["s"], a.lu)
    lines = []
    for regime, kind in [(r, k) for r in a.regimes.split(",") for k in a.statements.split(",")]:
        stmts = statements(kind)
        image = None
        if regime == "resident":
            image = ctx.crs_expand_mm(d_crs)
            ctx.set_resident_mm(image)
        out = ctx.empty(nb * 5 * p.ct_limbs * 8)
        run = {
            "plain": lambda: ctx.prove_batch(d_crs, inst["d_ssp"], stmts, deltas, mags, signs, out=out),
            "public": lambda: ctx.prove_batch_public(d_crs, inst["d_ssp"], a.lu, stmts, deltas, mags, signs, out=out),
        }
        for k in ("plain", "public"):  # warm-up: allocations, transient image, exact-division state
            run[k]()
        torch.cuda.synchronize()
        ok = ctx.to_host(ctx.verify_public(vk, a.lu, inst["alpha"], inst["beta"], inst["sk"], out, [x[:ub] for x in stmts]))
        ms = {"plain": [], "public": []}
        for _ in range(a.reps):
            for k in ("plain", "public"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run[k]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = dict(tool="public_input_time", regime=regime, statements=kind, nproofs=nb, lu=a.lu, reps=a.reps, accepted=int(ok.sum()),
                    plain_ms_median=round(med["plain"], 3), public_ms_median=round(med["public"], 3),
                    public_over_plain=round(med["public"] / med["plain"], 4),
                    plain_ms=[round(x, 3) for x in ms["plain"]], public_ms=[round(x, 3) for x in ms["public"]])
        print(json.dumps(line), flush=True)
        lines.append(line)
        if image is not None:
            ctx.set_resident_mm(None)
            del image
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
