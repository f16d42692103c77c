"""Same-box timing of Context.circuit_assign (mfh_circuit_assign) against Circuit.assign, default size (D = 2^15, M = 21 845).
The circuit is the one of test_default_size_circuit_batch: 16 public inputs, 3 000 private inputs and 13 500 random AND / OR / XOR / NOT gates.
Printed (one JSON line, also written to --out):
  * load: circuit_load once (levelising on the host, the upload);
  * call: the median wall time of circuit_assign for --nb statements (packing the input bits, staging, the launch, the copies back; the call synchronises);
  * kernel: k_circuit_eval alone (HIP events of mfh_set_timing, kind "circuit_assign");
  * python: Circuit.assign for --py statements, scaled to --nb (the rows are checked equal).
dev tool.  usage: python tools/circuit_assign_time.py [--nb 1020] [--reps 7] [--py 1020] [--out FILE]"""
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
from c_lwe_snarks_amd import circuit  # noqa: E402


def random_circuit(rng, npub, npriv, ngates):
    c = circuit.Circuit()
    ws = c.public(npub) + c.private(npriv)
    for _ in range(ngates):
        kind = ("XOR", "AND", "OR", "NOT")[int(rng.integers(0, 4))]
        a, b = (ws[int(rng.integers(0, len(ws)))] for _ in range(2))
        ws.append(c.NOT(a) if kind == "NOT" else getattr(c, kind)(a, b))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1020)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--py", type=int, default=1020, help="statements timed through Circuit.assign")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = mf.DEFAULT
    npub, npriv, ngates = 16, 3000, 13500
    rng = np.random.default_rng(55)
    c = random_circuit(rng, npub, npriv, ngates)
    cc = c.compile(p)
    bits = rng.integers(0, 2, size=(a.nb, npub + npriv), dtype=np.uint8)
    ctx = mf.Context(p, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prog = ctx.circuit_load(cc)
    load_ms = (time.perf_counter() - t0) * 1e3
    ctx.circuit_assign(prog, bits)  # first call: staging buffers
    call, kern = [], []
    ctx.set_timing(True)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        witness, holds = ctx.circuit_assign(prog, bits)
        call.append((time.perf_counter() - t0) * 1e3)
        n, tot, _ = ctx.timing_drain("circuit_assign")
        kern.append(tot)
    ctx.set_timing(False)
    npy = min(a.py, a.nb)
    t0 = time.perf_counter()
    ref = [c.assign(bits[b, :npub].tolist(), bits[b, npub:].tolist()) for b in range(npy)]
    py_ms = (time.perf_counter() - t0) * 1e3 / npy
    same = all(witness[b].tobytes() == ref[b] for b in range(npy))
    lvl = np.zeros(cc.nwires + 1, dtype=np.int64)
    nin = cc.nwires - len(cc.gates)
    for g, (op, x, y) in enumerate(cc.gates.tolist()):
        lvl[nin + 1 + g] = 1 + max(lvl[x], lvl[y])
    depth = int(lvl.max())
    res = {"tool": "circuit_assign_time", "d": p.d, "m": p.m, "nb": a.nb, "npub": npub, "npriv": npriv, "ngates": ngates, "depth": depth,
           "load_ms": round(load_ms, 3), "call_ms": round(statistics.median(call), 3), "call_ms_all": [round(x, 3) for x in call],
           "kernel_ms": round(statistics.median(kern), 3), "kernel_ms_all": [round(x, 3) for x in kern],
           "python_ms_per_statement": round(py_ms, 3), "python_statements_timed": npy, "python_ms_for_nb": round(py_ms * a.nb, 1),
           "python_over_call": round(py_ms * a.nb / statistics.median(call), 1), "rows_equal": bool(same), "holds_all": bool(holds.all())}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    prog.close()
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
