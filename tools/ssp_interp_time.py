"""Same-box timing of mfh_ssp_from_rows against mfh_ssp_upload of the identical image, default size (D = 2^15, M = 21 845).
The circuit is a random one of AND / OR / XOR / NOT gates filling about 30 000 of the 32 767 rows.  Printed (one JSON line, also written to --out):
  * first call of the context: builds t and its seed table, then interpolates;
  * warm calls: the median wall time of ssp_from_rows (host sorting of the rows, the 1 MB copy, the launches; the call synchronises);
  * kernel: the gather launches alone (k_interp + k_interp_sum, HIP events of mfh_set_timing, kind "ssp_interp");
  * upload: the median wall time of ssp_upload of the same image from host uint64 (5.7 GB over PCIe, reduced on the device);
  * the kernel's fraction of two bounds: writing the image once at HBM speed, and VALU issue of the gather's instruction count.
dev tool.  usage: python tools/ssp_interp_time.py [--reps 5] [--out FILE]"""
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

HBM_SPEC_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6290.0  # MI355X HBM3E: spec, and a measured float4 copy
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9  # CUs x SIMDs x lanes per SIMD per clock x 2.4 GHz: full-rate VALU issue
VALU_PER_MAC = 378 / 32  # k_interp's inner loop (gfx950 ISA): 378 VALU instructions per nonzero for 32 coefficients


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = mf.DEFAULT
    rng = np.random.default_rng(1)
    c = random_circuit(rng, 16, 3000, 13500)
    cc = c.compile(p)
    ctx = mf.Context(p, 0)
    d_ssp = ctx.empty((p.m + 3) * p.d * 4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.ssp_from_rows(cc.rows, d_ssp)
    first_ms = (time.perf_counter() - t0) * 1e3
    warm, kern = [], []
    ctx.set_timing(True)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.ssp_from_rows(cc.rows, d_ssp)
        warm.append((time.perf_counter() - t0) * 1e3)
        n, tot, rows = ctx.timing_drain("ssp_interp")
        kern.append(tot)
    ctx.set_timing(False)
    host = ctx.ssp_to_host_u64(d_ssp)
    d_up = ctx.empty((p.m + 3) * p.d * 4)
    up = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.ssp_upload(host, d_up)
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)
    same = bool(torch.equal(d_up, d_ssp))
    nnz = int(cc.rows[0][-1]) + (p.d - 1 - cc.nrows)  # entries + padding rows of v_0 (no entry of the circuit is 0)
    write_bytes = (p.m + 3) * p.d * 4
    k_ms = statistics.median(kern)
    macs = nnz * p.d
    out = dict(
        tool="ssp_interp_time", d=p.d, m=p.m, nrows=cc.nrows, wires=cc.nwires, nnz_with_padding=nnz, reps=a.reps,
        first_call_ms=round(first_ms, 2), warm_call_ms=round(statistics.median(warm), 3), warm_call_ms_all=[round(x, 3) for x in warm],
        kernel_ms=round(k_ms, 3), kernel_ms_all=[round(x, 3) for x in kern],
        upload_ms=round(statistics.median(up), 2), upload_ms_all=[round(x, 2) for x in up], upload_over_warm_call=round(statistics.median(up) / statistics.median(warm), 1),
        images_identical=same,
        write_floor_ms_spec=round(write_bytes / HBM_SPEC_GBS / 1e6, 3), write_floor_ms_achievable=round(write_bytes / HBM_ACHIEVABLE_GBS / 1e6, 3),
        kernel_frac_of_write_floor_spec=round(write_bytes / HBM_SPEC_GBS / 1e6 / k_ms, 3),
        mac_per_s=round(macs / (k_ms * 1e-3), 1), valu_bound_ms=round(macs * VALU_PER_MAC / VALU_LANE_OPS * 1e3, 3),
        kernel_frac_of_valu_bound=round(macs * VALU_PER_MAC / VALU_LANE_OPS * 1e3 / k_ms, 3),
        seed_table_bytes=(p.d - 1) * ((p.d + 31) // 32) * 4,
    )
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()
    assert same, "ssp_from_rows and ssp_upload of its image differ"


if __name__ == "__main__":
    main()
