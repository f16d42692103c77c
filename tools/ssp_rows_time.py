"""Timings of the row SSP (mfh_ssp_set_rows, csrc/ssp_rows.hip), one JSON line per measurement, appended to profiles/ssp_rows_time.jsonl.
dev tool.

  registration  mfh_ssp_set_rows at d = 2^15 (first call of a context: builds the tree of t; second call: the tree kept) and at d = 2^20
                (a Circuit of 64 public + 20 000 private inputs and 470 000 gates; Circuit.build / compile / assign timed on the host too)
  witness       the witness pass of 255 statements at the default size: row interpolation against the dense k_witness_mm8q pass (mfh_witness_poly_mm),
                same circuit and bits, alternated A B A B in one process
  batch         mfh_prove_batch of 1020 statements at the default size, d_ssp = NULL (rows) against the dense SSP, alternated
  big           at d = 2^20: the witness pass of 255 statements, mfh_setup_messages (host setup scalars), and mfh_prove_batch_public of 255 statements
usage: python tools/ssp_rows_time.py [--parts registration,witness,batch,big] [--reps 5] [--out FILE]"""
import argparse
import ctypes
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
from c_lwe_snarks_amd import circuit as C  # noqa: E402
import oracle_lib as ol  # noqa: E402

P = mf.P
SEED = bytes((53 * i + 7) & 0xFF for i in range(40))


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def random_circuit(rng, npub, npriv, ngates):
    c = C.Circuit()
    ws = c.public(npub) + c.private(npriv)
    kinds = rng.integers(0, 4, ngates)
    ia, ib = rng.integers(0, 1 << 40, ngates), rng.integers(0, 1 << 40, ngates)
    for k in range(ngates):
        a, b = ws[ia[k] % len(ws)], ws[ib[k] % len(ws)]
        kd = kinds[k]
        ws.append(c.NOT(a) if kd == 3 else c.XOR(a, b) if kd == 0 else c.AND(a, b) if kd == 1 else c.OR(a, b))
    return c


def statements(c, rng, npub, npriv, nb):
    return [c.assign([int(x) for x in rng.integers(0, 2, npub)], [int(x) for x in rng.integers(0, 2, npriv)]) for _ in range(nb)]


def keys(ctx, rng, p):
    alpha, beta, s = (int(x) for x in rng.integers(1, P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    err = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    return alpha, beta, s, ctx.to_device(sk), ctx.to_device(err)


def draws(rng, nb):
    deltas = [int(x) for x in rng.integers(0, P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    return deltas, mags, signs


def witness_mm(ctx, d_ssp, bits_list, deltas, out):
    stride = (ctx.params.m + 6) // 8
    bits = b"".join(bytes(b[:stride]).ljust(stride, b"\0") for b in bits_list)
    dl = (ctypes.c_uint32 * len(bits_list))(*deltas)
    ctx._chk(ctx.lib.mfh_witness_poly_mm(ctx._h, mf._ptr(d_ssp), len(bits_list), bits, stride, ctypes.cast(dl, ctypes.c_void_p), mf._ptr(out)))


def ab(fa, fb, reps):
    fa(), fb()  # warm-up (fragment image, scratch, staging)
    ta, tb = [], []
    for _ in range(reps):
        t0 = now(); fa(); ta.append((now() - t0) * 1e3)
        t0 = now(); fb(); tb.append((now() - t0) * 1e3)
    return statistics.median(ta), statistics.median(tb), ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="registration,witness,batch,big")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssp_rows_time.jsonl"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    dev = torch.cuda.get_device_name(0)
    lines = []

    def emit(rec):
        rec = dict(rec, device=dev, measured="one MI355X, this tool")
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    rng = np.random.default_rng(7)
    p = mf.DEFAULT
    need_default = any(x in parts for x in ("registration", "witness", "batch"))
    if need_default:
        c = random_circuit(rng, 16, 3000, 13500)
        cc = c.compile(p)
        ctx = mf.Context(p, 0)
        ctx.set_seed(SEED)
    if "registration" in parts:
        t0 = now(); ctx.ssp_set_rows(cc.rows, lu_max=16); t1 = now(); ctx.ssp_set_rows(cc.rows, lu_max=16); t2 = now()
        emit(dict(what="registration", d=p.d, m=p.m, nrows=cc.nrows, lu_max=16, first_ms=(t1 - t0) * 1e3, again_ms=(t2 - t1) * 1e3,
                  note="first: the tree of t built (per context); again: the tree kept, rows + prefix only"))
    if "witness" in parts or "batch" in parts:
        dense = ctx.ssp_from_rows(cc.rows)
        ctx.ssp_set_rows(cc.rows, lu_max=16)
        ctx.ssp_prepare(None)
    if "witness" in parts:
        nb = 255
        st = statements(c, rng, 16, 3000, nb)
        dl = [int(x) for x in rng.integers(0, P, nb, dtype=np.uint64)]
        wa, wb = ctx.empty(nb * p.d * 4), ctx.empty(nb * p.d * 4)
        ma, mb, ta, tb = ab(lambda: witness_mm(ctx, None, st, dl, wa), lambda: witness_mm(ctx, dense, st, dl, wb), a.reps)
        assert bool((wa == wb).all())
        emit(dict(what="witness_pass_255", d=p.d, rows_ms=ma, dense_k_witness_mm8q_ms=mb, ratio=ma / mb, rows_all=ta, dense_all=tb, identical=True))
    if "batch" in parts:
        alpha, beta, s, sk, err = keys(ctx, rng, p)
        d_crs = ctx.setup(None, alpha, beta, s, sk, err).clone()
        nb = 1020
        st = statements(c, rng, 16, 3000, nb)
        deltas, mags, signs = draws(rng, nb)
        oa, ob = ctx.empty(nb * 5 * p.ct_limbs * 8), ctx.empty(nb * 5 * p.ct_limbs * 8)
        ma, mb, ta, tb = ab(lambda: ctx.prove_batch(d_crs, None, st, deltas, mags, signs, out=oa),
                            lambda: ctx.prove_batch(d_crs, dense, st, deltas, mags, signs, out=ob), a.reps)
        assert bool((oa == ob).all())
        emit(dict(what="prove_batch_1020", d=p.d, rows_ms=ma, dense_ms=mb, ratio=ma / mb, rows_all=ta, dense_all=tb, identical=True))
    if need_default:
        ctx.close()
    if "big" in parts:
        p = mf.Params(d=1 << 20, m=699050)
        t0 = time.perf_counter(); c = random_circuit(rng, 64, 20000, 470000); t1 = time.perf_counter()
        cc = c.compile(p); t2 = time.perf_counter()
        st = statements(c, rng, 64, 20000, 255); t3 = time.perf_counter()
        emit(dict(what="host_circuit_2pow20", gates=470000, nrows=cc.nrows, build_s=t1 - t0, compile_s=t2 - t1, assign_255_s=t3 - t2))
        ctx = mf.Context(p, 0)
        ctx.set_seed(SEED)
        t0 = now(); ctx.ssp_set_rows(cc.rows, lu_max=64); t1 = now(); ctx.ssp_set_rows(cc.rows, lu_max=64); t2 = now()
        emit(dict(what="registration", d=p.d, m=p.m, nrows=cc.nrows, lu_max=64, first_ms=(t1 - t0) * 1e3, again_ms=(t2 - t1) * 1e3))
        ctx.ssp_prepare(None)
        dl = [int(x) for x in rng.integers(0, P, 255, dtype=np.uint64)]
        w = ctx.empty(255 * p.d * 4)
        witness_mm(ctx, None, st, dl, w)
        tw = []
        for _ in range(max(2, a.reps // 2)):
            t0 = now(); witness_mm(ctx, None, st, dl, w); tw.append((now() - t0) * 1e3)
        alpha, beta, s, sk, err = keys(ctx, rng, p)
        t0 = now(); ctx.setup_messages(None, alpha, beta, s); t1 = now()
        emit(dict(what="witness_pass_255", d=p.d, rows_ms=statistics.median(tw), rows_all=tw, setup_messages_ms=(t1 - t0) * 1e3,
                  note="compare: the generator-defined witness pass, 700 ms per 255 statements (DESIGN 7)"))
        d_crs = ctx.setup_public(None, alpha, beta, s, 64, sk, err).clone()
        deltas, mags, signs = draws(rng, 255)
        ctx.prove_batch_public(d_crs, None, 64, st, deltas, mags, signs)
        t0 = now(); ctx.prove_batch_public(d_crs, None, 64, st, deltas, mags, signs); t1 = now()
        emit(dict(what="prove_batch_public_255", d=p.d, m=p.m, lu=64, ms=(t1 - t0) * 1e3))
        ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
