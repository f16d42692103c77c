"""Same-box timing of Context.circuit_assign (mfh_circuit_assign) against Circuit.assign.
Legs (--leg, default all):
  * default: D = 2^15, M = 21 845, the circuit of test_default_size_circuit_batch (16 public inputs, 3 000 private inputs, 13 500 random AND / OR /
    XOR / NOT gates), LDS program (mfh_circuit_create), --nb statements;
  * 2p20: D = 2^20, M = 699 050, the circuit of test_two_pow_20_circuit_proved_and_verified (64 public, 20 000 private inputs, 470 000 random gates),
    device-memory program (circuit_load(state="global"), mfh_circuit_create_global), 255 and 1 020 statements;
  * chain: a 60 000-gate XOR / NOT chain (depth 60 000) on 40 000 inputs, global program, 100 statements: its time and launch count;
  * chacha: the ChaCha20 block statement (words.ChaCha20Block: 896 inputs, 31 746 gates, 512 equalities) at D = 2^16, M = 43 690, --nb statements,
    both kinds of mfh_circuit_create_ex program (kinds "circuit_assign_ex" / "circuit_assign_global_ex");
  * chacha_prove: prove_batch_public for 255 of those statements through the row SSP at D = 2^16 (median of --reps calls after one warm-up);
  * chacha_out: is the output pass free?  The ChaCha20 block statement (k_circuit_eval<true>) against the same circuit with its 512 block bits as
    computed outputs (k_circuit_eval<true, true>), the two programs called in turn in one process, --reps calls each; then the same comparison on a
    chain of 200 adds x += rotl(x, 1) (depth 6 400, 32 outputs), which tells a cost per output from a cost per level;
  * sha256: the SHA-256 compression statement (words.Sha256Compress, chaining value = IV: 768 inputs, 60 930 gates, 256 outputs) at D = 2^17,
    M = 87 381, device-memory program (kind "circuit_assign_global_out"), 255 and 1 020 statements;
  * sha256_prove: prove_batch_public for 255 of those statements through the row SSP at D = 2^17;
  * sha256_sum: the same statement written with weighted sums (words.Sha256Compress(adds="sum"): 27 346 gate wires, 368 WSUM heads) at D = 2^16,
    M = 43 690, LDS program (kind "circuit_assign_sum"), against the sha256 leg's circuit at D = 2^17: the two programs called in turn in one process,
    255 and 1 020 statements;
  * sha256_sum_prove: for 255 statements of each of the two, in one process: ssp_set_rows + ssp_prepare (the registration of the rows: up to 151 entries
    a row with sums, 3 - 6 without), one witness_poly call through the row SSP (its witness pass), setup_public, and prove_batch_public called in turn
    (median of min(--reps, 5) calls after one warm-up); "witness_plus_prove_ms" = the circuit_assign call + the batch proof.
  * merkle: the two whole statements, 255 statements each, every step once in one process: words.Sha256Message(100) at D = 2^17, M = 87 381, then
    words.MerklePath(20) (573 014 wires, 1 018 072 rows) at D = 2^20, M = 699 050 -- Circuit build and compile, circuit_load, circuit_assign,
    ssp_set_rows + ssp_prepare, the row check (ssp_rows_violations) against witness_poly_many through the row SSP on the same statements (calls
    alternated, median of 5 after one warm-up each; also the row check's kernel alone, kind "ssp_rows_violations"), setup_public,
    prove_batch_public (first call and a second) and verify_public; digests / roots checked against hashlib / tests/sha256_ref.py.
Printed per leg (one JSON line each, also appended to --out):
  * load: circuit_load once (levelising on the host, the upload);
  * call: the median wall time of circuit_assign (packing the input bits, staging, the launches, the copies back; the call synchronises);
  * kernel: the kernel launches alone (HIP events of mfh_set_timing, kind "circuit_assign" / "circuit_assign_global"), summed over a call's chunks;
  * python: Circuit.assign for --py statements (--py2 at 2^20), scaled to the batch (the rows are checked equal).
dev tool.  usage: python tools/circuit_assign_time.py [--leg all|default|2p20|chain|chacha|chacha_prove|chacha_out|sha256|sha256_prove|sha256_sum|sha256_sum_prove|merkle] [--nb 1020] [--reps 7] [--py 1020] [--py2 4]
[--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

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


def _time_calls(ctx, prog, bits, reps, kind):
    ctx.circuit_assign(prog, bits)  # first call: staging buffers
    call, kern, launches = [], [], 0
    ctx.set_timing(True)
    for _ in range(reps):
        t0 = time.perf_counter()
        witness, holds = ctx.circuit_assign(prog, bits)
        call.append((time.perf_counter() - t0) * 1e3)
        n, tot, _ = ctx.timing_drain(kind)
        kern.append(tot)
        launches = n
    ctx.set_timing(False)
    return witness, holds, call, kern, launches


def _depth(cc):
    lvl = np.zeros(cc.nwires + 1, dtype=np.int64)
    nin = cc.nwires - len(cc.gates)
    for g, (op, x, y) in enumerate(cc.gates.tolist()):
        lvl[nin + 1 + g] = 1 + max(lvl[x], lvl[y])
    return int(lvl.max())


def _depth_ex(cc):
    """levels of an extended program (Compiled.program): CONST gates are level 1, a gate 1 + the highest level of the operands it reads"""
    lvl = np.zeros(cc.nwires + 1, dtype=np.int64)
    nin = cc.nwires - len(cc.program)
    for g, (op, x, y, z) in enumerate(cc.program.tolist()):
        lvl[nin + 1 + g] = 1 if op in (circuit.GATE_CONST0, circuit.GATE_CONST1) else 1 + max(lvl[x], lvl[y], lvl[z] if z else 0)
    return int(lvl.max())


def _chacha_statements(st, rng, nb):
    from c_lwe_snarks_amd import words

    rows = []
    for _ in range(nb):
        key = bytes(rng.integers(0, 256, size=32, dtype=np.uint8).tolist())
        counter = int(rng.integers(0, 1 << 32, dtype=np.uint64))
        nonce = bytes(rng.integers(0, 256, size=12, dtype=np.uint8).tolist())
        # the public block from the circuit itself: evaluate with a zero block, read the computed words back
        bits = st.bits(key, counter, nonce, bytes(64))
        val = st.circuit.evaluate(bits[:640], bits[640:])
        block = b"".join(words.unpack(np.array([val[b.node] for b in w], dtype=np.uint8))[0].to_bytes(4, "little") for w in st.out)
        rows.append(st.bits(key, counter, nonce, block))
    return np.stack(rows)


def _emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def leg_default(a):
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
    witness, holds, call, kern, _ = _time_calls(ctx, prog, bits, a.reps, "circuit_assign")
    npy = min(a.py, a.nb)
    t0 = time.perf_counter()
    ref = [c.assign(bits[b, :npub].tolist(), bits[b, npub:].tolist()) for b in range(npy)]
    py_ms = (time.perf_counter() - t0) * 1e3 / npy
    same = all(witness[b].tobytes() == ref[b] for b in range(npy))
    res = {"tool": "circuit_assign_time", "d": p.d, "m": p.m, "nb": a.nb, "npub": npub, "npriv": npriv, "ngates": ngates, "depth": _depth(cc),
           "load_ms": round(load_ms, 3), "call_ms": round(statistics.median(call), 3), "call_ms_all": [round(x, 3) for x in call],
           "kernel_ms": round(statistics.median(kern), 3), "kernel_ms_all": [round(x, 3) for x in kern],
           "python_ms_per_statement": round(py_ms, 3), "python_statements_timed": npy, "python_ms_for_nb": round(py_ms * a.nb, 1),
           "python_over_call": round(py_ms * a.nb / statistics.median(call), 1), "rows_equal": bool(same), "holds_all": bool(holds.all())}
    _emit(res, a.out)
    prog.close()
    ctx.close()
    return same


def leg_2p20(a):
    p = mf.Params(d=1 << 20, m=699050)
    npub, npriv, ngates = 64, 20000, 470000
    rng = np.random.default_rng(2021)
    c = random_circuit(rng, npub, npriv, ngates)
    cc = c.compile(p)
    depth = _depth(cc)
    ctx = mf.Context(p, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prog = ctx.circuit_load(cc, state="global")
    load_ms = (time.perf_counter() - t0) * 1e3
    ok = True
    for nb in (255, 1020):
        bits = rng.integers(0, 2, size=(nb, npub + npriv), dtype=np.uint8)
        witness, holds, call, kern, launches = _time_calls(ctx, prog, bits, a.reps, "circuit_assign_global")
        npy = min(a.py2, nb)
        t0 = time.perf_counter()
        ref = [c.assign(bits[b, :npub].tolist(), bits[b, npub:].tolist()) for b in range(npy)]
        py_ms = (time.perf_counter() - t0) * 1e3 / npy
        same = all(witness[b].tobytes() == ref[b] for b in range(npy))
        ok = ok and same
        res = {"tool": "circuit_assign_time", "leg": "2p20", "state": prog.state, "d": p.d, "m": p.m, "nb": nb, "npub": npub, "npriv": npriv,
               "ngates": ngates, "depth": depth, "load_ms": round(load_ms, 3), "launches_per_call": launches,
               "call_ms": round(statistics.median(call), 3), "call_ms_all": [round(x, 3) for x in call],
               "kernel_ms": round(statistics.median(kern), 3), "kernel_ms_all": [round(x, 3) for x in kern],
               "python_ms_per_statement": round(py_ms, 3), "python_statements_timed": npy, "python_ms_for_nb": round(py_ms * nb, 1),
               "python_over_call": round(py_ms * nb / statistics.median(call), 1), "rows_equal": bool(same)}
        _emit(res, a.out)
    prog.close()
    ctx.close()
    return ok


def leg_chain(a):
    nin, ngates, nb = 40000, 60000, 100
    p = mf.Params(d=256, m=nin + ngates + 1)
    k = np.arange(ngates, dtype=np.int64)
    prev = np.where(k == 0, 1, nin + k)
    nots = k % 5 == 4
    gates = np.stack([np.where(nots, 3, 0), prev, np.where(nots, prev, 1 + (k + 1) % nin)], axis=1).astype(np.uint32)
    desc = SimpleNamespace(gates=gates, asserts=np.array([[nin + ngates, 1]], dtype=np.uint32), nwires=nin + ngates)
    bits = np.random.default_rng(60).integers(0, 2, size=(nb, nin), dtype=np.uint8)
    ctx = mf.Context(p, 0)
    t0 = time.perf_counter()
    prog = ctx.circuit_load(desc, state="global")
    load_ms = (time.perf_counter() - t0) * 1e3
    witness, holds, call, kern, launches = _time_calls(ctx, prog, bits, a.reps, "circuit_assign_global")
    xs = np.where(nots[None, :], 0, bits[:, (k + 1) % nin])
    last = bits[:, 0] ^ np.bitwise_xor.reduce(xs, axis=1) ^ (int(nots.sum()) & 1)
    same = bool(np.array_equal(holds, last == 1))
    res = {"tool": "circuit_assign_time", "leg": "chain", "state": prog.state, "d": p.d, "m": p.m, "nb": nb, "nin": nin, "ngates": ngates,
           "depth": ngates, "load_ms": round(load_ms, 3), "launches_per_call": launches, "call_ms": round(statistics.median(call), 3),
           "call_ms_all": [round(x, 3) for x in call], "kernel_ms": round(statistics.median(kern), 3), "kernel_ms_all": [round(x, 3) for x in kern],
           "kernel_us_per_level": round(statistics.median(kern) * 1e3 / ngates, 3), "last_gate_equal": same}
    _emit(res, a.out)
    prog.close()
    ctx.close()
    return same


def leg_chacha(a):
    from c_lwe_snarks_amd import words

    p = mf.Params(d=1 << 16, m=43690)
    st = words.ChaCha20Block()
    cc = st.circuit.compile(p)
    depth = _depth_ex(cc)
    rng = np.random.default_rng(8439)
    bits = _chacha_statements(st, rng, a.nb)
    ctx = mf.Context(p, 0)
    ok = True
    outs = {}
    for state, kind in (("lds", "circuit_assign_ex"), ("global", "circuit_assign_global_ex")):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prog = ctx.circuit_load(cc, state=state)
        load_ms = (time.perf_counter() - t0) * 1e3
        witness, holds, call, kern, launches = _time_calls(ctx, prog, bits, a.reps, kind)
        outs[state] = witness
        npy = min(a.py2, a.nb)
        t0 = time.perf_counter()
        ref = [st.circuit.assign(bits[b, :640], bits[b, 640:], p) for b in range(npy)]
        py_ms = (time.perf_counter() - t0) * 1e3 / npy
        same = all(witness[b].tobytes() == ref[b] for b in range(npy)) and bool(holds.all())
        ok = ok and same
        res = {"tool": "circuit_assign_time", "leg": "chacha", "state": state, "d": p.d, "m": p.m, "nb": a.nb, "npub": cc.lu, "npriv": 256,
               "ngates": len(cc.program), "nequal": len(cc.equal), "depth": depth, "load_ms": round(load_ms, 3), "launches_per_call": launches,
               "call_ms": round(statistics.median(call), 3), "call_ms_all": [round(x, 3) for x in call],
               "kernel_ms": round(statistics.median(kern), 3), "kernel_ms_all": [round(x, 3) for x in kern],
               "kernel_us_per_level": round(statistics.median(kern) * 1e3 / depth, 3),
               "python_ms_per_statement": round(py_ms, 3), "python_statements_timed": npy, "python_ms_for_nb": round(py_ms * a.nb, 1),
               "python_over_call": round(py_ms * a.nb / statistics.median(call), 1), "rows_equal": bool(same)}
        _emit(res, a.out)
        prog.close()
    ok = ok and bool(np.array_equal(outs["lds"], outs["global"]))
    ctx.close()
    return ok


def leg_chacha_prove(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    from c_lwe_snarks_amd import words

    p = mf.Params(d=1 << 16, m=43690)
    st = words.ChaCha20Block()
    cc = st.circuit.compile(p)
    nb = 255
    rng = np.random.default_rng(8440)
    bits = _chacha_statements(st, rng, nb)
    ctx = mf.Context(p, 0)
    prog = ctx.circuit_load(cc)
    witness, holds = ctx.circuit_assign(prog, bits)
    prog.close()
    ctx.set_seed(bytes(range(40)))
    ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)
    ctx.ssp_prepare(None)
    alpha, beta, s = (int(x) for x in rng.integers(1, circuit.P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    d_crs = ctx.setup_public(None, alpha, beta, s, cc.lu, d_sk, d_err).clone()
    stmts = [witness[b].tobytes() for b in range(nb)]
    deltas = [int(x) for x in rng.integers(0, circuit.P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    times = []
    for _ in range(a.reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        proofs = ctx.prove_batch_public(d_crs, None, cc.lu, stmts, deltas, mags, signs)
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    vk = ctx.derive_vk(None, s, cc.lu)
    ok = bool(ctx.to_host(ctx.verify_public(vk, cc.lu, alpha, beta, d_sk, proofs, stmts), np.uint8).all())
    res = {"tool": "circuit_assign_time", "leg": "chacha_prove", "d": p.d, "m": p.m, "nb": nb, "lu": cc.lu, "nrows": cc.nrows,
           "prove_batch_public_ms": round(statistics.median(times[1:]), 3), "prove_ms_all": [round(x, 3) for x in times],
           "holds_all": bool(holds.all()), "verified_all": ok}
    _emit(res, a.out)
    ctx.close()
    return ok and bool(holds.all())


def leg_chacha_out(a):
    from c_lwe_snarks_amd import words

    p = mf.Params(d=1 << 16, m=43690)
    st = words.ChaCha20Block()
    cc = st.circuit.compile(p)
    # the same statement with the block computed: counter and nonce public, the 16 block words outputs (the same wires 1 .. 640), the key private
    w = words.Words()
    counter, nonce = w.public(), w.public(3)
    key = w.private(8)
    block = [w.output(x) for x in words.chacha20_block(w, key, counter, nonce)]
    # (outputs are declared after the private key here, but the layout puts every public wire first: wires 129 .. 640, as in ChaCha20Block)
    co = w.c.compile(p)
    assert co.lu == cc.lu == 640 and co.nwires == cc.nwires and co.nrows == cc.nrows and np.array_equal(co.program, cc.program)
    assert len(co.outputs) == 512 and co.wire(block[0][0]) == 129
    rng = np.random.default_rng(8439)
    bits = _chacha_statements(st, rng, a.nb)
    ok = _alternate(a, p, "chacha20 block", cc, co, bits)
    # a second pair with three times the depth and a sixteenth of the outputs: 200 adds x += rotl(x, 1), each waiting for the top bit of the one
    # before, the result tied to a public word by equalities or declared an output.  A cost of the pass itself would follow nout; a difference in the level loop follows the depth.
    p2 = mf.DEFAULT
    pair = []
    for out in (False, True):
        w = words.Words()
        r = None if out else w.public()
        acc = w.private()
        for _ in range(200):
            acc = w.add(acc, w.rotl(acc, 1))
        if out:
            w.output(acc)
        else:
            w.assert_same_u32(acc, r)
        pair.append(w.c.compile(p2))
    assert np.array_equal(pair[0].program, pair[1].program) and len(pair[1].outputs) == 32
    xv = rng.integers(0, 1 << 32, size=a.nb, dtype=np.uint64)
    rv = xv.copy()
    for _ in range(200):
        rv = (rv + ((rv << np.uint64(1)) | (rv >> np.uint64(31)))) & np.uint64(0xFFFFFFFF)
    bits2 = np.concatenate([words.pack(rv[:, None]), words.pack(xv[:, None])], axis=1)
    return _alternate(a, p2, "200 adds x += rotl(x, 1)", pair[0], pair[1], bits2) and ok


def _alternate(a, p, what, cc, co, bits):
    """the LDS programs of cc (no outputs, k_circuit_eval<true>) and co (the same gates with outputs, k_circuit_eval<true, true>) called in turn"""
    ctx = mf.Context(p, 0)
    progs = {"circuit_assign_ex": ctx.circuit_load(cc, state="lds"), "circuit_assign_out": ctx.circuit_load(co, state="lds")}
    for prog in progs.values():
        ctx.circuit_assign(prog, bits)  # first calls: staging buffers
    kern = {k: [] for k in progs}
    outs = {}
    ctx.set_timing(True)
    for _ in range(a.reps):
        for kind, prog in progs.items():
            outs[kind], holds = ctx.circuit_assign(prog, bits)
            kern[kind].append(ctx.timing_drain(kind)[1])
    ctx.set_timing(False)
    same = bool(np.array_equal(outs["circuit_assign_ex"], outs["circuit_assign_out"]))
    med = {k: statistics.median(v) for k, v in kern.items()}
    depth = _depth_ex(cc)
    res = {"tool": "circuit_assign_time", "leg": "chacha_out", "circuit": what, "d": p.d, "m": p.m, "nb": len(bits), "nout": len(co.outputs),
           "depth": depth, "reps": a.reps,
           "kernel_ms_ex": round(med["circuit_assign_ex"], 4), "kernel_ms_ex_all": [round(x, 4) for x in kern["circuit_assign_ex"]],
           "kernel_ms_out": round(med["circuit_assign_out"], 4), "kernel_ms_out_all": [round(x, 4) for x in kern["circuit_assign_out"]],
           "out_minus_ex_us": round((med["circuit_assign_out"] - med["circuit_assign_ex"]) * 1e3, 2),
           "out_minus_ex_ns_per_level": round((med["circuit_assign_out"] - med["circuit_assign_ex"]) * 1e6 / depth, 2),
           "spread_ex_us": round((max(kern["circuit_assign_ex"]) - min(kern["circuit_assign_ex"])) * 1e3, 2), "rows_equal": same}
    _emit(res, a.out)
    for prog in progs.values():
        prog.close()
    ctx.close()
    return same


def _sha256_statements(st, rng, nb):
    from c_lwe_snarks_amd import words

    msgs = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 56)), dtype=np.uint8).tolist()) for _ in range(nb)]
    return msgs, np.stack([st.bits(words.sha256_pad(m)) for m in msgs])


def leg_sha256(a):
    import hashlib

    from c_lwe_snarks_amd import words

    p = mf.Params(d=1 << 17, m=87381)
    st = words.Sha256Compress("iv")
    t0 = time.perf_counter()
    cc = st.circuit.compile(p)
    compile_ms = (time.perf_counter() - t0) * 1e3
    depth = _depth_ex(cc)
    ctx = mf.Context(p, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prog = ctx.circuit_load(cc, state="auto")
    load_ms = (time.perf_counter() - t0) * 1e3
    ok = prog.state == "global"
    rng = np.random.default_rng(1802)
    for nb in (255, 1020):
        msgs, bits = _sha256_statements(st, rng, nb)
        witness, holds, call, kern, launches = _time_calls(ctx, prog, bits, a.reps, "circuit_assign_global_out")
        digests = all(st.digest_of(witness[b]) == hashlib.sha256(msgs[b]).digest() for b in range(nb))
        npy = min(a.py2, nb)
        t0 = time.perf_counter()
        ref = [st.circuit.assign(bits[b, :256], bits[b, 256:], p) for b in range(npy)]
        py_ms = (time.perf_counter() - t0) * 1e3 / npy
        same = all(witness[b].tobytes() == ref[b] for b in range(npy)) and bool(holds.all()) and digests
        ok = ok and same
        res = {"tool": "circuit_assign_time", "leg": "sha256", "state": prog.state, "d": p.d, "m": p.m, "nb": nb, "npub": cc.lu, "npriv": 512,
               "ngates": len(cc.program), "nout": len(cc.outputs), "depth": depth, "compile_ms": round(compile_ms, 1), "load_ms": round(load_ms, 3),
               "launches_per_call": launches, "call_ms": round(statistics.median(call), 3), "call_ms_all": [round(x, 3) for x in call],
               "kernel_ms": round(statistics.median(kern), 3), "kernel_ms_all": [round(x, 3) for x in kern],
               "kernel_us_per_level": round(statistics.median(kern) * 1e3 / depth / max(launches, 1), 3),
               "python_ms_per_statement": round(py_ms, 3), "python_statements_timed": npy, "python_ms_for_nb": round(py_ms * nb, 1),
               "python_over_call": round(py_ms * nb / statistics.median(call), 1), "rows_equal": bool(same), "digests_equal_hashlib": bool(digests)}
        _emit(res, a.out)
    prog.close()
    ctx.close()
    return ok


def leg_sha256_prove(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    from c_lwe_snarks_amd import words

    p = mf.Params(d=1 << 17, m=87381)
    st = words.Sha256Compress("iv")
    cc = st.circuit.compile(p)
    nb = 255
    rng = np.random.default_rng(1803)
    _, bits = _sha256_statements(st, rng, nb)
    ctx = mf.Context(p, 0)
    prog = ctx.circuit_load(cc, state="auto")
    witness, holds = ctx.circuit_assign(prog, bits)
    prog.close()
    ctx.set_seed(bytes(range(40)))
    t0 = time.perf_counter()
    ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)
    ctx.ssp_prepare(None)
    ctx.sync()
    rows_ms = (time.perf_counter() - t0) * 1e3
    alpha, beta, s = (int(x) for x in rng.integers(1, circuit.P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    t0 = time.perf_counter()
    d_crs = ctx.setup_public(None, alpha, beta, s, cc.lu, d_sk, d_err).clone()
    ctx.sync()
    setup_ms = (time.perf_counter() - t0) * 1e3
    stmts = [witness[b].tobytes() for b in range(nb)]
    deltas = [int(x) for x in rng.integers(0, circuit.P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    times = []
    for _ in range(a.reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        proofs = ctx.prove_batch_public(d_crs, None, cc.lu, stmts, deltas, mags, signs)
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    vk = ctx.derive_vk(None, s, cc.lu)
    ok = bool(ctx.to_host(ctx.verify_public(vk, cc.lu, alpha, beta, d_sk, proofs, stmts), np.uint8).all())
    res = {"tool": "circuit_assign_time", "leg": "sha256_prove", "d": p.d, "m": p.m, "nb": nb, "lu": cc.lu, "nrows": cc.nrows,
           "ssp_set_rows_prepare_ms": round(rows_ms, 1), "setup_public_ms": round(setup_ms, 1),
           "prove_batch_public_ms": round(statistics.median(times[1:]), 3), "prove_ms_all": [round(x, 3) for x in times],
           "holds_all": bool(holds.all()), "verified_all": ok}
    _emit(res, a.out)
    ctx.close()
    return ok and bool(holds.all())


def _sha256_variants():
    """(name, Params, statement, compiled, timing kind) of the ripple-carry statement at d = 2^17 and of the statement with sums at d = 2^16"""
    from c_lwe_snarks_amd import words

    out = []
    for name, p, adds, kind in (("ripple", mf.Params(d=1 << 17, m=87381), "ripple", "circuit_assign_global_out"),
                                ("sum", mf.Params(d=1 << 16, m=43690), "sum", "circuit_assign_sum")):
        st = words.Sha256Compress("iv", adds=adds)
        out.append(SimpleNamespace(name=name, p=p, st=st, cc=st.circuit.compile(p), kind=kind))
    return out


def _depth_sum(cc):
    """levels of a program with WSUM gates: a head and its bit records 1 + the highest level of its terms"""
    lvl = np.zeros(cc.nwires + 1, dtype=np.int64)
    nin = cc.nwires - len(cc.program)
    head = 0
    for g, (op, x, y, z) in enumerate(cc.program.tolist()):
        o = nin + 1 + g
        if op == circuit.GATE_WSUM:
            head = o
            lvl[o] = 1 + int(lvl[cc.terms[x: x + y, 0]].max())
        elif op == circuit.GATE_WSUM_BIT:
            lvl[o] = lvl[head]
        else:
            lvl[o] = 1 if op in (circuit.GATE_CONST0, circuit.GATE_CONST1) else 1 + max(lvl[x], lvl[y], lvl[z] if z else 0)
    return int(lvl.max())


def leg_sha256_sum(a):
    import hashlib

    vs = _sha256_variants()
    ok = True
    for v in vs:
        v.ctx = mf.Context(v.p, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v.prog = v.ctx.circuit_load(v.cc, state="auto")
        v.load_ms = (time.perf_counter() - t0) * 1e3
        v.depth = _depth_sum(v.cc)
    ok = ok and vs[0].prog.state == "global" and vs[1].prog.state == "lds" and vs[1].prog.sums
    rng = np.random.default_rng(1806)
    for nb in (255, 1020):
        msgs, bits = _sha256_statements(vs[0].st, rng, nb)
        for v in vs:
            v.ctx.circuit_assign(v.prog, bits)  # first call: staging buffers
            v.call, v.kern = [], []
        for _ in range(a.reps):  # in turn
            for v in vs:
                v.ctx.set_timing(True)
                t0 = time.perf_counter()
                v.witness, v.holds = v.ctx.circuit_assign(v.prog, bits)
                v.call.append((time.perf_counter() - t0) * 1e3)
                v.launches, tot, _ = v.ctx.timing_drain(v.kind)
                v.kern.append(tot)
                v.ctx.set_timing(False)
        for v in vs:
            digests = all(v.st.digest_of(v.witness[b]) == hashlib.sha256(msgs[b]).digest() for b in range(nb))
            same = all(v.witness[b].tobytes() == v.st.circuit.assign(bits[b, :256], bits[b, 256:], v.p) for b in range(min(a.py2, nb)))
            ok = ok and digests and same and bool(v.holds.all())
            heads = int((v.cc.program[:, 0] == circuit.GATE_WSUM).sum())
            _emit({"tool": "circuit_assign_time", "leg": "sha256_sum", "adds": v.name, "state": v.prog.state, "d": v.p.d, "m": v.p.m, "nb": nb,
                   "nwires": v.cc.nwires, "nrows": v.cc.nrows, "heads": heads, "terms": len(v.cc.terms), "depth": v.depth,
                   "load_ms": round(v.load_ms, 3), "launches_per_call": v.launches, "call_ms": round(statistics.median(v.call), 3),
                   "call_ms_all": [round(x, 3) for x in v.call], "kernel_ms": round(statistics.median(v.kern), 3),
                   "kernel_ms_all": [round(x, 3) for x in v.kern],
                   "kernel_us_per_level": round(statistics.median(v.kern) * 1e3 / v.depth / max(v.launches, 1), 3),
                   "rows_equal": bool(same), "digests_equal_hashlib": bool(digests)}, a.out)
    for v in vs:
        v.prog.close()
        v.ctx.close()
    return ok


def leg_sha256_sum_prove(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol

    vs = _sha256_variants()
    nb, reps = 255, min(a.reps, 5)
    rng = np.random.default_rng(1807)
    _, bits = _sha256_statements(vs[0].st, rng, nb)
    deltas = [int(x) for x in rng.integers(0, circuit.P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    for v in vs:
        p, cc = v.p, v.cc
        v.ctx = ctx = mf.Context(p, 0)
        v.prog = ctx.circuit_load(cc, state="auto")
        ctx.circuit_assign(v.prog, bits)
        ctx.set_seed(bytes(range(40)))
        ctx.sync()
        t0 = time.perf_counter()
        ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)
        ctx.ssp_prepare(None)
        ctx.sync()
        v.rows_ms = (time.perf_counter() - t0) * 1e3
        v.alpha, v.beta, v.s = (int(x) for x in rng.integers(1, circuit.P, size=3, dtype=np.uint64))
        v.d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
        d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
        t0 = time.perf_counter()
        v.d_crs = ctx.setup_public(None, v.alpha, v.beta, v.s, cc.lu, v.d_sk, d_err).clone()
        ctx.sync()
        v.setup_ms = (time.perf_counter() - t0) * 1e3
        v.assign, v.wpoly, v.prove = [], [], []
    for r in range(reps + 1):  # in turn; the first round warms up
        for v in vs:
            ctx = v.ctx
            ctx.sync()
            t0 = time.perf_counter()
            v.witness, v.holds = ctx.circuit_assign(v.prog, bits)
            t1 = time.perf_counter()
            v.stmts = [v.witness[b].tobytes() for b in range(nb)]
            ctx.sync()
            t2 = time.perf_counter()
            ctx.witness_poly(None, v.stmts[0], deltas[0])
            ctx.sync()
            t3 = time.perf_counter()
            v.proofs = ctx.prove_batch_public(v.d_crs, None, v.cc.lu, v.stmts, deltas, mags, signs)
            ctx.sync()
            t4 = time.perf_counter()
            if r:
                v.assign.append((t1 - t0) * 1e3)
                v.wpoly.append((t3 - t2) * 1e3)
                v.prove.append((t4 - t3) * 1e3)
    ok = True
    for v in vs:
        vk = v.ctx.derive_vk(None, v.s, v.cc.lu)
        good = bool(v.ctx.to_host(v.ctx.verify_public(vk, v.cc.lu, v.alpha, v.beta, v.d_sk, v.proofs, v.stmts), np.uint8).all()) and bool(v.holds.all())
        ok = ok and good
        lens = np.diff(v.cc.rows[0].astype(np.int64))
        _emit({"tool": "circuit_assign_time", "leg": "sha256_sum_prove", "adds": v.name, "d": v.p.d, "m": v.p.m, "nb": nb, "lu": v.cc.lu,
               "nwires": v.cc.nwires, "nrows": v.cc.nrows, "row_entries": int(lens.sum()), "longest_row": int(lens.max()),
               "ssp_set_rows_prepare_ms": round(v.rows_ms, 1), "setup_public_ms": round(v.setup_ms, 1),
               "witness_poly_ms": round(statistics.median(v.wpoly), 3), "circuit_assign_call_ms": round(statistics.median(v.assign), 3),
               "prove_batch_public_ms": round(statistics.median(v.prove), 3), "prove_ms_all": [round(x, 3) for x in v.prove],
               "witness_plus_prove_ms": round(statistics.median(v.assign) + statistics.median(v.prove), 3), "verified_all": good}, a.out)
    for v in vs:
        v.prog.close()
        v.ctx.close()
    return ok and statistics.median(vs[1].assign) + statistics.median(vs[1].prove) < statistics.median(vs[0].assign) + statistics.median(vs[0].prove)

def _whole_statement(a, name, p, build, make_bits, result_of, expected):
    """every step of one statement class at p for 255 statements, one JSON record; True when the results are right, no row is violated and every proof verifies"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol

    nb = 255
    rng = np.random.default_rng(2025)
    t0 = time.perf_counter()
    st = build()
    build_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cc = st.circuit.compile(p)
    compile_ms = (time.perf_counter() - t0) * 1e3
    cases = [make_bits(st, rng) for _ in range(nb)]
    bits = np.stack([b for b, _ in cases])
    ctx = mf.Context(p, 0)
    ctx.set_seed(bytes(range(40)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prog = ctx.circuit_load(cc, state="auto")
    load_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    witness, holds = ctx.circuit_assign(prog, bits)
    assign_first_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    witness, holds = ctx.circuit_assign(prog, bits)
    assign_ms = (time.perf_counter() - t0) * 1e3
    state = prog.state
    prog.close()
    right = all(result_of(st, witness[b]) == expected(key) for b, (_, key) in enumerate(cases)) and bool(holds.all())
    t0 = time.perf_counter()
    ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)
    ctx.ssp_prepare(None)
    ctx.sync()
    rows_ms = (time.perf_counter() - t0) * 1e3
    stmts = [witness[b].tobytes() for b in range(nb)]
    deltas = [int(x) for x in rng.integers(0, circuit.P, size=nb, dtype=np.uint64)]
    # the row check against the witness pass of the row SSP: the same statements, calls alternated, the first round warms up
    check, wpoly, kern = [], [], []
    ctx.set_timing(True)
    for r in range(6):
        ctx.sync()
        t0 = time.perf_counter()
        count, first = ctx.ssp_rows_violations(witness)
        t1 = time.perf_counter()
        kern_ms = ctx.timing_drain("ssp_rows_violations")[1]
        ctx.sync()
        t2 = time.perf_counter()
        w = ctx.witness_poly_many(None, stmts, deltas)
        ctx.sync()
        t3 = time.perf_counter()
        del w
        if r:
            check.append((t1 - t0) * 1e3)
            kern.append(kern_ms)
            wpoly.append((t3 - t2) * 1e3)
    ctx.set_timing(False)
    clean = not count.any()
    alpha, beta, s = (int(x) for x in rng.integers(1, circuit.P, size=3, dtype=np.uint64))
    d_sk = ctx.to_device(ol.rand_values(rng, p.n, p.L, p.logq))
    d_err = ctx.to_device(ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    ctx.sync()
    t0 = time.perf_counter()
    d_crs = ctx.setup_public(None, alpha, beta, s, cc.lu, d_sk, d_err).clone()
    ctx.sync()
    setup_ms = (time.perf_counter() - t0) * 1e3
    del d_err
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    prove = []
    for _ in range(2):
        ctx.sync()
        t0 = time.perf_counter()
        proofs = ctx.prove_batch_public(d_crs, None, cc.lu, stmts, deltas, mags, signs)
        ctx.sync()
        prove.append((time.perf_counter() - t0) * 1e3)
    vk = ctx.derive_vk(None, s, cc.lu)
    ctx.sync()
    t0 = time.perf_counter()
    ok = ctx.to_host(ctx.verify_public(vk, cc.lu, alpha, beta, d_sk, proofs, stmts), np.uint8)
    verify_ms = (time.perf_counter() - t0) * 1e3
    verified = bool(ok.all())
    lens = np.diff(cc.rows[0].astype(np.int64))
    _emit({"tool": "circuit_assign_time", "leg": "merkle", "statement": name, "d": p.d, "m": p.m, "nb": nb, "lu": cc.lu, "state": state,
           "nwires": cc.nwires, "nrows": cc.nrows, "row_entries": int(lens.sum()), "longest_row": int(lens.max()),
           "build_ms": round(build_ms, 1), "compile_ms": round(compile_ms, 1), "circuit_load_ms": round(load_ms, 1),
           "circuit_assign_first_ms": round(assign_first_ms, 2), "circuit_assign_ms": round(assign_ms, 2),
           "ssp_set_rows_prepare_ms": round(rows_ms, 1),
           "rows_violations_ms": round(statistics.median(check), 3), "rows_violations_ms_all": [round(x, 3) for x in check],
           "rows_violations_kernel_ms": round(statistics.median(kern), 3),
           "witness_poly_many_ms": round(statistics.median(wpoly), 3), "witness_poly_many_ms_all": [round(x, 3) for x in wpoly],
           "setup_public_ms": round(setup_ms, 1), "prove_batch_public_ms_all": [round(x, 2) for x in prove], "verify_public_ms": round(verify_ms, 2),
           "results_right": bool(right), "violations": int(count.sum()), "verified_all": verified}, a.out)
    ctx.close()
    return right and clean and verified


def leg_merkle(a):
    import hashlib

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sha256_ref
    from c_lwe_snarks_amd import words

    def message_bits(st, rng):
        m = rng.bytes(100)
        return st.bits(m), m

    def path_bits(st, rng):
        leaf, sibs, index = rng.bytes(32), [rng.bytes(32) for _ in range(st.depth)], int(rng.integers(0, 1 << st.depth))
        return st.bits(leaf, sibs, index), (leaf, sibs, index)

    ok = _whole_statement(a, "Sha256Message(100)", mf.Params(d=1 << 17, m=87381), lambda: words.Sha256Message(100), message_bits,
                          lambda st, row: st.digest_of(row), lambda m: hashlib.sha256(m).digest())
    return _whole_statement(a, "MerklePath(20)", mf.Params(d=1 << 20, m=699050), lambda: words.MerklePath(20), path_bits,
                            lambda st, row: st.root_of(row), lambda k: sha256_ref.merkle_root(*k)) and ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="all", choices=["all", "default", "2p20", "chain", "chacha", "chacha_prove", "chacha_out", "sha256", "sha256_prove", "sha256_sum",
                                                      "sha256_sum_prove", "merkle"])
    ap.add_argument("--nb", type=int, default=1020)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--py", type=int, default=1020, help="statements timed through Circuit.assign (default leg)")
    ap.add_argument("--py2", type=int, default=4, help="statements timed through Circuit.assign (2p20, chacha and sha256 legs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ok = True
    for name, fn in (("default", leg_default), ("chain", leg_chain), ("2p20", leg_2p20), ("chacha", leg_chacha), ("chacha_prove", leg_chacha_prove),
                     ("chacha_out", leg_chacha_out), ("sha256", leg_sha256), ("sha256_prove", leg_sha256_prove), ("sha256_sum", leg_sha256_sum),
                     ("sha256_sum_prove", leg_sha256_sum_prove), ("merkle", leg_merkle)):
        if a.leg in ("all", name):
            ok = fn(a) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
