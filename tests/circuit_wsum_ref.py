"""Helpers of the weighted-sum gate tests: random circuits that mix wsum gates with every other gate kind, and a numpy restatement of the evaluation
of mfh_circuit_create_sum programs (Compiled.program / terms / asserts / equal / outputs alone), 32 statements per word."""
import numpy as np

from c_lwe_snarks_amd import circuit as C

from circuit_ex_ref import gate_word

M32 = 0xFFFFFFFF
P = C.P


def random_sum_circuit(rng, npub, npriv, ngates, nsums, nasserts=0, nequal=0, noutputs=0, max_terms=40):
    """inputs, then about ngates gate wires: random gates of every kind on earlier wires with nsums wsum gates spread among them (1 .. max_terms terms,
    repeated wires, shifts 0 .. 12, now and then all on one shift), then assertions, equalities and computed outputs on random wires"""
    c = C.Circuit()
    ws = c.public(npub) + c.private(npriv)
    kinds = ("XOR", "AND", "OR", "NOT", "MAJ", "FA", "LUT", "CONST", "NAND", "ANDN")
    total = npub + npriv + ngates
    sum_at = set(rng.choice(np.arange(npub + npriv + 1, total), size=nsums, replace=False).tolist())
    while len(ws) < total:
        if sum_at and len(ws) >= min(sum_at):
            sum_at.discard(min(sum_at))
            n = int(rng.integers(1, max_terms + 1))
            top = int(rng.integers(0, 13))
            shifts = rng.integers(0, top + 1, size=n) if rng.integers(0, 4) else np.full(n, top)
            ws += c.wsum([(ws[int(rng.integers(0, len(ws)))], int(s)) for s in shifts])
            continue
        kind = kinds[int(rng.integers(0, len(kinds)))]
        a, b, d = (ws[int(rng.integers(0, len(ws)))] for _ in range(3))
        if kind == "NOT":
            ws.append(c.NOT(a))
        elif kind == "MAJ":
            ws.append(c.MAJ(a, b, d))
        elif kind == "FA":
            s, k = c.full_add(a, b, d)
            ws += [k, s]
        elif kind == "LUT":
            ws.append(c.gate(int(rng.integers(0, 16)), a, b))
        elif kind == "CONST":
            ws.append(c.const(int(rng.integers(0, 2))))
        else:
            ws.append(getattr(c, kind)(a, b))
    for _ in range(nasserts):
        c.assert_equal(ws[int(rng.integers(0, len(ws)))], int(rng.integers(0, 2)))
    for _ in range(nequal):
        a, b = rng.choice(len(ws), size=2, replace=False)
        c.assert_same(ws[int(a)], ws[int(b)])
    for _ in range(noutputs):
        c.output(ws[int(rng.integers(0, len(ws)))])
    return c


def bitsliced_sum(cc, bits, m):
    """witness bytes [nb, (m + 7) // 8] and holds [nb] of a program with WSUM gates and computed outputs: a head's output word i is bit i of the 32
    per-statement sums, a WSUM_BIT record writes nothing; an output wire p takes wire w's word after the last gate, and the pairs' own equalities hold"""
    nb, nin = bits.shape
    program, terms = cc.program.tolist(), np.asarray(cc.terms, dtype=np.int64).reshape(-1, 2)
    nw = nin + len(program)
    pairs = {(int(p), int(w)) for p, w in cc.outputs}
    out_bits = np.zeros((nb, nw), dtype=np.uint8)
    holds = np.zeros(nb, dtype=bool)
    lanes = np.arange(32, dtype=np.uint32)
    for s0 in range(0, nb, 32):
        blk = bits[s0: s0 + 32] & 1
        n = len(blk)
        weights = (np.uint32(1) << np.arange(n, dtype=np.uint32))[:, None]
        st = np.zeros(nw + 1, dtype=np.uint32)
        st[1: nin + 1] = (blk.astype(np.uint32) * weights).sum(axis=0, dtype=np.uint32)
        for g, (op, a, b, c) in enumerate(program):
            o = nin + 1 + g
            if op == C.GATE_WSUM_BIT:
                continue
            if op == C.GATE_WSUM:
                t = terms[a: a + b]
                sums = (((st[t[:, 0]][:, None] >> lanes[None, :]) & 1).astype(np.uint64) << t[:, 1].astype(np.uint64)[:, None]).sum(axis=0)  # [32]
                for i in range(c):
                    st[o + i] = np.uint32((((sums >> np.uint64(i)) & np.uint64(1)) << lanes.astype(np.uint64)).sum())
                continue
            st[o] = gate_word(op, st[a], st[b], st[c])
        for p, w in cc.outputs.tolist():
            st[p] = st[w]
        ok = np.uint32(M32)
        for w, v in cc.asserts:
            ok &= st[w] if v else ~st[w]
        for a, b in cc.equal.tolist():
            if (a, b) not in pairs:
                ok &= ~(st[a] ^ st[b])
        holds[s0: s0 + n] = [(int(ok) >> j) & 1 for j in range(n)]
        out_bits[s0: s0 + n] = ((st[1:][None, :] >> np.arange(n, dtype=np.uint32)[:, None]) & 1).astype(np.uint8)
    packed = np.packbits(out_bits, axis=1, bitorder="little")
    wit = np.zeros((nb, (m + 7) // 8), dtype=np.uint8)
    wit[:, : packed.shape[1]] = packed
    return wit, holds


def row_values_int(rows, bits: bytes):
    """every row's value on a witness, mod p, in Python integers (vectorised over the entries): bit i - 1 of bits = wire i, wire 0 = 1"""
    row_ptr, wire, coef = (np.asarray(a, dtype=np.int64) for a in rows)
    bit = np.concatenate([[1], np.unpackbits(np.frombuffer(bits, dtype=np.uint8), bitorder="little")]).astype(np.int64)
    contrib = coef * bit[wire]  # < 2^32 each
    acc = np.concatenate([[0], np.cumsum(contrib)])  # < 2^63 for fewer than 2^31 entries
    return [int(acc[row_ptr[j + 1]] - acc[row_ptr[j]]) % P for j in range(len(row_ptr) - 1)]
