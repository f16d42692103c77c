"""numpy restatement of mfh_circuit_assign vectorised by level: fast enough to check 470 000 gates x 1 020 statements.

The program (Compiled.gates / .asserts, or any object with gates, asserts and nwires) is levelled as mfh_circuit_create does it (inputs level 0, a gate
one more than its highest operand).  The wire state is one row of uint64 words per wire, bit j of word k = statement 64 k + j, and every level is one
gather, one op and one scatter over all its gates and all statements at once."""
import numpy as np

XOR, AND, OR, NOT = 0, 1, 2, 3


def gate_levels(nin, gates):
    """level of every gate (1-based): 1 + the highest level of its operands, inputs 0"""
    ops, a, b = (np.asarray(gates, dtype=np.int64).reshape(-1, 3)[:, k].tolist() for k in range(3))
    lw = [0] * (nin + len(ops) + 1)
    out = [0] * len(ops)
    for g in range(len(ops)):
        la = lw[a[g]]
        lb = la if ops[g] == NOT else lw[b[g]]
        lw[nin + 1 + g] = out[g] = 1 + (la if la > lb else lb)
    return np.asarray(out, dtype=np.int64)


def wire_words(desc, bits):
    """the wire state after the last level: uint64 [nw + 1, ceil(nb / 64)] (row 0 unused)"""
    bits = np.asarray(bits, dtype=np.uint8) & 1
    nb, nin = bits.shape
    gates = np.asarray(desc.gates, dtype=np.int64).reshape(-1, 3)
    nw = nin + len(gates)
    assert nw == desc.nwires
    nwd = max(1, (nb + 63) // 64)
    st = np.zeros((nw + 1, nwd), dtype=np.uint64)
    if nin and nb:
        t = np.zeros((nin, nwd * 64), dtype=np.uint8)
        t[:, :nb] = bits.T
        st[1: nin + 1] = np.packbits(t, axis=1, bitorder="little").view("<u8")
    if len(gates):
        lvl = gate_levels(nin, gates)
        order = np.argsort(lvl, kind="stable")
        op, a, b = gates[order, 0], gates[order, 1], gates[order, 2]
        out = nin + 1 + order
        ends = np.searchsorted(lvl[order], np.arange(1, int(lvl.max()) + 1), side="right")
        g0 = 0
        for g1 in ends.tolist():
            o, x, y = op[g0:g1], st[a[g0:g1]], st[b[g0:g1]]
            res = np.where((o == XOR)[:, None], x ^ y, np.where((o == AND)[:, None], x & y, np.where((o == OR)[:, None], x | y, ~x)))
            st[out[g0:g1]] = res
            g0 = g1
    return st


def evaluate(desc, bits, m):
    """(witness uint8 [nb, (m + 7) // 8], holds bool [nb]): the rows and flags of mfh_circuit_assign with bits_stride = (m + 7) // 8"""
    bits = np.asarray(bits, dtype=np.uint8)
    nb = bits.shape[0]
    st = wire_words(desc, bits)
    nw = st.shape[0] - 1
    asserts = np.asarray(desc.asserts, dtype=np.int64).reshape(-1, 2)
    ok = np.full(st.shape[1], np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    if len(asserts):
        v = st[asserts[:, 0]]
        v = np.where((asserts[:, 1] == 1)[:, None], v, ~v)
        ok = np.bitwise_and.reduce(v, axis=0)
    holds = np.unpackbits(ok.view(np.uint8), bitorder="little")[:nb].astype(bool)
    witness = np.zeros((nb, (m + 7) // 8), dtype=np.uint8)
    step = 8192  # wires per transpose (a multiple of 8: whole output bytes)
    for w0 in range(0, nw, step):
        w1 = min(nw, w0 + step)
        tb = np.unpackbits(st[1 + w0: 1 + w1].view(np.uint8), axis=1, bitorder="little")[:, :nb]  # [wires, statements]
        witness[:, w0 // 8: (w1 + 7) // 8] = np.packbits(np.ascontiguousarray(tb.T), axis=1, bitorder="little")
    return witness, holds
