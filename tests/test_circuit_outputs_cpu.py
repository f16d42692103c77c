"""CPU: computed public outputs of circuit.Circuit (Circuit.output, Compiled.outputs, outputs_of).

1. the row of an output pair (p, w) is 1 - p - w: +-1 mod p exactly when p = w, over all four bit pairs;
2. outputs are public inputs in the wire layout, in declaration order among public() calls; Compiled.outputs / equal carry the pairs;
3. a circuit without outputs compiles to the arrays it compiled to before outputs existed (digests recorded from the code before), and declaring no
   output leaves Compiled.outputs empty;
4. evaluate / assign / holds ignore the caller's bits at output positions;
5. nothing may read an output wire;
6. a 32-bit add whose sum is a computed output: every row of the witness is +-1 mod p, whatever the caller wrote at the output positions, and a
   witness with one output bit flipped breaks exactly that pair's row."""
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

import circuit_ref as R
from circuit_ex_ref import random_ex_circuit

from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P = C.P
SMALL = SimpleNamespace(d=256, m=64)
ADD = SimpleNamespace(d=512, m=341)  # the 32-bit add: 160 wires, 256 rows


def _bits(values):
    out = bytearray((len(values) + 7) // 8)
    for i, v in enumerate(values):
        out[i >> 3] |= (v & 1) << (i & 7)
    return bytes(out)


def test_output_row_is_pm1_iff_equal():
    c = C.Circuit()
    x = c.private()
    p = c.output(x)
    cc = c.compile(SMALL)
    assert cc.lu == 1 and cc.nwires == 2 and cc.nrows == 3 and cc.wire(p) == 1 and cc.wire(x) == 2
    assert cc.outputs.dtype == np.uint32 and cc.outputs.tolist() == [[1, 2]] and cc.equal.tolist() == [[1, 2]]
    row_ptr, wire, coef = cc.rows
    last = sorted(zip(wire[row_ptr[2]: row_ptr[3]].tolist(), coef[row_ptr[2]: row_ptr[3]].tolist()))
    assert last == [(0, 1), (1, P - 1), (2, P - 1)]  # 1 - p - w, assert_same's row
    for pv in (0, 1):
        for wv in (0, 1):
            v = R.row_values(cc.rows, _bits([pv, wv]))[2]
            assert (v in (1, P - 1)) == (pv == wv), (pv, wv, v)


def test_outputs_keep_declaration_order_among_publics():
    c = C.Circuit()
    a = c.public()
    x = c.private(3)
    o1 = c.output(c.XOR(x[0], x[1]))
    b = c.public()
    c.assert_same(x[1], x[2])
    o2 = c.output(x[2])
    d = c.public()
    cc = c.compile(SMALL)
    assert cc.lu == 5 and c.lu == 5
    assert [cc.wire(w) for w in (a, o1, b, o2, d)] == [1, 2, 3, 4, 5]
    assert [cc.wire(w) for w in x] == [6, 7, 8] and cc.nwires == 9
    assert cc.outputs.tolist() == [[2, 9], [4, 8]]
    assert cc.equal.tolist() == [[2, 9], [7, 8], [4, 8]]  # creation order, the pairs among the equalities
    assert cc.program.tolist() == [[C.GATE_XOR, 6, 7, 0]]
    assert cc.nrows == 9 + 1 + 3


GOLDEN = {  # sha256[:32] of the arrays random_ex_circuit(default_rng(20261016), 5, 11, 400, 6, 5) compiled to before Circuit.output existed
    "row_ptr": ((780,), "7c3e58589ae71608366e73b4fba3c662"),
    "wire": ((2295,), "39621eba2b2a2f4371dcfc15409821b3"),
    "coef": ((2295,), "7619d00bba90fa03a4ab87030c832b0f"),
    "gates": ((376, 3), "4bad1b2ff90734258111e8fcb7a15ad7"),
    "program": ((376, 4), "d658a5ccbfc36dc8658dc434a45c9a0c"),
    "asserts": ((6, 2), "bea1c58f65ababeed836a88ab32d4fdf"),
    "equal": ((5, 2), "27b6b80d32e3eff28325c46d2c6d4ed9"),
}


def test_without_outputs_compile_is_unchanged():
    c = random_ex_circuit(np.random.default_rng(20261016), 5, 11, 400, nasserts=6, nequal=5)
    cc = c.compile(SimpleNamespace(d=1 << 15, m=21845))
    arrays = {"row_ptr": cc.rows[0], "wire": cc.rows[1], "coef": cc.rows[2], "gates": cc.gates, "program": cc.program, "asserts": cc.asserts,
              "equal": cc.equal}
    for name, (shape, digest) in GOLDEN.items():
        a = arrays[name]
        assert a.dtype == np.uint32 and a.shape == shape, name
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32] == digest, name
    assert cc.outputs.dtype == np.uint32 and cc.outputs.shape == (0, 2)
    # the same circuit built a second time compiles to the same arrays, and an output added to it changes lu, equal and outputs only by its pair
    c2 = random_ex_circuit(np.random.default_rng(20261016), 5, 11, 400, nasserts=6, nequal=5)
    c2.output(C.Wire(20))
    cc2 = c2.compile(SimpleNamespace(d=1 << 15, m=21845))
    assert cc2.lu == cc.lu + 1 and cc2.nwires == cc.nwires + 1 and cc2.nrows == cc.nrows + 2
    assert len(cc2.program) == len(cc.program) and np.array_equal(cc2.program[:, 0], cc.program[:, 0])
    assert len(cc2.equal) == 6 and cc2.equal[-1].tolist() == cc2.outputs[0].tolist() == [6, cc2.wires[20]]


def test_evaluate_assign_holds_ignore_the_output_positions():
    rng = np.random.default_rng(5)
    c = C.Circuit()
    a = c.public(2)
    x = c.private(6)
    g = c.AND(c.XOR(x[0], a[0]), c.OR(x[1], x[2]))
    s, k = c.full_add(x[3], x[4], x[5])
    outs = [c.output(w) for w in (g, s, k, x[0])]
    c.assert_equal(c.OR(a[1], c.NOT(a[1])), 1)
    cc = c.compile(SMALL)
    assert cc.lu == 6
    for _ in range(40):
        pub = rng.integers(0, 2, size=6).tolist()
        prv = rng.integers(0, 2, size=6).tolist()
        val = c.evaluate(pub, prv)
        exp = [(prv[0] ^ pub[0]) & (prv[1] | prv[2]), prv[3] ^ prv[4] ^ prv[5], int(prv[3] + prv[4] + prv[5] >= 2), prv[0]]
        assert [val[o.node] for o in outs] == exp
        assert c.holds(pub, prv)  # with garbage at the output positions
        clean = pub[:2] + [0, 0, 0, 0]
        wit = c.assign(pub, prv)
        assert wit == c.assign(clean, prv) == c.assign(pub[:2] + exp, prv)
        assert R.satisfied(cc.rows, wit)
        stmt = c.outputs_of(wit)
        assert stmt == c.statement(pub[:2] + exp) and len(stmt) == 1
        assert c.outputs_of(np.frombuffer(wit, dtype=np.uint8)) == stmt
    with pytest.raises(C.CircuitError):
        c.evaluate([0, 0], [0] * 6)  # the output positions are part of the public bits
    with pytest.raises(C.CircuitError):
        c.outputs_of(b"")


def test_nothing_reads_an_output_wire():
    c = C.Circuit()
    x = c.private(2)
    o = c.output(x[0])
    for bad in (lambda: c.AND(o, x[1]), lambda: c.NOT(o), lambda: c.MAJ(x[0], x[1], o), lambda: c.gate(6, x[0], o), lambda: c.assert_equal(o, 1),
                lambda: c.assert_same(o, x[1]), lambda: c.assert_same(x[1], o), lambda: c.output(o)):
        with pytest.raises(C.CircuitError, match="computed public output"):
            bad()
    cc = c.compile(SMALL)
    assert cc.nwires == 3 and len(cc.program) == 0 and cc.outputs.tolist() == [[1, 2]]  # nothing was added by the refused calls


def test_add_with_output_sum_satisfies_every_row():
    w = W.Words()
    x, y = w.private(), w.private()
    s = w.output(w.add(x, y))
    c = w.c
    cc = c.compile(ADD)
    assert cc.lu == 32 and cc.nwires == 160 and cc.nrows == 160 + 64 + 32 and len(cc.outputs) == 32
    assert [cc.wire(b) for b in s] == list(range(1, 33))
    rng = np.random.default_rng(11)
    for xv, yv in [(0, 0), (0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF)] + [tuple(int(v) for v in rng.integers(0, 1 << 32, size=2, dtype=np.uint64))
                                                                        for _ in range(5)]:
        garbage = rng.integers(0, 2, size=32).tolist()
        prv = W.pack([xv, yv])
        wit = c.assign(garbage, prv)
        vals = R.row_values(cc.rows, wit)
        assert len(vals) == cc.nrows and all(v in (1, P - 1) for v in vals)
        assert W.unpack(np.unpackbits(np.frombuffer(c.outputs_of(wit), dtype=np.uint8), bitorder="little"))[0] == (xv + yv) & 0xFFFFFFFF
        assert c.holds(garbage, prv)
        # a claimed sum that differs in one bit breaks that pair's equality row and no other
        bad = bytearray(wit)
        bad[1] ^= 1 << 3  # output bit 11 = wire 12
        vals = R.row_values(cc.rows, bytes(bad))
        wrong = [j for j, v in enumerate(vals) if v not in (1, P - 1)]
        assert wrong == [160 + 64 + 11]
