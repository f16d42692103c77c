"""CPU: the gate program of circuit.Compiled (gates / asserts, the input of mfh_circuit_create).

1. gates and asserts restate the circuit in SSP wire numbering: gate g writes wire nin + 1 + g, its operands lie in [1, nin + g], NOT has b = a;
2. a numpy bitsliced evaluation of the program -- the computation of the device kernel, one uint32 word per wire, bit j = statement j -- equals
   Circuit.evaluate / holds / assign on random circuits, statement for statement;
3. the fields added to Compiled leave the existing ones, and equality of two compilations, as they were."""
import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from circuit_program_ref import bitsliced, random_circuit


def test_gates_and_asserts_restate_the_circuit():
    p = mf.DEBUG
    c = C.Circuit()
    u = c.public(2)
    x = c.private(3)
    g0 = c.XOR(u[0], x[0])
    g1 = c.AND(g0, x[1])
    g2 = c.OR(g1, u[1])
    g3 = c.NOT(g2)
    g4 = c.AND(x[2], x[2])
    c.assert_equal(g3, 0)
    c.assert_equal(x[1], 1)
    cc = c.compile(p)
    assert cc.gates.dtype == np.uint32 and cc.asserts.dtype == np.uint32
    nin = 5
    assert [cc.wire(g) for g in (g0, g1, g2, g3, g4)] == [nin + 1 + g for g in range(5)]
    assert cc.gates.tolist() == [
        [C.GATE_XOR, 1, 3],
        [C.GATE_AND, 6, 4],
        [C.GATE_OR, 7, 2],
        [C.GATE_NOT, 8, 8],
        [C.GATE_AND, 5, 5],
    ]
    assert cc.asserts.tolist() == [[9, 0], [4, 1]]
    assert (C.GATE_XOR, C.GATE_AND, C.GATE_OR, C.GATE_NOT) == (0, 1, 2, 3)


def test_operands_precede_outputs_on_random_circuits():
    rng = np.random.default_rng(3)
    for interleave in (False, True):
        c = random_circuit(rng, 4, 20, 300, nasserts=10, interleave=interleave)
        cc = c.compile(mf.Params(d=1024, m=512))
        ng = len(cc.gates)
        nin = cc.nwires - ng
        assert nin == 24 and ng == 300 and cc.gates.shape == (300, 3) and cc.asserts.shape == (10, 2)
        for g, (op, a, b) in enumerate(cc.gates.tolist()):
            assert 1 <= a <= nin + g and 1 <= b <= nin + g
            assert op in (0, 1, 2, 3) and (op != C.GATE_NOT or a == b)
        assert all(1 <= w <= nin + ng and v in (0, 1) for w, v in cc.asserts.tolist())


def test_empty_program():
    c = C.Circuit()
    c.public(3)
    c.private(2)
    cc = c.compile(mf.DEBUG)
    assert cc.gates.shape == (0, 3) and cc.asserts.shape == (0, 2)
    assert C.Compiled(rows=cc.rows, lu=cc.lu, wires=cc.wires, nrows=cc.nrows, nwires=cc.nwires).gates.shape == (0, 3)


def test_existing_fields_unchanged_and_equality_works():
    rng = np.random.default_rng(8)
    c = random_circuit(rng, 3, 10, 50, nasserts=4)
    a, b = c.compile(mf.DEBUG), c.compile(mf.DEBUG)
    assert a.lu == 3 and a.nwires == 63
    assert a.wires == b.wires and a.nrows == b.nrows and a.lu == b.lu
    assert a == a  # array fields stay out of the comparison


@pytest.mark.parametrize("npub,npriv,ngates,nasserts,nb", [
    (3, 12, 40, 6, 70),
    (0, 10, 50, 5, 33),     # lu = 0
    (4, 8, 0, 3, 31),       # no gates
    (16, 100, 800, 40, 65),
])
def test_bitsliced_program_equals_evaluate(npub, npriv, ngates, nasserts, nb):
    p = mf.Params(d=4096, m=2048)
    rng = np.random.default_rng(npub * 1000 + ngates)
    c = random_circuit(rng, npub, npriv, ngates, nasserts=nasserts, interleave=ngates > 0)
    cc = c.compile(p)
    bits = rng.integers(0, 2, size=(nb, npub + npriv), dtype=np.uint8)
    wit, holds = bitsliced(cc, bits, p.m)
    for b in range(nb):
        pub, priv = bits[b, :npub].tolist(), bits[b, npub:].tolist()
        assert wit[b].tobytes() == c.assign(pub, priv), b
        assert bool(holds[b]) == c.holds(pub, priv), b
    # holds is not trivially false: an XOR asserted to 1 holds on exactly the statements with different inputs
    c2 = C.Circuit()
    x = c2.private(2)
    c2.assert_equal(c2.XOR(x[0], x[1]), 1)
    cc2 = c2.compile(p)
    allin = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.uint8)
    assert bitsliced(cc2, allin, p.m)[1].tolist() == [False, True, True, False]
