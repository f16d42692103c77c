"""CPU: the level-vectorised numpy evaluator of tests/circuit_levels_ref.py (the reference of the GPU tests above MFH_CIRCUIT_MAX_WIRES).

1. it equals circuit_program_ref.bitsliced and Circuit.assign / holds on random circuits, with and without assertions, with interleaved inputs, at
   batch sizes around its 64-statement words;
2. its levels are those of mfh_circuit_create (inputs 0, a gate one more than its highest operand; NOT reads one operand);
3. a deep chain evaluates to its closed form (prefix parities), and rows are zero past nin + ngates."""
from types import SimpleNamespace

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from circuit_levels_ref import evaluate, gate_levels
from circuit_program_ref import bitsliced, random_circuit


@pytest.mark.parametrize("npub,npriv,ngates,nasserts,interleave,nb", [
    (3, 12, 40, 6, True, 70),
    (0, 10, 50, 0, False, 33),     # lu = 0, no assertion: every statement holds
    (4, 8, 0, 3, False, 31),       # no gates
    (16, 100, 800, 40, True, 65),
    (5, 30, 300, 2, True, 1),
    (2, 40, 500, 1, False, 128),
    (8, 60, 600, 5, True, 200),
])
def test_equals_bitsliced_and_assign(npub, npriv, ngates, nasserts, interleave, nb):
    p = mf.Params(d=4096, m=2048)
    rng = np.random.default_rng(npub * 1000 + ngates + nb)
    c = random_circuit(rng, npub, npriv, ngates, nasserts=nasserts, interleave=interleave)
    cc = c.compile(p)
    bits = rng.integers(0, 2, size=(nb, npub + npriv), dtype=np.uint8)
    wit, holds = evaluate(cc, bits, p.m)
    ref_w, ref_h = bitsliced(cc, bits, p.m)
    assert wit.shape == ref_w.shape and wit.dtype == np.uint8 and holds.dtype == bool
    assert np.array_equal(wit, ref_w)
    assert np.array_equal(holds, ref_h)
    for b in range(nb):
        pub, priv = bits[b, :npub].tolist(), bits[b, npub:].tolist()
        assert wit[b].tobytes() == c.assign(pub, priv), b
        assert bool(holds[b]) == c.holds(pub, priv), b
    if nasserts == 0:
        assert holds.all()


def test_holds_is_not_trivial():
    c = C.Circuit()
    x = c.private(2)
    c.assert_equal(c.XOR(x[0], x[1]), 1)
    c.assert_equal(c.NOT(x[0]), 0)
    p = mf.DEBUG
    cc = c.compile(p)
    allin = np.array([[0, 0], [0, 1], [1, 0], [1, 1]] * 20, dtype=np.uint8)
    assert evaluate(cc, allin, p.m)[1].tolist() == [False, False, True, False] * 20


def test_levels_of_create():
    # nin = 3: wires 4 .. 8 = gates 0 .. 4
    gates = [(0, 1, 2), (3, 4, 4), (1, 5, 1), (2, 2, 3), (0, 6, 7)]
    assert gate_levels(3, gates).tolist() == [1, 2, 3, 1, 4]
    assert gate_levels(5, np.zeros((0, 3), dtype=np.uint32)).tolist() == []


def test_deep_chain_prefix_parities():
    """g_k = g_{k-1} XOR x_{k mod nin}, every fifth step a NOT: depth = ngates, value = parity of a prefix of the inputs plus the NOTs so far"""
    nin, ngates, nb = 40, 3000, 70
    gates = np.zeros((ngates, 3), dtype=np.uint32)
    for k in range(ngates):
        prev = 1 if k == 0 else nin + k
        gates[k] = (C.GATE_NOT, prev, prev) if k % 5 == 4 else (C.GATE_XOR, prev, 1 + (k + 1) % nin)
    desc = SimpleNamespace(gates=gates, asserts=np.array([[nin + ngates, 1]], dtype=np.uint32), nwires=nin + ngates)
    assert gate_levels(nin, gates).max() == ngates
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 2, size=(nb, nin), dtype=np.uint8)
    m = 4096
    wit, holds = evaluate(desc, bits, m)
    val = bits[:, 0].astype(np.uint8).copy()
    exp = np.zeros((nb, m), dtype=np.uint8)
    exp[:, :nin] = bits
    for k in range(ngates):
        val = 1 - val if k % 5 == 4 else val ^ bits[:, (k + 1) % nin]
        exp[:, nin + k] = val
    assert np.array_equal(wit, np.packbits(exp, axis=1, bitorder="little"))
    assert np.array_equal(holds, val == 1)
    assert not wit[:, (nin + ngates + 7) // 8:].any()
