"""CPU: the extended gates (MAJ, SUM3, CONST, LUT2), equalities, the 32-bit word layer and the ChaCha20 block statement.

1. every new row, enumerated over all bit assignments, is +-1 mod p exactly when the output is right -- all 16 LUT2 tables, MAJ, SUM3 with its MAJ's
   row and the bit rows, CONST, assert_same -- and the LUT2 rows of XOR / AND / OR / NOT are today's rows of those gates;
2. circuits of the four original ops compile as before (program / equal extend Compiled, the old fields unchanged);
3. a numpy bitsliced evaluation of Compiled.program (the computation of k_circuit_eval_ex) equals Circuit.evaluate / holds / assign on random mixed
   circuits; the validation rules of mfh_circuit_create_ex, restated in Python, accept compiled circuits and reject one case per rule;
4. words: random expressions against Python integers, the exact costs of an add, the RFC 8439 quarter-round and block vectors, the block statement's
   wire and row counts."""
import itertools

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W
from circuit_ex_ref import (M32, bitsliced_ex, chacha20_block_int, einval_cases, quarter_round_int, random_ex_circuit, validate_ex)

P = C.P


def _value(row, bits):
    """a row (list of (wire, coef)) at wire values bits (bits[0] = 1, the constant) mod p"""
    return sum(coef * bits[w] for w, coef in row) % P


def _rows(cc):
    row_ptr, wire, coef = cc.rows
    return [list(zip(wire[row_ptr[j]: row_ptr[j + 1]].tolist(), coef[row_ptr[j]: row_ptr[j + 1]].tolist())) for j in range(cc.nrows)]


def _pm1(v):
    return v in (1, P - 1)


# ------------------------------------------------------------------ 1. rows, exhaustively
def _gate_row(build):
    """compile a circuit of three inputs a, b, c and one gate; return (row of the gate, wire map of a, b, c, out)"""
    c = C.Circuit()
    x = c.private(3)
    out = build(c, *x)
    cc = c.compile(mf.DEBUG)
    rows = _rows(cc)
    return rows[cc.nwires], [cc.wire(w) for w in x] + [cc.wire(out)]


@pytest.mark.parametrize("tt", range(16))
def test_lut2_rows(tt):
    row, (wa, wb, _, wc) = _gate_row(lambda c, a, b, d: c.gate(tt, a, b))
    for a, b, out in itertools.product((0, 1), repeat=3):
        bits = {0: 1, wa: a, wb: b, wc: out, 3: 0}
        assert _pm1(_value(row, bits)) == (out == (tt >> (a + 2 * b)) & 1), (tt, a, b, out)


def test_lut2_rows_of_the_original_functions_are_todays_rows():
    for tt, build in ((0b0110, "XOR"), (0b1000, "AND"), (0b1110, "OR")):
        row, wires = _gate_row(lambda c, a, b, d: c.gate(tt, a, b))
        old, wires_old = _gate_row(lambda c, a, b, d: getattr(c, build)(a, b))
        assert wires == wires_old and sorted(row) == sorted(old), build
    row, _ = _gate_row(lambda c, a, b, d: c.gate(0b0101, a, a))  # NOT a as a LUT2 of (a, a)
    old, _ = _gate_row(lambda c, a, b, d: c.NOT(a))
    assert sorted(row) == sorted(old)


def test_lut2_row_classes():
    a, b, c = 1, 2, 3
    assert C.lut2_row(0, a, b, c) == ([(c, -1)], 1) and C.lut2_row(15, a, b, c) == ([(c, 1)], 0)
    assert C.lut2_row(0b0110, a, b, c) == ([(a, 1), (b, 1), (c, 1)], -1)
    assert C.lut2_row(0b1001, a, b, c) == ([(a, 1), (b, 1), (c, -1)], 0)
    assert C.lut2_row(0b1000, a, b, c) == ([(a, 2), (b, 2), (c, -4)], -1)  # AND
    assert C.lut2_row(0b1110, a, b, c) == ([(a, -2), (b, -2), (c, 4)], -1)  # OR


def test_named_gates():
    c = C.Circuit()
    x, y = c.private(2)
    gates = {"NAND": c.NAND(x, y), "NOR": c.NOR(x, y), "XNOR": c.XNOR(x, y), "ANDN": c.ANDN(x, y), "ORN": c.ORN(x, y)}
    ref = {"NAND": lambda a, b: 1 - (a & b), "NOR": lambda a, b: 1 - (a | b), "XNOR": lambda a, b: 1 - (a ^ b), "ANDN": lambda a, b: a & (1 - b),
           "ORN": lambda a, b: a | (1 - b)}
    for a, b in itertools.product((0, 1), repeat=2):
        val = c.evaluate([], [a, b])
        for name, w in gates.items():
            assert val[w.node] == ref[name](a, b), (name, a, b)


def test_maj_row():
    row, (wa, wb, wd, wk) = _gate_row(lambda c, a, b, d: c.MAJ(a, b, d))
    for a, b, d, k in itertools.product((0, 1), repeat=4):
        assert _pm1(_value(row, {0: 1, wa: a, wb: b, wd: d, wk: k})) == (k == int(a + b + d >= 2))


def test_sum3_with_its_maj_and_bit_rows():
    """with the MAJ row, the SUM3 row and the two bit rows over all of F_p's {0, 1} assignments -- and over k, s in {0, 1, 2, p - 1} -- only the true
    (k, s) satisfies every row"""
    c = C.Circuit()
    x = c.private(3)
    s, k = c.full_add(*x)
    cc = c.compile(mf.DEBUG)
    rows = _rows(cc)
    ws, wk = cc.wire(s), cc.wire(k)
    assert wk + 1 == ws and cc.nrows == 5 + 2
    check = [rows[wk - 1], rows[ws - 1], rows[5], rows[6]]  # bit rows of k and s, the MAJ row, the SUM3 row
    for a, b, d in itertools.product((0, 1), repeat=3):
        sat = []
        for kv, sv in itertools.product((0, 1, 2, P - 1), repeat=2):
            bits = {0: 1, cc.wire(x[0]): a, cc.wire(x[1]): b, cc.wire(x[2]): d, wk: kv, ws: sv}
            if all(_pm1(_value(r, bits)) for r in check):
                sat.append((kv, sv))
        assert sat == [(int(a + b + d >= 2), a ^ b ^ d)], (a, b, d, sat)
    assert cc.program.tolist() == [[C.GATE_MAJ, 1, 2, 3], [C.GATE_SUM3, 1, 2, 3]]


def test_const_rows_and_sharing():
    c = C.Circuit()
    c.private(1)
    z, o = c.const(0), c.const(1)
    assert c.const(0) == z and c.const(1) == o
    cc = c.compile(mf.DEBUG)
    rows = _rows(cc)
    assert cc.nwires == 3 and cc.nrows == 5
    for w, v, row in ((z, 0, rows[3]), (o, 1, rows[4])):
        for x in (0, 1):
            assert _pm1(_value(row, {0: 1, cc.wire(w): x})) == (x == v)
    assert cc.program.tolist() == [[C.GATE_CONST0, 0, 0, 0], [C.GATE_CONST1, 0, 0, 0]]
    assert c.evaluate([], [1]) == [1, 0, 1]


def test_assert_same_row_and_order():
    c = C.Circuit()
    x = c.private(3)
    g = c.XOR(x[0], x[1])
    c.assert_same(x[2], g)
    c.assert_equal(x[0], 1)
    c.assert_same(x[0], x[1])
    cc = c.compile(mf.DEBUG)
    rows = _rows(cc)
    assert cc.nrows == 4 + 1 + 1 + 2 and cc.nwires == 4
    assert cc.equal.tolist() == [[3, 4], [1, 2]]  # creation order, after the value assertion's row
    assert rows[5] == [(1, 1)]
    for r, (wa, wb) in zip(rows[6:], cc.equal.tolist()):
        for a, b in itertools.product((0, 1), repeat=2):
            assert _pm1(_value(r, {0: 1, wa: a, wb: b})) == (a == b)
    assert c.holds([], [1, 1, 0]) and not c.holds([], [1, 1, 1]) and not c.holds([], [1, 0, 1])
    with pytest.raises(C.CircuitError):
        c.assert_same(x[0], x[0])


def test_satisfying_witness_satisfies_every_row():
    """Circuit.assign of a holding statement makes every row +-1 (the SSP is satisfied), and a failing equality breaks exactly its row"""
    rng = np.random.default_rng(5)
    c = random_ex_circuit(rng, 3, 6, 120)
    pub, prv = rng.integers(0, 2, 3).tolist(), rng.integers(0, 2, 6).tolist()
    val = c.evaluate(pub, prv)
    nodes = [i for i in range(len(val)) if i >= 9]
    for a, b in zip(nodes[:10], nodes[10:20]):
        if val[a] == val[b]:
            c.assert_same(C.Wire(a), C.Wire(b))
    cc = c.compile(mf.Params(d=1024, m=512))
    bits = {0: 1}
    for node, v in enumerate(val):
        bits[cc.wires[node]] = v
    assert c.holds(pub, prv)
    assert all(_pm1(_value(r, bits)) for r in _rows(cc))
    wa, wb = cc.equal[0].tolist()
    bits[wb] = 1 - bits[wb]
    bad = [j for j, r in enumerate(_rows(cc)) if not _pm1(_value(r, bits))]
    assert cc.nrows - len(cc.equal) in bad and (wb - 1) not in bad


# ------------------------------------------------------------------ 2. old-op circuits unchanged
def test_old_op_circuits_compile_as_before():
    from circuit_program_ref import random_circuit

    rng = np.random.default_rng(11)
    c = random_circuit(rng, 3, 10, 60, nasserts=5)
    cc = c.compile(mf.Params(d=1024, m=512))
    assert cc.gates.shape == (60, 3) and cc.program.shape == (60, 4) and cc.equal.shape == (0, 2)
    assert np.array_equal(cc.program[:, :3], cc.gates) and not cc.program[:, 3].any() and (cc.program[:, 0] <= 3).all()
    # the rows of the original four gates, as the module docstring gives them
    rows = _rows(cc)
    for g, (op, a, b) in enumerate(cc.gates.tolist()):
        o = cc.nwires - 60 + 1 + g
        exp = {0: [(a, 1), (b, 1), (o, 1), (0, P - 1)], 1: [(a, 2), (b, 2), (o, P - 4), (0, P - 1)], 2: [(a, P - 2), (b, P - 2), (o, 4), (0, P - 1)],
               3: [(a, 1), (o, 1)]}[op]
        assert rows[cc.nwires + g] == exp
    empty = C.Compiled(rows=cc.rows, lu=cc.lu, wires=cc.wires, nrows=cc.nrows, nwires=cc.nwires)
    assert empty.program.shape == (0, 4) and empty.equal.shape == (0, 2) and empty == cc


# ------------------------------------------------------------------ 3. bitsliced reference and validation
@pytest.mark.parametrize("npub,npriv,ngates,nasserts,nequal,nb", [
    (3, 12, 60, 5, 4, 70),
    (0, 10, 200, 3, 10, 33),
    (16, 40, 800, 20, 30, 65),
])
def test_bitsliced_ex_equals_evaluate(npub, npriv, ngates, nasserts, nequal, nb):
    rng = np.random.default_rng(npub * 1000 + ngates)
    c = random_ex_circuit(rng, npub, npriv, ngates, nasserts, nequal)
    p = mf.Params(d=4096, m=1200)
    cc = c.compile(p)
    assert set(cc.program[:, 0].tolist()) & {4, 5, 6, 7} and (cc.program[:, 0] >= 16).any()
    nin = npub + npriv
    bits = rng.integers(0, 2, size=(nb, nin), dtype=np.uint8)
    wit, holds = bitsliced_ex(cc, bits, p.m)
    for b in range(nb):
        pub, prv = bits[b, :npub].tolist(), bits[b, npub:].tolist()
        assert wit[b].tobytes() == c.assign(pub, prv, p), b
        assert bool(holds[b]) == c.holds(pub, prv), b
    assert validate_ex(nin, cc.program, cc.asserts, cc.equal, p.m) is None


def test_bitsliced_ex_holds_both_ways():
    rng = np.random.default_rng(4)
    c = random_ex_circuit(rng, 2, 8, 100)
    x = [C.Wire(i) for i in range(10)]
    c.assert_same(x[2], x[3])
    c.assert_equal(x[4], 1)
    p = mf.Params(d=1024, m=512)
    cc = c.compile(p)
    bits = rng.integers(0, 2, size=(100, 10), dtype=np.uint8)
    _, holds = bitsliced_ex(cc, bits, p.m)
    exp = (bits[:, 2] == bits[:, 3]) & (bits[:, 4] == 1)
    assert 10 < exp.sum() < 90 and np.array_equal(holds, exp)


def test_validation_rules():
    for name, (nin, program, asserts, equal, m, flags, text) in einval_cases().items():
        assert validate_ex(nin, program, asserts, equal, m, flags) == text, name
    ok = [(0, 1, 2, 0), (4, 1, 2, 5), (5, 1, 2, 5), (6, 0, 0, 0), (7, 0, 0, 0), (C.GATE_LUT2(13), 8, 9, 0), (3, 10, 10, 0)]
    assert validate_ex(4, ok, [(11, 0)], [(1, 11)], 64) is None
    assert validate_ex(60, [(6, 0, 0, 0)] * 3, [], [], 64) is None  # exactly m - 1
    assert validate_ex(40000 - 100, [(6, 0, 0, 0)] * 99, [], [], 40000, 1) is None  # global: m - 1 alone


def test_circuit_rejects_bad_uses():
    c = C.Circuit()
    x = c.private(2)
    with pytest.raises(C.CircuitError):
        c.gate(16, x[0], x[1])
    with pytest.raises(C.CircuitError):
        c.const(2)
    with pytest.raises(C.CircuitError):
        c.MAJ(x[0], x[1], C.Wire(7))
    with pytest.raises(C.CircuitError):
        c.assert_same(x[0], C.Wire(9))


# ------------------------------------------------------------------ 4. words and ChaCha20
def _eval_words(w, words, pub_vals, priv_vals):
    c = w.c
    val = c.evaluate(W.pack(pub_vals) if pub_vals else [], W.pack(priv_vals) if priv_vals else [])
    return [sum(val[b.node] << i for i, b in enumerate(x)) for x in words]


def test_pack_unpack():
    rng = np.random.default_rng(2)
    vals = [int(v) for v in rng.integers(0, 1 << 32, size=7, dtype=np.uint64)] + [0, M32]
    bits = W.pack(vals)
    assert bits.shape == (9 * 32,) and bits.dtype == np.uint8 and W.unpack(bits) == vals
    assert bits[:32].tolist() == [(vals[0] >> i) & 1 for i in range(32)]
    arr = np.array([vals[:3], vals[3:6]], dtype=np.uint64)
    b2 = W.pack(arr)
    assert b2.shape == (2, 96) and np.array_equal(W.unpack(b2), arr.astype(np.uint32))


def test_random_word_expressions():
    rng = np.random.default_rng(17)
    ops = ["add", "xor", "and_", "or_", "not_", "rotl", "rotr", "shr", "ch", "maj", "const"]
    for trial in range(6):
        w = W.Words()
        pub, priv = w.public(2), w.private(3)
        pv = [int(v) for v in rng.integers(0, 1 << 32, size=2, dtype=np.uint64)]
        sv = [int(v) for v in rng.integers(0, 1 << 32, size=3, dtype=np.uint64)]
        wires, vals = pub + priv, pv + sv
        for _ in range(40):
            op = ops[int(rng.integers(0, len(ops)))]
            i, j, k = (int(rng.integers(0, len(wires))) for _ in range(3))
            x, y, z = vals[i], vals[j], vals[k]
            n = int(rng.integers(0, 33))
            if op == "add":
                wires.append(w.add(wires[i], wires[j])); vals.append((x + y) & M32)
            elif op in ("xor", "and_", "or_"):
                wires.append(getattr(w, op)(wires[i], wires[j])); vals.append({"xor": x ^ y, "and_": x & y, "or_": x | y}[op])
            elif op == "not_":
                wires.append(w.not_(wires[i])); vals.append(~x & M32)
            elif op == "rotl":
                wires.append(w.rotl(wires[i], n)); vals.append(((x << (n % 32)) | (x >> (32 - n % 32))) & M32)
            elif op == "rotr":
                wires.append(w.rotr(wires[i], n)); vals.append(((x >> (n % 32)) | (x << (32 - n % 32))) & M32)
            elif op == "shr":
                wires.append(w.shr(wires[i], n)); vals.append(x >> n)
            elif op == "ch":
                wires.append(w.ch(wires[i], wires[j], wires[k])); vals.append((x & y) ^ (~x & z & M32))
            elif op == "maj":
                wires.append(w.maj(wires[i], wires[j], wires[k])); vals.append((x & y) ^ (x & z) ^ (y & z))
            else:
                v = int(rng.integers(0, 1 << 32, dtype=np.uint64))
                wires.append(w.const(v)); vals.append(v)
        assert _eval_words(w, wires, pv, sv) == vals, trial
        # assert_u32 / assert_same_u32 hold exactly on the true values
        w.assert_u32(wires[-1], vals[-1])
        w.assert_same_u32(wires[-2], w.const(vals[-2]))
        assert w.c.holds(W.pack(pv), W.pack(sv))
        w.assert_u32(wires[0], vals[0] ^ 1)
        assert not w.c.holds(W.pack(pv), W.pack(sv))


def test_word_costs():
    w = W.Words()
    x, y = w.public(), w.private()
    c = w.c
    base = len(c._nodes)
    s = w.add(x, y)
    cc = c.compile(mf.Params(d=1024, m=512))
    assert len(c._nodes) - base == 64 and cc.nwires == 64 + 64 and cc.nrows == 128 + 64  # 64 wires: 64 bit rows + 64 gate rows
    assert cc.program[:2, 0].tolist() == [C.GATE_XOR, C.GATE_AND]
    assert cc.program[2:, 0].tolist() == [C.GATE_MAJ, C.GATE_SUM3] * 31
    n = len(c._nodes)
    w.xor(s, x)
    assert len(c._nodes) - n == 32
    n = len(c._nodes)
    w.rotl(s, 7), w.rotr(s, 3)
    assert len(c._nodes) == n
    w.shr(s, 5), w.shr(x, 9), w.const(0xDEADBEEF)
    assert len(c._nodes) - n == 2  # the two shared constant wires, once
    n = len(c._nodes)
    w.maj(x, y, s)
    assert len(c._nodes) - n == 32


def test_rfc8439_quarter_round():
    a, b, c, d = 0x11111111, 0x01020304, 0x9B8D6F43, 0x01234567
    exp = (0xEA2A92F4, 0xCB1CF8CE, 0x4581472E, 0x5881C4BB)
    assert quarter_round_int(a, b, c, d) == exp
    w = W.Words()
    ins = w.private(4)
    out = W.quarter_round(w, *ins)
    assert tuple(_eval_words(w, out, [], [a, b, c, d])) == exp


RFC_KEY = bytes(range(32))
RFC_NONCE = bytes.fromhex("000000090000004a00000000")
RFC_BLOCK = bytes.fromhex(
    "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
    "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_rfc8439_block_through_evaluate():
    assert chacha20_block_int(RFC_KEY, 1, RFC_NONCE) == RFC_BLOCK
    st = W.ChaCha20Block()
    c = st.circuit
    bits = st.bits(RFC_KEY, 1, RFC_NONCE, RFC_BLOCK)
    assert bits.shape == (896,)
    val = c.evaluate(bits[:640], bits[640:])
    out = b"".join(sum(val[b.node] << i for i, b in enumerate(word)).to_bytes(4, "little") for word in st.out)
    assert out == RFC_BLOCK and out[:8].hex() == "10f1e7e4d13b5915" and out[-4:].hex() == "a2503c4e"
    assert c.holds(bits[:640], bits[640:])
    for flip in (0, 31, 32 + 7, 128 + 300, 639):  # counter, nonce, block bits
        b2 = bits.copy()
        b2[flip] ^= 1
        assert not c.holds(b2[:640], b2[640:]), flip
    rng = np.random.default_rng(9)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8).tolist())
    assert not c.holds(st.public_bits(1, RFC_NONCE, RFC_BLOCK), st.private_bits(key))
    blk = chacha20_block_int(key, 7, RFC_NONCE)
    assert c.holds(st.public_bits(7, RFC_NONCE, blk), st.private_bits(key))


def test_block_statement_counts():
    st = W.ChaCha20Block()
    p = mf.Params(d=1 << 16, m=43690)
    cc = st.circuit.compile(p)
    assert cc.lu == 640 and cc.nwires == 32642 and cc.nrows == 64900
    assert cc.nwires == 896 + 2 + 336 * 64 + 320 * 32 and cc.nrows == 32642 + 31746 + 512
    assert len(cc.equal) == 512 and len(cc.asserts) == 0 and len(cc.program) == 31746
    assert cc.nwires <= 32767 and cc.nwires <= p.m - 1 and cc.nrows <= p.d - 1
    assert validate_ex(896, cc.program, cc.asserts, cc.equal, p.m) is None
    with pytest.raises(C.CircuitError):
        st.circuit.compile(mf.DEFAULT)  # 64 900 rows do not fit d = 2^15
