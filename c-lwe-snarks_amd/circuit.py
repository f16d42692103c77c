"""Boolean circuits as square span programs: the front end of mfh_ssp_from_rows (include/mfhip.h).

A circuit is built from public and private input wires and AND / OR / XOR / NOT gates, with assertions that a wire is 0 or 1.  compile(params) turns it
into constraint rows, one row per constraint point r_j = j + 2.  Row j asks  v_0(r_j) + sum_i a_i v_i(r_j)  in {-1, +1}, where a_i is the bit on wire i.
Context.ssp_from_rows interpolates the rows into the SSP on the device.

Wire layout: wire 0 is the constant v_0.  Public inputs take wires 1 .. lu in the order they were declared.  Private inputs follow, then the gate outputs
in creation order.  Witness bit i - 1 is wire i, so bits [0, lu) are the public statement (Context.prove_batch_public / verify_public with this lu).

Rows, all values mod p: every wire w gets 2w - 1 (it is 0 or 1).  Then each gate and each assertion gets one row:
    c = a XOR b : a + b + c - 1          c = a AND b : 2a + 2b - 4c - 1          c = a OR b : -2a - 2b + 4c - 1
    c = NOT a   : a + c                  assert a = 1 : a                         assert a = 0 : 1 - a
Each row is +-1 exactly when c is the gate's output (tests/test_circuit_cpu.py checks all eight (a, b, c)).

    c = Circuit()
    x = c.private(8); z = c.public()
    ...
    cc = c.compile(mf.DEFAULT)                         # rows, lu, wire map
    d_ssp = ctx.ssp_from_rows(cc.rows)
    witness = c.assign(public_bits, private_bits)      # (m + 7) // 8 bytes for Context.prove / prove_batch
    prog = ctx.circuit_load(cc)                        # ... or a whole batch on the device:
    witness, holds = ctx.circuit_assign(prog, bits)    # bits [nb, nin] = public then private bits; witness [nb, (m + 7) // 8]

A circuit too large for the dense SSP (d = 2^20: about 500 000 gates) is registered as its rows instead (mfh_ssp_set_rows):

    p = mf.Params(d=1 << 20, m=699050)
    cc = c.compile(p)
    ctx.ssp_set_rows(cc.rows, lu_max=cc.lu)            # no dense SSP; d_ssp=None below means these rows
    ctx.ssp_prepare(None)
    crs = ctx.setup_public(None, alpha, beta, s, cc.lu, d_sk, d_err)
    prog = ctx.circuit_load(cc, state="global")        # above 32 767 wires the wire state lives in device memory
    witness, holds = ctx.circuit_assign(prog, bits)
    proofs = ctx.prove_batch_public(crs, None, cc.lu, witness, deltas, mags, signs)
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

P = 0xFFFFFFFB  # GAMMA_P
_M1 = P - 1  # -1 mod p
# gate ops of Compiled.gates: MFH_GATE_* of include/mfhip.h (mfh_circuit_create)
GATE_XOR, GATE_AND, GATE_OR, GATE_NOT = 0, 1, 2, 3
_OPS = {"xor": GATE_XOR, "and": GATE_AND, "or": GATE_OR, "not": GATE_NOT}


class CircuitError(ValueError):
    pass


@dataclass(frozen=True)
class Wire:
    """a wire of one Circuit (node = its index among the circuit's inputs and gate outputs, in creation order)"""

    node: int


@dataclass(frozen=True)
class Compiled:
    rows: tuple      # (row_ptr, wire, coef): uint32 arrays in CSR form, for Context.ssp_from_rows
    lu: int          # public inputs = wires 1 .. lu
    wires: tuple     # wires[node]: the SSP wire of each node (Wire.node)
    nrows: int
    nwires: int      # wires 1 .. nwires are used
    # the gate program of Context.circuit_load (mfh_circuit_create), in SSP wire numbering: gate g = (op, a, b) writes wire nin + 1 + g (nin = nwires -
    # len(gates)), operands in [1, nin + g], b = a for NOT; asserts[e] = (wire, value)
    gates: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), dtype=np.uint32), compare=False)
    asserts: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), dtype=np.uint32), compare=False)

    def wire(self, w: Wire) -> int:
        return self.wires[w.node]


class Circuit:
    def __init__(self):
        self._nodes = []    # ("pub",) / ("priv",) / (gate, a, b) / ("not", a): operands are node indices
        self._asserts = []  # (node, value)
        self._pub = []      # node indices of the public inputs, in declaration order
        self._priv = []
        self._params = None

    # -- building -------------------------------------------------------------------------------------------------------
    def _check(self, w):
        if not isinstance(w, Wire) or not 0 <= w.node < len(self._nodes):
            raise CircuitError(f"{w!r} is not a wire of this circuit")

    def _new(self, kind, *ops):
        for w in ops:
            self._check(w)
        self._nodes.append((kind,) + tuple(w.node for w in ops))
        return Wire(len(self._nodes) - 1)

    def public(self, count=None):
        """one public input wire, or a list of `count` of them"""
        if count is not None:
            return [self.public() for _ in range(count)]
        w = self._new("pub")
        self._pub.append(w.node)
        return w

    def private(self, count=None):
        """one private input wire, or a list of `count` of them"""
        if count is not None:
            return [self.private() for _ in range(count)]
        w = self._new("priv")
        self._priv.append(w.node)
        return w

    def AND(self, a: Wire, b: Wire) -> Wire:
        return self._new("and", a, b)

    def OR(self, a: Wire, b: Wire) -> Wire:
        return self._new("or", a, b)

    def XOR(self, a: Wire, b: Wire) -> Wire:
        return self._new("xor", a, b)

    def NOT(self, a: Wire) -> Wire:
        return self._new("not", a)

    def assert_equal(self, w: Wire, value: int):
        if value not in (0, 1):
            raise CircuitError("assert_equal: the value must be 0 or 1")
        self._check(w)
        self._asserts.append((w.node, int(value)))

    # -- layout and rows --------------------------------------------------------------------------------------------------
    @property
    def lu(self) -> int:
        return len(self._pub)

    def _layout(self):
        wires = [0] * len(self._nodes)
        nxt = 1
        for group in (self._pub, self._priv, [i for i, n in enumerate(self._nodes) if n[0] not in ("pub", "priv")]):
            for i in group:
                wires[i] = nxt
                nxt += 1
        return wires, nxt - 1

    def compile(self, params) -> Compiled:
        """the constraint rows for an SSP of params.d points and params.m wires; CircuitError if the circuit needs more than m - 1 wires or d - 1 rows"""
        wires, nw = self._layout()
        ngates = nw - len(self._pub) - len(self._priv)
        nrows = nw + ngates + len(self._asserts)
        if nw > params.m - 1:
            raise CircuitError(f"the circuit needs {nw} wires, the SSP has {params.m - 1} (m - 1)")
        if nrows > params.d - 1:
            raise CircuitError(f"the circuit needs {nrows} rows, the SSP has {params.d - 1} points (d - 1)")
        rows = [[(w, 2), (0, _M1)] for w in range(1, nw + 1)]  # every wire is a bit
        for i, node in enumerate(self._nodes):
            kind, c = node[0], wires[i]
            if kind in ("pub", "priv"):
                continue
            a = wires[node[1]]
            if kind == "not":
                rows.append([(a, 1), (c, 1)])
                continue
            b = wires[node[2]]
            if kind == "xor":
                rows.append([(a, 1), (b, 1), (c, 1), (0, _M1)])
            elif kind == "and":
                rows.append([(a, 2), (b, 2), (c, P - 4), (0, _M1)])
            else:  # or
                rows.append([(a, P - 2), (b, P - 2), (c, 4), (0, _M1)])
        for node, value in self._asserts:
            rows.append([(wires[node], 1)] if value else [(wires[node], _M1), (0, 1)])
        assert len(rows) == nrows
        row_ptr = np.zeros(nrows + 1, dtype=np.uint32)
        np.cumsum([len(r) for r in rows], out=row_ptr[1:])
        wire = np.array([w for r in rows for w, _ in r], dtype=np.uint32)
        coef = np.array([x for r in rows for _, x in r], dtype=np.uint32)
        gates = np.array([(_OPS[n[0]], wires[n[1]], wires[n[-1]]) for n in self._nodes if n[0] not in ("pub", "priv")], dtype=np.uint32).reshape(-1, 3)
        asserts = np.array([(wires[node], value) for node, value in self._asserts], dtype=np.uint32).reshape(-1, 2)
        self._params = params
        return Compiled(rows=(row_ptr, wire, coef), lu=len(self._pub), wires=tuple(wires), nrows=nrows, nwires=nw, gates=gates, asserts=asserts)

    # -- assignments ------------------------------------------------------------------------------------------------------
    def evaluate(self, public_bits, private_bits):
        """the bit on every node (Wire.node order)"""
        public_bits, private_bits = list(public_bits), list(private_bits)
        if len(public_bits) != len(self._pub) or len(private_bits) != len(self._priv):
            raise CircuitError(f"the circuit has {len(self._pub)} public and {len(self._priv)} private inputs")
        val = [0] * len(self._nodes)
        for i, x in zip(self._pub, public_bits):
            val[i] = int(x) & 1
        for i, x in zip(self._priv, private_bits):
            val[i] = int(x) & 1
        for i, node in enumerate(self._nodes):
            kind = node[0]
            if kind == "not":
                val[i] = 1 - val[node[1]]
            elif kind == "xor":
                val[i] = val[node[1]] ^ val[node[2]]
            elif kind == "and":
                val[i] = val[node[1]] & val[node[2]]
            elif kind == "or":
                val[i] = val[node[1]] | val[node[2]]
        return val

    def holds(self, public_bits, private_bits) -> bool:
        """every assertion holds on this input (then the witness of assign satisfies every row)"""
        val = self.evaluate(public_bits, private_bits)
        return all(val[n] == v for n, v in self._asserts)

    def assign(self, public_bits, private_bits, params=None) -> bytes:
        """the input bits of a proof: (m + 7) // 8 bytes, LSB first, bit i - 1 = wire i (m from params, else from the last compile)"""
        params = params if params is not None else self._params
        if params is None:
            raise CircuitError("assign: compile the circuit first (or pass params)")
        wires, nw = self._layout()
        if nw > params.m - 1:
            raise CircuitError(f"the circuit needs {nw} wires, the SSP has {params.m - 1} (m - 1)")
        val = self.evaluate(public_bits, private_bits)
        out = bytearray((params.m + 7) // 8)
        for i, v in enumerate(val):
            if v:
                out[(wires[i] - 1) >> 3] |= 1 << ((wires[i] - 1) & 7)
        return bytes(out)

    def statement(self, public_bits) -> bytes:
        """the public statement u (bits [0, lu) of the input, LSB first) as Context.verify_public takes it"""
        public_bits = list(public_bits)
        if len(public_bits) != len(self._pub):
            raise CircuitError(f"the circuit has {len(self._pub)} public inputs")
        out = bytearray(max(1, (len(public_bits) + 7) // 8))
        for i, x in enumerate(public_bits):
            out[i >> 3] |= (int(x) & 1) << (i & 7)
        return bytes(out)
