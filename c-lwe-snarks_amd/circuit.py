"""Boolean circuits as square span programs: the front end of mfh_ssp_from_rows (include/mfhip.h).

A circuit is built from public and private input wires and gates -- AND / OR / XOR / NOT, MAJ and its paired SUM3 (full_add), any two-input function
(gate, NAND, NOR, XNOR, ANDN, ORN), constants (const) and weighted sums (wsum) -- with assertions that a wire is 0 or 1 and that two wires are equal.  compile(params) turns it
into constraint rows, one row per constraint point r_j = j + 2.  Row j asks  v_0(r_j) + sum_i a_i v_i(r_j)  in {-1, +1}, where a_i is the bit on wire i.
Context.ssp_from_rows interpolates the rows into the SSP on the device.

Wire layout: wire 0 is the constant v_0.  Public inputs take wires 1 .. lu in the order they were declared.  Private inputs follow, then the gate outputs
in creation order.  Witness bit i - 1 is wire i, so bits [0, lu) are the public statement (Context.prove_batch_public / verify_public with this lu).

Computed public outputs: p = c.output(w) declares a public wire p whose value is DEFINED as that of wire w.  In the layout p is a public input like any
other (wires 1 .. lu in declaration order, public() and output() interleaved as declared) and it costs one equality row 1 - p - w, in the equalities'
place in the row order; Compiled.outputs records (p, w).  evaluate / assign / holds ignore what the caller put at p's input position and use w's value,
and so does Context.circuit_assign, so the caller gives the inputs and reads the statement back: outputs_of(witness_row).  Nothing may read an output
wire (no gate, assertion or equality takes it as an operand): its value exists only once the whole circuit has been evaluated.

Rows, all values mod p: every wire w gets 2w - 1 (it is 0 or 1).  Then each gate and each assertion gets one row:
    c = a XOR b : a + b + c - 1          c = a AND b : 2a + 2b - 4c - 1          c = a OR b : -2a - 2b + 4c - 1
    c = NOT a   : a + c                  assert a = 1 : a                         assert a = 0 : 1 - a
    k = MAJ(a, b, c)  : 2a + 2b + 2c - 4k - 1           s = SUM3(a, b, c) : 1 - a - b - c + 2k - s  (k = the MAJ gate just before, same operands)
    c = CONST0 : 1 - c                   c = CONST1 : c                           assert_same(a, b) : 1 - a - b  (no wire)
    c = LUT2(tt)(a, b) = (tt >> (a + 2b)) & 1, by the class of tt:
        tt = 0 : 1 - c      tt = 15 : c      c = a : 1 - a - c      c = NOT a : a + c      c = b : 1 - b - c      c = NOT b : b + c
        XOR (6) : a + b + c - 1      XNOR (9) : a + b - c
        one 1, at (x, y)    : 2a' + 2b' - 4c - 1      (a' = a if x = 1 else 1 - a; b' likewise from y)
        three 1s, 0 at (x, y): 2a' + 2b' + 4c - 5
    o_0 .. o_{n-1} = WSUM(terms), terms = (x_e, shift_e), n = bitlength(sum_e 2^shift_e) <= 24: TWO rows for the n output wires together,
        2X - 1  and  2X + 1,   X = sum_e 2^shift_e x_e - sum_i 2^i o_i
    The first is +-1 iff X in {0, 1} mod p, the second iff X in {0, -1}: together X = 0 mod p.  Operands and outputs are bits (their bit rows), so
    |X| < 2^n <= 2^24 < p and X = 0 over the integers: the o_i are the binary expansion of the sum.  A wire may occur in several terms.
Each row is +-1 exactly when c is the gate's output (tests/test_circuit_cpu.py checks all eight (a, b, c) of the first four gates,
tests/test_circuit_gates_cpu.py every other row over all its inputs).  SUM3 is sound only because MAJ's row forces k, which is why full_add emits the
two back to back.  Row order: the bit rows, one row per gate in creation order (a wsum's two rows at the place of its first output wire, none for
its other output wires), the value assertions, then the equalities in creation order.  Compiled.row_source(j) maps a row index back to its wire, gate record,
assertion or equality (Context.ssp_rows_violations reports row indices).

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
# ... and of Compiled.program (mfh_circuit_create_ex)
GATE_MAJ, GATE_SUM3, GATE_CONST0, GATE_CONST1 = 4, 5, 6, 7
# ... and of the programs of mfh_circuit_create_sum: a head (GATE_WSUM, first_term, nterms, nbits), then nbits - 1 records (GATE_WSUM_BIT, i, 0, 0)
GATE_WSUM, GATE_WSUM_BIT = 8, 9
WSUM_MAX_BITS = 24  # the most output wires of one wsum gate: |X| < 2^24 keeps the two rows sound mod p


def GATE_LUT2(tt):
    return 16 + tt


_OPS = {"xor": GATE_XOR, "and": GATE_AND, "or": GATE_OR, "not": GATE_NOT, "maj": GATE_MAJ, "sum3": GATE_SUM3}
# truth tables of the named two-input gates: bit (a + 2b) is the output on (a, b)
TT_NAND, TT_NOR, TT_XNOR, TT_ANDN, TT_ORN = 0b0111, 0b0001, 0b1001, 0b0010, 0b1011  # ANDN = a AND NOT b, ORN = a OR NOT b


def lut2_row(tt, a, b, c):
    """the constraint row of c = LUT2(tt)(a, b) on SSP wires a, b, c: ([(wire, coef mod p)], constant mod p)"""
    ones = [(x, y) for y in (0, 1) for x in (0, 1) if (tt >> (x + 2 * y)) & 1]
    if tt == 0:
        return [(c, -1)], 1
    if tt == 15:
        return [(c, 1)], 0
    if tt == 0b1010:  # c = a
        return [(a, -1), (c, -1)], 1
    if tt == 0b0101:  # c = NOT a
        return [(a, 1), (c, 1)], 0
    if tt == 0b1100:  # c = b
        return [(b, -1), (c, -1)], 1
    if tt == 0b0011:  # c = NOT b
        return [(b, 1), (c, 1)], 0
    if tt == 0b0110:
        return [(a, 1), (b, 1), (c, 1)], -1
    if tt == 0b1001:
        return [(a, 1), (b, 1), (c, -1)], 0
    if len(ones) == 1:
        (x, y), sign, const = ones[0], -4, -1
    else:
        assert len(ones) == 3
        (x, y), = [(x, y) for y in (0, 1) for x in (0, 1) if not (tt >> (x + 2 * y)) & 1]
        sign, const = 4, -5
    # 2a' = 2a (x = 1) or 2 - 2a (x = 0)
    const += (0 if x else 2) + (0 if y else 2)
    return [(a, 2 if x else -2), (b, 2 if y else -2), (c, sign)], const


def _modrow(terms, const):
    """a row of (wire, coef) with coefficients mod p, the constant as wire 0 (omitted when 0)"""
    row = [(w, x % P) for w, x in terms]
    if const % P:
        row.append((0, const % P))
    return row


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
    # the same program with three operands (mfh_circuit_create_ex): program[g] = (op, a, b, c), c = 0 but for MAJ / SUM3, a = b = c = 0 for CONST;
    # gates = program[:, :3].  equal[e] = (a, b): the wires of assert_same, in creation order
    program: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), dtype=np.uint32), compare=False)
    equal: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), dtype=np.uint32), compare=False)
    # computed public outputs (mfh_circuit_create_out): outputs[e] = (p, w), public wire p defined as wire w, in declaration order; each pair is also in equal
    outputs: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), dtype=np.uint32), compare=False)
    # the terms of the wsum gates (mfh_circuit_create_sum): terms[e] = (wire, shift); a head record of program names its slice, sorted by shift
    terms: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), dtype=np.uint32), compare=False)

    def wire(self, w: Wire) -> int:
        return self.wires[w.node]

    def row_source(self, j: int):
        """what row j of rows constrains, by compile's row order: ("bit", wire) -- the bit row of that SSP wire; ("gate", g) -- a row of program[g] (both rows
        of a WSUM head map to the head; a WSUM_BIT record has no row); ("assert", e) -- asserts[e]; ("equal", e) -- equal[e].  Names a row that
        Context.ssp_rows_violations reports."""
        j = int(j)
        if not 0 <= j < self.nrows:
            raise CircuitError(f"row_source: row {j} is not one of the {self.nrows} rows")
        if j < self.nwires:
            return ("bit", j + 1)
        k = j - self.nwires
        op = self.program[:, 0]
        ends = np.cumsum(np.where(op == GATE_WSUM, 2, np.where(op == GATE_WSUM_BIT, 0, 1)))  # ends[g]: gate rows up to and including program[g]
        ngate = int(ends[-1]) if len(ends) else 0
        if k < ngate:
            return ("gate", int(np.searchsorted(ends, k, side="right")))
        k -= ngate
        if k < len(self.asserts):
            return ("assert", k)
        return ("equal", k - len(self.asserts))


class Circuit:
    def __init__(self):
        # ("pub",) / ("priv",) / ("out", w) / (gate, a, b) / ("not", a) / ("maj" | "sum3", a, b, c) / ("lut", tt, a, b) / ("const", v) /
        # ("wsum", nbits, ((a, shift), ...)) / ("wsumbit", i, head): operands are node indices
        self._nodes = []
        self._asserts = []  # (node, value)
        self._equal = []    # (node, node) of assert_same
        self._const = {}    # value -> node of the shared constant wire
        self._pub = []      # node indices of the public inputs, in declaration order (computed outputs among them)
        self._outputs = []  # (node of the output wire p, node w) of output
        self._priv = []
        self._params = None

    # -- building -------------------------------------------------------------------------------------------------------
    def _check(self, w):
        if not isinstance(w, Wire) or not 0 <= w.node < len(self._nodes):
            raise CircuitError(f"{w!r} is not a wire of this circuit")
        if self._nodes[w.node][0] == "out":
            raise CircuitError(f"{w!r} is a computed public output: nothing may read it")

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

    def public_last(self, wires):
        """move the public input wires `wires`, in the order given, behind every public wire declared so far.  Public wires are laid out in declaration
        order, and a gate reads only wires made before it: an input that the computed outputs depend on is declared early, and this puts it behind
        the outputs in the statement all the same.  It changes the layout alone, no node."""
        wires = list(wires)
        nodes = [w.node for w in wires]
        for w in wires:
            self._check(w)
        if len(set(nodes)) != len(nodes) or any(self._nodes[n][0] != "pub" for n in nodes):
            raise CircuitError("public_last: distinct public input wires of this circuit")
        moved = set(nodes)
        self._pub = [n for n in self._pub if n not in moved] + nodes

    def output(self, w: Wire) -> Wire:
        """a public wire whose value is defined as that of wire w (a computed public output): a public input in the wire layout, one equality row
        1 - p - w, and a pair in Compiled.outputs.  The returned wire only names the position in the statement: nothing may read it."""
        self._check(w)
        p = self._new("out", w)
        self._pub.append(p.node)
        self._equal.append((p.node, w.node))
        self._outputs.append((p.node, w.node))
        return p

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

    def MAJ(self, a: Wire, b: Wire, c: Wire) -> Wire:
        """1 iff at least two of a, b, c are 1"""
        return self._new("maj", a, b, c)

    def full_add(self, a: Wire, b: Wire, c: Wire):
        """(sum, carry) of a + b + c: a MAJ gate (the carry) and its SUM3 gate, back to back -- 2 wires, 4 rows"""
        k = self.MAJ(a, b, c)
        s = self._new("sum3", a, b, c)
        return s, k

    def gate(self, tt: int, a: Wire, b: Wire) -> Wire:
        """any two-input function: the output on (a, b) is bit (a + 2b) of the truth table tt in [0, 16)"""
        if not isinstance(tt, int) or not 0 <= tt < 16:
            raise CircuitError("gate: the truth table must be an integer in [0, 16)")
        for w in (a, b):
            self._check(w)
        self._nodes.append(("lut", tt, a.node, b.node))
        return Wire(len(self._nodes) - 1)

    def NAND(self, a: Wire, b: Wire) -> Wire:
        return self.gate(TT_NAND, a, b)

    def NOR(self, a: Wire, b: Wire) -> Wire:
        return self.gate(TT_NOR, a, b)

    def XNOR(self, a: Wire, b: Wire) -> Wire:
        return self.gate(TT_XNOR, a, b)

    def ANDN(self, a: Wire, b: Wire) -> Wire:
        """a AND NOT b"""
        return self.gate(TT_ANDN, a, b)

    def ORN(self, a: Wire, b: Wire) -> Wire:
        """a OR NOT b"""
        return self.gate(TT_ORN, a, b)

    def wsum(self, terms):
        """the binary expansion of sum_e 2^shift_e * x_e for terms = [(wire x_e, shift_e), ...], a wire as often as wanted: nbits = bitlength(sum_e
        2^shift_e) output wires, least significant first, and two rows for all of them.  The terms are kept sorted by shift (stable)."""
        terms = list(terms)
        if not terms:
            raise CircuitError("wsum: no terms")
        for w, sh in terms:
            self._check(w)
            if not isinstance(sh, (int, np.integer)) or sh < 0:
                raise CircuitError("wsum: a shift must be a non-negative integer")
        terms.sort(key=lambda t: t[1])
        nbits = sum(1 << int(sh) for _, sh in terms).bit_length()
        if nbits > WSUM_MAX_BITS:
            raise CircuitError(f"wsum: the sum needs {nbits} bits, a gate has at most {WSUM_MAX_BITS}")
        self._nodes.append(("wsum", nbits, tuple((w.node, int(sh)) for w, sh in terms)))
        head = len(self._nodes) - 1
        for i in range(1, nbits):
            self._nodes.append(("wsumbit", i, head))
        return [Wire(head + i) for i in range(nbits)]

    def const(self, value: int) -> Wire:
        """the wire that is always `value` (0 or 1): one shared wire per value and circuit, made on first use"""
        if value not in (0, 1):
            raise CircuitError("const: the value must be 0 or 1")
        if value not in self._const:
            self._nodes.append(("const", int(value)))
            self._const[value] = len(self._nodes) - 1
        return Wire(self._const[value])

    def const_value(self, w: Wire):
        """0 or 1 if w is one of the circuit's constant wires (const), else None"""
        self._check(w)
        node = self._nodes[w.node]
        return node[1] if node[0] == "const" else None

    def assert_same(self, a: Wire, b: Wire):
        """assert that wires a and b carry the same bit: one row, no wire"""
        self._check(a)
        self._check(b)
        if a.node == b.node:
            raise CircuitError("assert_same: a wire is always equal to itself")
        self._equal.append((a.node, b.node))

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
        for group in (self._pub, self._priv, [i for i, n in enumerate(self._nodes) if n[0] not in ("pub", "priv", "out")]):
            for i in group:
                wires[i] = nxt
                nxt += 1
        return wires, nxt - 1

    def compile(self, params) -> Compiled:
        """the constraint rows for an SSP of params.d points and params.m wires; CircuitError if the circuit needs more than m - 1 wires or d - 1 rows"""
        wires, nw = self._layout()
        ngates = nw - len(self._pub) - len(self._priv)
        # one row per gate wire, but two for the nbits wires of a wsum
        nrows = nw + ngates - sum(n[1] - 2 for n in self._nodes if n[0] == "wsum") + len(self._asserts) + len(self._equal)
        if nw > params.m - 1:
            raise CircuitError(f"the circuit needs {nw} wires, the SSP has {params.m - 1} (m - 1)")
        if nrows > params.d - 1:
            raise CircuitError(f"the circuit needs {nrows} rows, the SSP has {params.d - 1} points (d - 1)")
        rows = [[(w, 2), (0, _M1)] for w in range(1, nw + 1)]  # every wire is a bit
        for i, node in enumerate(self._nodes):
            kind, c = node[0], wires[i]
            if kind in ("pub", "priv", "out"):
                continue
            if kind == "const":
                rows.append([(c, 1)] if node[1] else [(c, _M1), (0, 1)])
                continue
            if kind == "lut":
                rows.append(_modrow(*lut2_row(node[1], wires[node[2]], wires[node[3]], c)))
                continue
            if kind == "wsumbit":
                continue
            if kind == "wsum":  # 2X - 1 and 2X + 1, X = sum 2^shift x - sum 2^i o_i
                x2 = [(wires[a], 2 << sh) for a, sh in node[2]] + [(c + k, P - (2 << k)) for k in range(node[1])]
                rows.append(x2 + [(0, _M1)])
                rows.append(x2 + [(0, 1)])
                continue
            a = wires[node[1]]
            if kind == "not":
                rows.append([(a, 1), (c, 1)])
                continue
            if kind in ("maj", "sum3"):
                b, cc = wires[node[2]], wires[node[3]]
                if kind == "maj":
                    rows.append([(a, 2), (b, 2), (cc, 2), (c, P - 4), (0, _M1)])
                else:  # the carry k is the MAJ gate's wire, created just before
                    rows.append([(a, _M1), (b, _M1), (cc, _M1), (wires[i - 1], 2), (c, _M1), (0, 1)])
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
        for a, b in self._equal:
            rows.append([(wires[a], _M1), (wires[b], _M1), (0, 1)])
        assert len(rows) == nrows
        row_ptr = np.zeros(nrows + 1, dtype=np.uint32)
        np.cumsum([len(r) for r in rows], out=row_ptr[1:])
        wire = np.array([w for r in rows for w, _ in r], dtype=np.uint32)
        coef = np.array([x for r in rows for _, x in r], dtype=np.uint32)
        program = np.array([self._record(n, wires) for n in self._nodes if n[0] not in ("pub", "priv", "out")], dtype=np.uint32).reshape(-1, 4)
        asserts = np.array([(wires[node], value) for node, value in self._asserts], dtype=np.uint32).reshape(-1, 2)
        equal = np.array([(wires[a], wires[b]) for a, b in self._equal], dtype=np.uint32).reshape(-1, 2)
        outputs = np.array([(wires[p], wires[w]) for p, w in self._outputs], dtype=np.uint32).reshape(-1, 2)
        terms = np.array([(wires[a], sh) for n in self._nodes if n[0] == "wsum" for a, sh in n[2]], dtype=np.uint32).reshape(-1, 2)
        first = np.cumsum([0] + [len(n[2]) for n in self._nodes if n[0] == "wsum"])  # a head's first_term: the heads' slices follow each other
        heads = np.flatnonzero(program[:, 0] == GATE_WSUM)
        program[heads, 1] = first[:-1]
        gates = np.ascontiguousarray(program[:, :3])
        self._params = params
        return Compiled(rows=(row_ptr, wire, coef), lu=len(self._pub), wires=tuple(wires), nrows=nrows, nwires=nw, gates=gates, asserts=asserts,
                        program=program, equal=equal, outputs=outputs, terms=terms)

    @staticmethod
    def _record(node, wires):
        """(op, a, b, c) of one gate node in SSP wire numbering"""
        kind = node[0]
        if kind == "const":
            return (GATE_CONST1 if node[1] else GATE_CONST0, 0, 0, 0)
        if kind == "lut":
            return (GATE_LUT2(node[1]), wires[node[2]], wires[node[3]], 0)
        if kind == "wsum":  # first_term is filled in by compile
            return (GATE_WSUM, 0, len(node[2]), node[1])
        if kind == "wsumbit":
            return (GATE_WSUM_BIT, node[1], 0, 0)
        if kind in ("maj", "sum3"):
            return (_OPS[kind], wires[node[1]], wires[node[2]], wires[node[3]])
        return (_OPS[kind], wires[node[1]], wires[node[-1]], 0)

    # -- assignments ------------------------------------------------------------------------------------------------------
    def evaluate(self, public_bits, private_bits):
        """the bit on every node (Wire.node order).  public_bits has one entry per public wire, computed outputs included: what stands at an output's
        position is ignored, the node takes the value of the wire it is defined as"""
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
            elif kind == "maj":
                val[i] = int(val[node[1]] + val[node[2]] + val[node[3]] >= 2)
            elif kind == "sum3":
                val[i] = val[node[1]] ^ val[node[2]] ^ val[node[3]]
            elif kind == "lut":
                val[i] = (node[1] >> (val[node[2]] + 2 * val[node[3]])) & 1
            elif kind == "const":
                val[i] = node[1]
            elif kind == "out":
                val[i] = val[node[1]]
            elif kind == "wsum":
                total = sum(val[a] << sh for a, sh in node[2])
                for k in range(node[1]):
                    val[i + k] = (total >> k) & 1
        return val

    def holds(self, public_bits, private_bits) -> bool:
        """every assertion and every equality holds on this input (then the witness of assign satisfies every row)"""
        val = self.evaluate(public_bits, private_bits)
        return all(val[n] == v for n, v in self._asserts) and all(val[a] == val[b] for a, b in self._equal)

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

    def outputs_of(self, witness_bits) -> bytes:
        """the public statement u read back from a witness row (bytes of assign, or a row of Context.circuit_assign): bits [0, lu), LSB first, as
        Context.verify_public takes it -- with computed outputs, the statement the circuit arrived at"""
        lu = len(self._pub)
        row = bytes(bytearray(witness_bits)[: (lu + 7) // 8])
        if len(row) * 8 < lu:
            raise CircuitError(f"outputs_of: the witness row has fewer than {lu} bits")
        out = bytearray(max(1, (lu + 7) // 8))
        out[: len(row)] = row
        if lu & 7:
            out[lu >> 3] &= (1 << (lu & 7)) - 1
        return bytes(out)

    def statement(self, public_bits) -> bytes:
        """the public statement u (bits [0, lu) of the input, LSB first) as Context.verify_public takes it (the bits as given: for a circuit with
        computed outputs read the statement from the witness, outputs_of)"""
        public_bits = list(public_bits)
        if len(public_bits) != len(self._pub):
            raise CircuitError(f"the circuit has {len(self._pub)} public inputs")
        out = bytearray(max(1, (len(public_bits) + 7) // 8))
        for i, x in enumerate(public_bits):
            out[i >> 3] |= (int(x) & 1) << (i & 7)
        return bytes(out)
