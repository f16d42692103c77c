"""Helpers of the extended-gate tests: random circuits over every gate, a numpy restatement of the bitsliced evaluation of mfh_circuit_create_ex
programs, the validation rules of mfh_circuit_create_ex restated in Python, and ChaCha20 on Python integers (RFC 8439)."""
import numpy as np

from c_lwe_snarks_amd import circuit as C

MAX_WIRES = 32767  # MFH_CIRCUIT_MAX_WIRES
M32 = 0xFFFFFFFF


def random_ex_circuit(rng, npub, npriv, ngates, nasserts=0, nequal=0):
    """inputs, then ngates random gates of every kind on earlier wires (full adders count two), then assertions and equalities on random wires"""
    c = C.Circuit()
    ws = c.public(npub) + c.private(npriv)
    kinds = ("XOR", "AND", "OR", "NOT", "MAJ", "FA", "LUT", "CONST", "NAND", "NOR", "XNOR", "ANDN", "ORN")
    while len(ws) < npub + npriv + ngates:
        kind = kinds[int(rng.integers(0, len(kinds)))]
        a, b, d = (ws[int(rng.integers(0, len(ws)))] for _ in range(3))
        if kind == "NOT":
            ws.append(c.NOT(a))
        elif kind == "MAJ":
            ws.append(c.MAJ(a, b, d))
        elif kind == "FA":
            if len(ws) + 2 > npub + npriv + ngates:
                continue
            s, k = c.full_add(a, b, d)
            ws += [k, s]
        elif kind == "LUT":
            ws.append(c.gate(int(rng.integers(0, 16)), a, b))
        elif kind == "CONST":
            ws.append(c.const(int(rng.integers(0, 2))))  # shared: a second use makes no new wire
        else:
            ws.append(getattr(c, kind)(a, b))
    for _ in range(nasserts):
        c.assert_equal(ws[int(rng.integers(0, len(ws)))], int(rng.integers(0, 2)))
    for _ in range(nequal):
        a, b = rng.choice(len(ws), size=2, replace=False)
        c.assert_same(ws[int(a)], ws[int(b)])
    return c


def gate_word(op, x, y, z):
    """the bitsliced word of one gate (k_circuit_eval_ex)"""
    if op >= 16:
        t = [np.uint32(M32 if (op >> i) & 1 else 0) for i in range(4)]  # 0 - bit i
        return (~x & ~y & t[0]) | (x & ~y & t[1]) | (~x & y & t[2]) | (x & y & t[3])
    return {
        C.GATE_XOR: lambda: x ^ y, C.GATE_AND: lambda: x & y, C.GATE_OR: lambda: x | y, C.GATE_NOT: lambda: ~x,
        C.GATE_MAJ: lambda: (x & y) | (z & (x | y)), C.GATE_SUM3: lambda: x ^ y ^ z,
        C.GATE_CONST0: lambda: np.uint32(0), C.GATE_CONST1: lambda: np.uint32(M32),
    }[op]()


def bitsliced_ex(cc, bits, m):
    """witness bytes [nb, (m + 7) // 8] and holds [nb] from cc.program / asserts / equal alone, 32 statements per word"""
    nb, nin = bits.shape
    ng = len(cc.program)
    nw = nin + ng
    out_bits = np.zeros((nb, nw), dtype=np.uint8)
    holds = np.zeros(nb, dtype=bool)
    for s0 in range(0, nb, 32):
        blk = bits[s0: s0 + 32] & 1
        n = len(blk)
        weights = (np.uint32(1) << np.arange(n, dtype=np.uint32))[:, None]
        st = np.zeros(nw + 1, dtype=np.uint32)
        st[1: nin + 1] = (blk.astype(np.uint32) * weights).sum(axis=0, dtype=np.uint32)
        for g, (op, a, b, c) in enumerate(cc.program.tolist()):
            st[nin + 1 + g] = gate_word(op, st[a], st[b], st[c])
        ok = np.uint32(M32)
        for w, v in cc.asserts:
            ok &= st[w] if v else ~st[w]
        for a, b in cc.equal:
            ok &= ~(st[a] ^ st[b])
        holds[s0: s0 + n] = [(int(ok) >> j) & 1 for j in range(n)]
        out_bits[s0: s0 + n] = ((st[1:][None, :] >> np.arange(n, dtype=np.uint32)[:, None]) & 1).astype(np.uint8)
    packed = np.packbits(out_bits, axis=1, bitorder="little")
    wit = np.zeros((nb, (m + 7) // 8), dtype=np.uint8)
    wit[:, : packed.shape[1]] = packed
    return wit, holds


def validate_ex(nin, program, asserts, equal, m, flags=0):
    """the mfh_last_error text (after "mfh_circuit_create_ex: ") mfh_circuit_create_ex gives this program, or None if it accepts it"""
    program = np.asarray(program, dtype=np.int64).reshape(-1, 4).tolist()
    asserts = np.asarray(asserts, dtype=np.int64).reshape(-1, 2).tolist()
    equal = np.asarray(equal, dtype=np.int64).reshape(-1, 2).tolist()
    if flags & ~1:
        return "unknown flag bits"
    nw = nin + len(program)
    if nw > m - 1:
        return "nin + ngates > m - 1"
    if not flags & 1 and nw > MAX_WIRES:
        return "nin + ngates > MFH_CIRCUIT_MAX_WIRES (the wire state must fit 128 KiB of LDS)"
    if nw >= 1 << 24:
        return "nin + ngates >= 2^24 (the records' 24-bit wire field)"
    for g, (op, a, b, c) in enumerate(program):
        o = nin + 1 + g
        if 8 <= op < 16 or op >= 32:
            return "unknown gate op"
        if op in (C.GATE_CONST0, C.GATE_CONST1):
            if a or b or c:
                return "a CONST gate with an operand other than 0"
            continue
        three = op in (C.GATE_MAJ, C.GATE_SUM3)
        if not (1 <= a < o and 1 <= b < o) or (three and not 1 <= c < o):
            return "a gate operand is 0 or not below the gate's output wire"
        if not three and c:
            return "a one- or two-input gate with a third operand c != 0"
        if op == C.GATE_NOT and b != a:
            return "a NOT gate with b != a"
        if op == C.GATE_SUM3:
            if g == 0 or program[g - 1][0] != C.GATE_MAJ:
                return "a SUM3 gate not directly after a MAJ gate"
            if program[g - 1][1:] != [a, b, c]:
                return "a SUM3 gate whose operands differ from its MAJ's"
    for w, v in asserts:
        if not 1 <= w <= nw:
            return "an assertion on wire 0 or above nin + ngates"
        if v > 1:
            return "an assertion value other than 0 / 1"
    for a, b in equal:
        if not (1 <= a <= nw and 1 <= b <= nw):
            return "an equality on wire 0 or above nin + ngates"
        if a == b:
            return "an equality of a wire with itself"
    return None


# one case per rule: name -> (nin, program, asserts, equal, m, flags, text); nin = 4, m = 64 unless stated
_OK = [(0, 1, 2, 0), (4, 1, 2, 5), (5, 1, 2, 5)]  # wires 5, 6, 7


def einval_cases():
    return {
        "op 8": (4, [(8, 1, 2, 0)], [], [], 64, 0, "unknown gate op"),
        "op 15": (4, [(15, 1, 2, 0)], [], [], 64, 0, "unknown gate op"),
        "op 32": (4, [(32, 1, 2, 0)], [], [], 64, 0, "unknown gate op"),
        "unknown flag": (4, _OK, [], [], 64, 2, "unknown flag bits"),
        "operand 0": (4, [(1, 0, 2, 0)], [], [], 64, 0, "a gate operand is 0 or not below the gate's output wire"),
        "LUT2 operand = own output": (4, [(C.GATE_LUT2(7), 1, 5, 0)], [], [], 64, 0, "a gate operand is 0 or not below the gate's output wire"),
        "MAJ c = 0": (4, [(4, 1, 2, 0)], [], [], 64, 0, "a gate operand is 0 or not below the gate's output wire"),
        "MAJ c above": (4, [(4, 1, 2, 6)], [], [], 64, 0, "a gate operand is 0 or not below the gate's output wire"),
        "XOR with c": (4, [(0, 1, 2, 3)], [], [], 64, 0, "a one- or two-input gate with a third operand c != 0"),
        "LUT2 with c": (4, [(C.GATE_LUT2(9), 1, 2, 3)], [], [], 64, 0, "a one- or two-input gate with a third operand c != 0"),
        "NOT with c": (4, [(3, 1, 1, 2)], [], [], 64, 0, "a one- or two-input gate with a third operand c != 0"),
        "NOT b != a": (4, [(3, 1, 2, 0)], [], [], 64, 0, "a NOT gate with b != a"),
        "CONST with operand": (4, [(6, 1, 0, 0)], [], [], 64, 0, "a CONST gate with an operand other than 0"),
        "CONST1 with c": (4, [(7, 0, 0, 1)], [], [], 64, 0, "a CONST gate with an operand other than 0"),
        "SUM3 first": (4, [(5, 1, 2, 3)], [], [], 64, 0, "a SUM3 gate not directly after a MAJ gate"),
        "SUM3 after XOR": (4, [(0, 1, 2, 0), (5, 1, 2, 3)], [], [], 64, 0, "a SUM3 gate not directly after a MAJ gate"),
        "SUM3 after SUM3": (4, [(4, 1, 2, 3), (5, 1, 2, 3), (5, 1, 2, 3)], [], [], 64, 0, "a SUM3 gate not directly after a MAJ gate"),
        "SUM3 other operands": (4, [(4, 1, 2, 3), (5, 1, 2, 4)], [], [], 64, 0, "a SUM3 gate whose operands differ from its MAJ's"),
        "SUM3 permuted operands": (4, [(4, 1, 2, 3), (5, 2, 1, 3)], [], [], 64, 0, "a SUM3 gate whose operands differ from its MAJ's"),
        "assert on wire 0": (4, _OK, [(0, 1)], [], 64, 0, "an assertion on wire 0 or above nin + ngates"),
        "assert value 2": (4, _OK, [(5, 2)], [], 64, 0, "an assertion value other than 0 / 1"),
        "equality on wire 0": (4, _OK, [], [(0, 5)], 64, 0, "an equality on wire 0 or above nin + ngates"),
        "equality above nin + ngates": (4, _OK, [], [(5, 8)], 64, 0, "an equality on wire 0 or above nin + ngates"),
        "equality a = b": (4, _OK, [], [(6, 6)], 64, 0, "an equality of a wire with itself"),
        "nin + ngates > m - 1": (61, _OK, [], [], 64, 0, "nin + ngates > m - 1"),
        "nin + ngates > m - 1, global": (61, _OK, [], [], 64, 1, "nin + ngates > m - 1"),
        "LDS limit": (MAX_WIRES - 2, _OK, [], [], 40000, 0, "nin + ngates > MFH_CIRCUIT_MAX_WIRES (the wire state must fit 128 KiB of LDS)"),
    }


# ---------------------------------------------------------------------------------------------------------------------- ChaCha20 on integers
def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def quarter_round_int(a, b, c, d):
    a = (a + b) & M32; d = _rotl(d ^ a, 16)
    c = (c + d) & M32; b = _rotl(b ^ c, 12)
    a = (a + b) & M32; d = _rotl(d ^ a, 8)
    c = (c + d) & M32; b = _rotl(b ^ c, 7)
    return a, b, c, d


def double_round_int(x):
    x = list(x)
    for i in (0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14):
        x[i[0]], x[i[1]], x[i[2]], x[i[3]] = quarter_round_int(*(x[j] for j in i))
    return x


def chacha20_block_int(key: bytes, counter: int, nonce: bytes) -> bytes:
    kw = [int.from_bytes(key[i: i + 4], "little") for i in range(0, 32, 4)]
    nw = [int.from_bytes(nonce[i: i + 4], "little") for i in range(0, 12, 4)]
    state = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + kw + [counter & M32] + nw
    x = state
    for _ in range(10):
        x = double_round_int(x)
    return b"".join(((a + b) & M32).to_bytes(4, "little") for a, b in zip(x, state))
