"""32-bit words over one circuit.Circuit, and the ChaCha20 block function (RFC 8439) written with them.

A word is a tuple of 32 wires, least significant bit first.  Costs, in gate wires (each also one SSP row besides the wire's bit row):
    add          64   bit 0 a half adder (XOR, AND), bits 1 .. 31 a full adder each (MAJ + SUM3; the last carry is unused)
    xor / and_ / or_ / not_   32
    ch           96   z ^ (x & (y ^ z))
    maj          32   one MAJ per bit
    rotl / rotr   0   rewiring only
    shr           0   the vacated bits are the circuit's shared zero wire (1 wire for the whole circuit)
    const         0   the shared zero and one wires (at most 2 for the whole circuit)
    assert_u32        32 value assertions (rows, no wires)
    assert_same_u32   32 equalities (rows, no wires)

    w = Words()
    x, y = w.public(), w.private()
    w.assert_u32(w.add(w.rotl(x, 7), y), 0xDEADBEEF)
    cc = w.c.compile(mf.DEFAULT)
    bits = np.concatenate([pack([x_value]), pack([y_value])], axis=1)   # public words, then private words, as Context.circuit_assign takes them

The ChaCha20 block statement (ChaCha20Block) takes 32 642 wires and 64 900 rows: it fits d = 2^16 (m = 43 690) and the LDS kernel.
"""
from __future__ import annotations

import numpy as np

from .circuit import Circuit, CircuitError

MASK = 0xFFFFFFFF


def pack(values):
    """input bits of words: uint8 [len(values) * 32], word i's bit j at 32 i + j (Circuit.evaluate / Context.circuit_assign order); values may also be a
    2-D array [nb, nwords], giving [nb, nwords * 32]"""
    v = np.asarray(values, dtype=np.uint64)
    bits = ((v[..., None] >> np.arange(32, dtype=np.uint64)) & 1).astype(np.uint8)
    return bits.reshape(v.shape[:-1] + (v.shape[-1] * 32,)) if v.ndim else bits


def unpack(bits):
    """the words of 32 bits each, LSB first: a list of ints from a 1-D array, else an array [..., nwords] of uint32"""
    b = np.asarray(bits, dtype=np.uint64)
    if b.shape[-1] % 32:
        raise CircuitError("unpack: the bit count must be a multiple of 32")
    w = (b.reshape(b.shape[:-1] + (b.shape[-1] // 32, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    return [int(x) for x in w] if w.ndim == 1 else w


class Words:
    """32-bit word operations on one Circuit (self.c)"""

    def __init__(self, circuit: Circuit | None = None):
        self.c = circuit if circuit is not None else Circuit()

    # -- inputs and constants -------------------------------------------------------------------------------------------
    def public(self, count=None):
        """one public input word, or a list of `count` of them"""
        if count is not None:
            return [self.public() for _ in range(count)]
        return tuple(self.c.public(32))

    def private(self, count=None):
        """one private input word, or a list of `count` of them"""
        if count is not None:
            return [self.private() for _ in range(count)]
        return tuple(self.c.private(32))

    def const(self, value: int):
        """the word `value`: the circuit's shared constant wires, no new wire beyond them"""
        return tuple(self.c.const((value >> i) & 1) for i in range(32))

    # -- arithmetic and logic -------------------------------------------------------------------------------------------
    def add(self, x, y):
        """x + y mod 2^32: 64 wires"""
        out = [self.c.XOR(x[0], y[0])]
        carry = self.c.AND(x[0], y[0])
        for i in range(1, 32):
            s, carry = self.c.full_add(x[i], y[i], carry)
            out.append(s)
        return tuple(out)

    def xor(self, x, y):
        return tuple(self.c.XOR(a, b) for a, b in zip(x, y))

    def and_(self, x, y):
        return tuple(self.c.AND(a, b) for a, b in zip(x, y))

    def or_(self, x, y):
        return tuple(self.c.OR(a, b) for a, b in zip(x, y))

    def not_(self, x):
        return tuple(self.c.NOT(a) for a in x)

    def ch(self, x, y, z):
        """bitwise x ? y : z (SHA-2's Ch)"""
        return self.xor(z, self.and_(x, self.xor(y, z)))

    def maj(self, x, y, z):
        """bitwise majority (SHA-2's Maj)"""
        return tuple(self.c.MAJ(a, b, d) for a, b, d in zip(x, y, z))

    # -- rewiring -------------------------------------------------------------------------------------------------------
    @staticmethod
    def rotl(x, n: int):
        n %= 32
        return tuple(x[(i - n) % 32] for i in range(32))

    @staticmethod
    def rotr(x, n: int):
        return Words.rotl(x, -n)

    def shr(self, x, n: int):
        """x >> n for n in [0, 32]: the top n bits are the shared zero wire"""
        if not 0 <= n <= 32:
            raise CircuitError("shr: the shift must be in [0, 32]")
        return tuple(x[i + n] if i + n < 32 else self.c.const(0) for i in range(32))

    # -- assertions -----------------------------------------------------------------------------------------------------
    def assert_u32(self, x, value: int):
        """x = value: 32 value assertions"""
        for i in range(32):
            self.c.assert_equal(x[i], (value >> i) & 1)

    def assert_same_u32(self, x, y):
        """x = y: 32 equalities"""
        for a, b in zip(x, y):
            self.c.assert_same(a, b)


# ---------------------------------------------------------------------------------------------------------------------- ChaCha20 (RFC 8439)
CHACHA_CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"


def quarter_round(w: Words, a, b, c, d):
    """RFC 8439 2.1 on four words: 4 adds, 4 xors, 4 rotations"""
    a = w.add(a, b); d = w.rotl(w.xor(d, a), 16)
    c = w.add(c, d); b = w.rotl(w.xor(b, c), 12)
    a = w.add(a, b); d = w.rotl(w.xor(d, a), 8)
    c = w.add(c, d); b = w.rotl(w.xor(b, c), 7)
    return a, b, c, d


def double_round(w: Words, x):
    """a column round and a diagonal round (RFC 8439 2.3) on the 16-word state x: 32 adds, 32 xors"""
    x = list(x)
    for i in (0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14):
        x[i[0]], x[i[1]], x[i[2]], x[i[3]] = quarter_round(w, *(x[j] for j in i))
    return x


def chacha20_block(w: Words, key, counter, nonce):
    """the 16 output words of the ChaCha20 block function (RFC 8439 2.3): key = 8 words, counter = 1 word, nonce = 3 words -- 336 adds, 320 xors"""
    state = [w.const(v) for v in CHACHA_CONSTANTS] + list(key) + [counter] + list(nonce)
    x = state
    for _ in range(10):
        x = double_round(w, x)
    return [w.add(a, b) for a, b in zip(x, state)]


def le_words(data: bytes):
    """little-endian 32-bit words of a byte string (RFC 8439's serialisation)"""
    if len(data) % 4:
        raise CircuitError("le_words: the length must be a multiple of 4")
    return [int.from_bytes(data[i: i + 4], "little") for i in range(0, len(data), 4)]


class ChaCha20Block:
    """The statement "I know a 256-bit key whose ChaCha20 block, at this public counter and nonce, is this public 64-byte block".

    Public inputs (lu = 640): the counter word, the 3 nonce words, the 16 block words; private: the 8 key words.  The computed block is tied to the
    public one by 512 equalities.  32 642 wires (896 inputs, 2 constants, 336 adds x 64, 320 xors x 32) and 64 900 rows."""

    def __init__(self):
        self.w = w = Words()
        self.counter = w.public()
        self.nonce = w.public(3)
        self.block = w.public(16)
        self.key = w.private(8)
        self.out = chacha20_block(w, self.key, self.counter, self.nonce)
        for o, b in zip(self.out, self.block):
            w.assert_same_u32(o, b)

    @property
    def circuit(self) -> Circuit:
        return self.w.c

    @staticmethod
    def public_bits(counter: int, nonce: bytes, block: bytes):
        """the 640 public bits: counter, nonce (12 bytes), block (64 bytes)"""
        if len(nonce) != 12 or len(block) != 64:
            raise CircuitError("ChaCha20Block: the nonce is 12 bytes and the block 64")
        return pack([counter & MASK] + le_words(nonce) + le_words(block))

    @staticmethod
    def private_bits(key: bytes):
        """the 256 private bits of a 32-byte key"""
        if len(key) != 32:
            raise CircuitError("ChaCha20Block: the key is 32 bytes")
        return pack(le_words(key))

    def bits(self, key: bytes, counter: int, nonce: bytes, block: bytes):
        """one statement's 896 input bits, public then private (a row of Context.circuit_assign's input)"""
        return np.concatenate([self.public_bits(counter, nonce, block), self.private_bits(key)])
